#!/usr/bin/env python3
"""IQ4_NL against Q8_0 and IQ4_XS against Q6_K on the device: the product per call (a hipGraph of calls over rotating weight copies, median
over replays, the two types of a pair alternated), the upload of a 4096 x 11008 weight (host bytes -> resident form, and the converter alone
from device bytes) and the device quantizer on 11008 rows of 4096, each beside its twin's.  IQ4_NL is a plain Q8_0 weight once resident and
IQ4_XS lives in Q6_K's resident form, so each pair's products are expected to take the same time.
usage: python tools/iq4_time.py [M:K:N ...]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

IQ4_NL, Q8_0, IQ4_XS, Q6_K = 120, 8, 123, 114
PAIRS = ((IQ4_NL, Q8_0), (IQ4_XS, Q6_K))
NAME = {IQ4_NL: "IQ4_NL", Q8_0: "Q8_0", IQ4_XS: "IQ4_XS", Q6_K: "Q6_K"}
RESIDENT_B_PER_WEIGHT = {IQ4_NL: 1.25, Q8_0: 1.25, IQ4_XS: 1.625, Q6_K: 1.625}   # resident bytes per weight (INTEGRATION.md's table)


def _events(fn, reps):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(np.min(ts)), float(np.max(ts))


def product_graph(t, M, K, N):
    copies = max(2, min(16, -(-int(400e6) // int(M * K * RESIDENT_B_PER_WEIGHT[t]))))   # > 256 MB of distinct weights: no Infinity Cache hits
    g = torch.Generator(device="cuda")
    g.manual_seed(M + K + N)
    ws = []
    for _ in range(copies):
        w = torch.randn((M, K), generator=g, device="cuda")
        ws.append(device.Weight.from_device(t, device.quantize_rows(t, w), K))
        del w
    x = torch.randn((N, K), generator=g, device="cuda")
    out = torch.empty((N, M), device="cuda")
    work = device.alloc_work(t, K, N)
    for w in ws:
        device.mul_mat(w, x, out=out, work=work)
    torch.cuda.synchronize()
    nodes = copies * max(1, -(-32 // copies))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(nodes):
            device.mul_mat(ws[i % copies], x, out=out, work=work)
    graph.replay()
    torch.cuda.synchronize()
    # the graph holds raw pointers: x, out and work must outlive it (the next capture empties torch's cache), and so must the weights
    return {"graph": graph, "nodes": nodes, "ws": ws, "keep": (x, out, work)}


def compare(pair, M, K, N, rounds=5):
    a, b = pair
    gs = {t: product_graph(t, M, K, N) for t in pair}
    per = {a: [], b: []}
    for _ in range(rounds):                            # alternate the two types: the box's drift hits both alike
        for t in pair:
            med, _, _ = _events(gs[t]["graph"].replay, 10)
            per[t].append(med / gs[t]["nodes"] * 1e3)
    ta, tb = float(np.median(per[a])), float(np.median(per[b]))
    spread = max(max(v) - min(v) for v in per.values())
    print(f"mul_mat {M}x{K}x{N}: {NAME[a]} {ta:8.2f} us  {NAME[b]} {tb:8.2f} us  {NAME[a]}/{NAME[b]} {ta / tb:5.3f}  "
          f"(spread of round medians {spread:.2f} us)", flush=True)
    torch.cuda.synchronize()
    for g in gs.values():                              # the graphs go first, then what they point to
        del g["graph"]
    for g in gs.values():
        for w in g["ws"]:
            w.free()


def upload(t, M=4096, K=11008):
    x = torch.randn((M, K), device="cuda")
    dev_rows = device.quantize_rows(t, x)
    rows = dev_rows.cpu().numpy()
    for label, make in (("from host", lambda: device.Weight.from_host(t, rows, K)),
                        ("from device", lambda: device.Weight.from_device(t, dev_rows, K))):
        make().free()
        ts = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = make()                                 # (the upload synchronises its stream before it returns)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            w.free()
        print(f"{NAME[t]} upload {M}x{K} {label}: {np.median(ts):7.3f} ms median of 7 (min {min(ts):.3f})", flush=True)


def quantizer(t, nrows=11008, K=4096):
    x = torch.randn((nrows, K), device="cuda")
    device.quantize_rows(t, x)
    med, lo, hi = _events(lambda: device.quantize_rows(t, x), 20)
    print(f"{NAME[t]} device quantizer {nrows} rows of {K}: {med * 1e3:8.1f} us median of 20 (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)


if __name__ == "__main__":
    device.init(0)
    shapes = sys.argv[1:] or ["4096:4096:1", "4096:11008:1", "4096:11008:16", "4096:11008:512"]
    for pair in PAIRS:
        for s in shapes:
            compare(pair, *[int(v) for v in s.split(":")])
    for pair in PAIRS:
        for t in pair:
            upload(t)
    for pair in PAIRS:
        for t in pair:
            quantizer(t)
