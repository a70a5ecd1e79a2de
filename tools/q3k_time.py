#!/usr/bin/env python3
"""Q3_K against Q6_K on the device: the product per call (a hipGraph of calls over rotating weight copies, median over replays, the two
types alternated), the upload of a 4096 x 11008 weight (host bytes -> resident form, and the converter alone from device bytes) and the
device quantizer on 11008 rows of 4096.  Q3_K lives in Q6_K's resident form, so the two products are expected to take the same time.
usage: python tools/q3k_time.py [M:K:N ...]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

Q3_K, Q6_K = 111, 114
RESIDENT_B_PER_WEIGHT = 1.0 + 8.0 / 32                # the int8 planes plus the two f32 scales per 32-element k-block


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
    copies = max(2, min(16, -(-int(400e6) // int(M * K * RESIDENT_B_PER_WEIGHT))))   # > 256 MB of distinct weights: no Infinity Cache hits
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


def compare(M, K, N, rounds=5):
    gs = {t: product_graph(t, M, K, N) for t in (Q3_K, Q6_K)}
    per = {Q3_K: [], Q6_K: []}
    for _ in range(rounds):                            # alternate the two types: the box's drift hits both alike
        for t in (Q3_K, Q6_K):
            med, _, _ = _events(gs[t]["graph"].replay, 10)
            per[t].append(med / gs[t]["nodes"] * 1e3)
    q3, q6 = float(np.median(per[Q3_K])), float(np.median(per[Q6_K]))
    spread = max(max(v) - min(v) for v in per.values())
    print(f"mul_mat {M}x{K}x{N}: Q3_K {q3:8.2f} us  Q6_K {q6:8.2f} us  Q3_K/Q6_K {q3 / q6:5.3f}  (spread of round medians {spread:.2f} us)", flush=True)
    torch.cuda.synchronize()
    for g in gs.values():                              # the graphs go first, then what they point to
        del g["graph"]
    for g in gs.values():
        for w in g["ws"]:
            w.free()


def upload(M=4096, K=11008):
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 256, size=(M, K // 256 * 110), dtype=np.uint8)
    rows.reshape(-1, 110)[:, 108:110] = np.array([0.001], np.float16).view(np.uint8)   # a small finite d
    dev_rows = torch.from_numpy(rows).cuda()
    for label, make in (("from host", lambda: device.Weight.from_host(Q3_K, rows, K)),
                        ("from device", lambda: device.Weight.from_device(Q3_K, dev_rows, K))):
        make().free()
        ts = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = make()                                 # (the upload synchronises its stream before it returns)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            w.free()
        print(f"Q3_K upload {M}x{K} {label}: {np.median(ts):7.3f} ms median of 7 (min {min(ts):.3f})", flush=True)


def quantizer(nrows=11008, K=4096):
    x = torch.randn((nrows, K), device="cuda")
    device.quantize_rows(Q3_K, x)
    med, lo, hi = _events(lambda: device.quantize_rows(Q3_K, x), 20)
    print(f"Q3_K device quantizer {nrows} rows of {K}: {med * 1e3:8.1f} us median of 20 (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)


if __name__ == "__main__":
    device.init(0)
    shapes = sys.argv[1:] or ["4096:4096:1", "4096:11008:1", "4096:11008:16", "4096:11008:512"]
    for s in shapes:
        compare(*[int(v) for v in s.split(":")])
    upload()
    quantizer()
