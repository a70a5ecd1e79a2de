#!/usr/bin/env python3
"""BF16 against F16 on the device: the product per call (a hipGraph of calls over rotating weight copies, median over replays, the two
types alternated), the upload of a 4096 x 11008 BF16 weight (host bytes -> resident form, and from device bytes) and the device row
conversion f32 -> bf16 on 11008 rows of 4096.  BF16 has F16's resident bytes, plan and kernel forms (bf16 MFMAs at the f16 rate), so the
two products are expected to take the same time.
usage: python tools/bf16_time.py [M:K:N ...]"""
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

BF16, F16 = 130, 1
RESIDENT_B_PER_WEIGHT = 4.0                            # the row-major 16-bit copy and the k-panels


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


def _weight(t, w, K):
    return device.Weight.from_device(BF16, device.quantize_rows(BF16, w), K) if t == BF16 else device.Weight.from_device(F16, w.half(), K)


def product_graph(t, M, K, N):
    copies = max(2, min(16, -(-int(400e6) // int(M * K * RESIDENT_B_PER_WEIGHT))))   # > 256 MB of distinct weights: no Infinity Cache hits
    g = torch.Generator(device="cuda")
    g.manual_seed(M + K + N)
    ws = []
    for _ in range(copies):
        w = torch.randn((M, K), generator=g, device="cuda")
        ws.append(_weight(t, w, K))
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
    gs = {t: product_graph(t, M, K, N) for t in (BF16, F16)}
    per = {BF16: [], F16: []}
    for _ in range(rounds):                            # alternate the two types: the box's drift hits both alike
        for t in (BF16, F16):
            med, _, _ = _events(gs[t]["graph"].replay, 10)
            per[t].append(med / gs[t]["nodes"] * 1e3)
    b, h = float(np.median(per[BF16])), float(np.median(per[F16]))
    spread = max(max(v) - min(v) for v in per.values())
    print(f"mul_mat {M}x{K}x{N}: BF16 {b:8.2f} us  F16 {h:8.2f} us  BF16/F16 {b / h:5.3f}  (spread of round medians {spread:.2f} us)", flush=True)
    torch.cuda.synchronize()
    for g in gs.values():                              # the graphs go first, then what they point to
        del g["graph"]
    for g in gs.values():
        for w in g["ws"]:
            w.free()


def upload(M=4096, K=11008):
    rng = np.random.default_rng(1)
    rows = rng.integers(0, 65536, size=(M, K), dtype=np.uint64).astype(np.uint16)
    dev_rows = torch.from_numpy(rows.view(np.int16)).cuda()
    for label, make in (("from host", lambda: device.Weight.from_host(BF16, rows, K)),
                        ("from device", lambda: device.Weight.from_device(BF16, dev_rows, K))):
        make().free()
        ts = []
        for _ in range(7):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            w = make()                                 # (the upload synchronises its stream before it returns)
            torch.cuda.synchronize()
            ts.append((time.perf_counter() - t0) * 1e3)
            w.free()
        print(f"BF16 upload {M}x{K} {label}: {np.median(ts):7.3f} ms median of 7 (min {min(ts):.3f})", flush=True)


def conversion(nrows=11008, K=4096):
    x = torch.randn((nrows, K), device="cuda")
    y = device.quantize_rows(BF16, x)
    med, lo, hi = _events(lambda: device.quantize_rows(BF16, x), 20)
    print(f"BF16 row conversion f32 -> bf16, {nrows} rows of {K}: {med * 1e3:8.1f} us median of 20 (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)
    med, lo, hi = _events(lambda: device.dequantize_rows(BF16, y.view(torch.uint8).reshape(-1), K), 20)
    print(f"BF16 row conversion bf16 -> f32, {nrows} rows of {K}: {med * 1e3:8.1f} us median of 20 (min {lo * 1e3:.1f}, max {hi * 1e3:.1f})", flush=True)


if __name__ == "__main__":
    device.init(0)
    shapes = sys.argv[1:] or ["4096:4096:1", "4096:4096:4", "4096:4096:16", "4096:4096:128", "4096:4096:512",
                              "4096:11008:1", "4096:11008:16", "4096:11008:512", "4096:4096:4096"]
    for s in shapes:
        compare(*[int(v) for v in s.split(":")])
    upload()
    conversion()
