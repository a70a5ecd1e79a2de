#!/usr/bin/env python3
"""Q2_K against Q6_K on the device, GPU-side (a hipGraph of calls over rotating weight copies, median over replays, the two types alternated):
  - the one-call product (Q6_K's plan, with its fused mat-vec at N <= 4; Q2_K's: the two-step forms and the min pass behind them)
  - the min pass alone (the test hook ggml_hip_debug_q2k_min_pass_dev behind one INIT, replayed over the same rotating weights)
and the Q2_K device quantizer on 11008 rows of 4096.
usage: python tools/q2k_time.py [M:K:N ...]"""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import _lib, device  # noqa: E402

Q2_K, Q6_K = 110, 114
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
    return float(np.median(ts))


def product_graph(t, M, K, N, pass_only):
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

    def call(w):
        if pass_only:                                  # (dst -= T in place, again and again: finite values, the same work)
            _lib.check(_lib.lib().ggml_hip_debug_q2k_min_pass_dev(w.handle, N, C.c_void_p(out.data_ptr()), M, C.c_void_p(work.data_ptr()),
                                                                  work.numel(), 0, C.c_void_p(torch.cuda.current_stream().cuda_stream)),
                       "min pass")
        else:
            device.mul_mat(w, x, out=out, work=work)
    if pass_only:
        out.zero_()
        device.mul_mat_init(ws[0], x, work)            # (one image serves every copy: the same K and N)
    for w in ws:
        call(w)
    torch.cuda.synchronize()
    nodes = copies * max(1, -(-32 // copies))
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        for i in range(nodes):
            call(ws[i % copies])
    graph.replay()
    torch.cuda.synchronize()
    # the graph holds raw pointers: x, out and work must outlive it, and so must the weights
    return {"graph": graph, "nodes": nodes, "ws": ws, "keep": (x, out, work)}


def compare(M, K, N, rounds=5):
    gs = {"Q2_K": product_graph(Q2_K, M, K, N, False), "Q6_K": product_graph(Q6_K, M, K, N, False),
          "pass": product_graph(Q2_K, M, K, N, True)}
    per = {k: [] for k in gs}
    for _ in range(rounds):                            # alternate: the box's drift hits all three alike
        for k, g in gs.items():
            per[k].append(_events(g["graph"].replay, 10) / g["nodes"] * 1e3)
    med = {k: float(np.median(v)) for k, v in per.items()}
    spread = max(max(v) - min(v) for v in per.values())
    print(f"mul_mat {M}x{K}x{N}: Q2_K {med['Q2_K']:8.2f} us  Q6_K {med['Q6_K']:8.2f} us  Q2_K/Q6_K {med['Q2_K'] / med['Q6_K']:5.3f}  "
          f"the min pass alone {med['pass']:7.2f} us  (spread of round medians {spread:.2f} us)", flush=True)
    torch.cuda.synchronize()
    for g in gs.values():                              # the graphs go first, then what they point to
        del g["graph"]
    for g in gs.values():
        for w in g["ws"]:
            w.free()


def quantizer(nrows=11008, K=4096):
    x = torch.randn((nrows, K), device="cuda")
    device.quantize_rows(Q2_K, x)
    med = _events(lambda: device.quantize_rows(Q2_K, x), 20)
    print(f"Q2_K device quantizer {nrows} rows of {K}: {med * 1e3:8.1f} us median of 20", flush=True)


if __name__ == "__main__":
    device.init(0)
    shapes = sys.argv[1:] or ["4096:4096:1", "4096:11008:1", "4096:11008:16", "4096:11008:512"]
    for s in shapes:
        compare(*[int(v) for v in s.split(":")])
    quantizer()
