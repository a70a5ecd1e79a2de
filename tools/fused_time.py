#!/usr/bin/env python3
"""Q4_0: the fused route of mul_mat (src1 quantized inside the K3m launch) against INIT + COMPUTE, alternating blocks of steps in ONE process on
real quantised data (developer tool, GPU box; GGML_HIP_LIB selects a variant build).
usage: python tools/fused_time.py [M:K:N ...]   (default 4096:4096:4096)"""
import os
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402
from ggmlsharp_amd._lib import lib  # noqa: E402


def block(fn, n):
    s = torch.cuda.Event(enable_timing=True)
    e = torch.cuda.Event(enable_timing=True)
    s.record()
    for _ in range(n):
        fn()
    e.record()
    e.synchronize()
    return s.elapsed_time(e) / n * 1e3


def run(M, K, N, blocks=6, steps=500, preheat_s=3.0):
    g = torch.Generator(device="cuda")
    g.manual_seed(7)
    W = device.Weight.from_device(2, device.quantize_rows(2, torch.randn((M, K), generator=g, device="cuda")), K)
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    out = torch.empty((N, M), device="cuda")
    work = device.alloc_work(2, K, N)
    print(f"{os.environ.get('GGML_HIP_LIB', 'product')[-40:]} M {M} K {K} N {N}: fused route {lib().ggml_hip_mul_mat_init_fused(W.handle, N)}", flush=True)

    def fused():
        device.mul_mat(W, x, out=out, work=work)

    def two():
        device.mul_mat_init(W, x, work)
        device.mul_mat_compute(W, N, out, work)
    t0 = time.time()
    while time.time() - t0 < preheat_s:
        block(two, 200)
    res = {"two": [], "mul_mat": []}
    for _ in range(blocks):
        res["two"].append(block(two, steps))
        res["mul_mat"].append(block(fused, steps))
    for k, v in res.items():
        print(f"  {k:8s} us/step:", " ".join(f"{t:7.2f}" for t in v), " median %.2f" % sorted(v)[len(v) // 2], flush=True)
    W.free()


if __name__ == "__main__":
    device.init(0)
    for a in sys.argv[1:] or ["4096:4096:4096"]:
        run(*(int(v) for v in a.split(":")))
