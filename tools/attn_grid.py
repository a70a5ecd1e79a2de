#!/usr/bin/env python3
"""The attention grid (csrc/attn.hip, ggml_hip_attn_dev): GPU-side time per call over cache lengths, both cache types, both forms.

    python tools/attn_grid.py > attn_grid.txt            # measure, on a machine with an MI355X

32 heads over 8 kv heads, D = 128, causal.  Timed as a REPLAYED graph of 32 calls rotating over cache copies (past the Infinity Cache
where the cache is small), events around the replays.  DECODE rows carry the fraction of the 8 TB/s roof for the bytes the cache holds
(K and V, each read once); PROMPT rows the fraction of the 2.5 PF f16 matrix-core roof for the causal 2 * 2 * n^2 / 2 * D
* n_head flops."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

F16, Q8_0 = 1, 8
N_HEAD, N_HEAD_KV, D = 32, 8, 128
CALLS, REPLAYS = 32, 5


def measure(kv_type, n_q, n_kv):
    rb = device.kv_row_bytes(kv_type, D)
    nb_head, nb_pos = rb, N_HEAD_KV * rb
    cache_bytes = n_kv * nb_pos
    copies = max(1, min(8, (600 << 20) // (2 * cache_bytes)))
    src = torch.rand((n_kv, N_HEAD_KV * D), device="cuda") * 2 - 1
    caches = []
    for _ in range(copies):
        k = torch.empty(cache_bytes, dtype=torch.uint8, device="cuda")
        v = torch.empty(cache_bytes, dtype=torch.uint8, device="cuda")
        device.kv_store(kv_type, src, k, nb_pos, n_kv)
        device.kv_store(kv_type, src.flip(0), v, nb_pos, n_kv)
        caches.append((k, v))
    q = torch.rand((n_q, N_HEAD, D), device="cuda") * 2 - 1
    out = torch.empty_like(q)
    work = torch.empty(max(device.attn_work_size(kv_type, D, N_HEAD, N_HEAD_KV, n_q, n_kv), 16), dtype=torch.uint8, device="cuda")
    run = lambda i: device.attention(kv_type, q, caches[i % copies][0], caches[i % copies][1], nb_pos, nb_head, N_HEAD_KV, n_kv, out=out, work=work)
    run(0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(CALLS):
                run(i)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    best = float("inf")
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1000.0 / CALLS)
    return best, 2 * cache_bytes


def main():
    device.init(0)
    print("# us per ggml_hip_attn_dev call, GPU side: replayed graphs of 32 calls rotating over cache copies; 32 heads over 8 kv heads, D = 128, causal")
    print("# DECODE: fraction of 8 TB/s for the cache's bytes (K + V) read once.  PROMPT: fraction of 2.5 PF f16 for the causal flops.")
    print("form    type   n_q    n_kv        us   roof")
    for kv_type, name in ((F16, "f16"), (Q8_0, "q8_0")):
        for n_kv in (2048, 8192, 32768):
            for n_q in (1, 4):
                us, nbytes = measure(kv_type, n_q, n_kv)
                print(f"decode  {name:5s} {n_q:4d} {n_kv:7d} {us:9.1f} {nbytes / (us * 1e-6) / 8e12:6.3f}", flush=True)
        for n in (512, 2048):
            us, _ = measure(kv_type, n, n)
            flops = 2.0 * 2.0 * n * n / 2.0 * D * N_HEAD
            print(f"prompt  {name:5s} {n:4d} {n:7d} {us:9.1f} {flops / (us * 1e-6) / 2.5e15:6.3f}", flush=True)


if __name__ == "__main__":
    main()
