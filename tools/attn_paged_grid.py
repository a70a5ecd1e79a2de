#!/usr/bin/env python3
"""The paged attention grid (csrc/attn.hip, ggml_hip_attn_paged_dev): one paged call for n_seq sequences against the n_seq calls of
ggml_hip_attn_dev that do the same work, GPU-side time per STEP.

    python tools/attn_paged_grid.py > attn_paged_grid.txt      # measure, on a machine with an MI355X

32 heads over 8 kv heads, D = 128, causal.  A step is one paged call, or n_seq contiguous calls; timed as a REPLAYED graph of 32 steps
rotating over pool copies, events around the replays, the best of 5 replays.  The pool is n_seq * ceil(n_kv / 128) pages under a random page
assignment; the contiguous calls read slices of the same pool (the same bytes, laid out in order).  The contiguous side is measured twice,
before and after the paged side: the difference between its two figures is the run-to-run spread a ratio has to be read against.
`oversized` is the paged call with n_kv_max = 8 x n_kv (seven of eight DECODE workgroups launched to leave at once)."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

F16, Q8_0 = 1, 8
N_HEAD, N_HEAD_KV, D = 32, 8, 128
STEPS, REPLAYS = 32, 5
PAGE = 128


def timed(step):
    """us per step: a graph of STEPS steps, replayed"""
    step(0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(STEPS):
                step(i)
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
        best = min(best, e0.elapsed_time(e1) * 1000.0 / STEPS)
    return best


def measure(kv_type, n_seq, n_q, n_kv, oversize=1):
    """(contiguous us, paged us, contiguous us again) per step"""
    rb = device.kv_row_bytes(kv_type, D)
    nb_head, nb_pos = rb, N_HEAD_KV * rb
    nb_page = PAGE * nb_pos
    chunks = (n_kv + PAGE - 1) // PAGE
    n_pages = n_seq * chunks
    pool_bytes = n_pages * nb_page
    copies = max(1, min(8, (600 << 20) // (2 * pool_bytes)))
    n_kv_max = oversize * n_kv
    ld_pages = (n_kv_max + PAGE - 1) // PAGE
    rng = np.random.default_rng(n_seq * 1000003 + n_kv)
    table = np.full((n_seq, ld_pages), -1, np.int32)
    table[:, :chunks] = rng.permutation(n_pages).astype(np.int32).reshape(n_seq, chunks)
    pages = torch.from_numpy(table).cuda()
    d_len = torch.full((n_seq,), n_kv - n_q, dtype=torch.int32, device="cuda")
    src = torch.rand((PAGE, N_HEAD_KV * D), device="cuda") * 2 - 1
    caches = []
    for _ in range(copies):
        k = torch.empty(pool_bytes, dtype=torch.uint8, device="cuda")
        v = torch.empty(pool_bytes, dtype=torch.uint8, device="cuda")
        for p in range(n_pages):                                    # every page holds finite rows
            device.kv_store(kv_type, src, k[p * nb_page:], nb_pos, PAGE)
            device.kv_store(kv_type, src.flip(0), v[p * nb_page:], nb_pos, PAGE)
        caches.append(device.PagedCache(kv_type, k, v, nb_page, nb_pos, nb_head, n_pages, pages, d_len, n_kv_max))
    q = torch.rand((n_seq * n_q, N_HEAD, D), device="cuda") * 2 - 1
    out = torch.empty_like(q)
    work = torch.empty(max(device.attn_paged_work_size(kv_type, D, N_HEAD, N_HEAD_KV, n_seq, n_q, n_kv_max), 16), dtype=torch.uint8, device="cuda")
    work1 = torch.empty(max(device.attn_work_size(kv_type, D, N_HEAD, N_HEAD_KV, n_q, n_kv), 16), dtype=torch.uint8, device="cuda")

    def paged(i):
        device.attn_paged(caches[i % copies], q, N_HEAD_KV, len_bias=n_q, out=out, work=work)

    def contiguous(i):
        pc = caches[i % copies]
        for b in range(n_seq):
            o = b * chunks * nb_page
            device.attention(kv_type, q[b * n_q:(b + 1) * n_q], pc.k[o:], pc.v[o:], nb_pos, nb_head, N_HEAD_KV, n_kv, out=out[b * n_q:(b + 1) * n_q], work=work1)

    first = timed(contiguous)
    mid = timed(paged)
    return first, mid, timed(contiguous)


def main():
    device.init(0)
    print("# us per STEP, GPU side: one ggml_hip_attn_paged_dev call for n_seq sequences against n_seq ggml_hip_attn_dev calls; replayed graphs of")
    print("# 32 steps rotating over pool copies; 32 heads over 8 kv heads, D = 128, causal.  contig / contig2: the contiguous side before and after")
    print("# the paged side (their difference is the spread).  ratio = paged / min(contig, contig2).")
    print("form      type  n_seq  n_q    n_kv  n_kv_max    contig   contig2     paged  ratio")

    def row(form, name, kv_type, n_seq, n_q, n_kv, oversize=1):
        a, p, b = measure(kv_type, n_seq, n_q, n_kv, oversize)
        print(f"{form:9s} {name:5s} {n_seq:5d} {n_q:4d} {n_kv:7d} {oversize * n_kv:9d} {a:9.1f} {b:9.1f} {p:9.1f} {p / min(a, b):6.3f}", flush=True)

    for kv_type, name in ((F16, "f16"), (Q8_0, "q8_0")):
        for n_kv in (2048, 8192):
            for n_seq in (1, 8, 32):
                row("decode", name, kv_type, n_seq, 1, n_kv)
        row("oversized", name, kv_type, 8, 1, 2048, oversize=8)
        row("prompt", name, kv_type, 4, 512, 512)


if __name__ == "__main__":
    main()
