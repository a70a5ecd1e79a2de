#!/usr/bin/env python3
"""The ragged paged attention call (ggml_hip_attn_paged_ragged_dev) beside the route a host has without it for the same step: one uniform
paged call (ggml_hip_attn_paged_dev) per distinct n_q.  Whole-call GPU time, us, on the same build.

Both contenders are hipGraphs of CALLS whole steps on one stream over the same pool, page table and lengths, replayed in turn -- ragged,
uniform, ragged, ... -- and the median of the round medians is reported with their spread.  Q8_0 cache, D = 128, 32 heads over 8 kv heads,
every sequence on its own pages.  Two mixes of 64 sequences:
  mixed:   60 decode one token over 1000 .. 4000 cached positions, 4 prefill 512 tokens into an empty cache (the uniform route: two calls);
  decode:  all 64 decode one token (the uniform route: one call -- here the ragged entry can only lose, by its index launch and its exits).
usage: python tools/attn_ragged_time.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

Q8_0 = 8
D, N_HEAD, N_HEAD_KV, PAGE = 128, 32, 8, 128
CALLS = 4
MIXES = (("mixed", [1] * 60 + [512] * 4, [int(x) for x in np.linspace(1000, 4000, 60)] + [0] * 4),
         ("decode", [1] * 64, [int(x) for x in np.linspace(1000, 4000, 64)]))


def _median_replay(graph, reps=10):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def run(label, n_qs, lens, rounds=5):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(len(n_qs) + sum(n_qs))
    n_seq, n_tok = len(n_qs), sum(n_qs)
    n_kv_max = (max(l + n for l, n in zip(lens, n_qs)) + PAGE - 1) // PAGE * PAGE
    ld_pages = n_kv_max // PAGE
    need = [(l + n + PAGE - 1) // PAGE for l, n in zip(lens, n_qs)]
    n_pages = sum(need)
    rb = device.kv_row_bytes(Q8_0, D)
    nb_head, nb_pos = rb, N_HEAD_KV * rb
    nb_page = PAGE * nb_pos
    pools = [device.quantize_rows(Q8_0, torch.randn((n_pages * PAGE * N_HEAD_KV, D), generator=gen, device="cuda")).reshape(-1) for _ in range(2)]
    table = np.full((n_seq, ld_pages), -1, np.int32)
    ids = np.random.default_rng(n_seq).permutation(n_pages)
    at = 0
    for b, k in enumerate(need):
        table[b, :k] = ids[at:at + k]
        at += k
    pages = torch.from_numpy(table).cuda()
    d_len = torch.tensor(lens, dtype=torch.int32, device="cuda")
    q = torch.randn((n_tok, N_HEAD, D), generator=gen, device="cuda")
    q_start = torch.from_numpy(np.concatenate([[0], np.cumsum(n_qs)]).astype(np.int32)).cuda()
    pc = device.PagedCache(Q8_0, pools[0], pools[1], nb_page, nb_pos, nb_head, n_pages, pages, d_len, n_kv_max)
    n_dec = min(n_tok, 8 * n_seq)
    out_r = torch.zeros_like(q)
    work_r = torch.empty(device.attn_paged_ragged_work_size(Q8_0, D, N_HEAD, N_HEAD_KV, n_seq, n_tok, n_dec, n_kv_max), dtype=torch.uint8, device="cuda")
    # the uniform route: the sequences of each distinct n_q, contiguous in the batch here, as one paged call over their rows of the table
    groups = []
    row = 0
    for n_q in sorted(set(n_qs)):
        idx = [b for b, n in enumerate(n_qs) if n == n_q]
        assert idx == list(range(idx[0], idx[-1] + 1))
        g_pc = device.PagedCache(Q8_0, pools[0], pools[1], nb_page, nb_pos, nb_head, n_pages, pages[idx[0]:idx[-1] + 1], d_len[idx[0]:idx[-1] + 1], n_kv_max)
        rows = n_q * len(idx)
        work = torch.empty(max(device.attn_paged_work_size(Q8_0, D, N_HEAD, N_HEAD_KV, len(idx), n_q, n_kv_max), 16), dtype=torch.uint8, device="cuda")
        groups.append((g_pc, int(q_start[idx[0]]), rows, n_q, work))
    out_u = torch.zeros_like(q)

    def ragged():
        device.attn_paged_ragged(pc, q_start, q, N_HEAD_KV, add_q=True, n_dec_rows_max=n_dec, out=out_r, work=work_r)

    def uniform():
        for g_pc, r0, rows, n_q, work in groups:
            device.attn_paged(g_pc, q[r0:r0 + rows], N_HEAD_KV, len_bias=n_q, out=out_u[r0:r0 + rows], work=work)

    graphs = {}
    for name, fn in (("ragged", ragged), ("uniform", uniform)):
        fn()
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for _ in range(CALLS):
                fn()
        g.replay()
        torch.cuda.synchronize()
        graphs[name] = g
    assert torch.equal(out_r, out_u), "the ragged call and the uniform calls differ"
    per = {k: [] for k in graphs}
    for _ in range(rounds):                                   # alternate the contenders: the box's drift hits both alike
        for k, g in graphs.items():
            per[k].append(_median_replay(g) / CALLS * 1e3)
    a, b = float(np.median(per["ragged"])), float(np.median(per["uniform"]))
    spread = max(max(v) - min(v) for v in per.values())
    print(f"{label}: {n_seq} sequences, {n_tok} rows, n_kv_max {n_kv_max}, {len(groups)} uniform call(s): ragged {a:8.1f} us  uniform {b:8.1f} us  "
          f"ragged/uniform {a / b:5.2f}  (spread of round medians {spread:.1f} us)", flush=True)


if __name__ == "__main__":
    device.init(0)
    for mix in MIXES:
        run(*mix)
