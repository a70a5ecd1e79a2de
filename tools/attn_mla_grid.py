#!/usr/bin/env python3
"""The MLA grid (csrc/mla.hip, ggml_hip_attn_mla_paged_dev): GPU-side time per call beside the two roofs of the chip.

    python tools/attn_mla_grid.py > profiles/attn_mla_grid.txt            # measure, on a machine with an MI355X

Rows: DECODE (n_q = 1) at 16 and 128 heads over 1 / 32 / 128 sequences of 4K / 32K positions, VERIFY (n_q = 4) at 128 heads and 32 sequences, PREFILL
of one sequence of 512 / 2048 tokens (n_q = n_kv, causal); both cache types.  The span of the SPLIT form is a compile-time constant (plan.h MLA_SPAN): the
table prints the one the library was built with -- build once per value to compare.
Timed as tools/ssm_grid.py times: a REPLAYED graph of CALLS calls, events around the replays, the MEDIAN of 21.  The pool is one latent pool of at least
512 MiB (beyond the 256 MiB Infinity Cache) and call i of a graph walks its own pages, so a decode call does not find its cache in a cache the previous
call filled; CALLS = ceil(512 MiB / the batch's cache bytes), between 2 and 64.
  bytes  = n_seq * n_kv * the bytes of a row: every position of the batch once (a call with more than 64 rows per sequence reads it once per row tile);
  flop   = rows * visible positions * 2 * (576 + 512): the score over 576 columns and the value over 512, the duplicated score of a row half not counted;
  mem    = bytes / time / 8 TB/s;  mfma = flop / time / 2.5 PF;  part = the bytes of the partials the merge reads / bytes (the merge is not timed alone)."""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

F16, Q8_0 = 1, 8
DK, DV, PAGE = 576, 512, 128
REPLAYS, POOL_MIN = 21, 512 << 20
SCALE = 0.135
ROWS = ([("decode", h, s, 1, kv) for h in (16, 128) for s in (1, 32, 128) for kv in (4096, 32768)]
        + [("verify", 128, 32, 4, kv) for kv in (4096, 32768)]
        + [("prefill", h, 1, n, n) for h in (16, 128) for n in (512, 2048)])


def timed(run, calls):
    run(0)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            for i in range(calls):
                run(i)
    torch.cuda.current_stream().wait_stream(s)
    g.replay()
    torch.cuda.synchronize()
    times = []
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        times.append(e0.elapsed_time(e1) * 1000.0 / calls)
    return statistics.median(times)


def filled_pool(kv_type, n_pages, nb_pos):
    """a pool of n_pages pages of finite rows (one block of seeded rows stored over and over)"""
    pool = torch.empty(n_pages * PAGE * nb_pos, dtype=torch.uint8, device="cuda")
    block = 1 << 15
    x = torch.rand((block, DK), device="cuda") * 2.0 - 1.0
    n = n_pages * PAGE
    for p0 in range(0, n, block):
        device.kv_store(kv_type, x[:min(block, n - p0)], pool, nb_pos, n, pos0=p0)
    return pool


def measure(kv_type, kind, n_head, n_seq, n_q, n_kv):
    rb = device.kv_row_bytes(kv_type, DK)
    nb_pos = (rb + 15) // 16 * 16
    per_seq = (n_kv + PAGE - 1) // PAGE
    batch_bytes = n_seq * n_kv * rb
    calls = max(2, min(64, (POOL_MIN + batch_bytes - 1) // batch_bytes))
    n_pages = calls * n_seq * per_seq
    pool = filled_pool(kv_type, n_pages, nb_pos)
    d_len = torch.full((n_seq,), n_kv - n_q, dtype=torch.int32, device="cuda")
    caches = []
    for i in range(calls):
        tab = (torch.arange(n_seq * per_seq, dtype=torch.int32) + i * n_seq * per_seq).reshape(n_seq, per_seq).cuda()
        caches.append(device.LatentCache(kv_type, pool, PAGE * nb_pos, nb_pos, n_pages, tab, d_len, n_kv))
    q = torch.rand((n_seq * n_q, n_head, DK), device="cuda") * 2.0 - 1.0
    out = torch.empty((n_seq * n_q, n_head, DV), device="cuda")
    plan = device.attn_mla_plan(kv_type, n_head, n_q, n_kv, n_seq)
    work = torch.empty(max(int(plan.work_bytes), 16), dtype=torch.uint8, device="cuda")
    us = timed(lambda i: device.attn_mla_paged(caches[i], q, SCALE, len_bias=n_q, out=out, work=work), calls)
    assert torch.isfinite(out).all()
    rows = n_seq * n_q * n_head
    visible = sum(n_kv - n_q + t + 1 for t in range(n_q)) * n_seq * n_head       # causal: row t sees n_kv - n_q + t + 1 positions
    flop = visible * 2 * (DK + DV)
    part = rows * plan.n_spans * (DV + 4) * 4 if plan.form == 1 else 0
    return us, calls, plan, batch_bytes, flop, part


def main():
    device.init(0)
    print("# MLA grid: %s" % torch.cuda.get_device_name(0))
    print("# kind     type  heads  seqs  n_q   n_kv  form span  calls     time_us    mem(8TB/s)  mfma(2.5PF)  part/bytes")
    for kv_type, tname in ((F16, "F16"), (Q8_0, "Q8_0")):
        for kind, n_head, n_seq, n_q, n_kv in ROWS:
            us, calls, plan, nbytes, flop, part = measure(kv_type, kind, n_head, n_seq, n_q, n_kv)
            print("%-9s %-5s %5d %5d %4d %6d  %-5s %3d  %5d  %10.1f  %10.1f %%  %10.1f %%  %9.3f" % (
                kind, tname, n_head, n_seq, n_q, n_kv, "SPLIT" if plan.form == 1 else "WALK", plan.span, calls, us,
                100.0 * nbytes / (us * 1e-6) / 8e12, 100.0 * flop / (us * 1e-6) / 2.5e15, part / nbytes))
            sys.stdout.flush()
            torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
