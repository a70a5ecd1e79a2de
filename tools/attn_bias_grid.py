#!/usr/bin/env python3
"""The attention grid of tools/attn_grid.py for the mask entries (csrc/attn.hip, ggml_hip_attn_bias_dev), by the same method: GPU-side time per
call of a REPLAYED graph of 32 calls rotating over cache copies, events around the replays; here the MEDIAN of 7 replays with their spread.

    python tools/attn_bias_grid.py                        # the price of the mask: the bias entry with a zero mask against the _ex entry without one
    python tools/attn_bias_grid.py --entries base,ex      # the existing entries alone (base: ggml_hip_attn_dev; ex: ggml_hip_attn_ex_dev, soft-cap 30 and sinks)
    python tools/attn_bias_grid.py --entries base,ex --lib /path/to/another/libggml_hip.so      # the same on another build of the library

The last two, run alternately on this build and on the parent commit's, show whether the existing entries kept their time: the margin is the
spread of the parent's own repeated runs.  32 heads over 8 kv heads, D = 128, causal; n_kv 2048 / 8192 / 32768 with n_q 1 / 4 (DECODE), n_q = n_kv =
512 / 2048 (PROMPT); both cache types."""
import argparse
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import _lib, device  # noqa: E402

F16, Q8_0 = 1, 8
N_HEAD, N_HEAD_KV, D = 32, 8, 128
CALLS, REPLAYS = 32, 7
BIAS_SYMBOLS = ("ggml_hip_alibi_slopes", "ggml_hip_attn_bias_dev", "ggml_hip_attn_paged_bias_dev", "ggml_hip_attn_paged_ragged_bias_dev")


def measure(kv_type, n_q, n_kv, entries):
    """{entry: (median, min, max) us per call}; the entries share the caches, the queries and the work buffer"""
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
    sinks = torch.zeros(N_HEAD, device="cuda")
    mask = torch.zeros((n_q, n_kv), dtype=torch.float16, device="cuda") if "bias" in entries else None
    extra = {"base": {}, "ex": dict(softcap=30.0, sinks=sinks), "bias": dict(mask=mask)}
    res = {}
    for entry in entries:
        kw = extra[entry]
        run = lambda i: device.attention(kv_type, q, caches[i % copies][0], caches[i % copies][1], nb_pos, nb_head, N_HEAD_KV, n_kv, out=out, work=work, **kw)
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
        us = []
        for _ in range(REPLAYS):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            g.replay()
            e1.record()
            torch.cuda.synchronize()
            us.append(e0.elapsed_time(e1) * 1000.0 / CALLS)
        res[entry] = (statistics.median(us), min(us), max(us))
    return res


def shapes():
    for kv_type, name in ((F16, "f16"), (Q8_0, "q8_0")):
        for n_kv in (2048, 8192, 32768):
            for n_q in (1, 4):
                yield "decode", kv_type, name, n_q, n_kv
        for n in (512, 2048):
            yield "prompt", kv_type, name, n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="", help="base,ex: time the existing entries alone (for a comparison between two builds)")
    ap.add_argument("--lib", default="", help="another build of libggml_hip.so to load instead of this tree's")
    args = ap.parse_args()
    if args.lib:
        _lib.LIB_PATH = os.path.abspath(args.lib)
        for name in BIAS_SYMBOLS:                                    # (a build from before the mask entries does not export them)
            _lib.HIP_SYMBOLS.pop(name, None)
    device.init(0)
    print(f"# us per call, GPU side: replayed graphs of {CALLS} calls rotating over cache copies, median of {REPLAYS} replays (min .. max); 32 heads over 8 kv heads, D = 128, causal")
    if args.entries:
        entries = args.entries.split(",")
        print(f"# library: {args.lib or 'this tree'}")
        print("form    type   n_q    n_kv  entry       us      min      max")
        for form, kv_type, name, n_q, n_kv in shapes():
            for entry, (med, lo, hi) in measure(kv_type, n_q, n_kv, entries).items():
                print(f"{form:7s} {name:5s} {n_q:4d} {n_kv:7d}  {entry:5s} {med:8.1f} {lo:8.1f} {hi:8.1f}", flush=True)
        return
    print("# ex: ggml_hip_attn_ex_dev with every option off (no mask).  bias: ggml_hip_attn_bias_dev with a mask of zeros, no slopes, the same bits.")
    print("form    type   n_q    n_kv     ex us  (min .. max)    bias us  (min .. max)   bias / ex")
    for form, kv_type, name, n_q, n_kv in shapes():
        r = measure(kv_type, n_q, n_kv, ("base", "bias"))
        a, b = r["base"], r["bias"]
        print(f"{form:7s} {name:5s} {n_q:4d} {n_kv:7d} {a[0]:9.1f} ({a[1]:.1f} .. {a[2]:.1f}) {b[0]:10.1f} ({b[1]:.1f} .. {b[2]:.1f}) {b[0] / a[0]:9.3f}", flush=True)


if __name__ == "__main__":
    main()
