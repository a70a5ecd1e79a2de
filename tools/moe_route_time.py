#!/usr/bin/env python3
"""The router and the combine of a mixture-of-experts block (ggml_hip_moe_route_dev, ggml_hip_moe_combine_dev): GPU time per call, us.

Each contender is a hipGraph of CALLS calls on one stream, replayed; the median of the round medians is reported with the spread of the
rounds.  The combine's time stands beside its byte bound: the pair rows, the addend (the residual) and the weights read, the result
written, over 8 TB/s.  At these sizes the operands (tens of MB) fit the 256 MB Infinity Cache, so a replayed call reads them from there
and not from HBM: the bound is the HBM one all the same, the figure a caller inside a decoder's graph would see lies between the two.
usage: python tools/moe_route_time.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

# (experts, n_used, tokens, M): a Mixtral-sized block, a fine-grained MoE's block
SHAPES = ((8, 2, 512, 4096), (128, 8, 512, 2048))
CALLS = 20
HBM_BYTES_PER_US = 8e6          # 8 TB/s


def _median_replay(graph, reps=20):
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        graph.replay()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def _graph_of(fn):
    fn()
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        for _ in range(CALLS):
            fn()
    g.replay()
    torch.cuda.synchronize()
    return g


def run(n_expert, n_used, n_tokens, M, rounds=5):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(n_expert + M)
    logits = torch.randn((n_tokens, n_expert), generator=gen, device="cuda")
    ids = torch.empty((n_tokens, n_used), dtype=torch.int32, device="cuda")
    wts = torch.empty((n_tokens, n_used), device="cuda")
    y = torch.randn((n_tokens, n_used, M), generator=gen, device="cuda")
    resid = torch.randn((n_tokens, M), generator=gen, device="cuda")
    out = torch.empty((n_tokens, M), device="cuda")
    graphs = {
        "route softmax": _graph_of(lambda: device.moe_route(logits, n_used, gating=0, normalize=True, ids=ids, weights=wts)),
        "route sigmoid": _graph_of(lambda: device.moe_route(logits, n_used, gating=1, normalize=True, ids=ids, weights=wts)),
        "combine": _graph_of(lambda: device.moe_combine(y, wts, addend=resid, out=out)),
    }
    per = {k: [] for k in graphs}
    for _ in range(rounds):                                   # alternate the contenders: the box's drift hits all alike
        for k, g in graphs.items():
            per[k].append(_median_replay(g) / CALLS * 1e3)
    med = {k: float(np.median(v)) for k, v in per.items()}
    spread = max(max(v) - min(v) for v in per.values())
    nbytes = 4 * (n_tokens * n_used * M + 2 * n_tokens * M + n_tokens * n_used)
    bound = nbytes / HBM_BYTES_PER_US
    print(f"{n_expert} experts, {n_used} used, {n_tokens} tokens, M {M}: route softmax {med['route softmax']:6.2f} us  sigmoid {med['route sigmoid']:6.2f} us  "
          f"combine {med['combine']:6.2f} us  beside {nbytes / 1e6:.1f} MB / 8 TB/s = {bound:5.2f} us ({med['combine'] / bound:4.2f} x)  "
          f"(spread of round medians {spread:.2f} us)", flush=True)


if __name__ == "__main__":
    device.init(0)
    for shape in SHAPES:
        run(*shape)
