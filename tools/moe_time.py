#!/usr/bin/env python3
"""Expert-routed products (ggml_hip_mul_mat_id_dev) on the device, us per projection.

By-id route: ONE launch for all (token, slot) pairs of a projection against the same pairs issued as separate N = 1 ggml_hip_mul_mat_dev
calls.  Both contenders are hipGraphs of NODES projections on one stream, every projection on its own set of experts (rotating copies: more
than 256 MB of distinct weights, so nothing is served from the Infinity Cache), replayed in turn -- by-id, separate, by-id, ... -- and the
median of the round medians is reported with their spread.
Batch route: 512 tokens x 2 of 8 experts of 4096 x 4096 (ids on the host: no synchronize) against ONE 4096 x 4096 x 1024 product of the same
type -- the same number of rows through one expert, an upper bound on the useful work.
usage: python tools/moe_time.py [byid|batch ...]"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

Q4_0, Q8_0, Q4_K = 2, 8, 112
NAME = {Q4_0: "Q4_0", Q8_0: "Q8_0", Q4_K: "Q4_K"}
RESIDENT_B_PER_WEIGHT = {Q4_0: 0.69, Q8_0: 1.25, Q4_K: 0.94}
# (experts, M, K, n_tokens, n_used): a fine-grained MoE's expert at 8 per token, a Mixtral-sized expert at 2 per token, 8 pairs of 4096 x 4096
BYID_SHAPES = ((128, 768, 2048, 1, 8), (8, 14336, 4096, 1, 2), (8, 4096, 4096, 1, 8))
NODES = 16


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


def _expert_rows(t, M, K, n, gen):
    """n distinct experts' rows in type t's format (one random matrix quantized, then rolled by rows: distinct bytes, one quantizer run)"""
    rows = device.quantize_rows(t, torch.randn((M, K), generator=gen, device="cuda"))
    return [torch.roll(rows, shifts=i, dims=0).contiguous() for i in range(n)]


def byid(t, n_expert, M, K, n_tokens, n_used, rounds=5):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(M + K)
    touched = n_tokens * n_used * M * K * RESIDENT_B_PER_WEIGHT[t]           # bytes a projection streams
    copies = max(2, min(NODES, -(-int(400e6) // int(touched))))
    base = _expert_rows(t, M, K, min(n_expert, 8), gen)
    sets, ids = [], []
    for c in range(copies):
        # a projection touches n_tokens * n_used experts: those are distinct weights per copy, the others of a large set share resident weights
        hot = [device.Weight.from_device(t, base[(c + i) % len(base)], K) for i in range(n_tokens * n_used)]
        ws = [hot[e % len(hot)] for e in range(n_expert)]
        sets.append((device.ExpertSet(ws), ws, hot))
        ids.append(torch.arange(n_tokens * n_used, dtype=torch.int32, device="cuda").reshape(n_tokens, n_used))
    x = torch.randn((n_tokens, K), generator=gen, device="cuda")
    out = torch.empty((n_tokens, n_used, M), device="cuda")
    work = torch.empty(16, dtype=torch.uint8, device="cuda")
    assert sets[0][0].route(n_tokens, n_used) == 1

    def one(c):
        device.mul_mat_id(sets[c][0], ids[c], x, out=out, work=work)

    def separate(c):
        for tk in range(n_tokens):
            for s in range(n_used):
                device.mul_mat(sets[c][2][tk * n_used + s], x[tk:tk + 1], out=out[tk, s:s + 1], work=work)

    graphs = {}
    for label, fn in (("by-id", one), ("separate", separate)):
        for c in range(copies):
            fn(c)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(NODES):
                fn(i % copies)
        g.replay()
        torch.cuda.synchronize()
        graphs[label] = g
    per = {k: [] for k in graphs}
    for _ in range(rounds):                                   # alternate the contenders: the box's drift hits both alike
        for k, g in graphs.items():
            per[k].append(_median_replay(g) / NODES * 1e3)
    a, b = float(np.median(per["by-id"])), float(np.median(per["separate"]))
    spread = max(max(v) - min(v) for v in per.values())
    print(f"{NAME[t]} {n_expert} experts of {M}x{K}, {n_tokens * n_used} pairs: by-id {a:7.2f} us  separate {b:7.2f} us  by-id/separate {a / b:5.3f}  "
          f"({copies} weight copies, spread of round medians {spread:.2f} us)", flush=True)
    graphs.clear()
    torch.cuda.synchronize()
    for es, _, hot in sets:
        es.free()
        for w in hot:
            w.free()


def batch(t, n_expert=8, M=4096, K=4096, n_tokens=512, n_used=2, rounds=5):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(7)
    copies = 4
    base = _expert_rows(t, M, K, n_expert, gen)
    sets = []
    for c in range(copies):
        ws = [device.Weight.from_device(t, torch.roll(base[e], shifts=c + 1, dims=0).contiguous(), K) for e in range(n_expert)]
        sets.append((device.ExpertSet(ws), ws))
    h_ids = np.stack([np.random.default_rng(tk).permutation(n_expert)[:n_used] for tk in range(n_tokens)]).astype(np.int32)
    ids = torch.from_numpy(h_ids).cuda()
    x = torch.randn((n_tokens, K), generator=gen, device="cuda")
    xs = torch.randn((n_tokens * n_used, K), generator=gen, device="cuda")
    out = torch.empty((n_tokens, n_used, M), device="cuda")
    out1 = torch.empty((n_tokens * n_used, M), device="cuda")
    work = torch.empty(sets[0][0].work_size(n_tokens, n_used), dtype=torch.uint8, device="cuda")
    work1 = device.alloc_work(t, K, n_tokens * n_used)
    assert sets[0][0].route(n_tokens, n_used) == 2

    def routed(c):
        device.mul_mat_id(sets[c][0], ids, x, h_ids=h_ids, out=out, work=work)

    def single(c):
        device.mul_mat(sets[c][1][0], xs, out=out1, work=work1)

    graphs = {}
    for label, fn in (("mul_mat_id", routed), ("one product", single)):
        for c in range(copies):
            fn(c)
        torch.cuda.synchronize()
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g):
            for i in range(2 * copies):
                fn(i % copies)
        g.replay()
        torch.cuda.synchronize()
        graphs[label] = g
    per = {k: [] for k in graphs}
    for _ in range(rounds):
        for k, g in graphs.items():
            per[k].append(_median_replay(g) / (2 * copies) * 1e3)
    a, b = float(np.median(per["mul_mat_id"])), float(np.median(per["one product"]))
    spread = max(max(v) - min(v) for v in per.values())
    print(f"{NAME[t]} batch route {n_tokens} tokens x {n_used} of {n_expert} experts of {M}x{K}: {a:8.1f} us  one {M}x{K}x{n_tokens * n_used} product {b:8.1f} us  "
          f"ratio {a / b:5.2f}  (spread of round medians {spread:.1f} us)", flush=True)
    graphs.clear()
    torch.cuda.synchronize()
    for es, ws in sets:
        es.free()
        for w in ws:
            w.free()


if __name__ == "__main__":
    device.init(0)
    what = sys.argv[1:] or ["byid", "batch"]
    for t in (Q4_0, Q8_0, Q4_K):
        if "byid" in what:
            for shape in BYID_SHAPES:
                byid(t, *shape)
        if "batch" in what:
            batch(t)
