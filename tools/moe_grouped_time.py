#!/usr/bin/env python3
"""The grouped route of expert-routed products (ggml_hip_mul_mat_id_grouped_dev) beside the batch route (ggml_hip_mul_mat_id_dev, route 2,
with the ids given on the host so that it needs no synchronize): whole-call GPU time, us, on the same build.

Both contenders are hipGraphs of CALLS whole calls on one stream over the same set, ids and src1, replayed in turn -- grouped, batch,
grouped, ... -- and the median of the round medians is reported with their spread.  The ids are a top-k-like routing: n_used distinct
experts per token, drawn uniformly.  A set's weights are streamed from HBM where the set is larger than the 256 MB Infinity Cache (the two
14336 x 4096 shapes); the 128-expert set of 768 x 2048 is about its size.
usage: python tools/moe_grouped_time.py"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

Q4_0, Q8_0 = 2, 8
NAME = {Q4_0: "Q4_0", Q8_0: "Q8_0"}
# (type, experts, M, K, n_used): a Mixtral-sized expert at 2 per token, a fine-grained MoE's expert at 8 per token
SHAPES = ((Q4_0, 8, 14336, 4096, 2), (Q8_0, 8, 14336, 4096, 2), (Q8_0, 128, 768, 2048, 8))
TOKENS = (32, 128, 512)
CALLS = 4


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


def run(t, n_expert, M, K, n_used, rounds=5):
    gen = torch.Generator(device="cuda")
    gen.manual_seed(M + K)
    rows = device.quantize_rows(t, torch.randn((M, K), generator=gen, device="cuda"))
    ws = [device.Weight.from_device(t, torch.roll(rows, shifts=e, dims=0).contiguous(), K) for e in range(n_expert)]
    es = device.ExpertSet(ws)
    assert es.grouped_serves() == 1
    for n_tokens in TOKENS:
        h_ids = np.stack([np.random.default_rng(tk).permutation(n_expert)[:n_used] for tk in range(n_tokens)]).astype(np.int32)
        ids = torch.from_numpy(h_ids).cuda()
        x = torch.randn((n_tokens, K), generator=gen, device="cuda")
        out = torch.empty((n_tokens, n_used, M), device="cuda")
        work_g = torch.empty(es.grouped_work_size(n_tokens, n_used), dtype=torch.uint8, device="cuda")
        work_b = torch.empty(es.work_size(n_tokens, n_used), dtype=torch.uint8, device="cuda")
        assert es.route(n_tokens, n_used) == 2

        def grouped():
            device.mul_mat_id_grouped(es, ids, x, out=out, work=work_g)

        def batch():
            device.mul_mat_id(es, ids, x, h_ids=h_ids, out=out, work=work_b)

        graphs = {}
        for label, fn in (("grouped", grouped), ("batch", batch)):
            fn()
            torch.cuda.synchronize()
            g = torch.cuda.CUDAGraph()
            with torch.cuda.graph(g):
                for _ in range(CALLS):
                    fn()
            g.replay()
            torch.cuda.synchronize()
            graphs[label] = g
        per = {k: [] for k in graphs}
        for _ in range(rounds):                               # alternate the contenders: the box's drift hits both alike
            for k, g in graphs.items():
                per[k].append(_median_replay(g) / CALLS * 1e3)
        a, b = float(np.median(per["grouped"])), float(np.median(per["batch"]))
        spread = max(max(v) - min(v) for v in per.values())
        tiles = int(np.sum((np.bincount(h_ids.reshape(-1), minlength=n_expert) + 31) // 32))
        print(f"{NAME[t]} {n_expert} experts of {M}x{K}, {n_tokens} tokens x {n_used} ({tiles} column tiles filled): grouped {a:8.1f} us  batch (h_ids) {b:8.1f} us  "
              f"grouped/batch {a / b:5.2f}  (spread of round medians {spread:.1f} us)", flush=True)
        graphs.clear()
        torch.cuda.synchronize()
    es.free()
    for w in ws:
        w.free()


if __name__ == "__main__":
    device.init(0)
    for shape in SHAPES:
        run(*shape)
