#!/usr/bin/env python3
"""The rope grid (csrc/rope.hip, ggml_hip_rope_dev / ggml_hip_rope_kv_store_dev): GPU-side time per call, both modes, both cache types.

    python tools/rope_grid.py > profiles/rope_grid.txt            # measure, on a machine with an MI355X

32 heads over 8 kv heads, D = n_dims = 128, positions p0 + t.  Timed as tools/attn_grid.py times: a REPLAYED graph of 32 calls rotating over
buffer copies, events around the replays, the best of 5.  Three rows per (mode, cache type, n_tokens):
  rope      ggml_hip_rope_dev on the Q rows, in place           bytes: the rows read and written once (2 * n * 32 * 128 * 4)
  fused     ggml_hip_rope_kv_store_dev on the K rows            bytes: the rows read once, the cache rows written once
  2-call    ggml_hip_rope_dev into a temporary, then ggml_hip_kv_store_dev -- what the fused entry equals bit for bit; its roof column
            is for the FUSED entry's bytes too (the bytes the operation must move), so the two rows compare directly
roof = bytes / time / 8 TB/s.  At 1 and 4 tokens a call moves kilobytes: those rows measure a launch, not the memory system."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

F16, Q8_0 = 1, 8
N_HEAD, N_HEAD_KV, D = 32, 8, 128
CALLS, REPLAYS = 32, 5
P0 = 1000


def timed(run):
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
    return best


def measure(mode, kv_type, n):
    rp = device.rope_params(D, mode)
    rb = device.kv_row_bytes(kv_type, D)
    nb_head, nb_pos, n_pos = rb, N_HEAD_KV * rb, P0 + n
    q_bytes = 2 * n * N_HEAD * D * 4
    k_bytes = n * N_HEAD_KV * D * 4 + n * N_HEAD_KV * rb
    copies = max(1, min(8, (600 << 20) // max(q_bytes, n_pos * nb_pos)))
    qs = [torch.rand((n, N_HEAD, D), device="cuda") * 2 - 1 for _ in range(copies)]
    ks = [torch.rand((n, N_HEAD_KV, D), device="cuda") * 2 - 1 for _ in range(copies)]
    tmps = [torch.empty((n, N_HEAD_KV, D), device="cuda") for _ in range(copies)]
    caches = [torch.zeros(n_pos * nb_pos, dtype=torch.uint8, device="cuda") for _ in range(copies)]
    us_rope = timed(lambda i: device.rope(rp, qs[i % copies], pos0=P0, out=qs[i % copies]))
    us_fused = timed(lambda i: device.rope_kv_store(rp, kv_type, ks[i % copies], caches[i % copies], nb_pos, nb_head, n_pos, pos0=P0))

    def two(i):
        t = device.rope(rp, ks[i % copies], pos0=P0, out=tmps[i % copies])
        device.kv_store(kv_type, t.view(n, N_HEAD_KV * D), caches[i % copies], nb_pos, n_pos, pos0=P0)

    us_two = timed(two)
    return (us_rope, q_bytes), (us_fused, k_bytes), (us_two, k_bytes)


def main():
    device.init(0)
    print("# us per call, GPU side: replayed graphs of 32 calls rotating over buffer copies; 32 heads over 8 kv heads, D = n_dims = 128")
    print("# rope: ggml_hip_rope_dev on Q in place.  fused: ggml_hip_rope_kv_store_dev on K.  2-call: rope into a temporary + kv_store (the same bits).")
    print("# roof: fraction of 8 TB/s for the bytes the operation must move (2-call: the fused entry's bytes)")
    print("entry   mode    type  n_tokens        us   roof")
    for mode, mname in ((0, "normal"), (2, "neox")):
        for kv_type, tname in ((F16, "f16"), (Q8_0, "q8_0")):
            for n in (1, 4, 512, 2048):
                for name, (us, nbytes) in zip(("rope", "fused", "2-call"), measure(mode, kv_type, n)):
                    print(f"{name:7s} {mname:7s} {tname:5s} {n:8d} {us:9.2f} {nbytes / (us * 1e-6) / 8e12:6.3f}", flush=True)


if __name__ == "__main__":
    main()
