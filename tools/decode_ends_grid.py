#!/usr/bin/env python3
"""The decode-ends grid (csrc/get_rows.hip, sample.hip: ggml_hip_get_rows_dev, ggml_hip_argmax_rows_dev, ggml_hip_sample_topk_dev): GPU-side
time per call.

    python tools/decode_ends_grid.py > profiles/decode_ends_grid.txt      # measure, on a machine with an MI355X

Timed as tools/rope_grid.py times: a REPLAYED graph of 32 calls rotating over buffer copies, events around the replays, the best of 5.
  get_rows   Q8_0, Q4_K and F16 at 32000 x 4096, Q8_0 at 152064 x 4096; 1 / 4 / 512 / 2048 random ids.
             bytes: a row in its file format read once + K floats written, per id
  argmax     ggml_hip_argmax_rows_dev, 1 and 8 rows of 32000 / 152064 / 262144 logits.           bytes: the logits read once
  sample     ggml_hip_sample_topk_dev, k = 40, top_p 0.9, with the pick; the same shapes.        bytes: the same
  sample-k1  the same entry at k = 1 (one round in each stage): sample - sample-k1 is what the 39 further rounds of both stages cost
roof = bytes / time / 8 TB/s.  floor = time / 3 us, the launch floor DESIGN.md 17 measured (one launch; the sampler is two): given for the
one-row (one-id) cases, which move kilobytes and measure launches, not the memory system.
Timed here, not checked: the kernel forms these vocabularies select (k = 40: 8 / 38 / 64 chunks, 2 / 8 / 16 candidate keys per thread in the
merge) are held to their yardsticks by tests/test_decode_ends.py, at vocabularies of 4, 8, 16, 32, 64 and 128 chunks of 4096 logits, of
4, 8, ... 128 chunks and one logit, and of 2^20 logits (every merge form, full and nearly empty)."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import _lib, device  # noqa: E402

F16, Q8_0, Q4_K = 1, 8, _lib.Q4_K
K = 4096
CALLS, REPLAYS = 32, 5
FLOOR_US = 3.0


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


def make_weight(type, M):
    """M random rows of K in the file format of `type`, made on the device in slices, as a resident weight"""
    rb = _lib.row_bytes(type, K)
    rows = torch.empty((M, rb), dtype=torch.uint8, device="cuda")
    step = 8192
    for r0 in range(0, M, step):
        x = torch.randn((min(step, M - r0), K), device="cuda")
        rows[r0:r0 + x.shape[0]] = x.to(torch.float16).view(torch.uint8) if type == F16 else device.quantize_rows(type, x)
    w = device.Weight.from_device(type, rows, K)
    torch.cuda.synchronize()
    return w, rb


def line(name, what, n, us, nbytes, one):
    floor = f"{us / FLOOR_US:6.2f}" if one else "     -"
    print(f"{name:9s} {what:16s} {n:6d} {us:9.2f} {nbytes / (us * 1e-6) / 8e12:6.3f} {floor}", flush=True)


def main():
    device.init(0)
    print("# us per call, GPU side: replayed graphs of 32 calls rotating over buffer copies")
    print("# roof: fraction of 8 TB/s for the bytes the call must move.  floor: time / 3 us (one launch), one-row cases only")
    print("entry     what               n/rows        us   roof  floor")
    for type, tname, M in ((Q8_0, "q8_0", 32000), (Q4_K, "q4_k", 32000), (F16, "f16", 32000), (Q8_0, "q8_0", 152064)):
        w, rb = make_weight(type, M)
        for n in (1, 4, 512, 2048):
            copies = 8
            ids = [torch.randint(0, M, (n,), dtype=torch.int32, device="cuda") for _ in range(copies)]
            outs = [torch.empty((n, K), device="cuda") for _ in range(copies)]
            us = timed(lambda i: device.get_rows(w, ids[i % copies], out=outs[i % copies]))
            line("get_rows", f"{tname} {M}x{K}", n, us, n * (rb + K * 4), n == 1)
        w.free()
    for V in (32000, 152064, 262144):
        for rows in (1, 8):
            copies = 8
            logits = [torch.randn((rows, V), device="cuda") * 3 for _ in range(copies)]
            u = torch.rand(rows, device="cuda")
            tok = torch.zeros(rows, dtype=torch.int32, device="cuda")
            for name, k in (("argmax", 1), ("sample", 40), ("sample-k1", 1)):
                work = device.topk_work(rows, V, k)
                ids = torch.zeros((rows, k), dtype=torch.int32, device="cuda")
                probs = torch.zeros((rows, k), device="cuda")
                if name == "argmax":
                    us = timed(lambda i: device.argmax_rows(logits[i % copies], ids=tok, work=work))
                else:
                    us = timed(lambda i: device.sample_topk(logits[i % copies], k, inv_temp=1.25, top_p=0.9, u=u, ids=ids, probs=probs, token=tok, work=work))
                line(name, f"{V} logits", rows, us, rows * V * 4, rows == 1)


if __name__ == "__main__":
    main()
