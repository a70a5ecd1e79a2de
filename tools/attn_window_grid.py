#!/usr/bin/env python3
"""The windowed attention grid (csrc/attn.hip, ggml_hip_attn_ex_dev / ggml_hip_attn_paged_ex_dev): GPU-side time per call of a sliding-window
call against the base entry at the same cache length, and against the base entry on a cache of W positions -- the floor a windowed call can
hope for, since it reads no more than that.

    python tools/attn_window_grid.py > attn_window_grid.txt            # measure, on a machine with an MI355X

32 heads over 8 kv heads, D = 128, causal.  Timed like tools/attn_grid.py: a REPLAYED graph of 32 calls rotating over cache copies (past the
Infinity Cache where the cache is small), events around the replays, the best of 5.  The base entries are measured BEFORE and AFTER the
windowed side in the same process: the difference of the two figures is the spread a ratio has to be read against."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

F16, Q8_0 = 1, 8
N_HEAD, N_HEAD_KV, D = 32, 8, 128
CALLS, REPLAYS = 32, 5
PAGE = 128


def timed(run):
    """us per call of run(i): captured as CALLS calls, replayed REPLAYS times, the best"""
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


class Contiguous:
    """cache copies of n_kv positions and the calls over them"""

    def __init__(self, kv_type, n_q, n_kv):
        rb = device.kv_row_bytes(kv_type, D)
        self.kv_type, self.n_q, self.n_kv, self.nb_head, self.nb_pos = kv_type, n_q, n_kv, rb, N_HEAD_KV * rb
        cache_bytes = n_kv * self.nb_pos
        self.copies = max(1, min(8, (600 << 20) // (2 * cache_bytes)))
        src = torch.rand((n_kv, N_HEAD_KV * D), device="cuda") * 2 - 1
        self.caches = []
        for _ in range(self.copies):
            k = torch.empty(cache_bytes, dtype=torch.uint8, device="cuda")
            v = torch.empty(cache_bytes, dtype=torch.uint8, device="cuda")
            device.kv_store(kv_type, src, k, self.nb_pos, n_kv)
            device.kv_store(kv_type, src.flip(0), v, self.nb_pos, n_kv)
            self.caches.append((k, v))
        self.q = torch.rand((n_q, N_HEAD, D), device="cuda") * 2 - 1
        self.out = torch.empty_like(self.q)
        self.work = torch.empty(max(device.attn_work_size(kv_type, D, N_HEAD, N_HEAD_KV, n_q, n_kv), 16), dtype=torch.uint8, device="cuda")

    def us(self, window=0):
        def run(i):
            k, v = self.caches[i % self.copies]
            device.attention(self.kv_type, self.q, k, v, self.nb_pos, self.nb_head, N_HEAD_KV, self.n_kv, out=self.out, work=self.work, window=window)
        return timed(run)


class Paged:
    """pool copies for n_seq sequences of n_kv positions each (identity tables) and the paged calls over them"""

    def __init__(self, kv_type, n_seq, n_kv):
        rb = device.kv_row_bytes(kv_type, D)
        nb_head, nb_pos = rb, N_HEAD_KV * rb
        nb_page = PAGE * nb_pos
        per_seq = n_kv // PAGE
        n_pages = n_seq * per_seq
        pool_bytes = n_pages * nb_page
        self.copies = max(1, min(8, (600 << 20) // (2 * pool_bytes)))
        src = torch.rand((n_pages * PAGE, N_HEAD_KV * D), device="cuda") * 2 - 1
        pages = torch.arange(n_pages, dtype=torch.int32, device="cuda").reshape(n_seq, per_seq)
        d_len = torch.full((n_seq,), n_kv, dtype=torch.int32, device="cuda")
        self.pcs = []
        for _ in range(self.copies):
            k = torch.empty(pool_bytes, dtype=torch.uint8, device="cuda")
            v = torch.empty(pool_bytes, dtype=torch.uint8, device="cuda")
            device.kv_store(kv_type, src, k, nb_pos, n_pages * PAGE)            # (pages back to back: the pool is one contiguous cache)
            device.kv_store(kv_type, src.flip(0), v, nb_pos, n_pages * PAGE)
            self.pcs.append(device.PagedCache(kv_type, k, v, nb_page, nb_pos, nb_head, n_pages, pages, d_len, n_kv))
        self.q = torch.rand((n_seq, N_HEAD, D), device="cuda") * 2 - 1
        self.out = torch.empty_like(self.q)
        self.work = torch.empty(max(device.attn_paged_work_size(kv_type, D, N_HEAD, N_HEAD_KV, n_seq, 1, n_kv), 16), dtype=torch.uint8, device="cuda")

    def us(self, window=0):
        return timed(lambda i: device.attn_paged(self.pcs[i % self.copies], self.q, N_HEAD_KV, out=self.out, work=self.work, window=window))


def main():
    device.init(0)
    print("# us per call, GPU side: replayed graphs of 32 calls rotating over cache copies; 32 heads over 8 kv heads, D = 128, causal")
    print("# base / base2: the base entry at the same n_kv before and after the windowed side; floor / floor2: the base entry on a cache of W positions")
    print("# (PROMPT: n_q = n_kv = W), likewise; win: the _ex entry with window W; chunks: the windowed DECODE grid per kv head (and sequence) against the base grid")
    print("form    type  n_seq   n_q    n_kv      W   chunks      base     base2     floor    floor2       win  win/base  win/floor")
    windows = (128, 1024, 4096)
    for kv_type, name in ((F16, "f16"), (Q8_0, "q8_0")):
        for n_kv in (8192, 32768):
            full = Contiguous(kv_type, 1, n_kv)
            floors = {W: Contiguous(kv_type, 1, W) for W in windows}
            base = full.us()
            floor = {W: floors[W].us() for W in windows}
            win = {W: full.us(W) for W in windows}
            base2 = full.us()
            for W in windows:
                floor2 = floors[W].us()
                pl = device.attn_ex_plan(kv_type, D, N_HEAD, N_HEAD_KV, 1, n_kv, window=W)
                print(f"decode  {name:5s} {1:5d} {1:5d} {n_kv:7d} {W:6d} {pl.n_chunks:3d}/{n_kv // PAGE:<4d} {base:9.1f} {base2:9.1f} {floor[W]:9.1f} {floor2:9.1f} "
                      f"{win[W]:9.1f} {win[W] / min(base, base2):9.3f} {win[W] / min(floor[W], floor2):10.3f}", flush=True)
            del full, floors
        n, W = 2048, 512
        full, small = Contiguous(kv_type, n, n), Contiguous(kv_type, W, W)
        base, floor = full.us(), small.us()
        win = full.us(W)
        base2, floor2 = full.us(), small.us()
        print(f"prompt  {name:5s} {1:5d} {n:5d} {n:7d} {W:6d}    -     {base:9.1f} {base2:9.1f} {floor:9.1f} {floor2:9.1f} {win:9.1f} {win / min(base, base2):9.3f} "
              f"{win / min(floor, floor2):10.3f}", flush=True)
        del full, small
        n_seq, n_kv, W = 8, 8192, 1024
        full, small = Paged(kv_type, n_seq, n_kv), Paged(kv_type, n_seq, W)
        base, floor = full.us(), small.us()
        win = full.us(W)
        base2, floor2 = full.us(), small.us()
        pl = device.attn_paged_ex_plan(kv_type, D, N_HEAD, N_HEAD_KV, n_seq, 1, n_kv, window=W)
        print(f"paged   {name:5s} {n_seq:5d} {1:5d} {n_kv:7d} {W:6d} {pl.n_chunks:3d}/{n_kv // PAGE:<4d} {base:9.1f} {base2:9.1f} {floor:9.1f} {floor2:9.1f} {win:9.1f} "
              f"{win / min(base, base2):9.3f} {win / min(floor, floor2):10.3f}", flush=True)
        del full, small


if __name__ == "__main__":
    main()
