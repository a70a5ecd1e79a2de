#!/usr/bin/env python3
"""The tiled-conv grid (csrc/ssm_conv_tile.hip, ggml_hip_ssm_conv_tiled_ragged_dev) beside the sequential entry (ggml_hip_ssm_conv_ragged_dev): GPU-side time
per call on the convs of the two layers of tools/ssm_grid.py (Mamba-2: 4352 channels; Mamba-1: 5120 channels; d_conv 4, bias and silu), by that tool's method
-- a REPLAYED graph of CALLS calls, events around the replays, the best of 5, the slots rotating through a pool of 256.

    python tools/ssm_conv_grid.py [--parent-lib PATH] [--variant-lib PATH ...] > profiles/ssm_conv_grid.txt      # on a machine with an MI355X

--parent-lib: a libggml_hip.so built from the PARENT commit; its sequential entry is timed in the same visit (the `parent` columns), which is what the
token-count window at the top of ssm_conv_kernel is judged against at decode.  Without it those columns repeat this build's sequential entry.
--variant-lib: a libggml_hip.so built from THIS tree with other SSM_CONV_TILE / SSM_CONV_SEQ_MAX_TOKENS in csrc/plan.h (nothing else follows them); each is
timed at 2048 tokens and over the sweep, which is how tile and seq_max_tokens were picked: a variant with seq_max_tokens = 3 runs every swept length tiled.

PREFILL: one continued sequence of 128 / 512 / 2048 / 8192 tokens, out of place; at 2048 also in place.  MIXED: 64 decode sequences of one token and one
prefill of 2048 in ONE call.  DECODE: 1 / 64 / 256 sequences of one token -- the tiled entry there is form 2 with nothing long: the sequential launch and
three near-empty ones, the price of one captured graph for every step.  SWEEP: one sequence of n tokens around seq_max_tokens, twice (the spread).
COPY: torch's device copy of the same rows, x -> y, timed the same way: what moving the rows once costs.
bytes = the rows read and written + 2 x the slots of the batch;  hbm = bytes / time / 8 TB/s."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import _lib, device  # noqa: E402
from tools.ssm_grid import LAYERS, N_SLOTS, timed  # noqa: E402

K = 4


def _p(t):
    return None if t is None else C.c_void_p(t.data_ptr())


class Build:
    """the conv entries of one library, as functions of tensors"""

    def __init__(self, lib):
        self.lib = lib
        for name in ("ggml_hip_ssm_conv_ragged_dev", "ggml_hip_ssm_conv_tiled_ragged_dev", "ggml_hip_ssm_conv_tiled_plan", "ggml_hip_ssm_conv_tiled_work_size"):
            if hasattr(lib, name):
                fn = getattr(lib, name)
                fn.restype, fn.argtypes = _lib.HIP_SYMBOLS[name]

    def plan(self, n_ch, n_seq, n):
        out = _lib.ggml_hip_ssm_conv_plan_t()
        assert self.lib.ggml_hip_ssm_conv_tiled_plan(n_ch, K, n_seq, n, C.byref(out)) == 0
        return out

    def work(self, n_ch, n_seq, n):
        return torch.empty(max(int(self.lib.ggml_hip_ssm_conv_tiled_work_size(n_ch, K, n_seq, n)), 1), dtype=torch.uint8, device="cuda")

    def _args(self, x, w, b, q, ln, sl, pool, y):
        return (_p(x), x.stride(0), _p(w), _p(b), 1, x.shape[1], K, q.numel() - 1, _p(q), x.shape[0], _p(ln), _p(sl), _p(pool), pool.stride(0) * 4, pool.shape[0],
                _p(y), y.stride(0))

    def old(self, x, w, b, q, ln, sl, pool, y):
        rc = self.lib.ggml_hip_ssm_conv_ragged_dev(*self._args(x, w, b, q, ln, sl, pool, y), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc

    def new(self, x, w, b, q, ln, sl, pool, y, work):
        rc = self.lib.ggml_hip_ssm_conv_tiled_ragged_dev(*self._args(x, w, b, q, ln, sl, pool, y), _p(work), work.numel(),
                                                         C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc


def tensors(n_ch, counts, calls):
    n, n_seq = sum(counts), len(counts)
    x = torch.rand((n, n_ch), device="cuda") * 2 - 1
    w = torch.rand((n_ch, K), device="cuda") - 0.5
    b = torch.rand((n_ch,), device="cuda")
    q = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).cuda()
    ln = torch.full((n_seq,), 100, dtype=torch.int32, device="cuda")
    slots = [((torch.arange(n_seq, dtype=torch.int32) + i * n_seq) % N_SLOTS).cuda() for i in range(calls)]
    return x, w, b, q, ln, slots, torch.empty_like(x)


def nbytes(n_ch, counts):
    return 2 * sum(counts) * n_ch * 4 + 2 * len(counts) * (K - 1) * n_ch * 4


def measure(build, n_ch, counts, calls, pool, which, in_place=False):
    x, w, b, q, ln, slots, y = tensors(n_ch, counts, calls)
    dst = x if in_place else y
    if which == "old":
        return timed(lambda i: build.old(x, w, b, q, ln, slots[i % calls], pool, dst), calls)
    if which == "copy":
        return timed(lambda i: y.copy_(x), calls)
    work = build.work(n_ch, len(counts), sum(counts))
    return timed(lambda i: build.new(x, w, b, q, ln, slots[i % calls], pool, dst, work), calls)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    ap.add_argument("--variant-lib", action="append", default=[])
    args = ap.parse_args()
    device.init(0)
    this = Build(_lib.lib())
    parent = Build(C.CDLL(os.path.abspath(args.parent_lib))) if args.parent_lib else this
    variants = [(os.path.basename(p), Build(C.CDLL(os.path.abspath(p)))) for p in args.variant_lib]
    pl = this.plan(4352, 1, 1 << 20)
    T, S = pl.tile, pl.seq_max_tokens
    print(f"# us per call, GPU side: replayed graphs, the slots rotating through a pool of {N_SLOTS}; every sequence continues from its slot; d_conv {K}, bias, silu")
    print(f"# plan: tile {T}, seq_max_tokens {S}.  parent: {'the parent build' if args.parent_lib else 'this build (no --parent-lib)'}")
    print("# old: ggml_hip_ssm_conv_ragged_dev; new: ggml_hip_ssm_conv_tiled_ragged_dev; copy: a device copy of the rows; hbm: rows in and out + slots / new / 8 TB/s")
    sweep = sorted({4, 8, 12, 16, 24, 32, 48, 64, 96, 112, 120, 128, 144, 160, 192, 256, 384, 512} | {S, S + 1})
    for lname, L in LAYERS:
        n_ch = L["n_ch"]
        pool = torch.zeros((N_SLOTS, (K - 1) * n_ch), device="cuda")
        print(f"layer {lname}: {n_ch} channels")
        print("batch           n_seq  tokens    old_us    new_us   copy_us  old/new  new/copy    hbm")
        rows = [("prefill", [n], False) for n in (128, 512, 2048, 8192)] + [("prefill_inplace", [2048], True), ("mixed", [1] * 64 + [2048], False)]
        rows += [("decode", [1] * n_seq, False) for n_seq in (1, 64, 256)]
        rows += [("sweep", [n], False) for n in sweep for _ in range(2)]
        for name, counts, in_place in rows:
            calls = 8 if name == "decode" else 2
            us_old = measure(this, n_ch, counts, calls, pool, "old", in_place)
            us_new = measure(this, n_ch, counts, calls, pool, "new", in_place)
            us_copy = measure(this, n_ch, counts, calls, pool, "copy")
            print(f"{name:15s} {len(counts):5d} {sum(counts):7d} {us_old:9.2f} {us_new:9.2f} {us_copy:9.2f} {us_old / us_new:8.2f} {us_new / us_copy:9.2f} "
                  f"{nbytes(n_ch, counts) / (us_new * 1e-6) / 8e12:6.3f}", flush=True)
        print("# the sequential entry at decode, the parent's build against this one (the token-count window at the top of the kernel)")
        print("batch           n_seq  parent_us   this_us  this/parent")
        for n_seq in (64, 256):
            for rep in range(2):
                us_parent = measure(parent, n_ch, [1] * n_seq, 8, pool, "old")
                us_this = measure(this, n_ch, [1] * n_seq, 8, pool, "old")
                print(f"{'decode':15s} {n_seq:5d} {us_parent:10.2f} {us_this:9.2f} {us_this / us_parent:12.3f}", flush=True)
        if variants:
            print("# builds with other constants in plan.h: the tiled entry, one sequence of n tokens")
            print("variant                  tile  seq_max   " + " ".join(f"{n:>8d}" for n in [2048] + sweep))
            for vname, v in [("this", this)] + variants:
                vp = v.plan(n_ch, 1, 1 << 20)
                us = [measure(v, n_ch, [n], 2, pool, "new") for n in [2048] + sweep]
                print(f"{vname:24s} {vp.tile:4d} {vp.seq_max_tokens:8d}   " + " ".join(f"{u:8.2f}" for u in us), flush=True)
            print(f"{'(old entry)':24s} {'':4s} {'':8s}   " + " ".join(f"{measure(this, n_ch, [n], 2, pool, 'old'):8.2f}" for n in [2048] + sweep), flush=True)


if __name__ == "__main__":
    main()
