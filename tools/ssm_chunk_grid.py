#!/usr/bin/env python3
"""The chunked-scan grid (csrc/ssm_chunk.hip, ggml_hip_ssm_scan_chunked_ragged_dev) beside the sequential entry (ggml_hip_ssm_scan_ragged_dev): GPU-side time
per call on the Mamba-2 layer of tools/ssm_grid.py (64 heads of 64, d_state 128, one group), by that tool's method -- a REPLAYED graph of CALLS calls, events
around the replays, the best of 5, the slots rotating through a pool of 256 so that no call finds its state in a cache the call before filled.

    python tools/ssm_chunk_grid.py [--parent-lib PATH] > profiles/ssm_chunk_grid.txt            # on a machine with an MI355X

--parent-lib: a libggml_hip.so built from the PARENT commit; its sequential entry is timed in the same visit (the `parent` columns), which is what
seq_max_tokens and the decode rows are judged against.  Without it those columns repeat this build's sequential entry.

PREFILL: one continued sequence of 128 / 512 / 2048 / 8192 tokens.  MIXED: 64 decode sequences of one token and one prefill of 2048 in ONE call.  SWEEP: one
sequence of n tokens around seq_max_tokens (at or below it the chunked entry runs the sequential kernel: the same launch behind one more host plan).
DECODE: the SEQUENTIAL entry at 64 and 256 sequences of one token, the parent's build against this one: the token-count window must cost nothing.
flops  = the four products of the statement, C B^T once per group: chunks * (G * 2 Q Q N + H * (2 Q Q P + 2 * 2 Q P N)); roof = flops / time / 155 TF.
bytes  = 2 x the states + the rows read and written + the work buffer's traffic (S written, read and H_in written by the pass, H_in read): 4 x chunks x
         the state; hbm = bytes / time / 8 TB/s."""
import argparse
import ctypes as C
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import _lib, device  # noqa: E402
from tools.ssm_grid import N_SLOTS, timed  # noqa: E402

H, P, N, G = 64, 64, 128, 1


def old_entry(lib):
    """the sequential entry of a library, as a function with ssm_scan_ragged's tensors"""
    fn = lib.ggml_hip_ssm_scan_ragged_dev
    fn.restype, fn.argtypes = _lib.HIP_SYMBOLS["ggml_hip_ssm_scan_ragged_dev"]

    def call(x, dt, A, B, Cc, q, ln, sl, pool, D, y):
        p = lambda t: C.c_void_p(t.data_ptr())
        rc = fn(p(x), x.stride(0), x.stride(1), p(dt), dt.stride(0), None, p(A), 1, 0, p(B), p(Cc), B.stride(0), p(D), H, P, N, G, q.numel() - 1, p(q), x.shape[0],
                p(ln), p(sl), p(pool), pool.stride(0) * 4, pool.shape[0], p(y), y.stride(0), y.stride(1), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
    return call


def tensors(counts, calls):
    n, n_seq = sum(counts), len(counts)
    x = torch.rand((n, H, P), device="cuda") * 2 - 1
    dt = torch.rand((n, H), device="cuda") * 2 - 1
    A = -(torch.rand((H,), device="cuda") + 0.5)
    bc = torch.rand((n, 2 * G * N), device="cuda") * 2 - 1
    B, Cc = bc[:, :G * N].view(n, G, N), bc[:, G * N:].view(n, G, N)
    D = torch.rand((H,), device="cuda")
    q = torch.tensor([0] + list(torch.tensor(counts).cumsum(0)), dtype=torch.int32).cuda()
    ln = torch.full((n_seq,), 100, dtype=torch.int32, device="cuda")
    slots = [((torch.arange(n_seq, dtype=torch.int32) + i * n_seq) % N_SLOTS).cuda() for i in range(calls)]
    return x, dt, A, B, Cc, D, q, ln, slots, torch.empty_like(x)


def measure(counts, calls, pool, parent, this, chunked=True):
    x, dt, A, B, Cc, D, q, ln, slots, y = tensors(counts, calls)
    us_parent = timed(lambda i: parent(x, dt, A, B, Cc, q, ln, slots[i % calls], pool, D, y), calls)
    us_seq = timed(lambda i: this(x, dt, A, B, Cc, q, ln, slots[i % calls], pool, D, y), calls)
    if not chunked:
        return us_parent, us_seq, None
    n, n_seq = sum(counts), len(counts)
    work = torch.empty(max(device.ssm_scan_chunked_work_size(H, P, N, G, False, n_seq, n), 1), dtype=torch.uint8, device="cuda")
    us_new = timed(lambda i: device.ssm_scan_chunked_ragged(x, dt, A, B, Cc, q, ln, slots[i % calls], pool, D=D, out=y, work=work), calls)
    return us_parent, us_seq, us_new


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent-lib", default=None)
    args = ap.parse_args()
    device.init(0)
    this = old_entry(_lib.lib())
    parent = old_entry(C.CDLL(os.path.abspath(args.parent_lib))) if args.parent_lib else this
    pl = device.ssm_scan_chunked_plan(H, P, N, G, False, 1, 1 << 20)
    Q, smt = pl.chunk, pl.seq_max_tokens
    pool = torch.zeros((N_SLOTS, H * P * N), device="cuda")
    state = H * P * N * 4
    print(f"# us per call, GPU side: replayed graphs, the slots rotating through a pool of {N_SLOTS}; every sequence continues from its slot")
    print(f"# mamba2: {H} heads of {P}, d_state {N}, {G} group.  plan: chunk {Q}, seq_max_tokens {smt}.  parent: {'the parent build' if args.parent_lib else 'this build (no --parent-lib)'}")
    print("# roof: the four products' flops / 155 TF;  hbm: states, rows and the work buffer's traffic / 8 TB/s")
    print("batch          n_seq  tokens  parent_us    seq_us    new_us  parent/new   roof    hbm")
    sweep = sorted({16, 32, 40, 48, 56, 96, 128, 192, 256} | {smt, smt + 1, Q, Q + 1})
    rows = [("prefill", [n]) for n in (128, 512, 2048, 8192)] + [("mixed", [1] * 64 + [2048])] + [("sweep", [n]) for n in sweep]
    for name, counts in rows:
        n = sum(counts)
        us_parent, us_seq, us_new = measure(counts, 2, pool, parent, this)
        chunks = sum(-(-c // Q) for c in counts if c > smt)
        flops = chunks * (G * 2 * Q * Q * N + H * (2 * Q * Q * P + 4 * Q * P * N))
        nbytes = 2 * len(counts) * state + n * (2 * H * P + H + 2 * G * N) * 4 + 4 * chunks * state
        print(f"{name:12s} {len(counts):7d} {n:7d} {us_parent:10.2f} {us_seq:9.2f} {us_new:9.2f} {us_parent / us_new:11.2f} {flops / (us_new * 1e-6) / 155e12:6.3f} "
              f"{nbytes / (us_new * 1e-6) / 8e12:6.3f}", flush=True)
    print("# the sequential entry at decode, the parent's build against this one (the token-count window at the top of the kernel)")
    print("batch          n_seq  tokens  parent_us   this_us  this/parent")
    for n_seq in (64, 256):
        for rep in range(2):
            us_parent, us_seq, _ = measure([1] * n_seq, 8, pool, parent, this, chunked=False)
            print(f"{'decode':12s} {n_seq:7d} {n_seq:7d} {us_parent:10.2f} {us_seq:9.2f} {us_seq / us_parent:12.3f}", flush=True)


if __name__ == "__main__":
    main()
