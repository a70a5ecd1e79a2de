#!/usr/bin/env python3
"""The SSM grid (csrc/ssm.hip, ggml_hip_ssm_scan_ragged_dev / ggml_hip_ssm_conv_ragged_dev): GPU-side time per call beside the bytes the call must move.

    python tools/ssm_grid.py > profiles/ssm_grid.txt            # measure, on a machine with an MI355X

Two layers: a Mamba-2 layer (64 heads of 64, d_state 128, one group: a 2 MiB state per sequence; its conv has 4096 + 2 * 128 channels, d_conv 4) and a
Mamba-1 layer (d_inner 5120 as 5120 heads of 1, d_state 16, A per state).  Batches: DECODE, one token for each of 1 / 64 / 256 sequences, and PREFILL, one
sequence of 512 / 2048 tokens; every sequence continues from its slot (d_len > 0), so the state is read and written.
Timed as tools/rope_grid.py times: a REPLAYED graph of CALLS calls, events around the replays, the best of 5.  The pool has 256 slots (512 MiB for the
Mamba-2 scan, beyond the 256 MiB Infinity Cache) and call i of a graph uses the slots (i * n_seq + b) % 256, so a decode call does not find its state in
a cache the previous call filled.
bytes = 2 x the states of the batch (read once, written once) + the rows read (x, dt, B, C; the conv: x) and written (y);  roof = bytes / time / 8 TB/s."""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from ggmlsharp_amd import device  # noqa: E402

N_SLOTS, REPLAYS = 256, 5
LAYERS = (("mamba2", dict(H=64, P=64, N=128, G=1, aps=False, n_ch=64 * 64 + 2 * 128, d_conv=4)),
          ("mamba1", dict(H=5120, P=1, N=16, G=1, aps=True, n_ch=5120, d_conv=4)))
BATCHES = (("decode", 1, 1), ("decode", 64, 1), ("decode", 256, 1), ("prefill", 1, 512), ("prefill", 1, 2048))


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
    best = float("inf")
    for _ in range(REPLAYS):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        g.replay()
        e1.record()
        torch.cuda.synchronize()
        best = min(best, e0.elapsed_time(e1) * 1000.0 / calls)
    return best


def batch_tensors(n_seq, n_q, calls):
    q_start = (torch.arange(n_seq + 1, dtype=torch.int32) * n_q).cuda()
    d_len = torch.full((n_seq,), 100, dtype=torch.int32, device="cuda")
    slots = [((torch.arange(n_seq, dtype=torch.int32) + i * n_seq) % N_SLOTS).cuda() for i in range(calls)]
    return q_start, d_len, slots


def measure_scan(L, n_seq, n_q, calls):
    H, P, N, G = L["H"], L["P"], L["N"], L["G"]
    n = n_seq * n_q
    pool = torch.zeros((N_SLOTS, H * P * N), device="cuda")
    x = torch.rand((n, H, P), device="cuda") * 2 - 1
    dt = torch.rand((n, H), device="cuda") * 2 - 1
    A = -(torch.rand((H, N) if L["aps"] else (H,), device="cuda") + 0.5)
    bc = torch.rand((n, 2 * G * N), device="cuda") * 2 - 1
    B, C = bc[:, :G * N].view(n, G, N), bc[:, G * N:].view(n, G, N)
    D = torch.rand((H,), device="cuda")
    y = torch.empty_like(x)
    q_start, d_len, slots = batch_tensors(n_seq, n_q, calls)
    us = timed(lambda i: device.ssm_scan_ragged(x, dt, A, B, C, q_start, d_len, slots[i % calls], pool, D=D, out=y), calls)
    nbytes = 2 * n_seq * H * P * N * 4 + n * (2 * H * P + H + 2 * G * N) * 4
    return us, nbytes


def measure_conv(L, n_seq, n_q, calls):
    n_ch, K = L["n_ch"], L["d_conv"]
    n = n_seq * n_q
    pool = torch.zeros((N_SLOTS, (K - 1) * n_ch), device="cuda")
    x = torch.rand((n, n_ch), device="cuda") * 2 - 1
    w = torch.rand((n_ch, K), device="cuda") - 0.5
    b = torch.rand((n_ch,), device="cuda")
    y = torch.empty_like(x)
    q_start, d_len, slots = batch_tensors(n_seq, n_q, calls)
    us = timed(lambda i: device.ssm_conv_ragged(x, w, q_start, d_len, slots[i % calls], pool, bias=b, act=True, out=y), calls)
    nbytes = 2 * n_seq * (K - 1) * n_ch * 4 + 2 * n * n_ch * 4
    return us, nbytes


def main():
    device.init(0)
    print("# us per call, GPU side: replayed graphs, the slots rotating through a pool of 256; every sequence continues from its slot")
    print("# mamba2: 64 heads of 64, d_state 128, 1 group (conv: 4352 channels, d_conv 4).  mamba1: 5120 heads of 1, d_state 16, A per state (conv: 5120 channels)")
    print("# bytes: 2 x the states + the rows read and written;  roof: fraction of 8 TB/s for those bytes")
    print("entry  layer   batch    n_seq  n_q        us      MiB   roof")
    for lname, L in LAYERS:
        for bname, n_seq, n_q in BATCHES:
            calls = 8 if bname == "decode" else 2
            for ename, fn in (("scan", measure_scan), ("conv", measure_conv)):
                us, nbytes = fn(L, n_seq, n_q, calls)
                print(f"{ename:6s} {lname:7s} {bname:8s} {n_seq:5d} {n_q:4d} {us:9.2f} {nbytes / 2 ** 20:8.2f} {nbytes / (us * 1e-6) / 8e12:6.3f}", flush=True)


if __name__ == "__main__":
    main()
