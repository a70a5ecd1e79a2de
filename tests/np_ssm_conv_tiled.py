"""A numpy model of the tiled causal conv (csrc/ssm_conv_tile.hip; include/ggml_hip_ext.h, ggml_hip_ssm_conv_tiled_ragged_dev), launch by launch, over a whole
ragged batch -- with dst and x ONE array when the call is in place, so that what a later launch reads is what an earlier one left there.

    launch 1   the sequential kernel: every present sequence of 1 .. S tokens, np_ssm.conv_f32 from its slot (zeros where fresh), rows and slot written
    launch 2   the index: per long sequence its tiles of T tokens, counted from the sequence's own first row
    launch 3   the edges: per tile the d_conv - 1 rows in front of it into a staging buffer -- x rows for tile j > 0; for j = 0 the slot (zeros where
               fresh), and then the slot is written from the sequence's last d_conv - 1 rows of x
    launch 4   the tiles, in ascending order (one legal order of many): np_ssm.conv_f32 on the tile's rows with the staged rows as its window

The arithmetic is np_ssm.conv_f32's, the statement; the model only decides WHICH rows meet.  MUTANTS are the five ways to get that wrong which the kernel
file's header names; tests/test_ssm_conv_tiled.py asserts that each changes a bit of its batch."""
import numpy as np

import np_ssm

F = np.float32
MUTANTS = ("zero_halo", "halo_after_writes", "slot_after_writes", "fresh_reads_slot", "packed_tiles")
IN_PLACE_ONLY = ("halo_after_writes", "slot_after_writes")          # these two are the statement itself out of place


def present(q_start, b, n_tokens_max):
    s, e = int(q_start[b]), int(q_start[b + 1])
    return 0 <= s <= e <= n_tokens_max


def tiles_of(qs, nq, T, packed=False):
    """(first row in the sequence, tokens) of every tile of a sequence of nq rows at packed row qs"""
    if not packed:
        return [(t0, min(T, nq - t0)) for t0 in range(0, nq, T)]
    cuts = sorted({0, nq} | {r - qs for r in range((qs // T + 1) * T, qs + nq, T)})
    return [(lo, hi - lo) for lo, hi in zip(cuts[:-1], cuts[1:])]


def conv_tiled(x, w, bias, q_start, d_len, slot, pool, n_tokens_max, T, S, in_place=False, mutant=None, fill=np.nan):
    """x [rows, n_ch] f32, w [n_ch, K], bias [n_ch] or None, pool [n_slots, K - 1, n_ch] (a fresh sequence's slot may hold anything).
    -> (dst [rows, n_ch], the pool after the call); dst holds `fill` (x, in place) where nothing was written"""
    assert mutant is None or mutant in MUTANTS
    K, n_ch, n_slots = w.shape[1], w.shape[0], pool.shape[0]
    assert T >= K - 1 and S >= K - 1
    xb = np.array(x, F)
    dst = xb if in_place else np.full(xb.shape, fill, F)
    pool = np.array(pool, F)
    long_seqs = []
    for b in range(len(slot)):
        if not present(q_start, b, n_tokens_max):
            continue
        qs, nq, sl = int(q_start[b]), int(q_start[b + 1] - q_start[b]), int(slot[b])
        if nq == 0:
            continue
        if nq > S:
            long_seqs.append((b, qs, nq, sl))
            continue
        if not 0 <= sl < n_slots:
            dst[qs:qs + nq] = 0.0
            continue
        acc, win = np_ssm.conv_f32(xb[qs:qs + nq], w, bias, None if d_len[b] == 0 else pool[sl])
        dst[qs:qs + nq] = acc
        pool[sl] = win
    # the index
    tiles = [(b, qs, nq, sl, t0, n) for b, qs, nq, sl in long_seqs for t0, n in tiles_of(qs, nq, T, packed=mutant == "packed_tiles")]
    # the edges
    halo = {}
    for ci, (b, qs, nq, sl, t0, n) in enumerate(tiles):
        if not 0 <= sl < n_slots:
            continue
        if mutant == "packed_tiles":                                 # the K - 1 packed rows in front, whoever owns them (zeros in front of row 0)
            rows = np.zeros((K - 1, n_ch), F)
            lo = qs + t0 - (K - 1)
            rows[max(0, -lo):] = xb[max(lo, 0):qs + t0]
            halo[ci] = rows
        elif t0 > 0:
            halo[ci] = np.zeros((K - 1, n_ch), F) if mutant == "zero_halo" else xb[qs + t0 - (K - 1):qs + t0].copy()
        else:
            fresh = d_len[b] == 0 and mutant != "fresh_reads_slot"
            halo[ci] = np.zeros((K - 1, n_ch), F) if fresh else pool[sl].copy()
        if t0 == 0 and mutant != "slot_after_writes":
            pool[sl] = xb[qs + nq - (K - 1):qs + nq]
    # the tiles
    for ci, (b, qs, nq, sl, t0, n) in enumerate(tiles):
        lo = qs + t0
        if not 0 <= sl < n_slots:
            dst[lo:lo + n] = 0.0
            continue
        win0 = halo[ci]
        if mutant == "halo_after_writes" and t0 > 0:
            win0 = xb[lo - (K - 1):lo].copy()                        # (in place: the tile in front has written these rows)
        dst[lo:lo + n] = np_ssm.conv_f32(xb[lo:lo + n], w, bias, win0)[0]
    if mutant == "slot_after_writes":
        for b, qs, nq, sl in long_seqs:
            if 0 <= sl < n_slots:
                pool[sl] = xb[qs + nq - (K - 1):qs + nq]
    return dst, pool
