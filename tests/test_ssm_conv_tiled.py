"""The tiled causal conv (include/ggml_hip_ext.h: ggml_hip_ssm_conv_tiled_ragged_dev, _plan, _work_size; csrc/ssm_conv_tile.hip, ssm.cpp, plan.cpp).

The conv's statement is a fixed fma chain per token, so the token-parallel form owes the SAME BITS as the sequential one: every comparison here is on uint32.
Yardsticks, all older than the form: np_ssm.conv_f32 (the statement), np_ssm.silu64 (act = 1: 3 * 2^-24 relative of the silu of the statement's bits), and
the sequential entry ggml_hip_ssm_conv_ragged_dev called on the same batch.

ONE ragged batch, built from the plan's tile T and seq_max_tokens S (never written here): counts 0, 1, S, S + 1, 2 T, 2 T + 1, 2 T + 2 and 2 T + T / 2 + 3,
and -- since the measured S is above 2 T, where those run sequential -- the same four from M, the first multiple of T above S: long sequences of whole tiles,
with last tiles of 1 and 2 tokens (shorter than d_conv - 1) and with a partial tail; a long sequence directly behind a long one, a short one between two long ones; a sequence that ends beyond n_tokens_max
and one with reversed bounds (both absent; the rows between them and the next sequence belong to nobody); slot ids -1 and n_slots, one long and one short;
fresh sequences over NaN-byte slots and continued ones in both forms; rows nobody owns in the middle and at the end, holding 3.0e38; an n_tokens_max that is
no multiple of T.  tests/np_ssm_conv_tiled.py models the form launch by launch and names five mutants; each changes a bit of THIS batch."""
import ctypes as C
import fnmatch
import functools
import os
import re

import numpy as np
import pytest

import np_ssm
import np_ssm_conv_tiled as npt
import test_ssm as ts
from ggmlsharp_amd import _lib

ROOT = ts.ROOT
NEW_SYMBOLS = ("ggml_hip_ssm_conv_tiled_ragged_dev", "ggml_hip_ssm_conv_tiled_plan", "ggml_hip_ssm_conv_tiled_work_size")
SENTINEL, NAN_BYTES, GUARD, FAKE = ts.SENTINEL, ts.NAN_BYTES, ts.GUARD, ts.FAKE
OK, ERR_SHAPE, ERR_ARG = ts.OK, ts.ERR_SHAPE, ts.ERR_ARG
F, U = np.float32, np_ssm.U
_p, _up, _bits, _stream, Pool = ts._p, ts._up, ts._bits, ts._stream, ts.Pool
dev = ts.dev
WORK_GUARD = 256                                                     # bytes in front of and behind the work buffer

# (name, n_ch, what pushes a 4-channel-eligible n_ch onto the 1-channel path): the paddings of x and dst follow in _pads
SHAPES = {
    "c1": (1, None), "c5": (5, None),                                # the 1-channel path
    "c64": (64, None),                                               # the 4-channel path, under one workgroup
    "c1028": (1028, None),                                           # the 4-channel path, two workgroups, the second holds one thread
    "c64_odd_ldx": (64, "ldx"),                                      # 1-channel: ldx no multiple of 4
    "c64_shifted": (64, "ptr"),                                      # 1-channel: d_x 4 bytes off a 16-byte boundary
}
D_CONVS = (2, 3, 4)


def _plan(n_ch, d_conv, n_seq, n_tokens_max):
    out = _lib.ggml_hip_ssm_conv_plan_t()
    rc = _lib.lib().ggml_hip_ssm_conv_tiled_plan(n_ch, d_conv, n_seq, n_tokens_max, C.byref(out))
    return rc, out


def _work_size(n_ch, d_conv, n_seq, n_tokens_max):
    return int(_lib.lib().ggml_hip_ssm_conv_tiled_work_size(n_ch, d_conv, n_seq, n_tokens_max))


def _fields(p):
    return tuple(int(getattr(p, f)) for f, _ in _lib.ggml_hip_ssm_conv_plan_t._fields_)


@functools.lru_cache(maxsize=None)
def _t_and_s():
    """T and seq_max_tokens of the plan; the same for every shape, which test_the_batch_is_what_it_says asserts"""
    rc, p = _plan(64, 4, 1, 1 << 20)
    assert rc == OK and p.form == 2
    return int(p.tile), int(p.seq_max_tokens)


# ---------------------------------------------------------------- the batch, built from the plan's T and seq_max_tokens
@functools.lru_cache(maxsize=None)
def batch():
    """M is the smallest count of at least 2 T that is a multiple of T and long (above S): M = 2 T where S < 2 T, and then the four counts M, M + 1,
    M + 2, M + T / 2 + 3 ARE 2 T, 2 T + 1, 2 T + 2, 2 T + T / 2 + 3.  Where the measured S is larger those four literal counts run sequential, and the
    batch holds them too (sequences 13 .. 16), so that both readings of "2 T + 1" are here: that count, and a long sequence whose last tile has one token"""
    T, S = _t_and_s()
    M = max(2 * T, -(-(S + 1) // T) * T)
    #         0               1      2  3  (4, 5: absent)  6  7  8      9      10     11 12
    counts = [M + T // 2 + 3, M + 1, S, M, None, None, 0, 1, M + 2, S + 1, S + 2, 2, 3]
    slot = [7, 2, 5, 0, 9, 12, 4, 11, 1, 13, -1, None, 3]
    d_len = [4, 0, 3, 0, 5, 2, 6, 0, 9, 0, 1, 2, 7]
    if M != 2 * T:
        counts += [2 * T, 2 * T + 1, 2 * T + 2, 2 * T + T // 2 + 3]
        slot += [6, 8, 10, 14]
        d_len += [0, 2, 0, 8]
    n_slots = 15
    slot = np.array([n_slots if v is None else v for v in slot], np.int32)
    d_len = np.array(d_len, np.int32)
    q = [0]
    for b, n in enumerate(counts):
        if b == 4:
            gap = q[-1]
            q.append(None)                                          # 4 = [gap, beyond n_tokens_max), 5 = [beyond, gap + 2): reversed
        elif b == 5:
            q.append(gap + 2)
        else:
            q.append(q[-1] + n)
    tail = 3 if (q[-1] + 3) % T else 4
    n_tokens_max = q[-1] + tail
    q[5] = n_tokens_max + 7
    n_seq = len(counts)
    k = ts.Batch(n_tokens_max, np.array(q, np.int32), d_len, slot, tuple(b for b in range(n_seq) if counts[b] and 0 <= slot[b] < n_slots),
                 tuple(b for b in range(n_seq) if counts[b] and not 0 <= slot[b] < n_slots))
    k.counts, k.n_slots, k.T, k.S, k.M, k.gap, k.tail = counts, n_slots, T, S, M, gap, tail
    k.long = tuple(b for b in k.served if counts[b] > S)
    k.short = tuple(b for b in k.served if counts[b] <= S)
    return k


def test_the_batch_is_what_it_says():
    k = batch()
    T, S, M, q, n = k.T, k.S, k.M, k.q_start, k.n_tokens_max
    for n_ch, _ in SHAPES.values():
        for K in D_CONVS:
            rc, p = _plan(n_ch, K, k.n_seq, n)
            assert rc == OK and (p.form, p.tile, p.seq_max_tokens) == (2, T, S)
    assert M % T == 0 and M >= 2 * T and S < M <= max(2 * T, S + T)
    extra = list(range(13, k.n_seq))
    assert extra == ([] if M == 2 * T else [13, 14, 15, 16])
    present = [b for b in range(k.n_seq) if 0 <= q[b] <= q[b + 1] <= n]
    assert present == [0, 1, 2, 3, 6, 7, 8, 9, 10, 11, 12] + extra
    got = [int(q[b + 1] - q[b]) for b in present]
    assert got == [M + T // 2 + 3, M + 1, S, M, 0, 1, M + 2, S + 1, S + 2, 2, 3] + [2 * T, 2 * T + 1, 2 * T + 2, 2 * T + T // 2 + 3][:len(extra)]
    assert set(got) >= {0, 1, S, S + 1, 2 * T, 2 * T + 1, 2 * T + 2, 2 * T + T // 2 + 3}
    assert 0 <= q[4] <= q[5] and q[5] > n                            # 4: ends beyond n_tokens_max
    assert q[5] > q[6] and 0 <= q[6]                                 # 5: reversed bounds
    assert all(k.d_len[b] > 0 and 0 <= k.slot[b] < k.n_slots for b in (4, 5, 6))   # (absent and idle: slots of their own, which must stay)
    assert k.served == tuple([0, 1, 2, 3, 7, 8, 9, 12] + extra)
    assert len({int(k.slot[b]) for b in range(k.n_seq) if 0 <= k.slot[b] < k.n_slots}) == 11 + len(extra) <= k.n_slots
    assert k.zeroed == (10, 11) and [int(k.slot[b]) for b in k.zeroed] == [-1, k.n_slots] and k.counts[10] > S >= k.counts[11]
    assert k.long == (0, 1, 3, 8, 9) and k.short == tuple([2, 7, 12] + extra)
    for group in (k.long, k.short):                                  # fresh and continued in both forms
        assert {bool(k.d_len[b]) for b in group} == {False, True}, group
    assert k.counts[0] > S and k.counts[1] > S and q[1] == q[0] + k.counts[0]      # a long sequence directly behind a long one
    assert k.counts[2] <= S < k.counts[3] and q[3] == q[2] + k.counts[2] and q[2] == q[1] + k.counts[1]   # a short one between two long ones
    assert [k.counts[b] % T for b in (3, 1, 8)] == [0, 1, 2]         # long: whole tiles; last tiles of 1 and 2 tokens, shorter than d_conv - 1 = 3, and 2
    assert k.counts[0] > 2 * T and k.counts[0] % T == T // 2 + 3
    owned = np.zeros(n, bool)
    for b in k.served + k.zeroed:
        assert not owned[q[b]:q[b + 1]].any()
        owned[q[b]:q[b + 1]] = True
    free = list(np.flatnonzero(~owned))
    assert free == [k.gap, k.gap + 1] + list(range(n - k.tail, n)) and 0 < k.gap < n - k.tail - 2
    assert n % T != 0 and 100 <= n <= 2000
    rc, p = _plan(64, 4, k.n_seq, n)
    assert len(k.long) + 1 <= p.seqs_max and sum(-(-k.counts[b] // T) for b in k.long + (10,)) <= p.tiles_max


# ---------------------------------------------------------------- the inputs and references, computed once
@functools.lru_cache(maxsize=None)
def case(n_ch, d_conv):
    k = batch()
    rng = np.random.default_rng(5000 + 10 * n_ch + d_conv)
    c = dict(n_ch=n_ch, d_conv=d_conv)
    c["x"] = rng.normal(0.0, 1.0, (k.n_tokens_max, n_ch)).astype(F)
    owned = np.zeros(k.n_tokens_max, bool)
    for b in k.served + k.zeroed:
        owned[k.q_start[b]:k.q_start[b + 1]] = True
    c["x"][~owned] = F(3.0e38)                                       # rows nobody owns
    c["w"] = rng.normal(0.0, 0.7, (n_ch, d_conv)).astype(F)
    c["bias"] = rng.normal(0.0, 0.5, n_ch).astype(F)
    c["pool"] = rng.normal(0.0, 1.0, (k.n_slots, d_conv - 1, n_ch)).astype(F)
    c["owned"] = owned
    return c


@functools.lru_cache(maxsize=None)
def statement(n_ch, d_conv, b, bias):
    """(rows, new slot) of sequence b of the batch: np_ssm.conv_f32"""
    k, c = batch(), case(n_ch, d_conv)
    lo, hi = k.rows(b)
    return np_ssm.conv_f32(c["x"][lo:hi], c["w"], c["bias"] if bias else None, None if k.d_len[b] == 0 else c["pool"][k.slot[b]])


def _model_pool(c, k):
    """the pool the model sees: NaN in the slots of the fresh sequences"""
    pool = c["pool"].copy()
    for b in range(k.n_seq):
        if k.d_len[b] == 0 and 0 <= k.slot[b] < k.n_slots:
            pool[k.slot[b]] = np.nan
    return pool


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "ggmlsharp_amd", "csrc", "exports.map")).read(), flags=re.S)
    pats = re.search(r"global:([^;]*);", exports).group(1).split()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), name
    assert "ggml_hip_ssm_conv_plan_t" in hdr and "ggml_hip_ssm_conv_plan_t" in cs and C.sizeof(_lib.ggml_hip_ssm_conv_plan_t) == 48
    from ggmlsharp_amd import device
    for name in ("ssm_conv_tiled_plan", "ssm_conv_tiled_work_size", "ssm_conv_tiled_ragged"):
        assert callable(getattr(device, name)), name


def test_the_plan_and_the_work_size_are_functions_of_their_arguments():
    T, S = _t_and_s()
    seen = {}
    args = [(n_ch, K, n_seq, n) for n_ch in (1, 5, 64, 1028, 4352) for K in D_CONVS for n_seq in (1, 9, 4096) for n in (0, 1, S, S + 1, 2 * T + 1, 2048, 1 << 20)]
    for rep in range(2):
        for a in args if rep == 0 else reversed(args):
            rc, p = _plan(*a)
            assert rc == OK
            f = _fields(p)
            assert seen.setdefault(a, f) == f
            assert p.work_bytes == _work_size(*a)
            n_ch, K, n_seq, n = a
            assert (p.tile, p.seq_max_tokens, p.vec, p.reserved) == (T, S, 4 if n_ch % 4 == 0 else 1, 0)      # the shape alone, never the batch
            if n <= S:
                assert (p.form, p.launches, p.tiles_max, p.seqs_max, p.work_bytes) == (1, 1, 0, 0, 0)
            else:
                assert (p.form, p.launches) == (2, 4) and p.work_bytes > 0
                assert p.seqs_max == min(n_seq, n // (S + 1)) and p.tiles_max == p.seqs_max + (n - p.seqs_max) // T
                assert p.work_bytes >= 16 + 8 * p.tiles_max + p.tiles_max * (K - 1) * n_ch * 4
    # the invariants plan.h states
    assert T >= max(D_CONVS) - 1 and S >= max(D_CONVS) - 1
    # monotone in n_seq and in n_tokens_max
    for n_ch, K in ((5, 2), (4352, 4)):
        for n_seq in (1, 2, 64, 4096):
            sizes = [_work_size(n_ch, K, n_seq, n) for n in range(0, 40 * T, 7)]
            assert sizes == sorted(sizes)
        for n in (S + 1, 2048, 100000):
            sizes = [_work_size(n_ch, K, n_seq, n) for n_seq in (1, 2, 3, 8, 100, 4096)]
            assert sizes == sorted(sizes)
    # refused shapes: the plan says so, the size is 0
    for bad in ((0, 4, 1, 64), ((1 << 24) + 1, 4, 1, 64), (64, 1, 1, 64), (64, 5, 1, 64), (64, 4, 0, 64), (64, 4, 4097, 64), (64, 4, 1, -1), (64, 4, 1, (1 << 20) + 1)):
        assert _plan(*bad)[0] == ERR_SHAPE and _work_size(*bad) == 0, bad
    assert _lib.lib().ggml_hip_ssm_conv_tiled_plan(64, 4, 1, 64, None) == ERR_ARG


def test_tiles_max_and_seqs_max_bound_random_batches():
    T, S = _t_and_s()
    rng = np.random.default_rng(99)
    for _ in range(2000):
        n_seq = int(rng.integers(1, 40))
        n = int(rng.integers(S + 1, 60 * T))
        # a valid batch: counts that fit in n rows, a random share of them long
        counts, left = [], n
        for b in range(n_seq):
            c = int(rng.choice([0, 1, int(rng.integers(1, S + 1)), S + 1, int(rng.integers(S + 1, 4 * T + S)), T, 2 * T, 2 * T + 1]))
            c = min(c, left)
            counts.append(c)
            left -= c
        if rng.integers(0, 4) == 0 and left:                         # everything that is left in one sequence
            counts[int(rng.integers(0, n_seq))] += left
        rc, p = _plan(int(rng.choice([1, 64, 4352])), int(rng.choice(D_CONVS)), n_seq, n)
        assert rc == OK and p.form == 2
        long = [c for c in counts if c > S]
        assert len(long) <= p.seqs_max and sum(-(-c // T) for c in long) <= p.tiles_max, (counts, n)


def _rc(**kw):
    """one call on pointers that are no device memory; every caller changes at least one argument into something a host check refuses"""
    assert kw
    a = dict(x=FAKE, ldx=64, w=FAKE, bias=None, act=0, n_ch=64, d_conv=4, n_seq=3, q_start=FAKE, n_tokens_max=400, len=FAKE, slot=FAKE, state=FAKE,
             nb_slot=3 * 64 * 4, n_slots=4, dst=FAKE, ldd=64, work=FAKE, work_bytes=None)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = 1 << 40
    return _lib.lib().ggml_hip_ssm_conv_tiled_ragged_dev(_p(a["x"]), a["ldx"], _p(a["w"]), _p(a["bias"]), a["act"], a["n_ch"], a["d_conv"], a["n_seq"],
                                                         _p(a["q_start"]), a["n_tokens_max"], _p(a["len"]), _p(a["slot"]), _p(a["state"]), a["nb_slot"],
                                                         a["n_slots"], _p(a["dst"]), a["ldd"], _p(a["work"]), a["work_bytes"], None)


def test_refusals_need_no_device():
    """(every call below is refused by a host check: its pointers are no device memory, so none may get as far as a launch)"""
    rc = _rc
    ts._batch_refusals(rc, 3 * 64 * 4)
    assert rc(n_ch=0, ldx=64) == ERR_SHAPE
    assert rc(n_ch=(1 << 24) + 1, ldx=1 << 25, ldd=1 << 25, nb_slot=1 << 28) == ERR_SHAPE
    for d_conv in (1, 5, 0, -2):
        assert rc(d_conv=d_conv) == ERR_SHAPE, d_conv
    for act in (2, -1):
        assert rc(act=act) == ERR_ARG, act
    assert rc(ldx=63) == ERR_SHAPE
    assert rc(ldd=63) == ERR_SHAPE
    assert rc(x=None) == ERR_ARG
    assert rc(w=None) == ERR_ARG
    assert rc(dst=None) == ERR_ARG
    assert rc(x=FAKE + 2) == ERR_SHAPE
    assert rc(w=FAKE + 1) == ERR_SHAPE
    assert rc(bias=FAKE + 2) == ERR_SHAPE
    assert rc(dst=FAKE + 3) == ERR_SHAPE
    assert rc(d_conv=2, nb_slot=64 * 4 - 16) == ERR_SHAPE
    # the work buffer's: a size below the work size, a null buffer where one is needed; where none is needed both are accepted -- shown with
    # n_tokens_max = 0, which returns 0 after every other check and before a device is touched
    need = _work_size(64, 4, 3, 400)
    assert need > 0
    assert rc(work_bytes=need - 1) == ERR_ARG
    assert rc(work=None) == ERR_ARG
    assert rc(work=None, work_bytes=0) == ERR_ARG
    assert _work_size(64, 4, 3, 0) == 0 and rc(n_tokens_max=0, work=None, work_bytes=0) == OK
    assert rc(n_tokens_max=0, act=3) == ERR_ARG                      # (after every other check: the others still refuse)


@pytest.mark.parametrize("d_conv", D_CONVS)
@pytest.mark.parametrize("n_ch", (1, 5))
@pytest.mark.parametrize("in_place", (False, True))
def test_the_model_of_the_form_is_the_statement(n_ch, d_conv, in_place):
    """per-sequence tiles, a staged window and a slot written from the inputs reproduce conv_f32 on the batch, in place and out of place"""
    k, c = batch(), case(n_ch, d_conv)
    dst, pool = npt.conv_tiled(c["x"], c["w"], c["bias"], k.q_start, k.d_len, k.slot, _model_pool(c, k), k.n_tokens_max, k.T, k.S, in_place=in_place)
    for b in k.served:
        lo, hi = k.rows(b)
        rows, slot = statement(n_ch, d_conv, b, True)
        assert np.array_equal(dst[lo:hi].view(np.uint32), rows.view(np.uint32)), b
        assert np.array_equal(pool[k.slot[b]].view(np.uint32), slot.view(np.uint32)), b
    for b in k.zeroed:
        lo, hi = k.rows(b)
        assert not dst[lo:hi].view(np.uint32).any()
    free = ~c["owned"]
    assert np.array_equal(dst[free].view(np.uint32), c["x"][free].view(np.uint32)) if in_place else np.isnan(dst[free]).all()
    unserved = [s for s in range(k.n_slots) if s not in [int(k.slot[b]) for b in k.served]]
    assert np.array_equal(pool[unserved].view(np.uint32), _model_pool(c, k)[unserved].view(np.uint32))


@pytest.mark.parametrize("d_conv", D_CONVS)
@pytest.mark.parametrize("mutant", npt.MUTANTS)
def test_every_mutant_of_the_model_changes_a_bit_of_the_batch(mutant, d_conv):
    """the batch can see the three hazards: a halo of zeros, halo rows read after in-place writes, the new slot taken after in-place writes, the slot of a
    fresh sequence read, tiles cut on packed-row boundaries with the window taken from the rows in front regardless of owner"""
    k, c = batch(), case(5, d_conv)
    for in_place in (False, True):
        if not in_place and mutant in npt.IN_PLACE_ONLY:
            continue
        a = (c["x"], c["w"], c["bias"], k.q_start, k.d_len, k.slot, _model_pool(c, k), k.n_tokens_max, k.T, k.S)
        good = npt.conv_tiled(*a, in_place=in_place)
        with np.errstate(all="ignore"):                              # (a mutant may meet the 3.0e38 of a row nobody owns)
            bad = npt.conv_tiled(*a, in_place=in_place, mutant=mutant)
        rows = [np.array_equal(good[0][slice(*k.rows(b))].view(np.uint32), bad[0][slice(*k.rows(b))].view(np.uint32)) for b in k.served]
        slots = [np.array_equal(good[1][k.slot[b]].view(np.uint32), bad[1][k.slot[b]].view(np.uint32)) for b in k.served]
        assert not all(rows + slots), (mutant, in_place)


# ---------------------------------------------------------------- GPU
def _pads(name):
    """(pad_x, pad_d, shift) of a shape's batch call: paddings that keep the 4-channel path where the shape is meant to take it"""
    n_ch, push = SHAPES[name]
    if push == "ldx":
        return 3, 8, 0
    if push == "ptr":
        return 4, 8, 1
    return (4, 8, 0) if n_ch % 4 == 0 else (3, 6, 0)


def _call(dev, c, q_start, d_len, slot, pool, n, row0=0, bias=True, act=0, pad_x=0, pad_d=0, shift=0, in_place=False, old=False, work_off=0, work_extra=0):
    """one call over rows [row0, row0 + n) of the case's packed inputs: the tiled entry, or with old the sequential one.  x and dst start `shift` elements
    behind a 16-byte boundary; the work buffer starts work_off bytes behind one, is work_extra bytes longer than needed and holds NaN bytes.
    -> (rows [n][n_ch] as uint32, the pool image after the call); the guards of dst and of the work buffer, the padding columns and d_x are checked here"""
    torch = dev.torch
    n_ch, K = c["n_ch"], c["d_conv"]
    ldx = n_ch + pad_x
    ldd = ldx if in_place else n_ch + pad_d
    x = np.full((n, ldx), 3.0e38, F)
    x[:, :n_ch] = c["x"][row0:row0 + n]
    head = GUARD + shift
    xbuf = np.full(head + n * ldx + GUARD, SENTINEL, np.uint32)
    xbuf[head:head + n * ldx] = x.view(np.uint32).reshape(-1)
    d_x, d_w, d_b = _up(dev, xbuf), _up(dev, c["w"]), _up(dev, c["bias"])
    d_q, d_l, d_s = _up(dev, np.asarray(q_start, np.int32)), _up(dev, np.asarray(d_len, np.int32)), _up(dev, np.asarray(slot, np.int32))
    d_pool = _up(dev, pool.image)
    dst = d_x if in_place else torch.full((head + n * ldd + GUARD,), SENTINEL, dtype=torch.int32, device="cuda")
    assert d_x.data_ptr() % 16 == 0 and dst.data_ptr() % 16 == 0 and d_w.data_ptr() % 16 == 0 and d_b.data_ptr() % 16 == 0
    L = _lib.lib()
    common = (_p(d_x.data_ptr() + 4 * head), ldx, _p(d_w.data_ptr()), _p(d_b.data_ptr()) if bias else None, int(act), n_ch, K, len(slot), _p(d_q.data_ptr()), n,
              _p(d_l.data_ptr()), _p(d_s.data_ptr()), _p(pool.ptr(d_pool)), pool.nb_slot, pool.n_slots, _p(dst.data_ptr() + 4 * head), ldd)
    if old:
        rc = L.ggml_hip_ssm_conv_ragged_dev(*common, _stream(dev))
    else:
        need = _work_size(n_ch, K, len(slot), n)
        size = need + work_extra
        wbuf = torch.full((WORK_GUARD + work_off + size + WORK_GUARD,), 255, dtype=torch.uint8, device="cuda")
        assert wbuf.data_ptr() % 256 == 0
        rc = L.ggml_hip_ssm_conv_tiled_ragged_dev(*common, _p(wbuf.data_ptr() + WORK_GUARD + work_off) if size else None, size, _stream(dev))
    assert rc == 0, L.ggml_hip_last_error()
    torch.cuda.synchronize()
    if not old:
        wb = wbuf.cpu().numpy()
        assert (wb[:WORK_GUARD + work_off] == 255).all() and (wb[WORK_GUARD + work_off + size:] == 255).all(), "guards of the work buffer written"
    out = _bits(dst)
    assert (out[:head] == SENTINEL).all() and (out[head + n * ldd:] == SENTINEL).all(), "guards of dst written"
    body = out[head:head + n * ldd].reshape(n, ldd)
    if in_place:
        assert np.array_equal(body[:, n_ch:], x.view(np.uint32)[:, n_ch:]), "padding columns written"
    else:
        assert (body[:, n_ch:] == SENTINEL).all(), "padding columns written"
        assert np.array_equal(_bits(d_x), xbuf), "d_x written"
    return body[:, :n_ch], _bits(d_pool)


def _batch_pool(c, pad=None):
    k = batch()
    elems = (c["d_conv"] - 1) * c["n_ch"]
    pool = Pool(k.n_slots, elems, (-elems) % 4 + 4 if pad is None else pad)
    for s in range(k.n_slots):
        pool.put(s, c["pool"][s])
    for b in range(k.n_seq):
        if k.d_len[b] == 0 and 0 <= k.slot[b] < k.n_slots:
            pool.put_nan(int(k.slot[b]))
    return pool


@pytest.mark.gpu
@pytest.mark.parametrize("d_conv", D_CONVS)
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_tiled_conv_over_the_ragged_batch(dev, name, d_conv):
    k = batch()
    n_ch, push = SHAPES[name]
    c = case(n_ch, d_conv)
    n, elems = k.n_tokens_max, (d_conv - 1) * n_ch
    pad_x, pad_d, shift = _pads(name)
    rc, p = _plan(n_ch, d_conv, k.n_seq, n)
    assert rc == OK and p.form == 2 and p.vec == (4 if n_ch % 4 == 0 else 1)
    pool = _batch_pool(c)
    args = (dev, c, k.q_start, k.d_len, k.slot, pool, n)
    kw = dict(pad_x=pad_x, pad_d=pad_d, shift=shift)
    # (bias, act 0): the statement bit for bit, rows and slots; rows and pool as tests/test_ssm.py _rows_and_pool_of_the_batch states
    y, after = _call(*args, **kw)
    for b in k.served:
        lo, hi = k.rows(b)
        want, want_slot = statement(n_ch, d_conv, b, True)
        assert np.array_equal(y[lo:hi], want.view(np.uint32)), ("rows", b)
        assert np.array_equal(pool.slot(after, int(k.slot[b])), want_slot.view(np.uint32).reshape(-1)), ("slot", b)
    owned = ts._rows_and_pool_of_the_batch(k, y, after, pool, elems)
    assert np.array_equal(owned, c["owned"])
    # all four (bias, act) pairs: the sequential entry on the same batch, bit for bit (act = 1 is the same expression on the same bits)
    for bias in (True, False):
        for act in (0, 1):
            y_new, after_new = (y, after) if (bias, act) == (True, 0) else _call(*args, bias=bias, act=act, **kw)
            y_old, after_old = _call(*args, bias=bias, act=act, old=True, **kw)
            assert np.array_equal(y_new, y_old) and np.array_equal(after_new, after_old), (bias, act)
            if act:                                                  # ... and the old bar: 3 * 2^-24 relative of the silu of the statement's bits
                for b in k.served:
                    lo, hi = k.rows(b)
                    ref = np_ssm.silu64(statement(n_ch, d_conv, b, bias)[0])
                    worst = float((np.abs(y_new[lo:hi].view(F).astype(np.float64) - ref) / np.abs(ref)).max())
                    assert worst <= 3.0 * U, (b, worst / U)
            elif not bias:
                for b in k.served:
                    lo, hi = k.rows(b)
                    assert np.array_equal(y_new[lo:hi], statement(n_ch, d_conv, b, False)[0].view(np.uint32)), ("rows without bias", b)
            # in place: the same rows (the rows nobody owns keep x) and the same pool
            y_in, after_in = _call(*args, bias=bias, act=act, in_place=True, pad_x=pad_x, shift=shift)
            assert np.array_equal(y_in[owned], y_new[owned]) and np.array_equal(y_in[~owned], c["x"].view(np.uint32)[~owned]), (bias, act)
            assert np.array_equal(after_in, after_new), (bias, act)
    # (iii): the work buffer's address, length and old contents
    y2, after2 = _call(*args, work_off=52, work_extra=1000, **kw)
    assert np.array_equal(y2, y) and np.array_equal(after2, after)


def _split_points(n, d_conv):
    k = batch()
    return sorted({1, max(1, d_conv - 2), k.S, k.T - 1, k.T, n - 1})


@pytest.mark.gpu
@pytest.mark.parametrize("d_conv", D_CONVS)
@pytest.mark.parametrize("name", ("c5", "c64", "c1028"))
def test_a_sequence_alone_and_split_over_calls(dev, name, d_conv):
    k = batch()
    n_ch, _ = SHAPES[name]
    c = case(n_ch, d_conv)
    elems = (d_conv - 1) * n_ch
    pad_x, pad_d, shift = _pads(name)
    pool = _batch_pool(c)
    y, after = _call(dev, c, k.q_start, k.d_len, k.slot, pool, k.n_tokens_max, pad_x=pad_x, pad_d=pad_d)
    # (i) + (iii): every served sequence alone -- n_seq = 1, another slot number in another pool, other strides, another n_tokens_max (which may take
    # a sequence of S tokens' call to form 2 and back), a longer work buffer at another offset
    for b in k.served:
        lo, hi = k.rows(b)
        one = Pool(3, elems, (-elems) % 4)
        one.put(2, c["pool"][k.slot[b]]) if k.d_len[b] else one.put_nan(2)
        y1, after1 = _call(dev, c, [0, hi - lo], [k.d_len[b]], [2], one, hi - lo + 1, row0=lo, pad_x=0 if n_ch % 4 == 0 else 1, pad_d=4 if n_ch % 4 == 0 else 2,
                           work_off=4, work_extra=300)
        assert np.array_equal(y1[:hi - lo], y[lo:hi]), ("rows alone", b)
        assert np.array_equal(one.slot(after1, 2), pool.slot(after, int(k.slot[b]))), ("state alone", b)
    # (ii): a long sequence split over two calls of the tiled entry -- parts of 1 .. S tokens run sequential, the others tiled
    for b in (0, 1):                                                 # continued and fresh
        lo, hi = k.rows(b)
        for cut in _split_points(hi - lo, d_conv):
            two = Pool(2, elems, (-elems) % 4 + 4)
            two.put(1, c["pool"][k.slot[b]]) if k.d_len[b] else two.put_nan(1)
            ya, mid = _call(dev, c, [0, cut], [k.d_len[b]], [1], two, cut, row0=lo, pad_x=pad_x)
            two.image = mid
            yb, end = _call(dev, c, [0, hi - lo - cut], [int(k.d_len[b]) + cut], [1], two, hi - lo - cut, row0=lo + cut, pad_d=pad_d)
            assert np.array_equal(np.concatenate([ya, yb]), y[lo:hi]), ("rows split", b, cut)
            assert np.array_equal(two.slot(end, 1), pool.slot(after, int(k.slot[b]))), ("state split", b, cut)


def test_the_split_points_are_what_the_contract_names():
    k = batch()
    for K in D_CONVS:
        n = k.counts[0]
        cuts = _split_points(n, K)
        assert {1, k.S, k.T - 1, k.T, n - 1} <= set(cuts) and max(1, K - 2) in cuts and all(0 < cut < n for cut in cuts)
        assert any(cut <= k.S < n - cut for cut in cuts) and any(n - cut <= k.S < cut for cut in cuts)     # a part in each form, both ways round
        assert n - 1 > k.S                                           # the one-token tail follows a tiled part


def _t(dev, a):
    return dev.torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
def test_a_captured_step_follows_the_batch_and_no_tokens_is_accepted(dev):
    """a captured tiled-conv + chunked-scan step replayed after d_q_start, d_len and d_slot changed on the device: sequences move between the forms of
    both entries in both directions.  Then n_tokens_max = 0"""
    torch = dev.torch
    T, S = _t_and_s()
    H, P, N, G, n_ch, K, n_slots = 4, 16, 16, 1, 64, 4, 8
    sp = dev.ssm_scan_chunked_plan(H, P, N, G, False, 6, 1 << 20)
    hi, lo = max(S, sp.seq_max_tokens) + 5, min(S, sp.seq_max_tokens)
    cnt1, cnt2 = [2 * hi + 3, 1, lo, hi, 0, 2], [lo, hi + 1, 2 * hi, 1, 3, hi]
    n = max(sum(cnt1), sum(cnt2)) + 2
    down = [b for b in range(6) if cnt1[b] > max(S, sp.seq_max_tokens) and cnt2[b] <= lo]
    up = [b for b in range(6) if cnt2[b] > max(S, sp.seq_max_tokens) and cnt1[b] <= lo]
    assert down and up
    rng = np.random.default_rng(271)
    t = functools.partial(_t, dev)
    x, dt, A = t(rng.normal(0, 1, (n, H, P)).astype(F)), t((2.0 * rng.normal(0, 1, (n, H)) - 1.0).astype(F)), t((-np.exp(rng.uniform(-3, 1, H))).astype(F))
    B, Cc, D = t(rng.normal(0, 1, (n, G, N)).astype(F)), t(rng.normal(0, 1, (n, G, N)).astype(F)), t(rng.normal(0, 1, H).astype(F))
    cx, cw, cb = t(rng.normal(0, 1, (n, n_ch)).astype(F)), t(rng.normal(0, 0.7, (n_ch, K)).astype(F)), t(rng.normal(0, 0.5, n_ch).astype(F))
    pool0, cpool0 = t(rng.normal(0, 1, (n_slots, H * P * N)).astype(F)), t(rng.normal(0, 1, (n_slots, (K - 1) * n_ch)).astype(F))
    work = torch.empty(dev.ssm_scan_chunked_work_size(H, P, N, G, False, 6, n), dtype=torch.uint8, device="cuda")
    cwork = torch.empty(dev.ssm_conv_tiled_work_size(n_ch, K, 6, n), dtype=torch.uint8, device="cuda")
    assert dev.ssm_conv_tiled_plan(n_ch, K, 6, n).form == 2 and cwork.numel() > 0
    q1, q2 = (np.concatenate([[0], np.cumsum(cn)]).astype(np.int32) for cn in (cnt1, cnt2))
    one = (q1, np.array([4, 0, 3, 0, 5, 2], np.int32), np.array([7, 2, 5, 0, 1, -1], np.int32))
    two = (q2, np.array([0, 3, 0, 2, 0, 6], np.int32), np.array([3, 1, n_slots, 6, 0, 2], np.int32))

    def step(q, ln, sl, pool, cpool, y, cy, tiled=True):
        if tiled:
            dev.ssm_conv_tiled_ragged(cx, cw, q, ln, sl, cpool, bias=cb, act=True, out=cy, work=cwork)
        else:
            dev.ssm_conv_ragged(cx, cw, q, ln, sl, cpool, bias=cb, act=True, out=cy)
        dev.ssm_scan_chunked_ragged(x, dt, A, B, Cc, q, ln, sl, pool, dt_bias=None, D=D, out=y, work=work)

    def fresh():
        return pool0.clone(), cpool0.clone(), torch.zeros_like(x), torch.zeros_like(cx)

    want = {}
    for key, (q, ln, sl) in (("one", one), ("two", two)):
        pool, cpool, y, cy = fresh()
        step(t(q), t(ln), t(sl), pool, cpool, y, cy, tiled=False)   # the yardstick: the same step with the sequential conv
        torch.cuda.synchronize()
        want[key] = [_bits(v) for v in (pool, cpool, y, cy)]
    assert not any(np.array_equal(a, b) for a, b in zip(want["one"], want["two"]))
    d_q, d_l, d_s = (t(v) for v in one)
    pool, cpool, y, cy = fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(d_q, d_l, d_s, pool, cpool, y, cy)
    torch.cuda.current_stream().wait_stream(s)
    for key, (q, ln, sl) in (("two", two), ("one", one), ("two", two)):
        d_q.copy_(t(q)), d_l.copy_(t(ln)), d_s.copy_(t(sl))
        for dst, src in zip((pool, cpool, y, cy), fresh()):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip((pool, cpool, y, cy), want[key]):
            assert np.array_equal(_bits(got), w), key
    # n_tokens_max = 0: accepted, nothing written, no work buffer needed
    before = [_bits(v) for v in (cpool, cy)]
    dev.ssm_conv_tiled_ragged(cx, cw, d_q, d_l, d_s, cpool, bias=cb, n_tokens_max=0, out=cy)
    torch.cuda.synchronize()
    for got, w in zip((cpool, cy), before):
        assert np.array_equal(_bits(got), w)


@pytest.mark.gpu
def test_the_python_face_on_the_xbc_of_a_mamba2_block(dev):
    """what a Mamba-2 block hands over: ONE [n_tokens, d_inner + 2 G N] tensor xBC (256 + 512 channels), convolved IN PLACE by the tiled entry with the
    work buffer left to the wrapper, and the chunked scan on views of it.  Rows, conv slots and scan slots are bit for bit those of the same step with the
    sequential conv"""
    torch = dev.torch
    k = batch()
    H, P, N, G, K = 4, 64, 128, 2, 4
    d_inner, gn, n = H * P, G * N, k.n_tokens_max
    n_ch = d_inner + 2 * gn
    assert (d_inner, 2 * gn) == (256, 512)
    rng = np.random.default_rng(314)
    t = functools.partial(_t, dev)
    d_q, d_l, d_s = t(k.q_start), t(k.d_len), t(k.slot)
    xBC0 = t(rng.normal(0, 1, (n, n_ch)).astype(F))
    w, bias = t(rng.normal(0, 0.7, (n_ch, K)).astype(F)), t(rng.normal(0, 0.5, n_ch).astype(F))
    dt, A, D = t((2.0 * rng.normal(0, 1, (n, H)) - 1.0).astype(F)), t((-np.exp(rng.uniform(-3, 1, H))).astype(F)), t(rng.normal(0, 1, H).astype(F))
    cpool0 = torch.full((k.n_slots, (K - 1) * n_ch + 4), float("nan"), dtype=torch.float32, device="cuda")
    cpool0[:, :(K - 1) * n_ch] = t(rng.normal(0, 1, (k.n_slots, (K - 1) * n_ch)).astype(F))
    pool0 = t(rng.normal(0, 1, (k.n_slots, H * P * N)).astype(F))
    fresh = [int(k.slot[b]) for b in k.served if k.d_len[b] == 0]
    cpool0.view(torch.int32)[fresh] = -1
    pool0.view(torch.int32)[fresh] = -1
    got = {}
    for key in ("tiled", "sequential"):
        xBC, cpool_w, pool = xBC0.clone(), cpool0.clone(), pool0.clone()
        cpool = cpool_w[:, :(K - 1) * n_ch]
        conv = dev.ssm_conv_tiled_ragged if key == "tiled" else dev.ssm_conv_ragged
        r = conv(xBC, w, d_q, d_l, d_s, cpool, bias=bias, act=True, out=xBC)
        assert r is xBC and cpool.stride(0) == (K - 1) * n_ch + 4
        x = xBC[:, :d_inner].unflatten(1, (H, P))
        B = xBC[:, d_inner:d_inner + gn].unflatten(1, (G, N))
        Cc = xBC[:, d_inner + gn:].unflatten(1, (G, N))
        y = torch.zeros((n, H, P), dtype=torch.float32, device="cuda")
        dev.ssm_scan_chunked_ragged(x, dt, A, B, Cc, d_q, d_l, d_s, pool, D=D, out=y)
        torch.cuda.synchronize()
        got[key] = [_bits(v) for v in (xBC, cpool_w, pool, y)]
    for a, b, what in zip(got["tiled"], got["sequential"], ("xBC", "conv slots", "scan slots", "y")):
        assert np.array_equal(a, b), what
    assert not np.array_equal(got["tiled"][0], _bits(xBC0))
    p = dev.ssm_conv_tiled_plan(n_ch, K, k.n_seq, n)
    assert (p.form, p.tile, p.seq_max_tokens, p.vec) == (2, k.T, k.S, 4) and p.work_bytes == dev.ssm_conv_tiled_work_size(n_ch, K, k.n_seq, n)
