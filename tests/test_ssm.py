"""The SSM entries (include/ggml_hip_ext.h, SSM: ggml_hip_ssm_conv_ragged_dev, ggml_hip_ssm_scan_ragged_dev; csrc/ssm.hip, ssm.cpp, plan.cpp).

Yardsticks (tests/np_ssm.py): the scan's statement in float64 with the bar DERIVED there from u = 2^-24 -- the kernels are held to 1 x the bar for y and for
the final state, and so is the float32 model; four mutants of the statement exceed it by >= 100 x, so the bar can see a mistake.  The conv (act = 0) and its
slot are bit for bit the statement with an exact binary32 fma; act = 1 is within 3 * 2^-24 relative of the silu of those bits.  The three bitwise contracts of
the scan -- a sequence alone, a sequence split over calls, nothing from the batch / slot number / n_tokens_max / strides -- need no reference.

ONE ragged batch serves every shape: counts 0, 1, 2, 3, 9 and 130 (below, at and above d_conv - 1 for d_conv 2 and 4), one sequence that is not present, a
slot id of -1 and one of n_slots, fresh (d_len 0, the slot preloaded with NaN bytes) and continued sequences, two packed rows nobody owns.
Scan shapes: the Mamba-1 form (P = 1, N = 16, per-state A) at 8 and 264 heads (one workgroup, more than one); the Mamba-2 form (P = 64, N = 128) with one and
two groups; N = 48, three slices in a group of four lanes, with rows that fill no whole wave; 7 heads of the Mamba-1 form and N = 32 with 9 rows, whose
lanes end inside a quad (the state moves by quads of lanes where no lane of a group idles).  Conv: 1, 5, 64 and 1028 channels (more than one workgroup).

ONE SHAPE PER KERNEL FORM.  The scan is compiled once per (lanes of a row LP, FULL: N == 16 LP, A per state); twelve more shapes (SHAPES, below the first
seven) reach the forms those seven do not, and test_every_form_the_plan_can_pick_has_a_shape compares the forms of SHAPES with the forms the plan hands out
over every N, so a form added to the plan must bring its shape.  Two kernel-shaped mutants (np_ssm.KERNEL_MUTANTS: the butterfly a step short, the A of
state 0 for every state) exceed the bar a hundredfold where they apply.  The batch call of every shape gives dst, dt and A strides of their own (other than
x's, above n_head, above N or 1) with 3.0e38 or the sentinel in the gaps; D and dt_bias are null at two shapes.  A SECOND batch (BATCH_2) has sequences of
exactly 7, 8 and 16 tokens (the conv's token loop is unrolled by 8) and the other ways to be absent: an end beyond n_tokens_max, a start above the end."""
import ctypes as C
import fnmatch
import functools
import os
import re

import numpy as np
import pytest

import np_ssm
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ggml_hip_ssm_conv_state_bytes", "ggml_hip_ssm_state_bytes", "ggml_hip_ssm_scan_plan", "ggml_hip_ssm_conv_ragged_dev",
               "ggml_hip_ssm_scan_ragged_dev")
SENTINEL = 0x7FC00123                                               # a NaN no kernel here produces
NAN_BYTES = 0xFFFFFFFF
OK, ERR_TYPE, ERR_SHAPE, ERR_ARG = 0, -2, -3, -4
FAKE = 0x1000                                                       # a non-null, 16-byte aligned pointer no refusal may touch
GUARD = 64                                                          # elements
F = np.float32
U = np_ssm.U

# ---------------------------------------------------------------- the batch
N_TOKENS_MAX = 150
Q_START = np.array([-3, 0, 1, 1, 3, 12, 142, 143, 145, 148], np.int32)
D_LEN = np.array([4, 7, 3, 0, 5, 0, 2, 0, 2], np.int32)
N_SLOTS = 10
SLOT = np.array([7, 2, 5, 0, 9, 4, -1, N_SLOTS, 1], np.int32)
N_SEQ = SLOT.size
SERVED = (1, 3, 4, 5, 8)                                            # present, not idle, a slot inside the pool
ZEROED = (6, 7)                                                     # present, not idle, a slot id outside the pool: +0.0f rows, no state
SPLITS = ((4, 4), (5, 1), (5, 64))                                  # (sequence, tokens in the first of two calls)

# the second batch: 7, 8 and 16 tokens (one short of, exactly and twice the conv's unroll of 8) and 5; sequence 3 and 6 end beyond n_tokens_max, sequence 4
# starts above its end and beyond n_tokens_max; rows 31, 32, 38 and 39 belong to nobody
N_TOKENS_MAX_2 = 40
Q_START_2 = np.array([0, 7, 15, 31, 50, 33, 38, 44], np.int32)
D_LEN_2 = np.array([0, 3, 0, 2, 1, 4, 1], np.int32)
SLOT_2 = np.array([4, 0, 9, 1, 2, 6, 3], np.int32)
SERVED_2 = (0, 1, 2, 5)


class Batch:
    """a ragged batch over the pool of N_SLOTS slots; the packed rows it addresses are rows [0, n_tokens_max) of a case's inputs"""

    def __init__(self, n_tokens_max, q_start, d_len, slot, served, zeroed):
        self.n_tokens_max, self.q_start, self.d_len, self.slot, self.served, self.zeroed = n_tokens_max, q_start, d_len, slot, served, zeroed
        self.n_seq = slot.size

    def rows(self, b):
        return int(self.q_start[b]), int(self.q_start[b + 1])


BATCH_1 = Batch(N_TOKENS_MAX, Q_START, D_LEN, SLOT, SERVED, ZEROED)
BATCH_2 = Batch(N_TOKENS_MAX_2, Q_START_2, D_LEN_2, SLOT_2, SERVED_2, ())

# seed: the inputs of a shape follow it alone (the first seven keep the seeds they had as the only shapes, 71 + their place in the sorted names)
SHAPES = {
    "mamba1_8": dict(H=8, P=1, N=16, G=1, aps=True, seed=73),
    "mamba1_264": dict(H=264, P=1, N=16, G=1, aps=True, seed=71),
    "mamba2_g1": dict(H=4, P=64, N=128, G=1, aps=False, seed=74),
    "mamba2_g2": dict(H=4, P=64, N=128, G=2, aps=False, seed=75),
    "n48": dict(H=4, P=5, N=48, G=2, aps=False, seed=77),
    # the state moves by quads of lanes where N is a power-of-two multiple of 16: a last quad that is only partly inside the rows, one and two lanes per row
    "mamba1_7": dict(H=7, P=1, N=16, G=1, aps=True, seed=72),
    "n32": dict(H=3, P=3, N=32, G=3, aps=False, seed=76),
    # one shape per (LP, FULL, A per state) the seven above do not reach -- the smallest that does, with what else it covers
    "n16_head": dict(H=5, P=3, N=16, G=1, aps=False, seed=79),       # 1, FULL, per head; 15 rows: a partial last quad
    "n32_aps": dict(H=3, P=43, N=32, G=1, aps=True, seed=84),        # 2, FULL; 129 rows: a second workgroup that holds one row
    "n48_aps": dict(H=2, P=3, N=48, G=2, aps=True, seed=86),         # 4, plain
    "n64": dict(H=5, P=13, N=64, G=1, aps=False, seed=87),           # 4, FULL; 65 rows: a second workgroup that holds one row
    "n64_aps": dict(H=2, P=2, N=64, G=2, aps=True, seed=88),         # 4, FULL
    "n80": dict(H=4, P=3, N=80, G=2, aps=False, seed=89),            # 8, plain: 5 of 8 lanes live
    "n112_aps": dict(H=3, P=11, N=112, G=1, aps=True, seed=76),      # 8, plain; 33 rows: a second workgroup
    "n128_aps": dict(H=2, P=3, N=128, G=1, aps=True, seed=77),       # 8, FULL
    "n144": dict(H=3, P=5, N=144, G=3, aps=False, seed=78),          # 16, plain: 9 of 16 lanes live
    "n240_aps": dict(H=2, P=3, N=240, G=1, aps=True, seed=80),       # 16, plain: 15 of 16 lanes live
    "n256": dict(H=6, P=3, N=256, G=2, aps=False, seed=81),          # 16, FULL; 18 rows: a second workgroup that holds two
    "n256_aps": dict(H=2, P=2, N=256, G=1, aps=True, seed=82),       # 16, FULL
}
FIRST_SEVEN = ("mamba1_264", "mamba1_7", "mamba1_8", "mamba2_g1", "mamba2_g2", "n32", "n48")


def _rows(b):
    return BATCH_1.rows(b)


def test_the_batch_is_what_it_says():
    counts = [int(Q_START[b + 1] - Q_START[b]) for b in range(1, N_SEQ)]
    assert counts == [1, 0, 2, 9, 130, 1, 2, 3]
    present = [b for b in range(N_SEQ) if 0 <= Q_START[b] <= Q_START[b + 1] <= N_TOKENS_MAX]
    assert present == list(range(1, N_SEQ)) and Q_START[N_SEQ] == N_TOKENS_MAX - 2
    live = [b for b in present if Q_START[b + 1] > Q_START[b]]
    assert tuple(b for b in live if 0 <= SLOT[b] < N_SLOTS) == SERVED and tuple(b for b in live if not 0 <= SLOT[b] < N_SLOTS) == ZEROED
    assert sorted(SLOT[b] for b in ZEROED) == [-1, N_SLOTS]
    assert [int(D_LEN[b]) == 0 for b in SERVED] == [False, True, False, True, False]
    assert len({int(SLOT[b]) for b in SERVED}) == len(SERVED)


def test_the_second_batch_is_what_it_says():
    q, n = Q_START_2, SLOT_2.size
    assert n == 7 and D_LEN_2.size == n and q.size == n + 1
    present = tuple(b for b in range(n) if 0 <= q[b] <= q[b + 1] <= N_TOKENS_MAX_2)
    assert present == SERVED_2 and all(0 <= SLOT_2[b] < N_SLOTS for b in range(n))
    assert [int(q[b + 1] - q[b]) for b in SERVED_2] == [7, 8, 16, 5]
    assert q[3] <= q[4] and q[4] > N_TOKENS_MAX_2                    # 3: ends beyond n_tokens_max
    assert q[4] > q[5] and q[4] > N_TOKENS_MAX_2                     # 4: starts above its end, and beyond n_tokens_max
    assert 0 <= q[6] <= q[7] and q[7] > N_TOKENS_MAX_2               # 6: ends beyond n_tokens_max
    owned = np.zeros(N_TOKENS_MAX_2, bool)
    for b in SERVED_2:
        assert not owned[q[b]:q[b + 1]].any()
        owned[q[b]:q[b + 1]] = True
    assert list(np.flatnonzero(~owned)) == [31, 32, 38, 39]
    assert [int(D_LEN_2[b]) == 0 for b in SERVED_2] == [True, False, True, False]
    assert len({int(s) for s in SLOT_2}) == n                        # (the absent sequences name slots of their own: what must stay unchanged)
    assert all(D_LEN_2[b] > 0 for b in range(n) if b not in SERVED_2)


def test_the_first_seven_shapes_keep_their_inputs():
    assert [SHAPES[name]["seed"] for name in FIRST_SEVEN] == list(range(71, 78)) and len(SHAPES) == 19
    assert sorted(FIRST_SEVEN) == list(FIRST_SEVEN) and list(SHAPES)[:7] == ["mamba1_8", "mamba1_264", "mamba2_g1", "mamba2_g2", "n48", "mamba1_7", "n32"]


# ---------------------------------------------------------------- the scan's inputs and references, computed once
@functools.lru_cache(maxsize=None)
def scan_case(name):
    s = SHAPES[name]
    H, P, N, G = s["H"], s["P"], s["N"], s["G"]
    rng = np.random.default_rng(s["seed"])
    c = dict(s)
    c["x"] = rng.normal(0.0, 1.0, (N_TOKENS_MAX, H, P)).astype(F)
    c["dt"] = (2.0 * rng.normal(0.0, 1.0, (N_TOKENS_MAX, H)) - 1.0).astype(F)
    c["dt"][13, 0] = F(25.0)                                         # (the branch d > 20, in the long sequence)
    c["A"] = (-np.exp(rng.uniform(-3.0, 2.5, (H, N) if s["aps"] else (H,)))).astype(F)
    c["B"] = rng.normal(0.0, 1.0, (N_TOKENS_MAX, G, N)).astype(F)
    c["C"] = rng.normal(0.0, 1.0, (N_TOKENS_MAX, G, N)).astype(F)
    c["D"] = rng.normal(0.0, 1.0, H).astype(F)
    c["dt_bias"] = (0.5 * rng.normal(0.0, 1.0, H)).astype(F)
    c["pool"] = rng.normal(0.0, 1.0, (N_SLOTS, H, P, N)).astype(F)  # what the slots hold before the call (the fresh sequences' are NaN bytes on the device)
    return c


def _seq_args(c, b, k=BATCH_1, with_D=True, with_bias=True):
    lo, hi = k.rows(b)
    h0 = None if k.d_len[b] == 0 else c["pool"][k.slot[b]]
    return ((c["x"][lo:hi], c["dt"][lo:hi], c["A"], c["B"][lo:hi], c["C"][lo:hi]),
            dict(D=c["D"] if with_D else None, dt_bias=c["dt_bias"] if with_bias else None, h0=h0))


@functools.lru_cache(maxsize=None)
def scan_ref(name, b, k=BATCH_1, with_D=True, with_bias=True):
    """(y, h, bar_y, bar_h) of sequence b of batch k in float64"""
    a, kw = _seq_args(scan_case(name), b, k, with_D, with_bias)
    return np_ssm.scan_f64(*a, want_bar=True, **kw)


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
    assert "ggml_hip_ssm_plan_t" in hdr and "ggml_hip_ssm_plan_t" in cs and C.sizeof(_lib.ggml_hip_ssm_plan_t) == 32


def test_the_exact_fma_of_the_yardstick():
    # a * b + c lies a hair above the midpoint of two binary32 values: rounding the binary64 sum (a tie there) and then to binary32 would go DOWN
    a, b, c = F(1 + 2.0 ** -12), F(1 + 2.0 ** -12), F(2.0 ** -60)
    exact = (1 + 2.0 ** -11) + 2.0 ** -24                             # + 2^-60: above the midpoint between 1 + 2^-11 and 1 + 2^-11 + 2^-23
    assert np_ssm.fmaf(a, b, c) == F(1 + 2.0 ** -11 + 2.0 ** -23) and F(exact) == F(1 + 2.0 ** -11)
    rng = np.random.default_rng(1)
    x, y, z = (rng.normal(0, 1, 4096).astype(F) for _ in range(3))
    assert np.array_equal(np_ssm.fmaf(x, y, np.zeros_like(z)), x * y) and np.array_equal(np_ssm.fmaf(x, np.ones_like(y), z), x + z)


def _model_within_the_bar(name, k=BATCH_1, with_D=True, with_bias=True):
    c = scan_case(name)
    for b in k.served:
        y, h, bar_y, bar_h = scan_ref(name, b, k, with_D, with_bias)
        a, kw = _seq_args(c, b, k, with_D, with_bias)
        y32, h32 = np_ssm.scan_f32(*a, **kw)
        ry, rh = float((np.abs(y32 - y) / bar_y).max()), float((np.abs(h32 - h) / bar_h).max())
        print(f"{name} seq {b}: model / bar  y {ry:.3f}  state {rh:.3f};  bar / |y| median {float(np.median(bar_y / np.maximum(np.abs(y), 1e-30))):.2e}")
        assert ry <= 1.0 and rh <= 1.0, (name, b, ry, rh)


def _mutants_exceed_the_bar(name, mutants, k=BATCH_1, with_D=True, with_bias=True):
    c = scan_case(name)
    for mutant in mutants:
        for b in k.served:
            y, h, bar_y, bar_h = scan_ref(name, b, k, with_D, with_bias)
            a, kw = _seq_args(c, b, k, with_D, with_bias)
            with np.errstate(all="ignore"):
                ym, _ = np_ssm.scan_f64(*a, mutant=mutant, **kw)
                diff = np.abs(ym - y)
                worst = float(np.where(np.isfinite(diff), diff / bar_y, np.inf).max())
            print(f"{name} seq {b}: {mutant} / bar  y {worst:.3g}")
            assert worst >= 100.0, (name, mutant, b, worst)


def _statement_mutants(name, with_D=True):
    """(a group index off by one is the statement itself with one group, a dropped D the statement itself without D)"""
    G = SHAPES[name]["G"]
    return tuple(m for m in np_ssm.MUTANTS if not (m == "group_off_by_one" and G == 1) and not (m == "drop_D" and not with_D))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_float32_model_is_within_the_bar(name):
    _model_within_the_bar(name)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_four_mutants_of_the_statement_exceed_the_bar_a_hundredfold(name):
    """(a group index off by one is the statement itself with one group: that mutant is judged where G = 2)"""
    _mutants_exceed_the_bar(name, _statement_mutants(name))


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_two_kernel_shaped_mutants_exceed_the_bar_a_hundredfold(name):
    """the butterfly one step short where a row has more than one lane, the A of state 0 for every state where A is per state: every shape but the
    one-lane per-head one is judged by at least one"""
    s = SHAPES[name]
    mutants = (("short_butterfly",) if s["N"] > 16 else ()) + (("a_of_state_0",) if s["aps"] else ())
    assert mutants or name == "n16_head"
    _mutants_exceed_the_bar(name, mutants)


OPTIONAL_SHAPES = ("n144", "n32_aps")
OPTIONAL_OPERANDS = ((False, True), (True, False), (False, False))  # (with D, with dt_bias)


@pytest.mark.parametrize("with_D,with_bias", OPTIONAL_OPERANDS)
@pytest.mark.parametrize("name", OPTIONAL_SHAPES)
def test_the_model_and_the_mutants_without_the_optional_operands(name, with_D, with_bias):
    _model_within_the_bar(name, BATCH_1, with_D, with_bias)
    _mutants_exceed_the_bar(name, _statement_mutants(name, with_D), BATCH_1, with_D, with_bias)


SECOND_BATCH_SHAPES = ("mamba1_8", "n144", "n256")


@pytest.mark.parametrize("name", SECOND_BATCH_SHAPES)
def test_the_model_and_the_mutants_over_the_second_batch(name):
    _model_within_the_bar(name, BATCH_2)
    _mutants_exceed_the_bar(name, _statement_mutants(name), BATCH_2)


def _forms(shapes):
    return {(_plan(s["H"], s["P"], s["N"], s["G"], 1)[1][3], s["N"] == 16 * _plan(s["H"], s["P"], s["N"], s["G"], 1)[1][3], int(s["aps"])) for s in shapes}


def test_every_form_the_plan_can_pick_has_a_shape():
    """the scan is compiled once per (lanes_per_row, N == 16 lanes_per_row, A per state): the forms of SHAPES are the forms the plan hands out over every
    served N, so a form added to the plan fails here until a shape reaches it -- and so does taking any one of the twelve later shapes away"""
    reachable = set()
    for N in range(16, 257, 16):
        rc, p = _plan(4, 64, N, 1, 1)
        assert rc == OK and p[3] == np_ssm.lanes_per_row(N)
        reachable |= {(p[3], N == 16 * p[3], aps) for aps in (0, 1)}
    assert len(reachable) == 16 and _forms(SHAPES.values()) == reachable
    for name in SHAPES:
        if name not in FIRST_SEVEN:
            assert _forms(s for n, s in SHAPES.items() if n != name) != reachable, name
    for lp in (2, 4, 8, 16):
        rows = [s["H"] * s["P"] for s in SHAPES.values() if np_ssm.lanes_per_row(s["N"]) == lp]
        assert any(r > 256 // lp for r in rows), ("no shape with more than one workgroup", lp)
        assert any(r % (256 // lp) for r in rows), ("no shape with a partly filled last workgroup", lp)
    assert any(s["H"] * s["P"] % 256 for s in SHAPES.values() if s["N"] == 16)


@pytest.mark.parametrize("name", ("mamba1_8", "n48", "n256", "n240_aps"))
def test_the_model_does_not_care_where_a_sequence_is_split(name):
    c = scan_case(name)
    for b, cut in SPLITS:
        (x, dt, A, B, Cc), k = _seq_args(c, b)
        y, h = np_ssm.scan_f32(x, dt, A, B, Cc, **k)
        y1, h1 = np_ssm.scan_f32(x[:cut], dt[:cut], A, B[:cut], Cc[:cut], **k)
        y2, h2 = np_ssm.scan_f32(x[cut:], dt[cut:], A, B[cut:], Cc[cut:], **dict(k, h0=h1))
        assert np.array_equal(np.concatenate([y1, y2]).view(np.uint32), y.view(np.uint32)) and np.array_equal(h2.view(np.uint32), h.view(np.uint32))


def _plan(n_head, P, N, G, n_seq):
    out = _lib.ggml_hip_ssm_plan_t()
    rc = _lib.lib().ggml_hip_ssm_scan_plan(n_head, P, N, G, n_seq, C.byref(out))
    return rc, (out.form, out.launches, out.slices, out.lanes_per_row, out.rows_per_workgroup, out.workgroups)


def test_the_plan_is_a_function_of_its_arguments_alone():
    L = _lib.lib()
    seen = {}
    for rep in range(2):
        for n_head, P, N, G, n_seq in ((8, 1, 16, 1, 1), (264, 1, 16, 1, 9), (4, 64, 128, 2, 9), (4, 5, 48, 2, 9), (64, 64, 256, 8, 4096), (3, 7, 80, 3, 2)):
            rc, p = _plan(n_head, P, N, G, n_seq)
            assert rc == OK
            lp = 1
            while lp < N // 16:
                lp *= 2
            rows = 256 // lp
            assert p == (1, 1, N // 16, lp, rows, -(-n_head * P // rows) * n_seq)
            assert seen.setdefault((n_head, P, N, G, n_seq), p) == p
            if rep == 0:                                            # (other host entries in between change nothing)
                assert L.ggml_hip_ssm_state_bytes(n_head, P, N) == n_head * P * N * 4
    assert [_plan(4, 64, n, 1, 1)[1][3] for n in (16, 32, 48, 64, 80, 128, 144, 256)] == [1, 2, 4, 4, 8, 8, 16, 16]
    for bad in ((0, 64, 128, 1, 1), (4, 0, 128, 1, 1), (4, 257, 128, 1, 1), (4, 64, 0, 1, 1), (4, 64, 24, 1, 1), (4, 64, 272, 1, 1), (4, 64, 128, 3, 1),
                (4, 64, 128, 0, 1), (4, 64, 128, 1, 0), (4, 64, 128, 1, 4097), ((1 << 20) + 1, 1, 16, 1, 1)):
        assert _plan(*bad)[0] == ERR_SHAPE, bad
    assert L.ggml_hip_ssm_scan_plan(4, 64, 128, 1, 1, None) == ERR_ARG
    assert L.ggml_hip_ssm_state_bytes(4, 64, 24) == 0 and L.ggml_hip_ssm_state_bytes(4, 300, 16) == 0
    assert L.ggml_hip_ssm_conv_state_bytes(1028, 4) == 3 * 1028 * 4 and L.ggml_hip_ssm_conv_state_bytes(5, 2) == 20
    assert L.ggml_hip_ssm_conv_state_bytes(5, 1) == 0 and L.ggml_hip_ssm_conv_state_bytes(5, 5) == 0 and L.ggml_hip_ssm_conv_state_bytes(0, 4) == 0


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _conv_rc(**kw):
    """one conv call on pointers that are no device memory; every caller changes at least one argument into something a host check refuses"""
    assert kw
    a = dict(x=FAKE, ldx=64, w=FAKE, bias=None, act=0, n_ch=64, d_conv=4, n_seq=3, q_start=FAKE, n_tokens_max=16, len=FAKE, slot=FAKE, state=FAKE,
             nb_slot=3 * 64 * 4, n_slots=4, dst=FAKE, ldd=64)
    a.update(kw)
    return _lib.lib().ggml_hip_ssm_conv_ragged_dev(_p(a["x"]), a["ldx"], _p(a["w"]), _p(a["bias"]), a["act"], a["n_ch"], a["d_conv"], a["n_seq"], _p(a["q_start"]),
                                                   a["n_tokens_max"], _p(a["len"]), _p(a["slot"]), _p(a["state"]), a["nb_slot"], a["n_slots"], _p(a["dst"]),
                                                   a["ldd"], None)


def _scan_rc(**kw):
    """one scan call on pointers that are no device memory; every caller changes at least one argument into something a host check refuses"""
    assert kw
    a = dict(x=FAKE, ldx_tok=64, ldx_head=8, dt=FAKE, ld_dt=8, dt_bias=None, A=FAKE, a_ld=1, aps=0, B=FAKE, C=FAKE, ld_bc=32, D=None, n_head=8, P=8, N=16, G=2,
             n_seq=3, q_start=FAKE, n_tokens_max=16, len=FAKE, slot=FAKE, state=FAKE, nb_slot=8 * 8 * 16 * 4, n_slots=4, dst=FAKE, ldd_tok=64, ldd_head=8)
    a.update(kw)
    return _lib.lib().ggml_hip_ssm_scan_ragged_dev(_p(a["x"]), a["ldx_tok"], a["ldx_head"], _p(a["dt"]), a["ld_dt"], _p(a["dt_bias"]), _p(a["A"]), a["a_ld"],
                                                   a["aps"], _p(a["B"]), _p(a["C"]), a["ld_bc"], _p(a["D"]), a["n_head"], a["P"], a["N"], a["G"], a["n_seq"],
                                                   _p(a["q_start"]), a["n_tokens_max"], _p(a["len"]), _p(a["slot"]), _p(a["state"]), a["nb_slot"], a["n_slots"],
                                                   _p(a["dst"]), a["ldd_tok"], a["ldd_head"], None)


def _batch_refusals(rc, slot_bytes):
    """the refusals both entries share (ssm.cpp check_ssm_batch), each on an otherwise valid call"""
    for n_seq in (0, -1, 4097):
        assert rc(n_seq=n_seq) == ERR_SHAPE, n_seq
    assert rc(q_start=None) == ERR_ARG
    assert rc(q_start=FAKE + 2) == ERR_SHAPE
    assert rc(n_tokens_max=-1) == ERR_ARG
    assert rc(n_tokens_max=(1 << 20) + 1) == ERR_SHAPE
    assert rc(len=None) == ERR_ARG
    assert rc(slot=None) == ERR_ARG
    assert rc(len=FAKE + 2) == ERR_SHAPE
    assert rc(slot=FAKE + 1) == ERR_SHAPE
    assert rc(n_slots=0) == ERR_ARG
    assert rc(n_slots=-3) == ERR_ARG
    assert rc(nb_slot=slot_bytes - 16) == ERR_SHAPE                  # below the slot's bytes
    assert rc(nb_slot=slot_bytes + 8) == ERR_SHAPE                   # no multiple of 16
    assert rc(nb_slot=1 << 30, n_slots=1 << 20) == ERR_SHAPE         # a pool beyond 2^48 bytes
    assert rc(state=None) == ERR_ARG
    assert rc(state=FAKE + 4) == ERR_SHAPE


def test_conv_refusals_need_no_device():
    """(every call below is refused by the host check its line names: its pointers are no device memory, so none may get as far as a launch)"""
    rc = _conv_rc
    _batch_refusals(rc, 3 * 64 * 4)
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
    assert rc(d_conv=2, nb_slot=64 * 4 - 16) == ERR_SHAPE            # (the slot's bytes follow d_conv)


def test_scan_refusals_need_no_device():
    """(every call below is refused by the host check its line names: its pointers are no device memory, so none may get as far as a launch)"""
    rc = _scan_rc
    _batch_refusals(rc, 8 * 8 * 16 * 4)
    assert rc(n_head=0) == ERR_SHAPE
    assert rc(n_head=(1 << 20) + 1) == ERR_SHAPE
    for P in (0, 257, -1):
        assert rc(P=P) == ERR_SHAPE, P
    for N in (0, 8, 24, 272):
        assert rc(N=N) == ERR_SHAPE, N
    for G in (0, 3, 16):
        assert rc(G=G) == ERR_SHAPE, G
    for aps in (2, -1):
        assert rc(aps=aps) == ERR_ARG, aps
    assert rc(ldx_head=7) == ERR_SHAPE
    assert rc(ldd_head=7) == ERR_SHAPE
    assert rc(ldx_tok=7) == ERR_SHAPE
    assert rc(ldd_tok=-8) == ERR_SHAPE
    assert rc(ld_dt=7) == ERR_SHAPE
    assert rc(a_ld=0) == ERR_SHAPE
    assert rc(aps=1, a_ld=15) == ERR_SHAPE                           # per state: at least N
    assert rc(aps=1, a_ld=18) == ERR_SHAPE                           # ... and a multiple of 4
    assert rc(aps=1, a_ld=16, A=FAKE + 4) == ERR_SHAPE               # ... and 16-byte aligned
    assert rc(ld_bc=31) == ERR_SHAPE                                 # below G * N
    assert rc(ld_bc=34) == ERR_SHAPE                                 # no multiple of 4
    for name in ("x", "dt", "A", "B", "C", "dst"):
        assert rc(**{name: None}) == ERR_ARG, name
    for name in ("B", "C"):
        assert rc(**{name: FAKE + 4}) == ERR_SHAPE, name
    for name in ("x", "dt", "dt_bias", "A", "D", "dst"):
        assert rc(**{name: FAKE + 2}) == ERR_SHAPE, name
    assert rc(N=32, ld_bc=64, nb_slot=8 * 8 * 16 * 4) == ERR_SHAPE   # (the slot's bytes follow the shape)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


def _stream(dev):
    return C.c_void_p(dev.torch.cuda.current_stream().cuda_stream)


def _up(dev, a):
    """a numpy array of 4-byte elements -> an int32 tensor on the device holding its bits"""
    return dev.torch.from_numpy(np.ascontiguousarray(a).view(np.int32).reshape(-1).copy()).cuda()


def _bits(t):
    return t.cpu().numpy().view(np.uint32)


class Pool:
    """a pool image on the host: guards, n_slots slots `stride` elements apart with `elems` used; everything else the sentinel"""

    def __init__(self, n_slots, elems, pad):
        self.n_slots, self.elems, self.stride = n_slots, elems, elems + pad
        assert (self.stride * 4) % 16 == 0
        self.image = np.full(GUARD + n_slots * self.stride + GUARD, SENTINEL, np.uint32)

    def slot(self, img, s):
        lo = GUARD + s * self.stride
        return img[lo:lo + self.elems]

    def put(self, s, values):
        self.slot(self.image, s)[:] = np.ascontiguousarray(values, F).reshape(-1).view(np.uint32)

    def put_nan(self, s):
        self.slot(self.image, s)[:] = NAN_BYTES

    def ptr(self, t):
        return t.data_ptr() + 4 * GUARD

    @property
    def nb_slot(self):
        return 4 * self.stride


def _batch_pool(contents, elems, pad, k=BATCH_1):
    """the pool of the batch: every slot holds contents[s], the fresh sequences' slots NaN bytes"""
    pool = Pool(N_SLOTS, elems, pad)
    for s in range(N_SLOTS):
        pool.put(s, contents[s])
    for b in range(k.n_seq):
        if k.d_len[b] == 0 and 0 <= k.slot[b] < N_SLOTS:
            pool.put_nan(int(k.slot[b]))
    return pool


def _rows_and_pool_of_the_batch(k, y, after, pool, elems):
    """what both entries owe a batch beside the served sequences' values.  Rows (y: uint32 [n_tokens_max, ...], preloaded with the sentinel): a slot id
    outside the pool gives +0.0f, and no row but a served or zeroed sequence's is written -- not the rows nobody owns, not those an absent sequence names.
    The pool: the fresh served sequences' slots were NaN bytes before the call, and only the served sequences' slots changed -- not the gaps, the guards,
    the idle and the absent sequences' slots.  -> the mask of the owned rows"""
    owned = np.zeros(k.n_tokens_max, bool)
    changed = np.zeros(after.size, bool)
    for b in k.served:
        lo, hi = k.rows(b)
        owned[lo:hi] = True
        s0 = GUARD + int(k.slot[b]) * pool.stride
        changed[s0:s0 + elems] = True
        if k.d_len[b] == 0:
            assert (pool.slot(pool.image, int(k.slot[b])) == NAN_BYTES).all(), b
    for b in k.zeroed:
        lo, hi = k.rows(b)
        owned[lo:hi] = True
        assert not y[lo:hi].any(), b
    assert (y[~owned] == SENTINEL).all(), "a row of no present sequence was written"
    assert np.array_equal(after[~changed], pool.image[~changed]), "state outside the served slots was written"
    return owned


def _scan_call(dev, c, q_start, d_len, slot, pool, n_tokens_max, row0=0, pad_head=0, pad_tok=0, pad_bc=0, pad_head_d=None, pad_tok_d=None, pad_dt=0, pad_a=0,
               with_D=True, with_bias=True):
    """one scan call over rows [row0, row0 + n_tokens_max) of the case's packed inputs, with the given paddings of the strides: pad_head / pad_tok of x
    (and of dst, unless pad_head_d / pad_tok_d give dst its own), pad_bc of B and C, pad_dt of dt (ld_dt = n_head + pad_dt), pad_a of A (a_ld = N + pad_a
    per state, 1 + pad_a per head); every gap of an input holds 3.0e38.  with_D / with_bias False: a null pointer.
    -> (dst bits [n_tokens_max][H][P], the pool image after the call); the guards and the paddings of dst and every input are checked here"""
    H, P, N, G = c["H"], c["P"], c["N"], c["G"]
    n = n_tokens_max
    sl = slice(row0, row0 + n)
    ldh, ldt = P + pad_head, H * (P + pad_head) + pad_tok
    ldh_d = P + (pad_head if pad_head_d is None else pad_head_d)
    ldt_d = H * ldh_d + (pad_tok if pad_tok_d is None else pad_tok_d)
    x = np.full((n, ldt), 3.0e38, F)
    x[:, :H * ldh].reshape(n, H, ldh)[:, :, :P] = c["x"][sl]
    ld_bc = 2 * G * N + pad_bc
    bc = np.full((n, ld_bc), 3.0e38, F)
    bc[:, :G * N] = c["B"][sl].reshape(n, G * N)
    bc[:, G * N:2 * G * N] = c["C"][sl].reshape(n, G * N)
    ld_dt = H + pad_dt
    dt = np.full((n, ld_dt), 3.0e38, F)
    dt[:, :H] = c["dt"][sl]
    a_ld = (N if c["aps"] else 1) + pad_a
    A = np.full((H, a_ld), 3.0e38, F)
    A[:, :a_ld - pad_a] = c["A"].reshape(H, -1)
    d_x, d_bc, d_dt, d_A = _up(dev, x), _up(dev, bc), _up(dev, dt), _up(dev, A)
    d_D, d_db = _up(dev, c["D"]), _up(dev, c["dt_bias"])
    d_q, d_l, d_s = _up(dev, np.asarray(q_start, np.int32)), _up(dev, np.asarray(d_len, np.int32)), _up(dev, np.asarray(slot, np.int32))
    d_pool = _up(dev, pool.image)
    dst = dev.torch.full((GUARD + max(n, 1) * ldt_d + GUARD,), SENTINEL, dtype=dev.torch.int32, device="cuda")
    rc = _lib.lib().ggml_hip_ssm_scan_ragged_dev(
        _p(d_x.data_ptr()), ldt, ldh, _p(d_dt.data_ptr()), ld_dt, _p(d_db.data_ptr()) if with_bias else None, _p(d_A.data_ptr()), a_ld, int(c["aps"]),
        _p(d_bc.data_ptr()), _p(d_bc.data_ptr() + 4 * G * N), ld_bc, _p(d_D.data_ptr()) if with_D else None, H, P, N, G, len(slot), _p(d_q.data_ptr()), n,
        _p(d_l.data_ptr()), _p(d_s.data_ptr()), _p(pool.ptr(d_pool)), pool.nb_slot, pool.n_slots, _p(dst.data_ptr() + 4 * GUARD), ldt_d, ldh_d, _stream(dev))
    assert rc == 0, _lib.lib().ggml_hip_last_error()
    dev.torch.cuda.synchronize()
    out = _bits(dst)
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + n * ldt_d:] == SENTINEL).all(), "guards of dst written"
    body = out[GUARD:GUARD + n * ldt_d].reshape(n, ldt_d)
    assert (body[:, H * ldh_d:] == SENTINEL).all(), "token padding of dst written"
    body = body[:, :H * ldh_d].reshape(n, H, ldh_d)
    assert (body[:, :, P:] == SENTINEL).all(), "head padding of dst written"
    for t, want in ((d_x, x), (d_bc, bc), (d_dt, dt), (d_A, A)):
        assert np.array_equal(_bits(t), want.view(np.uint32).reshape(-1)), "an input was written"
    return body[:, :, :P], _bits(d_pool)


def _scan_batch(dev, name, k, with_D=True, with_bias=True):
    """the batch call of a shape: dst with paddings of its own (ldd_head != ldx_head, ldd_tok != ldx_tok), ld_dt above n_head, a_ld above N (by 4 or 8) or
    3 for one A per head.  Served sequences against float64 under the bar, then what _rows_and_pool_of_the_batch states.  -> (y, after, pool)"""
    c = scan_case(name)
    H, P, N = c["H"], c["P"], c["N"]
    elems = H * P * N
    pool = _batch_pool(c["pool"].reshape(N_SLOTS, -1), elems, 8, k)
    pad_a = (4 if N % 32 else 8) if c["aps"] else 2
    y, after = _scan_call(dev, c, k.q_start, k.d_len, k.slot, pool, k.n_tokens_max, pad_head=3, pad_tok=5, pad_bc=4, pad_head_d=1, pad_tok_d=2, pad_dt=3,
                          pad_a=pad_a, with_D=with_D, with_bias=with_bias)
    for b in k.served:
        lo, hi = k.rows(b)
        ref_y, ref_h, bar_y, bar_h = scan_ref(name, b, k, with_D, with_bias)
        got_y = y[lo:hi].view(F).astype(np.float64)
        got_h = pool.slot(after, int(k.slot[b])).view(F).astype(np.float64).reshape(H, P, N)
        ry, rh = float((np.abs(got_y - ref_y) / bar_y).max()), float((np.abs(got_h - ref_h) / bar_h).max())
        print(f"{name} seq {b}: kernel / bar  y {ry:.3f}  state {rh:.3f}")
        assert np.isfinite(got_y).all() and np.isfinite(got_h).all() and ry <= 1.0 and rh <= 1.0, (name, b, ry, rh)
    _rows_and_pool_of_the_batch(k, y, after, pool, elems)
    return y, after, pool


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_scan_over_the_ragged_batch(dev, name):
    c = scan_case(name)
    elems = c["H"] * c["P"] * c["N"]
    # rows: served sequences against float64 under the bar; a slot id outside the pool: +0.0f; everyone else's rows: not written.  The pool: only the
    # served sequences' slots changed
    y, after, pool = _scan_batch(dev, name, BATCH_1)

    # (i) + (iii): every served sequence alone -- n_seq = 1, another slot number in another pool, other strides (of x, dst, dt and A), another n_tokens_max
    for b in SERVED:
        lo, hi = _rows(b)
        one = Pool(3, elems, 0)
        one.put(2, c["pool"][SLOT[b]]) if D_LEN[b] else one.put_nan(2)
        y1, after1 = _scan_call(dev, c, [0, hi - lo], [D_LEN[b]], [2], one, hi - lo + 1, row0=lo)
        assert np.array_equal(y1[:hi - lo], y[lo:hi]), ("rows alone", name, b)
        assert np.array_equal(one.slot(after1, 2), pool.slot(after, int(SLOT[b]))), ("state alone", name, b)
    # (ii): a sequence split over two calls at any point
    for b, cut in SPLITS:
        lo, hi = _rows(b)
        two = Pool(2, elems, 4)
        two.put(1, c["pool"][SLOT[b]]) if D_LEN[b] else two.put_nan(1)
        ya, mid = _scan_call(dev, c, [0, cut], [D_LEN[b]], [1], two, cut, row0=lo, pad_head=1)
        two.image = mid
        yb, end = _scan_call(dev, c, [0, hi - lo - cut], [int(D_LEN[b]) + cut], [1], two, hi - lo - cut, row0=lo + cut)
        assert np.array_equal(np.concatenate([ya, yb]), y[lo:hi]), ("rows split", name, b, cut)
        assert np.array_equal(two.slot(end, 1), pool.slot(after, int(SLOT[b]))), ("state split", name, b, cut)


@pytest.mark.gpu
@pytest.mark.parametrize("with_D,with_bias", OPTIONAL_OPERANDS)
@pytest.mark.parametrize("name", OPTIONAL_SHAPES)
def test_scan_without_the_optional_operands(dev, name, with_D, with_bias):
    """D and / or dt_bias null on the device: the statement without the term, under the same bar (its CPU twin holds the model and the mutants to it)"""
    _scan_batch(dev, name, BATCH_1, with_D=with_D, with_bias=with_bias)


@pytest.mark.gpu
@pytest.mark.parametrize("name", SECOND_BATCH_SHAPES)
def test_scan_over_the_second_batch(dev, name):
    _scan_batch(dev, name, BATCH_2)


# ---------------------------------------------------------------- the conv
@functools.lru_cache(maxsize=None)
def conv_case(n_ch, d_conv):
    rng = np.random.default_rng(1000 * d_conv + n_ch)
    c = dict(n_ch=n_ch, d_conv=d_conv)
    c["x"] = rng.normal(0.0, 1.0, (N_TOKENS_MAX, n_ch)).astype(F)
    c["w"] = rng.normal(0.0, 0.7, (n_ch, d_conv)).astype(F)
    c["bias"] = rng.normal(0.0, 0.5, n_ch).astype(F)
    c["pool"] = rng.normal(0.0, 1.0, (N_SLOTS, d_conv - 1, n_ch)).astype(F)
    return c


def _conv_call(dev, c, pool, bias, act, pad_x=0, pad_d=0, in_place=False, k=BATCH_1):
    n_ch, K, n = c["n_ch"], c["d_conv"], k.n_tokens_max
    ldx = n_ch + pad_x
    ldd = ldx if in_place else n_ch + pad_d
    x = np.full((n, ldx), 3.0e38, F)
    x[:, :n_ch] = c["x"][:n]
    xbuf = np.full(GUARD + n * ldx + GUARD, SENTINEL, np.uint32)
    xbuf[GUARD:-GUARD] = x.view(np.uint32).reshape(-1)
    d_x, d_w, d_b = _up(dev, xbuf), _up(dev, c["w"]), _up(dev, c["bias"])
    d_q, d_l, d_s = _up(dev, k.q_start), _up(dev, k.d_len), _up(dev, k.slot)
    d_pool = _up(dev, pool.image)
    dst = d_x if in_place else dev.torch.full((GUARD + n * ldd + GUARD,), SENTINEL, dtype=dev.torch.int32, device="cuda")
    rc = _lib.lib().ggml_hip_ssm_conv_ragged_dev(_p(d_x.data_ptr() + 4 * GUARD), ldx, _p(d_w.data_ptr()), _p(d_b.data_ptr()) if bias else None, int(act), n_ch, K,
                                                 k.n_seq, _p(d_q.data_ptr()), n, _p(d_l.data_ptr()), _p(d_s.data_ptr()), _p(pool.ptr(d_pool)),
                                                 pool.nb_slot, pool.n_slots, _p(dst.data_ptr() + 4 * GUARD), ldd, _stream(dev))
    assert rc == 0, _lib.lib().ggml_hip_last_error()
    dev.torch.cuda.synchronize()
    out = _bits(dst)
    assert (out[:GUARD] == SENTINEL).all() and (out[-GUARD:] == SENTINEL).all(), "guards of dst written"
    body = out[GUARD:-GUARD].reshape(n, ldd)
    if in_place:
        assert np.array_equal(body[:, n_ch:], x.view(np.uint32)[:, n_ch:]), "padding columns written"
    else:
        assert (body[:, n_ch:] == SENTINEL).all(), "padding columns written"
        assert np.array_equal(_bits(d_x), xbuf), "d_x written"
    return body[:, :n_ch], _bits(d_pool)


def _conv_batch(dev, n_ch, d_conv, k):
    """the conv over batch k, every assertion of the entry: (act 0, bias) and (act 0, no bias) and their slots bit for bit, rows and pool as
    _rows_and_pool_of_the_batch states, in place, (act 1, no bias) and (act 1, bias) within 3 * 2^-24 relative of the silu of the conv's bits"""
    c = conv_case(n_ch, d_conv)
    n = k.n_tokens_max
    elems = (d_conv - 1) * n_ch
    pad = (-elems) % 4 + 4                                           # (a slot stride that is a multiple of 16 bytes, above the slot's bytes)
    pool = _batch_pool(c["pool"].reshape(N_SLOTS, -1), elems, pad, k)

    def statement(b, bias):
        lo, hi = k.rows(b)
        return np_ssm.conv_f32(c["x"][lo:hi], c["w"], c["bias"] if bias else None, None if k.d_len[b] == 0 else c["pool"][k.slot[b]])

    y, after = _conv_call(dev, c, pool, bias=True, act=0, pad_x=3, pad_d=6, k=k)
    for b in k.served:
        lo, hi = k.rows(b)
        want, want_slot = statement(b, True)
        assert np.array_equal(y[lo:hi], want.view(np.uint32)), ("rows", b)
        assert np.array_equal(pool.slot(after, int(k.slot[b])), want_slot.view(np.uint32).reshape(-1)), ("slot", b)
    owned = _rows_and_pool_of_the_batch(k, y, after, pool, elems)
    # in place: d_dst == d_x gives the same rows (the rows nobody owns keep x) and the same pool
    y2, after2 = _conv_call(dev, c, pool, bias=True, act=0, pad_x=3, in_place=True, k=k)
    assert np.array_equal(y2[owned], y[owned]) and np.array_equal(y2[~owned], c["x"][:n].view(np.uint32)[~owned]) and np.array_equal(after2, after)
    # act = 0, no bias: bit for bit too; the slot does not see the bias
    y4, after4 = _conv_call(dev, c, pool, bias=False, act=0, pad_d=1, k=k)
    for b in k.served:
        lo, hi = k.rows(b)
        assert np.array_equal(y4[lo:hi], statement(b, False)[0].view(np.uint32)), ("rows without bias", b)
    assert np.array_equal(y4[~owned], y[~owned]) and np.array_equal(after4, after)
    # act = 1, without and with bias: within 3 * 2^-24 relative of the silu of the conv's bits; the slot does not see act or bias
    for bias in (False, True):
        y3, after3 = _conv_call(dev, c, pool, bias=bias, act=1, k=k)
        worst = 0.0
        for b in k.served:
            lo, hi = k.rows(b)
            ref = np_ssm.silu64(statement(b, bias)[0])
            worst = max(worst, float((np.abs(y3[lo:hi].view(F).astype(np.float64) - ref) / np.abs(ref)).max()))
        print(f"n_ch {n_ch} d_conv {d_conv} bias {int(bias)}: silu relative error / 2^-24 = {worst / U:.3f}")
        assert worst <= 3.0 * U, worst / U
        assert np.array_equal(y3[~owned], y[~owned]) and np.array_equal(after3, after)


@pytest.mark.gpu
@pytest.mark.parametrize("d_conv", (2, 3, 4))
@pytest.mark.parametrize("n_ch", (1, 5, 64, 1028))
def test_conv_over_the_ragged_batch(dev, n_ch, d_conv):
    _conv_batch(dev, n_ch, d_conv, BATCH_1)


@pytest.mark.gpu
@pytest.mark.parametrize("d_conv", (2, 3, 4))
@pytest.mark.parametrize("n_ch", (5, 1028))
def test_conv_over_the_second_batch(dev, n_ch, d_conv):
    _conv_batch(dev, n_ch, d_conv, BATCH_2)


# ---------------------------------------------------------------- the python face, a captured step, no tokens at all
@pytest.mark.gpu
def test_a_captured_step_follows_the_batch_and_no_tokens_is_accepted(dev):
    torch = dev.torch
    c, cc = scan_case("mamba1_8"), conv_case(64, 4)
    H, P, N, G = c["H"], c["P"], c["N"], c["G"]
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    x, dt, A, B, Cc, D, db = (t(c[k]) for k in ("x", "dt", "A", "B", "C", "D", "dt_bias"))
    cx, cw, cb = t(cc["x"]), t(cc["w"]), t(cc["bias"])
    pool0, cpool0 = t(c["pool"].reshape(N_SLOTS, -1)), t(cc["pool"].reshape(N_SLOTS, -1))
    # the second batch: the sequences moved, the fresh ones continued and the other way round, the slots permuted
    q2 = np.array([0, 9, 9, 11, 141, 142, 143, 145, 148, 150], np.int32)
    len2 = np.array([0, 3, 1, 0, 2, 0, 0, 5, 1], np.int32)
    slot2 = np.array([3, 1, 8, 6, -1, 0, 2, 9, N_SLOTS], np.int32)

    def step(q, ln, sl, pool, cpool, y, cy):
        dev.ssm_scan_ragged(x, dt, A, B, Cc, q, ln, sl, pool, dt_bias=db, D=D, out=y)
        dev.ssm_conv_ragged(cx, cw, q, ln, sl, cpool, bias=cb, act=True, out=cy)

    def fresh():
        return pool0.clone(), cpool0.clone(), torch.zeros_like(x), torch.zeros_like(cx)

    want = {}
    for key, (q, ln, sl) in (("one", (Q_START, D_LEN, SLOT)), ("two", (q2, len2, slot2))):
        pool, cpool, y, cy = fresh()
        step(t(q), t(ln), t(sl), pool, cpool, y, cy)
        torch.cuda.synchronize()
        want[key] = [_bits(v) for v in (pool, cpool, y, cy)]
    assert not all(np.array_equal(a, b) for a, b in zip(want["one"], want["two"]))
    d_q, d_l, d_s = t(Q_START), t(D_LEN), t(SLOT)
    pool, cpool, y, cy = fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(d_q, d_l, d_s, pool, cpool, y, cy)
    torch.cuda.current_stream().wait_stream(s)
    for key, (q, ln, sl) in (("two", (q2, len2, slot2)), ("one", (Q_START, D_LEN, SLOT))):
        d_q.copy_(t(q)), d_l.copy_(t(ln)), d_s.copy_(t(sl))
        for dst, src in zip((pool, cpool, y, cy), fresh()):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip((pool, cpool, y, cy), want[key]):
            assert np.array_equal(_bits(got), w), key
    # n_tokens_max = 0: accepted, nothing written
    before = [_bits(v) for v in (pool, cpool, y, cy)]
    dev.ssm_scan_ragged(x, dt, A, B, Cc, d_q, d_l, d_s, pool, dt_bias=db, D=D, n_tokens_max=0, out=y)
    dev.ssm_conv_ragged(cx, cw, d_q, d_l, d_s, cpool, bias=cb, n_tokens_max=0, out=cy)
    torch.cuda.synchronize()
    for got, w in zip((pool, cpool, y, cy), before):
        assert np.array_equal(_bits(got), w)


@pytest.mark.gpu
def test_the_python_face_on_the_views_of_a_mamba2_block(dev):
    """what a Mamba-2 block hands over: ONE [n_tokens, d_inner + 2 G N] tensor xBC, convolved in place, and the scan on views of it -- x, B and C with the
    token stride of xBC, dt and out as views of wider tensors, a state pool with a slot stride above the slot, A one value per head.  Every stride the
    wrapper derives is pinned: the rows and the final slots are bit for bit those of the raw entry on contiguous copies of the conv's output, and under
    the float64 bar computed from that output"""
    torch = dev.torch
    name = "mamba2_g2"
    c = scan_case(name)
    H, P, N, G = c["H"], c["P"], c["N"], c["G"]
    d_inner, gn, elems, n = H * P, G * N, H * P * N, N_TOKENS_MAX
    assert (d_inner, 2 * gn) == (256, 512)
    cc = conv_case(d_inner + 2 * gn, 4)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_q, d_l, d_s = t(Q_START), t(D_LEN), t(SLOT)
    fresh = [int(SLOT[b]) for b in SERVED if D_LEN[b] == 0]

    def pool_of(contents, pad):                                      # [N_SLOTS, elements] as a view of a wider tensor; the fresh slots hold NaN bytes
        wide = torch.full((N_SLOTS, contents.shape[1] + pad), float("nan"), dtype=torch.float32, device="cuda")
        view = wide[:, :contents.shape[1]]
        view.copy_(t(contents))
        view.view(torch.int32)[fresh] = -1
        return view

    cpool, pool = pool_of(cc["pool"].reshape(N_SLOTS, -1), 4), pool_of(c["pool"].reshape(N_SLOTS, -1), 8)
    xBC = t(cc["x"])
    assert tuple(xBC.shape) == (n, 768)
    dev.ssm_conv_ragged(xBC, t(cc["w"]), d_q, d_l, d_s, cpool, bias=t(cc["bias"]), act=True, out=xBC)
    x = xBC[:, :d_inner].unflatten(1, (H, P))
    B = xBC[:, d_inner:d_inner + gn].unflatten(1, (G, N))
    Cc = xBC[:, d_inner + gn:].unflatten(1, (G, N))
    dt = torch.full((n, H + 3), 3.0e38, dtype=torch.float32, device="cuda")[:, :H]
    dt.copy_(t(c["dt"]))
    wide = torch.full((n, H, P + 8), float("nan"), dtype=torch.float32, device="cuda")
    wide.view(torch.int32).fill_(SENTINEL)
    out = wide[:, :, :P]
    assert (x.stride(0), x.stride(1), out.stride(0), out.stride(1), dt.stride(0), pool.stride(0)) == (768, P, H * (P + 8), P + 8, H + 3, elems + 8)
    got = dev.ssm_scan_ragged(x, dt, t(c["A"]), B, Cc, d_q, d_l, d_s, pool, dt_bias=t(c["dt_bias"]), D=t(c["D"]), out=out)
    torch.cuda.synchronize()
    assert got is out
    conv = xBC.cpu().numpy()
    y, state = _bits(wide)[:, :, :P], _bits(pool.contiguous())
    assert (_bits(wide)[:, :, P:] == SENTINEL).all(), "the padding of out was written"
    # the raw entry on contiguous copies of the conv's output, over the same pool contents
    c2 = dict(c, x=conv[:, :d_inner].reshape(n, H, P).copy(), B=conv[:, d_inner:d_inner + gn].reshape(n, G, N).copy(),
              C=conv[:, d_inner + gn:].reshape(n, G, N).copy())
    raw_pool = _batch_pool(c["pool"].reshape(N_SLOTS, -1), elems, 0)
    y_raw, after = _scan_call(dev, c2, Q_START, D_LEN, SLOT, raw_pool, n)
    assert np.array_equal(y, y_raw), "rows"
    for b in SERVED:
        lo, hi = _rows(b)
        assert np.array_equal(state[int(SLOT[b])], raw_pool.slot(after, int(SLOT[b]))), ("slot", b)
        a, kw = _seq_args(c2, b)
        ref_y, ref_h, bar_y, bar_h = np_ssm.scan_f64(*a, want_bar=True, **kw)
        got_y, got_h = y[lo:hi].view(F).astype(np.float64), state[int(SLOT[b])].view(F).astype(np.float64).reshape(H, P, N)
        ry, rh = float((np.abs(got_y - ref_y) / bar_y).max()), float((np.abs(got_h - ref_h) / bar_h).max())
        print(f"{name} on the conv's output, seq {b}: kernel / bar  y {ry:.3f}  state {rh:.3f}")
        assert np.isfinite(got_y).all() and np.isfinite(got_h).all() and ry <= 1.0 and rh <= 1.0, (b, ry, rh)
    _rows_and_pool_of_the_batch(BATCH_1, y, after, raw_pool, elems)
    unserved = [s for s in range(N_SLOTS) if s not in [int(SLOT[b]) for b in SERVED]]
    assert np.array_equal(state[unserved], raw_pool.image[GUARD:GUARD + N_SLOTS * elems].reshape(N_SLOTS, elems)[unserved]), "a slot of no served sequence"
