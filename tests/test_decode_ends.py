"""The ends of a decode step (include/ggml_hip_ext.h: ggml_hip_get_rows_dev, ggml_hip_argmax_rows_dev, ggml_hip_sample_topk_dev and their host
queries; csrc/get_rows.hip, sample.hip, decode_ends.cpp).

Yardsticks:
  get_rows   bits: download the weight, dequantize its file-format rows with the library's own dequantize entry (F32: the rows; F16: numpy's
             exact widening), index on the host; a row of +0.0 for an id outside [0, M).  Compared as uint32, zero mismatches.
  ids        exact: tests/np_sampling.py topk_ids (test_moe_route.py's rule on a vocabulary).
  probs      np_sampling's float64 restatement on the device's own ids, inside the bound DERIVED in np_sampling's docstring (statistic <= 1).
  the pick   exact: n_keep and the token recomputed from the downloaded d_probs by the sequential f32 statement.
  the loop   a captured step get_rows -> rms_norm_mul -> mul_mat -> argmax whose token feeds the next replay: the tokens of eager steps and of
             a host loop that looks up and picks in numpy.
Shapes are the smallest at which each mechanism can go wrong: K of one and two k-blocks (super-blocks), M on both sides of the 256-row pad,
one id, a few, more than one workgroup's worth; vocabularies below / at / past one lane set, one chunk, two chunks; a chunk shorter than k.
The merge stage of the sampler is picked by size (launch_sample_topk: 1, 2, 4, ... 64 candidate keys per thread, and the k = 1 form): the
vocabularies above reach the rungs 1, 2 and 4; BIG_KINDS below are chosen by chunk count so that k = 64 fills every rung 1 .. 64 exactly
(4, 8, ... 128 chunks and 2^20 logits) and enters every rung 2 .. 64 at one chunk more than the rung below holds (5, 9, ... 129 chunks, the
last of one logit), with k = 1, 2 and 40 at three of them; test_the_cases_reach_every_form_of_the_merge counts the rungs.  Two further cases
have 130 and 4096 rows."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_sampling as S
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ggml_hip_get_rows_serves_for", "ggml_hip_get_rows_dev", "ggml_hip_topk_chunk", "ggml_hip_topk_work_size", "ggml_hip_argmax_rows_dev",
               "ggml_hip_sample_topk_dev")
F32, F16, Q4_0, Q4_1, Q4_2, Q4_3, Q5_0, Q5_1, Q8_0, Q8_1 = range(10)
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS, BF16 = _lib.Q2_K, _lib.Q3_K, _lib.Q4_K, _lib.Q5_K, _lib.Q6_K, _lib.IQ4_NL, _lib.IQ4_XS, _lib.BF16
SERVED = {"f32": F32, "f16": F16, "bf16": BF16, "q4_0": Q4_0, "q4_1": Q4_1, "q4_2": Q4_2, "q5_0": Q5_0, "q5_1": Q5_1, "q8_0": Q8_0, "iq4_nl": IQ4_NL,
          "iq4_xs": IQ4_XS, "q2_k": Q2_K, "q3_k": Q3_K, "q4_k": Q4_K, "q5_k": Q5_K, "q6_k": Q6_K}
MUST_SERVE = ("q4_0", "q4_1", "q5_0", "q5_1", "q8_0", "q4_2", "f16", "f32", "bf16", "q4_k", "q5_k", "q6_k", "iq4_nl")
SENTINEL = 0x7FC00123                                               # a NaN no kernel here produces
OK, ERR_TYPE, ERR_SHAPE, ERR_ARG = 0, -2, -3, -4
FAKE = 0x1000                                                       # a non-null pointer no refusal may touch


def _p(x):
    return None if x is None else C.c_void_p(int(x))


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name


def test_serves_for_over_the_type_table():
    L = _lib.lib()
    for name in MUST_SERVE:
        assert L.ggml_hip_get_rows_serves_for(SERVED[name]) == 1, name
    for name, t in SERVED.items():                                   # every type that can be a resident weight is reproducible from its planes
        assert L.ggml_hip_get_rows_serves_for(t) == 1, name
    for t in (Q4_3, Q8_1, 10, 11, 12, 13, 99, -1, 121, 200):         # no weight type: null slots, the integer types, no type at all
        assert L.ggml_hip_get_rows_serves_for(t) == 0, t


def test_the_chunk_and_the_work_size():
    L = _lib.lib()
    Cn = L.ggml_hip_topk_chunk()
    assert Cn >= 256 and Cn % 256 == 0
    ws = L.ggml_hip_topk_work_size
    rows, vocabs, ks = (1, 2, 9, 4096), (64, Cn - 1, Cn, Cn + 1, 3 * Cn, 1 << 20), (1, 2, 40, 64)
    for v in vocabs:
        for k in ks:
            sizes = [ws(r, v, k) for r in rows]
            assert all(s > 0 for s in sizes) and sizes == sorted(sizes), (v, k, sizes)
    for r in rows:
        for k in ks:
            sizes = [ws(r, v, k) for v in vocabs]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (r, k, sizes)
        for v in vocabs:
            sizes = [ws(r, v, k) for k in ks]
            assert sizes == sorted(sizes) and sizes[0] < sizes[-1], (r, v, sizes)
    # 0 only for refused shapes
    for r, v, k in ((0, 100, 1), (-1, 100, 1), (4097, 100, 1), (1, 0, 1), (1, (1 << 20) + 1, 1), (1, 100, 0), (1, 100, 65), (1, 5, 6)):
        assert ws(r, v, k) == 0, (r, v, k)
    assert ws(1, 1, 1) > 0 and ws(4096, 1 << 20, 64) > 0


def _get_rows_rc(w=FAKE, ids=FAKE, n_ids=2, dst=FAKE, ldd=64):
    return _lib.lib().ggml_hip_get_rows_dev(_p(w), _p(ids), n_ids, _p(dst), ldd, None)


def test_get_rows_refusals_need_no_device():
    """(ldd < K needs a weight to read K from: test_get_rows_refuses_a_short_ldd, on the GPU, where the refusal still comes before any launch)"""
    assert _get_rows_rc(n_ids=0) == OK
    assert _get_rows_rc(w=None, ids=None, dst=None, n_ids=0) == OK
    assert _get_rows_rc(w=None) == ERR_ARG
    assert _get_rows_rc(ids=None) == ERR_ARG
    assert _get_rows_rc(dst=None) == ERR_ARG
    assert _get_rows_rc(n_ids=-1) == ERR_ARG
    assert _get_rows_rc(n_ids=(1 << 20) + 1) == ERR_SHAPE
    assert _get_rows_rc(ids=FAKE + 2) == ERR_ARG                     # 4-byte alignment of d_ids and d_dst, refused before the weight is read
    assert _get_rows_rc(dst=FAKE + 1) == ERR_ARG


def _sample_rc(logits=FAKE, ld=100, n_rows=2, n_vocab=100, k=4, inv_temp=1.0, top_p=0.9, u=FAKE, ids=FAKE, probs=FAKE, token=FAKE, work=FAKE, work_bytes=None):
    if work_bytes is None:
        work_bytes = _lib.lib().ggml_hip_topk_work_size(n_rows, n_vocab, k)
    return _lib.lib().ggml_hip_sample_topk_dev(_p(logits), ld, n_rows, n_vocab, k, inv_temp, top_p, _p(u), _p(ids), _p(probs), _p(token), _p(work), work_bytes, None)


def _argmax_rc(logits=FAKE, ld=100, n_rows=2, n_vocab=100, ids=FAKE, work=FAKE, work_bytes=None):
    if work_bytes is None:
        work_bytes = _lib.lib().ggml_hip_topk_work_size(n_rows, n_vocab, 1)
    return _lib.lib().ggml_hip_argmax_rows_dev(_p(logits), ld, n_rows, n_vocab, _p(ids), _p(work), work_bytes, None)


def test_sampler_refusals_need_no_device():
    for rc in (_sample_rc, _argmax_rc):
        assert rc(n_rows=0) == OK
        assert rc(n_rows=-1, work_bytes=1 << 20) == ERR_SHAPE
        assert rc(n_rows=4097, work_bytes=1 << 30) == ERR_SHAPE
        assert rc(n_vocab=0, ld=0, work_bytes=1 << 20) == ERR_SHAPE
        assert rc(n_vocab=(1 << 20) + 1, ld=1 << 21, work_bytes=1 << 30) == ERR_SHAPE
        assert rc(ld=99) == ERR_SHAPE
        assert rc(logits=None) == ERR_ARG
        assert rc(ids=None) == ERR_ARG
        assert rc(work=None) == ERR_ARG
        need = _lib.lib().ggml_hip_topk_work_size(2, 100, 4 if rc is _sample_rc else 1)
        assert rc(work_bytes=need - 1) == ERR_ARG
    assert _sample_rc(k=0, work_bytes=1 << 20) == ERR_SHAPE
    assert _sample_rc(k=65, work_bytes=1 << 20) == ERR_SHAPE
    assert _sample_rc(k=6, n_vocab=5, ld=5, work_bytes=1 << 20) == ERR_SHAPE
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        assert _sample_rc(inv_temp=bad) == ERR_ARG, bad
    assert _sample_rc(probs=None) == ERR_ARG                         # a pick needs the probabilities it is defined on
    for name in ("logits", "ids", "u", "probs", "token"):            # 4-byte alignment of every f32 / int32 pointer; 8 bytes for the work buffer
        assert _sample_rc(**{name: FAKE + 2}) == ERR_ARG, name
    for name in ("logits", "ids"):
        assert _argmax_rc(**{name: FAKE + 2}) == ERR_ARG, name
    assert _sample_rc(work=FAKE + 4) == ERR_ARG and _argmax_rc(work=FAKE + 4) == ERR_ARG
    # (what is allowed -- probs without a pick, ids alone -- runs on the GPU below: with valid arguments the entry launches)


def test_the_restatement_on_rows_worked_by_hand():
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = np.array([[1, 3, 3, 2, 3, 0], [nan, -inf, nan, -inf, 5, nan], [0.0, -0.0, -1, 0.0, -0.0, -2], [nan] * 6], np.float32)
    assert S.topk_ids(rows, 4).tolist() == [[1, 2, 4, 3], [4, 1, 3, 0], [0, 1, 3, 4], [0, 1, 2, 3]]
    assert S.topk_ids(rows, 1)[:, 0].tolist() == [1, 4, 0, 0]
    l = np.array([[0.0, np.log(3.0), -50.0, np.log(3.0) - np.log(2.0)]], np.float32)
    ids = S.topk_ids(l, 3)
    assert ids.tolist() == [[1, 3, 0]]
    want = np.array([[0.5, 0.25, 1.0 / 6.0]]) / (0.5 + 0.25 + 1.0 / 6.0)              # 3 : 1.5 : 1
    assert np.allclose(S.probs64(l, ids, 1.0), want, rtol=1e-6)
    assert np.allclose(S.probs32(l, ids, 1.0), want, rtol=1e-6)
    assert np.allclose(S.probs64(l, ids, 2.0), np.array([[9.0, 2.25, 1.0]]) / 12.25, rtol=1e-6)     # temperature 0.5 squares the ratios
    p = np.array([0.5, 0.25, 0.125, 0.125], np.float32)              # (sums of these are exact)
    assert S.keep_pick(p, 0.0, 0.5) == (1, 0)                        # top_p cuts after rank 0: p_0 >= 0 already
    assert S.keep_pick(p, 0.5, 0.999) == (1, 0)
    assert S.keep_pick(p, 0.6, 0.0) == (2, 0)                        # u = 0: the target is 0, the first running sum exceeds it
    assert S.keep_pick(p, 0.6, 0.7) == (2, 1)                        # C = 0.75, target 0.525: 0.5 does not exceed it, 0.75 does
    assert S.keep_pick(p, 0.9, np.float32(0.9999999)) == (4, 3)      # 0.875 < 0.9: all four kept; u just under 1: the last rank
    assert S.keep_pick(p, 1.0, np.float32(0.9999999)) == (4, 3)      # top_p >= 1: k without summing
    assert S.keep_pick(p, 1.0, 0.5) == (4, 1)                        # target 0.5: the running sum must EXCEED it
    assert S.keep_pick(p, 0.75, 0.25) == (2, 0)
    assert S.keep_pick(np.array([np.nan] * 3, np.float32), 0.5, 0.5) == (3, 2)       # unspecified values: still one of the k ranks


# ---------------------------------------------------------------- the sampler's cases (CPU and GPU share them)
VOCAB_KINDS = ("1", "63", "65", "C-1", "C", "C+1", "2C+5", "40000")
KS = (1, 2, 40, 64)
INV_TEMP = {1: 1.0, 2: 1.25, 40: 0.7, 64: 1.25}
PROB_ROWS = (0, 1, 2, 3, 4, 5, 7, 8)                                  # (row 6 holds NaN and +-inf: ids and "the token is one of them" only)


def _vocab(kind):
    Cn = _lib.lib().ggml_hip_topk_chunk()
    return {"1": 1, "63": 63, "65": 65, "C-1": Cn - 1, "C": Cn, "C+1": Cn + 1, "2C+5": 2 * Cn + 5, "40000": 40000}[kind]


_ROWS = {}


def sampler_rows(kind):
    """nine rows of n_vocab logits (computed once per vocabulary and never written): 0, 8 plain; 1 all equal; 2 / 3 the maximum at index 0 /
    n_vocab - 1; 4 equal maxima on both sides of the first chunk boundary (or at both ends of a shorter row); 5 three values, so more than k equal
    ones; 6 NaN and +-inf sprinkled; 7 -0.0 against +0.0 (and -1).  A chunk shorter than k is the last chunk of C + 1 and 2C + 5."""
    if kind in _ROWS:
        return _ROWS[kind]
    V, Cn = _vocab(kind), _lib.lib().ggml_hip_topk_chunk()
    rng = np.random.default_rng(1000 + V)
    x = rng.normal(0.0, 3.0, (9, V)).astype(np.float32)
    top = np.float32(np.abs(x).max() + 1.0)
    x[1] = np.float32(1.5)
    x[2, 0] = top
    x[3, V - 1] = top
    a, b = (Cn - 1, Cn) if V > Cn else (0, V - 1)
    x[4, a] = x[4, b] = top
    x[5] = rng.integers(0, 3, V).astype(np.float32)
    n6 = max(1, V // 7)
    for val in (np.nan, np.inf, -np.inf):
        x[6, rng.integers(0, V, n6)] = np.float32(val)
    x[7] = rng.choice(np.array([-0.0, 0.0, -1.0], np.float32), V)
    x.setflags(write=False)
    _ROWS[kind] = x
    return x


def _ks(V):
    return [k for k in KS if k <= V]


# ---- the vocabularies that select the upper rungs of the merge ladder, by chunk count
BIG_FULL = (4, 8, 16, 32, 64, 128)                                    # n_vocab = n_chunks * C: with k = 64 the rung n_chunks / 4 is full
BIG_NEXT = (5, 9, 17, 33, 65, 129)                                    # n_vocab = (n_chunks - 1) * C + 1: the next rung up, a last chunk of one logit
BIG_TOP = 256                                                         # n_vocab = 2^20, the header's maximum
BIG_KS = {n: (64,) for n in BIG_FULL + BIG_NEXT + (BIG_TOP,)}
for _n in (17, 65, 256):
    BIG_KS[_n] = (2, 40) + BIG_KS[_n]
for _n in (5, 65, 256):
    BIG_KS[_n] = (1,) + BIG_KS[_n]
BIG_KINDS = tuple("%dC" % n for n in BIG_FULL) + tuple("%dC+1" % (n - 1) for n in BIG_NEXT) + ("2^20",)
ROW_COUNT_CASES = ((130, "2C+5", 64), (4096, "65", 2))                # (n_rows, a kind of VOCAB_KINDS, k): blockIdx / n_chunks away from 9 rows
MERGE_RUNGS = (1, 2, 4, 8, 16, 32, 64)


def _big_chunks(kind):
    return BIG_TOP if kind == "2^20" else int(kind.split("C")[0]) + (1 if kind.endswith("+1") else 0)


def _big_vocab(kind):
    Cn, n = _lib.lib().ggml_hip_topk_chunk(), _big_chunks(kind)
    return 1 << 20 if kind == "2^20" else (n - 1) * Cn + 1 if kind.endswith("+1") else n * Cn


def big_rows(kind):
    """nine rows of n_vocab logits (computed once per vocabulary and never written), with `top` above every plain logit: 0 plain; 1 all equal;
    2 the 64 best inside the last full chunk at permuted offsets, top + 0.125 s, under a larger value at n_vocab - 1; 3 one winner in each of
    min(64, n_chunks) chunks from the first to the last, at offset 37 c modulo the chunk's length, top + 16 - 0.25 s; 4 `top` at the last index
    of every chunk: with more than k chunks, more than k equal maxima; 5 three values; 6 NaN and +-inf sprinkled; 7 / 8 in the second chunk,
    the sixteen best where ONE thread of the chunk kernel holds them all under the one-by-one / the float4 load, descending.
    -> (x [9, n_vocab], its rank order [9, 64] under S.topk_ids: a prefix of it is the rank order of a smaller k)"""
    if ("big", kind) in _ROWS:
        return _ROWS["big", kind]
    V, Cn, n_chunks = _big_vocab(kind), _lib.lib().ggml_hip_topk_chunk(), _big_chunks(kind)
    rng = np.random.default_rng(2000 + V)
    x = rng.normal(0.0, 3.0, (9, V)).astype(np.float32)
    top = np.float32(np.ceil(np.abs(x).max()) + 1.0)                  # (an integer: the steps of 1/8 below are exact)
    x[1] = np.float32(1.5)
    full = n_chunks - 1 if V % Cn == 0 else n_chunks - 2              # the last FULL chunk
    offs = rng.permutation(Cn - 1)[:64]                               # (not its last index: n_vocab - 1 may be that)
    x[2, full * Cn + offs] = top + np.float32(0.125) * np.arange(64, dtype=np.float32)
    x[2, V - 1] = top + np.float32(8.0)
    chunks = np.unique(np.round(np.linspace(0, n_chunks - 1, min(64, n_chunks))).astype(np.int64))
    assert len(chunks) == min(64, n_chunks) and chunks[0] == 0 and chunks[-1] == n_chunks - 1
    lens = np.minimum(Cn, V - chunks * Cn)
    x[3, chunks * Cn + (chunks * 37) % lens] = top + np.float32(16.0) - np.float32(0.25) * np.arange(len(chunks), dtype=np.float32)
    x[4, np.minimum(np.arange(1, n_chunks + 1) * Cn, V) - 1] = top
    x[5] = rng.integers(0, 3, V).astype(np.float32)
    n6 = max(1, V // 7)
    for val in (np.nan, np.inf, -np.inf):
        x[6, rng.integers(0, V, n6)] = np.float32(val)
    down = top + np.float32(8.0) - np.float32(0.25) * np.arange(16, dtype=np.float32)
    x[7, Cn + 7 + 256 * np.arange(16)] = down
    x[8, [Cn + (256 * j + 7) * 4 + q for j in range(4) for q in range(4)]] = down
    x.setflags(write=False)
    order = S.topk_ids(x, 64)
    order.setflags(write=False)
    _ROWS["big", kind] = (x, order)
    return _ROWS["big", kind]


def many_rows(n_rows, kind):
    """n_rows plain rows of a vocabulary of VOCAB_KINDS, every row different (computed once) -> (x, its rank order [n_rows, 64 or n_vocab])"""
    if (n_rows, kind) not in _ROWS:
        V = _vocab(kind)
        x = np.random.default_rng(3000 + n_rows).normal(0.0, 3.0, (n_rows, V)).astype(np.float32)
        x.setflags(write=False)
        order = S.topk_ids(x, min(64, V))
        order.setflags(write=False)
        _ROWS[(n_rows, kind)] = (x, order)
    return _ROWS[(n_rows, kind)]


def _merge_form(n_vocab, k, probs):
    """launch_sample_topk's ladder restated: the merge kernel's keys per thread, "ONE" for the k = 1 form without probabilities"""
    Cn = _lib.lib().ggml_hip_topk_chunk()
    n_cand = -(-n_vocab // Cn) * k
    if k == 1 and not probs:
        return "ONE", n_cand
    npt = -(-n_cand // 256)
    return next(N for N in MERGE_RUNGS if npt <= N), n_cand


def test_the_cases_reach_every_form_of_the_merge():
    """A RESTATEMENT of launch_sample_topk's ladder (csrc/sample.hip): npt = ceil(n_chunks * k / 256) rounded up to 1, 2, 4, ... 64, and the
    form of k == 1 && !probs.  A change to the ladder there changes _merge_form here.  Over the (vocabulary, k) of the GPU tests below: all
    seven rungs run, every rung N >= 2 both FULL (n_cand == 256 N) and at its lowest occupancy under k = 64 (one chunk more than the rung
    below holds, n_cand == 128 N + 64), and the k = 1 form runs at the large vocabularies too."""
    Cn = _lib.lib().ggml_hip_topk_chunk()
    assert len(BIG_KINDS) == 13 and len(set(BIG_KINDS)) == 13
    for kind in BIG_KINDS:
        V, n = _big_vocab(kind), _big_chunks(kind)
        assert -(-V // Cn) == n and V <= 1 << 20, (kind, V)
        assert V - (n - 1) * Cn == (1 if kind.endswith("+1") else Cn), kind      # the last chunk: one logit, shorter than k, or full
        assert _lib.lib().ggml_hip_topk_work_size(9, V, 64) == 9 * n * 64 * 8
    assert _big_vocab("2^20") == 1 << 20
    reached = {}                                                      # rung -> the n_cand it ran at
    for kind in BIG_KINDS:
        for k in BIG_KS[_big_chunks(kind)]:
            form, n_cand = _merge_form(_big_vocab(kind), k, True)
            reached.setdefault(form, set()).add(n_cand)
    for n_rows, kind, k in ROW_COUNT_CASES:
        form, n_cand = _merge_form(_vocab(kind), k, True)
        reached.setdefault(form, set()).add(n_cand)
    assert sorted(reached) == list(MERGE_RUNGS), sorted(reached)
    for N in MERGE_RUNGS[1:]:
        assert 256 * N in reached[N], ("no case fills rung", N)
        assert 128 * N + 64 in reached[N], ("no case enters rung at its lowest occupancy", N)
    small = {_merge_form(_vocab(kind), k, True)[0] for kind in VOCAB_KINDS for k in _ks(_vocab(kind))}
    assert small == {1, 2, 4}                                         # what the small vocabularies alone reach
    assert {n for n in BIG_KS if 1 in BIG_KS[n]} == {5, 65, 256}      # the argmax entry: 5, 65 and 256 keys in the ONE form's 256 threads
    assert all(_merge_form(_big_vocab(kind), 1, False) == ("ONE", _big_chunks(kind)) for kind in BIG_KINDS)


def _probability_cases():
    """every (label, x, rank order for k, k) whose probabilities a GPU test checks: the yardstick's CPU guards run over all of them"""
    for kind in VOCAB_KINDS:
        x = sampler_rows(kind)
        for k in _ks(x.shape[1]):
            yield (kind, k), x[list(PROB_ROWS)], S.topk_ids(x, k)[list(PROB_ROWS)], k
    for kind in BIG_KINDS:
        x, order = big_rows(kind)
        for k in BIG_KS[_big_chunks(kind)]:
            yield (kind, k), x[list(PROB_ROWS)], order[list(PROB_ROWS), :k], k
    for n_rows, kind, k in ROW_COUNT_CASES:
        x, order = many_rows(n_rows, kind)
        yield (n_rows, kind, k), x, order[:, :k], k


def test_the_generator_stays_inside_the_spread_the_bound_assumes():
    """(l_0 - l_(k-1)) * inv_temp <= 60 for every probability-checked row of every case: no e_s is subnormal.  No case is left out."""
    n = 0
    for label, x, ids, k in _probability_cases():
        sp = S.spread(x, ids, INV_TEMP[k])
        assert sp <= S.Z_MAX, (label, sp)
        assert np.isfinite(np.take_along_axis(x, ids.astype(np.int64), axis=1)).all()
        n += 1
    assert n == sum(len(_ks(_vocab(kind))) for kind in VOCAB_KINDS) + sum(len(BIG_KS[_big_chunks(kind)]) for kind in BIG_KINDS) + len(ROW_COUNT_CASES)


def test_the_model_constant_is_what_the_model_measures():
    """the numpy f32 model of the statement over the GPU test's inputs: inside the derived bound, and MODEL_WORST records its worst"""
    worst, where = 0.0, None
    for label, x, ids, k in _probability_cases():
        st = S.statistic(S.probs32(x, ids, INV_TEMP[k]), x, ids, INV_TEMP[k])
        if st > worst:
            worst, where = st, label
    # (no lower edge: another numpy build's f32 exp may round better than the one the constant was recorded with)
    print("model worst statistic", worst, "at", where, "recorded", S.MODEL_WORST, "bar 1.0")
    assert worst <= S.MODEL_WORST < 1.0, worst


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


def _sentinel(dev, n):
    torch = dev.torch
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def _keeps_sentinel(dev, a):
    return bool((a.view(dev.torch.int32) == SENTINEL).all())


GUARD = 64       # elements


# ---- get_rows
def _file_rows(dev, type, M, K, seed):
    """M rows of K elements in the file format of `type` (numpy uint8 [M, row bytes]), from the library's own quantizers"""
    torch = dev.torch
    rng = np.random.default_rng(seed)
    x = rng.normal(0.0, 1.0, (M, K)).astype(np.float32)
    if type == F32:
        return x.view(np.uint8).reshape(M, -1)
    if type == F16:
        return x.astype(np.float16).view(np.uint8).reshape(M, -1)
    return dev.quantize_rows(type, torch.from_numpy(x).cuda()).cpu().numpy().reshape(M, -1)


def _dequantized(dev, type, rows_u8, K):
    """the type table's dequantize row function on file-format rows -> f32 [M, K] (numpy)"""
    torch = dev.torch
    M = rows_u8.shape[0]
    flat = np.ascontiguousarray(rows_u8).reshape(-1)
    if type == F32:
        return flat.view(np.float32).reshape(M, K).copy()
    if type == F16:
        return flat.view(np.float16).reshape(M, K).astype(np.float32)
    return dev.dequantize_rows(type, torch.from_numpy(flat).cuda(), K).cpu().numpy()


def _get_rows(dev, w, ids_np, ldd, extra_rows=2):
    """the entry into a sentinel-filled [n + extra_rows, ldd] buffer between guards -> f32 bits [n, K]; everything else must keep its sentinel"""
    torch = dev.torch
    n = len(ids_np)
    d_ids = torch.from_numpy(np.asarray(ids_np, np.int32)).cuda()
    buf = _sentinel(dev, GUARD + (n + extra_rows) * ldd + GUARD)
    rc = _lib.lib().ggml_hip_get_rows_dev(w.handle, _p(d_ids.data_ptr()), n, _p(buf.data_ptr() + 4 * GUARD), ldd, _stream(dev))
    assert rc == 0, _lib.lib().ggml_hip_last_error()
    torch.cuda.synchronize()
    body = buf[GUARD:GUARD + (n + extra_rows) * ldd].view(n + extra_rows, ldd)
    assert _keeps_sentinel(dev, buf[:GUARD]) and _keeps_sentinel(dev, buf[GUARD + (n + extra_rows) * ldd:]), "guards written"
    assert _keeps_sentinel(dev, body[n:]), "rows beyond n_ids written"
    assert _keeps_sentinel(dev, body[:n, w.K:]), "padding columns written"
    return body[:n, :w.K].cpu().numpy().view(np.uint32)


def _ids_for(M, n, rng):
    special = [M - 1, -1, 0, M, 2 ** 31 - 1, 0]                     # the last row, below, the first, one past, the largest int32, a repeat
    ids = special + rng.integers(-2, M + 2, 130).tolist()
    return np.array(ids[:n], np.int32)


def _ks_for(name):
    if name in ("f32", "f16", "bf16"):
        return (5, 32, 36, 64)
    return (256, 512) if name.endswith("_k") or name == "iq4_xs" else (32, 64)


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(SERVED))
def test_get_rows_is_download_then_dequantize_bit_for_bit(dev, name):
    type = SERVED[name]
    rng = np.random.default_rng(7)
    checked = 0
    for K in _ks_for(name):
        for M in (1, 255, 257, 300):
            rows = _file_rows(dev, type, M, K, seed=K * 1000 + M)
            w = dev.Weight.from_host(type, rows, K)
            down = w.download().reshape(M, -1)
            assert np.array_equal(down, rows)
            table = _dequantized(dev, type, down, K).view(np.uint32)
            assert table.shape == (M, K)
            for n in (1, 3, 130):
                ids = _ids_for(M, n, rng)
                inside = (ids >= 0) & (ids < M)
                want = np.where(inside[:, None], table[np.where(inside, ids, 0)], np.uint32(0))
                for ldd in (K, K + 3):
                    got = _get_rows(dev, w, ids, ldd)
                    bad = int((got != want).sum())
                    assert bad == 0, (name, K, M, n, ldd, bad)
                    checked += got.size
            # invariance: one id at a time, and in reverse order, the same bits
            ids = _ids_for(M, 6, rng)
            whole = _get_rows(dev, w, ids, K)
            assert np.array_equal(_get_rows(dev, w, ids[::-1].copy(), K + 3), whole[::-1])
            for i, one in enumerate(ids):
                assert np.array_equal(_get_rows(dev, w, ids[i:i + 1], K, extra_rows=1)[0], whole[i]), (name, K, M, i)
            w.free()
    assert checked > 0


@pytest.mark.gpu
def test_get_rows_refuses_a_short_ldd(dev):
    w = dev.Weight.from_host(Q8_0, _file_rows(dev, Q8_0, 4, 64, seed=1), 64)
    buf = _sentinel(dev, 256)
    ids = dev.torch.zeros(2, dtype=dev.torch.int32, device="cuda")
    assert _lib.lib().ggml_hip_get_rows_dev(w.handle, _p(ids.data_ptr()), 2, _p(buf.data_ptr()), 63, _stream(dev)) == ERR_SHAPE
    assert _lib.lib().ggml_hip_get_rows_dev(w.handle, _p(ids.data_ptr()), 0, _p(buf.data_ptr()), 63, _stream(dev)) == OK
    dev.torch.cuda.synchronize()
    assert _keeps_sentinel(dev, buf)
    w.free()


# ---- the sampler
def _sample(dev, logits_np, ld, k, inv_temp=1.0, top_p=1.0, u=None, probs=True, argmax=False):
    """an entry on logits placed ld apart (the padding columns hold a LARGER value than any finite logit: never read); the outputs sit between
    guards, which must keep their sentinel.  -> (ids [T, k], probs f32 [T, k] or None, token [T] or None) numpy"""
    torch = dev.torch
    T, V = logits_np.shape
    buf = np.full((T, ld), np.float32(3.0e38), np.float32)
    buf[:, :V] = logits_np
    d_l = torch.from_numpy(buf).cuda()
    ids = _sentinel(dev, GUARD + T * k + GUARD)
    pr = _sentinel(dev, GUARD + T * k + GUARD)
    tok = _sentinel(dev, GUARD + T + GUARD)
    d_u = torch.from_numpy(np.asarray(u, np.float32)).cuda() if u is not None else None
    nbytes = _lib.lib().ggml_hip_topk_work_size(T, V, k)
    assert nbytes > 0
    work = torch.empty(nbytes + 8 * GUARD, dtype=torch.uint8, device="cuda")
    work.view(torch.int32)[nbytes // 4:] = SENTINEL
    if argmax:
        rc = _lib.lib().ggml_hip_argmax_rows_dev(_p(d_l.data_ptr()), ld, T, V, _p(ids.data_ptr() + 4 * GUARD), _p(work.data_ptr()), nbytes, _stream(dev))
    else:
        rc = _lib.lib().ggml_hip_sample_topk_dev(_p(d_l.data_ptr()), ld, T, V, k, inv_temp, top_p, _p(d_u.data_ptr()) if u is not None else None,
                                                 _p(ids.data_ptr() + 4 * GUARD), _p(pr.data_ptr() + 4 * GUARD) if probs else None,
                                                 _p(tok.data_ptr() + 4 * GUARD) if u is not None else None, _p(work.data_ptr()), nbytes, _stream(dev))
    assert rc == 0, _lib.lib().ggml_hip_last_error()
    torch.cuda.synchronize()
    for b, n in ((ids, T * k), (pr, T * k if probs and not argmax else 0), (tok, T if u is not None else 0)):
        assert _keeps_sentinel(dev, b[:GUARD]) and _keeps_sentinel(dev, b[GUARD + n:]), "guards written"
    assert _keeps_sentinel(dev, work.view(torch.int32)[nbytes // 4:]), "work buffer overrun"
    out_ids = ids[GUARD:GUARD + T * k].cpu().numpy().reshape(T, k)
    out_p = pr[GUARD:GUARD + T * k].view(torch.float32).cpu().numpy().reshape(T, k) if probs and not argmax else None
    out_t = tok[GUARD:GUARD + T].cpu().numpy() if u is not None else None
    return out_ids, out_p, out_t


INDEP_TOP_P = 0.9
INDEP_U = np.array([0.37, 0.81, 0.05, 0.64, 0.93, 0.22, 0.48, 0.76, 0.11], np.float32)      # one uniform per row, all different: row r must read u[r]


def _check_tokens(p, ids, tok, rows, u, where):
    """tok[i] is the sequential statement on the probabilities written for row rows[i] (rows of PROB_ROWS), and one of the row's ids always"""
    for i, r in enumerate(rows):
        assert tok[i] in ids[i], (where, r)
        if r in PROB_ROWS:
            n_keep, s = S.keep_pick(p[i], INDEP_TOP_P, u[i])
            assert tok[i] == ids[i, s], (where, r, n_keep, s)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", VOCAB_KINDS)
def test_ids_probabilities_and_independence(dev, kind):
    """a row's THREE outputs -- ids, probabilities, token -- are bitwise the same alone, among 3 and 9 rows and at either ld; the token is also
    held to keep_pick on the row's own downloaded probabilities every time, so it has a reference that is not the kernel"""
    x = sampler_rows(kind)
    V = x.shape[1]
    worst = 0.0
    for k in _ks(V):
        it = INV_TEMP[k]
        want_ids = S.topk_ids(x, k)
        ref = None
        for n_rows in (9, 3, 1):
            for ld in (V, V + 3):
                ids, p, tok = _sample(dev, x[:n_rows], ld, k, inv_temp=it, top_p=INDEP_TOP_P, u=INDEP_U[:n_rows])
                assert np.array_equal(ids, want_ids[:n_rows]), (kind, k, n_rows, ld)
                if ref is None:
                    ref = (ids, p.view(np.uint32), tok)
                    rows = list(PROB_ROWS)
                    st = S.statistic(p[rows], x[rows], ids[rows], it)
                    worst = max(worst, st)
                    assert st <= 1.0, (kind, k, st)
                    assert (np.abs(p[rows].astype(np.float64).sum(axis=1) - 1.0) <= (k + 2) * S.U).all()
                # independence: a row's bits are the same among 9, 3 and alone, at either ld
                assert np.array_equal(p.view(np.uint32), ref[1][:n_rows]), (kind, k, n_rows, ld)
                _check_tokens(p, ids, tok, range(n_rows), INDEP_U, (kind, k, n_rows, ld))
                for r in range(n_rows):
                    if r in PROB_ROWS:
                        assert tok[r] == ref[2][r], (kind, k, n_rows, ld, r)
                am, _, _ = _sample(dev, x[:n_rows], ld, 1, argmax=True)
                assert np.array_equal(am[:, 0], ids[:, 0]), (kind, k, n_rows, ld)
        for r in range(1, 9):                                        # every special row alone, with the uniform it had among the nine
            ids, p, tok = _sample(dev, x[r:r + 1], V + 3, k, inv_temp=it, top_p=INDEP_TOP_P, u=INDEP_U[r:r + 1])
            assert np.array_equal(ids[0], ref[0][r]) and np.array_equal(p.view(np.uint32)[0], ref[1][r]), (kind, k, r)
            _check_tokens(p, ids, tok, [r], INDEP_U[r:r + 1], (kind, k, "alone"))
            if r in PROB_ROWS:
                assert tok[0] == ref[2][r], (kind, k, r)
        ids_np, p_np, none = _sample(dev, x, V, k, inv_temp=it)                       # no pick: the same ids and probabilities, no token
        assert np.array_equal(ids_np, want_ids) and np.array_equal(p_np.view(np.uint32), ref[1]) and none is None
        ids_only, none, _ = _sample(dev, x, V, k, inv_temp=it, probs=False)           # ids alone: no probabilities, no pick
        assert np.array_equal(ids_only, want_ids) and none is None
    print(kind, "worst probability statistic", worst, "model", S.MODEL_WORST, "bar 1.0")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", VOCAB_KINDS)
def test_n_keep_and_the_pick_are_the_sequential_statement_on_the_written_probabilities(dev, kind):
    x = sampler_rows(kind)
    V = x.shape[1]
    rng = np.random.default_rng(5)
    for k in _ks(V):
        it = INV_TEMP[k]
        base_ids, base_p, _ = _sample(dev, x, V, k, inv_temp=it)
        for top_p in (0.0, 0.5, 0.9, 1.0):
            for u in (0.0, 0.25, np.float32(0.9999999), None):
                uu = rng.random(9).astype(np.float32) if u is None else np.full(9, u, np.float32)
                assert (uu < 1.0).all()
                ids, p, tok = _sample(dev, x, V, k, inv_temp=it, top_p=top_p, u=uu)
                assert np.array_equal(ids, base_ids) and np.array_equal(p.view(np.uint32), base_p.view(np.uint32))
                for r in range(9):
                    assert tok[r] in ids[r], (kind, k, top_p, u, r)                   # (row 6 too: unspecified, but one of its k ids)
                    if r in PROB_ROWS:
                        n_keep, s = S.keep_pick(p[r], top_p, uu[r])
                        assert tok[r] == ids[r, s], (kind, k, top_p, float(uu[r]), r, n_keep, s)


def _held_to_the_yardsticks(x, ids, p, want_ids, k, where):
    """ids exact on every row; the probabilities of rows x (all of them probability-checked) inside the derived bound, summing to 1 -> the statistic"""
    assert np.array_equal(ids, want_ids), (where, "first differing rows", np.nonzero((ids != want_ids).any(axis=1))[0][:4].tolist())
    st = S.statistic(p, x, ids, INV_TEMP[k])
    print(where, "probability statistic", st)
    assert st <= 1.0, (where, st)
    assert (np.abs(p.astype(np.float64).sum(axis=1) - 1.0) <= (k + 2) * S.U).all(), where
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("kind", BIG_KINDS)
def test_every_merge_rung_at_both_edges(dev, kind):
    """big_rows at the k of BIG_KS: the nine rows at ld = n_vocab and n_vocab + 3 (between them the float4 and the one-by-one load of every
    vocabulary: for (n - 1) C + 1 logits, + 3 is the aligned stride, with a tail of one), rows 2, 3 and 4 alone, the ids-only call, and the
    argmax entry at both strides.  Ids exact, probabilities inside the bound and bitwise the same every time, the token by keep_pick."""
    x, order = big_rows(kind)
    V = x.shape[1]
    rows = list(PROB_ROWS)
    worst = 0.0
    for ld in (V, V + 3):
        am, _, _ = _sample(dev, x, ld, 1, argmax=True)
        assert np.array_equal(am[:, 0], order[:, 0]), (kind, "argmax", ld)
    for k in BIG_KS[_big_chunks(kind)]:
        it = INV_TEMP[k]
        want_ids = order[:, :k]
        ref = None
        for ld in (V, V + 3):
            ids, p, tok = _sample(dev, x, ld, k, inv_temp=it, top_p=INDEP_TOP_P, u=INDEP_U)
            assert np.array_equal(ids, want_ids), (kind, k, ld, "first differing rows", np.nonzero((ids != want_ids).any(axis=1))[0].tolist())
            if ref is None:
                ref = (ids, p.view(np.uint32), tok)
                worst = max(worst, _held_to_the_yardsticks(x[rows], ids[rows], p[rows], want_ids[rows], k, (kind, k)))
            assert np.array_equal(p.view(np.uint32), ref[1]), (kind, k, ld)
            _check_tokens(p, ids, tok, range(9), INDEP_U, (kind, k, ld))
            assert np.array_equal(tok[rows], ref[2][rows]), (kind, k, ld)
        for r in (2, 3, 4):                                          # alone, with the uniform the row had among the nine
            ids, p, tok = _sample(dev, x[r:r + 1], V + 3, k, inv_temp=it, top_p=INDEP_TOP_P, u=INDEP_U[r:r + 1])
            assert np.array_equal(ids[0], ref[0][r]) and np.array_equal(p.view(np.uint32)[0], ref[1][r]), (kind, k, r)
            _check_tokens(p, ids, tok, [r], INDEP_U[r:r + 1], (kind, k, "alone"))
            assert tok[0] == ref[2][r], (kind, k, r)
        ids_only, none, _ = _sample(dev, x, V + 3, k, inv_temp=it, probs=False)        # ids alone (k = 1: the ONE form, as the argmax entry)
        assert np.array_equal(ids_only, want_ids) and none is None, (kind, k)
    print(kind, "worst probability statistic", worst, "model", S.MODEL_WORST, "bar 1.0")


@pytest.mark.gpu
@pytest.mark.parametrize("n_rows,kind,k", ROW_COUNT_CASES)
def test_a_row_is_found_among_many(dev, n_rows, kind, k):
    """many plain rows, all different: a workgroup's row and chunk come from blockIdx / n_chunks, and row r reads u[r]"""
    x, order = many_rows(n_rows, kind)
    V = x.shape[1]
    want_ids = order[:, :k]
    u = np.random.default_rng(n_rows).random(n_rows).astype(np.float32)
    ref = None
    for ld in (V, V + 3):
        ids, p, tok = _sample(dev, x, ld, k, inv_temp=INV_TEMP[k], top_p=INDEP_TOP_P, u=u)
        if ref is None:
            ref = p.view(np.uint32)
            _held_to_the_yardsticks(x, ids, p, want_ids, k, (n_rows, kind, k))
        assert np.array_equal(ids, want_ids) and np.array_equal(p.view(np.uint32), ref), (n_rows, kind, k, ld)
        for r in range(n_rows):
            n_keep, s = S.keep_pick(p[r], INDEP_TOP_P, u[r])
            assert tok[r] == ids[r, s], (n_rows, kind, k, ld, r, n_keep, s)
        am, _, _ = _sample(dev, x, ld, 1, argmax=True)
        assert np.array_equal(am[:, 0], want_ids[:, 0]), (n_rows, kind, ld)
    ids_only, none, _ = _sample(dev, x, V, k, inv_temp=INV_TEMP[k], probs=False)
    assert np.array_equal(ids_only, want_ids) and none is None


# ---- the loop
def _toy(dev, type, seed):
    """tied embeddings: one weight [vocab 300, hidden 256] of `type`, a norm gain of mixed signs (so that a token's own row does not win the LM head)"""
    rng = np.random.default_rng(seed)
    rows = _file_rows(dev, type, 300, 256, seed)
    w = dev.Weight.from_host(type, rows, 256)
    g = dev.torch.from_numpy(rng.normal(0.0, 1.0, (1, 256)).astype(np.float32)).cuda()
    return w, g


class _Step:
    """get_rows -> rms_norm_mul -> mul_mat -> (argmax | sample_topk) on fixed buffers: what a graph captures"""

    def __init__(self, dev, w, g, sample):
        torch = dev.torch
        self.dev, self.w, self.g, self.sample = dev, w, g, sample
        self.token = torch.zeros(1, dtype=torch.int32, device="cuda")
        self.h = torch.zeros((1, 256), device="cuda")
        self.n = torch.zeros((1, 256), device="cuda")
        self.y = torch.zeros((1, 256), device="cuda")
        self.logits = torch.zeros((1, 300), device="cuda")
        self.mm_work = dev.alloc_work(w.type, 256, 1)
        self.k_work = dev.topk_work(1, 300, 8 if sample else 1)
        self.u = torch.zeros(1, device="cuda")
        self.ids = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
        self.probs = torch.zeros((1, 8), device="cuda")

    def __call__(self):
        dev = self.dev
        dev.get_rows(self.w, self.token, out=self.h)
        _lib.check(_lib.lib().ggml_hip_rms_norm_mul_rows_dev(_p(self.h.data_ptr()), _p(self.g.data_ptr()), _p(self.n.data_ptr()), _p(self.y.data_ptr()), 1, 256,
                                                             _stream(dev)), "rms_norm_mul_rows")
        dev.mul_mat(self.w, self.y, out=self.logits, work=self.mm_work)
        if self.sample:
            dev.sample_topk(self.logits, 8, inv_temp=1.0, top_p=0.9, u=self.u, ids=self.ids, probs=self.probs, token=self.token, work=self.k_work)
        else:
            dev.argmax_rows(self.logits, ids=self.token, work=self.k_work)


def _capture(dev, step):
    torch = dev.torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step()
    torch.cuda.current_stream().wait_stream(s)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["q8_0", "q4_k"])
def test_a_captured_step_feeds_its_own_token_to_the_next_replay(dev, name):
    torch = dev.torch
    type = SERVED[name]
    w, g = _toy(dev, type, seed=300 + type)
    START, N = 17, 8
    # eager steps
    eager = _Step(dev, w, g, sample=False)
    eager.token.fill_(START)
    want = []
    for _ in range(N):
        eager()
        torch.cuda.synchronize()
        want.append(int(eager.token.item()))
    # the captured step: run once outside the capture, captured once, replayed N times; nothing is written to the device in between
    step = _Step(dev, w, g, sample=False)
    step.token.fill_(START)
    step()
    torch.cuda.synchronize()
    graph = _capture(dev, step)
    step.token.fill_(START)
    torch.cuda.synchronize()
    got = []
    for _ in range(N):
        graph.replay()
        torch.cuda.synchronize()
        got.append(int(step.token.item()))
    assert got == want, (got, want)
    # (the toy moves: a fixed point would not show that a replay reads the token the one before it wrote.  With tied embeddings the score of
    # j after i is a symmetric form in the two rows, so the typical orbit of the argmax is a pair of tokens; the sampling graph below wanders)
    assert len(set(want)) >= 2 and want[0] != START, want
    # a host loop: the lookup and the argmax in numpy, the norm and the LM head on the device
    table = _dequantized(dev, type, w.download().reshape(300, -1), 256)
    host, tok = [], START
    hs = _Step(dev, w, g, sample=False)
    for _ in range(N):
        hs.h.copy_(torch.from_numpy(table[tok:tok + 1]))
        _lib.check(_lib.lib().ggml_hip_rms_norm_mul_rows_dev(_p(hs.h.data_ptr()), _p(g.data_ptr()), _p(hs.n.data_ptr()), _p(hs.y.data_ptr()), 1, 256, _stream(dev)), "pair")
        dev.mul_mat(w, hs.y, out=hs.logits, work=hs.mm_work)
        torch.cuda.synchronize()
        tok = int(np.argmax(hs.logits.cpu().numpy()[0]))             # (the first of equal maxima: the rule's tie order)
        host.append(tok)
    assert host == want, (host, want)
    # a second graph samples: top-k 8, top-p 0.9, the uniforms rewritten between replays
    us = np.random.default_rng(9).random(N).astype(np.float32)
    es = _Step(dev, w, g, sample=True)
    es.token.fill_(START)
    want_s = []
    for i in range(N):
        es.u.fill_(float(us[i]))
        es()
        torch.cuda.synchronize()
        want_s.append(int(es.token.item()))
    ss = _Step(dev, w, g, sample=True)
    ss.token.fill_(START)
    ss()
    torch.cuda.synchronize()
    graph_s = _capture(dev, ss)
    ss.token.fill_(START)
    got_s = []
    for i in range(N):
        ss.u.fill_(float(us[i]))
        graph_s.replay()
        torch.cuda.synchronize()
        got_s.append(int(ss.token.item()))
        assert got_s[-1] in ss.ids.cpu().numpy()[0]
    assert got_s == want_s, (got_s, want_s)
    w.free()
