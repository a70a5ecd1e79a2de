"""numpy restatements for tests/test_attention_mla.py: the float64 REFERENCE of MLA (absorbed form) over a dequantized latent cache, and the
float32 / float16 MODEL of the arithmetic include/ggml_hip_ext.h writes down in its section MLA (csrc/mla.hip's header comment).

  cache       one row of D_K = 576 elements per position, shared by every head: columns 0 .. 511 are the latent AND the value, 512 .. 575 the rotated
              key part.  q f32 [n_q, n_head, 576], dst [n_q, n_head, 512].  A ROW is (t, h); vis(t) is np_attention.visible.
  reference   dst[t, h] = softmax_j(scale * q[t, h] . row_j) row_j[:512] over the visible j, everything float64, the rows the DEQUANTIZED cache
              (F16 widened; Q8_0 (float32)q * d) -- never the library;
  model       vectorised over the rows: Q, the staged rows (a Q8_0 row: f16 of its dequantized value) and the weights P rounded to float16,
              scores and sums in float32, the online softmax per STEP of 64 positions (two per chunk of 128) with l the sum of the ROUNDED
              weights; WALK walks every step, SPLIT runs the steps of each span of `span` chunks on their own and merges the partials against
              the global maximum in ascending span order.  The model does not pin expf or the order of the additions inside a step (numpy's own).
  mutants     four wrong statements the bar must see (model(..., mutant=)): "v_shift" takes V from columns 64 .. 575; "score512" scores over the
              first 512 columns only; "vis_off" sees one position too few; "merge_no_b" merges the spans without b_s.

The statistic of a case is np_attention.statistic: max |dst - ref| / max |V|.  SCALE = 0.5 is the sweep's: scores of inputs in [-1, 1] over 576
columns have a standard deviation of 8, so the softmax is peaked (a few positions carry a row) and a wrongly weighted span or position moves dst by
a large part of max |V|; DeepSeek-V3's own scale, mscale^2 / sqrt(192) = 0.135, is flatter and makes every error, the mutants' included, smaller.

Measured for the model on the sweep of tests/test_attention_mla.py (cases(): n_head in {1, 16, 24}, both cache types, n_kv in
{1, 31, 128, 129, 379, 128 span + 1, 256 span + 37}, causal on and off, seeded inputs in [-1, 1]) at span = 4:

    SPLIT (n_q in {1, 3, 8})  worst 1.87e-03 (recorded as 1.9e-03)
    WALK  (n_q in {9, 70})    worst 2.15e-03 (recorded as 2.2e-03)

The kernels are held to 4 x these (the factor np_attention.py uses: expf and the order of accumulation inside a step):

    TOL_SPLIT = 4 * MODEL_WORST_SPLIT = 7.6e-03        TOL_WALK = 4 * MODEL_WORST_WALK = 8.8e-03

test_the_model_constants_are_what_the_model_measures recomputes both on the CPU, test_the_bar_sees_the_four_mutants holds every mutant's worst
statistic to at least 100 x the tolerance of its form."""
import numpy as np

import np_attention as A

F16, Q8_0 = A.F16, A.Q8_0
D_K, D_V = 576, 512
CHUNK, STEP = 128, 64
SPLIT_MAX_Q = 8
SPLIT, WALK = 1, 2
SCALE = 0.5
MODEL_WORST_SPLIT = 1.9e-03
MODEL_WORST_WALK = 2.2e-03
TOL_SPLIT = 4 * MODEL_WORST_SPLIT
TOL_WALK = 4 * MODEL_WORST_WALK
MUTANTS = ("v_shift", "score512", "vis_off", "merge_no_b")


def form_of(n_q):
    return SPLIT if n_q <= SPLIT_MAX_Q else WALK


def tol_of(n_q):
    return TOL_SPLIT if n_q <= SPLIT_MAX_Q else TOL_WALK


def row_bytes(kv_type):
    return A.row_bytes(kv_type, D_K)


def _vis(n_q, n_head, n_kv, causal, shift=0):
    """vis of every row (t, h) -> int [n_q * n_head]"""
    v = np.array([max(A.visible(t, n_kv, n_q, causal) - shift, 0) for t in range(n_q)], np.int64)
    return np.repeat(v, n_head)


def reference(q, rows, n_kv, causal, scale):
    """q f32 [n_q, n_head, 576]; rows deq f32 [>= n_kv, 576] -> float64 [n_q, n_head, 512]; rows with no visible position are 0"""
    n_q, n_head, _ = q.shape
    R = n_q * n_head
    out = np.zeros((R, D_V), np.float64)
    if n_kv == 0:
        return out.reshape(n_q, n_head, D_V)
    vis = _vis(n_q, n_head, n_kv, causal)
    K = rows[:n_kv].astype(np.float64)
    s = float(np.float32(scale)) * (q.reshape(R, D_K).astype(np.float64) @ K.T)
    s[np.arange(n_kv)[None, :] >= vis[:, None]] = -np.inf
    live = vis > 0
    p = np.exp(s[live] - s[live].max(axis=1, keepdims=True))
    out[live] = (p / p.sum(axis=1, keepdims=True)) @ K[:, :D_V]
    return out.reshape(n_q, n_head, D_V)


def _h(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def _steps(qh, Kh, Vh, vis, st0, st1, sc, n_kv):
    """the step body over steps [st0, st1) for every row -> (m, l, O)"""
    R = qh.shape[0]
    m = np.full(R, -np.inf, np.float32)
    l = np.zeros(R, np.float32)
    O = np.zeros((R, D_V), np.float32)
    for st in range(st0, st1):
        j0, j1 = st * STEP, min(n_kv, st * STEP + STEP)
        if j1 <= j0:
            break
        s = (sc * (qh @ Kh[j0:j1].T).astype(np.float32)).astype(np.float32)
        seen = np.arange(j0, j1)[None, :] < vis[:, None]
        s = np.where(seen, s, np.float32(-np.inf)).astype(np.float32)
        mn = np.maximum(m, s.max(axis=1))
        some = mn != -np.inf
        with np.errstate(invalid="ignore"):
            alpha = np.where(m == -np.inf, np.float32(0), np.exp((m - mn).astype(np.float32))).astype(np.float32)
            P = _h(np.where(seen & some[:, None], np.exp((s - mn[:, None]).astype(np.float32)), np.float32(0)))
        l = (l * alpha + P.sum(axis=1, dtype=np.float32)).astype(np.float32)
        O = (O * alpha[:, None] + (P @ Vh[j0:j1]).astype(np.float32)).astype(np.float32)
        m = mn
    return m, l, O


def model(q, rows, n_kv, causal, scale, span, mutant=None):
    """the statement's arithmetic for the form n_q selects -> f32 [n_q, n_head, 512]"""
    n_q, n_head, _ = q.shape
    R = n_q * n_head
    out = np.zeros((R, D_V), np.float32)
    if n_kv == 0:
        return out.reshape(n_q, n_head, D_V)
    sc = np.float32(scale)
    vis = _vis(n_q, n_head, n_kv, causal, 1 if mutant == "vis_off" else 0)
    qh, Kh = _h(q.reshape(R, D_K)), _h(rows[:n_kv])
    Vh = Kh[:, 64:D_K] if mutant == "v_shift" else Kh[:, :D_V]
    if mutant == "score512":
        qh, Kh = qh[:, :D_V], Kh[:, :D_V]
    n_steps = (int(vis.max()) + STEP - 1) // STEP
    if n_steps == 0:
        return out.reshape(n_q, n_head, D_V)
    if form_of(n_q) == WALK:
        m, l, O = _steps(qh, Kh, Vh, vis, 0, n_steps, sc, n_kv)
        live = l != 0
        out[live] = O[live] / l[live, None]
        return out.reshape(n_q, n_head, D_V)
    per = span * (CHUNK // STEP)
    parts = []
    for s0 in range(0, n_steps, per):
        m, l, O = _steps(qh, Kh, Vh, vis, s0, min(s0 + per, n_steps), sc, n_kv)
        parts.append((m, l, O))                                      # (a row without a visible position in the span: m = -inf, l = 0, O = 0 -- b = 0 below)
    M = np.max([m for m, _, _ in parts], axis=0)
    L, Acc = np.zeros(R, np.float32), np.zeros((R, D_V), np.float32)
    for m, l, O in parts:
        with np.errstate(invalid="ignore"):
            b = np.where(m == M, np.float32(1), np.exp((m - M).astype(np.float32))).astype(np.float32)
        b = np.where(m == -np.inf, np.float32(0), b).astype(np.float32)
        if mutant == "merge_no_b":
            b = np.where(m == -np.inf, np.float32(0), np.float32(1)).astype(np.float32)
        L = (L + l * b).astype(np.float32)
        Acc = (Acc + O * b[:, None]).astype(np.float32)
    live = vis > 0
    out[live] = Acc[live] / L[live, None]
    return out.reshape(n_q, n_head, D_V)


# ---- the sweep both the CPU model test and the GPU tests walk ----
N_HEADS = (1, 16, 24)
N_QS = {SPLIT: (1, 3, 8), WALK: (9, 70)}


def n_kvs(span):
    return (1, 31, CHUNK, CHUNK + 1, 379, CHUNK * span + 1, 2 * CHUNK * span + 37)


def cases(form, span, n_heads=N_HEADS):
    """(kv_type, n_head, n_q, n_kv, causal) of a form"""
    return [(t, nh, n_q, n_kv, causal) for t in (F16, Q8_0) for nh in n_heads for n_q in N_QS[form] for n_kv in n_kvs(span) for causal in (True, False)]


_ROWS, _QS, _REFS = {}, {}, {}


def cache_rows(kv_type, n, tag="c"):
    """(raw uint8 [n, row_bytes], deq f32 [n, 576]) of a seeded cache of n positions, computed once; a shorter cache of a tag is a prefix of a longer"""
    key = (kv_type, tag)
    if key not in _ROWS or _ROWS[key][0].shape[0] < n:
        rng = np.random.default_rng([kv_type, 576] + [ord(c) for c in str(tag)])
        x = rng.uniform(-1, 1, (max(n, 2048), D_K)).astype(np.float32)
        raw = A.encode_rows(kv_type, x)
        _ROWS[key] = (raw, A.decode_rows(kv_type, raw, D_K))
    raw, deq = _ROWS[key]
    return raw[:n], deq[:n]


def queries(n_head, n_q, tag="q"):
    key = (n_head, n_q, tag)
    if key not in _QS:
        rng = np.random.default_rng([n_head, n_q, 77] + [ord(c) for c in str(tag)])
        _QS[key] = rng.uniform(-1, 1, (n_q, n_head, D_K)).astype(np.float32)
    return _QS[key]


def case_reference(case, tag="c"):
    """(ref float64 [n_q, n_head, 512], V deq) of a sweep case, computed once"""
    key = (case, tag)
    if key not in _REFS:
        kv_type, n_head, n_q, n_kv, causal = case
        deq = cache_rows(kv_type, n_kv, tag)[1]
        _REFS[key] = (reference(queries(n_head, n_q), deq, n_kv, causal, SCALE), deq[:, :D_V])
    return _REFS[key]
