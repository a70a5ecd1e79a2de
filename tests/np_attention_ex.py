"""numpy restatements for tests/test_attention_ex.py: tests/np_attention.py's float64 REFERENCE and float32 / float16 MODEL extended by the three
options of ggml_hip_attn_ex_dev / ggml_hip_attn_paged_ex_dev (include/ggml_hip_ext.h, ATTENTION OPTIONS): a sliding window, attention sinks, a
logit soft-cap.  np_attention.py itself is imported, not edited; with every option off the functions here ARE its functions (consequence 1).

  reference   row t sees lo_t <= j < hi_t, hi_t = visible(t), lo_t = max(0, hi_t - W); s = cap * tanh(scale / cap * q . K_j) under a cap;
              dst = sum_j p_j V_j with p = exp(s_j) / (sum_j exp(s_j) + exp(sink_h)); everything float64, K and V the dequantized cache.
  model       DECODE: per chunk lo_t // 128 .. (hi_t - 1) // 128 the partial (m, l, a) over the row's visible positions of the chunk, merged
              against M = max(max m_c, sink) in ascending order, then L += exp(sink - M).  PROMPT: the online softmax over the same chunks,
              then mn = max(m, sink), alpha = exp(m - mn), l = l alpha + exp(sink - mn), O = O alpha.  sc' = scale / cap is one float32 division.

THE INPUTS of the sweep are not np_attention's: with q, K, V uniform in [-1, 1] the softmax is nearly flat, and dropping a position, adding a
sink or capping the scores moves dst by less than the PROMPT tolerance -- a kernel that ignored an option would pass.  Here every q element
is shifted by +1 and every element of K_j by -2 ln(j + 1) / sqrt(D), which adds about -2 ln(j + 1) to the score of position j: the unvaried
softmax weighs position j like (j + 1)^-2, position 0 holds about 0.6 of it, and every window that hides position 0, a sink of 2 .. 3 and a
cap of 0.5 each move dst by a large fraction of max |V|.  test_every_variant_case_differs_from_the_unvaried_reference checks that on the CPU:
every case in which the option CAN act (a window below some row's hi_t; a cap with two visible positions in some row; a sink with one) differs
from the unvaried float64 reference by at least 100 x its tolerance in the statistic max |dst - ref| / max |V|.

Measured for the model on the sweep (shapes() x variants(): D in {64, 128}, heads (4, 2) and (8, 1), both cache types, n_kv in {1, 129, 379}, n_q in
{1, 3} (DECODE) and {9, 130} (PROMPT), window alone for W in {1, 5, 123, 128, 200}, sinks alone, cap alone, and all three for every W):

    DECODE worst 7.04e-07 (recorded as 7.2e-07)           PROMPT worst 8.39e-04 (recorded as 8.5e-04)

Both exceed np_attention's constants (1.2e-07, 3.7e-04): the shifted q and K are up to 2 and about 2.5 in magnitude, so their f16 roundings and
the float32 dot products carry larger absolute errors, and fewer visible positions average less of it away.  The kernels are held to 4 x these:

    TOL_DECODE_EX = 4 * MODEL_WORST_DECODE_EX = 2.88e-06      TOL_PROMPT_EX = 4 * MODEL_WORST_PROMPT_EX = 3.4e-03

test_the_ex_model_constants_are_what_the_model_measures recomputes both on the CPU."""
import numpy as np

import np_attention as A

F16, Q8_0, CHUNK = A.F16, A.Q8_0, A.CHUNK
MODEL_WORST_DECODE_EX = 7.2e-07
MODEL_WORST_PROMPT_EX = 8.5e-04
TOL_DECODE_EX = 4 * MODEL_WORST_DECODE_EX if MODEL_WORST_DECODE_EX > A.MODEL_WORST_DECODE else A.TOL_DECODE
TOL_PROMPT_EX = 4 * MODEL_WORST_PROMPT_EX if MODEL_WORST_PROMPT_EX > A.MODEL_WORST_PROMPT else A.TOL_PROMPT


def window_lo(hi, window):
    return max(0, hi - window) if window > 0 else 0


def _sc(scale, softcap):
    """(float32 scale, float32 cap, float32 sc' = scale / cap in one division)"""
    sc, cap = np.float32(scale), np.float32(softcap)
    return sc, cap, (np.float32(sc / cap) if softcap else np.float32(0))


def reference(q, K, V, n_kv, causal, scale, window=0, softcap=0.0, sinks=None):
    """np_attention.reference under the options -> float64 [n_q, n_head, D]; rows with no visible position are 0"""
    if not window and not softcap and sinks is None:
        return A.reference(q, K, V, n_kv, causal, scale)
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    out = np.zeros((n_q, n_head, D), np.float64)
    q64, K64, V64 = q.astype(np.float64), K.astype(np.float64), V.astype(np.float64)
    sc, cap, scp = _sc(scale, softcap)
    for t in range(n_q):
        hi = A.visible(t, n_kv, n_q, causal)
        lo = window_lo(hi, window)
        if hi == 0:
            continue
        for h in range(n_head):
            dot = K64[lo:hi, h // G] @ q64[t, h]
            s = float(cap) * np.tanh(float(scp) * dot) if softcap else float(sc) * dot
            m = s.max() if sinks is None else max(s.max(), float(sinks[h]))
            p = np.exp(s - m)
            den = p.sum() + (0.0 if sinks is None else np.exp(float(sinks[h]) - m))
            out[t, h] = (p / den) @ V64[lo:hi, h // G]
    return out


def _scores32(sc, cap, scp, dot):
    dot = dot.astype(np.float32)
    return (cap * np.tanh(scp * dot).astype(np.float32)).astype(np.float32) if cap else (sc * dot).astype(np.float32)


def model_decode(q, K, V, n_kv, causal, scale, window=0, softcap=0.0, sinks=None):
    """the DECODE form's arithmetic under the options, float32 -> f32 [n_q, n_head, D]"""
    if not window and not softcap and sinks is None:
        return A.model_decode(q, K, V, n_kv, causal, scale)
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    sc, cap, scp = _sc(scale, softcap)
    out = np.zeros((n_q, n_head, D), np.float32)
    for t in range(n_q):
        hi = A.visible(t, n_kv, n_q, causal)
        lo = window_lo(hi, window)
        if hi == 0:
            continue
        for h in range(n_head):
            parts = []
            for c in range(lo // CHUNK, (hi - 1) // CHUNK + 1):
                j0, j1 = max(c * CHUNK, lo), min(hi, c * CHUNK + CHUNK)
                s = _scores32(sc, cap, scp, K[j0:j1, h // G] @ q[t, h])
                m = s.max()
                p = np.exp(s - m).astype(np.float32)
                parts.append((m, p.sum(dtype=np.float32), (p @ V[j0:j1, h // G]).astype(np.float32)))
            M = max(m for m, _, _ in parts)
            if sinks is not None:
                M = max(M, np.float32(sinks[h]))
            L, Acc = np.float32(0), np.zeros(D, np.float32)
            for m, l, a in parts:
                b = np.exp(np.float32(m - M)).astype(np.float32)
                L = np.float32(L + l * b)
                Acc = (Acc + a * b).astype(np.float32)
            if sinks is not None:
                with np.errstate(under="ignore"):
                    L = np.float32(L + np.exp(np.float32(np.float32(sinks[h]) - M)).astype(np.float32))
            out[t, h] = Acc / L
    return out


def model_prompt(q, K, V, n_kv, causal, scale, window=0, softcap=0.0, sinks=None):
    """the PROMPT form's arithmetic under the options: f16 operands, f32 sums, the online softmax per chunk -> f32 [n_q, n_head, D]"""
    if not window and not softcap and sinks is None:
        return A.model_prompt(q, K, V, n_kv, causal, scale)
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    sc, cap, scp = _sc(scale, softcap)
    qh, Kh, Vh = A._h(q), A._h(K), A._h(V)
    out = np.zeros((n_q, n_head, D), np.float32)
    for t in range(n_q):
        hi = A.visible(t, n_kv, n_q, causal)
        lo = window_lo(hi, window)
        if hi == 0:
            continue
        for h in range(n_head):
            m, l, O = np.float32(-np.inf), np.float32(0), np.zeros(D, np.float32)
            for c in range(lo // CHUNK, (hi - 1) // CHUNK + 1):
                j0, j1 = max(c * CHUNK, lo), min(hi, c * CHUNK + CHUNK)
                s = _scores32(sc, cap, scp, Kh[j0:j1, h // G] @ qh[t, h])
                mn = max(m, s.max())
                alpha = np.float32(0) if m == -np.inf else np.exp(np.float32(m - mn)).astype(np.float32)
                P = A._h(np.exp(s - mn).astype(np.float32))
                l = np.float32(l * alpha + P.sum(dtype=np.float32))
                O = (O * alpha + (P @ Vh[j0:j1, h // G]).astype(np.float32)).astype(np.float32)
                m = mn
            if sinks is not None:
                sink = np.float32(sinks[h])
                mn = max(m, sink)
                with np.errstate(under="ignore"):
                    alpha = np.exp(np.float32(m - mn)).astype(np.float32)
                    l = np.float32(l * alpha + np.exp(np.float32(sink - mn)).astype(np.float32))
                O = (O * alpha).astype(np.float32)
            out[t, h] = O / l
    return out


# ---- the sweep both the CPU tests and the GPU tests walk ----
HEADS = ((4, 2), (8, 1))
N_KV = (1, CHUNK + 1, 3 * CHUNK - 5)
N_Q = {"decode": (1, 3), "prompt": (9, 130)}
WINDOWS = (1, 5, 123, 128, 200)
SOFTCAP = 0.5
ALPHA = 2.0                                                          # the score of position j is shifted by about -ALPHA ln(j + 1)


def sinks_of(n_head):
    """the sinks of the sweep, f32 [n_head]: 2 .. 3, above every score of the shifted inputs (the largest is near 0)"""
    return np.linspace(2.0, 3.0, n_head).astype(np.float32)


def variants(n_head):
    """the (window, softcap, sinks) of a shape: window alone for every W, sinks alone, the cap alone, all three for every W"""
    s = sinks_of(n_head)
    return [(W, 0.0, None) for W in WINDOWS] + [(0, 0.0, s), (0, SOFTCAP, None)] + [(W, SOFTCAP, s) for W in WINDOWS]


def shapes(form):
    """(D, n_head, n_head_kv, kv_type, n_q, n_kv) of the sweep for form 'decode' / 'prompt'"""
    return [(D, nh, nhk, t, n_q, n_kv) for D in (64, 128) for nh, nhk in HEADS for t in (F16, Q8_0) for n_kv in N_KV for n_q in N_Q[form]]


def can_act(shape, variant, causal=True):
    """whether the options can change anything in a case: a window below some row's hi, a cap with two visible positions, a sink with one"""
    n_q, n_kv = shape[4], shape[5]
    window, softcap, sinks = variant
    top = max(A.visible(t, n_kv, n_q, causal) for t in range(n_q))
    return (window > 0 and top > window) or (softcap != 0 and top >= 2) or (sinks is not None and top >= 1)


_INPUTS = {}


def inputs(shape):
    """seeded (q, Kraw, Vraw, Kd, Vd) of a shape, computed once: q in [0, 2], K_j in [-1, 1] - ALPHA ln(j + 1) / sqrt(D), V in [-1, 1]"""
    if shape not in _INPUTS:
        D, n_head, n_head_kv, kv_type, n_q, n_kv = shape
        rng = np.random.default_rng([20, D, n_head, n_head_kv, kv_type, n_q, n_kv])
        q = (rng.uniform(-1, 1, (n_q, n_head, D)) + 1.0).astype(np.float32)
        K = rng.uniform(-1, 1, (n_kv, n_head_kv, D)) - ALPHA * np.log(np.arange(n_kv) + 1.0)[:, None, None] / np.sqrt(D)
        V = rng.uniform(-1, 1, (n_kv, n_head_kv, D)).astype(np.float32)
        Kraw, Vraw = A.encode_rows(kv_type, K.astype(np.float32)), A.encode_rows(kv_type, V)
        _INPUTS[shape] = (q, Kraw, Vraw, A.decode_rows(kv_type, Kraw, D), A.decode_rows(kv_type, Vraw, D))
    return _INPUTS[shape]


_REFS = {}


def _vkey(variant):
    return (variant[0], variant[1], variant[2] is not None)


def case_reference(shape, variant=(0, 0.0, None), n_kv=None, causal=True):
    """the float64 reference of a shape under a variant (the unvaried one by default), computed once"""
    n_kv = shape[5] if n_kv is None else n_kv
    key = (shape, _vkey(variant), n_kv, causal)
    if key not in _REFS:
        q, _, _, Kd, Vd = inputs(shape)
        _REFS[key] = reference(q, Kd, Vd, n_kv, causal, 1.0 / np.sqrt(shape[0]), *variant)
    return _REFS[key]
