"""numpy restatements for tests/test_attention_bias.py: tests/np_attention_ex.py's float64 REFERENCE and float32 / float16 MODEL extended by the mask
tensor and the ALiBi slopes of ggml_hip_attn_bias_dev / ggml_hip_attn_paged_bias_dev / ggml_hip_attn_paged_ragged_bias_dev (include/ggml_hip_ext.h,
ATTENTION WITH A MASK TENSOR AND ALiBi SLOPES).  np_attention.py and np_attention_ex.py are imported, not edited; without a mask the functions here
ARE np_attention_ex's.

  mask        float16 [n_q, >= n_kv]: row t is query row t, column j position j.  -inf hides position j from row t (besides the causal and the window
              rule); any other value mk changes the score to fma(slope_h, mk, s_j), s_j the (soft-capped) score; slope_h = 1 without slopes.
  reference   float64 over the dequantized cache, the softmax over the row's visible positions, sinks in the denominator only; a row that sees
              nothing is 0.
  model       DECODE: per chunk of the row's structural range the partial over the chunk's visible positions (an empty chunk contributes nothing),
              merged as np_attention_ex does.  PROMPT: the online softmax over the same chunks, f16 operands; an empty chunk leaves (m, l, O) alone.
  alibi_slopes  upstream's rule in float32: n2 = 2^floor(log2 n_head), m0 = 2^(-max_bias / n2), m1 = 2^(-(max_bias / 2) / n2),
              slope_h = m0^(h + 1) for h < n2, else m1^(2 (h - n2) + 1); max_bias = 0: ones.

THE INPUTS of the sweep are PEAKED: q in [0, 2], and every element of K_j is raised by b_j / sqrt(D), which adds about b_j to the score of position j:
b = 8 at positions 5 and 69, 8.7 at 128, 7 at 261 and 325 (peaks()) -- a handful of positions, some in every chunk, holds nearly all of the softmax,
about half of it in chunk 0 and half in chunk 1.  Hiding a chunk, hiding 30 % of the positions at random (the last row always loses its first and
its last peak), or biasing by the distance then moves dst by a large fraction of max |V|.  The soft-cap of the sweep is 10 (0.5 would flatten the
peaks) and the sinks are 0 .. 1, about the score of a position that is no peak.
test_every_mask_case_differs_from_the_unmasked_reference checks on the CPU that every case in which the mask CAN act (some visible position is
hidden, or a row sees two positions whose biases differ) lies at least 100 x its tolerance from the reference without the mask.

Measured for the model on the sweep (shapes() x variants(): D in {64, 128}, heads (4, 2) and (8, 1), both cache types, n_kv in {1, 129, 379}, n_q in
{1, 3} (DECODE) and {9, 140} (PROMPT); a random mask, the same with ALiBi slopes, the ALiBi distance mask, chunk [128, 256) hidden, the first
chunk hidden, one row hidden, and the mask under window 123, soft-cap 0.5 and sinks), statistic max |dst - ref| / max |V|:

    DECODE worst 7.23e-07 (recorded as 7.3e-07)           PROMPT worst 8.46e-04 (recorded as 8.5e-04)

The kernels are held to 4 x these, or to np_attention_ex's tolerances (2.88e-06, 3.4e-03) where those are larger:

    TOL_DECODE_BIAS = 2.92e-06      TOL_PROMPT_BIAS = 3.4e-03

The smallest distance of an acting case from its unmasked reference is 0.29 (DECODE) and 0.366 (PROMPT): above 100 x the tolerance in both forms.

test_the_bias_model_constants_are_what_the_model_measures recomputes both on the CPU."""
import numpy as np

import np_attention as A
import np_attention_ex as X

F16, Q8_0, CHUNK = A.F16, A.Q8_0, A.CHUNK
MODEL_WORST_DECODE_BIAS = 7.3e-07
MODEL_WORST_PROMPT_BIAS = 8.5e-04
TOL_DECODE_BIAS = max(4 * MODEL_WORST_DECODE_BIAS, X.TOL_DECODE_EX)
TOL_PROMPT_BIAS = max(4 * MODEL_WORST_PROMPT_BIAS, X.TOL_PROMPT_EX)
NINF = np.float16(-np.inf)


def alibi_slopes(n_head, max_bias):
    """upstream's ALiBi slopes, float32 [n_head]"""
    if max_bias == 0:
        return np.ones(n_head, np.float32)
    n2 = 1 << int(np.floor(np.log2(n_head)))
    m0 = np.power(np.float32(2), np.float32(-np.float32(max_bias) / np.float32(n2)), dtype=np.float32)
    m1 = np.power(np.float32(2), np.float32(-(np.float32(max_bias) / np.float32(2)) / np.float32(n2)), dtype=np.float32)
    return np.array([np.power(m0, np.float32(h + 1), dtype=np.float32) if h < n2 else np.power(m1, np.float32(2 * (h - n2) + 1), dtype=np.float32)
                     for h in range(n_head)], np.float32)


def _rows(n_q, n_kv, causal, window, mask):
    """per query row: (lo, hi, the visible positions as an index array)"""
    out = []
    for t in range(n_q):
        hi = A.visible(t, n_kv, n_q, causal)
        lo = X.window_lo(hi, window)
        j = np.arange(lo, hi)
        if mask is not None and hi > lo:
            j = j[np.asarray(mask[t, lo:hi]) != NINF]
        out.append((lo, hi, j))
    return out


def reference(q, K, V, n_kv, causal, scale, window=0, softcap=0.0, sinks=None, mask=None, slopes=None):
    """np_attention_ex.reference under a mask and slopes -> float64 [n_q, n_head, D]"""
    if mask is None:
        return X.reference(q, K, V, n_kv, causal, scale, window, softcap, sinks)
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    out = np.zeros((n_q, n_head, D), np.float64)
    q64, K64, V64 = q.astype(np.float64), K.astype(np.float64), V.astype(np.float64)
    sc, cap, scp = X._sc(scale, softcap)
    for t, (lo, hi, j) in enumerate(_rows(n_q, n_kv, causal, window, mask)):
        if len(j) == 0:
            continue
        mk = np.asarray(mask[t, j], np.float64)
        for h in range(n_head):
            dot = K64[j, h // G] @ q64[t, h]
            s = float(cap) * np.tanh(float(scp) * dot) if softcap else float(sc) * dot
            s = s + (1.0 if slopes is None else float(slopes[h])) * mk
            m = s.max() if sinks is None else max(s.max(), float(sinks[h]))
            p = np.exp(s - m)
            den = p.sum() + (0.0 if sinks is None else np.exp(float(sinks[h]) - m))
            out[t, h] = (p / den) @ V64[j, h // G]
    return out


def _biased(s, slope, mk):
    """fma(slope, mk, s) in one float32 rounding (the float64 product and sum of float32 / float16 values carry it exactly enough)"""
    return (np.float64(slope) * mk.astype(np.float64) + s.astype(np.float64)).astype(np.float32)


def model_decode(q, K, V, n_kv, causal, scale, window=0, softcap=0.0, sinks=None, mask=None, slopes=None):
    """the DECODE form's arithmetic under a mask, float32 -> f32 [n_q, n_head, D]"""
    if mask is None:
        return X.model_decode(q, K, V, n_kv, causal, scale, window, softcap, sinks)
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    sc, cap, scp = X._sc(scale, softcap)
    out = np.zeros((n_q, n_head, D), np.float32)
    for t, (lo, hi, vis) in enumerate(_rows(n_q, n_kv, causal, window, mask)):
        if len(vis) == 0:
            continue
        for h in range(n_head):
            slope = np.float32(1) if slopes is None else np.float32(slopes[h])
            parts = []
            for c in range(lo // CHUNK, (hi - 1) // CHUNK + 1):
                j = vis[(vis >= c * CHUNK) & (vis < c * CHUNK + CHUNK)]
                if len(j) == 0:
                    continue                                         # (the empty partial: b = exp(-inf) = 0 adds nothing)
                s = _biased(X._scores32(sc, cap, scp, K[j, h // G] @ q[t, h]), slope, np.asarray(mask[t, j], np.float32))
                m = s.max()
                p = np.exp(s - m).astype(np.float32)
                parts.append((m, p.sum(dtype=np.float32), (p @ V[j, h // G]).astype(np.float32)))
            M = max(m for m, _, _ in parts)
            if sinks is not None:
                M = max(M, np.float32(sinks[h]))
            L, Acc = np.float32(0), np.zeros(D, np.float32)
            for m, l, a in parts:
                with np.errstate(under="ignore"):
                    b = np.exp(np.float32(m - M)).astype(np.float32)
                L = np.float32(L + l * b)
                Acc = (Acc + a * b).astype(np.float32)
            if sinks is not None:
                with np.errstate(under="ignore"):
                    L = np.float32(L + np.exp(np.float32(np.float32(sinks[h]) - M)).astype(np.float32))
            out[t, h] = Acc / L
    return out


def model_prompt(q, K, V, n_kv, causal, scale, window=0, softcap=0.0, sinks=None, mask=None, slopes=None):
    """the PROMPT form's arithmetic under a mask: f16 operands, f32 sums, the online softmax per chunk -> f32 [n_q, n_head, D]"""
    if mask is None:
        return X.model_prompt(q, K, V, n_kv, causal, scale, window, softcap, sinks)
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    sc, cap, scp = X._sc(scale, softcap)
    qh, Kh, Vh = A._h(q), A._h(K), A._h(V)
    out = np.zeros((n_q, n_head, D), np.float32)
    for t, (lo, hi, vis) in enumerate(_rows(n_q, n_kv, causal, window, mask)):
        if len(vis) == 0:
            continue
        for h in range(n_head):
            slope = np.float32(1) if slopes is None else np.float32(slopes[h])
            m, l, O = np.float32(-np.inf), np.float32(0), np.zeros(D, np.float32)
            for c in range(lo // CHUNK, (hi - 1) // CHUNK + 1):
                j = vis[(vis >= c * CHUNK) & (vis < c * CHUNK + CHUNK)]
                if len(j) == 0:
                    continue                                         # (alpha = 1, every P = 0: the state is kept)
                s = _biased(X._scores32(sc, cap, scp, Kh[j, h // G] @ qh[t, h]), slope, np.asarray(mask[t, j], np.float32))
                mn = max(m, s.max())
                with np.errstate(under="ignore"):
                    alpha = np.float32(0) if m == -np.inf else np.exp(np.float32(m - mn)).astype(np.float32)
                    P = A._h(np.exp(s - mn).astype(np.float32))
                l = np.float32(l * alpha + P.sum(dtype=np.float32))
                O = (O * alpha + (P @ Vh[j, h // G]).astype(np.float32)).astype(np.float32)
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
HEADS = X.HEADS
N_KV = (1, CHUNK + 1, 3 * CHUNK - 5)
N_Q = {"decode": (1, 3), "prompt": (9, 140)}
PEAK = 8.0
WINDOW, SOFTCAP = 123, 10.0
MAX_BIAS = 8.0


def sinks_of(n_head):
    """the sinks of the sweep, f32 [n_head]: 0 .. 1, about the score of a position that is no peak"""
    return np.linspace(0.0, 1.0, n_head).astype(np.float32)


def shapes(form):
    """(D, n_head, n_head_kv, kv_type, n_q, n_kv) of the sweep for form 'decode' / 'prompt'"""
    return [(D, nh, nhk, t, n_q, n_kv) for D in (64, 128) for nh, nhk in HEADS for t in (F16, Q8_0) for n_kv in N_KV for n_q in N_Q[form]]


def peaks(n_kv):
    """what is added to the score of each position: PEAK at 5 and 69, PEAK + 0.7 at 128 (one position against two), PEAK - 1 at 261 and 325;
    n_kv = 134 (the draft tree: 129 committed positions, five drafts) has PEAK at every draft as well"""
    b = np.zeros(n_kv)
    for j, v in ((5, PEAK), (69, PEAK), (128, PEAK + 0.7), (261, PEAK - 1), (325, PEAK - 1)):
        if j < n_kv:
            b[j] = v
    if n_kv == 134:
        b[129:] = PEAK
    return b


_INPUTS = {}


def inputs(shape):
    """seeded (q, Kraw, Vraw, Kd, Vd) of a shape, computed once: q in [0, 2], K_j in [-1, 1] + PEAK / sqrt(D) at the peaks, V in [-1, 1] without zeros"""
    if shape not in _INPUTS:
        D, n_head, n_head_kv, kv_type, n_q, n_kv = shape
        rng = np.random.default_rng([23, D, n_head, n_head_kv, kv_type, n_q, n_kv])
        q = (rng.uniform(-1, 1, (n_q, n_head, D)) + 1.0).astype(np.float32)
        K = rng.uniform(-1, 1, (n_kv, n_head_kv, D)) + peaks(n_kv)[:, None, None] / np.sqrt(D)
        V = rng.uniform(-1, 1, (n_kv, n_head_kv, D)).astype(np.float32)
        V = np.where(np.abs(V) < 1.0 / 64, np.float32(1.0 / 64), V)  # (no element of V rounds to a zero: the sign of a zero never decides a bit test)
        Kraw, Vraw = A.encode_rows(kv_type, K.astype(np.float32)), A.encode_rows(kv_type, V)
        _INPUTS[shape] = (q, Kraw, Vraw, A.decode_rows(kv_type, Kraw, D), A.decode_rows(kv_type, Vraw, D))
    return _INPUTS[shape]


def random_mask(n_q, n_kv, seed):
    """about 30 % -inf, the rest biases in [-4, 0] rounded to f16; the last row hides the first and the last peak (position 0 where there is none)"""
    rng = np.random.default_rng([29, n_q, n_kv, seed])
    m = rng.uniform(-4, 0, (n_q, n_kv)).astype(np.float16)
    m[rng.uniform(0, 1, (n_q, n_kv)) < 0.3] = NINF
    m[n_q - 1, 5 if n_kv > 5 else 0] = NINF
    m[n_q - 1, np.flatnonzero(peaks(n_kv))[-1:]] = NINF              # (and the last one: the one a window leaves)
    return m


def alibi_mask(n_q, n_kv):
    """-(P - j) for the row at position P = n_kv - n_q + t and j <= P (exact in f16 below 2048); 0 above the diagonal, where causal = 1 hides it"""
    P = (n_kv - n_q + np.arange(n_q))[:, None]
    j = np.arange(n_kv)[None, :]
    return np.where(j <= P, -(P - j), 0).astype(np.float16)


def causal_mask(n_q, n_kv):
    """the causal pattern as a mask: 0 where row t sees position j under causal = 1, -inf elsewhere"""
    m = np.full((n_q, n_kv), NINF, np.float16)
    for t in range(n_q):
        m[t, :A.visible(t, n_kv, n_q, True)] = 0
    return m


VARIANTS = ("random", "random+slopes", "alibi", "chunk1", "chunk0", "row", "random+options")


def variant(shape, name):
    """the keyword arguments (causal, window, softcap, sinks, mask, slopes) of a named variant of a shape"""
    D, n_head, n_head_kv, kv_type, n_q, n_kv = shape
    kw = dict(causal=True, window=0, softcap=0.0, sinks=None, mask=None, slopes=None)
    if name in ("random", "random+slopes", "random+options"):
        kw["mask"] = random_mask(n_q, n_kv, 0)
        if name == "random+slopes":
            kw["slopes"] = alibi_slopes(n_head, MAX_BIAS)
        if name == "random+options":
            kw.update(window=WINDOW, softcap=SOFTCAP, sinks=sinks_of(n_head))
    elif name == "alibi":
        kw.update(mask=alibi_mask(n_q, n_kv), slopes=alibi_slopes(n_head, MAX_BIAS))
    elif name in ("chunk1", "chunk0"):
        m = np.zeros((n_q, n_kv), np.float16)
        c = 1 if name == "chunk1" else 0
        m[:, c * CHUNK:(c + 1) * CHUNK] = NINF
        kw["mask"] = m
    elif name == "row":
        m = np.zeros((n_q, n_kv), np.float16)
        m[n_q // 2] = NINF                                           # one row sees nothing: +0.0f; the others are the unmasked call's
        kw["mask"] = m
    else:
        raise KeyError(name)
    return kw


def can_act(shape, kw):
    """whether the mask can change anything: some visible position is hidden, or some row sees two positions whose biases differ"""
    n_q, n_kv = shape[4], shape[5]
    mask = kw["mask"]
    for t in range(n_q):
        hi = A.visible(t, n_kv, n_q, kw["causal"])
        lo = X.window_lo(hi, kw["window"])
        row = np.asarray(mask[t, lo:hi])
        if (row == NINF).any():
            return True
        if len(row) >= 2 and np.ptp(row.astype(np.float32)) > 0:
            return True
    return False


_REFS = {}


def case_reference(shape, name=None):
    """the float64 reference of a shape under a named variant, computed once; name None: the variant's options WITHOUT its mask and slopes is not
    meant -- None is plain causal attention"""
    key = (shape, name)
    if key not in _REFS:
        q, _, _, Kd, Vd = inputs(shape)
        kw = dict(causal=True) if name is None else variant(shape, name)
        _REFS[key] = reference(q, Kd, Vd, shape[5], kw.pop("causal"), 1.0 / np.sqrt(shape[0]), **kw)
    return _REFS[key]


def unmasked_reference(shape, name):
    """the variant's own options without its mask and slopes (what a kernel that ignored the mask would compute)"""
    key = (shape, name, "unmasked")
    if key not in _REFS:
        q, _, _, Kd, Vd = inputs(shape)
        kw = variant(shape, name)
        kw.update(mask=None, slopes=None)
        _REFS[key] = reference(q, Kd, Vd, shape[5], kw.pop("causal"), 1.0 / np.sqrt(shape[0]), **kw)
    return _REFS[key]
