"""numpy restatements for tests/test_attention.py: the float64 REFERENCE of attention over a dequantized KV cache, and the float32 / float16
MODEL of the arithmetic include/ggml_hip_ext.h writes down for ggml_hip_attn_dev's two forms (csrc/attn.hip's header comment).

  reference   dst[t, h] = softmax_j(scale * q[t, h] . K[j, h // G]) V[j, h // G] over the visible j, everything float64, K and V the
              DEQUANTIZED cache (F16 widened; Q8_0 (float32)q * d) -- never the library;
  model       DECODE: float32 throughout, chunks of 128 positions, per chunk (m, l, a) with p = exp(s - m), the partials merged against the
              global maximum in ascending chunk order.  PROMPT: Q, the staged K / V (a Q8_0 row: f16 of its dequantized value) and the
              weights P rounded to float16, scores and sums in float32, the online softmax per chunk of 128 with l the sum of the ROUNDED
              weights.  The model does not pin expf or the order of the additions inside a chunk (numpy's own).

The statistic of a case is  max |dst - ref| / max |V|.  Measured for the model on the sweep of tests/test_attention.py (cases(): D in
{64, 128}, (n_head, n_head_kv) in {(4, 4), (4, 2), (8, 1)}, both cache types, n_kv in {1, 31, 128, 129, 379}, seeded inputs in [-1, 1]):

    DECODE (n_q in {1, 3})            worst 1.13e-07 (recorded as 1.2e-07)
    PROMPT (n_q = 9, n_q = n_kv = 379) worst 3.68e-04 (recorded as 3.7e-04)

The kernels are held to 4 x these (the factor covers expf and the order of accumulation inside a chunk):

    TOL_DECODE = 4 * MODEL_WORST_DECODE = 4.8e-07        TOL_PROMPT = 4 * MODEL_WORST_PROMPT = 1.48e-03

test_the_model_constants_are_what_the_model_measures recomputes both on the CPU."""
import numpy as np

F16, Q8_0 = 1, 8
CHUNK = 128
DECODE_MAX_Q = 8
MODEL_WORST_DECODE = 1.2e-07
MODEL_WORST_PROMPT = 3.7e-04
TOL_DECODE = 4 * MODEL_WORST_DECODE
TOL_PROMPT = 4 * MODEL_WORST_PROMPT


def row_bytes(kv_type, D):
    return 2 * D if kv_type == F16 else D // 32 * 36


def quantize_q8_0(x):
    """quantize_row_q8_0 restated (Ggml.cs:733-762): x f32 [..., k] -> uint8 [..., k // 32 * 36]; held against the oracle in the tests"""
    x = np.asarray(x, np.float32)
    b = x.reshape(x.shape[:-1] + (x.shape[-1] // 32, 32))
    amax = np.abs(b).max(axis=-1)
    d = (amax / np.float32(127.0)).astype(np.float32)
    with np.errstate(divide="ignore"):
        inv = np.where(d != 0, np.float32(1.0) / d, np.float32(0.0)).astype(np.float32)
    q = np.rint(b * inv[..., None]).astype(np.int8)
    out = np.zeros(b.shape[:-1] + (36,), np.uint8)
    out[..., :4] = d[..., None].view(np.uint8)
    out[..., 4:] = q.view(np.uint8)
    return out.reshape(x.shape[:-1] + (-1,))


def encode_rows(kv_type, x):
    """f32 [..., D] -> the cache's bytes [..., row_bytes]"""
    x = np.asarray(x, np.float32)
    if kv_type == F16:
        with np.errstate(over="ignore"):
            return np.ascontiguousarray(x.astype(np.float16)).view(np.uint8).reshape(x.shape[:-1] + (-1,))
    return quantize_q8_0(x)


def decode_rows(kv_type, raw, D):
    """the cache's bytes [..., row_bytes] -> deq f32 [..., D]"""
    raw = np.ascontiguousarray(raw)
    if kv_type == F16:
        return raw.view(np.float16).astype(np.float32).reshape(raw.shape[:-1] + (D,))
    b = raw.reshape(raw.shape[:-1] + (D // 32, 36))
    d = np.ascontiguousarray(b[..., :4]).view(np.float32)
    q = np.ascontiguousarray(b[..., 4:]).view(np.int8).astype(np.float32)
    return (q * d).astype(np.float32).reshape(raw.shape[:-1] + (D,))


def visible(t, n_kv, n_q, causal):
    return int(min(max(n_kv - n_q + t + 1, 0), n_kv)) if causal else int(n_kv)


def reference(q, K, V, n_kv, causal, scale):
    """q f32 [n_q, n_head, D]; K, V deq f32 [>= n_kv, n_head_kv, D] -> float64 [n_q, n_head, D]; rows with no visible position are 0"""
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    out = np.zeros((n_q, n_head, D), np.float64)
    q64, K64, V64 = q.astype(np.float64), K.astype(np.float64), V.astype(np.float64)
    for t in range(n_q):
        n = visible(t, n_kv, n_q, causal)
        if n == 0:
            continue
        for h in range(n_head):
            s = float(np.float32(scale)) * (K64[:n, h // G] @ q64[t, h])
            p = np.exp(s - s.max())
            out[t, h] = (p / p.sum()) @ V64[:n, h // G]
    return out


def model_decode(q, K, V, n_kv, causal, scale):
    """the DECODE form's arithmetic in float32 -> f32 [n_q, n_head, D]"""
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    sc = np.float32(scale)
    out = np.zeros((n_q, n_head, D), np.float32)
    for t in range(n_q):
        n = visible(t, n_kv, n_q, causal)
        if n == 0:
            continue
        for h in range(n_head):
            parts = []
            for j0 in range(0, n, CHUNK):
                j1 = min(n, j0 + CHUNK)
                s = (sc * (K[j0:j1, h // G] @ q[t, h]).astype(np.float32)).astype(np.float32)
                m = s.max()
                p = np.exp(s - m).astype(np.float32)
                parts.append((m, p.sum(dtype=np.float32), (p @ V[j0:j1, h // G]).astype(np.float32)))
            M = max(m for m, _, _ in parts)
            L, A = np.float32(0), np.zeros(D, np.float32)
            for m, l, a in parts:
                b = np.exp(np.float32(m - M)).astype(np.float32)
                L = np.float32(L + l * b)
                A = (A + a * b).astype(np.float32)
            out[t, h] = A / L
    return out


def _h(x):
    with np.errstate(over="ignore"):
        return np.asarray(x, np.float32).astype(np.float16).astype(np.float32)


def model_prompt(q, K, V, n_kv, causal, scale):
    """the PROMPT form's arithmetic: f16 operands, f32 sums, the online softmax per chunk -> f32 [n_q, n_head, D]"""
    n_q, n_head, D = q.shape
    G = n_head // K.shape[1]
    sc = np.float32(scale)
    qh, Kh, Vh = _h(q), _h(K), _h(V)
    out = np.zeros((n_q, n_head, D), np.float32)
    for t in range(n_q):
        n = visible(t, n_kv, n_q, causal)
        if n == 0:
            continue
        for h in range(n_head):
            m, l, O = np.float32(-np.inf), np.float32(0), np.zeros(D, np.float32)
            for j0 in range(0, n, CHUNK):
                j1 = min(n, j0 + CHUNK)
                s = (sc * (Kh[j0:j1, h // G] @ qh[t, h]).astype(np.float32)).astype(np.float32)
                mn = max(m, s.max())
                alpha = np.float32(0) if m == -np.inf else np.exp(np.float32(m - mn)).astype(np.float32)
                P = _h(np.exp(s - mn).astype(np.float32))
                l = np.float32(l * alpha + P.sum(dtype=np.float32))
                O = (O * alpha + (P @ Vh[j0:j1, h // G]).astype(np.float32)).astype(np.float32)
                m = mn
            out[t, h] = O / l
    return out


def statistic(dst, ref, V):
    return float(np.abs(np.asarray(dst, np.float64) - ref).max() / np.abs(V).max())


# ---- the sweep both the CPU model test and the GPU tests walk ----
HEADS = ((4, 4), (4, 2), (8, 1))
N_KV = (1, 31, CHUNK, CHUNK + 1, 3 * CHUNK - 5)
PROMPT_MIN_Q = DECODE_MAX_Q + 1


def cases(form):
    """(D, n_head, n_head_kv, kv_type, n_q, n_kv) of the common sweep for form 'decode' / 'prompt'"""
    out = []
    for D in (64, 128):
        for n_head, n_head_kv in HEADS:
            for kv_type in (F16, Q8_0):
                for n_kv in N_KV:
                    if form == "decode":
                        out += [(D, n_head, n_head_kv, kv_type, 1, n_kv), (D, n_head, n_head_kv, kv_type, 3, n_kv)]
                    else:
                        out.append((D, n_head, n_head_kv, kv_type, PROMPT_MIN_Q, n_kv))
                        if n_kv == 3 * CHUNK - 5:
                            out.append((D, n_head, n_head_kv, kv_type, n_kv, n_kv))
    return out


_INPUTS = {}


def inputs(case):
    """seeded q, the cache's bytes and their dequantized values for a case, computed once: (q, Kraw, Vraw, Kd, Vd), |.| <= 1"""
    if case not in _INPUTS:
        D, n_head, n_head_kv, kv_type, n_q, n_kv = case
        rng = np.random.default_rng([D, n_head, n_head_kv, kv_type, n_q, n_kv])
        q = rng.uniform(-1, 1, (n_q, n_head, D)).astype(np.float32)
        K = rng.uniform(-1, 1, (n_kv, n_head_kv, D)).astype(np.float32)
        V = rng.uniform(-1, 1, (n_kv, n_head_kv, D)).astype(np.float32)
        Kraw, Vraw = encode_rows(kv_type, K), encode_rows(kv_type, V)
        _INPUTS[case] = (q, Kraw, Vraw, decode_rows(kv_type, Kraw, D), decode_rows(kv_type, Vraw, D))
    return _INPUTS[case]


_REFS = {}


def case_reference(case, causal=True):
    key = (case, causal)
    if key not in _REFS:
        D, n_head, n_head_kv, kv_type, n_q, n_kv = case
        q, _, _, Kd, Vd = inputs(case)
        _REFS[key] = reference(q, Kd, Vd, n_kv, causal, 1.0 / np.sqrt(D))
    return _REFS[key]
