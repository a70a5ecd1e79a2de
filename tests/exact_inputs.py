"""Exact inputs for the bitwise tier (tests/test_exact_cpu.py, tests/test_exact_gpu.py).  Test infrastructure only: no conftest.

Every scale is a power of two.  An activation block holds one element of magnitude exactly 127 * 2^b, so the Q8_0 rule gives
d = amax / 127 = 2^b and id = 2^-b with no rounding; a weight block is written raw with d = 2^a and m = mu * 2^a.  Every block term
(d_w * d_a) * sumi -- and the reference's per-element Q4_1 form (d0 * q + m0) * (d1 * qy) -- is then an integer times 2^(a + b).  With
a base exponent per weight row (a) and per activation row (b), and block exponents at or above them, an output element is S * 2^(a + b)
for the integer S = sum_k w_k * x_k (w, x the elements in units of 2^a, 2^b), and
whenever sum_k |w_k * x_k| < 2^24 every partial sum of every association is an f32 integer multiple of 2^(a + b): exact.  The
reference's sequential f32 loop then returns the exact value, and so must any correct kernel, whatever its K split, tile or MFMA.

Activation elements (n + 1/2) * 2^b are exact ties of x * id, so a wrong rounding rule moves a result by a representable, nonzero amount.
Near-ties (a non-power-of-two amax, x with rint(f32(x * id)) != rint(f32(x / d))) separate multiplying by the reciprocal from dividing.

exact_product() computes from the construction's own integers and exponents -- never through a dequantizer.
"""
import numpy as np

F32, F16, Q4_0, Q4_1, Q4_2, Q5_0, Q5_1, Q8_0, Q8_1 = 0, 1, 2, 3, 4, 6, 7, 8, 9
LEGACY = (Q4_0, Q4_1, Q4_2, Q5_0, Q5_1, Q8_0)
TYPE_SIZE = {Q4_0: 20, Q4_1: 24, Q4_2: 10, Q5_0: 22, Q5_1: 24, Q8_0: 36}
BLCK = {Q4_0: 32, Q4_1: 32, Q4_2: 16, Q5_0: 32, Q5_1: 32, Q8_0: 32}
F16_SCALE = (Q4_2, Q5_0, Q5_1)          # d (and m) stored as IEEE halves; the others as f32
MIN_TYPES = (Q4_1, Q5_1)

# exponent zones of a + b (the exponent of an element's unit term)
ZONES = ("normal", "tiny", "subnormal")
EXACT_BOUND = 1 << 24


def wmax(t):
    """the largest |integer weight| a raw block of type t holds here (min types: |q + mu| with mu in MU_RANGE)"""
    return {Q4_0: 8, Q4_2: 8, Q5_0: 16, Q8_0: 128, Q4_1: 15 + 8, Q5_1: 31 + 8}[t]


MU_RANGE = (-8, 8)    # m = mu * 2^a, mu a small integer (negative and positive)


# ------------------------------------------------------------------------------------------------------------- exponents
def zone_exponents(t, zone, rng, n_w, n_x):
    """per weight row a, per activation row b, such that a + b falls in `zone` for every pair and each scale is representable:
    f32 d for Q4_0 / Q4_1 / Q8_0 down to the f32 subnormals, f16 d for the others down to 2^-24 (the f16 subnormals); b >= -120 keeps
    id = 2^-b finite, and 127 * 2^b stays normal."""
    f16 = t in F16_SCALE
    if zone == "normal":
        a = rng.integers(-12, 3, n_w)
        b = rng.integers(-10, 6, n_x)
    elif zone == "tiny":                 # a + b around -110: normal f32 results far below 1
        a = rng.integers(-24, -13, n_w) if f16 else rng.integers(-62, -57, n_w)
        b = rng.integers(-92, -87, n_x) if f16 else rng.integers(-52, -47, n_x)
    elif zone == "subnormal":            # a + b in [-149, -127]: unit terms below the smallest normal f32
        if f16:
            a = rng.integers(-24, -14, n_w)                       # (f16 subnormal d included)
            b = rng.integers(-120, -112, n_x)
        else:
            a = rng.integers(-142, -132, n_w)                     # an f32-subnormal weight d
            b = rng.integers(-6, 3, n_x)
    else:
        raise ValueError(zone)
    a, b = np.asarray(a, np.int64), np.asarray(b, np.int64)
    if zone == "subnormal":
        s = a[:, None] + b[None, :]
        assert s.min() >= -149 and s.max() <= -127, (t, s.min(), s.max())
    return a, b


# ------------------------------------------------------------------------------------------------------------- activations
def act_rows(N, K, b, rng, wbound, ties=True, jitter=0):
    """N f32 rows of K elements with per-row exponent b[n].  Returns (x f32 [N, K], q int64 [N, K] the Q8_0 quants every rule must
    give, d f32 [N, K/32] the block scales, info dict of counts).  `wbound` is the largest |integer weight| the rows will meet:
    the sum of |q| per row is held below 2^24 / wbound, so the bound of assert_exactly_representable holds for any such weight.

    Block kinds (cycled over rows and blocks): 'mixed' (anchor +-127, a random body, six ties), 'zero', 'outlier' (the anchor alone),
    'const' (all +-127), 'negative' (every element <= 0, six ties).  Ties are (n + 1/2) for n in [-127, 126] -- both parities, both
    signs, 126.5 and -126.5 among them -- and their quant is the half-to-even integer.  A long K lowers the body's range, then keeps
    ties in a prefix of the blocks only, then turns 'const' blocks into 'outlier' ones, so that the bound holds.  With `jitter`, a block's
    exponent is b[n] + e for e drawn per block from 0..jitter (act_ints() gives the integers in units of 2^b[n])."""
    assert K % 32 == 0
    nb = K // 32
    b = np.asarray(b, np.int64)
    budget = (EXACT_BOUND - 1) // (wbound << jitter) - 1
    per_block = budget // nb
    body = int(max(0, min(100, (per_block - 7 * 127) // 31)))
    cyc = np.array(KINDS)
    kind = cyc[(np.arange(N)[:, None] + np.arange(nb)[None, :]) % len(cyc)]
    if per_block < 32 * 127:
        kind[kind == "const"] = "outlier"
    tie_blk = np.isin(kind, ("mixed", "negative")) & ties
    if per_block < 7 * 127 + 31 * body:                          # ties in a prefix of the blocks only
        spare = budget - nb * (127 + 31 * body)
        tie_blk &= np.cumsum(tie_blk, axis=1) <= max(spare // (6 * 127), 0)
    neg = kind == "negative"
    sgn = np.where(neg | (rng.random((N, nb)) < 0.5), -1.0, 1.0)
    pos = rng.integers(0, 32, (N, nb))
    blk = np.zeros((N, nb, 32))
    if body:
        v = rng.integers(-body, body + 1, (N, nb, 32)).astype(np.float64)
        v = np.where(neg[..., None], -np.abs(v), v)
        blk = np.where(np.isin(kind, ("mixed", "negative"))[..., None], v, 0.0)
    # six tie positions per block, none of them the anchor
    key = rng.random((N, nb, 32))
    np.put_along_axis(key, pos[..., None], 2.0, axis=-1)
    tp = np.argsort(key, axis=-1)[..., :6]
    tn = rng.integers(-127, 127, (N, nb, 6))
    tn = np.where(neg[..., None], -(np.abs(tn) % 127) - 1, tn)
    tn[..., 0] = np.where(neg, -127, 126)                        # 126.5 (roundf: 127, rint: 126) / -126.5
    cur = np.take_along_axis(blk, tp, axis=-1)
    np.put_along_axis(blk, tp, np.where(tie_blk[..., None], tn + 0.5, cur), axis=-1)
    np.put_along_axis(blk, pos[..., None], (127 * sgn)[..., None], axis=-1)
    blk = np.where((kind == "const")[..., None], 127 * sgn[..., None], blk)
    blk = np.where((kind == "zero")[..., None], 0.0, blk)
    q = np.rint(blk).astype(np.int64)                            # numpy rint: half to even
    eb = b[:, None] + (rng.integers(0, jitter + 1, (N, nb)) if jitter else 0 * pos)
    d = np.where(kind == "zero", 0.0, np.ldexp(np.float32(1), eb)).astype(np.float32)
    tv = tn[tie_blk]
    info = {"ties": int(tv.size), "ties_odd": int((tv % 2 != 0).sum()), "ties_even": int((tv % 2 == 0).sum()),
            "ties_neg": int((tv < 0).sum()), "ties_126_5": int((np.abs(tv + 0.5) == 126.5).sum()),
            "blocks": {str(k): int((kind == k).sum()) for k in KINDS}}
    assert ((np.abs(q) << (eb - b[:, None])[..., None]).sum(axis=(1, 2)) * wbound < EXACT_BOUND).all()
    x = np.ldexp(blk, eb[..., None]).reshape(N, K)
    xs = x.astype(np.float32)
    assert np.array_equal(xs.astype(np.float64), x), "an activation is not an f32"
    return xs, q.reshape(N, K), d, info


KINDS = ("mixed", "zero", "mixed", "outlier", "negative", "mixed", "const", "mixed")


def act_ints(q, d, b):
    """activation quants q [N, K] with block scales d [N, K/32] as integers in units of 2^b[n] (what exact_product takes)"""
    N, K = q.shape
    f = np.where(d > 0, np.ldexp(d.astype(np.float64), -np.asarray(b, np.int64)[:, None]), 0).astype(np.int64)
    return (q.reshape(N, -1, 32) * f[..., None]).reshape(N, K)


def _block_rule(t, blk):
    """(offset, d, id, code(v_scaled)) of type t's quantizer on one block, in f32 as the reference computes them"""
    blk = blk.astype(np.float32)
    if t in (Q4_0, Q4_2, Q5_0):
        mx = blk[int(np.argmax(np.abs(blk)))]                       # the first max-|x| element
        d = np.float32(mx / np.float32(-8 if t != Q5_0 else -16))
        off = np.float32(0)
    elif t in (Q4_1, Q5_1):
        off = np.float32(blk.min())
        d = np.float32((blk.max() - off) / np.float32(15 if t == Q4_1 else 31))
    else:
        d = np.float32(np.abs(blk).max() / np.float32(127))
        off = np.float32(0)
    idv = np.float32(np.float32(1) / d) if d != 0 else np.float32(0)
    code = {Q4_0: lambda v: min(15.0, np.rint(v) + 8), Q4_2: lambda v: min(15.0, np.rint(v) + 8),
            Q5_0: lambda v: min(31.0, np.trunc(np.float32(v + np.float32(16.5)))), Q4_1: np.rint,
            Q5_1: lambda v: np.trunc(np.float32(v + np.float32(0.5)))}.get(t, np.rint)
    return off, d, idv, code


def near_tie_rows(N, K, rng, t=Q8_0, per_block=4):
    """rows for type t's quantizer (Q8_0 / Q8_1: the activation rule) whose blocks have a non-power-of-two scale, holding elements x whose
    code differs between f32((x - off) * id) -- what the reference computes -- and f32((x - off) / d): a kernel that divides instead of
    multiplying by the reciprocal gets another quant.  Found by a float32 search at construction time, a few ulps around
    off + (k + 1/2) * d; the block's max, min and first max-|x| element are left as they are.  Returns (x f32 [N, K], count planted)."""
    bs = 16 if t == Q4_2 else 32
    x = (rng.standard_normal((N, K)) * 3).astype(np.float32)
    planted = 0
    for n in range(N):
        for i in range(K // bs):
            blk = x[n, bs * i: bs * i + bs]
            off, d, idv, code = _block_rule(t, blk)
            lo, hi = blk.min(), blk.max()
            amax = np.abs(blk).max()
            free = [j for j in range(bs) if lo < blk[j] < hi and abs(blk[j]) < amax]
            found = []
            for _ in range(200):
                if len(found) >= min(per_block, len(free)):
                    break
                k = int(rng.integers(-130, 130))
                c = np.float32(np.float64(off) + (k + 0.5) * np.float64(abs(d)))
                for u in range(13):
                    v = c
                    step = np.float32(np.inf if u % 2 else -np.inf)
                    for _s in range((u + 1) // 2):
                        v = np.nextafter(v, step)
                    if not (lo < v < hi and abs(v) < amax) or v in found:
                        continue
                    if code(np.float32(np.float32(v - off) * idv)) != code(np.float32(np.float32(v - off) / d)):
                        found.append(v)
                        break
            pos = rng.choice(free, size=len(found), replace=False)
            blk[pos] = found
            planted += len(found)
    return x, planted


def q8_rule(x):
    """the reference's Q8_0 activation rule restated in numpy (per 32: d = amax / 127, id = 1 / d, q = rint(x * id) half to even), in f32."""
    xb = x.reshape(-1, 32).astype(np.float32)
    amax = np.abs(xb).max(axis=1)
    d = (amax / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore"):
        idv = np.where(d != 0, np.float32(1) / d, np.float32(0)).astype(np.float32)
    q = np.rint((xb * idv[:, None]).astype(np.float32).astype(np.float64)).astype(np.int64)
    return d.reshape(x.shape[:-1] + (-1,)), q.reshape(x.shape)


# ------------------------------------------------------------------------------------------------------------- weights
def weight_blocks(t, M, K, a, rng, codes=None, jitter=0):
    """raw reference-format blocks of type t, [M, row bytes], with d = 2^(a[m] + e) for a block of row m, m = mu * 2^(a[m] + e) (min types),
    e drawn per block from 0..jitter (so a kernel that reads another block's scale is off by a power of two).  Returns (raw uint8,
    w int64 [M, K] the integer each element is worth in units of 2^a[m]).  Codes are uniform over the whole code range (every nibble,
    every qh bit, Q8_0's -128) unless `codes` gives them."""
    bs = BLCK[t]
    nb = K // bs
    ts = TYPE_SIZE[t]
    raw = np.zeros((M, nb, ts), np.uint8)
    nbits = {Q4_0: 4, Q4_1: 4, Q4_2: 4, Q5_0: 5, Q5_1: 5, Q8_0: 8}[t]
    if codes is None:
        codes = rng.integers(0, 1 << nbits, (M, K))
    codes = np.asarray(codes, np.int64).reshape(M, nb, bs)
    mu = rng.integers(MU_RANGE[0], MU_RANGE[1] + 1, (M, nb)) if t in MIN_TYPES else np.zeros((M, nb), np.int64)
    a = np.asarray(a, np.int64)
    de = rng.integers(0, jitter + 1, (M, nb)) if jitter else np.zeros((M, nb), np.int64)
    ea = a[:, None] + de
    if t in F16_SCALE:
        assert ea.min() >= -24 and ea.max() <= 15
        raw[:, :, 0:2] = np.ldexp(np.ones((M, nb)), ea).astype(np.float16)[..., None].view(np.uint8)
    else:
        raw[:, :, 0:4] = np.ldexp(np.ones((M, nb), np.float32), ea).astype(np.float32)[..., None].view(np.uint8)
    mv = np.ldexp(mu.astype(np.float64), ea)
    if t == Q4_1:
        raw[:, :, 4:8] = mv.astype(np.float32)[..., None].view(np.uint8)
    if t == Q5_1:
        assert np.array_equal(mv.astype(np.float16).astype(np.float64), mv)
        raw[:, :, 2:4] = mv.astype(np.float16)[..., None].view(np.uint8)
    lo = codes & 15
    qs = (lo[..., 0::2] | (lo[..., 1::2] << 4)).astype(np.uint8) if nbits < 8 else None
    if t in (Q4_0, Q4_2):
        raw[..., ts - bs // 2:] = qs
        w = codes - 8
    elif t == Q4_1:
        raw[..., 8:] = qs
        w = codes + mu[..., None]
    elif t in (Q5_0, Q5_1):
        qh = ((codes >> 4) << np.arange(32)).sum(axis=-1).astype(np.uint32)
        o = 2 if t == Q5_0 else 4
        raw[..., o:o + 4] = qh[..., None].view(np.uint8).reshape(M, nb, 4)
        raw[..., o + 4:] = qs
        w = codes - 16 if t == Q5_0 else codes + mu[..., None]
    else:
        raw[..., 4:] = (codes - 128).astype(np.int8).view(np.uint8)
        w = codes - 128
    return raw.reshape(M, nb * ts), (w << de[..., None]).reshape(M, K)


def split3_kept(m):
    """what the min-piece forms keep of an f32 min m: split3 (csrc/common.h) restated -- three bf16 pieces taken by truncating the f32
    encoding to its high 16 bits.  Exact for every normal m of at most 24 significant bits; for an f32-SUBNORMAL m the bits below 2^-133
    (the low 16 bits of its encoding) are in no piece, so the kept value is m truncated toward zero to a multiple of 2^-133."""
    m = np.ascontiguousarray(m, np.float32)
    b0 = (m.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r1 = (m - b0).astype(np.float32)
    b1 = (r1.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    r2 = (r1 - b1).astype(np.float32)
    p2 = (r2.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
    return (b0.astype(np.float64) + b1 + p2)


def min_piece_ints(t, raw, K, a):
    """the integer each element of a Q4_1 / Q5_1 weight is worth, in units of 2^a[m], as the min-piece forms (GGML_HIP_PLAN_MIN_PIECES)
    compute it: d * code + split3_kept(m).  Equal to weight_blocks' w wherever split3 is exact."""
    assert t in MIN_TYPES
    b = np.asarray(raw, np.uint8).reshape(len(a), K // 32, TYPE_SIZE[t])
    if t == Q4_1:
        d = b[..., 0:4].copy().view(np.float32)[..., 0].astype(np.float64)
        m = b[..., 4:8].copy().view(np.float32)[..., 0]
    else:
        d = b[..., 0:2].copy().view(np.float16)[..., 0].astype(np.float64)
        m = b[..., 2:4].copy().view(np.float16)[..., 0].astype(np.float32)
    v = d[..., None] * decode_codes(t, raw, K).reshape(len(a), -1, 32) + split3_kept(m)[..., None]
    w = np.ldexp(v, -np.asarray(a, np.int64)[:, None, None])
    assert np.array_equal(w, np.round(w)), "not an integer in units of 2^a"
    return w.astype(np.int64).reshape(len(a), K)


def weight_tie_rows(t, K, a, rng):
    """f32 rows for the WEIGHT quantizer of type t whose d is exactly 2^a[r]: Q4_0 / Q4_2 max = -8 * 2^a, Q5_0 max = -16 * 2^a,
    Q4_1 (max - min) = 15 * 2^a, Q5_1 (max - min) = 31 * 2^a, Q8_0 / Q8_1 amax = 127 * 2^a.  Each block holds exact ties (n + 1/2)
    * 2^a of both parities; some blocks hold +A and -A in both orders (the first max-|x| wins: the sign of d follows it) and an
    element that reaches the clamp at 15 / 31."""
    bs = 16 if t == Q4_2 else 32
    R = len(a)
    x = np.zeros((R, K), np.float64)
    for r in range(R):
        for i in range(K // bs):
            blk = np.zeros(bs)
            style = (r + i) % 4
            if t in (Q4_0, Q4_2, Q5_0):
                A = 8 if t != Q5_0 else 16
                blk[:] = rng.integers(-A + 1, A, bs) + 0.5 * (rng.random(bs) < 0.5)
                blk = np.clip(blk, -A + 0.5, A - 0.5)
                p, p2 = rng.choice(bs, 2, replace=False)
                if style == 0:                   # -A first: d = 2^a; +A elsewhere reaches the clamp (q = 2A -> 2A - 1)
                    blk[min(p, p2)], blk[max(p, p2)] = -A, A
                elif style == 1:                 # +A first: d = -2^a, -A later is the clamped one
                    blk[min(p, p2)], blk[max(p, p2)] = A, -A
                else:
                    blk[p] = -A
            elif t in (Q4_1, Q5_1):
                L = 15 if t == Q4_1 else 31
                mu = int(rng.integers(-12, 4))
                blk[:] = mu + rng.integers(0, L, bs) + 0.5 * (rng.random(bs) < 0.5)
                p, p2 = rng.choice(bs, 2, replace=False)
                blk[p], blk[p2] = mu, mu + L
                blk = np.clip(blk, mu, mu + L)
            else:                                # Q8_0 / Q8_1: the activation rule
                blk[:] = rng.integers(-127, 127, bs) + 0.5
                p, p2 = rng.choice(bs, 2, replace=False)
                if style == 0:
                    blk[p], blk[p2] = 127, -127
                else:
                    blk[p] = -127 if style == 1 else 127
                    blk[p2] = 126.5 if style != 3 else -126.5
            x[r, i * bs:(i + 1) * bs] = blk
    xs = np.ldexp(x, np.asarray(a)[:, None]).astype(np.float32)
    assert np.array_equal(xs.astype(np.float64), np.ldexp(x, np.asarray(a)[:, None]))
    return xs


def expected_weight_quants(t, x, divide=False):
    """the weight quantizer's integer codes for rows x, restated in numpy (f32 arithmetic as the reference does it):
    Q4_0 / Q4_2 min(15, rint(x * id) + 8) with d = max / -8; Q5_0 min(31, (int)(x * id + 16.5f)) with d = max / -16;
    Q4_1 rint((x - min) * id) with d = (max - min) / 15; Q5_1 (uint)((x - min) * id + 0.5f) with d = (max - min) / 31;
    Q8_0 / Q8_1 rint(x * id).  Half to even for rint.  Returns (d f32 [rows, blocks], codes int64 [rows, K])."""
    bs = 16 if t == Q4_2 else 32
    xb = x.astype(np.float32).reshape(x.shape[0], -1, bs)
    if t in (Q4_0, Q4_2, Q5_0):
        first = np.argmax(np.abs(xb) == np.abs(xb).max(axis=-1, keepdims=True), axis=-1)     # the first max-|x| element
        mx = np.take_along_axis(xb, first[..., None], axis=-1)[..., 0]
        d = (mx / np.float32(-8 if t != Q5_0 else -16)).astype(np.float32)
    elif t in (Q4_1, Q5_1):
        mn, mx = xb.min(axis=-1), xb.max(axis=-1)
        d = ((mx - mn) / np.float32(15 if t == Q4_1 else 31)).astype(np.float32)
    else:
        d = (np.abs(xb).max(axis=-1) / np.float32(127)).astype(np.float32)
    with np.errstate(divide="ignore", invalid="ignore"):
        idv = np.where(d != 0, np.float32(1) / d, np.float32(0)).astype(np.float32)[..., None]
        if divide:                     # (a wrong kernel's x / d, for showing that near-ties separate the two)
            xb = np.where(d[..., None] != 0, (xb / d[..., None]).astype(np.float32), np.float32(0))
            if t in (Q4_1, Q5_1):
                xb = np.where(d[..., None] != 0, ((x.astype(np.float32).reshape(xb.shape) - mn[..., None]).astype(np.float32) / d[..., None]).astype(np.float32), 0)
                mn = np.zeros_like(mn)
            idv = np.ones_like(idv)
    if t in (Q4_0, Q4_2):
        c = np.minimum(15, np.rint((xb * idv).astype(np.float32).astype(np.float64)) + 8)
    elif t == Q5_0:
        c = np.minimum(31, np.trunc(((xb * idv).astype(np.float32) + np.float32(16.5)).astype(np.float32).astype(np.float64)))
    elif t == Q4_1:
        c = np.rint(((xb - mn[..., None]).astype(np.float32) * idv).astype(np.float32).astype(np.float64))
    elif t == Q5_1:
        c = np.trunc((((xb - mn[..., None]).astype(np.float32) * idv).astype(np.float32) + np.float32(0.5)).astype(np.float32).astype(np.float64))
    else:
        c = np.rint((xb * idv).astype(np.float32).astype(np.float64))
    return d, c.astype(np.int64).reshape(x.shape)


def decode_codes(t, raw, K):
    """the integer codes of raw blocks (no scale applied): the inverse of weight_blocks' packing, for checking a quantizer's output."""
    bs, ts = (16, 10) if t == Q4_2 else (32, {Q4_0: 20, Q4_1: 24, Q5_0: 22, Q5_1: 24, Q8_0: 36, Q8_1: 44}[t])
    b = np.asarray(raw, np.uint8).reshape(-1, K // bs, ts)
    if t in (Q8_0, Q8_1):                       # (Q8_1: d, s0, s1, then the quants)
        o = 4 if t == Q8_0 else 12
        return b[..., o:o + 32].view(np.int8).astype(np.int64).reshape(-1, K)
    qs = b[..., ts - bs // 2:]
    lo = np.stack([qs & 15, qs >> 4], axis=-1).reshape(b.shape[0], -1, bs).astype(np.int64)
    if t in (Q5_0, Q5_1):
        o = 2 if t == Q5_0 else 4
        qh = b[..., o:o + 4].copy().view(np.uint32)[..., 0]
        lo |= ((qh[..., None] >> np.arange(32, dtype=np.uint32)) & 1).astype(np.int64) << 4
    return lo.reshape(-1, K)


# ------------------------------------------------------------------------------------------------------------- products
def exact_product(w, a, q, b):
    """dst [N, M] = S * 2^(a[m] + b[n]) with S = sum_k w[m, k] * q[n, k], in float64 from the construction's integers alone.  The sums
    are below 2^53 (and below 2^24 where the product is meant to be exact in f32), so a float64 matmul is exact."""
    S = np.asarray(q, np.float64) @ np.asarray(w, np.float64).T
    return np.ldexp(S, (np.asarray(b)[:, None] + np.asarray(a)[None, :]).astype(np.int64))


def assert_exactly_representable(w, q, a=None, b=None):
    """per element: sum_k |w_k * q_k| < 2^24 units of the element's one term exponent (2^(a + b)) -- every association of the f32
    additions is then exact -- and the exact value is an f32 (a + b >= -149 and no overflow).  Asserted, not assumed."""
    T = np.abs(np.asarray(q, np.float64)) @ np.abs(np.asarray(w, np.float64)).T
    assert T.max(initial=0) < EXACT_BOUND, f"sum |terms| reaches {T.max():.0f} units (bound 2^24)"
    if a is not None:
        e = np.asarray(b)[:, None] + np.asarray(a)[None, :]
        assert e.min() >= -149, e.min()
        assert (np.ldexp(T, e) < np.float64(np.finfo(np.float32).max)).all()
    return T


def f32_bits(v):
    return np.ascontiguousarray(v, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------------------- the representative table
PERSIST, Q8K_FLAG, MIN_PIECES, WIDE = 4, 8, 32, 1
K3P = (5, 6)                 # K3p families (gemm_qmp.hip): the scale table is refilled inside the K loop beyond K = 20480
K3P_TABLE_K = 20480
BUDGET = 3 << 32             # M * K * N of a representative: the GPU tests' cost cap (K3p's in-loop table refill behind Q4_0 needs 1.2e10)
FORCES = (0, 1, 2, 3)
DENSE = (F32, F16)
TABLE_TYPES = LEGACY + DENSE
# Not in this tier (yet): the k-quant extension types.  They reach plan keys of their own (Q8K activations, two-scale forms); the coverage
# guard states them as excluded by name, so that every OTHER type's new form still cannot land without an exact case.
KQUANT_TYPES = (111, 112, 113, 114)      # Q3_K, Q4_K, Q5_K, Q6_K
GRID_K = (32, 64, 96, 160, 256, 288, 352, 512, 1024, 1056, 1536, 2048, 2080, 2336, 4096, 4160, 4352, 8192, 11008, 16384, 20480,
          20512, 22016)
GRID_N = (1, 2, 3, 4, 5, 7, 8, 9, 13, 16, 17, 31, 33, 63, 65, 100, 127, 129, 130, 255, 257, 300, 513, 1025)
GRID_M = (1, 17, 31, 33, 63, 65, 100, 129, 200, 257, 300, 513, 1000, 2049, 4096, 4097, 8193, 11008, 16385, 32001, 65537, 262144)


def plan_key(t, force, K, p):
    """what a representative must stand for: the kernel (family, form, image, flags that change the code path), K3p's in-loop table
    refill, and whether K leaves a partial last stage / range or pad blocks."""
    refill = p.family in K3P and K > K3P_TABLE_K
    if t in DENSE:
        partial = K % 32 != 0
    else:
        nbk = K // 32
        partial = bool(p.kunit > 0 and (nbk % p.kunit != 0 or (p.kstyle == 2 and nbk < p.kunit * p.ksplit)))
    return (t, force, p.family, p.form, p.image_kind, p.flags & (PERSIST | Q8K_FLAG | MIN_PIECES), refill, partial)


def sweep_keys(Ks, Ns, Ms, types=TABLE_TYPES, budget=None):
    """{key: (M, K, N) cheapest} over a grid (WIDE plans excluded: planes over 4 GiB cannot be a test case)"""
    import ctypes as C
    from ggmlsharp_amd import _lib
    L = _lib.lib()
    out = {}
    p = _lib.ggml_hip_mm_plan_t()
    try:
        for force in FORCES:
            L.ggml_hip_debug_force_gemm(force)
            for t in types:
                if t in DENSE and force:
                    continue
                for K in Ks:
                    if t in KQUANT_TYPES and K % 256:
                        continue                          # (a k-quant row is whole super-blocks)
                    for N in Ns:
                        for M in Ms:
                            cost = M * K * N
                            if budget is not None and cost > budget:
                                continue
                            assert L.ggml_hip_mm_plan(t, M, K, N, C.byref(p)) == 0, (t, M, K, N)
                            if p.flags & WIDE:
                                continue
                            key = plan_key(t, force, K, p)
                            rank = cost << 2 * ((M % p.tile_m == 0) + (N % p.tile_n == 0))   # a shape aligned to the tile counts 4x per axis
                            if key not in out or rank < out[key][0]:
                                out[key] = (rank, (M, K, N))
    finally:
        L.ggml_hip_debug_force_gemm(0)
    return {k: v[1] for k, v in out.items()}


def unreached(wide, table):
    """the keys of a sweep that a table has no case for"""
    return sorted(set(wide) - set(table))


def jitter_for(t, K):
    """1 (a per-block exponent of 0 or 1 on both operands) where the 2^24 bound leaves room for it at this K, else 0"""
    return int((K // 32) * 127 * 4 * wmax(t) < (1 << 23))


def representatives():
    """the GPU tests' table: the cheapest (M, K, N) per key within BUDGET, M and N ragged where the grid allows"""
    return sweep_keys(GRID_K, GRID_N, GRID_M, budget=BUDGET)
