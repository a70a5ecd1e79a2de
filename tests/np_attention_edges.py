"""Sweeps, input generators and recorded model constants for tests/test_attention_edges.py: the attention kernels (csrc/attn.hip) at every group
size, at explicit scales, over long caches, under peaked scores and at planted mask edges.  Pure numpy; the float64 REFERENCE and the float32 /
float16 MODELS are np_attention's and np_attention_ex's (imported, not edited), and so are encode_rows, decode_rows, statistic and visible.

A case is a Case tuple: the form ('decode' / 'prompt'), the generator of its inputs, the shape, the cache's rows (n_rows >= n_kv: the launch is
sized by n_rows), causal, scale (None: 1 / sqrt(D)), window and softcap.  Four tiers; the first two run the same inputs and share one regime and
one bar, the other two have their own:

  flat     shape_cases(form): np_attention.inputs' own distribution (uniform in [-1, 1], seeded by the shape) at the group sizes, pass counts,
           chunk counts and tile edges np_attention.cases never reaches.
  scale    scale_cases(form): flat inputs at scale None / 0.25 / 0.03125, and at the two explicit scales under a soft-cap of 0.5 (sc' = scale / cap).
           The PROMPT shapes are those with n_q >= n_kv: only rows that see a few positions move by 100 bars when the scale of a flat softmax moves.
  peaked   peaked_cases(form): 'peaked' is the flat inputs with q multiplied by 3 SIGMA, which gives scale * q . k a standard deviation of SIGMA = 4
           (the value used; the PROMPT bar it gives is below 1e-2); 'rising' adds SLOPE * j to the score of position j (q in [0, 2], every element
           of K_j shifted by SLOPE * j / sqrt(D): np_attention_ex's ALPHA shift, linear instead of logarithmic), so every chunk raises the running
           maximum by 128 SLOPE = 10.2; 'falling' subtracts it, so the maximum sits in chunk 0, f16(p) underflows from chunk 2 on and the float32
           weights of the last chunk of 1100 reach e^-88, the subnormals.  SLOPE = 0.08 (0.1 put the PROMPT bar above 1e-2: the f16 operands of
           that form carry the shift of 64 at position 641 with an absolute error that grows with it).
  planted  planted_cases(form): K of +-0.125 entries, q[t, h] = beta * deq(K)[j*(t), h / G]: key j* beats every other key of the cache by at least
           MARGIN = 30 in the score (beta: the smallest power of two that does it, from the largest correlation between two keys of a kv head --
           chosen here, on the CPU), so a row that sees j* returns V[j*] to n_kv e^-30.  'last': j* = vis(t) - 1; 'beyond': j* = vis(t), the first
           invisible position (the cache holds n_kv + 3 rows); 'wlo': j* = lo_t, the first position inside the window; 'wbehind': j* = lo_t - 1.
           A row that has no such position gets q = 0.  The first D / 2 entries of K_j are one pattern per kv head times (-1)^j, the rest is random:
           neighbours are anti-correlated (-1/2) and keys two apart correlated (+1/2), so the row whose plant went out of sight never picks the
           position the plant stood on before as the best of the rest -- with wholly random keys one row in W = 5 did, and its two references
           then agree (the 100-bar test found it).

THINNED, by name (the CPU half recomputes every model constant and must stay inside about a minute): the PROMPT cases of the peaked tier and both
forms of the planted tier run TWO of the four (D, cache type) pairs per shape, rotating through DT so that every pair is run; the scale tier runs
the pair its SCALE_SHAPES entry names.  The flat tier runs all four everywhere, and the lists of G, R, n_q and n_kv are whole in every tier.

The bar of a (form, tier) is 4 x the model's worst statistic max |model - ref| / max |V| on that tier's own sweep (np_attention's rule and factor);
where a flat constant does not exceed np_attention's, np_attention's TOL stands.  Measured for the model (recorded rounded up):

    flat + scale   DECODE 1.31e-07 (1.4e-07; n_kv = 5 < n_q = 8)         PROMPT 4.59e-04 (4.7e-04; n_q = n_kv = 257 at scale 0.25)
    peaked         DECODE 3.34e-06 (3.4e-06; 'rising' at 1100)           PROMPT 1.79e-03 (1.8e-03; 'peaked' at (257, 641))
    planted        DECODE 1.03e-06 (1.1e-06; 'beyond' at n_kv = 129)     PROMPT 2.50e-04 (2.6e-04; 'wbehind', W = 128)

Both flat constants exceed np_attention's (1.2e-07, 3.7e-04), so the flat bars are 4 x these: 5.6e-07 and 1.88e-03.  The others: 1.36e-05 and
7.2e-03 (peaked), 4.4e-06 and 1.04e-03 (planted).  deq(K) of a planted cache is +-0.125 exactly in both cache types and beta a power of two, so
every planted score is exact in float32 and in float16: what the planted bars measure is the softmax and the V sum, not the dot product.

test_the_edge_model_constants_are_what_the_model_measures recomputes every one on the CPU."""
import collections

import numpy as np

import np_attention as A
import np_attention_ex as X

F16, Q8_0, CHUNK = A.F16, A.Q8_0, A.CHUNK
Case = collections.namedtuple("Case", "form gen D n_head n_head_kv kv_type n_q n_kv n_rows causal scale window softcap")

MODEL_WORST = {("decode", "flat"): 1.4e-07, ("prompt", "flat"): 4.7e-04,
               ("decode", "peaked"): 3.4e-06, ("prompt", "peaked"): 1.8e-03,
               ("decode", "planted"): 1.1e-06, ("prompt", "planted"): 2.6e-04}
_BASE = {"decode": (A.MODEL_WORST_DECODE, A.TOL_DECODE), "prompt": (A.MODEL_WORST_PROMPT, A.TOL_PROMPT)}


def tol(form, tier):
    rec = MODEL_WORST[(form, tier)]
    return _BASE[form][1] if tier == "flat" and rec <= _BASE[form][0] else 4 * rec


TIERS = ("flat", "peaked", "planted")
TIER_OF = {"flat": "flat", "peaked": "peaked", "rising": "peaked", "falling": "peaked", "last": "planted", "beyond": "planted", "wlo": "planted",
           "wbehind": "planted"}
DT = ((64, F16), (128, Q8_0), (128, F16), (64, Q8_0))               # the (D, cache type) pairs, in the order the thinned sweeps rotate through


def mk(form, gen, D, n_head, n_head_kv, kv_type, n_q, n_kv, n_rows=None, causal=True, scale=None, window=0, softcap=0.0):
    return Case(form, gen, D, n_head, n_head_kv, kv_type, n_q, n_kv, n_kv if n_rows is None else n_rows, causal, scale, window, softcap)


def scale_of(case):
    return 1.0 / float(np.sqrt(np.float64(case.D))) if case.scale is None else case.scale


# ---- 1. the shape tier ----
DECODE_HEADS = ((3, 1, 3), (12, 3, 5), (5, 1, 7), (14, 2, 4), (12, 1, 8), (16, 1, 8), (16, 1, 1), (6, 6, 6), (2, 2, 8),
                (4, 2, 2))                                           # (n_head, n_head_kv, n_q); the last is added here: no other case has n_q = 2
DECODE_N_KV = (127, 128, 641, 1100)                                  # 641: six chunks, the last holding one position; 1100: nine
DECODE_SHORT = (5, 1, 8, 5)                                          # n_kv = 5 < n_q = 8: rows 0 .. 2 see nothing
PROMPT_SHAPES = ((32, 32), (33, 160), (127, 128), (128, 128), (128, 255), (129, 429), (257, 257), (257, 641), (40, 17))      # (n_q, n_kv)
PROMPT_HEADS = ((3, 1), (12, 3), (16, 1), (5, 5))
SLACK = 300                                                          # n_rows - n_kv of the cases that read n_kv on the device


def shape_cases(form):
    out = []
    if form == "decode":
        for nh, nhk, n_q in DECODE_HEADS:
            for n_kv in DECODE_N_KV:
                for D, t in DT:
                    causal = not (n_kv == 128 and (D, t) == DT[1])                      # one case per head tuple is not causal
                    n_rows = n_kv + SLACK if (n_kv == 641 and (D, t) == DT[2]) else n_kv      # one reads n_kv on the device, n_kv_max > n_kv
                    out.append(mk(form, "flat", D, nh, nhk, t, n_q, n_kv, n_rows, causal))
        nh, nhk, n_q, n_kv = DECODE_SHORT
        out += [mk(form, "flat", D, nh, nhk, t, n_q, n_kv) for D, t in DT]
        return out
    for nh, nhk in PROMPT_HEADS:
        for n_q, n_kv in PROMPT_SHAPES:
            for D, t in DT:
                causal = not ((n_q, n_kv) == (33, 160) and (D, t) == DT[1])
                n_rows = n_kv + SLACK if ((n_q, n_kv) == (32, 32) and (D, t) == DT[2]) or (n_q, n_kv) == (127, 128) else n_kv
                out.append(mk(form, "flat", D, nh, nhk, t, n_q, n_kv, n_rows, causal))
    return out


# ---- 2. the scale tier ----
SCALES = (None, 0.25, 0.03125)
SCALE_SOFTCAP = 0.5
SCALE_SHAPES = {"decode": ((64, 5, 1, F16, 7, 641), (128, 5, 1, Q8_0, 7, 641),          # R = 35: four full passes and a ragged one, per cache type
                           (128, 16, 1, F16, 8, 1100), (64, 16, 1, Q8_0, 8, 1100), (128, 3, 1, F16, 3, 127), (64, 12, 3, Q8_0, 5, 128)),
                "prompt": ((64, 3, 1, F16, 257, 257), (128, 3, 1, Q8_0, 257, 257),      # three workgroups, per cache type
                           (128, 12, 3, F16, 40, 17), (64, 12, 3, Q8_0, 40, 17), (64, 5, 5, Q8_0, 128, 128))}


def scale_cases(form):
    """(shape, softcap) -> the cases at the scales it runs: all three without a cap, the two explicit ones under SCALE_SOFTCAP"""
    out = {}
    for s in SCALE_SHAPES[form]:
        out[(s, 0.0)] = [mk(form, "flat", *s, scale=sc) for sc in SCALES]
        out[(s, SCALE_SOFTCAP)] = [mk(form, "flat", *s, scale=sc, softcap=SCALE_SOFTCAP) for sc in SCALES[1:]]
    return out


# ---- 3. the peaked tier ----
SIGMA = 4.0
SLOPE = 0.08
PEAKED_GENS = ("peaked", "rising", "falling")
PEAKED_DECODE = ((5, 1, 7), (12, 3, 5))
PEAKED_PROMPT_HEADS = ((5, 1), (12, 3))
PEAKED_N_KV = (641, 1100)
PEAKED_PROMPT_SHAPES = ((129, 429), (257, 641))


def peaked_cases(form):
    out = []
    for gi, gen in enumerate(PEAKED_GENS):
        if form == "decode":
            out += [mk(form, gen, D, nh, nhk, t, n_q, n_kv) for nh, nhk, n_q in PEAKED_DECODE for n_kv in PEAKED_N_KV for D, t in DT]
        else:
            for hi, (nh, nhk) in enumerate(PEAKED_PROMPT_HEADS):
                for si, (n_q, n_kv) in enumerate(PEAKED_PROMPT_SHAPES):
                    i = gi + hi + si                                                    # thinned: two pairs per (generator, heads, shape)
                    out += [mk(form, gen, D, nh, nhk, t, n_q, n_kv) for D, t in (DT[i % 4], DT[(i + 2) % 4])]
    return out


# ---- 4. the planted tier ----
MARGIN = 30.0
PLANT_WINDOWS = (5, 128, 200)
PLANT_EXTRA = 3                                                      # rows the cache holds beyond n_kv: the 'beyond' plant of the last row lies there
PLANT_DECODE = ((5, 1, 7), (16, 1, 8))
PLANT_DECODE_N_KV = (128, 129, 641)
PLANT_PROMPT_SHAPES = ((33, 160), (128, 255), (129, 429), (257, 641))
PLANT_PROMPT_HEADS = (3, 1)


def planted_shapes(form):
    """(D, n_head, n_head_kv, kv_type, n_q, n_kv) of the planted tier; thinned: two (D, cache type) pairs per shape"""
    out, i = [], 0
    if form == "decode":
        for nh, nhk, n_q in PLANT_DECODE:
            for n_kv in PLANT_DECODE_N_KV:
                out += [(D, nh, nhk, t, n_q, n_kv) for D, t in (DT[i % 4], DT[(i + 1) % 4])]
                i += 1
        return out
    nh, nhk = PLANT_PROMPT_HEADS
    for n_q, n_kv in PLANT_PROMPT_SHAPES:
        out += [(D, nh, nhk, t, n_q, n_kv) for D, t in (DT[i % 4], DT[(i + 1) % 4])]
        i += 1
    return out


def planted_pairs(form, shape):
    """the (seen, unseen) pairs of cases of a shape: the plant on either side of the causal edge, and of the window's edge for every W"""
    n_rows = shape[5] + PLANT_EXTRA
    return [(mk(form, "last", *shape, n_rows=n_rows), mk(form, "beyond", *shape, n_rows=n_rows))] + \
           [(mk(form, "wlo", *shape, n_rows=n_rows, window=W), mk(form, "wbehind", *shape, n_rows=n_rows, window=W)) for W in PLANT_WINDOWS]


def planted_cases(form):
    return [c for s in planted_shapes(form) for pair in planted_pairs(form, s) for c in pair]


def plant_position(case, t):
    """j*(t) of a planted case, or None where the row has no such position"""
    hi = A.visible(t, case.n_kv, case.n_q, case.causal)
    lo = X.window_lo(hi, case.window)
    j = {"last": hi - 1, "beyond": hi, "wlo": lo, "wbehind": lo - 1}[case.gen]
    return j if hi >= 1 and 0 <= j < case.n_rows else None


def tier_cases(form, tier):
    if tier == "flat":                                               # (the scale tier runs flat inputs: one regime, one bar)
        return list(dict.fromkeys(shape_cases(form) + [c for cs in scale_cases(form).values() for c in cs]))       # (some default-scale cases are in both)
    return peaked_cases(form) if tier == "peaked" else planted_cases(form)


# ---- inputs, references and models, each computed once ----
_IN, _BETA, _REF, _MODEL = {}, {}, {}, {}


def _shape(case):
    return (case.D, case.n_head, case.n_head_kv, case.kv_type, case.n_q, case.n_rows)


def input_key(case):
    """what the inputs of a case depend on; the cache's bytes depend on its first two fields alone"""
    kv = ("flat" if case.gen == "peaked" else "plant" if TIER_OF[case.gen] == "planted" else case.gen,) + _shape(case)
    return (kv, (case.gen, case.n_kv, case.causal, case.window) if TIER_OF[case.gen] == "planted" else case.gen)


def _encode(kv_type, D, q, K, V):
    Kraw, Vraw = A.encode_rows(kv_type, K.astype(np.float32)), A.encode_rows(kv_type, V.astype(np.float32))
    return (q.astype(np.float32), Kraw, Vraw, A.decode_rows(kv_type, Kraw, D), A.decode_rows(kv_type, Vraw, D))


def plant_beta(case):
    """the smallest power of two beta with scale * beta * (|K_j*|^2 - K_j . K_j*) >= MARGIN for every two keys j != j* of a kv head"""
    key = input_key(case)[0]
    if key not in _BETA:
        Kd = _plant_kv(case)[3].astype(np.float64)
        own, other = np.inf, -np.inf
        for hk in range(case.n_head_kv):
            g = Kd[:, hk] @ Kd[:, hk].T
            own = min(own, np.diag(g).min())
            np.fill_diagonal(g, -np.inf)
            other = max(other, g.max())
        _BETA[key] = float(2.0 ** np.ceil(np.log2(MARGIN / (scale_of(case) * (own - other)))))
    return _BETA[key]


def _plant_kv(case):
    key = input_key(case)[0]
    if key not in _IN:
        D, nh, nhk, t, n_q, n_rows = _shape(case)
        rng = np.random.default_rng([40, D, nh, nhk, t, n_q, n_rows])
        K = rng.choice(np.array([-0.125, 0.125]), (n_rows, nhk, D))
        K[:, :, :D // 2] = K[:1, :, :D // 2] * np.where(np.arange(n_rows) % 2, -1.0, 1.0)[:, None, None]      # the parity half (the docstring)
        V = rng.uniform(-1, 1, (n_rows, nhk, D))
        _IN[key] = _encode(t, D, np.zeros((n_q, nh, D)), K, V)
    return _IN[key]


def inputs(case):
    """(q, Kraw, Vraw, Kd, Vd) of a case: the cache holds n_rows rows; none of the arrays may be written to"""
    key = input_key(case)
    if key in _IN:
        return _IN[key]
    D, nh, nhk, t, n_q, n_rows = _shape(case)
    G = nh // nhk
    if case.gen in ("flat", "peaked"):
        q, Kraw, Vraw, Kd, Vd = A.inputs(_shape(case))
        if case.gen == "peaked":
            q = (q * np.float32(3.0 * SIGMA)).astype(np.float32)
        _IN[key] = (q, Kraw, Vraw, Kd, Vd)
    elif case.gen in ("rising", "falling"):
        rng = np.random.default_rng([41, case.gen == "rising", D, nh, nhk, t, n_q, n_rows])
        q = rng.uniform(-1, 1, (n_q, nh, D)) + 1.0
        ramp = SLOPE * np.arange(n_rows)[:, None, None] / np.sqrt(D)
        K = rng.uniform(-1, 1, (n_rows, nhk, D)) + (ramp if case.gen == "rising" else -ramp)
        _IN[key] = _encode(t, D, q, K, rng.uniform(-1, 1, (n_rows, nhk, D)))
    else:
        _, Kraw, Vraw, Kd, Vd = _plant_kv(case)
        beta = np.float32(plant_beta(case))
        q = np.zeros((n_q, nh, D), np.float32)
        for tq in range(n_q):
            j = plant_position(case, tq)
            if j is not None:
                q[tq] = beta * Kd[j, np.arange(nh) // G]
        _IN[key] = (q, Kraw, Vraw, Kd, Vd)
    return _IN[key]


def case_reference(case):
    if case not in _REF:
        q, _, _, Kd, Vd = inputs(case)
        _REF[case] = X.reference(q, Kd, Vd, case.n_kv, case.causal, scale_of(case), case.window, case.softcap)
    return _REF[case]


def model_statistic(case):
    """the statistic of the form's numpy model on a case"""
    if case not in _MODEL:
        q, _, _, Kd, Vd = inputs(case)
        fn = X.model_decode if case.form == "decode" else X.model_prompt
        _MODEL[case] = A.statistic(fn(q, Kd, Vd, case.n_kv, case.causal, scale_of(case), case.window, case.softcap), case_reference(case), Vd)
    return _MODEL[case]


def model_worst(form, tier):
    """the model's worst statistic over a tier's sweep"""
    return max(model_statistic(c) for c in tier_cases(form, tier))
