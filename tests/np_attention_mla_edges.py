"""Sweeps, input generators, mutants and recorded model constants for tests/test_attention_mla_edges.py: the MLA kernels (csrc/mla.hip) at the step,
chunk and span edges, at explicit scales, under steep scores and at planted keys.  Pure numpy; the float64 REFERENCE, the float32 / float16 MODEL and
_steps are np_attention_mla's (imported, not edited), encode_rows, decode_rows, statistic and visible np_attention's.

A case is a Case tuple: form (SPLIT / WALK, as n_q files it), tier ('merged': a case of np_attention_mla's own sweep), generator, cache type, n_head, n_q, n_kv, the rows the cache holds (n_rows >= n_kv:
n_kv_max of the launch), causal, scale and slope.  The span is a parameter of every sweep (the test reads it from the plan); S = 128 span below.

  flat     flat_cases: np_attention_mla's own inputs (uniform in [-1, 1], its seeds, SCALE), causal on and off, both cache types, at
           n_kv in {63, 64, 65, 127, 191, 192, 193, S - 1, S, 2 S, 2 S + 1} x (n_q, n_head) in FLAT_SPLIT + FLAT_WALK, and n_kv = 8 S + 1 at
           FLAT_LONG.  Nothing is thinned.
  scale    scale_cases: flat inputs at SCALES[1:] = 0.135 and 0.03125, (n_q, n_head) in {(3, 16), (9, 16)}, n_kv in {129, 2 S + 37}, causal, both
           cache types; each against the reference AT THAT SCALE.  The same shapes at SCALES[0] = SCALE are cases of np_attention_mla's own sweep
           and keep its bar; scale_triples gives the three cases of a shape side by side.  The bar of a PAIR of scales is the larger of the two.
  steep    steep_cases: 'rising' / 'falling' -- a flat cache whose column 575 (a rope column, no part of V) holds j / 64 and flat queries whose
           column 575 holds +-slope * 64 / scale, so the score of position j carries +-slope * j; slopes 0.08 (the running maximum moves by 5 a
           step) and 0.3 (by 19 a step and by 0.3 S > 88 a span: past the largest argument of a float32 expf).  n_kv in {379, 2 S + 37},
           (n_q, n_head) in {(1, 16), (8, 3), (9, 16), (70, 1)}, causal, both cache types.
  planted  planted_pairs: a cache of +-0.125 entries (exact in both cache types), q[t, h] = beta * row[j*(t)]: key j* beats every other key of the
           cache by at least MARGIN = 30 in the score at SCALE (beta the smallest power of two that does it, from the largest correlation two
           rows of the generated cache have; chosen here, on the CPU).  'last': j* = vis(t) - 1, 'beyond': j* = vis(t), the first position the row
           must not see; the cache holds n_kv + 3 finite rows and n_kv_max = n_kv + 3, so the 'beyond' key of a row that sees all n_kv lies where
           the kernel must stage zeros.  Causal n_q = 8 and 9 (n_head = 5: rows of different tokens share a row half) at
           n_kv in {68, 132, S + 4, 2 S + 4}, causal (70, 1) at n_kv = 100 (the row halves of the first tile end at vis 62 and 94), all three not
           causal at n_kv in {64, 65, S, S + 1}; every shape in both cache types.  A 'last' row is V[j*] BIT FOR BIT in the model (statistic 0.0
           in every case): every other weight is below e^-30 < 2^-25, an f16 zero, and what the earlier steps and spans left is scaled by e^-30
           or less and vanishes in the sum.  'beyond' rows are held to the reference inside the planted bar.

Two more mutants (mutant_model), each the same result as the model until expf overflows -- a rescale against another maximum than the running /
global one:
  merge_first_max   SPLIT: the merge takes M = m_0, the first span's maximum, b_s = expf(m_s - m_0)
  walk_no_rescale   WALK: O and l are never multiplied by alpha -- every step's own (m, l, O) (np_attention_mla._steps over that step alone) is added
                    as it stands times expf(m_st - m_0), m_0 the first step's maximum.  (Leaving alpha out while the maximum still moves is a
                    different thing: it overweights the earlier steps by e^(rise of the maximum) and the flat sweep sees it at once.)
test_attention_mla_edges.py shows both INSIDE np_attention_mla's tolerances on its flat sweep, and non-finite on the steep tier.

The bar of a (form, tier) is 4 x the model's worst statistic max |model - ref| / max |V| on that tier's own sweep (np_attention_mla's rule and
factor).  Measured for the model at span = 4 (recorded rounded up):

    flat      SPLIT 1.71e-03 (1.8e-03; (1, 256) at n_kv = 193, Q8_0, causal)     WALK 1.97e-03 (2.0e-03; (129, 3) at n_kv = 127, Q8_0, causal)
    scale     SPLIT 1.76e-04 (1.8e-04; 0.135, (3, 16) at 129, Q8_0)               WALK 2.24e-04 (2.3e-04; 0.135, (9, 16) at 129, Q8_0)
    steep     SPLIT 1.64e-03 (1.7e-03; 'rising' 0.3, (8, 3) at 1061, Q8_0)        WALK 1.94e-03 (2.0e-03; 'falling' 0.3, (9, 16) at 379, Q8_0)
    planted   SPLIT 1.19e-04 (1.2e-04; 'beyond', (8, 5) at 68, F16)               WALK 1.70e-04 (1.7e-04; 'beyond', (70, 1) at 100, F16)

The bars: 7.2e-03 and 8.0e-03 (flat), 7.2e-04 and 9.2e-04 (scale), 6.8e-03 and 8.0e-03 (steep), 4.8e-04 and 6.8e-04 (planted).  Every one is
below 1e-2; no tier had to be shrunk.  beta = 16 gives a margin of 58.5.
test_the_edge_model_constants_are_what_the_model_measures recomputes every one on the CPU."""
import collections

import numpy as np

import np_attention as A
import np_attention_mla as M

F16, Q8_0 = A.F16, A.Q8_0
SPLIT, WALK = M.SPLIT, M.WALK
FORMS = (SPLIT, WALK)
D_K, D_V, CHUNK, STEP = M.D_K, M.D_V, M.CHUNK, M.STEP
KV_TYPES = (F16, Q8_0)
Case = collections.namedtuple("Case", "form tier gen kv_type n_head n_q n_kv n_rows causal scale slope")

TIERS = ("flat", "scale", "steep", "planted")
MODEL_WORST = {(SPLIT, "flat"): 1.8e-03, (WALK, "flat"): 2.0e-03,
               (SPLIT, "scale"): 1.8e-04, (WALK, "scale"): 2.3e-04,
               (SPLIT, "steep"): 1.7e-03, (WALK, "steep"): 2.0e-03,
               (SPLIT, "planted"): 1.2e-04, (WALK, "planted"): 1.7e-04}
MUTANTS = ("merge_first_max", "walk_no_rescale")
MUTANT_FORM = {"merge_first_max": SPLIT, "walk_no_rescale": WALK}


def tol(form, tier):
    return 4 * MODEL_WORST[(form, tier)]


def mk(tier, gen, kv_type, n_head, n_q, n_kv, n_rows=None, causal=True, scale=M.SCALE, slope=0.0):
    return Case(M.form_of(n_q), tier, gen, kv_type, n_head, n_q, n_kv, n_kv if n_rows is None else n_rows, causal, scale, slope)


def span_positions(span):
    return CHUNK * span


# ---- 1. the flat tier ----
FLAT_SPLIT = ((2, 5), (4, 20), (5, 13), (6, 1), (7, 64), (1, 256))   # (n_q, n_head): the n_q and head counts the merged sweep never runs
FLAT_WALK = ((13, 5), (65, 1), (129, 3), (10, 64))                   # 65 rows: a tile and one row, of many tokens and of one each; seven tiles; ten per token
FLAT_LONG = ((1, 16), (8, 2), (9, 2))                                # the shapes of the 8 S + 1 cache: nine spans for the merge


def flat_n_kvs(span):
    S = span_positions(span)
    return (63, 64, 65, 127, 191, 192, 193, S - 1, S, 2 * S, 2 * S + 1)


def flat_cases(span, shapes=None):
    S = span_positions(span)
    out = []
    for n_q, n_head in (FLAT_SPLIT + FLAT_WALK + FLAT_LONG if shapes is None else shapes):
        n_kvs = (8 * S + 1,) if (n_q, n_head) in FLAT_LONG else flat_n_kvs(span)
        out += [mk("flat", "flat", t, n_head, n_q, n_kv, causal=causal) for n_kv in n_kvs for t in KV_TYPES for causal in (True, False)]
    return out


# ---- 2. the scale tier ----
SCALES = (M.SCALE, 0.135, 0.03125)                                   # the sweep's, DeepSeek-V3's own (mscale^2 / sqrt(192)), a small power of two
SCALE_SHAPES = ((3, 16), (9, 16))


def scale_n_kvs(span):
    return (CHUNK + 1, 2 * span_positions(span) + 37)


def scale_triples(span):
    """the three cases of every (shape, n_kv, cache type), one per entry of SCALES; the first is a case of np_attention_mla's sweep"""
    return [tuple(mk("merged" if sc == M.SCALE else "scale", "flat", t, n_head, n_q, n_kv, scale=sc) for sc in SCALES)
            for n_q, n_head in SCALE_SHAPES for n_kv in scale_n_kvs(span) for t in KV_TYPES]


def scale_cases(span):
    return [c for tr in scale_triples(span) for c in tr[1:]]


def scale_bar(case):
    """the bar a case of a scale triple is held to: np_attention_mla's at SCALE, the scale tier's at the others"""
    return M.tol_of(case.n_q) if case.scale == M.SCALE else tol(case.form, "scale")


# ---- 3. the steep tier ----
SLOPES = (0.08, 0.3)
STEEP_GENS = ("rising", "falling")
STEEP_SHAPES = ((1, 16), (8, 3), (9, 16), (70, 1))
RAMP_COL = D_K - 1                                                   # column 575
RAMP_UNIT = 64.0                                                     # K_j[575] = j / 64: exact in f16 below 2048 positions
EXPF_MAX = 88.0                                                      # expf overflows in float32 above 88.72


def steep_n_kvs(span):
    return (379, 2 * span_positions(span) + 37)


def steep_cases(span):
    return [mk("steep", gen, t, n_head, n_q, n_kv, slope=slope)
            for gen in STEEP_GENS for slope in SLOPES for n_q, n_head in STEEP_SHAPES for n_kv in steep_n_kvs(span) for t in KV_TYPES]


# ---- 4. the planted tier ----
MARGIN = 30.0
PLANT_EXTRA = 3                                                      # finite rows the cache holds beyond n_kv
PLANT_SHAPES = ((8, 5), (9, 5), (70, 1))


def planted_shapes(span):
    """(n_q, n_head, n_kv, causal) of the planted tier: the vis of the rows of one call lie on both sides of a step, chunk or span edge"""
    S = span_positions(span)
    out = [(n_q, n_head, n_kv, True) for n_q, n_head in PLANT_SHAPES[:2] for n_kv in (68, 132, S + 4, 2 * S + 4)]
    out.append(PLANT_SHAPES[2] + (100, True))
    out += [(n_q, n_head, n_kv, False) for n_q, n_head in PLANT_SHAPES for n_kv in (64, 65, S, S + 1)]
    return out


def planted_pairs(span):
    """the ('last', 'beyond') pairs of cases: the plant on either side of the edge of what a row sees"""
    return [tuple(mk("planted", gen, t, n_head, n_q, n_kv, n_rows=n_kv + PLANT_EXTRA, causal=causal) for gen in ("last", "beyond"))
            for n_q, n_head, n_kv, causal in planted_shapes(span) for t in KV_TYPES]


def planted_cases(span):
    return [c for pair in planted_pairs(span) for c in pair]


def plant_position(case, t):
    """j*(t) of a planted case"""
    vis = A.visible(t, case.n_kv, case.n_q, case.causal)
    return vis - 1 if case.gen == "last" else vis


def tier_cases(form, tier, span):
    cs = {"flat": flat_cases, "scale": scale_cases, "steep": steep_cases, "planted": planted_cases}[tier](span)
    return [c for c in cs if c.form == form]


# ---- inputs, references and models, each computed once ----
_CACHE, _BETA, _IN, _REF, _MODEL = {}, {}, {}, {}, {}
_GEN_ROWS = 2304                                                     # rows a generated cache holds at least (a shorter cache is a prefix of a longer)


def _generated(kind, kv_type, n):
    """(raw, deq) of the first n rows of the ramp cache ('ramp': flat with column 575 = j / 64) or the planted cache ('plant': +-0.125)"""
    key = (kind, kv_type)
    if key not in _CACHE or _CACHE[key][0].shape[0] < n:
        rows = max(n, _GEN_ROWS)
        if kind == "ramp":
            x = np.random.default_rng([kv_type, D_K, 31]).uniform(-1, 1, (rows, D_K)).astype(np.float32)
            x[:, RAMP_COL] = np.arange(rows, dtype=np.float32) / np.float32(RAMP_UNIT)
        else:
            x = np.random.default_rng([D_K, 44]).choice(np.array([-0.125, 0.125], np.float32), (rows, D_K))      # (the same rows in both cache types)
        raw = A.encode_rows(kv_type, x)
        _CACHE[key] = (raw, A.decode_rows(kv_type, raw, D_K), x)
    raw, deq, _ = _CACHE[key]
    return raw[:n], deq[:n]


def generated_source(kind, kv_type, n):
    """the float32 rows a generated cache was encoded from"""
    _generated(kind, kv_type, n)
    return _CACHE[(kind, kv_type)][2][:n]


def plant_beta(span):
    """(beta, margin): the smallest power of two with SCALE * beta * (|row_j*|^2 - row_j . row_j*) >= MARGIN for every two rows j != j* of the largest
    planted cache (every other is a prefix of it), and the margin it gives"""
    n = max(c.n_rows for c in planted_cases(span))
    if n not in _BETA:
        rows = _generated("plant", F16, n)[1].astype(np.float64)
        g = rows @ rows.T
        own = np.diag(g).min()
        np.fill_diagonal(g, -np.inf)
        gap = own - g.max()
        beta = float(2.0 ** np.ceil(np.log2(MARGIN / (M.SCALE * gap))))
        _BETA[n] = (beta, M.SCALE * beta * gap)
    return _BETA[n]


def inputs(case, span=None):
    """(q f32 [n_q, n_head, 576], raw uint8 [n_rows, row bytes], deq f32 [n_rows, 576]) of a case; none of the arrays may be written to.  span: needed
    by the planted cases alone (beta is taken from the tier's largest cache)"""
    if case in _IN:
        return _IN[case]
    q = M.queries(case.n_head, case.n_q)
    if case.gen == "flat":
        raw, deq = M.cache_rows(case.kv_type, case.n_rows)
    elif case.gen in STEEP_GENS:
        raw, deq = _generated("ramp", case.kv_type, case.n_rows)
        q = q.copy()
        q[:, :, RAMP_COL] = np.float32((1.0 if case.gen == "rising" else -1.0) * case.slope * RAMP_UNIT / case.scale)
    else:
        raw, deq = _generated("plant", case.kv_type, case.n_rows)
        beta = np.float32(plant_beta(span)[0])
        q = np.zeros((case.n_q, case.n_head, D_K), np.float32)
        for t in range(case.n_q):
            q[t, :] = beta * deq[plant_position(case, t)]
    _IN[case] = (q, raw, deq)
    return _IN[case]


def values(case, span=None):
    """the V of a case's statistic: the dequantized columns 0 .. 511 of its n_kv positions"""
    return inputs(case, span)[2][:case.n_kv, :D_V]


def case_reference(case, span=None):
    if case not in _REF:
        q, _, deq = inputs(case, span)
        _REF[case] = M.reference(q, deq, case.n_kv, case.causal, case.scale)
    return _REF[case]


def case_model(case, span):
    """the numpy model's output on a case"""
    q, _, deq = inputs(case, span)
    return M.model(q, deq, case.n_kv, case.causal, case.scale, span)


def model_statistic(case, span):
    key = (case, span)
    if key not in _MODEL:
        _MODEL[key] = A.statistic(case_model(case, span), case_reference(case, span), values(case, span))
    return _MODEL[key]


def model_worst(form, tier, span):
    """the model's worst statistic over a tier's sweep"""
    return max(model_statistic(c, span) for c in tier_cases(form, tier, span))


# ---- the two mutants ----
def mutant_model(q, rows, n_kv, causal, scale, span, mutant):
    """np_attention_mla.model's arithmetic with one of MUTANTS in place of the merge (SPLIT) or of the walk's rescale (WALK) -> f32 [n_q, n_head, 512]"""
    n_q, n_head, _ = q.shape
    assert M.form_of(n_q) == MUTANT_FORM[mutant]
    R = n_q * n_head
    out = np.zeros((R, D_V), np.float32)
    vis = M._vis(n_q, n_head, n_kv, causal)
    n_steps = (int(vis.max()) + STEP - 1) // STEP if n_kv else 0
    if n_steps == 0:
        return out.reshape(n_q, n_head, D_V)
    sc = np.float32(scale)
    qh, Kh = M._h(q.reshape(R, D_K)), M._h(rows[:n_kv])
    Vh = Kh[:, :D_V]
    per = span * (CHUNK // STEP) if mutant == "merge_first_max" else 1
    parts = [M._steps(qh, Kh, Vh, vis, s0, min(s0 + per, n_steps), sc, n_kv) for s0 in range(0, n_steps, per)]
    m0 = parts[0][0]                                                 # (finite for every row with a visible position: position 0 is one)
    L, Acc = np.zeros(R, np.float32), np.zeros((R, D_V), np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        for m, l, O in parts:
            b = np.where(m == -np.inf, np.float32(0), np.exp((m - m0).astype(np.float32))).astype(np.float32)
            L = (L + l * b).astype(np.float32)
            Acc = (Acc + O * b[:, None]).astype(np.float32)
        live = vis > 0
        out[live] = Acc[live] / L[live, None]
    return out.reshape(n_q, n_head, D_V)


def mutant_statistic(got, ref, V):
    """np_attention.statistic, infinite where the output is not finite"""
    return A.statistic(got, ref, V) if np.isfinite(got).all() else float("inf")
