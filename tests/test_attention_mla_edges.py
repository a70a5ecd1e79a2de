"""The MLA kernels where tests/test_attention_mla.py does not go (csrc/mla.hip: the step body, the SPLIT partials and their merge, the WALK, their
paged twins): n_kv and vis on both sides of every step (64), chunk (128) and span (128 span) edge, every n_q of the SPLIT form, WALK calls of a tile
and one row and of seven tiles, 5 .. 256 heads, a cache of nine spans, explicit scales, scores that rise or fall by more than expf can carry across
a span, and single planted keys that pin WHICH position a row sees.

Yardsticks (tests/np_attention_mla_edges.py): always the float64 reference over the DEQUANTIZED cache; the statistic max |dst - ref| / max |V|;
the bar of a (form, tier) is 4 x what the numpy model measures on that tier's own sweep, recomputed on the CPU here.  Conditions on the INPUTS,
checked on the CPU: the references of a case at any two scales lie at least 100 bars apart; moving a planted key across the edge of what a row sees
moves EVERY row by at least 100 bars; a 'last' row is V[j*] bit for bit in the model; the two rescale mutants ("merge_first_max",
"walk_no_rescale") are INSIDE np_attention_mla's tolerances on its own flat sweep -- the gap -- and non-finite on the steep tier.
Bit contracts on the device: a planted 'last' row is the staged V row; 33 paged decode sequences of ragged lengths over a shuffled table are the
contiguous calls; rows of equal vis agree between n_q = 1, 2, 5, 8 and between 9 and 129, head h of 256 is the row alone; the SPLIT result does not
depend on what the work buffer held (0x7F bytes: m = 3.4e38; 0xFF bytes: NaN; the partials of a longer call).  The span is read from the plan."""
import itertools

import numpy as np
import pytest

import np_attention as A
import np_attention_mla as M
import np_attention_mla_edges as E
import test_attention_mla as T                                       # _plan, span, Pool, paged, contiguous_cache

F16, Q8_0 = A.F16, A.Q8_0
SPLIT, WALK = M.SPLIT, M.WALK
DK, DV = M.D_K, M.D_V
PAGE = M.CHUNK


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _vis_of(case):
    return {A.visible(t, case.n_kv, case.n_q, case.causal) for t in range(case.n_q)}


# ---------------------------------------------------------------- CPU
def test_the_sweeps_hold_every_row_count_head_count_and_edge_by_name():
    span = T.span()
    S = PAGE * span
    flat = E.flat_cases(span)
    every = flat + E.scale_cases(span) + E.steep_cases(span) + E.planted_cases(span)
    assert len(set(every)) == len(every)
    assert {c.n_q for c in every} >= set(range(1, 11)) | {13, 65, 70, 129}
    assert {c.n_head for c in flat} >= {1, 2, 3, 5, 13, 16, 20, 64, 256}
    # the flat tier: every listed (n_q, n_head) at every listed n_kv, both cache types, causal on and off; the nine-span cache at its three shapes
    have = {(c.n_q, c.n_head, c.n_kv, c.kv_type, c.causal) for c in flat}
    for shape in ((2, 5), (4, 20), (5, 13), (6, 1), (7, 64), (1, 256), (13, 5), (65, 1), (129, 3), (10, 64)):
        for n_kv in (63, 64, 65, 127, 191, 192, 193, S - 1, S, 2 * S, 2 * S + 1):
            for t, causal in itertools.product((F16, Q8_0), (True, False)):
                assert shape + (n_kv, t, causal) in have, (shape, n_kv, t, causal)
    for shape in ((1, 16), (8, 2), (9, 2)):
        for t, causal in itertools.product((F16, Q8_0), (True, False)):
            assert shape + (8 * S + 1, t, causal) in have
    assert max(c.n_kv for c in every) == 8 * S + 1 and all(c.n_head <= 16 for c in every if c.n_kv > 2 * S + 37)
    for form in E.FORMS:                                             # every edge value is the vis of some row of each form
        vis = set().union(*(_vis_of(c) for c in flat if c.form == form))
        assert vis >= {63, 64, 65, 127, 191, 192, 193, S - 1, S, 2 * S, 2 * S + 1, 8 * S + 1}, form
    # the scale tier
    for tr in E.scale_triples(span):
        assert [c.scale for c in tr] == [0.5, 0.135, 0.03125] and len({c[3:9] for c in tr}) == 1
        assert (tr[0].kv_type, tr[0].n_head, tr[0].n_q, tr[0].n_kv, True) in M.cases(tr[0].form, span, (16,))      # the first IS a case of the merged sweep
    assert {(c.n_q, c.n_head, c.n_kv, c.kv_type) for c in E.scale_cases(span)} == set(itertools.product((3, 9), (16,), (129, 2 * S + 37), (F16, Q8_0)))
    # the steep tier
    assert {(c.gen, c.slope, c.n_q, c.n_head, c.n_kv, c.kv_type) for c in E.steep_cases(span)} == \
        {(g, s) + sh + (n, t) for g in ("rising", "falling") for s in (0.08, 0.3) for sh in ((1, 16), (8, 3), (9, 16), (70, 1)) for n in (379, 2 * S + 37)
         for t in (F16, Q8_0)}
    assert all(c.causal for c in E.steep_cases(span))
    # the planted tier: the vis of the rows of one call on both sides of every edge
    pl = E.planted_cases(span)
    for n_q in (8, 9):
        for edge in (64, 128, S, 2 * S):
            for t in (F16, Q8_0):
                got = [c for c in pl if (c.n_q, c.n_kv, c.kv_type, c.causal) == (n_q, edge + 4, t, True)]
                assert {c.gen for c in got} == {"last", "beyond"} and all(_vis_of(c) >= set(range(edge - 3, edge + 5)) for c in got), (n_q, edge, t)
    for n_q in (8, 9, 70):
        for n_kv in (64, 65, S, S + 1):
            assert {(c.gen, c.kv_type) for c in pl if (c.n_q, c.n_kv, c.causal) == (n_q, n_kv, False)} == set(itertools.product(("last", "beyond"), (F16, Q8_0)))
    c70 = [c for c in pl if c.n_q == 70 and c.causal]
    assert {(c.n_head, c.n_kv) for c in c70} == {(1, 100)} and len(c70) == 4
    assert [A.visible(t, 100, 70, True) for t in (31, 63)] == [62, 94]                        # the largest vis of the two row halves of tile 0
    assert all(c.n_rows == c.n_kv + 3 for c in pl)
    # the plan files every case under the form it is listed as
    for c in every:
        rc, p = T._plan(c.kv_type, c.n_head, c.n_q, c.n_rows)
        assert rc == 0 and p.form == c.form == M.form_of(c.n_q) and p.span == span, c
    for form in E.FORMS:
        for tier in E.TIERS:
            assert E.tier_cases(form, tier, span)


@pytest.mark.parametrize("tier", E.TIERS)
@pytest.mark.parametrize("form", E.FORMS)
def test_the_edge_model_constants_are_what_the_model_measures(form, tier):
    span = T.span()
    rec = E.MODEL_WORST[(form, tier)]
    worst = E.model_worst(form, tier, span)
    print("form", form, tier, "model worst", worst, "recorded", rec, "bar", E.tol(form, tier))
    assert rec / 1.25 <= worst <= rec, (form, tier, worst, rec)
    assert E.tol(form, tier) == 4 * rec and E.tol(form, tier) < 1e-2


@pytest.mark.parametrize("form", E.FORMS)
def test_the_references_of_a_case_at_any_two_scales_are_100_bars_apart(form):
    """a condition on the INPUTS: a kernel or launcher that ignores `scale`, or applies another, cannot pass (the bar of a pair: the larger of the two)"""
    span = T.span()
    least = np.inf
    for tr in E.scale_triples(span):
        if tr[0].form != form:
            continue
        for a, b in itertools.combinations(tr, 2):
            bar = max(E.scale_bar(a), E.scale_bar(b))
            d = A.statistic(E.case_reference(a), E.case_reference(b), E.values(a))
            least = min(least, d / bar)
            assert d >= 100 * bar, (a, b.scale, d, 100 * bar)
    print("form", form, "smallest distance between two scales, in bars", least)
    assert least < np.inf


def test_the_generators_do_what_they_say():
    span = T.span()
    S = PAGE * span
    # steep: the ramp column is exact as staged below 2048 positions (Q8_0: from position 64 on), the score of position j carries +-slope j, and the maximum of a span
    # moves by more than expf can carry at the larger slope
    assert max(E.SLOPES) * S > E.EXPF_MAX
    for c in E.steep_cases(span):
        q, raw, deq = E.inputs(c)
        n, lo = min(c.n_kv, 2048), 0 if c.kv_type == F16 else 64     # (a Q8_0 block takes its scale from the ramp once j / 64 >= 1: exact from there on)
        assert np.array_equal(M._h(deq[lo:n, E.RAMP_COL]), (np.arange(lo, n) / 64.0).astype(np.float32)), c
        assert np.abs(deq[:lo, E.RAMP_COL] - np.arange(lo) / 64.0).max(initial=0.0) <= 0.5 / 127
        sign = 1.0 if c.gen == "rising" else -1.0
        assert (q[:, :, E.RAMP_COL] == np.float32(sign * c.slope * 64.0 / c.scale)).all() and np.array_equal(q[:, :, :E.RAMP_COL], M.queries(c.n_head, c.n_q)[:, :, :E.RAMP_COL])
        assert np.abs(deq[:, :DV]).max() <= 1.0 and np.isfinite(deq).all()
        if c.n_kv > S and c.slope == max(E.SLOPES):
            s = (np.float32(c.scale) * (deq[:c.n_kv].astype(np.float64) @ q[-1, 0].astype(np.float64)))        # the last row sees every position
            m = np.array([s[j:j + S].max() for j in range(0, c.n_kv, S)])
            assert (sign * np.diff(m[:2]) > E.EXPF_MAX).all(), (c, m)
    # planted: +-0.125 survives both cache types, beta is a power of two, every score is exact and the margin is what the cache really gives
    beta, margin = E.plant_beta(span)
    assert margin >= E.MARGIN and np.log2(beta) == int(np.log2(beta)) and beta <= 64
    print("beta", beta, "margin", margin)
    for c in E.planted_cases(span):
        q, raw, deq = E.inputs(c, span)
        x = E.generated_source("plant", c.kv_type, c.n_rows)
        assert np.array_equal(A.decode_rows(c.kv_type, A.encode_rows(c.kv_type, x), DK), x) and np.array_equal(deq, x) and (np.abs(x) == 0.125).all(), c
        assert deq.shape[0] == c.n_kv + E.PLANT_EXTRA
        s = np.float32(c.scale) * (q[:, 0].astype(np.float64) @ deq.astype(np.float64).T)                     # every head of a token asks the same
        for t in range(c.n_q):
            j = E.plant_position(c, t)
            assert 0 <= j < c.n_rows and s[t, j] - np.delete(s[t], j).max() >= E.MARGIN, (c, t)
            assert np.array_equal(q[t], np.broadcast_to(np.float32(beta) * deq[j], q[t].shape))


def test_a_last_plant_is_the_v_row_bit_for_bit_in_the_model():
    span = T.span()
    n = 0
    for seen, _ in E.planted_pairs(span):
        q, _, deq = E.inputs(seen, span)
        got = E.case_model(seen, span)
        for t in range(seen.n_q):
            want = M._h(deq[E.plant_position(seen, t), :DV])
            assert np.array_equal(bits(got[t]), bits(np.broadcast_to(want, got[t].shape))), (seen, t)
            n += 1
        assert E.model_statistic(seen, span) == 0.0, seen
    assert n > 0


@pytest.mark.parametrize("form", E.FORMS)
def test_moving_the_plant_across_the_edge_moves_every_row_by_100_bars(form):
    span = T.span()
    bar = E.tol(form, "planted")
    least = np.inf
    for seen, unseen in E.planted_pairs(span):
        if seen.form != form:
            continue
        V = E.values(seen, span)
        vmax = np.abs(V).max()
        ra, rb = E.case_reference(seen, span), E.case_reference(unseen, span)
        deq = E.inputs(seen, span)[2]
        for t in range(seen.n_q):
            assert np.abs(ra[t] - deq[E.plant_position(seen, t), :DV]).max() / vmax <= 1e-3 * bar, (seen, t)      # the row IS V[j*], far below the bar
            d = np.abs(ra[t] - rb[t]).max(axis=-1).min() / vmax      # the least over the heads of the row's own statistic
            least = min(least, d)
            assert d >= 100 * bar, (seen, t, d, 100 * bar)
    print("form", form, "smallest move of a row", least, "100 bars", 100 * bar)
    assert least < np.inf


@pytest.mark.parametrize("mutant", E.MUTANTS)
def test_the_rescale_mutants_pass_the_merged_flat_sweep_and_not_the_steep_tier(mutant):
    """the gap and its closing: a rescale against the first maximum instead of the running / global one is the model's result on flat inputs -- inside
    np_attention_mla's tolerance on every case of ITS sweep -- and non-finite (or 100 bars out) on the steep tier"""
    span = T.span()
    form = E.MUTANT_FORM[mutant]
    flat = 0.0
    for case in M.cases(form, span):
        kv_type, n_head, n_q, n_kv, causal = case
        ref, V = M.case_reference(case)
        got = E.mutant_model(M.queries(n_head, n_q), M.cache_rows(kv_type, n_kv)[1], n_kv, causal, M.SCALE, span, mutant)
        flat = max(flat, E.mutant_statistic(got, ref, V))
    steep = 0.0
    for c in E.tier_cases(form, "steep", span):
        q, _, deq = E.inputs(c)
        steep = max(steep, E.mutant_statistic(E.mutant_model(q, deq, c.n_kv, c.causal, c.scale, span, mutant), E.case_reference(c), E.values(c)))
    print(mutant, "merged flat sweep", flat, "its tolerance", M.tol_of(M.N_QS[form][0]), "steep tier", steep, "100 bars", 100 * E.tol(form, "steep"))
    assert flat <= M.tol_of(M.N_QS[form][0]), (mutant, flat)
    assert steep >= 100 * E.tol(form, "steep"), (mutant, steep)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


_CACHES, _GOT = {}, {}


def _cache(dev, case, span):
    """the device cache of a case's n_rows rows (nb_pos: the row bytes rounded up to 16), built once per (generator, cache type, rows) -> (tensor, nb_pos)"""
    key = ("plant" if case.tier == "planted" else "ramp" if case.tier == "steep" else "flat", case.kv_type, case.n_rows)
    if key not in _CACHES:
        raw = E.inputs(case, span)[1]
        nb_pos = T._up16(raw.shape[1])
        buf = np.full((case.n_rows, nb_pos), 0xFF, np.uint8)
        buf[:, :raw.shape[1]] = raw
        _CACHES[key] = (dev.torch.from_numpy(buf.reshape(-1)).cuda(), nb_pos)
    return _CACHES[key]


def run(dev, case, span):
    """ggml_hip_attn_mla_dev on a case (n_kv_max = n_rows), computed once -> numpy [n_q, n_head, 512]"""
    if case not in _GOT:
        torch = dev.torch
        cache, nb_pos = _cache(dev, case, span)
        q = torch.from_numpy(E.inputs(case, span)[0]).cuda()
        out = dev.attention_mla(case.kv_type, q, cache, nb_pos, case.n_kv, case.scale, n_kv_max=case.n_rows, causal=case.causal)
        torch.cuda.synchronize()
        _GOT[case] = out.cpu().numpy()
    return _GOT[case]


def held(case, got, bar, span, what=""):
    """the statistic of an output against the case's f64 reference, asserted finite and inside the bar"""
    st = A.statistic(got, E.case_reference(case, span), E.values(case, span))
    print(what, tuple(case), "statistic", st, "bar", bar)
    assert np.isfinite(got).all() and st <= bar, (what, case, st, bar)
    return st


def _expect_form(case):
    rc, p = T._plan(case.kv_type, case.n_head, case.n_q, case.n_rows)
    assert rc == 0 and p.form == case.form, case


@pytest.mark.gpu
@pytest.mark.parametrize("n_q,n_head", E.FLAT_SPLIT + E.FLAT_WALK + E.FLAT_LONG, ids=lambda v: str(v))
def test_every_flat_edge_case_is_inside_its_bar(dev, n_q, n_head):
    span = T.span()
    cases = E.flat_cases(span, ((n_q, n_head),))
    assert len(cases) == (4 if (n_q, n_head) in E.FLAT_LONG else 44)
    worst = 0.0
    for case in cases:
        _expect_form(case)
        worst = max(worst, held(case, run(dev, case, span), E.tol(case.form, "flat"), span))
    print("WORST form", cases[0].form, "flat", (n_q, n_head), worst, "bar", E.tol(cases[0].form, "flat"))


@pytest.mark.gpu
@pytest.mark.parametrize("form", E.FORMS)
def test_every_scale_is_held_to_the_reference_at_that_scale(dev, form):
    span = T.span()
    worst = 0.0
    for tr in E.scale_triples(span):
        if tr[0].form != form:
            continue
        for case in tr:
            _expect_form(case)
            st = held(case, run(dev, case, span), E.scale_bar(case), span, "scale")
            if case.tier == "scale":
                worst = max(worst, st)
    print("WORST form", form, "scale", worst, "bar", E.tol(form, "scale"))


@pytest.mark.gpu
@pytest.mark.parametrize("form", E.FORMS)
def test_the_paged_entry_takes_the_scale_it_is_given(dev, form):
    torch = dev.torch
    span = T.span()
    case = next(c for c in E.scale_cases(span) if c.form == form and c.scale == 0.135 and c.n_kv > PAGE * span and c.kv_type == (F16 if form == SPLIT else Q8_0))
    n_pg = (case.n_kv + PAGE - 1) // PAGE
    pool = T.Pool(case.kv_type, n_pg + 3)
    table = ((), tuple(range(n_pg + 1, 1, -1)))                      # an empty sequence, and one over descending pages
    pool.put(table[1], E.inputs(case)[1])
    lc = pool.cache(dev, table, (0, case.n_kv), case.n_kv)
    q = torch.from_numpy(np.concatenate([E.inputs(case)[0]] * 2)).cuda()
    got = dev.attn_mla_paged(lc, q, case.scale).cpu().numpy().reshape(2, case.n_q, case.n_head, DV)
    assert not bits(got[0]).any()
    held(case, got[1], E.tol(form, "scale"), span, "paged scale")
    assert np.array_equal(bits(got[1]), bits(run(dev, case, span))), ("the contiguous call at the same scale", case)


@pytest.mark.gpu
@pytest.mark.parametrize("slope", E.SLOPES)
@pytest.mark.parametrize("gen", E.STEEP_GENS)
def test_every_steep_case_is_finite_and_inside_its_bar(dev, gen, slope):
    span = T.span()
    worst = {SPLIT: 0.0, WALK: 0.0}
    for case in E.steep_cases(span):
        if (case.gen, case.slope) != (gen, slope):
            continue
        _expect_form(case)
        worst[case.form] = max(worst[case.form], held(case, run(dev, case, span), E.tol(case.form, "steep"), span))
    for form in E.FORMS:
        assert worst[form] > 0.0
        print("WORST form", form, "steep", gen, slope, worst[form], "bar", E.tol(form, "steep"))


@pytest.mark.gpu
@pytest.mark.parametrize("n_q,n_head", E.PLANT_SHAPES, ids=lambda v: str(v))
def test_a_planted_key_is_returned_bit_for_bit_when_seen_and_not_seen_beyond_the_edge(dev, n_q, n_head):
    span = T.span()
    worst, n = 0.0, 0
    for seen, unseen in E.planted_pairs(span):
        if (seen.n_q, seen.n_head) != (n_q, n_head):
            continue
        _expect_form(seen)
        deq = E.inputs(seen, span)[2]
        got = run(dev, seen, span)
        for t in range(n_q):                                         # 'last': the row IS the staged V row of j* = vis(t) - 1
            want = M._h(deq[E.plant_position(seen, t), :DV])
            assert np.array_equal(bits(got[t]), bits(np.broadcast_to(want, got[t].shape))), ("last", seen, t, A.visible(t, seen.n_kv, n_q, seen.causal))
        worst = max(worst, held(unseen, run(dev, unseen, span), E.tol(unseen.form, "planted"), span, "beyond"))
        n += 1
    assert n == (16 if n_q < 70 else 10)
    print("WORST form", M.form_of(n_q), "planted", (n_q, n_head), worst, "bar", E.tol(M.form_of(n_q), "planted"))


# ---- bit contracts at the new shapes ----
def paged_lengths(span):
    S = PAGE * span
    return (0, 1, 63, 64, 65, 127, 128, 129, S - 1, S, S + 1, 2 * S + 37)


N_SEQ = 33


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_33_paged_decode_sequences_of_ragged_lengths_are_the_contiguous_calls_bit_for_bit(dev, kv_type):
    span = T.span()
    base = paged_lengths(span)
    lens = tuple(base[b % len(base)] for b in range(N_SEQ))
    needs = [(n + PAGE - 1) // PAGE for n in lens]
    n_pages = sum(needs) + 7                                         # seven pages belong to nobody: NaN bytes, like every row beyond a length
    perm = [int(p) for p in np.random.default_rng([kv_type, 33]).permutation(n_pages)]
    table, at = [], 0
    for k in needs:
        table.append(tuple(perm[at:at + k]))
        at += k
    flat_ids = [p for row in table for p in row]
    assert len(set(flat_ids)) == len(flat_ids) == sum(needs) and flat_ids != sorted(flat_ids) and all(0 <= p < n_pages for p in flat_ids)
    for n_q in (1, 8):
        got = T.paged(dev, kv_type, 16, n_q, True, lens, tuple(table), n_pages)
        for b, n in enumerate(lens):
            want = np.zeros((n_q, 16, DV), np.float32) if n == 0 else run(dev, E.mk("flat", "flat", kv_type, 16, n_q, n), span)
            assert np.isfinite(got[b]).all() and np.array_equal(bits(got[b]), bits(want)), ("paged decode", n_q, b, n)


def call(dev, kv_type, q, n_kv, causal):
    """the flat cache of n_kv positions under other queries -> numpy [n_q, n_head, 512]"""
    cache, nb_pos = T.contiguous_cache(dev, kv_type, n_kv)
    return dev.attention_mla(kv_type, dev.torch.from_numpy(np.ascontiguousarray(q)).cuda(), cache, nb_pos, n_kv, M.SCALE, causal=causal).cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_rows_of_equal_vis_agree_across_every_n_q_of_a_form_and_across_256_heads(dev, kv_type):
    span = T.span()
    long_kv = 2 * PAGE * span + 37
    for big, smalls, n_head in ((8, (1, 2, 5), 16), (129, (9,), 3)):
        for n_kv in (65, long_kv):
            for causal in (True, False):
                want = run(dev, E.mk("flat", "flat", kv_type, n_head, big, n_kv, causal=causal), span)
                for small in smalls:
                    assert T._plan(kv_type, n_head, small, n_kv)[1].form == T._plan(kv_type, n_head, big, n_kv)[1].form
                    rows = slice(big - small, big) if causal else slice(0, small)      # the last rows of the longer call, causal; the first, not causal
                    got = call(dev, kv_type, M.queries(n_head, big)[rows], n_kv, causal)
                    assert np.array_equal(bits(got), bits(want[rows])), ("n_q", small, big, causal, n_kv)
    for n_q in (2, 9):                                               # head h of a 256-head call against the same rows alone at n_head = 1
        want = run(dev, E.mk("flat", "flat", kv_type, 256, n_q, long_kv), span)
        assert np.isfinite(want).all()
        for h in (0, 100, 255):
            one = call(dev, kv_type, M.queries(256, n_q)[:, h:h + 1], long_kv, True)
            assert np.array_equal(bits(one[:, 0]), bits(want[:, h])), ("n_head", n_q, h)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_the_split_result_does_not_depend_on_what_the_work_buffer_held(dev, kv_type):
    """n_kv_max = n_kv + 2 S: two whole spans of every row get no partial, and the merge must not read what lies there -- 0x7F bytes (m = 3.4e38), 0xFF
    bytes (NaN), or the partials a longer call over the same buffer left"""
    torch = dev.torch
    span = T.span()
    S = PAGE * span
    guard = 512
    for n_q, n_head in ((1, 16), (8, 3)):
        for n_kv in (65, 2 * S + 37):
            n_kv_max = n_kv + 2 * S
            case = E.mk("flat", "flat", kv_type, n_head, n_q, n_kv)
            base = run(dev, case, span)
            cache, nb_pos = T.contiguous_cache(dev, kv_type, n_kv_max)           # (finite rows up to n_kv_max: the longer call reads them)
            q = torch.from_numpy(M.queries(n_head, n_q)).cuda()
            need = dev.attn_mla_work_size(kv_type, n_head, n_q, n_kv_max)
            assert need >= n_q * n_head * ((n_kv_max + S - 1) // S) * (DV + 4) * 4
            for fill in (0x7F, 0xFF, "longer"):
                work_big = torch.full((need + 2 * guard,), 0xA5 if fill == "longer" else fill, dtype=torch.uint8, device="cuda")
                work_big[:guard] = 0xA5
                work_big[guard + need:] = 0xA5
                work = work_big[guard:guard + need]
                if fill == "longer":
                    longer = dev.attention_mla(kv_type, q, cache, nb_pos, n_kv_max, M.SCALE, n_kv_max=n_kv_max, work=work).cpu().numpy()
                    assert np.isfinite(longer).all() and not np.array_equal(bits(longer), bits(base))
                got = dev.attention_mla(kv_type, q, cache, nb_pos, n_kv, M.SCALE, n_kv_max=n_kv_max, work=work).cpu().numpy()
                assert np.array_equal(bits(got), bits(base)), ("work prefill", fill, n_q, n_head, n_kv)
                w = work_big.cpu().numpy()
                assert (w[:guard] == 0xA5).all() and (w[guard + need:] == 0xA5).all(), "the work buffer's guards were written"


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_eight_rows_are_split_and_nine_rows_over_the_same_cache_are_walk(dev, kv_type):
    span = T.span()
    for n_kv in (65, 2 * PAGE * span + 37):
        assert T._plan(kv_type, 16, 8, n_kv)[1].form == SPLIT and T._plan(kv_type, 16, 9, n_kv)[1].form == WALK
        ref, V = M.case_reference((kv_type, 16, 9, n_kv, True))      # one reference: the last eight tokens of nine see what the eight alone see
        nine = run(dev, E.mk("flat", "flat", kv_type, 16, 9, n_kv), span)
        eight = call(dev, kv_type, M.queries(16, 9)[1:], n_kv, True)
        st9, st8 = A.statistic(nine, ref, V), A.statistic(eight, ref[1:], V)
        print("nine rows", kv_type, n_kv, "statistic", st9, "bar", M.TOL_WALK, "eight rows", st8, "bar", M.TOL_SPLIT)
        assert np.isfinite(nine).all() and np.isfinite(eight).all() and st9 <= M.TOL_WALK and st8 <= M.TOL_SPLIT
