"""The attention kernels where tests/test_attention*.py do not go (csrc/attn.hip: the DECODE and PROMPT chunk bodies, their paged twins, the _ex
variants): every group size G = n_head / n_head_kv the entries accept and is not a power of two, every n_q of the DECODE form, R = G n_q up to
128 rows in a workgroup with a ragged last pass behind full ones, caches of six and nine chunks, the PROMPT form at the wave edge (32 / 33), the
workgroup edge (127 / 128 / 129) and in a third workgroup (257), n_q > n_kv > 1, an explicit `scale` (alone, under a soft-cap as sc' = scale / cap,
and through the paged entry), softmaxes that are not flat, and mask edges that a single planted key makes visible.

Yardsticks (tests/np_attention_edges.py): always the float64 reference over the DEQUANTIZED cache, never the library; the statistic
max |dst - ref| / max |V|; the bar of a (form, regime) is 4 x what the numpy model measures on that regime's own sweep, recomputed on the CPU
here.  Two conditions on the INPUTS are checked on the CPU, as test_attention_ex.py does for its options: the references of a case at any two
scales lie at least 100 bars apart (a kernel or launcher that ignores the argument cannot pass), and moving a planted key across the causal edge
or the window's edge moves EVERY row that has such a position by at least 100 bars (a mask that is off by one cannot pass).
Bitwise promises of the headers, at shapes they were never held at: a paged sequence is the contiguous call (lengths 1100, 0, 641, 129 over a
shuffled table, with and without a window); a DECODE row does not depend on the rows around it; heads that share a kv head and are given the same
q rows return the same bits.

Nothing here failed because of a kernel: csrc/attn.hip and attn.cpp are unchanged.  Two things were the generator's and are fixed there: a slope
of 0.1 in the 'rising' / 'falling' inputs put the PROMPT bar of the peaked regime above 1e-2 (0.08 is used), and the scale tier's PROMPT shapes
with n_q < n_kv (every row sees hundreds of positions of a flat softmax) moved by 0.03 - 0.16 of max |V| between two scales against 100 bars of 0.188, so that tier runs the
shapes with n_q >= n_kv."""
import itertools

import numpy as np
import pytest

import np_attention as A
import np_attention_edges as E
import np_attention_ex as X
import test_attention as T                                           # Cache, _plan
import test_attention_paged as P                                     # Pool

F16, Q8_0 = A.F16, A.Q8_0
DECODE, PROMPT = 1, 2
FORMS = ("decode", "prompt")


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---------------------------------------------------------------- CPU
def test_the_sweeps_hold_every_group_size_row_count_and_edge_by_name():
    dec = E.shape_cases("decode")
    assert {c.n_head // c.n_head_kv for c in dec} >= {1, 3, 4, 5, 7, 12, 16}
    assert {c.n_q for c in dec} == set(range(1, 9))
    assert {c.n_head // c.n_head_kv * c.n_q for c in dec} >= {9, 20, 35, 28, 96, 128, 16, 6, 8}
    have = {(c.n_head, c.n_head_kv, c.n_q, c.n_kv, c.D, c.kv_type) for c in dec}
    for nh, nhk, n_q in ((3, 1, 3), (12, 3, 5), (5, 1, 7), (14, 2, 4), (12, 1, 8), (16, 1, 8), (16, 1, 1), (6, 6, 6), (2, 2, 8)):
        for n_kv in (127, 128, 641, 1100):
            for D, t in itertools.product((64, 128), (F16, Q8_0)):
                assert (nh, nhk, n_q, n_kv, D, t) in have, (nh, nhk, n_q, n_kv, D, t)
        assert any(not c.causal for c in dec if (c.n_head, c.n_head_kv, c.n_q) == (nh, nhk, n_q))
    assert any(c.n_kv == 5 and c.n_q == 8 for c in dec)
    pro = E.shape_cases("prompt")
    have = {(c.n_q, c.n_kv, c.n_head, c.n_head_kv, c.D, c.kv_type) for c in pro}
    for shape in ((32, 32), (33, 160), (127, 128), (128, 128), (128, 255), (129, 429), (257, 257), (257, 641), (40, 17)):
        for heads in ((3, 1), (12, 3), (16, 1), (5, 5)):
            for D, t in itertools.product((64, 128), (F16, Q8_0)):
                assert shape + heads + (D, t) in have, (shape, heads, D, t)
    for heads in E.PROMPT_HEADS:
        assert any(not c.causal for c in pro if (c.n_head, c.n_head_kv) == heads)
    for cases in (dec, pro):
        assert any(c.n_rows - c.n_kv >= E.SLACK for c in cases)      # n_kv on the device, n_kv_max > n_kv
    # the scale tier: all three scales without a cap, the two explicit ones under it; a ragged multi-pass DECODE case and a multi-workgroup
    # PROMPT case per cache type
    for form in FORMS:
        for (shape, cap), cs in E.scale_cases(form).items():
            assert [c.scale for c in cs] == list(E.SCALES if cap == 0 else E.SCALES[1:]) and all(c.softcap == cap for c in cs)
    for t in (F16, Q8_0):
        assert any(s[3] == t and s[1] // s[2] * s[4] > 8 and s[1] // s[2] * s[4] % 8 for s in E.SCALE_SHAPES["decode"])
        assert any(s[3] == t and s[4] > 128 for s in E.SCALE_SHAPES["prompt"])
    # the peaked tier: both forms, both cache types, both D, heads (5, 1) and (12, 3), the long caches
    for form, shapes in (("decode", {(7, 641), (7, 1100), (5, 641), (5, 1100)}), ("prompt", {(129, 429), (257, 641)})):
        cs = E.peaked_cases(form)
        assert {(c.n_q, c.n_kv) for c in cs} == shapes and {(c.n_head, c.n_head_kv) for c in cs} == {(5, 1), (12, 3)}
        for gen in E.PEAKED_GENS:
            assert {(c.D, c.kv_type) for c in cs if c.gen == gen} == set(E.DT)
    # the planted tier: the shapes, every window, every (D, cache type) pair in each form
    assert {s[1:3] + s[4:] for s in E.planted_shapes("decode")} == {(nh, nhk, n_q, n) for nh, nhk, n_q in ((5, 1, 7), (16, 1, 8)) for n in (128, 129, 641)}
    assert {s[4:] for s in E.planted_shapes("prompt")} == {(33, 160), (128, 255), (129, 429), (257, 641)}
    for form in FORMS:
        assert {s[:1] + s[3:4] for s in E.planted_shapes(form)} == set(E.DT)
        assert {c.window for c in E.planted_cases(form)} == {0, 5, 128, 200}
    # the limits, and no case twice
    for form in FORMS:
        for tier in E.TIERS:
            cs = E.tier_cases(form, tier)
            assert len(set(cs)) == len(cs) and cs
            for c in cs:
                assert c.form == form and c.n_head <= 16 and c.n_q <= 257 and c.n_kv <= 1100 and c.n_rows <= 1100 + E.SLACK
                assert (c.n_q <= A.DECODE_MAX_Q) == (form == "decode")


@pytest.mark.parametrize("tier", E.TIERS)
@pytest.mark.parametrize("form", FORMS)
def test_the_edge_model_constants_are_what_the_model_measures(form, tier):
    rec = E.MODEL_WORST[(form, tier)]
    worst = E.model_worst(form, tier)
    print(form, tier, "model worst", worst, "recorded", rec, "bar", E.tol(form, tier))
    assert rec / 1.25 <= worst <= rec, (form, tier, worst, rec)
    base_rec, base_tol = (A.MODEL_WORST_DECODE, A.TOL_DECODE) if form == "decode" else (A.MODEL_WORST_PROMPT, A.TOL_PROMPT)
    assert E.tol(form, tier) == (base_tol if tier == "flat" and rec <= base_rec else 4 * rec)
    if (form, tier) == ("prompt", "peaked"):
        assert E.tol(form, tier) <= 1e-2


@pytest.mark.parametrize("form", FORMS)
def test_the_references_of_a_case_at_any_two_scales_are_100_bars_apart(form):
    """a condition on the INPUTS: ignoring `scale` (or computing rsqrt(D), or dropping it from sc' = scale / cap) cannot pass"""
    bar = E.tol(form, "flat")
    least = np.inf
    for (shape, cap), cs in E.scale_cases(form).items():
        Vd = E.inputs(cs[0])[4]
        for a, b in itertools.combinations(cs, 2):
            d = A.statistic(E.case_reference(a), E.case_reference(b), Vd)
            least = min(least, d)
            assert d >= 100 * bar, (shape, cap, a.scale, b.scale, d, 100 * bar)
    print(form, "smallest distance between two scales", least, "100 bars", 100 * bar)


def _edge_rows(seen):
    """the rows of a planted pair that have a position on BOTH sides of the edge: every row with a visible position (the causal edge: the cache
    holds PLANT_EXTRA rows beyond n_kv), every row whose window starts above position 0 (the window's edge)"""
    hi = [A.visible(t, seen.n_kv, seen.n_q, seen.causal) for t in range(seen.n_q)]
    return [t for t in range(seen.n_q) if hi[t] >= 1 and (seen.window == 0 or X.window_lo(hi[t], seen.window) >= 1)]


@pytest.mark.parametrize("form", FORMS)
def test_moving_the_plant_across_an_edge_moves_every_row_by_100_bars(form):
    bar = E.tol(form, "planted")
    least, behind = np.inf, {W: 0 for W in E.PLANT_WINDOWS}
    for shape in E.planted_shapes(form):
        G = shape[1] // shape[2]
        for seen, unseen in E.planted_pairs(form, shape):
            rows = _edge_rows(seen)
            assert rows == [t for t in range(seen.n_q) if E.plant_position(seen, t) is not None and E.plant_position(unseen, t) is not None]
            if seen.window == 0:
                assert len(rows) == min(seen.n_q, seen.n_kv)
            else:
                behind[seen.window] += len(rows)                     # (none where W >= n_kv: no position lies behind such a window)
                assert (len(rows) > 0) == (seen.window < seen.n_kv)
            if not rows:
                continue
            beta = E.plant_beta(seen)
            assert beta == E.plant_beta(unseen) and np.log2(beta) == int(np.log2(beta))
            Vd = E.inputs(seen)[4]
            vmax = np.abs(Vd).max()
            ra, rb = E.case_reference(seen), E.case_reference(unseen)
            for t in rows:
                j = E.plant_position(seen, t)
                assert np.abs(ra[t] - Vd[j, np.arange(shape[1]) // G]).max() / vmax <= 1e-3 * bar, (seen, t)      # the row IS V[j*], far below the bar
                d = np.abs(ra[t] - rb[t]).max(axis=-1).min() / vmax  # the least over the heads of the row's own statistic
                least = min(least, d)
                assert d >= 100 * bar, (seen, t, d, 100 * bar)
    assert all(n > 0 for n in behind.values())
    print(form, "smallest move of a row", least, "100 bars", 100 * bar)


def test_the_generators_do_what_they_say():
    # peaked: scale * q . k has a standard deviation of about SIGMA
    c = E.mk("decode", "peaked", 64, 5, 1, F16, 7, 1100)
    q, _, _, Kd, _ = E.inputs(c)
    s = E.scale_of(c) * np.einsum("thd,jd->thj", q.astype(np.float64), Kd[:, 0].astype(np.float64))
    assert 0.9 * E.SIGMA <= s.std() <= 1.1 * E.SIGMA
    assert np.array_equal(E.inputs(c)[1], E.inputs(c._replace(gen="flat"))[1])                 # the flat cache, untouched
    # planted: deq(K) is +-0.125 exactly in both cache types and q = beta K with beta a power of two: every score is exact in f32 and in f16
    for form in FORMS:
        for c in E.planted_cases(form):
            q, _, _, Kd, _ = E.inputs(c)
            assert (np.abs(Kd) == 0.125).all() and np.abs(q).max() in (0.125 * E.plant_beta(c), 0.0) and E.plant_beta(c) <= 4096
    for D, t in E.DT:
        sc = np.float32(1.0 / np.sqrt(D))
        for gen in ("rising", "falling"):
            c = E.mk("decode", gen, D, 5, 1, t, 7, 1100)
            q, _, _, Kd, _ = E.inputs(c)
            s = (sc * (Kd[:, 0] @ q[-1, 0])).astype(np.float32)                                # the last row sees every position
            m = np.array([s[j:j + A.CHUNK].max() for j in range(0, 1100, A.CHUNK)])
            with np.errstate(under="ignore"):
                b = np.exp((m - m.max()).astype(np.float32))
            if gen == "rising":
                assert (np.diff(m) > 4).all() and b[-1] == 1                                   # every chunk raises the running maximum
            else:
                assert (np.diff(m) < -4).all() and b[0] == 1                                   # the maximum in chunk 0 ...
                assert b[-1] < 1e-33 and float(np.float16(b[2])) == 0.0                        # ... the last chunk near the f32 subnormals, f16(p) gone from chunk 2 on


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


_CACHES = {}


def _cache(dev, case, layout):
    """the 0xFF-padded device cache of a case's n_rows rows, built once per (cache bytes, layout)"""
    key = (E.input_key(case)[0], layout)
    if key not in _CACHES:
        _, Kraw, Vraw, _, _ = E.inputs(case)
        _CACHES[key] = T.Cache(dev, case.kv_type, case.D, case.n_head_kv, case.n_rows, layout, Kraw, Vraw)
    return _CACHES[key]


def run(dev, case, layout=0, pad=0, rows=None, n_kv=None, q=None):
    """one contiguous call on a case -> numpy [n_q, n_head, D], through device.attention: ggml_hip_attn_dev, or ggml_hip_attn_ex_dev when the case
    has a window or a cap.  n_kv is read on the device where the cache holds SLACK rows more than the case uses; pad: extra elements in the strides
    of q and dst, which must come back untouched; rows: these query rows as a batch of their own (n_kv is then the caller's); q: other queries"""
    torch = dev.torch
    qh = E.inputs(case)[0] if q is None else q
    if rows is not None:
        qh = qh[rows]
    n_q, n_head, D = qh.shape
    n_kv = case.n_kv if n_kv is None else n_kv
    on_dev = case.n_rows - case.n_kv >= E.SLACK
    cache = _cache(dev, case, layout)
    qd = torch.zeros((n_q, n_head, D + pad), device="cuda")
    qd[:, :, :D] = torch.from_numpy(np.ascontiguousarray(qh)).cuda()
    out = torch.full((n_q, n_head, D + pad), -7.0, device="cuda")
    d_n = torch.tensor([n_kv], dtype=torch.int32, device="cuda") if on_dev else None
    dev.attention(case.kv_type, qd[:, :, :D], cache.k, cache.v, cache.nb_pos, cache.nb_head, case.n_head_kv, 0 if on_dev else n_kv, d_n_kv=d_n,
                  n_kv_max=case.n_rows, causal=case.causal, scale=E.scale_of(case), out=out[:, :, :D], window=case.window, softcap=case.softcap)
    torch.cuda.synchronize()
    if pad:
        assert bool((out[:, :, D:] == -7.0).all()), ("padding", case)
    return out[:, :, :D].cpu().numpy()


def held(case, got, tier, what=""):
    """the statistic of an output against the case's f64 reference, asserted finite and inside the regime's bar"""
    bar = E.tol(case.form, tier)
    st = A.statistic(got, E.case_reference(case), E.inputs(case)[4])
    print(what, tuple(case), "statistic", st, "bar", bar)
    assert np.isfinite(got).all() and st <= bar, (what, case, st, bar)
    return st


def _expect_form(case):
    rc, p = T._plan(case.kv_type, case.D, case.n_head, case.n_head_kv, case.n_q, case.n_rows)
    assert rc == 0 and p.form == (DECODE if case.form == "decode" else PROMPT), case
    return p


SHAPE_PARAMS = [("decode", h) for h in E.DECODE_HEADS] + [("decode", E.DECODE_SHORT[:3])] + [("prompt", h) for h in E.PROMPT_HEADS]


@pytest.mark.gpu
@pytest.mark.parametrize("form,heads", SHAPE_PARAMS, ids=lambda v: v if isinstance(v, str) else "x".join(map(str, v)))
def test_every_shape_case_is_inside_its_bar(dev, form, heads):
    sel = [c for c in E.shape_cases(form) if ((c.n_head, c.n_head_kv, c.n_q) if form == "decode" else (c.n_head, c.n_head_kv)) == tuple(heads)]
    assert sel
    worst = 0.0
    for i, case in enumerate(sel):
        p = _expect_form(case)
        assert p.n_chunks == (case.n_rows + A.CHUNK - 1) // A.CHUNK
        worst = max(worst, held(case, run(dev, case, layout=i % 2, pad=4 * (i % 3)), "flat"))
    print("WORST", form, "flat", worst)


@pytest.mark.gpu
@pytest.mark.parametrize("D,kv_type", E.DT)
def test_eight_rows_are_decode_and_nine_rows_over_the_same_cache_are_prompt(dev, D, kv_type):
    case = next(c for c in E.shape_cases("decode") if (c.D, c.kv_type, c.n_head, c.n_head_kv, c.n_q, c.n_kv) == (D, kv_type, 12, 1, 8, 641))
    assert T._plan(kv_type, D, 12, 1, 8, case.n_rows)[1].form == DECODE and T._plan(kv_type, D, 12, 1, 9, case.n_rows)[1].form == PROMPT
    q8, _, _, Kd, Vd = E.inputs(case)
    q9 = np.concatenate([q8, np.random.default_rng(9).uniform(-1, 1, (1,) + q8.shape[1:]).astype(np.float32)])
    held(case, run(dev, case), "flat", "eight rows")
    got = run(dev, case, q=q9, pad=4)
    st = A.statistic(got, A.reference(q9, Kd, Vd, 641, True, E.scale_of(case)), Vd)
    print("nine rows", D, kv_type, "statistic", st, "bar", E.tol("prompt", "flat"))
    assert np.isfinite(got).all() and st <= E.tol("prompt", "flat")
    assert st > E.tol("decode", "flat")                              # (the f16 operands of the PROMPT form show: it was not the DECODE kernels again)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_every_scale_is_held_to_the_reference_at_that_scale(dev, form):
    worst, i = 0.0, 0
    for (shape, cap), cs in E.scale_cases(form).items():
        for case in cs:
            _expect_form(case)
            worst = max(worst, held(case, run(dev, case, layout=i % 2, pad=4 * (i % 3)), "flat", "scale"))
            i += 1
    print("WORST", form, "scale", worst)


N_PAGES = 20


def paged(dev, seqs, table, layout=0):
    """one paged call, a Case per sequence (None: an empty one) with its rows where `table` says -> numpy [n_seq, n_q, n_head, D]"""
    torch = dev.torch
    first = next(c for c in seqs if c is not None)
    pool = P.Pool(first.kv_type, first.D, first.n_head_kv, layout, N_PAGES)
    qs, lens = [], []
    for c, pages in zip(seqs, table):
        lens.append(0 if c is None else c.n_kv)
        qs.append(E.inputs(first if c is None else c)[0])
        if c is not None:
            assert c[2:7] == first[2:7] and c[9:] == first[9:]
            pool.put(0, pages, E.inputs(c)[1], c.n_kv)
            pool.put(1, pages, E.inputs(c)[2], c.n_kv)
    pc = pool.cache(dev, table, lens, max(lens))
    q = torch.from_numpy(np.concatenate(qs)).cuda()
    out = dev.attn_paged(pc, q, first.n_head_kv, causal=first.causal, scale=E.scale_of(first), window=first.window, softcap=first.softcap)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(seqs), first.n_q, first.n_head, first.D)


@pytest.mark.gpu
@pytest.mark.parametrize("form", FORMS)
def test_the_paged_entry_takes_the_scale_it_is_given(dev, form):
    for shape in E.SCALE_SHAPES[form][:2]:                           # one per cache type: R = 35 (DECODE), three workgroups (PROMPT)
        n_chunks = (shape[5] + A.CHUNK - 1) // A.CHUNK
        table = ((), tuple(range(N_PAGES - 1, N_PAGES - 1 - n_chunks, -1)))
        for case in E.scale_cases(form)[(shape, 0.0)][1:] + E.scale_cases(form)[(shape, E.SCALE_SOFTCAP)]:
            got = paged(dev, [None, case], table, layout=1)
            assert np.array_equal(bits(got[0]), np.zeros_like(bits(got[0])))
            held(case, got[1], "flat", "paged scale")
            assert np.array_equal(bits(got[1]), bits(run(dev, case))), ("the contiguous call at the same scale", case)


@pytest.mark.gpu
@pytest.mark.parametrize("gen", E.PEAKED_GENS)
@pytest.mark.parametrize("form", FORMS)
def test_every_peaked_case_is_inside_its_bar(dev, form, gen):
    worst = 0.0
    for i, case in enumerate(c for c in E.peaked_cases(form) if c.gen == gen):
        _expect_form(case)
        worst = max(worst, held(case, run(dev, case, layout=i % 2, pad=4 * (i % 3)), "peaked"))
    print("WORST", form, "peaked", gen, worst)


PLANT_PARAMS = [(form, i) for form in FORMS for i in range(len(E.planted_shapes(form)))]


@pytest.mark.gpu
@pytest.mark.parametrize("form,i", PLANT_PARAMS)
def test_a_planted_key_is_seen_on_one_side_of_every_edge_and_not_on_the_other(dev, form, i):
    shape = E.planted_shapes(form)[i]
    worst = 0.0
    for k, (seen, unseen) in enumerate(E.planted_pairs(form, shape)):
        for case in (seen, unseen):
            _expect_form(case)
            worst = max(worst, held(case, run(dev, case, layout=(i + k) % 2, pad=4 * (k % 3)), "planted", case.gen))
    print("WORST", form, "planted", worst)


# ---- bitwise promises at the new shapes ----
LENGTHS = (1100, 0, 641, 129)


def _table():
    perm = [int(p) for p in np.random.default_rng(5).permutation(N_PAGES)]
    out = []
    for n in LENGTHS:
        k = (n + A.CHUNK - 1) // A.CHUNK
        out.append(tuple(perm[:k]))
        perm = perm[k:]
    return tuple(out)


@pytest.mark.gpu
@pytest.mark.parametrize("window", [0, 200])
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_every_paged_sequence_is_the_contiguous_call_bit_for_bit(dev, kv_type, window):
    table = _table()
    assert sorted(p for row in table for p in row) != [p for row in table for p in row] and len({p for row in table for p in row}) == 9 + 6 + 2
    Da, Db = (128, 64) if kv_type == F16 else (64, 128)
    for form, D, nh, nhk, n_q in (("decode", Da, 5, 1, 7), ("decode", Db, 16, 1, 8), ("prompt", Db, 12, 3, 257)):
        seqs = [None if n == 0 else E.mk(form, "flat", D, nh, nhk, kv_type, n_q, n, window=window) for n in LENGTHS]
        got = paged(dev, seqs, table, layout=(D == 64))
        for b, c in enumerate(seqs):
            want = np.zeros_like(got[b]) if c is None else run(dev, c, layout=b % 2, pad=4)
            assert np.isfinite(got[b]).all() and np.array_equal(bits(got[b]), bits(want)), (form, D, nh, n_q, window, b, LENGTHS[b])
            if c is not None and not window:
                held(c, got[b], "flat", "paged")


@pytest.mark.gpu
@pytest.mark.parametrize("D,kv_type", E.DT)
def test_a_decode_row_of_35_does_not_depend_on_the_rows_around_it(dev, D, kv_type):
    case = E.mk("decode", "flat", D, 5, 1, kv_type, 7, 641)
    base = run(dev, case)
    for t in range(7):                                               # the row alone sees the same positions with n_kv - (n_q - 1 - t) in the cache
        alone = run(dev, case, rows=slice(t, t + 1), n_kv=641 - (6 - t), layout=t % 2)
        assert np.array_equal(bits(base[t:t + 1]), bits(alone)), (D, kv_type, t)


@pytest.mark.gpu
@pytest.mark.parametrize("D,kv_type", E.DT)
def test_heads_that_share_a_kv_head_and_a_query_return_the_same_bits(dev, D, kv_type):
    for form, nh, n_q, n_kv in (("decode", 5, 7, 641), ("decode", 16, 8, 1100), ("prompt", 5, 33, 160), ("prompt", 16, 129, 429)):
        case = E.mk(form, "flat", D, nh, 1, kv_type, n_q, n_kv)
        q = E.inputs(case)[0].copy()
        q[:, 1:] = q[:, :1]
        got = run(dev, case, q=q)
        assert np.isfinite(got).all() and np.abs(got).max() > 0
        for h in range(1, nh):
            assert np.array_equal(bits(got[:, 0]), bits(got[:, h])), (form, D, kv_type, nh, h)
