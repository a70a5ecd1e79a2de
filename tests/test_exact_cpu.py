"""The exact tier without a GPU: the construction of tests/exact_inputs.py against the oracle, and the coverage guard of its
representative table.

- The oracle's sequential f32 loop equals exact_product() bit for bit, for all six legacy types, in the normal, tiny-normal and
  subnormal zones: the construction really makes the reference's result independent of summation order.
- The oracle's quantizers round the tie rows as numpy's independent statement of each rule says (half to even where the reference
  calls Math.Round; (int)(v + 16.5f) / (uint)(v + 0.5f) for Q5_0 / Q5_1; the first max-|x| element sets the sign of d).
- The generators really produce ties of both parities and signs, near-ties, and each zone.
- Every kernel the plan reaches over test_plan_cpu.py's wide sweep -- keyed by (type, force, family, form, image, flags, K3p's in-loop
  table refill, a partial last stage or range) -- has a representative within the budget, so a new form cannot land without an exact
  case.  Left out: GGML_HIP_PLAN_WIDE plans (a weight plane over 4 GiB cannot be a test case) and, stated by name, the k-quant types
  (E.KQUANT_TYPES): this tier covers the six legacy types and F16 / F32."""
import numpy as np
import pytest

import exact_inputs as E
import oracle_lib as O

RNG = np.random.default_rng(7)


@pytest.mark.parametrize("zone", E.ZONES)
@pytest.mark.parametrize("t", E.LEGACY)
def test_oracle_mul_mat_is_bitwise_the_exact_product(t, zone):
    n_sub = 0
    for (M, K, N) in ((1, 32, 1), (5, 288, 7), (17, 1056, 3), (3, 4096, 9), (2, 22016, 2)):
        a, b = E.zone_exponents(t, zone, RNG, M, N)
        j = E.jitter_for(t, K)
        raw, w = E.weight_blocks(t, M, K, a, RNG, jitter=j)
        x, q, d, _ = E.act_rows(N, K, b, RNG, E.wmax(t) << j, jitter=j)
        qi = E.act_ints(q, d, b)
        E.assert_exactly_representable(w, qi, a, b)
        # the construction's integers are what the reference's quantizer and dequantizer see
        assert np.array_equal(O.dequantize_row(t, raw, K).astype(np.float64), np.ldexp(w.astype(np.float64), a[:, None]))
        dq, qq = E.q8_rule(x)
        assert np.array_equal(qq, q) and np.array_equal(dq, d)
        ref = O.mul_mat(t, raw, x, M, K, N)[0, 0]
        want = E.exact_product(w, a, qi, b)
        assert np.array_equal(E.f32_bits(ref), E.f32_bits(want)), (t, zone, M, K, N)
        n_sub += int(((want != 0) & (np.abs(want) < 2.0 ** -126)).sum())
    assert (n_sub > 0) == (zone == "subnormal"), n_sub


def test_the_bound_is_asserted():
    w = np.full((1, 64), 127)
    q = np.full((1, 64), 127)
    with pytest.raises(AssertionError):
        E.assert_exactly_representable(np.repeat(w, 1, 0), np.tile(q, (1, 32)).reshape(1, -1)[:, :64] * 40)
    E.assert_exactly_representable(w, q, np.array([0]), np.array([0]))
    with pytest.raises(AssertionError):
        E.assert_exactly_representable(w, q, np.array([-100]), np.array([-50]))      # 2^-150: below the f32 subnormals


@pytest.mark.parametrize("t", E.LEGACY + (E.Q8_1,))
def test_oracle_quantizers_round_the_tie_rows_as_stated(t):
    K = 256
    a = RNG.integers(-30, 10, 16)
    x = E.weight_tie_rows(t, K, a, RNG)
    d, codes = E.expected_weight_quants(t, x)
    raw = O.quantize_row(t, x)
    assert np.array_equal(E.decode_codes(t, raw, K), codes), t
    bs = 16 if t == E.Q4_2 else 32
    # d is the power of two (with the sign the first max-|x| element gives it) for every block
    assert np.array_equal(np.abs(d), np.repeat(np.ldexp(np.float32(1), a)[:, None], K // bs, axis=1).astype(np.float32))
    # the rows hold ties that decide the rule: half-even (rint) and half-up / truncation differ on them
    xi = (x.astype(np.float64).reshape(16, -1, bs) / np.abs(d.astype(np.float64))[..., None]).reshape(16, K)
    frac = xi - np.floor(xi)
    assert (frac == 0.5).sum() >= K, "too few exact ties"
    if t in (E.Q4_0, E.Q4_2, E.Q5_0):                    # the clamp at 15 / 31 is reached, and d of both signs
        assert (codes == (15 if t != E.Q5_0 else 31)).any() and (d > 0).any() and (d < 0).any()
    if t in (E.Q4_0, E.Q4_1, E.Q4_2, E.Q8_0, E.Q8_1):    # half to even: some ties round down, some up
        cand = np.abs(xi[frac == 0.5])
        assert (np.floor(cand) % 2 == 0).any() and (np.floor(cand) % 2 == 1).any()


def test_generators_produce_ties_near_ties_and_every_zone():
    b = np.array([0, -3, 5, -120])
    x, q, d, info = E.act_rows(4, 8 * 32, b, RNG, 8)
    assert info["ties"] >= 40 and info["ties_odd"] >= 10 and info["ties_even"] >= 10 and info["ties_neg"] >= 10
    assert info["ties_126_5"] >= 4
    assert all(info["blocks"][k] > 0 for k in E.KINDS)
    xs = x.astype(np.float64) / np.ldexp(1.0, b)[:, None]
    assert ((xs - np.floor(xs)) == 0.5).sum() == info["ties"]
    assert np.array_equal(np.rint(xs), q)                                      # the quants are the half-even ones
    assert ((np.abs(xs) == 126.5) & (q == np.sign(xs) * 126)).sum() == info["ties_126_5"]
    # a long K keeps the bound by giving up body and ties, not the bound
    _, q2, _, info2 = E.act_rows(2, 22016, np.zeros(2, np.int64), RNG, 128)
    assert (np.abs(q2).sum(axis=1) * 128 < E.EXACT_BOUND).all() and info2["ties"] > 0
    # near-ties, for every quantizer's rule: planted, each really separates (x - off) * id from (x - off) / d, and the oracle multiplies
    for t in E.LEGACY + (E.Q8_1,):
        xn, planted = E.near_tie_rows(4, 128, RNG, t)
        assert planted >= 4 * 4
        d, mul = E.expected_weight_quants(t, xn)
        _, div = E.expected_weight_quants(t, xn, divide=True)
        assert (mul != div).sum() == planted, t
        assert np.array_equal(E.decode_codes(t, O.quantize_row(t, xn), 128), mul), t
        assert not (np.log2(np.abs(d)) == np.round(np.log2(np.abs(d)))).any()   # (non-power-of-two scales)
    # the zones
    for t in E.LEGACY:
        for zone, lo, hi in (("normal", -30, 10), ("tiny", -125, -95), ("subnormal", -149, -127)):
            a, bb = E.zone_exponents(t, zone, RNG, 50, 50)
            s = a[:, None] + bb[None, :]
            assert s.min() >= lo and s.max() <= hi, (t, zone, s.min(), s.max())
            assert bb.min() >= -120
        a, _ = E.zone_exponents(t, "subnormal", RNG, 50, 1)
        if t in E.F16_SCALE:
            assert (a < -14).any()                                             # an f16-subnormal d
        else:
            assert (a < -126).all()                                            # an f32-subnormal d


# ------------------------------------------------------------------------------------------------------------- coverage guard
@pytest.fixture(scope="module")
def table():
    return E.representatives()


def test_representative_table_reaches_every_key_of_the_wide_sweep(table):
    """every key reachable over test_plan_cpu.py's sweep, for every quantized type and F16 / F32 (WIDE plans aside), has a representative
    within E.BUDGET -- except, by name, the k-quant types' keys"""
    import test_plan_cpu as P
    wide = E.sweep_keys(P.KS, P.NS, P.MS, types=E.TABLE_TYPES + E.KQUANT_TYPES)
    missing = E.unreached(wide, table)
    assert {k[0] for k in missing} <= set(E.KQUANT_TYPES), f"plan keys without an exact case: {[k for k in missing if k[0] not in E.KQUANT_TYPES][:5]}"
    assert all(k[0] in E.KQUANT_TYPES for k in missing) and any(k[0] in E.KQUANT_TYPES for k in wide)   # (the exclusion is real, and only that)
    assert all(M * K * N <= E.BUDGET for (M, K, N) in table.values())
    # the helper the guard stands on does report a dropped key
    k = next(k for k in wide if k[0] == E.Q8_0)
    assert E.unreached(wide, {kk: v for kk, v in table.items() if kk != k}) == sorted(set(missing) | {k})


def test_min_piece_forms_keep_what_split3_keeps():
    """the stated deviation, restated: a normal min of at most 24 significant bits is kept exactly; an f32-subnormal one is truncated
    toward zero to a multiple of 2^-133"""
    m = np.array([3 * 2.0 ** -20, -5 * 2.0 ** -40, 2.0 ** -126, 7 * 2.0 ** -140, -3 * 2.0 ** -135, 2.0 ** -133, 5 * 2.0 ** -133, -2.0 ** -149], np.float32)
    kept = E.split3_kept(m)
    assert list(kept) == [3 * 2.0 ** -20, -5 * 2.0 ** -40, 2.0 ** -126, 0.0, 0.0, 2.0 ** -133, 5 * 2.0 ** -133, 0.0]
    assert E.split3_kept(np.array([27 * 2.0 ** -137], np.float32))[0] == 2.0 ** -133        # 27/16 of 2^-133: its 11/16 are lost
    for t, zone, differs in ((E.Q4_1, "normal", False), (E.Q4_1, "tiny", False), (E.Q5_1, "subnormal", False), (E.Q4_1, "subnormal", True)):
        a, _ = E.zone_exponents(t, zone, RNG, 6, 1)
        raw, w = E.weight_blocks(t, 6, 256, a, RNG)
        assert (not np.array_equal(E.min_piece_ints(t, raw, 256, a), w)) == differs, (t, zone)


def test_representative_table_covers_the_forms_the_suite_knows(table):
    fams = {k[2] for k in table}
    assert set(range(1, 14)) <= fams, sorted(set(range(1, 14)) - fams)
    assert any(k[6] for k in table), "no K3p case refills its scale table inside the K loop"
    assert any(k[7] for k in table) and any(not k[7] for k in table if k[2] in (5, 6)), "partial last range"
    assert any(k[5] & E.MIN_PIECES for k in table) and any(k[5] & E.PERSIST for k in table)
    for t in E.TABLE_TYPES:
        for key in (k for k in table if k[0] == t):
            M, K, N = table[key]
            assert K % 32 == 0 and M >= 1 and N >= 1
