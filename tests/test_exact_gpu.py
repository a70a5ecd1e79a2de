"""The exact tier on the device (-m gpu): inputs whose every scale is a power of two (tests/exact_inputs.py), so that the reference's
f32 result is the exact value whatever the order of its additions -- and every kernel form must return the same BITS, not a value
within SURVEY 8(c)'s tolerance.  Ties (n + 1/2) * 2^b pin the rounding rule of every quantizer the products pass through; near-ties
pin multiply-by-reciprocal; the tiny-normal and subnormal zones pin the scale range.  The shapes are the representative table of
exact_inputs.representatives(), which tests/test_exact_cpu.py holds against the plan's reachable forms."""
import ctypes as C

import numpy as np
import pytest

import exact_inputs as E
import oracle_lib as O

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

RNG = np.random.default_rng(20261015)
FAMILY_NAME = {1: "gemv_fused", 2: "gemv_rows", 3: "k3s_mx", 4: "k3s_i8", 5: "k3p_mx", 6: "k3p_i8", 7: "mx", 8: "f16", 9: "i8",
               10: "dense", 11: "dense_gemv", 12: "dense16", 13: "dense32"}


@pytest.fixture(scope="module")
def dev():
    from ggmlsharp_amd import device
    device.init(0)
    return device


@pytest.fixture(scope="module")
def table():
    return E.representatives()


def _bits_equal(got, want, what):
    g, w = E.f32_bits(got), E.f32_bits(np.asarray(want, np.float32))
    bad = g != w
    if bad.any():
        i = tuple(np.argwhere(bad)[0])
        gv, wv = np.asarray(got, np.float32), np.asarray(want, np.float32)
        raise AssertionError(f"{what}: {int(bad.sum())} of {bad.size} outputs differ from the exact value; first at {i}: "
                             f"got {gv[i]!r} ({g[i]:#010x}), exact {wv[i]!r} ({w[i]:#010x})")


# ---------------------------------------------------------------------------------------------------------- quantizers
@pytest.mark.parametrize("t", E.LEGACY + (E.Q8_1,))
def test_quantize_rows_ties_and_near_ties_bit_exact(dev, t):
    """K8/K9's row quantizers on exact ties (first max wins, the clamp at 15 / 31) and on near-ties: bytes equal the oracle's."""
    for K in (32, 64, 288, 4096):
        a = RNG.integers(-20, 10, 12)
        rows = [E.weight_tie_rows(t, K, a, RNG)]
        rows.append(E.near_tie_rows(4, K, RNG, t)[0])
        for x in rows:
            x = np.ascontiguousarray(x)
            want = O.quantize_row(t, x)
            got = dev.quantize_rows(t, torch.from_numpy(x).cuda()).cpu().numpy()
            assert np.array_equal(got, want), f"type {t} K {K}"
            got2 = dev.quantize_rows_from(t, torch.from_numpy(x).cuda()).cpu().numpy()
            assert np.array_equal(got2, want), f"type {t} K {K} (strided-source entry)"


@pytest.mark.parametrize("t", E.LEGACY)
def test_add_q_f32_ties_bit_exact(dev, t):
    """quantize(dequantize(blocks) + x) with zero blocks (d = 0) and tie or near-tie rows in x: the add node's own quantizer rounds as
    the oracle's."""
    K = 288 if t != E.Q4_2 else 256
    for x in (E.weight_tie_rows(t, K, RNG.integers(-12, 6, 9), RNG), E.near_tie_rows(6, K, RNG, t)[0]):
        x = np.ascontiguousarray(x)
        blocks = O.quantize_row(t, np.zeros_like(x))
        want = O.add_q_f32(t, blocks, x)
        got = dev.add_q_f32_rows(t, torch.from_numpy(blocks).cuda(), torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.array_equal(got, want.reshape(got.shape)), t


@pytest.mark.parametrize("kind", [0, 1, 2, 3, 64])
def test_activation_images_round_ties_half_to_even(dev, kind):
    """K1 (quantize_act_kernel, quantize_act_bf6_kernel): every image kind, on exact-tie rows in every zone and on near-tie rows, holds
    exactly the oracle's Q8_0 quants and scales (decoded as test_quantize_act_planes_match_oracle does); kind 64 (image 0 with the min-term
    piece planes) also the three bf16 pieces of d * sum(q) (as test_min_term_piece_planes_hold_d_times_sum_exactly reads them)."""
    from ggmlsharp_amd._lib import lib, check
    from test_gpu_parity import _decode_act_image, _split3_bf16
    K = 288
    for N in (9, 130):
        b = np.concatenate([RNG.integers(-10, 6, N // 3), RNG.integers(-120, -100, N // 3), RNG.integers(60, 100, N - 2 * (N // 3))])
        x, q_exact, d_exact, _ = E.act_rows(N, K, b, RNG, 1)
        xn, _ = E.near_tie_rows(N, K, RNG)
        for rows, exact in ((x, True), (xn, False)):
            rows = np.ascontiguousarray(rows)
            ref = O.quantize_row(O.Q8_0, rows).reshape(N, K // 32, 36)
            ref_d = ref[:, :, :4].copy().view(np.float32).reshape(N, K // 32)
            ref_q = ref[:, :, 4:].copy().view(np.int8).astype(np.int32)
            if exact:                                  # (the construction's own quants: the oracle rounds half to even)
                assert np.array_equal(ref_q.reshape(N, K), q_exact) and np.array_equal(ref_d, d_exact)
            work = dev.alloc_work(O.Q8_0, K, N)
            work.fill_(0x7F)
            xd = torch.from_numpy(rows).cuda()
            check(lib().ggml_hip_quantize_act_dev(C.c_void_p(xd.data_ptr()), N, K, K, C.c_void_p(work.data_ptr()), work.numel(), kind, None),
                  "quantize_act")
            torch.cuda.synchronize()
            raw = work.cpu().numpy()
            nbk, Npad = K // 32, (N + 255) // 256 * 256
            nba = (nbk + 3) // 4 * 4
            img = nba * 4 * Npad * 16
            ad = raw[img: img + nba * Npad * 4].view(np.float32).reshape(nba, Npad)
            assert np.array_equal(ad[:nbk, :N].T.view(np.uint32), ref_d.view(np.uint32)), (kind, N, exact)
            q = _decode_act_image(kind & 3, raw, nba, Npad, N)
            assert np.array_equal(q[:, :nbk], ref_q), (kind, N, exact, int((q[:, :nbk] != ref_q).sum()))
            if kind == 64:
                nkg = (nbk + 7) // 8
                sv = np.zeros((N, (nkg + (nkg & 1)) * 8), dtype=np.float32)
                sv[:, :nbk] = ref_d * ref_q.sum(axis=2).astype(np.float32)
                base = nba * 2 * Npad * 16
                planes = raw[base: base + (nkg + (nkg & 1)) * 3 * Npad * 16].view(np.uint16).reshape(-1, 3, Npad, 8)
                for pc, wp in enumerate(_split3_bf16(sv)):
                    assert np.array_equal(planes[:, pc, :N, :].transpose(1, 0, 2).reshape(N, -1), wp), (N, exact, pc)


# ---------------------------------------------------------------------------------------------------------- products
def _zone_case(t, zone, M, K, N):
    """(raw weight, w ints, a, x f32, activation ints, b) for a quantized type, or dense values of at most 8 significant bits"""
    if t in E.DENSE:
        R = int(min(127, np.sqrt((E.EXACT_BOUND - 1) / K)))
        a, b = RNG.integers(-6, 3, M), RNG.integers(-6, 3, N)
        w, q = RNG.integers(-R, R + 1, (M, K)), RNG.integers(-R, R + 1, (N, K))
        wv = np.ldexp(w.astype(np.float64), a[:, None])
        raw = wv.astype(np.float32) if t == E.F32 else wv.astype(np.float16).view(np.uint16)
        x = np.ldexp(q.astype(np.float64), b[:, None]).astype(np.float32)
        return raw, w, a, x, q, b
    a, b = E.zone_exponents(t, zone, RNG, M, N)
    j = E.jitter_for(t, K)                              # (per-block exponents where the 2^24 bound leaves room)
    raw, w = E.weight_blocks(t, M, K, a, RNG, jitter=j)
    x, q, d, _ = E.act_rows(N, K, b, RNG, E.wmax(t) << j, jitter=j)
    return raw, w, a, x, E.act_ints(q, d, b), b


def _exact_on_device(w, a, q, b):
    """exact_product as a float64 torch matmul (exact: every sum stays within 53 bits)"""
    wt = torch.from_numpy(w.astype(np.float64)).cuda()
    qt = torch.from_numpy(q.astype(np.float64)).cuda()
    S = (qt @ wt.T).cpu().numpy()
    return np.ldexp(S, (b[:, None] + a[None, :]).astype(np.int64))


@pytest.mark.parametrize("t,zone", [(t, z) for t in E.TABLE_TYPES for z in E.ZONES if t not in E.DENSE or z == "normal"])   # (dense: normal only)
def test_every_representative_is_bitwise_the_exact_product(dev, table, t, zone):
    """each (M, K, N) of the table for type t, under its force: the plan's family and form first, then the one-call entry, the two-step
    INIT + COMPUTE, up to 4 rows the multi-weight mat-vec entry, and the multi-weight batch entry -- each bit for bit the exact product (a -0.0 is a difference)."""
    from ggmlsharp_amd._lib import lib, check, ggml_hip_mm_plan_t
    L = lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    keys = sorted(k for k in table if k[0] == t)
    assert keys
    cases = {}
    n_fused = 0
    p = ggml_hip_mm_plan_t()
    try:
        for key in keys:
            force = key[1]
            M, K, N = table[key]
            L.ggml_hip_debug_force_gemm(force)
            assert L.ggml_hip_mm_plan(t, M, K, N, C.byref(p)) == 0
            assert E.plan_key(t, force, K, p) == key, (key, (M, K, N))
            if (M, K, N) not in cases:                    # (one case per shape: the forces of a shape share it)
                raw, w, a, x, q, b = _zone_case(t, zone, M, K, N)
                E.assert_exactly_representable(w, q, a, b)
                want = _exact_on_device(w, a, q, b)
                pieces = want
                if t in E.MIN_TYPES:                      # what the min-piece forms compute: split3 of m (parity: the stated deviation)
                    wp = E.min_piece_ints(t, raw, K, a)
                    E.assert_exactly_representable(wp, q, a, b)
                    pieces = _exact_on_device(wp, a, q, b)
                cases[(M, K, N)] = (raw, x, want, pieces)
            raw, x, want, pieces = cases[(M, K, N)]
            if p.flags & E.MIN_PIECES:
                want = pieces                             # (equal to the exact product unless m is an f32 subnormal: Q4_1 only)
            what = f"type {t} {zone} M{M} K{K} N{N} force {force} {FAMILY_NAME.get(p.family)} form {p.form} image {p.image_kind}"
            W = dev.Weight.from_host(t, raw, K)           # (while the force is in effect: force 3 builds the MX digit planes)
            xd = torch.from_numpy(x).cuda()
            _bits_equal(dev.mul_mat(W, xd).cpu().numpy(), want, what + " one call")
            if p.flags & 16 and t not in E.DENSE:         # NEEDS_WORK: the quantized two-step form exists
                work = dev.alloc_work(t, K, N)
                two = torch.empty((N, M), dtype=torch.float32, device="cuda")
                dev.mul_mat_init(W, xd, work)
                dev.mul_mat_compute(W, N, two, work)
                _bits_equal(two.cpu().numpy(), want, what + " init + compute")
            if t not in E.DENSE:
                hw = (C.c_void_p * 2)(W.handle, W.handle)
                dp_ld = lambda outs: ((C.c_void_p * 2)(*[o.data_ptr() for o in outs]), (C.c_int64 * 2)(M, M))
                if N <= 4:                                # the one-launch multi-weight mat-vec (N <= 4), where the library has the form
                    fused = L.ggml_hip_mul_mat_multi_fused(hw, 2, N) == 1
                    n_fused += fused
                    outs = [torch.full((N, M), 3.0, device="cuda") for _ in range(2)]
                    check(L.ggml_hip_mul_mat_multi_dev(hw, 2, C.c_void_p(xd.data_ptr()), K, N, *dp_ld(outs), None, 0, None, None, st), "multi")
                    for o in outs:
                        _bits_equal(o.cpu().numpy(), want, what + (" multi-weight, one launch" if fused else " multi-weight, per matrix"))
                # the batch form with one shared quantization of src1 (one launch at 5..64 rows, Q4_0 / Q4_1, K >= 2048)
                outs = [torch.full((N, M), 3.0, device="cuda") for _ in range(2)]
                work = dev.alloc_work(t, K, N)
                check(L.ggml_hip_mul_mat_multi_work_dev(hw, 2, C.c_void_p(xd.data_ptr()), K, N, *dp_ld(outs), C.c_void_p(work.data_ptr()), work.numel(), st),
                      "multi with work")
                for o in outs:
                    _bits_equal(o.cpu().numpy(), want, what + " multi-weight with work")
            W.free()
    finally:
        L.ggml_hip_debug_force_gemm(0)
    if t in (E.Q4_0, E.Q5_1, E.Q8_0):                     # (types test_fused.py runs through the one-launch form)
        assert n_fused > 0, "no representative reached the one-launch multi-weight form"
