"""BF16 weights as an extension type (include/ggml_hip_ext.h GGML_HIP_TYPE_BF16 = 130).  The checker is tests/np_bf16.py: the one
f32 -> bf16 rule, and the product sum_k bf16(w) * bf16(x) in f64.
CPU tests: the rule on known bit patterns, the sizes, the plan (tree_ids by (K, N) alone, none of them F16's) and Seam 1's refusal.
GPU tests: byte-exact upload / download and row conversion, bit-exact products where every partial sum is exact, the library tolerance
on random data, the ranges F16 cannot hold, shards and the split entry, and F16's error codes wherever F16 is refused."""
import ctypes as C

import numpy as np
import pytest

import np_bf16 as B
import oracle_lib as O
from ggmlsharp_amd import _lib

RNG = np.random.default_rng(130)
BF16, F16 = 130, _lib.F16
F = np.float32
FAM_GEMV, FAM_TILE, FAM_D16 = 11, 10, 12        # plan.h: MMF_DENSE_GEMV, MMF_DENSE, MMF_DENSE16


def _plan(t, M, K, N):
    out = _lib.ggml_hip_mm_plan_t()
    rc = _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(out))
    return rc, out


# special f32 bit patterns: zeros, ones, the two tie directions, the largest finite (rounds up to inf), subnormals and their ties,
# infinities, NaNs with the payload high, low and everywhere
SPECIALS = np.array([0x00000000, 0x80000000, 0x3F800000, 0xBF800000, 0x3F808000, 0x3F818000, 0x3F807FFF, 0x3F808001, 0x7F7FFFFF,
                     0xFF7FFFFF, 0x7F7F7FFF, 0x00000001, 0x00008000, 0x00018000, 0x80018000, 0x007FFFFF, 0x00800000, 0x7F800000,
                     0xFF800000, 0x7F800001, 0xFF800001, 0x7FC00000, 0x7FFFFFFF, 0xFFFFFFFF, 0x7FA00000, 0x7F80FFFF], dtype=np.uint32)


# ---------------------------------------------------------------- CPU
def test_the_conversion_rule_on_known_bit_patterns():
    cases = {0x3F800000: 0x3F80, 0xBF800000: 0xBF80,
             0x3F808000: 0x3F80, 0x3F818000: 0x3F82,           # ties: to the even neighbour, down and up
             0x3F808001: 0x3F81, 0x3F807FFF: 0x3F80,
             0x7F7FFFFF: 0x7F80, 0xFF7FFFFF: 0xFF80,           # the largest finite f32 overflows to +-inf
             0x00008000: 0x0000, 0x00018000: 0x0002,           # subnormal ties, kept (not flushed)
             0x80018000: 0x8002, 0x007FFFFF: 0x0080, 0x00000001: 0x0000,
             0x7F800000: 0x7F80, 0xFF800000: 0xFF80,           # infinities
             0x7F800001: 0x7FC0, 0xFF800001: 0xFFC0,           # NaNs whose payload sits in the low bits stay NaNs (quiet)
             0xFFFFFFFF: 0xFFFF, 0x7FFFFFFF: 0x7FFF, 0x7FC00000: 0x7FC0, 0x7FA00000: 0x7FE0}
    u = np.array(list(cases), dtype=np.uint32)
    got = B.f32_to_bf16_bits(u)
    assert [hex(int(g)) for g in got] == [hex(v) for v in cases.values()]
    # every NaN stays a NaN with its sign; every other value is the nearest bf16 (ties to even)
    r = RNG.integers(0, 2 ** 32, size=200000, dtype=np.uint64).astype(np.uint32)
    b = B.f32_to_bf16_bits(r)
    f = r.view(np.float32)
    back = B.bf16_bits_to_f32(b)
    nan = np.isnan(f)
    assert np.all(np.isnan(back[nan])) and np.array_equal(np.signbit(back[nan]), np.signbit(f[nan]))
    fin = ~nan & np.isfinite(back)
    lo = B.bf16_bits_to_f32(r[fin] >> 16)                                      # truncation, and the next bf16 away from zero
    hi = B.bf16_bits_to_f32((r[fin] >> 16) + 1)
    d_lo, d_hi = np.abs(f[fin].astype(np.float64) - lo), np.abs(hi.astype(np.float64) - f[fin])
    want = np.where(d_lo < d_hi, lo, np.where(d_hi < d_lo, hi, np.where(((r[fin] >> 16) & 1) == 0, lo, hi)))
    assert np.array_equal(back[fin].view(np.uint32), want.view(np.uint32))
    # the widening is exact: bf16 -> f32 -> bf16 is the identity on every non-NaN pattern
    allb = np.arange(65536, dtype=np.uint32).astype(np.uint16)
    keep = ~np.isnan(B.bf16_bits_to_f32(allb))
    assert np.array_equal(B.f32_to_bf16_bits(B.bf16_bits_to_f32(allb[keep])), allb[keep])


def test_type_and_block_size():
    L = _lib.lib()
    assert L.ggml_hip_type_size(BF16) == 2 and L.ggml_hip_blck_size(BF16) == 1
    assert _lib.BF16 == BF16 and _lib.row_bytes(BF16, 11008) == 2 * 11008


def test_the_plan_follows_K_and_N_and_its_trees_are_not_F16s():
    """BF16's family and form are F16's at every shape (its bounds are F16's), its tree_id follows (K, N) alone and is never F16's"""
    f16_trees, bf16_trees = set(), set()
    for K in (64, 510, 512, 1024, 4096, 4100, 11008, 14336):
        for N in (1, 2, 4, 5, 8, 16, 17, 64, 128, 129, 256, 257, 512, 513, 1024, 3000):
            trees = set()
            for M in (1, 100, 300, 1024, 4096, 11008, 32000):
                rcb, pb = _plan(BF16, M, K, N)
                rcf, pf = _plan(F16, M, K, N)
                assert rcb == rcf == 0, (M, K, N, rcb, rcf)
                assert (pb.family, pb.form, pb.image_kind, pb.tile_m, pb.tile_n, pb.ksplit, pb.kstyle, pb.kunit, pb.workgroups, pb.flags) == \
                       (pf.family, pf.form, pf.image_kind, pf.tile_m, pf.tile_n, pf.ksplit, pf.kstyle, pf.kunit, pf.workgroups, pf.flags), (M, K, N)
                assert pb.arith == pf.arith + 50 and pb.tree_id != pf.tree_id
                trees.add(pb.tree_id)
                bf16_trees.add(pb.tree_id)
                f16_trees.add(pf.tree_id)
            assert len(trees) == 1, (K, N)
    assert not (bf16_trees & f16_trees)
    L = _lib.lib()
    for (K, N) in ((4096, 1), (4096, 16), (4096, 600), (1022, 40)):
        assert L.ggml_hip_act_image_kind(BF16, K, N) == L.ggml_hip_act_image_kind(F16, K, N)
        assert L.ggml_hip_mul_mat_work_size(BF16, K, N) == L.ggml_hip_mul_mat_work_size(F16, K, N)


def test_seam_1_refuses_a_bf16_tensor():
    """the reference's enum cannot express the type: Seam 1 refuses it before anything else"""
    L = _lib.lib()
    K, M, N = 64, 8, 2
    w = np.zeros((M, K), np.uint16)
    x = np.zeros((N, K), np.float32)
    d = np.zeros((N, M), np.float32)

    def tensor(t, arr, ne, esz):
        tt = _lib.ggml_tensor()
        tt.type = t
        for i in range(4):
            tt.ne[i] = ne[i] if i < len(ne) else 1
        tt.nb[0] = esz
        tt.nb[1] = esz * ne[0]
        tt.nb[2] = tt.nb[1] * tt.ne[1]
        tt.nb[3] = tt.nb[2]
        tt.data = arr.ctypes.data_as(C.c_void_p)
        return tt

    s0, s1, dst = tensor(BF16, w, (K, M), 2), tensor(_lib.F32, x, (K, N), 4), tensor(_lib.F32, d, (M, N), 4)
    p = _lib.ggml_compute_params(_lib.GGML_TASK_COMPUTE, 0, 1, 0, None)
    assert L.ggml_hip_compute_forward_mul_mat(C.byref(p), C.byref(s0), C.byref(s1), C.byref(dst)) == _lib.ERR_TYPE


# ---------------------------------------------------------------- GPU
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    return device


def _bits(shape, scale=1.0):
    """bf16 bits of N(0, scale) values"""
    return B.f32_to_bf16_bits((RNG.standard_normal(shape) * scale).astype(F))


def _close(got, ref, what, K):
    O.assert_mul_mat_close(got, np.asarray(ref, np.float64), K, what, normwise=1e-5 if np.size(ref) >= 256 else 1e-3)


@gpu
def test_upload_download_is_byte_exact_with_nan_and_inf_payloads(dev):
    import torch
    L = _lib.lib()
    M, K = 70, 520
    rows = RNG.integers(0, 65536, size=(M, K), dtype=np.uint64).astype(np.uint16)     # every bit pattern, NaN payloads included
    rows[0, :6] = [0x7F80, 0xFF80, 0x7FC1, 0xFF81, 0x7F81, 0x0001]
    W = dev.Weight.from_host(BF16, rows, K)
    assert L.ggml_hip_weight_type(W.handle) == BF16 and L.ggml_hip_weight_rows(W.handle) == M and L.ggml_hip_weight_cols(W.handle) == K
    assert np.array_equal(W.download().view(np.uint16).reshape(M, K), rows)
    shard = dev.Weight.from_host(BF16, rows, K, row_begin=11, row_end=40)
    assert np.array_equal(shard.download().view(np.uint16).reshape(29, K), rows[11:40])
    t = torch.from_numpy(rows.view(np.int16)).cuda()
    Wd = dev.Weight.from_device(BF16, t, K)
    assert np.array_equal(Wd.download().view(np.uint16).reshape(M, K), rows)
    Ws = dev.Weight.from_device(BF16, t, K, row_begin=5, row_end=37)
    assert L.ggml_hip_weight_type(Ws.handle) == BF16
    assert np.array_equal(Ws.download().view(np.uint16).reshape(32, K), rows[5:37])
    for w in (W, shard, Wd, Ws):
        w.free()


@gpu
def test_the_device_row_conversion_is_the_rule_and_its_inverse_is_exact(dev):
    import torch
    for (nrows, k) in ((1, len(SPECIALS)), (3, 1001), (64, 4096), (7, 1)):
        r = RNG.integers(0, 2 ** 32, size=(nrows, k), dtype=np.uint64).astype(np.uint32)
        r.reshape(-1)[:len(SPECIALS)] = SPECIALS[:min(len(SPECIALS), r.size)]
        x = torch.from_numpy(r.view(np.int32)).cuda().view(torch.float32)
        got = dev.quantize_rows(BF16, x).cpu().numpy().view(np.uint16).reshape(nrows, k)
        assert np.array_equal(got, B.f32_to_bf16_bits(r)), (nrows, k)
        back = dev.dequantize_rows(BF16, torch.from_numpy(got.view(np.uint8).reshape(-1)).cuda(), k).cpu().numpy()
        assert np.array_equal(back.view(np.uint32).reshape(nrows, k), got.astype(np.uint32) << 16), (nrows, k)


def _mm(dev, W, x, ld1=None, ldd=None):
    """the product through ggml_hip_mul_mat_dev, src1 with row stride ld1, dst with row stride ldd"""
    import torch
    N, K = x.shape
    ld1, ldd = ld1 or K, ldd or W.M
    xs = torch.zeros((N, ld1), dtype=torch.float32, device="cuda")
    xs[:, :K] = torch.from_numpy(np.ascontiguousarray(x)).cuda()
    out = torch.full((N, ldd), -7.0, dtype=torch.float32, device="cuda")
    work = dev.alloc_work(BF16, K, N)
    _lib.check(_lib.lib().ggml_hip_mul_mat_dev(W.handle, C.c_void_p(xs.data_ptr()), N, ld1, C.c_void_p(out.data_ptr()), ldd,
                                               C.c_void_p(work.data_ptr()), work.numel(), dev._stream()), "mul_mat_dev")
    o = out.cpu().numpy()
    assert np.all(o[:, W.M:] == -7.0)
    return o[:, :W.M]


EXACT_N = (1, 4, 5, 16, 17, 128, 129, 512, 513, 1024)


@gpu
@pytest.mark.parametrize("K", [1024, 1022])
def test_exact_tier_every_form_is_the_exact_sum_bit_for_bit(dev, K):
    """small integers: every product and partial sum is exact in f32 whatever the order, so dst is the exact sum in every form the plan
    reaches (K = 1022: K % 4 != 0, the tile fallback)"""
    M = 300
    w = RNG.integers(-8, 9, size=(M, K)).astype(F)
    W = dev.Weight.from_host(BF16, B.f32_to_bf16_bits(w), K)
    fams = set()
    for N in EXACT_N:
        x = RNG.integers(-8, 9, size=(N, K)).astype(F)
        want = (x.astype(np.float64) @ w.T.astype(np.float64)).astype(F)
        got = _mm(dev, W, x)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (K, N)
        fams.add(_plan(BF16, M, K, N)[1].family)
    assert fams == ({FAM_GEMV, FAM_D16} if K % 8 == 0 else {FAM_TILE}), fams
    W.free()


@gpu
def test_random_data_matches_the_restatement_ragged_and_strided(dev):
    for (M, K, N, ld1, ldd) in ((300, 1024, 1, 1024, 300), (77, 2048, 3, 2052, 80), (515, 4096, 16, 4096, 515), (300, 4096, 40, 4100, 333),
                                (257, 1024, 129, 1024, 260), (1000, 2048, 600, 2056, 1000), (130, 520, 33, 524, 131), (96, 1022, 20, 1030, 97)):
        wb = _bits((M, K))
        x = (RNG.standard_normal((N, K)) * 2.0).astype(F)
        W = dev.Weight.from_host(BF16, wb, K)
        _close(_mm(dev, W, x, ld1, ldd), B.mul_mat_bf16(wb, x), f"BF16 {M}x{K}x{N}", K)
        W.free()


@gpu
def test_values_beyond_the_range_of_f16_come_out_right(dev):
    """bf16 holds 1e5 and 1e-6 as normal values: F16 makes the first inf and flushes or rounds away the second; BF16 must not"""
    M, K = 200, 1024
    for N in (1, 16, 600):
        for sw, sx in ((1.0e5, 3.0), (3.0, 1.0e5), (1.0e-6, 1.0e-3), (1.0e-3, 1.0e-6)):
            wb = _bits((M, K), sw)
            x = (RNG.standard_normal((N, K)) * sx).astype(F)
            W = dev.Weight.from_host(BF16, wb, K)
            got = _mm(dev, W, x)
            assert np.all(np.isfinite(got))
            _close(got, B.mul_mat_bf16(wb, x), f"BF16 scales {sw} {sx} N {N}", K)
            W.free()


@gpu
def test_a_row_shard_is_the_bitwise_column_slice_in_every_form(dev):
    import torch
    for (M, K) in ((1024, 4096), (515, 1022)):
        wb = _bits((M, K))
        W = dev.Weight.from_host(BF16, wb, K)
        for N in EXACT_N:
            x = torch.from_numpy((RNG.standard_normal((N, K))).astype(F)).cuda()
            whole = dev.mul_mat(W, x)
            for (r0, r1) in ((0, 256), (256, M), (100, 357), (M - 1, M)):
                Ws = dev.Weight.from_host(BF16, wb, K, row_begin=r0, row_end=r1)
                assert torch.equal(dev.mul_mat(Ws, x), whole[:, r0:r1]), (M, K, N, r0, r1)
                Ws.free()
        W.free()


@gpu
def test_the_split_entry_over_slots_is_bitwise_the_single_slot_result(dev):
    import torch
    L = _lib.lib()
    M, K = 515, 2048
    wb = _bits((M, K))
    for N in (1, 16, 600):
        x = torch.from_numpy((RNG.standard_normal((N, K))).astype(F)).cuda()
        W = dev.Weight.from_host(BF16, wb, K)
        single = dev.mul_mat(W, x).cpu().numpy()
        W.free()
        try:
            for G in (2, 3):
                torch.cuda.synchronize()
                L.ggml_hip_shutdown()
                _lib.check(L.ggml_hip_init_devices(G, (C.c_int * G)(*([0] * G))), "init_devices")
                h = C.c_void_p()
                _lib.check(L.ggml_hip_split_weight_upload(BF16, wb.ctypes.data_as(C.c_void_p), K, M, 2 * K, C.byref(h)), "split upload")
                outs = [torch.full((N, M + 8), -5.0, device="cuda") for _ in range(G)]
                torch.cuda.synchronize()
                xs = (C.c_void_p * G)(*[x.data_ptr()] * G)
                ds = (C.c_void_p * G)(*[o.data_ptr() for o in outs])
                _lib.check(L.ggml_hip_mul_mat_split_dev(h, xs, N, K, ds, M + 8), "split mul_mat")
                _lib.check(L.ggml_hip_sync_slots(), "sync")
                for o in outs:
                    assert np.array_equal(o[:, :M].cpu().numpy().view(np.uint32), single.view(np.uint32)), (G, N)
                    assert torch.all(o[:, M:] == -5.0)
                L.ggml_hip_split_weight_free(h)
        finally:
            torch.cuda.synchronize()
            L.ggml_hip_shutdown()
            dev.init(0)


@gpu
def test_every_entry_treats_bf16_as_it_treats_f16(dev):
    """F16's error code wherever F16 is refused (and acceptance where F16 is accepted): the two-phase COMPUTE, the multi-weight entries,
    the epilogue, push and norm-fused entries, the host row functions and the quantize targets"""
    import torch
    L = _lib.lib()
    st = dev._stream()
    M, K = 200, 1024
    wf = RNG.standard_normal((M, K)).astype(np.float16)
    Wf = dev.Weight.from_host(F16, wf, K)
    Wb = dev.Weight.from_host(BF16, B.f32_to_bf16_bits(wf.astype(F)), K)
    vp = lambda t: C.c_void_p(t.data_ptr())
    for N in (1, 3, 16, 600):
        x = torch.from_numpy(RNG.standard_normal((N, K)).astype(F)).cuda()
        g = torch.from_numpy(RNG.standard_normal((N, K)).astype(F)).cuda()
        work = dev.alloc_work(F16, K, N)
        assert work.numel() == dev.alloc_work(BF16, K, N).numel()

        def rcs(W):
            out, out2 = torch.empty((N, M), device="cuda"), torch.empty((N, M), device="cuda")
            nrm, y = torch.empty((N, K), device="cuda"), torch.empty((N, K), device="cuda")
            add = torch.zeros((N, M), device="cuda")
            hw = (C.c_void_p * 2)(W.handle, W.handle)
            dp = (C.c_void_p * 2)(out.data_ptr(), out2.data_ptr())
            ld = (C.c_int64 * 2)(M, M)
            pp = (C.c_void_p * 1)(out.data_ptr())
            r = [L.ggml_hip_mul_mat_init_dev(W.handle, vp(x), N, K, vp(work), work.numel(), st),
                 L.ggml_hip_mul_mat_compute_dev(W.handle, N, vp(out), M, vp(work), work.numel(), st),
                 L.ggml_hip_mul_mat_epilogue_fused(W.handle, N),
                 L.ggml_hip_mul_mat_epilogue_dev(W.handle, vp(x), N, K, vp(out), M, vp(work), work.numel(), 1, vp(add), M, vp(out2), M,
                                                 C.c_float(1.0), st),
                 L.ggml_hip_mul_mat_epilogue_dev(W.handle, vp(x), N, K, vp(out), M, vp(work), work.numel(), 2, None, 0, None, 0,
                                                 C.c_float(0.5), st),
                 L.ggml_hip_mul_mat_push_fused(W.handle, N, 1),
                 L.ggml_hip_mul_mat_push_dev(W.handle, vp(x), N, K, pp, 1, 0, M, 0, vp(work), work.numel(), st),
                 L.ggml_hip_norm_mul_mat_fused(W.handle, N),
                 L.ggml_hip_norm_mul_mat_dev(W.handle, vp(x), K, vp(g), K, N, vp(nrm), vp(y), vp(out), M, vp(work), work.numel(), 0,
                                             None, 0, None, 0, C.c_float(1.0), st),
                 L.ggml_hip_mul_mat_multi_fused(hw, 2, N),
                 L.ggml_hip_mul_mat_multi_dev(hw, 2, vp(x), K, N, dp, ld, None, 0, None, None, st),
                 L.ggml_hip_mul_mat_multi_work_dev(hw, 2, vp(x), K, N, dp, ld, vp(work), work.numel(), st)]
            torch.cuda.synchronize()
            return r

        rf, rb = rcs(Wf), rcs(Wb)
        assert rf == rb, (N, rf, rb)
        assert rb[1] == _lib.ERR_TYPE                                # the two-phase COMPUTE is for quantized weights
    xr = np.zeros(64, np.float32)
    yr = np.zeros(64, np.uint8)
    for t_call in (lambda t: L.ggml_hip_quantize_row(t, xr.ctypes.data_as(C.c_void_p), yr.ctypes.data_as(C.c_void_p), 32),
                   lambda t: L.ggml_hip_dequantize_row(t, yr.ctypes.data_as(C.c_void_p), xr.ctypes.data_as(C.c_void_p), 32)):
        assert t_call(BF16) == t_call(F16) == _lib.ERR_TYPE
    xd = torch.zeros((2, 64), device="cuda")
    bd = torch.zeros(1024, dtype=torch.uint8, device="cuda")
    assert L.ggml_hip_quantize_rows_src_dev(BF16, 0, vp(xd), 64, 2, 64, vp(bd), st) == \
           L.ggml_hip_quantize_rows_src_dev(F16, 0, vp(xd), 64, 2, 64, vp(bd), st) == _lib.ERR_TYPE
    assert L.ggml_hip_add_q_f32_rows_dev(BF16, vp(bd), vp(xd), 2, 64, vp(bd), st) == \
           L.ggml_hip_add_q_f32_rows_dev(F16, vp(bd), vp(xd), 2, 64, vp(bd), st) == _lib.ERR_TYPE
    Wf.free()
    Wb.free()
