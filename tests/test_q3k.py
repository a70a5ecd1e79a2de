"""Q3_K as an UNPINNED EXTRA (include/ggml_hip_ext.h GGML_HIP_TYPE_Q3_K; ggmlsharp_amd/csrc/kquants.hip).  The checker is
tests/np_q3k.py, a numpy restatement of the published upstream format.  A Q3_K super-block transcodes exactly to a Q6_K one, and the
library keeps Q3_K in Q6_K's resident form byte for byte: the products of the two weights must be the same bits in every kernel family.
CPU tests: the restatement by hand and its round trips, the sizes and the plan.  GPU tests: the device path against the restatement and
against Q6_K."""
import ctypes as C

import numpy as np
import pytest

import np_kquants as KQ
import np_q3k as Q3
import oracle_lib as O
from ggmlsharp_amd import _lib

RNG = np.random.default_rng(3113)
Q3_K, Q4_K, Q5_K, Q6_K = 111, 112, 113, 114
F = np.float32


def _rand(shape, scale=1.0):
    return (RNG.standard_normal(shape) * scale).astype(np.float32)


def _random_blocks(nb):
    """raw super-blocks: every bit pattern of hmask, qs and scales; d a small finite half"""
    b = RNG.integers(0, 256, size=(nb, Q3.Q3K_BYTES), dtype=np.uint8)
    b[:, 108:110] = (RNG.random(nb).astype(np.float32) * 0.002 + 0.0001).astype(np.float16).reshape(-1, 1).view(np.uint8)
    return b


def _plan(t, M, K, N):
    out = _lib.ggml_hip_mm_plan_t()
    rc = _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(out))
    return rc, out


# ---------------------------------------------------------------- CPU: the restatement itself
def test_a_hand_built_super_block_decodes_to_the_values_worked_out_by_hand():
    # literal elements, worked out from the format's text
    b = np.zeros((1, 110), dtype=np.uint8)
    b[0, 5] = 0b01000010                  # hmask[5]: bit 1 -> element 32 + 5 = 37, bit 6 -> element 128 + 64 + 5 = 197
    b[0, 32 + 32 + 5] = 0xE4              # qs[32 n + l], n = 1, l = 5: bit pairs 0, 1, 2, 3 for s = 0..3 -> elements 133, 165, 197, 229
    b[0, 96 + 4] = 0xB0                   # scale 12: low nibble in the high half of scales[4] ...
    b[0, 96 + 8] = 0x80                   # ... high bits 6, 7 of scales[8]: code 0x2B = 43, sc = 11
    b[0, 96 + 6] = 0x50                   # scale 14: code 5, sc = -27
    b[0, 96 + 2] = 0x0F                   # scale 2: low nibble of scales[2] ...
    b[0, 96 + 10] = 0x03                  # ... bits 0, 1 of scales[10]: code 63, sc = 31
    b[0, 108:110] = np.array([0.5], np.float16).view(np.uint8)
    v = Q3.q3_values(b)[0]
    assert (v[37], v[133], v[165], v[197], v[229]) == (0, -4, -3, 2, -1)
    assert (v == -4).sum() == 256 - 4    # everything else: q2 = 0, hbit = 0
    sc = Q3.q3_scales(b)[0]
    assert (sc[2], sc[12], sc[14], sc[0], sc[8]) == (31, 11, -27, -32, -32)
    y = Q3.dequantize_q3_K(b)[0]
    assert y[197] == 11.0 and y[229] == 13.5 and y[37] == 0.0 and y[32] == -62.0
    assert y[133] == 64.0 and y[165] == 48.0 and y[0] == 64.0
    # a patterned block: every hmask bit, every bit pair of qs and every scale code position set and clear somewhere;
    # each element decoded in scalar Python straight from the format's text
    b = np.zeros((1, 110), dtype=np.uint8)
    b[0, 0:32] = [(0x5A ^ (29 * l)) & 0xFF for l in range(32)]
    b[0, 32:96] = [(71 * i + 13) & 0xFF for i in range(64)]
    b[0, 96:108] = [0x00, 0xFF, 0x3C, 0xA5, 0x0F, 0xF0, 0x96, 0x69, 0x1B, 0xE4, 0x72, 0x8D]
    b[0, 108:110] = np.array([0.375], np.float16).view(np.uint8)
    hm, qs, scb = [int(c) for c in b[0, 0:32]], [int(c) for c in b[0, 32:96]], [int(c) for c in b[0, 96:108]]
    codes = []
    for j in range(16):
        low = scb[j] & 15 if j < 8 else scb[j - 8] >> 4
        codes.append(low | (((scb[8 + j % 4] >> (2 * (j // 4))) & 3) << 4))
    assert sorted(set(c >> 4 for c in codes)) == [0, 1, 2, 3] and len(set(codes)) > 8
    want = np.empty(256, dtype=np.float32)
    seen_h = set()
    for e in range(256):
        n, s, l = e // 128, (e % 128) // 32, e % 32
        q2 = (qs[32 * n + l] >> (2 * s)) & 3
        hbit = (hm[l] >> (4 * n + s)) & 1
        seen_h.add((4 * n + s, hbit))
        want[e] = F(F(0.375) * F(codes[e // 16] - 32)) * F(q2 + 4 * hbit - 4)
    assert len(seen_h) == 16                                                 # every hmask bit position seen set and clear
    assert np.array_equal(Q3.dequantize_q3_K(b)[0].view(np.uint32), want.view(np.uint32))


def test_pack_unpack_round_trips_and_the_exact_transcoder_to_Q6_K():
    b = _random_blocks(300)
    v = Q3.q3_values(b)
    assert v.min() == -4 and v.max() == 3
    codes = Q3.q3_scale_codes(b[:, 96:108])
    repacked = Q3.pack_q3_K(v + 4, codes, b[:, 108:110].copy().view(np.float16).reshape(-1))
    assert np.array_equal(repacked, b)                                       # pack(unpack(bytes)) == bytes
    assert np.array_equal(Q3.pack_scale_codes(codes), b[:, 96:108])
    q6 = Q3.transcode_to_q6_K(b)
    assert np.array_equal(KQ.q6_values(q6), v)
    y3, y6 = Q3.dequantize_q3_K(b), KQ.dequantize_q6_K(q6)
    assert np.array_equal(y3.view(np.uint32), y6.view(np.uint32))            # the same weights, bit for bit
    w = Q3.quantize_q3_K(_rand((8, 256))).reshape(2, -1)
    x = _rand((3, 1024))
    assert np.array_equal(Q3.mul_mat_q3_K(w, x), KQ.mul_mat_q6_K(Q3.transcode_to_q6_K(w).reshape(2, -1), x))


def test_the_reference_quantizer_is_valid_and_its_refinement_helps():
    x = _rand((200, 256), 2.0)
    b = Q3.quantize_q3_K(x)
    assert b.shape == (200, 110)
    v, sc = Q3.q3_values(b), Q3.q3_scales(b)
    assert v.min() >= -4 and v.max() <= 3 and sc.min() >= -32 and sc.max() <= 31
    assert (np.abs(sc).max(axis=1) == 32).all()                             # the scale of largest magnitude is the one that maps to -32
    y = Q3.dequantize_q3_K(b)
    assert np.abs(y - x).max() <= 0.5 * np.abs(x).max()                      # three bits: a coarse but sane code
    assert Q3.weighted_error(x, b) <= Q3.weighted_error(x, Q3.quantize_q3_K(x, passes=0))
    # an all-zero super-block is 110 zero bytes
    assert not Q3.quantize_q3_K(np.zeros((1, 256), np.float32)).any()


def test_the_reference_quantizer_on_ties_signs_and_a_scale_that_rounds_to_zero():
    # step 1 without refinement: iscale = -4 / max with max the FIRST element of largest magnitude; nearest = half to even
    x = np.zeros((2, 16), np.float32)
    x[0, :7] = [-4.0, 0.5, 1.5, 2.5, -3.5, 4.0, -0.5]                        # -4 comes first: iscale = 1
    x[1, :3] = [4.0, -4.0, 2.5]                                              # +4 comes first: iscale = -1
    scale, L = Q3.make_q3_quants(x, passes=0)
    assert list(L[0, :7] - 4) == [-4, 0, 2, 2, -4, 3, 0]                     # 0.5 -> 0, 1.5 -> 2, 2.5 -> 2, -3.5 -> -4, 4 -> 3 (clamped), -0.5 -> 0
    assert list(L[1, :3] - 4) == [-4, 3, -2]                                 # -4 (the max), 4 -> clamped to 3, -2.5 -> -2
    assert (L[0, 7:] == 4).all() and (L[1, 3:] == 4).all()                  # zeros code 0 (stored + 4)
    scale0, L0 = Q3.make_q3_quants(np.zeros((1, 16), np.float32))
    assert scale0[0] == 0 and not L0.any()                                   # an all-zero sub-block: L = 0, not 4
    # one sub-block far smaller than the rest: its 6-bit scale code rounds to 32 (sc = 0), so the codes of step 1 stay
    x = _rand((1, 256), 50.0)
    x[0, 48:64] = _rand(16, 1e-3)
    b = Q3.quantize_q3_K(x)
    assert Q3.q3_scale_codes(b[:, 96:108])[0, 3] == 32
    _, L3 = Q3.make_q3_quants(x[:, 48:64])
    assert np.array_equal(Q3.q3_values(b)[0, 48:64] + 4, L3[0])
    # equal magnitudes of opposite sign in one sub-block: the first maps to -4, so it decides the sign of the sub-block's scale
    x = np.zeros((1, 256), np.float32)
    x[0, 0], x[0, 1], x[0, 16], x[0, 17] = 3.0, -3.0, -3.0, 3.0
    b = Q3.quantize_q3_K(x)
    ds = Q3.q3_d(b)[0] * Q3.q3_scales(b)[0].astype(F)
    assert ds[0] < 0 < ds[1] and not ds[2:].any()
    y = Q3.dequantize_q3_K(b)[0]
    assert y[0] > 0 > y[1] and y[16] < 0 < y[17]


def test_type_and_block_size():
    L = _lib.lib()
    assert L.ggml_hip_type_size(Q3_K) == 110 and L.ggml_hip_blck_size(Q3_K) == 256
    assert _lib.Q3_K == Q3_K and _lib.row_bytes(Q3_K, 11008) == 43 * 110 and _lib.row_bytes(Q6_K, 4096) == 16 * 210


def test_the_plan_of_Q3_K_is_the_plan_of_Q6_K():
    """the plan keys on (resident type Q4_2, a k-quant ext_type): Q3_K must get Q6_K's kernels, field for field"""
    fields = [f[0] for f in _lib.ggml_hip_mm_plan_t._fields_]
    for M in (1, 100, 1024, 4096, 16384, 32000):
        for K in (256, 2048, 4096, 11008, 14336, 36864):
            if K % 256:
                continue
            for N in (1, 2, 4, 5, 8, 9, 16, 32, 33, 64, 128, 256, 257, 512, 1024, 3000):
                rc3, p3 = _plan(Q3_K, M, K, N)
                rc6, p6 = _plan(Q6_K, M, K, N)
                assert rc3 == rc6 == 0, (M, K, N, rc3, rc6)
                assert [getattr(p3, f) for f in fields] == [getattr(p6, f) for f in fields], (M, K, N)
    assert _plan(Q3_K, 4096, 4096 + 32, 16)[0] == _lib.ERR_SHAPE                          # K % 256
    assert _plan(Q3_K, 4096, 11008 - 256 + 128, 1)[0] == _lib.ERR_SHAPE


# ---------------------------------------------------------------- GPU: the device path
gpu = pytest.mark.gpu


@pytest.fixture(scope="module")
def dev():
    pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    return device


def _close(got, ref, what, K):
    ref = np.asarray(ref, np.float64)
    O.assert_mul_mat_close(got, ref, K, what, normwise=1e-5 if ref.size >= 256 else 1e-3)   # THE mul_mat tolerance (tests/oracle_lib.py)


@gpu
def test_dequantize_is_bit_exact(dev):
    import torch
    for nb in (1, 7, 64):
        for b in (_random_blocks(nb), Q3.quantize_q3_K(_rand((nb, 256), 3.0))):
            want = Q3.dequantize_q3_K(b)
            got = dev.dequantize_rows(Q3_K, torch.from_numpy(b.reshape(1, -1)).cuda(), nb * 256).cpu().numpy().reshape(-1, 256)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), nb


@gpu
def test_device_quantizer_writes_the_restated_reference_quantizers_bytes(dev):
    import torch
    for (nrows, K, scale) in ((1, 256, 1.0), (7, 768, 3.0), (33, 2048, 0.01), (5, 11008, 40.0),
                              (1, 256, 3.0), (7, 768, 0.01), (33, 2048, 40.0), (5, 11008, 1.0)):
        x = _rand((nrows, K), scale)
        x[0, :256] = 0.0                                      # a zero super-block
        if nrows > 1:
            x[1] = np.abs(x[1])                               # a non-negative row
            x[-1, 32:64] = -1.5                               # two constant sub-blocks
            x[-1, 300 % K] = 1000.0 * scale                   # one outlier
            x[-1, 260 % K] = -x[-1, 270 % K]                  # equal magnitudes of opposite sign in one sub-block
            x[-1, 272 % K] = 0.25 * scale                     # ... and a sub-block with a tie for its largest magnitude
            x[-1, 273 % K] = -0.25 * scale
            x[-1, 512 % K:512 % K + 16] *= 1e-5                 # a sub-block whose 6-bit scale code rounds to 32: its first codes stay
        want = Q3.quantize_q3_K(x.reshape(-1, 256)).reshape(nrows, -1)
        got = dev.quantize_rows(Q3_K, torch.from_numpy(x).cuda()).cpu().numpy()
        assert got.shape == want.shape
        bad = np.nonzero((got != want).reshape(-1, 110).any(axis=1))[0]
        assert bad.size == 0, f"{nrows}x{K} scale {scale}: super-blocks {bad[:8]} differ"


@gpu
def test_upload_download_is_byte_exact_and_the_type_reported(dev):
    import torch
    from ggmlsharp_amd._lib import lib
    M, K = 70, 768
    rows = _random_blocks(M * K // 256).reshape(M, -1)
    W = dev.Weight.from_host(Q3_K, rows, K)
    assert lib().ggml_hip_weight_type(W.handle) == Q3_K and lib().ggml_hip_weight_rows(W.handle) == M
    assert np.array_equal(W.download().reshape(M, -1), rows)
    shard = dev.Weight.from_host(Q3_K, rows, K, row_begin=11, row_end=40)
    assert np.array_equal(shard.download().reshape(29, -1), rows[11:40])
    h = C.c_void_p()
    assert lib().ggml_hip_weight_upload(Q3_K, rows.ctypes.data_as(C.c_void_p), 700, M, 330, 0, M, None, C.byref(h)) == -3   # K % 256
    # from the device quantizer's output, on the device
    x = _rand((64, 1024))
    q = dev.quantize_rows(Q3_K, torch.from_numpy(x).cuda())
    Wd = dev.Weight.from_device(Q3_K, q, 1024)
    assert np.array_equal(Wd.download().reshape(64, -1), q.cpu().numpy())
    a = _rand((20, 1024))
    got = dev.mul_mat(Wd, torch.from_numpy(a).cuda()).cpu().numpy()
    _close(got, Q3.mul_mat_q3_K(q.cpu().numpy(), a), "Q3_K from the device quantizer", 1024)
    for w in (W, shard, Wd):
        w.free()


# every kernel family the plan picks for Q6_K: 1 the fused mat-vec, 4 K3s (K3s-16 on short matrices), 9 the staged int8 form, 6 K3p
FAMILY_SHAPES = [(300, 1024, 1, 1), (515, 4096, 3, 1), (300, 4096, 4, 1),
                 (300, 2048, 5, 4), (300, 2048, 16, 4), (1024, 4096, 40, 4), (4096, 4096, 64, 4),
                 (515, 768, 8, 9), (300, 1024, 100, 9), (130, 512, 600, 9),
                 (300, 2048, 1100, 6), (4096, 4096, 257, 6), (16384, 2048, 33, 6)]


@gpu
@pytest.mark.parametrize("M,K,N,family", FAMILY_SHAPES)
def test_the_product_is_bitwise_the_product_of_the_transcoded_Q6_K_weight(dev, M, K, N, family):
    """the converter puts every byte where the kernels expect it: a Q3_K weight and the Q6_K weight of its transcoded bytes give the same bits"""
    import torch
    assert _plan(Q6_K, M, K, N)[1].family == family and _plan(Q3_K, M, K, N)[1].family == family
    rows = _random_blocks(M * K // 256)
    rows[::3] = Q3.quantize_q3_K(_rand((rows[::3].shape[0], 256)))
    W3 = dev.Weight.from_host(Q3_K, rows.reshape(M, -1), K)
    W6 = dev.Weight.from_host(Q6_K, Q3.transcode_to_q6_K(rows).reshape(M, -1), K)
    x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
    assert torch.equal(dev.mul_mat(W3, x), dev.mul_mat(W6, x)), (M, K, N)
    W3.free()
    W6.free()


@gpu
def test_mul_mat_matches_the_restatement(dev):
    """the shape list of test_kquants.py::test_mul_mat_q5_K_matches_the_restatement, raw and quantized weights"""
    import torch
    for (M, K, N) in ((96, 256, 1), (300, 1024, 3), (128, 512, 8), (515, 768, 40), (256, 2048, 130), (640, 1024, 300),
                      (130, 512, 600), (257, 768, 1100), (200, 2048, 300), (130, 4352, 512), (200, 2048, 1100), (130, 2304, 2500),
                      (300, 2048, 33), (130, 4352, 64), (515, 2304, 9), (130, 11008, 100), (96, 2048, 250)):
        for raw in (False, True):
            rows = _random_blocks(M * K // 256) if raw else Q3.quantize_q3_K(_rand((M * K // 256, 256)))
            rows = rows.reshape(M, -1)
            x = _rand((N, K))
            W = dev.Weight.from_host(Q3_K, rows, K)
            got = dev.mul_mat(W, torch.from_numpy(x).cuda()).cpu().numpy()
            _close(got, Q3.mul_mat_q3_K(rows, x), f"Q3_K {M}x{K}x{N} raw={raw}", K)
            W.free()


@gpu
def test_mul_mat_at_4096_x_11008_x_512_on_a_sample(dev):
    import torch
    M, K, N = 4096, 11008, 512
    rs = np.random.default_rng(31113)
    rows = _random_blocks(M * K // 256).reshape(M, -1)
    ms = np.sort(rs.choice(M, size=64, replace=False))
    ns = np.sort(rs.choice(N, size=64, replace=False))
    rows[ms[::2]] = Q3.quantize_q3_K(_rand((32 * K // 256, 256))).reshape(32, -1)
    x = _rand((N, K))
    W = dev.Weight.from_host(Q3_K, rows, K)
    got = dev.mul_mat(W, torch.from_numpy(x).cuda())
    _close(got.cpu().numpy()[np.ix_(ns, ms)], Q3.mul_mat_q3_K(rows[ms], x[ns]), f"Q3_K {M}x{K}x{N} (64 x 64 sample)", K)
    W.free()


@gpu
def test_fused_mat_vec_with_the_Q8_K_rule_equals_the_two_step_form_bitwise(dev):
    import torch
    for (M, K, N) in ((100, 256, 1), (515, 4096, 2), (300, 4096, 4), (130, 11008, 1), (130, 11008, 4), (4096, 4096, 1)):
        rows = Q3.quantize_q3_K(_rand((M * K // 256, 256))).reshape(M, -1)
        x = _rand((N, K), 2.0)
        x[0, 256:512] = 0.0
        if K >= 1024:
            x[0, 700] = -x[0, 900]
        assert _plan(Q3_K, M, K, N)[1].family == 1
        W = dev.Weight.from_host(Q3_K, rows, K)
        xd = torch.from_numpy(x).cuda()
        one = dev.mul_mat(W, xd)
        work = dev.alloc_work(Q3_K, K, N)
        dev.mul_mat_init(W, xd, work)
        two = torch.empty_like(one)
        dev.mul_mat_compute(W, N, two, work)
        assert torch.equal(one, two), (M, K, N)
        _close(one.cpu().numpy(), Q3.mul_mat_q3_K(rows, x), f"Q3_K fused mat-vec {M}x{K}x{N}", K)
        W.free()


@gpu
@pytest.mark.parametrize("M,K,N,family", [(300, 4096, 2, 1), (300, 2048, 40, 4), (300, 2048, 1100, 6)])
def test_a_row_shard_is_the_bitwise_column_slice_of_the_whole(dev, M, K, N, family):
    import torch
    rows = Q3.quantize_q3_K(_rand((M * K // 256, 256))).reshape(M, -1)
    xd = torch.from_numpy(_rand((N, K))).cuda()
    assert _plan(Q3_K, M, K, N)[1].family == family and _plan(Q3_K, 160, K, N)[1].family == family
    whole = dev.mul_mat(dev.Weight.from_host(Q3_K, rows, K), xd)
    part = dev.mul_mat(dev.Weight.from_host(Q3_K, rows, K, row_begin=100, row_end=260), xd)
    assert torch.equal(part, whole[:, 100:260])


@gpu
@pytest.mark.parametrize("t", [Q3_K, Q4_K, Q5_K, Q6_K])
def test_K3p_on_a_tall_matrix_equals_its_K3s_shards_bitwise(dev, t):
    """M = 16384 is planned onto K3p, its 1024-row shards onto K3s: the k-quant extras keep the bitwise shard promise across that switch"""
    import torch
    M, K, N, S = 16384, 4096, 40, 1024
    assert _plan(t, M, K, N)[1].family == 6 and _plan(t, S, K, N)[1].family == 4
    g = torch.Generator(device="cuda")
    g.manual_seed(t)
    rows = dev.quantize_rows(t, torch.randn((M, K), generator=g, device="cuda"))
    xd = torch.randn((N, K), generator=g, device="cuda")
    W = dev.Weight.from_device(t, rows, K)
    whole = dev.mul_mat(W, xd)
    W.free()
    for r0 in range(0, M, S):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r0 + S)
        assert torch.equal(dev.mul_mat(Ws, xd), whole[:, r0:r0 + S]), (t, r0)
        Ws.free()


@gpu
def test_multi_work_and_push_entries_are_bitwise_the_single_calls(dev):
    import torch
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = 2048
    for (Ms, N) in (((300, 200), 3), ((300, 200, 130), 16), ((300, 200, 130, 77), 40), ((1024, 515, 300, 96), 600)):
        Ws = [dev.Weight.from_host(Q3_K, Q3.quantize_q3_K(_rand((M * K // 256, 256))).reshape(M, -1), K) for M in Ms]
        x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
        singles = [dev.mul_mat(w, x) for w in Ws]
        hw = (C.c_void_p * len(Ws))(*[w.handle for w in Ws])
        outs = [torch.full((N, M + 4), -2.0, device="cuda") for M in Ms]
        dp = (C.c_void_p * len(Ws))(*[o.data_ptr() for o in outs])
        ld = (C.c_int64 * len(Ws))(*[M + 4 for M in Ms])
        work = dev.alloc_work(Q3_K, K, N)
        _lib.check(L.ggml_hip_mul_mat_multi_work_dev(hw, len(Ws), C.c_void_p(x.data_ptr()), K, N, dp, ld, C.c_void_p(work.data_ptr()),
                                                     work.numel(), st), "multi with work")
        for o, s, M in zip(outs, singles, Ms):
            assert torch.equal(o[:, :M], s) and torch.all(o[:, M:] == -2.0), (Ms, N)
        # the push entry with this device as its only peer: its own buffer gets the product
        for w, s in zip(Ws, singles):
            dst = torch.full((N, w.M), -3.0, device="cuda")
            pp = (C.c_void_p * 1)(dst.data_ptr())
            _lib.check(L.ggml_hip_mul_mat_push_dev(w.handle, C.c_void_p(x.data_ptr()), N, K, pp, 1, 0, w.M, 0, C.c_void_p(work.data_ptr()),
                                                   work.numel(), st), "push")
            assert torch.equal(dst, s), (w.M, N)
        for w in Ws:
            w.free()
