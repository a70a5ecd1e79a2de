"""IQ4_NL and IQ4_XS as UNPINNED EXTRAS (include/ggml_hip_ext.h GGML_HIP_TYPE_IQ4_NL / _IQ4_XS; ggmlsharp_amd/csrc/iq4.hip).  The checker
is tests/np_iq4.py, a numpy restatement of the published upstream formats and quantizer.  An IQ4_NL block transcodes exactly to a Q8_0
block and the library keeps it as a plain Q8_0 weight: its product must be the bits of the transcoded Q8_0 weight's in every family.  An
IQ4_XS super-block lives in Q6_K's resident form: restricted to codebook values in -32..31 it has a Q6_K twin with the same bits.
CPU tests: the restatement by hand and its round trips, the sizes, the plan, Seam 1's refusal.  GPU tests: the device path against the
restatement, against Q8_0 and against Q6_K."""
import ctypes as C

import numpy as np
import pytest

import np_iq4 as I
import np_kquants as KQ
import np_restatement as R
import oracle_lib as O
from ggmlsharp_amd import _lib

RNG = np.random.default_rng(1203)
IQ4_NL, IQ4_XS = 120, 123
Q8_0, Q6_K = 8, 114
F = np.float32


def _rand(shape, scale=1.0):
    return (RNG.standard_normal(shape) * scale).astype(np.float32)


def _nl_blocks(nb, lo=0, hi=16):
    """raw IQ4_NL blocks: indices in lo..hi-1, d a small finite half"""
    idx = RNG.integers(lo, hi, size=(nb, 32))
    d = (RNG.random(nb).astype(np.float32) * 0.002 + 0.0001) * RNG.choice([-1, 1], nb)
    return I.pack_iq4_nl(idx, d.astype(np.float16))


def _xs_blocks(nb, lo=0, hi=16):
    """raw IQ4_XS super-blocks: indices in lo..hi-1, every scale code 0..63, d a small finite half"""
    idx = RNG.integers(lo, hi, size=(nb, 8, 32))
    codes = RNG.integers(0, 64, size=(nb, 8))
    codes[:, 0], codes[:, 7] = 0, 63                                         # both extremes of the scale codes in every super-block
    d = (RNG.random(nb).astype(np.float32) * 0.002 + 0.0001) * RNG.choice([-1, 1], nb)
    return I.pack_iq4_xs(idx, codes, d.astype(np.float16))


def _plan(t, M, K, N):
    out = _lib.ggml_hip_mm_plan_t()
    rc = _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(out))
    return rc, out


# ---------------------------------------------------------------- CPU: the restatement itself
def test_hand_built_blocks_decode_to_the_values_worked_out_by_hand():
    b = np.zeros((1, 18), np.uint8)
    b[0, 0:2] = np.array([0.5], np.float16).view(np.uint8)
    b[0, 2 + 0] = 0x0F                     # element 0: index 15 (113), element 16: index 0 (-127)
    b[0, 2 + 5] = 0x78                     # element 5: index 8 (1), element 21: index 7 (-10)
    y = I.dequantize_iq4_nl(b)[0]
    assert (y[0], y[16], y[5], y[21]) == (56.5, -63.5, 0.5, -5.0)
    assert (y[np.r_[1:5, 6:16, 17:21, 22:32]] == -63.5).all()                 # every other nibble 0: kv[0] = -127
    xs = np.zeros((1, 136), np.uint8)
    xs[0, 0:2] = np.array([0.25], np.float16).view(np.uint8)
    xs[0, 2:4] = np.array([0xC000], np.uint16).view(np.uint8)               # scales_h bits 14, 15 -> the high bits of sub-block 7's code
    xs[0, 4 + 3] = 0xF0                                                     # scales_l[3] high nibble: sub-block 7's low bits -> ls = 63
    xs[0, 4 + 1] = 0x05                                                     # sub-block 2: ls = 5
    xs[0, 8 + 0] = 0xF0                                                     # sub-block 0 (ls = 0): element 0 index 0, element 16 index 15
    xs[0, 8 + 16 * 7 + 3] = 0x0F                                            # sub-block 7: element 224 + 3 index 15, 224 + 19 index 0
    xs[0, 8 + 16 * 2] = 0x88                                                # sub-block 2: elements 64, 80 index 8
    assert list(I.xs_codes(xs)[0]) == [0, 0, 5, 0, 0, 0, 0, 63]
    y = I.dequantize_iq4_xs(xs)[0]
    assert (y[0], y[16], y[1]) == (1016.0, -904.0, 1016.0)                 # d (ls - 32) = -8
    assert (y[227], y[243], y[224]) == (875.75, -984.25, -984.25)          # d (ls - 32) = 7.75
    assert (y[64], y[80], y[65]) == (-6.75, -6.75, 857.25)                  # d (ls - 32) = -6.75
    # a patterned super-block decoded in scalar Python straight from the format's text
    xs = np.array([[(0x3C + 53 * i) & 0xFF for i in range(136)]], np.uint8)
    xs[0, 0:2] = np.array([-0.375], np.float16).view(np.uint8)
    sh = int(xs[0, 2]) | int(xs[0, 3]) << 8
    want = np.empty(256, np.float32)
    for e in range(256):
        ib, j = e // 32, e % 32
        ls = ((int(xs[0, 4 + ib // 2]) >> (4 * (ib % 2))) & 15) | (((sh >> (2 * ib)) & 3) << 4)
        byte = int(xs[0, 8 + 16 * ib + j % 16])
        want[e] = F(F(-0.375) * F(ls - 32)) * F(I.KV[(byte & 15) if j < 16 else (byte >> 4)])
    assert np.array_equal(I.dequantize_iq4_xs(xs)[0].view(np.uint32), want.view(np.uint32))


def test_pack_unpack_round_trips():
    b = RNG.integers(0, 256, size=(300, 18), dtype=np.uint8)
    assert np.array_equal(I.pack_iq4_nl(I.iq4nl_index(b), b[:, 0:2].copy().view(np.float16).reshape(-1)), b)
    b = RNG.integers(0, 256, size=(300, 136), dtype=np.uint8)
    assert np.array_equal(I.pack_iq4_xs(I.iq4xs_index(b), I.xs_codes(b), b[:, 0:2].copy().view(np.float16).reshape(-1)), b)
    assert np.array_equal(I.pack_xs_codes(I.xs_codes(b)), b[:, 2:8])


def test_the_IQ4_NL_to_Q8_0_transcode_is_exact():
    b = RNG.integers(0, 256, size=(500, 18), dtype=np.uint8)
    b[:, 0:2] = _nl_blocks(500)[:, 0:2]
    q8 = I.transcode_iq4nl_to_q8_0(b)
    assert set(np.unique(q8[:, 4:].view(np.int8))) <= set(I.KV.tolist())
    assert np.array_equal(I.dequantize_iq4_nl(b).view(np.uint32), R.dequantize_q8_0(q8).view(np.uint32))


def test_an_IQ4_XS_super_block_with_indices_6_to_10_transcodes_exactly_to_Q6_K():
    b = _xs_blocks(300, 6, 11)
    q6 = I.transcode_iq4xs_to_q6_K(b)
    v = I.iq4xs_values(b).reshape(-1, 256)
    assert v.min() == -22 and v.max() == 25
    assert np.array_equal(KQ.q6_values(q6), v)                                # q6 = v + 32
    sc = q6[:, 192:208].view(np.int8).astype(np.int32)
    assert np.array_equal(sc[:, 0::2], I.xs_codes(b) - 32) and np.array_equal(sc[:, 1::2], I.xs_codes(b) - 32)
    assert np.array_equal(q6[:, 208:210], b[:, 0:2])
    assert np.array_equal(I.dequantize_iq4_xs(b).view(np.uint32), KQ.dequantize_q6_K(q6).view(np.uint32))
    with pytest.raises(AssertionError):
        I.transcode_iq4xs_to_q6_K(_xs_blocks(4, 0, 16))


def edge_rows():
    """[8, 256] rows of the quantizer's edge cases (every 32-element block of them one case)"""
    x = np.zeros((8, 256), np.float32)
    x[1, 0:32] = _rand(32) * F(1e-16)                        # amax below 1e-15 ...
    x[1, 5] = np.nextafter(F(1e-15), F(0))                   # ... just below
    x[1, 32 + 7] = F(1e-15)                                  # exactly 1e-15 (not below: a live block)
    x[1, 64 + 9] = np.nextafter(F(1e-15), F(1))              # just above
    x[2, 3], x[2, 17] = 3.0, -3.0                            # a tie in |x|: +3 first
    x[2, 32 + 3], x[2, 32 + 17] = -3.0, 3.0                  # the same tie, -3 first
    x[2, 64:96] = 0.25
    x[2, 64 + 3], x[2, 64 + 17] = 3.0, -3.0                  # the tie among other values
    x[3] = np.abs(_rand(256))
    x[3, 40] = -5.0                                          # a negative maximum
    x[4] = _rand(256, 2.0)
    x[4, 64:96] = 0.0                                        # a super-block with one zero sub-block
    x[5] = _rand(256) * F(1e-39)                             # subnormal inputs only
    x[6] = _rand(256) * F(1e-39)
    x[6, 0:256:32] = 1.0                                     # subnormals beside a normal maximum
    x[7] = _rand(256, 3.0)
    x[7, 100] = 1e4                                          # an outlier
    return x


def test_the_quantizer_on_its_edge_cases():
    z = I.quantize_iq4_nl(np.zeros((3, 32), np.float32))
    assert (z[:, 0:2] == 0).all() and (z[:, 2:] == 0x88).all()             # d = +0, every index 8
    z = I.quantize_iq4_xs(np.zeros((2, 256), np.float32))
    assert (z[:, 0:2].copy().view(np.uint16) == 0x8000).all()               # -0.0f / 32 = -0
    assert (z[:, 2:4].copy().view(np.uint16) == 0xAAAA).all() and (z[:, 4:8] == 0).all() and (z[:, 8:] == 0x88).all()
    x = edge_rows()
    nl = I.quantize_iq4_nl(x).reshape(8, 8, 18)
    s = I.block_scales(x.reshape(-1, 32)).reshape(8, 8)
    assert s[1, 0] == 0 and (nl[1, 0, 2:] == 0x88).all()                    # just below 1e-15: a zero block
    assert s[1, 1] != 0 and s[1, 2] != 0                                     # 1e-15 and just above: a scale is fitted ...
    assert np.array_equal(nl[1, 1, 0:2], [0, 0]) and I.iq4nl_index(nl[1, 1])[0, 7] != 8   # ... which the half flushes to 0, the index stays
    assert s[2, 0] > 0 > s[2, 1]                                             # the first of equal magnitudes sets the sign of the scale
    y3 = I.dequantize_iq4_nl(nl[3].reshape(-1, 18)).reshape(-1)
    assert abs(y3[40] + 5.0) < 0.1                                           # a negative maximum: kept within a step of the code
    xs = I.quantize_iq4_xs(x)
    assert I.xs_codes(xs)[4, 2] == 32 and (xs[4, 8 + 32:8 + 48] == 0x88).all()   # the zero sub-block: code 32, indices 8
    assert (s[5] == 0).all() and (nl[5, :, 2:] == 0x88).all()               # subnormal inputs only: zero blocks
    assert (s[6] != 0).all()
    for blocks, y in ((nl.reshape(-1, 18), I.dequantize_iq4_nl(nl.reshape(-1, 18))), (xs, I.dequantize_iq4_xs(xs))):
        assert np.isfinite(y).all() and y.size == x.size


def _overflow_row():
    """a super-block whose second sub-block overflows the fit (w * q * q beyond f32): its scale is NaN"""
    x = _rand((1, 256))
    x[0, 32:64] = _rand(32, 1e19)
    return x


def test_an_overflowing_fit_gives_the_stated_nan_scale():
    x = _overflow_row()
    s = I.block_scales(x.reshape(-1, 32))
    assert np.isnan(s[1]) and np.isfinite(np.delete(s, 1)).all()
    xs = I.quantize_iq4_xs(x)
    assert I.xs_codes(xs)[0, 1] == 32 and (xs[0, 8 + 16:8 + 32] == 0x88).all()     # nearest(NaN) = 0: ls = 32, every index 8
    assert I.xs_codes(xs)[0, 0] != 32 and np.isfinite(I.dequantize_iq4_xs(xs)).all()
    nl = I.quantize_iq4_nl(x).reshape(8, 18)
    assert np.isnan(nl[1, 0:2].copy().view(np.float16)[0]) and (nl[1, 2:] == 0xFF).all()   # a NaN d, every index 15


def test_the_quantizer_is_a_sane_code():
    x = _rand((64, 1024))
    for q, dq in ((I.quantize_iq4_nl, I.dequantize_iq4_nl), (I.quantize_iq4_xs, I.dequantize_iq4_xs)):
        y = dq(q(x)).reshape(x.shape)
        assert np.sqrt(np.mean((y - x) ** 2)) < 0.1                        # about 4.25 - 4.5 bits per weight
    i = I.best_index(np.array([-200, -127, -115.5, -115.6, 0, 0.5, 6.9, 7, 113, 1e9, np.nan], np.float32))
    assert list(i) == [0, 0, 1, 0, 8, 8, 8, 9, 15, 15, 15]                # a tie (-115.5, 7) goes to the upper entry


def test_type_and_block_size():
    L = _lib.lib()
    assert L.ggml_hip_type_size(IQ4_NL) == 18 and L.ggml_hip_blck_size(IQ4_NL) == 32
    assert L.ggml_hip_type_size(IQ4_XS) == 136 and L.ggml_hip_blck_size(IQ4_XS) == 256
    assert _lib.IQ4_NL == IQ4_NL and _lib.IQ4_XS == IQ4_XS
    assert _lib.row_bytes(IQ4_NL, 11008) == 344 * 18 and _lib.row_bytes(IQ4_XS, 11008) == 43 * 136


def test_the_plans_are_those_of_Q8_0_and_Q6_K():
    """IQ4_NL is a plain Q8_0 weight to the plan, IQ4_XS a Q6_K weight: field for field, over a sweep that reaches every family"""
    L = _lib.lib()
    fields = [f[0] for f in _lib.ggml_hip_mm_plan_t._fields_]
    fam = {IQ4_NL: set(), IQ4_XS: set()}
    for (t, twin, step) in ((IQ4_NL, Q8_0, 32), (IQ4_XS, Q6_K, 256)):
        for M in (1, 96, 300, 1024, 4096, 16384, 32000):
            for K in (256, 512, 1024, 2048, 4096, 11008, 14336):
                for N in (1, 2, 4, 5, 8, 9, 16, 32, 33, 64, 128, 256, 257, 512, 600, 1024, 3000):
                    rc, p = _plan(t, M, K, N)
                    rc2, p2 = _plan(twin, M, K, N)
                    assert rc == rc2 == 0, (t, M, K, N, rc, rc2)
                    assert [getattr(p, f) for f in fields] == [getattr(p2, f) for f in fields], (t, M, K, N)
                    fam[t].add(p.family)
                    assert L.ggml_hip_act_image_kind(t, K, N) == L.ggml_hip_act_image_kind(twin, K, N)
                    assert L.ggml_hip_mul_mat_work_size(t, K, N) == L.ggml_hip_mul_mat_work_size(twin, K, N)
        assert _plan(t, 4096, 4096 + step // 2, 16)[0] == _lib.ERR_SHAPE
    assert fam[IQ4_NL] == {1, 4, 6, 8, 9} and fam[IQ4_XS] == {1, 4, 6, 9}
    assert _plan(IQ4_NL, 100, 48, 1)[0] == _lib.ERR_SHAPE and _plan(IQ4_XS, 100, 288, 1)[0] == _lib.ERR_SHAPE


TREE_IDS = {   # (4096, 4096, 1), (4096, 4096, 16), (4096, 11008, 512), (11008, 4096, 64), (300, 2048, 1100), (4096, 4096, 4096)
    0: (0x3D97F1F3, 0xBC7E15B1, 0xABB22FA1, 0xBC7E15B1, 0xABB22FA1, 0xABB22FA1),
    1: (0x12999374, 0x98D5246C, 0x57A40376, 0x98D5246C, 0xA08FD2C1, 0xA08FD2C1),
    2: (0x81EC0437, 0x7DD0398B, 0xA6159D07, 0x7DD0398B, 0x99637F0A, 0x99637F0A),
    3: (0x81EC0437, 0x6923AD24, 0x686C818A, 0x6923AD24, 0xF314B569, 0xF314B569),
    4: (0x81EC0437, 0x06B9963D, 0x7E4C8C31, 0x06B9963D, 0xD6A5C2F5, 0x06B9963D),
    6: (0x81EC0437, 0xB6E23919, 0x5E890255, 0xB6E23919, 0x86CE65D1, 0xC31B1FAE),
    7: (0x81EC0437, 0xAFEBA436, 0x686C818A, 0xAFEBA436, 0x40271E0E, 0xAFEBA436),
    8: (0x81EC0437, 0x8B0A9F63, 0x92D90F2F, 0x8B0A9F63, 0xBB1E72AB, 0xF8555DC6),
    110: (0xCD77340D, 0xE314137F, 0x136D429B, 0xE314137F, 0x4C061FB7, 0xE314137F),
    111: (0x79EBF79F, 0xFEB989A5, 0x764C7F99, 0xFEB989A5, 0xDEA5CF8D, 0xFEB989A5),
    112: (0x79EBF79F, 0xB7EBB0CE, 0x606C74F2, 0xB7EBB0CE, 0x38271176, 0xB7EBB0CE),
    113: (0x79EBF79F, 0xB7EBB0CE, 0x606C74F2, 0xB7EBB0CE, 0x38271176, 0xB7EBB0CE),
    114: (0x79EBF79F, 0xFEB989A5, 0x764C7F99, 0xFEB989A5, 0xDEA5CF8D, 0xFEB989A5),
    130: (0xA626715E, 0xB1B5A072, 0x115D2250, 0xB1B5A072, 0x1997F557, 0x1997F557),
}


def test_the_tree_ids_of_the_existing_types_are_unchanged():
    shapes = ((4096, 4096, 1), (4096, 4096, 16), (4096, 11008, 512), (11008, 4096, 64), (300, 2048, 1100), (4096, 4096, 4096))
    for t, ids in TREE_IDS.items():
        assert tuple(_plan(t, *s)[1].tree_id for s in shapes) == ids, t
    assert tuple(_plan(IQ4_NL, *s)[1].tree_id for s in shapes) == TREE_IDS[Q8_0]
    assert tuple(_plan(IQ4_XS, *s)[1].tree_id for s in shapes) == TREE_IDS[Q6_K]


@pytest.mark.parametrize("t", [IQ4_NL, IQ4_XS])
def test_seam_1_refuses_an_iq4_tensor(t):
    """the reference's enum cannot express the types: Seam 1 refuses them before anything else"""
    L = _lib.lib()
    K, M, N = 256, 8, 2
    w = np.zeros(M * _lib.row_bytes(t, K), np.uint8)
    x = np.zeros((N, K), np.float32)
    d = np.zeros((N, M), np.float32)

    def tensor(tt_type, arr, ne, nb0, nb1):
        tt = _lib.ggml_tensor()
        tt.type = tt_type
        for i in range(4):
            tt.ne[i] = ne[i] if i < len(ne) else 1
        tt.nb[0] = nb0
        tt.nb[1] = nb1
        tt.nb[2] = tt.nb[1] * tt.ne[1]
        tt.nb[3] = tt.nb[2]
        tt.data = arr.ctypes.data_as(C.c_void_p)
        return tt

    s0 = tensor(t, w, (K, M), L.ggml_hip_type_size(t), _lib.row_bytes(t, K))
    s1, dst = tensor(_lib.F32, x, (K, N), 4, 4 * K), tensor(_lib.F32, d, (M, N), 4, 4 * M)
    p = _lib.ggml_compute_params(_lib.GGML_TASK_COMPUTE, 0, 1, 0, None)
    assert L.ggml_hip_compute_forward_mul_mat(C.byref(p), C.byref(s0), C.byref(s1), C.byref(dst)) == _lib.ERR_TYPE


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


class _forced:
    """ggml_hip_debug_force_gemm for the block (the hook acts on the calling thread), reset to automatic after it"""
    def __init__(self, which):
        self.which = which

    def __enter__(self):
        _lib.lib().ggml_hip_debug_force_gemm(self.which)

    def __exit__(self, *a):
        _lib.lib().ggml_hip_debug_force_gemm(0)


@gpu
def test_dequantize_is_bit_exact(dev):
    import torch
    for nb in (1, 7, 64):
        for t, b, want in ((IQ4_NL, RNG.integers(0, 256, size=(8 * nb, 18), dtype=np.uint8), I.dequantize_iq4_nl),
                           (IQ4_XS, RNG.integers(0, 256, size=(nb, 136), dtype=np.uint8), I.dequantize_iq4_xs),
                           (IQ4_NL, I.quantize_iq4_nl(_rand((8 * nb, 32), 3.0)), I.dequantize_iq4_nl),
                           (IQ4_XS, I.quantize_iq4_xs(_rand((nb, 256), 3.0)), I.dequantize_iq4_xs)):
            got = dev.dequantize_rows(t, torch.from_numpy(b.reshape(1, -1)).cuda(), nb * 256).cpu().numpy().reshape(want(b).shape)
            assert np.array_equal(got.view(np.uint32), want(b).view(np.uint32)), (t, nb)


@gpu
def test_device_quantizer_writes_the_restatements_bytes(dev):
    import torch
    cases = [(1, 256, 1.0), (7, 768, 3.0), (33, 2048, 0.01), (5, 11008, 40.0), (3, 4096, 1e-3)]
    for t, q, nbytes in ((IQ4_NL, I.quantize_iq4_nl, 18), (IQ4_XS, I.quantize_iq4_xs, 136)):
        for (nrows, K, scale) in cases:
            x = _rand((nrows, K), scale)
            x[0, :256] = 0.0
            if nrows > 1:
                x[1, :256] = edge_rows()[nrows % 8]
            want = q(x).reshape(nrows, -1)
            got = dev.quantize_rows(t, torch.from_numpy(x).cuda()).cpu().numpy()
            bad = np.nonzero((got != want).reshape(-1, nbytes).any(axis=1))[0]
            assert got.shape == want.shape and bad.size == 0, f"{t} {nrows}x{K} scale {scale}: blocks {bad[:8]} differ"
        x = edge_rows()
        got = dev.quantize_rows(t, torch.from_numpy(x).cuda()).cpu().numpy()
        assert np.array_equal(got, q(x).reshape(8, -1)), t


@gpu
def test_device_quantizer_on_an_overflowing_fit(dev):
    """the NaN scale of an overflowed fit: IQ4_XS's bytes are the restatement's; IQ4_NL's too, but for the NaN d's sign and payload"""
    import torch
    x = _overflow_row()
    got = dev.quantize_rows(IQ4_XS, torch.from_numpy(x).cuda()).cpu().numpy()
    assert np.array_equal(got, I.quantize_iq4_xs(x).reshape(1, -1))
    got = dev.quantize_rows(IQ4_NL, torch.from_numpy(x).cuda()).cpu().numpy().reshape(8, 18)
    want = I.quantize_iq4_nl(x).reshape(8, 18)
    assert np.array_equal(np.delete(got, 1, axis=0), np.delete(want, 1, axis=0)) and np.array_equal(got[1, 2:], want[1, 2:])
    assert np.isnan(got[1, 0:2].copy().view(np.float16)[0])


@gpu
def test_device_quantizer_at_4096_x_11008_IQ4_XS(dev):
    """the whole matrix on the device, 128 of its rows (every row is independent) against the restatement"""
    import torch
    g = torch.Generator(device="cuda")
    g.manual_seed(123)
    x = torch.randn((4096, 11008), generator=g, device="cuda")
    got = dev.quantize_rows(IQ4_XS, x)
    rows = np.sort(np.random.default_rng(4096).choice(4096, size=128, replace=False))
    assert np.array_equal(got[torch.from_numpy(rows).cuda()].cpu().numpy(), I.quantize_iq4_xs(x[torch.from_numpy(rows).cuda()].cpu().numpy()).reshape(128, -1))


@gpu
def test_upload_download_is_byte_exact_and_the_type_reported(dev):
    import torch
    from ggmlsharp_amd._lib import lib
    for t, K in ((IQ4_NL, 736), (IQ4_XS, 768)):
        M = 70
        rows = RNG.integers(0, 256, size=(M, _lib.row_bytes(t, K)), dtype=np.uint8)   # every bit pattern of d: NaN, Inf, subnormal
        if t == IQ4_NL:
            rows.reshape(-1, 18)[:4, 0:2] = np.array([[0x00, 0x7C], [0x01, 0x7C], [0x01, 0x00], [0x00, 0x80]], np.uint8)  # inf, sNaN, subnormal, -0
        W = dev.Weight.from_host(t, rows, K)
        assert lib().ggml_hip_weight_type(W.handle) == t and lib().ggml_hip_weight_rows(W.handle) == M and lib().ggml_hip_weight_cols(W.handle) == K
        assert np.array_equal(W.download().reshape(M, -1), rows)
        shard = dev.Weight.from_host(t, rows, K, row_begin=11, row_end=40)
        assert np.array_equal(shard.download().reshape(29, -1), rows[11:40])
        Wd = dev.Weight.from_device(t, torch.from_numpy(rows).cuda(), K)
        assert np.array_equal(Wd.download().reshape(M, -1), rows)
        for w in (W, shard, Wd):
            w.free()
    # under ggml_hip_debug_force_gemm(3) an IQ4_NL weight gets Q8_0's two-digit planes too, and downloads the same bytes
    rows = _nl_blocks(64 * 32).reshape(64, -1)
    with _forced(3):
        W = dev.Weight.from_host(IQ4_NL, rows, 1024)
    assert np.array_equal(W.download().reshape(64, -1), rows)
    W.free()


@gpu
def test_the_refusals(dev):
    import torch
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = np.zeros(4096, np.uint8)
    h = C.c_void_p()
    assert L.ggml_hip_weight_upload(IQ4_NL, rows.ctypes.data_as(C.c_void_p), 48, 4, 54, 0, 4, None, C.byref(h)) == _lib.ERR_SHAPE   # K % 32
    assert L.ggml_hip_weight_upload(IQ4_XS, rows.ctypes.data_as(C.c_void_p), 288, 4, 272, 0, 4, None, C.byref(h)) == _lib.ERR_SHAPE  # K % 256
    x = torch.zeros((2, 512), device="cuda")
    b = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    vp = lambda a: C.c_void_p(a.data_ptr())  # noqa: E731
    assert L.ggml_hip_quantize_rows_dev(IQ4_NL, vp(x), 2, 48, vp(b), st) == _lib.ERR_SHAPE
    assert L.ggml_hip_quantize_rows_dev(IQ4_XS, vp(x), 2, 288, vp(b), st) == _lib.ERR_SHAPE
    assert L.ggml_hip_dequantize_rows_dev(IQ4_NL, vp(b), 2, 48, vp(x), st) == _lib.ERR_SHAPE
    assert L.ggml_hip_dequantize_rows_dev(IQ4_XS, vp(b), 2, 288, vp(x), st) == _lib.ERR_SHAPE
    for t in (IQ4_NL, IQ4_XS):                                # never inside a ggml_tensor: the row entries of the seams refuse them too
        assert L.ggml_hip_quantize_rows_src_dev(t, 0, vp(x), 512, 2, 512, vp(b), st) == _lib.ERR_TYPE
        assert L.ggml_hip_add_q_f32_rows_dev(t, vp(b), vp(x), 2, 512, vp(b), st) == _lib.ERR_TYPE
    torch.cuda.synchronize()


# IQ4_NL: every family a Q8_0 weight reaches -- 1 the fused mat-vec, 4 K3s (K3s-16 on short matrices), 6 K3p, 8 / 9 the staged f16 / int8
# forms; with ggml_hip_debug_force_gemm 1 / 2 / 3 the staged int8, f16 and MX forms (the MX form on the two-digit planes)
NL_FAMILY_SHAPES = [(300, 1024, 1, 0, 1), (515, 4096, 3, 0, 1), (96, 1024, 5, 0, 4), (300, 2048, 16, 0, 4), (1024, 4096, 40, 0, 4),
                    (96, 256, 9, 0, 8), (300, 512, 40, 0, 8), (96, 256, 600, 0, 9), (300, 512, 600, 0, 9),
                    (300, 2048, 600, 0, 6), (4096, 4096, 257, 0, 6), (16384, 2048, 33, 0, 6),
                    (300, 1024, 40, 1, 9), (300, 1024, 40, 2, 8), (300, 1024, 600, 3, 7), (515, 2048, 40, 3, 7)]


@gpu
@pytest.mark.parametrize("M,K,N,force,family", NL_FAMILY_SHAPES)
def test_IQ4_NL_is_bitwise_its_Q8_0_transcode(dev, M, K, N, force, family):
    import torch
    rows = _nl_blocks(M * K // 32)
    rows[::3] = I.quantize_iq4_nl(_rand((rows[::3].shape[0], 32)))
    x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
    with _forced(force):
        assert _plan(Q8_0, M, K, N)[1].family == family and _plan(IQ4_NL, M, K, N)[1].family == family
        Wn = dev.Weight.from_host(IQ4_NL, rows.reshape(M, -1), K)
        W8 = dev.Weight.from_host(Q8_0, I.transcode_iq4nl_to_q8_0(rows).reshape(M, -1), K)
        got, want = dev.mul_mat(Wn, x), dev.mul_mat(W8, x)
    assert torch.equal(got, want), (M, K, N, force)
    _close(got.cpu().numpy(), I.mul_mat_iq4_nl(rows.reshape(M, -1), x.cpu().numpy()), f"IQ4_NL {M}x{K}x{N} force {force}", K)
    Wn.free()
    W8.free()


# IQ4_XS: every kernel family the plan picks for Q6_K (tests/test_q3k.py's list): 1 the fused mat-vec, 4 K3s, 9 the staged int8 form, 6 K3p
XS_FAMILY_SHAPES = [(300, 1024, 1, 1), (515, 4096, 3, 1), (300, 4096, 4, 1),
                    (300, 2048, 5, 4), (300, 2048, 16, 4), (1024, 4096, 40, 4), (4096, 4096, 64, 4),
                    (515, 768, 8, 9), (300, 1024, 100, 9), (130, 512, 600, 9),
                    (300, 2048, 1100, 6), (4096, 4096, 257, 6), (16384, 2048, 33, 6)]


@gpu
@pytest.mark.parametrize("M,K,N,family", XS_FAMILY_SHAPES)
def test_IQ4_XS_restricted_to_indices_6_to_10_is_bitwise_its_Q6_K_twin(dev, M, K, N, family):
    import torch
    assert _plan(Q6_K, M, K, N)[1].family == family and _plan(IQ4_XS, M, K, N)[1].family == family
    rows = _xs_blocks(M * K // 256, 6, 11)
    Wx = dev.Weight.from_host(IQ4_XS, rows.reshape(M, -1), K)
    W6 = dev.Weight.from_host(Q6_K, I.transcode_iq4xs_to_q6_K(rows).reshape(M, -1), K)
    x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
    assert torch.equal(dev.mul_mat(Wx, x), dev.mul_mat(W6, x)), (M, K, N)
    Wx.free()
    W6.free()


@gpu
@pytest.mark.parametrize("M,K,N,family", XS_FAMILY_SHAPES)
def test_unrestricted_IQ4_XS_matches_the_restatement(dev, M, K, N, family):
    """the full codebook (-127 .. 113) and the scale codes 0 / 63 in every family the plan picks"""
    import torch
    for raw in (True, False):
        rows = _xs_blocks(M * K // 256) if raw else I.quantize_iq4_xs(_rand((M * K // 256, 256)))
        v = I.iq4xs_values(rows)
        assert not raw or (v.min() == -127 and v.max() == 113)
        x = _rand((N, K))
        W = dev.Weight.from_host(IQ4_XS, rows.reshape(M, -1), K)
        assert _plan(IQ4_XS, M, K, N)[1].family == family
        got = dev.mul_mat(W, torch.from_numpy(x).cuda()).cpu().numpy()
        _close(got, I.mul_mat_iq4_xs(rows.reshape(M, -1), x), f"IQ4_XS {M}x{K}x{N} raw={raw}", K)
        W.free()


@gpu
def test_mul_mat_at_4096_x_11008_x_512_on_a_sample(dev):
    import torch
    M, K, N = 4096, 11008, 512
    rs = np.random.default_rng(40961)
    ms = np.sort(rs.choice(M, size=64, replace=False))
    ns = np.sort(rs.choice(N, size=64, replace=False))
    x = _rand((N, K))
    xd = torch.from_numpy(x).cuda()
    for t, blocks, ref in ((IQ4_XS, _xs_blocks(M * K // 256), I.mul_mat_iq4_xs), (IQ4_NL, _nl_blocks(M * K // 32), I.mul_mat_iq4_nl)):
        rows = blocks.reshape(M, -1)
        W = dev.Weight.from_host(t, rows, K)
        got = dev.mul_mat(W, xd)
        _close(got.cpu().numpy()[np.ix_(ns, ms)], ref(rows[ms], x[ns]), f"{t} {M}x{K}x{N} (64 x 64 sample)", K)
        W.free()


@gpu
def test_fused_mat_vec_equals_the_two_step_form_bitwise(dev):
    import torch
    for t, make in ((IQ4_NL, _nl_blocks), (IQ4_XS, _xs_blocks)):
        for (M, K, N) in ((100, 256, 1), (515, 4096, 2), (300, 4096, 4), (130, 11008, 1), (4096, 4096, 1)):
            bs = 32 if t == IQ4_NL else 256
            rows = make(M * K // bs).reshape(M, -1)
            assert _plan(t, M, K, N)[1].family == 1
            W = dev.Weight.from_host(t, rows, K)
            xd = torch.from_numpy(_rand((N, K), 2.0)).cuda()
            one = dev.mul_mat(W, xd)
            work = dev.alloc_work(t, K, N)
            dev.mul_mat_init(W, xd, work)
            two = torch.empty_like(one)
            dev.mul_mat_compute(W, N, two, work)
            assert torch.equal(one, two), (t, M, K, N)
            W.free()


@gpu
@pytest.mark.parametrize("t", [IQ4_NL, IQ4_XS])
@pytest.mark.parametrize("M,K,N", [(300, 4096, 2), (300, 2048, 40), (300, 2048, 1100)])
def test_a_row_shard_is_the_bitwise_column_slice_of_the_whole(dev, t, M, K, N):
    import torch
    rows = (_nl_blocks(M * K // 32) if t == IQ4_NL else _xs_blocks(M * K // 256)).reshape(M, -1)
    xd = torch.from_numpy(_rand((N, K))).cuda()
    W = dev.Weight.from_host(t, rows, K)
    Ws = dev.Weight.from_host(t, rows, K, row_begin=100, row_end=260)
    whole, part = dev.mul_mat(W, xd), dev.mul_mat(Ws, xd)
    assert torch.equal(part, whole[:, 100:260])
    W.free()
    Ws.free()


@gpu
def test_K3p_on_a_tall_IQ4_XS_matrix_equals_its_K3s_shards_bitwise(dev):
    import torch
    M, K, N, S = 16384, 4096, 40, 1024
    assert _plan(IQ4_XS, M, K, N)[1].family == 6 and _plan(IQ4_XS, S, K, N)[1].family == 4
    g = torch.Generator(device="cuda")
    g.manual_seed(IQ4_XS)
    rows = dev.quantize_rows(IQ4_XS, torch.randn((M, K), generator=g, device="cuda"))
    xd = torch.randn((N, K), generator=g, device="cuda")
    W = dev.Weight.from_device(IQ4_XS, rows, K)
    whole = dev.mul_mat(W, xd)
    W.free()
    for r0 in range(0, M, S):
        Ws = dev.Weight.from_device(IQ4_XS, rows, K, row_begin=r0, row_end=r0 + S)
        assert torch.equal(dev.mul_mat(Ws, xd), whole[:, r0:r0 + S]), r0
        Ws.free()


@gpu
@pytest.mark.parametrize("t", [IQ4_NL, IQ4_XS])
def test_groups_epilogue_and_push_entries_are_bitwise_the_single_calls(dev, t):
    """projection groups (_mul_mat_multi_dev for IQ4_NL's fused groups, _multi_work_dev for both), the epilogue entry and the push entry;
    IQ4_NL's are the bits of its Q8_0 twins'"""
    import torch
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = 2048
    bs = 32 if t == IQ4_NL else 256
    fused_seen = 0
    for (Ms, N) in (((300, 200), 1), ((300, 200, 130), 3), ((300, 200, 130), 16), ((300, 200, 130, 77), 40), ((1024, 515, 300, 96), 600)):
        blocks = [(_nl_blocks if t == IQ4_NL else _xs_blocks)(M * K // bs).reshape(M, -1) for M in Ms]
        Ws = [dev.Weight.from_host(t, b, K) for b in blocks]
        x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
        singles = [dev.mul_mat(w, x) for w in Ws]
        hw = (C.c_void_p * len(Ws))(*[w.handle for w in Ws])
        if t == IQ4_NL:                                       # the Q8_0 twins: the same bits, and a fused group exactly where theirs is
            twins = [dev.Weight.from_host(Q8_0, I.transcode_iq4nl_to_q8_0(b).reshape(b.shape[0], -1), K) for b in blocks]
            for s, w8 in zip(singles, twins):
                assert torch.equal(s, dev.mul_mat(w8, x)), (Ms, N)
            hw8 = (C.c_void_p * len(twins))(*[w.handle for w in twins])
            assert L.ggml_hip_mul_mat_multi_fused(hw, len(Ws), N) == L.ggml_hip_mul_mat_multi_fused(hw8, len(twins), N), (Ms, N)
            for w8 in twins:
                w8.free()
        ld = (C.c_int64 * len(Ws))(*[M + 4 for M in Ms])
        work = dev.alloc_work(t, K, N)
        outs = [torch.full((N, M + 4), -2.0, device="cuda") for M in Ms]
        dp = (C.c_void_p * len(Ws))(*[o.data_ptr() for o in outs])
        _lib.check(L.ggml_hip_mul_mat_multi_work_dev(hw, len(Ws), C.c_void_p(x.data_ptr()), K, N, dp, ld, C.c_void_p(work.data_ptr()),
                                                     work.numel(), st), "multi with work")
        for o, s, M in zip(outs, singles, Ms):
            assert torch.equal(o[:, :M], s) and torch.all(o[:, M:] == -2.0), (Ms, N)
        if L.ggml_hip_mul_mat_multi_fused(hw, len(Ws), N):
            fused_seen += 1
            outs = [torch.full((N, M + 4), -2.0, device="cuda") for M in Ms]
            dp = (C.c_void_p * len(Ws))(*[o.data_ptr() for o in outs])
            _lib.check(L.ggml_hip_mul_mat_multi_dev(hw, len(Ws), C.c_void_p(x.data_ptr()), K, N, dp, ld, None, 0, None, None, st), "multi")
            for o, s, M in zip(outs, singles, Ms):
                assert torch.equal(o[:, :M], s), (Ms, N)
        for w, s in zip(Ws, singles):
            M = w.M
            dst = torch.full((N, M), -3.0, device="cuda")
            pp = (C.c_void_p * 1)(dst.data_ptr())
            _lib.check(L.ggml_hip_mul_mat_push_dev(w.handle, C.c_void_p(x.data_ptr()), N, K, pp, 1, 0, M, 0, C.c_void_p(work.data_ptr()),
                                                   work.numel(), st), "push")
            assert torch.equal(dst, s), (M, N)
            addend = torch.from_numpy(_rand((N, M))).cuda()
            out, out2 = torch.empty((N, M), device="cuda"), torch.empty((N, M), device="cuda")
            _lib.check(L.ggml_hip_mul_mat_epilogue_dev(w.handle, C.c_void_p(x.data_ptr()), N, K, C.c_void_p(out.data_ptr()), M,
                                                       C.c_void_p(work.data_ptr()), work.numel(), 1, C.c_void_p(addend.data_ptr()), M,
                                                       C.c_void_p(out2.data_ptr()), M, C.c_float(1.0), st), "epilogue add")
            assert torch.equal(out, s) and torch.equal(out2, s + addend), (M, N)
        for w in Ws:
            w.free()
    if t == IQ4_NL:
        assert fused_seen > 0                                 # the fused projection group ran for IQ4_NL
