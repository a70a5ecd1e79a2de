"""Q2_K as an UNPINNED EXTRA (include/ggml_hip_ext.h GGML_HIP_TYPE_Q2_K; ggmlsharp_amd/csrc/kquants.hip).  The checker is
tests/np_q2k.py, a numpy restatement of the published upstream format.  The block term of a Q2_K super-block is a Q6_K super-block, so the
library runs the product on Q6_K's kernels and subtracts the min term T behind it with a pass whose arithmetic np_q2k.min_term restates:
the product must be fl(B - T) bit for bit, with B the product of the transcoded Q6_K weight, in every kernel family.
CPU tests: the restatement by hand and its round trips, the sizes and the plan.  GPU tests: the device path against the restatement and
against Q6_K."""
import ctypes as C

import numpy as np
import pytest

import np_kquants as KQ
import np_q2k as Q2
import oracle_lib as O
from ggmlsharp_amd import _lib

RNG = np.random.default_rng(2110)
Q2_K, Q6_K = 110, 114
F = np.float32
PLAN_MIN_PASS, PLAN_FUSED_FAMILY = 64, 1


def _rand(shape, scale=1.0):
    return (RNG.standard_normal(shape) * scale).astype(np.float32)


def _random_blocks(nb, dmin=True):
    """raw super-blocks: every bit pattern of scales and qs; d and dmin small finite halves (dmin = 0 when asked)"""
    b = RNG.integers(0, 256, size=(nb, Q2.Q2K_BYTES), dtype=np.uint8)
    b[:, 80:82] = (RNG.random(nb).astype(np.float32) * 0.002 + 0.0001).astype(np.float16).reshape(-1, 1).view(np.uint8)
    b[:, 82:84] = ((RNG.random(nb).astype(np.float32) * 0.002 + 0.0001) * (1 if dmin else 0)).astype(np.float16).reshape(-1, 1).view(np.uint8)
    return b


def _plan(t, M, K, N):
    out = _lib.ggml_hip_mm_plan_t()
    rc = _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(out))
    return rc, out


# ---------------------------------------------------------------- CPU: the restatement itself
def test_a_hand_built_super_block_decodes_to_the_values_worked_out_by_hand():
    b = np.zeros((1, 84), dtype=np.uint8)
    b[0, 16 + 32 + 5] = 0xE4              # qs[32 n + l], n = 1, l = 5: bit pairs 0, 1, 2, 3 for s = 0..3 -> elements 133, 165, 197, 229
    b[0, 16 + 7] = 0x03                   # qs[7]: element 7 (n = 0, s = 0) gets q = 3
    b[0, 0] = 0x52                        # sub-block 0: sc 2, m 5
    b[0, 8] = 0x0B                        # sub-block 8 (elements 128..143): sc 11, m 0
    b[0, 10] = 0xF1                       # sub-block 10 (elements 160..175): sc 1, m 15
    b[0, 12] = 0x37                       # sub-block 12 (elements 192..207): sc 7, m 3
    b[0, 14] = 0xA0                       # sub-block 14 (elements 224..239): sc 0, m 10
    b[0, 80:82] = np.array([0.5], np.float16).view(np.uint8)
    b[0, 82:84] = np.array([0.25], np.float16).view(np.uint8)
    q = Q2.q2_values(b)[0]
    assert (q[7], q[133], q[165], q[197], q[229]) == (3, 0, 1, 2, 3)
    assert (q != 0).sum() == 4
    y = Q2.dequantize_q2_K(b)[0]
    assert y[7] == 0.5 * 2 * 3 - 0.25 * 5 == 1.75 and y[0] == -1.25
    assert y[133] == 0.0 and y[165] == 0.5 * 1 * 1 - 0.25 * 15 == -3.25
    assert y[197] == 0.5 * 7 * 2 - 0.75 == 6.25 and y[229] == 0.0 - 2.5
    assert y[16] == 0.0                                                     # sub-block 1: scale byte 0
    # a patterned block, each element decoded in scalar Python straight from the format's text
    b = np.zeros((1, 84), dtype=np.uint8)
    b[0, 0:16] = [(37 * j + 11) & 0xFF for j in range(16)]
    b[0, 16:80] = [(71 * i + 13) & 0xFF for i in range(64)]
    b[0, 80:82] = np.array([0.375], np.float16).view(np.uint8)
    b[0, 82:84] = np.array([0.0625], np.float16).view(np.uint8)
    scb, qs = [int(c) for c in b[0, 0:16]], [int(c) for c in b[0, 16:80]]
    want = np.empty(256, dtype=np.float32)
    for e in range(256):
        n, s, l = e // 128, (e % 128) // 32, e % 32
        qv = (qs[32 * n + l] >> (2 * s)) & 3
        sc, m = scb[e // 16] & 15, scb[e // 16] >> 4
        want[e] = F(F(F(0.375) * F(sc)) * F(qv)) - F(F(0.0625) * F(m))
    assert np.array_equal(Q2.dequantize_q2_K(b)[0].view(np.uint32), want.view(np.uint32))


def test_pack_unpack_round_trips_and_the_transcoder_to_Q6_K():
    b = _random_blocks(300)
    q = Q2.q2_values(b)
    assert q.min() == 0 and q.max() == 3
    repacked = Q2.pack_q2_K(q, Q2.q2_scales(b), Q2.q2_mins(b), b[:, 80:82].copy().view(np.float16).reshape(-1),
                            b[:, 82:84].copy().view(np.float16).reshape(-1))
    assert np.array_equal(repacked, b)                                       # pack(unpack(bytes)) == bytes
    q6 = Q2.transcode_to_q6_K(b)
    assert np.array_equal(KQ.q6_values(q6), q)
    # in exact arithmetic: dequant(Q2_K) == dequant(Q6_K(transcode)) - dmin * m
    y2 = Q2.dequantize_q2_K(b).astype(np.float64).reshape(-1, 16, 16)
    y6 = KQ.dequantize_q6_K(q6).astype(np.float64).reshape(-1, 16, 16)
    mt = (Q2.q2_dmin(b).astype(np.float64)[:, None] * Q2.q2_mins(b))[:, :, None]
    assert np.array_equal(y2, y6 - mt)
    # and the products: the f64 checker of Q2_K is Q6_K's of the transcoded bytes minus the min term
    w = Q2.quantize_q2_K(_rand((8, 256))).reshape(2, -1)
    x = _rand((3, 1024))
    got = Q2.mul_mat_q2_K(w, x).astype(np.float64)
    want = KQ.mul_mat_q6_K(Q2.transcode_to_q6_K(w).reshape(2, -1), x).astype(np.float64) - Q2.min_term(w, x)
    assert np.allclose(got, want, rtol=1e-5, atol=1e-5 * np.abs(want).max())


def test_the_min_term_restatement_is_exact_in_its_order():
    """S per super-block is an exact integer; the f32 loop in ascending super-blocks matches a scalar re-evaluation"""
    w = _random_blocks(3 * 4).reshape(3, -1)
    x = _rand((2, 1024), 3.0)
    T = Q2.min_term(w, x)
    d8, _, bs = KQ.quantize_q8_K(x.reshape(-1, 256))
    d8, bs = d8.reshape(2, 4), bs.reshape(2, 4, 16)
    wb = w.reshape(-1, 84)
    for n in range(2):
        for i in range(3):
            acc = F(0)
            for sb in range(4):
                blk = wb[i * 4 + sb]
                S = sum(int(blk[j] >> 4) * int(bs[n, sb, j]) for j in range(16))
                acc = F(acc + F(F(d8[n, sb] * Q2.q2_dmin(blk)[0]) * F(S)))
            assert T[n, i] == acc


def test_the_qkx1_restatement_for_16_is_np_kquants_for_32():
    x = _rand((64, 32), 2.0)
    x[3] = 1.5                                                              # a flat row
    x[4] = np.abs(x[4])
    for nmax in (3, 15, 31):
        a, b = Q2.make_qkx1_quants(x, nmax), KQ.make_qkx1_quants(x, nmax)
        assert all(np.array_equal(u, v) for u, v in zip(a, b)), nmax


def test_the_reference_quantizer_produces_valid_blocks_and_its_edge_cases():
    x = _rand((200, 256), 2.0)
    b = Q2.quantize_q2_K(x)
    assert b.shape == (200, 84)
    q, sc, m = Q2.q2_values(b), Q2.q2_scales(b), Q2.q2_mins(b)
    assert q.min() >= 0 and q.max() <= 3
    assert (sc.max(axis=1) == 15).all() and (m.max(axis=1) == 15).all()    # the largest scale / min maps to 15
    y = Q2.dequantize_q2_K(b)
    assert np.abs(y - x).max() <= 0.6 * np.abs(x).max()                      # two bits: coarse but sane
    # an all-zero super-block is 84 zero bytes
    assert not Q2.quantize_q2_K(np.zeros((1, 256), np.float32)).any()
    # sub-blocks that are exact multiples (powers of two) of codes 0..3: every min is 0 and so is dmin
    Lp = RNG.integers(0, 4, size=(4, 16, 16))
    Lp[:, :, 0], Lp[:, :, 1] = 0, 3
    xp = (Lp * np.array([0.5, 0.25, 1.0, 2.0] * 4, np.float32)[None, :, None]).astype(np.float32).reshape(4, 256)
    bp = Q2.quantize_q2_K(xp)
    assert not Q2.q2_mins(bp).any() and not Q2.q2_dmin(bp).any()
    assert np.abs(Q2.dequantize_q2_K(bp) - xp).max() <= 0.1 * xp.max()
    # one sub-block far smaller than the rest: its 4-bit scale rounds to 0 and its codes stay those of the first pass
    x = _rand((1, 256), 50.0)
    x[0, 48:64] = np.abs(_rand(16, 1e-3)) + 1e-3
    b = Q2.quantize_q2_K(x)
    assert Q2.q2_scales(b)[0, 3] == 0
    _, _, L3 = Q2.make_qkx1_quants(x[:, 48:64], 3)
    assert np.array_equal(Q2.q2_values(b)[0, 48:64], L3[0])


def test_type_and_block_size():
    L = _lib.lib()
    assert L.ggml_hip_type_size(Q2_K) == 84 and L.ggml_hip_blck_size(Q2_K) == 256
    assert _lib.Q2_K == Q2_K and _lib.row_bytes(Q2_K, 11008) == 43 * 84


def test_the_plan_of_Q2_K_is_the_plan_of_Q6_K_with_the_min_pass():
    """Q6_K's plan field for field -- except the fused mat-vec, which becomes the two-step mat-vec (Q6_K's COMPUTE-only plan) -- and the
    flag; its tree_id does not follow M"""
    fields = [f[0] for f in _lib.ggml_hip_mm_plan_t._fields_]
    for K in (256, 2048, 4096, 11008, 14336, 36864):
        for N in (1, 2, 4, 5, 8, 9, 16, 32, 33, 64, 128, 256, 257, 512, 1024, 3000):
            trees = set()
            for M in (1, 100, 1024, 4096, 16384, 32000):
                rc2, p2 = _plan(Q2_K, M, K, N)
                rc6, p6 = _plan(Q6_K, M, K, N)
                assert rc2 == rc6 == 0, (M, K, N, rc2, rc6)
                assert p2.flags & PLAN_MIN_PASS and not p6.flags & PLAN_MIN_PASS
                assert p2.family != PLAN_FUSED_FAMILY and p2.image_kind == 0
                trees.add(p2.tree_id)
                if p6.family != PLAN_FUSED_FAMILY:
                    same = [f for f in fields if f not in ("flags", "tree_id")]
                    assert [getattr(p2, f) for f in same] == [getattr(p6, f) for f in same], (M, K, N)
                    assert p2.flags == p6.flags | PLAN_MIN_PASS and p2.tree_id != p6.tree_id
                else:
                    assert N <= 4 and p2.family == 2 and p2.flags & 16          # the two-step mat-vec on K1's image
            assert len(trees) == 1, (K, N)
    assert _plan(Q2_K, 4096, 4096 + 32, 16)[0] == _lib.ERR_SHAPE                          # K % 256


def test_the_tree_ids_of_the_other_types_are_unchanged():
    """the min-pass flag enters tree_id only when set: Q6_K's ids are those of the hash over (arith, ksplit, kstyle, kunit, Q8K) alone"""
    def fnv(parts):
        h = 2166136261
        for v in parts:
            h = ((h ^ (v & 0xFFFFFFFF)) * 16777619) & 0xFFFFFFFF
        return h
    for t in (Q6_K, 111, 112, 113, _lib.Q8_0, _lib.Q4_0):
        for (M, K, N) in ((4096, 4096, 1), (4096, 4096, 16), (4096, 11008, 512), (11008, 4096, 64), (300, 2048, 1100)):
            rc, p = _plan(t, M, K, N)
            assert rc == 0
            assert p.tree_id == fnv([p.arith, p.ksplit, p.kstyle, p.kunit, p.flags & 8]), (t, M, K, N)


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


def _two_phase(dev, W, x):
    """the product through INIT + COMPUTE (no fused form)"""
    import torch
    N = x.shape[0]
    work = dev.alloc_work(W.type, W.K, N)
    dev.mul_mat_init(W, x, work)
    out = torch.empty((N, W.M), dtype=torch.float32, device="cuda")
    dev.mul_mat_compute(W, N, out, work)
    return out


def _expected(dev, rows, K, x):
    """fl(B - T): B the two-phase product of the transcoded Q6_K weight, T the restated min term"""
    M = rows.shape[0]
    W6 = dev.Weight.from_host(Q6_K, Q2.transcode_to_q6_K(rows).reshape(M, -1), K)
    B = _two_phase(dev, W6, x).cpu().numpy()
    W6.free()
    return (B - Q2.min_term(rows, x.cpu().numpy())).astype(F)


@gpu
def test_dequantize_is_bit_exact(dev):
    import torch
    for nb in (1, 7, 64):
        for b in (_random_blocks(nb), Q2.quantize_q2_K(_rand((nb, 256), 3.0))):
            want = Q2.dequantize_q2_K(b)
            got = dev.dequantize_rows(Q2_K, torch.from_numpy(b.reshape(1, -1)).cuda(), nb * 256).cpu().numpy().reshape(-1, 256)
            assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), nb


@gpu
def test_device_quantizer_writes_the_restated_reference_quantizers_bytes(dev):
    import torch
    for (nrows, K, scale) in ((1, 256, 1.0), (7, 768, 3.0), (33, 2048, 0.01), (5, 11008, 40.0),
                              (1, 256, 3.0), (7, 768, 0.01), (33, 2048, 40.0), (5, 11008, 1.0)):
        x = _rand((nrows, K), scale)
        x[0, :256] = 0.0                                      # a zero super-block
        if nrows > 1:
            x[1] = np.abs(x[1])                               # a non-negative row: mins 0
            x[-1, 32:64] = -1.5                               # two constant sub-blocks
            x[-1, 300 % K] = 1000.0 * scale                   # one outlier
            x[-1, 512 % K:512 % K + 16] *= 1e-5               # a sub-block whose 4-bit scale rounds to 0: its first codes stay
        want = Q2.quantize_q2_K(x.reshape(-1, 256)).reshape(nrows, -1)
        got = dev.quantize_rows(Q2_K, torch.from_numpy(x).cuda()).cpu().numpy()
        assert got.shape == want.shape
        bad = np.nonzero((got != want).reshape(-1, 84).any(axis=1))[0]
        assert bad.size == 0, f"{nrows}x{K} scale {scale}: super-blocks {bad[:8]} differ"


@gpu
def test_upload_download_is_byte_exact_and_the_type_reported(dev):
    import torch
    from ggmlsharp_amd._lib import lib
    M, K = 70, 768
    rows = _random_blocks(M * K // 256).reshape(M, -1)
    W = dev.Weight.from_host(Q2_K, rows, K)
    assert lib().ggml_hip_weight_type(W.handle) == Q2_K and lib().ggml_hip_weight_rows(W.handle) == M
    assert np.array_equal(W.download().reshape(M, -1), rows)
    shard = dev.Weight.from_host(Q2_K, rows, K, row_begin=11, row_end=40)
    assert np.array_equal(shard.download().reshape(29, -1), rows[11:40])
    h = C.c_void_p()
    assert lib().ggml_hip_weight_upload(Q2_K, rows.ctypes.data_as(C.c_void_p), 700, M, 252, 0, M, None, C.byref(h)) == -3   # K % 256
    x = _rand((64, 1024))
    q = dev.quantize_rows(Q2_K, torch.from_numpy(x).cuda())
    Wd = dev.Weight.from_device(Q2_K, q, 1024)
    assert lib().ggml_hip_weight_type(Wd.handle) == Q2_K
    assert np.array_equal(Wd.download().reshape(64, -1), q.cpu().numpy())
    Ws = dev.Weight.from_device(Q2_K, q, 1024, row_begin=5, row_end=37)
    assert np.array_equal(Ws.download().reshape(32, -1), q.cpu().numpy()[5:37])
    a = _rand((20, 1024))
    got = dev.mul_mat(Wd, torch.from_numpy(a).cuda()).cpu().numpy()
    _close(got, Q2.mul_mat_q2_K(q.cpu().numpy(), a), "Q2_K from the device quantizer", 1024)
    for w in (W, shard, Wd, Ws):
        w.free()


def _pass_form(M, N):
    """the min pass's form as kquants.hip launch_q2k_min_pass picks it: 2 (two 32-column tiles per wave) once the grid of 256-column
    workgroups fills the 256 CUs, else 1"""
    return 2 if -(-N // 32) * -(-M // 256) >= 256 else 1


# every kernel family the plan picks for Q2_K: 2 the two-step mat-vec, 4 K3s (K3s-16 on short matrices: 16-row tiles), 9 the staged int8
# form, 6 K3p -- the last three also with the min pass's two-tile form (the form of every prompt-sized product of a 4096-row matrix)
FAMILY_SHAPES = [(300, 1024, 1, 2), (515, 4096, 3, 2), (300, 4096, 4, 2),
                 (300, 2048, 5, 4), (300, 2048, 16, 4), (1024, 4096, 40, 4), (4096, 4096, 64, 4), (32768, 1024, 64, 4),
                 (515, 768, 8, 9), (300, 1024, 100, 9), (130, 512, 600, 9), (4096, 1024, 512, 9),
                 (300, 2048, 1100, 6), (4096, 4096, 257, 6), (16384, 2048, 33, 6), (4096, 2048, 512, 6)]


def test_the_family_shapes_reach_both_forms_of_the_min_pass():
    forms = {(f, _pass_form(M, N)) for (M, K, N, f) in FAMILY_SHAPES}
    assert {(4, 2), (9, 2), (6, 2), (4, 1), (9, 1), (6, 1), (2, 1)} <= forms
    assert _pass_form(4096, 512) == 2 and _pass_form(1024, 512) == 1      # the shard test below crosses the switch


@gpu
@pytest.mark.parametrize("M,K,N,family", FAMILY_SHAPES)
def test_the_product_is_bitwise_the_block_term_minus_the_restated_min_term(dev, M, K, N, family):
    import torch
    assert _plan(Q2_K, M, K, N)[1].family == family
    rows = _random_blocks(M * K // 256)
    rows[::3] = Q2.quantize_q2_K(_rand((rows[::3].shape[0], 256)))
    rows = rows.reshape(M, -1)
    x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
    want = _expected(dev, rows, K, x)
    W2 = dev.Weight.from_host(Q2_K, rows, K)
    got = dev.mul_mat(W2, x).cpu().numpy()
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (M, K, N, np.abs(got - want).max())
    W2.free()


@gpu
@pytest.mark.parametrize("M,K,N", [(300, 1024, 1), (300, 2048, 16), (300, 1024, 100), (300, 2048, 1100)])
def test_with_dmin_zero_the_product_is_the_block_term(dev, M, K, N):
    import torch
    rows = _random_blocks(M * K // 256, dmin=False).reshape(M, -1)
    x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
    W6 = dev.Weight.from_host(Q6_K, Q2.transcode_to_q6_K(rows).reshape(M, -1), K)
    B = _two_phase(dev, W6, x)
    W2 = dev.Weight.from_host(Q2_K, rows, K)
    assert torch.equal(dev.mul_mat(W2, x), B), (M, K, N)
    W2.free()
    W6.free()


@gpu
def test_mul_mat_matches_the_restatement(dev):
    import torch
    for (M, K, N) in ((96, 256, 1), (300, 1024, 3), (128, 512, 8), (515, 768, 40), (256, 2048, 130), (640, 1024, 300),
                      (130, 512, 600), (257, 768, 1100), (130, 4352, 512), (300, 2048, 33), (515, 2304, 9), (130, 11008, 100)):
        for raw in (False, True):
            rows = _random_blocks(M * K // 256) if raw else Q2.quantize_q2_K(_rand((M * K // 256, 256)))
            rows = rows.reshape(M, -1)
            x = _rand((N, K))
            W = dev.Weight.from_host(Q2_K, rows, K)
            got = dev.mul_mat(W, torch.from_numpy(x).cuda()).cpu().numpy()
            _close(got, Q2.mul_mat_q2_K(rows, x), f"Q2_K {M}x{K}x{N} raw={raw}", K)
            W.free()


@gpu
def test_mul_mat_at_4096_x_11008_x_512_on_a_sample(dev):
    import torch
    M, K, N = 4096, 11008, 512
    rs = np.random.default_rng(21102)
    rows = _random_blocks(M * K // 256).reshape(M, -1)
    ms = np.sort(rs.choice(M, size=64, replace=False))
    ns = np.sort(rs.choice(N, size=64, replace=False))
    rows[ms[::2]] = Q2.quantize_q2_K(_rand((32 * K // 256, 256))).reshape(32, -1)
    x = _rand((N, K))
    W = dev.Weight.from_host(Q2_K, rows, K)
    got = dev.mul_mat(W, torch.from_numpy(x).cuda())
    _close(got.cpu().numpy()[np.ix_(ns, ms)], Q2.mul_mat_q2_K(rows[ms], x[ns]), f"Q2_K {M}x{K}x{N} (64 x 64 sample)", K)
    W.free()


@gpu
@pytest.mark.parametrize("M,K,N,family", [(300, 4096, 2, 2), (300, 2048, 40, 4), (300, 1024, 100, 9), (300, 2048, 1100, 6)])
def test_a_row_shard_is_the_bitwise_column_slice_of_the_whole(dev, M, K, N, family):
    import torch
    rows = Q2.quantize_q2_K(_rand((M * K // 256, 256))).reshape(M, -1)
    xd = torch.from_numpy(_rand((N, K))).cuda()
    assert _plan(Q2_K, M, K, N)[1].family == family and _plan(Q2_K, 160, K, N)[1].family == family
    whole = dev.mul_mat(dev.Weight.from_host(Q2_K, rows, K), xd)
    part = dev.mul_mat(dev.Weight.from_host(Q2_K, rows, K, row_begin=100, row_end=260), xd)
    assert torch.equal(part, whole[:, 100:260])


@gpu
def test_shards_that_change_the_pass_form_and_the_family_are_bitwise_column_slices(dev):
    """4096 x 2048 x 512: K3p and the two-tile pass; its 1024-row shards: K3s and the one-tile pass"""
    import torch
    M, K, N, S = 4096, 2048, 512, 1024
    assert _plan(Q2_K, M, K, N)[1].family == 6 and _plan(Q2_K, S, K, N)[1].family == 4
    assert _pass_form(M, N) == 2 and _pass_form(S, N) == 1
    rows = _random_blocks(M * K // 256)
    rows[::2] = Q2.quantize_q2_K(_rand((rows[::2].shape[0], 256)))
    rows = rows.reshape(M, -1)
    xd = torch.from_numpy(_rand((N, K))).cuda()
    whole = dev.mul_mat(dev.Weight.from_host(Q2_K, rows, K), xd)
    for r0 in range(0, M, S):
        Ws = dev.Weight.from_host(Q2_K, rows, K, row_begin=r0, row_end=r0 + S)
        assert torch.equal(dev.mul_mat(Ws, xd), whole[:, r0:r0 + S]), r0
        Ws.free()


@gpu
@pytest.mark.parametrize("M,K,N", [(300, 1024, 1), (515, 2048, 40), (4096, 1024, 512), (1000, 4352, 600), (33, 256, 2100)])
def test_the_two_forms_of_the_min_pass_are_bitwise_equal_on_the_same_inputs(dev, M, K, N):
    """the pass alone (test hook) in each form on one INIT image and one dst, strided: the same bits, fl(B - T) of the restatement, and the
    padding columns untouched"""
    import torch
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rows = _random_blocks(M * K // 256).reshape(M, -1)
    x = _rand((N, K), 2.0)
    x[0, :256] = 0.0                                                        # a zero super-block of the activations: dy = 0
    xd = torch.from_numpy(x).cuda()
    W = dev.Weight.from_host(Q2_K, rows, K)
    work = dev.alloc_work(Q2_K, K, N)
    dev.mul_mat_init(W, xd, work)
    B = _rand((N, M), 5.0)
    want = (B - Q2.min_term(rows, x)).astype(F)
    outs = []
    for form in (1, 2):
        dst = torch.full((N, M + 3), -7.0, device="cuda")
        dst[:, :M] = torch.from_numpy(B).cuda()
        _lib.check(L.ggml_hip_debug_q2k_min_pass_dev(W.handle, N, C.c_void_p(dst.data_ptr()), M + 3, C.c_void_p(work.data_ptr()),
                                                     work.numel(), form, st), f"min pass form {form}")
        assert torch.all(dst[:, M:] == -7.0), form
        outs.append(dst[:, :M].cpu().numpy())
    assert np.array_equal(outs[0].view(np.uint32), outs[1].view(np.uint32)), (M, K, N)
    assert np.array_equal(outs[0].view(np.uint32), want.view(np.uint32)), (M, K, N)
    W6 = dev.Weight.from_host(Q6_K, Q2.transcode_to_q6_K(rows).reshape(M, -1), K)
    assert L.ggml_hip_debug_q2k_min_pass_dev(W6.handle, N, C.c_void_p(dst.data_ptr()), M + 3, C.c_void_p(work.data_ptr()),
                                             work.numel(), 0, st) == _lib.ERR_TYPE
    W6.free()
    W.free()


@gpu
def test_K3p_on_a_tall_matrix_equals_its_K3s_shards_bitwise(dev):
    import torch
    M, K, N, S = 16384, 4096, 40, 1024
    assert _plan(Q2_K, M, K, N)[1].family == 6 and _plan(Q2_K, S, K, N)[1].family == 4
    g = torch.Generator(device="cuda")
    g.manual_seed(Q2_K)
    rows = dev.quantize_rows(Q2_K, torch.randn((M, K), generator=g, device="cuda"))
    xd = torch.randn((N, K), generator=g, device="cuda")
    W = dev.Weight.from_device(Q2_K, rows, K)
    whole = dev.mul_mat(W, xd)
    W.free()
    for r0 in range(0, M, S):
        Ws = dev.Weight.from_device(Q2_K, rows, K, row_begin=r0, row_end=r0 + S)
        assert torch.equal(dev.mul_mat(Ws, xd), whole[:, r0:r0 + S]), r0
        Ws.free()


@gpu
def test_multi_work_push_and_two_phase_entries_are_bitwise_the_single_calls(dev):
    import torch
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    K = 2048
    for (Ms, N) in (((300, 200), 3), ((300, 200, 130), 16), ((300, 200, 130, 77), 40), ((1024, 515, 300, 96), 600)):
        Ws = [dev.Weight.from_host(Q2_K, Q2.quantize_q2_K(_rand((M * K // 256, 256))).reshape(M, -1), K) for M in Ms]
        x = torch.from_numpy(_rand((N, K), 2.0)).cuda()
        singles = [dev.mul_mat(w, x) for w in Ws]
        hw = (C.c_void_p * len(Ws))(*[w.handle for w in Ws])
        outs = [torch.full((N, M + 4), -2.0, device="cuda") for M in Ms]
        dp = (C.c_void_p * len(Ws))(*[o.data_ptr() for o in outs])
        ld = (C.c_int64 * len(Ws))(*[M + 4 for M in Ms])
        work = dev.alloc_work(Q2_K, K, N)
        _lib.check(L.ggml_hip_mul_mat_multi_work_dev(hw, len(Ws), C.c_void_p(x.data_ptr()), K, N, dp, ld, C.c_void_p(work.data_ptr()),
                                                     work.numel(), st), "multi with work")
        for o, s, M in zip(outs, singles, Ms):
            assert torch.equal(o[:, :M], s) and torch.all(o[:, M:] == -2.0), (Ms, N)
        for w, s in zip(Ws, singles):
            assert L.ggml_hip_mul_mat_push_fused(w.handle, N, 1) == 0
            # the push entry with this device as its only peer: its own buffer gets the product
            dst = torch.full((N, w.M), -3.0, device="cuda")
            pp = (C.c_void_p * 1)(dst.data_ptr())
            _lib.check(L.ggml_hip_mul_mat_push_dev(w.handle, C.c_void_p(x.data_ptr()), N, K, pp, 1, 0, w.M, 0, C.c_void_p(work.data_ptr()),
                                                   work.numel(), st), "push")
            assert torch.equal(dst, s), (w.M, N)
            # INIT + COMPUTE into a strided dst: the product in the first M columns, the padding untouched
            wide = torch.full((N, w.M + 7), -5.0, device="cuda")
            dev.mul_mat_init(w, x, work)
            dev.mul_mat_compute(w, N, wide[:, :w.M], work)
            assert torch.equal(wide[:, :w.M], s) and torch.all(wide[:, w.M:] == -5.0), (w.M, N)
        for w in Ws:
            w.free()


@gpu
def test_the_epilogue_entry_runs_the_pass_before_the_epilogue(dev):
    import torch
    L = _lib.lib()
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    M, K = 300, 2048
    W = dev.Weight.from_host(Q2_K, Q2.quantize_q2_K(_rand((M * K // 256, 256))).reshape(M, -1), K)
    for N in (1, 16, 600):
        x = torch.from_numpy(_rand((N, K))).cuda()
        prod = dev.mul_mat(W, x)
        work = dev.alloc_work(Q2_K, K, N)
        addend = torch.from_numpy(_rand((N, M))).cuda()
        out, out2 = torch.empty((N, M), device="cuda"), torch.empty((N, M), device="cuda")
        _lib.check(L.ggml_hip_mul_mat_epilogue_dev(W.handle, C.c_void_p(x.data_ptr()), N, K, C.c_void_p(out.data_ptr()), M,
                                                   C.c_void_p(work.data_ptr()), work.numel(), 1, C.c_void_p(addend.data_ptr()), M,
                                                   C.c_void_p(out2.data_ptr()), M, C.c_float(1.0), st), "epilogue add")
        assert torch.equal(out, prod) and torch.equal(out2, prod + addend), N
    W.free()
