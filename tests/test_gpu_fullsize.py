"""BASELINE.json's full-size configurations on the GPU (-m gpu).  The CPU oracle needs minutes at these sizes, so
parity is established through size-independent properties:
  * the HIP result equals an fp64 evaluation of the same arithmetic -- sum over blocks of d_w * d_a * (integer block
    dot) -- computed from operands dequantised by the bit-exact device kernels (themselves pinned to the oracle in
    test_gpu_parity.py), within 1e-3 relative (observed ~3e-6 of the rms);
  * row-split consistency: a row shard's result is bitwise the matching columns of the unsplit result (what the
    multi-GPU path relies on), and a src1 row subset gives bitwise the matching dst rows;
  * re-layout round trips are byte-exact and quantize(dequantize(q)) is a fixed point for Q8_0.
On top of the properties every configuration MEETS THE ORACLE on a sample (round 3): 64 weight rows x 64 src1 rows = 4096 outputs
whose operands are quantized on the host by the oracle (the device quantizer's bytes must equal them) and multiplied by
oracle_vec_dot -- the reference's scalar loop, block by block -- under SURVEY 8(c)'s metric.
"""
import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

Q4_0, Q5_0, Q8_0 = 2, 6, 8


@pytest.fixture(scope="module")
def dev():
    from ggmlsharp_amd import device
    device.init(0)
    return device


def _make(dev, t, M, K, N, seed, keep_w=False):
    g = torch.Generator(device="cuda")
    g.manual_seed(seed)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    rows = dev.quantize_rows(t, w)
    return (rows, x, w) if keep_w else (rows, x)


def _check_oracle_sample(t, rows, w, x, got, K, seed, nm=64, nn=64):
    """nm x nn outputs of a full-size product against the CPU oracle: the sampled weight rows and src1 rows are quantized by the
    oracle's quantize_row (Ggml.cs:334-377 / 609-653 / 733-762 ...) on the host -- the device quantizer's bytes for those rows
    must be the same bytes -- and every sampled output is oracle_vec_dot of the two block rows (Ggml.cs:1125-1162 ...).
    Metric: SURVEY 8(c), |gpu - ref| <= 1e-3 * max(|ref|, 1e-3 * rms) per element and <= 1e-3 norm-wise.  One stated widening:
    the floor term.  The reference adds its K / 32 block terms one after the other in f32; ANY other order of the same f32 terms
    (and every kernel here has one: K split over waves or stage sets) moves a sum by a few ulps of its largest partial sum, i.e.
    by up to ~ eps * sqrt(K / 32) * rms whatever the size of the result, so on outputs that happen to cancel to |ref| < 1e-3 rms
    the survey's floor of 1e-6 rms asks for more than f32 reordering can give.  The floor used is 8 * 2^-24 * sqrt(K / 32) * rms
    (5.4e-6 rms at K = 4096); above |ref| = 1e-2 rms the bound is the survey's, unchanged."""
    M, N = w.shape[0], x.shape[0]
    rs = np.random.default_rng(seed)
    ms = np.sort(rs.choice(M, size=min(nm, M), replace=False))
    ns = np.sort(rs.choice(N, size=min(nn, N), replace=False))
    wq = O.quantize_row(t, w[torch.from_numpy(ms).cuda()].cpu().numpy())
    dev_rows = rows[torch.from_numpy(ms).cuda()].cpu().numpy().reshape(len(ms), -1)
    assert np.array_equal(dev_rows, wq), "device quantizer differs from the oracle on sampled full-size rows"
    vt = O.lib().oracle_vec_dot_type(t)
    xq = O.quantize_row(vt, x[torch.from_numpy(ns).cuda()].cpu().numpy())
    ref = np.zeros((len(ns), len(ms)), dtype=np.float64)
    for a in range(len(ns)):
        for b in range(len(ms)):
            ref[a, b] = O.vec_dot(t, K, wq[b], xq[a])
    g = got[torch.from_numpy(ns).cuda()][:, torch.from_numpy(ms).cuda()].double().cpu().numpy()
    O.assert_mul_mat_close(g, ref, K, "sampled outputs of a full-size product")


def _check_dense_oracle_sample(t, w_raw, x, got, K, seed, nm=48, nn=48):
    """nm x nn outputs of a full-size DENSE product against the CPU oracle's mul_mat on the sampled weight rows and src1 rows
    (ggml_compute_forward_mul_mat_f32 / _f16_f32, Ggml.cs:5969-6178 / 6180-6438: f32 or Half products, f64 running sum).
    SURVEY 8(c)'s metric with the floor of the quantized samples: the kernels sum in f32, not f64."""
    M, N = w_raw.shape[0], x.shape[0]
    rs = np.random.default_rng(seed)
    ms = np.sort(rs.choice(M, size=min(nm, M), replace=False))
    ns = np.sort(rs.choice(N, size=min(nn, N), replace=False))
    ws = w_raw[torch.from_numpy(ms).cuda()].cpu().numpy()
    xs = x[torch.from_numpy(ns).cuda()].cpu().numpy()
    wo = ws if t == O.F32 else ws.view(np.uint16)
    ref = O.mul_mat(t, np.ascontiguousarray(wo), np.ascontiguousarray(xs), len(ms), K, len(ns), nth=4)[0, 0].astype(np.float64)
    g = got[torch.from_numpy(ns).cuda()][:, torch.from_numpy(ms).cuda()].double().cpu().numpy()
    O.assert_mul_mat_close(g, ref, K, "sampled outputs of a full-size dense product")


def _assert_close_dev(got, ref, K, what=""):
    """tests/oracle_lib.assert_mul_mat_close (THE mul_mat tolerance: SURVEY 8(c) with its one stated floor), evaluated on the device
    for whole full-size results; ref fp64 [N][M]"""
    err = (got.double() - ref).abs()
    rms = ref.pow(2).mean().sqrt().item()
    floor = max(1e-6, 8 * 2.0 ** -24 * float(np.sqrt(K / 32))) * rms
    bound = (1e-3 * ref.abs()).clamp_min(floor)
    bad = (~(err <= bound)).sum().item()
    assert bad == 0, f"{what}: {bad} elements beyond SURVEY 8(c); max err / rms = {err.max().item() / rms:.3e}"
    assert (torch.linalg.norm(got.double() - ref) / torch.linalg.norm(ref)).item() <= 1e-3


def _check_fp64(dev, t, rows, x, got, K):
    wd = dev.dequantize_rows(t, rows, K).double()
    xq = dev.dequantize_rows(Q8_0, dev.quantize_rows(Q8_0, x.contiguous()), K).double()
    ref = xq @ wd.T
    _assert_close_dev(got, ref, K, "fp64 evaluation of the block arithmetic")
    assert ((got.double() - ref).abs().max() / ref.pow(2).mean().sqrt()).item() < 1e-4


CONFIGS = [  # BASELINE.json configs (M, K, N), Q5_0 standing in for the absent Q5_K
    ("c2 batch-1", Q4_0, 4096, 4096, 1),
    ("c3 prompt-512", Q4_0, 4096, 4096, 512),
    ("metric 4096^3", Q4_0, 4096, 4096, 4096),
    ("c4a", Q8_0, 4096, 11008, 512),
    ("c4b", Q5_0, 4096, 11008, 512),
    ("c4a transposed reading", Q8_0, 11008, 4096, 512),
    ("c5 single-GPU total", Q4_0, 32000, 4096, 512),
    # the other forms at full size: Q4_1 (MX + min term), the SURVEY-D7 types on the int8 kernel and the mat-vec kernel,
    # a 16-row decode batch (two-step mat-vec form)
    ("q4_1 prompt-512", 3, 4096, 4096, 512),
    ("q4_2 prompt-512", 4, 4096, 4096, 512),
    ("q5_1 ffn-512", 7, 4096, 11008, 512),
    ("q5_1 batch-1", 7, 11008, 4096, 1),
    ("q4_2 batch-8", 4, 4096, 4096, 8),
    ("decode batch of 16", Q4_0, 11008, 4096, 16),
    # Q5_0 / Q5_1 / Q8_0 above 512 rows: int8 kernel below 1024 rows, the f16 kernel's unsplit forms from there (both tile shapes)
    ("q5_0 700 rows", Q5_0, 4096, 4096, 700),
    ("q5_1 1024 rows", 7, 4096, 4096, 1024),
    ("q8_0 4096^3", Q8_0, 4096, 4096, 4096),
    # r5: the min-term types at LONG K against the oracle.  K3p adds the block terms and the min terms apart and they
    # nearly cancel, so the reordering error grows with sqrt(K) -- K = 20480 is the last K on one scale table, 28672 runs the sliced
    # tables + the min-term product over 112 chunks (a 70B model's down projection at prompt size)
    ("q5_1 K=28672 prompt-512 (sliced K3p + min-term product)", 7, 4096, 28672, 512),
    ("q4_1 K=28672 prompt-512", 3, 4096, 28672, 512),
    ("q5_1 K=20480 prompt-512", 7, 2048, 20480, 512),
    ("q5_1 K=28672 batch of 32 (K3s + min-term product)", 7, 4096, 28672, 32),
]


@pytest.mark.parametrize("name,t,M,K,N", CONFIGS)
def test_fullsize_matches_fp64_block_arithmetic(dev, name, t, M, K, N):
    rows, x, w = _make(dev, t, M, K, N, seed=M + K + N, keep_w=True)
    W = dev.Weight.from_device(t, rows, K)
    got = dev.mul_mat(W, x)
    _check_fp64(dev, t, rows, x, got, K)
    _check_oracle_sample(t, rows, w, x, got, K, seed=M + N)
    W.free()


@pytest.mark.parametrize("M,K,N", [(4096, 4096, 4096), (2048, 4096 + 40, 2048 + 17), (4096, 11008, 512)])
def test_dense_f16_fullsize_matches_fp64(dev, M, K, N):
    """ggml_compute_forward_mul_mat_f16_f32 (Ggml.cs:6180-6438) at sizes served by the f16 MFMA kernel (dense16.hip): src1 is
    rounded to Half in INIT (:6362-6379), the products are exact, the sum is f32 here and f64 in the reference."""
    g = torch.Generator(device="cuda")
    g.manual_seed(M + N)
    w = torch.randn((M, K), generator=g, device="cuda").half()
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    W = dev.Weight.from_device(1, w.contiguous().view(torch.uint8), K)
    got = dev.mul_mat(W, x)
    ref = x.half().double() @ w.double().T
    _assert_close_dev(got, ref, K)
    assert np.array_equal(W.download(), w.cpu().numpy().view(np.uint8).reshape(-1))      # the row-major copy still round-trips
    _check_dense_oracle_sample(O.F16, w, x, got, K, seed=M + N)
    W.free()


@pytest.mark.parametrize("M,K,N", [(2048, 1056, 2048 + 17), (4096, 512, 4096), (2000, 1024, 64), (4096, 4096, 4096)])
def test_dense_f32_fullsize_matches_fp64(dev, M, K, N):
    """ggml_compute_forward_mul_mat_f32 (Ggml.cs:5969-6178; dot 2631-2640: f32 products, f64 sum) at sizes served by the
    split-bf16 kernel of dense16.hip (more than 256 src1 rows: six bf16 MFMAs per product, K10d) and by dense.hip's 64 x 64 tiles (the
    third: f32 fma chain in k order); sampled outputs also against the CPU oracle."""
    g = torch.Generator(device="cuda")
    g.manual_seed(M + N)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    W = dev.Weight.from_device(0, w.contiguous().view(torch.uint8), K)
    got = dev.mul_mat(W, x)
    ref = x.double() @ w.double().T
    _assert_close_dev(got, ref, K)
    # a row shard goes through the other tile size (fewer tiles): same k order, same bits
    Ws = dev.Weight.from_device(0, w.contiguous().view(torch.uint8), K, row_begin=128, row_end=640)
    assert torch.equal(dev.mul_mat(Ws, x), got[:, 128:640])
    Ws.free()
    _check_dense_oracle_sample(O.F32, w, x, got, K, seed=M + N)
    W.free()


def test_row_shard_and_column_subset_are_bitwise_slices(dev):
    M, K, N = 4096, 4096, 512
    rows, x = _make(dev, Q4_0, M, K, N, seed=3)
    W = dev.Weight.from_device(Q4_0, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((0, 512), (512, 1024), (3584, 4096), (1000, 1777)):     # 8-way split pieces and a ragged one
        Ws = dev.Weight.from_device(Q4_0, rows, K, row_begin=r0, row_end=r1)
        part = dev.mul_mat(Ws, x)
        assert torch.equal(part, full[:, r0:r1]), (r0, r1)
        Ws.free()
    sub = dev.mul_mat(W, x[128:512].contiguous())                            # 384 rows: the same two-way K split as 512
    assert torch.equal(sub, full[128:512])
    one = dev.mul_mat(W, x[7:8].contiguous())                                # N = 1 goes through the mat-vec kernel
    err = (one - full[7:8]).abs().max() / full[7:8].abs().max()
    assert err < 1e-5                                                        # different kernel, different summation tree
    W.free()


@pytest.mark.parametrize("t,N", [(Q5_0, 512), (Q8_0, 512), (Q8_0, 640), (Q8_0, 1024), (Q8_0, 4096), (7, 1024), (Q4_0, 2048), (Q4_0, 3)])
def test_row_shards_are_bitwise_slices_for_every_kernel_form(dev, t, N):
    """The kernel form (MX / f16 with or without the K split / int8 / mat-vec) is chosen from the type, N and K -- never
    from M -- so a row shard computes bit for bit the matching columns of the unsplit result, whatever serves the shape."""
    M, K = 4096, 1024
    rows, x = _make(dev, t, M, K, N, seed=11 + N)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((0, 512), (3584, 4096), (777, 2000)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, N, r0, r1)
        Ws.free()
    W.free()


@pytest.mark.parametrize("t", [Q8_0, Q5_0, Q4_0, 3, 4, 7])
@pytest.mark.parametrize("K,N", [(4096, 32), (4096, 16), (4096, 5), (2048, 24), (11008, 32), (6144, 31), (4096 + 64, 17), (28672, 9), (32768, 32)])
def test_k3s_16_row_tiles_are_bitwise_the_32_row_form(dev, t, K, N):
    """r5: the batched-decode forms run 16-row tiles where 32-row tiles leave CUs idle -- GEOMETRY that follows M, on the
    tree of the 32-row form (the same eight K ranges, block order, statement per block and wave-order sum).  So the plan's tree_id is the
    same for both, a 16384-row matrix (32-row tiles, two per workgroup) and its 4096-row / ragged shards (16-row tiles) agree BIT FOR BIT --
    and both meet the oracle sample and the fp64 evaluation.  Covers both slice counts (16 / 32 columns per workgroup), one table
    round and several (K = 11008, 28672), ragged N, and a K whose last k-blocks fall short of a wave's range."""
    from ggmlsharp_amd import _lib
    import ctypes as C
    M = 16384
    pa, pb = _lib.ggml_hip_mm_plan_t(), _lib.ggml_hip_mm_plan_t()
    assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(pa)) == 0 and _lib.lib().ggml_hip_mm_plan(t, 4096, K, N, C.byref(pb)) == 0
    assert pa.tree_id == pb.tree_id and pa.family == pb.family
    if pa.family not in (3, 4):
        pytest.skip("this type's mat-vec serves the shape (Q4_2 up to 8 rows)")
    assert pa.tile_m >= 32 and pb.tile_m == 16, (pa.tile_m, pb.tile_m)          # the two geometries really are different kernels
    rows, x, w = _make(dev, t, M, K, N, seed=K + N + t, keep_w=True)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((0, 4096), (4096, 8192), (12288, 12288 + 4000), (100, 100 + 1777), (16000, 16384)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        part = dev.mul_mat(Ws, x)
        assert torch.equal(part, full[:, r0:r1]), (t, K, N, r0, r1)
        if r0 == 0:
            _check_fp64(dev, t, rows[r0:r1], x, part, K)
            _check_oracle_sample(t, rows[r0:r1], w[r0:r1], x, part, K, seed=K + N)
        Ws.free()
    W.free()


@pytest.mark.parametrize("t,N", [(Q4_0, 32), (Q4_0, 24), (Q8_0, 24), (Q5_0, 32), (3, 32), (3, 64), (7, 32), (4, 32)])
def test_every_batched_decode_geometry_computes_the_same_bits(dev, t, N):
    """the batched-decode forms pick their geometry from M -- 16-row tiles (r5), one, two or four 32-row tiles per workgroup -- and the
    CPU plan test can only see that the LABELS agree.  Here every geometry really runs: a 33000-row matrix (four tiles per workgroup for Q4_0, two
    for the others) and shards of 12000 rows (two), 6000 rows (one) and 4096 / 1000 rows (16-row tiles where the type has them) must agree bit
    for bit, in the product build, with no developer switch."""
    from ggmlsharp_amd import _lib
    import ctypes as C
    M, K = 33000, 4096
    rows, x = _make(dev, t, M, K, N, seed=5 * N + t)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    seen = set()
    for (r0, r1) in ((0, 33000), (0, 12000), (12000, 18000), (18000, 22096), (32000, 33000), (22096, 22096 + 257)):
        pl = _lib.ggml_hip_mm_plan_t()
        assert _lib.lib().ggml_hip_mm_plan(t, r1 - r0, K, N, C.byref(pl)) == 0 and pl.family in (3, 4), (t, N, pl.family)
        seen.add((pl.tile_m, pl.tile_n))
        if (r0, r1) == (0, 33000):
            continue
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, N, r0, r1, pl.tile_m, pl.tile_n)
        Ws.free()
    assert len(seen) >= 2, seen                             # (the geometries really differed)
    W.free()


@pytest.mark.parametrize("K", [512, 544, 1056, 2080])
@pytest.mark.parametrize("N", [130, 256])
def test_banked_four_way_tree_matches_the_real_split(dev, K, N):
    """Q4_0, 129..256 rows: an 8192-row matrix runs the four-way summation tree as banked passes (two wave groups, two stage
    sets each), a 1024-row shard runs it really split.  Stage counts that do not divide by four (K = 544: 5 stages, 1056: 9,
    2080: 17) leave the stage sets unequal -- the bits must still agree, and match fp64."""
    M = 8192
    rows, x = _make(dev, Q4_0, M, K, N, seed=K + N)
    W = dev.Weight.from_device(Q4_0, rows, K)
    full = dev.mul_mat(W, x)
    _check_fp64(dev, Q4_0, rows, x, full, K)
    for (r0, r1) in ((0, 1024), (5000, 6024), (8000, 8192)):
        Ws = dev.Weight.from_device(Q4_0, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (K, N, r0, r1)
        Ws.free()
    W.free()


@pytest.mark.parametrize("N", [100, 200])
def test_small_batch_tile_forms_agree_bitwise(dev, N):
    """Batches up to 128 rows: the K split (four wave groups) is fixed by N and K, the tile height by how many tiles there are --
    32-row tiles for a 2048-row shard, 64-row tiles of 8 waves for an 8192-row shard, 128-row tiles of 16 waves for the
    16384-row matrix.  Same split, same order of the partial sums: a shard is bit for bit the matching columns of the unsplit
    result.  (Q4_1 and Q8_0: the f16 / min-term variants of the same rule.)"""
    M, K = 16384, 1024
    # (N = 200, Q4_0 / Q4_1: the four-way tree again -- really split for the shards, two wave groups running two stage sets each
    # for the whole matrix)
    for t in (Q4_0, 3, Q8_0):
        rows, x = _make(dev, t, M, K, N, seed=5 + t)
        W = dev.Weight.from_device(t, rows, K)
        full = dev.mul_mat(W, x)
        _check_fp64(dev, t, rows, x, full, K)
        for (r0, r1) in ((0, 2048), (8000, 9000), (0, 8192)):
            Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
            assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, r0, r1)
            Ws.free()
        W.free()


@pytest.mark.parametrize("N", [5, 9, 20, 32, 40, 64])
def test_batched_decode_form_follows_M_only_in_its_geometry(dev, N):
    """Batches of 5 to 64 rows (two 32-column slices above 32), K >= 2048 (gemm_qmx.hip K3s): eight waves with a contiguous eighth of K each, their sums added
    in wave order -- fixed by N and K.  One 32-row tile per workgroup while there are at most 256 tiles, two above, four (Q4_0)
    above 512: a shard is bit for bit the matching columns of the unsplit result.  K = 2048 holds a wave's range in its slots, 4096 + 64 and 6144
    refill them in turn."""
    # (16424 rows = 514 tiles: four per workgroup for Q4_0; 8492 rows: two)
    for (t, M, K) in ((Q4_0, 16384 + 40, 2048), (3, 8192 + 300, 4096 + 64), (Q4_0, 8192 + 300, 2048), (Q4_0, 300, 6144), (3, 100, 2048 + 32),
                      (Q8_0, 8192 + 300, 2048), (Q8_0, 300, 4096), (Q8_0, 130, 2048 + 64), (Q8_0, 8192 + 300, 4096 + 64), (Q8_0, 200, 11008)):   # (Q8_0: the int8 form of the same, gemm_q.hip)
        rows, x = _make(dev, t, M, K, N, seed=11 + t + N)
        W = dev.Weight.from_device(t, rows, K)
        full = dev.mul_mat(W, x)
        _check_fp64(dev, t, rows, x, full, K)
        for (r0, r1) in ((0, 2048), (M - 77, M), (0, min(M, 8192)), (31, 290)):
            if r1 > M:
                continue
            Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
            assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, M, K, N, r0, r1)
            Ws.free()
        W.free()


@pytest.mark.parametrize("N", [100, 300, 1536 + 5])
def test_dense_f16_tile_forms_agree_bitwise(dev, N):
    """F16 weights: the K split of a batch (four ways up to 128 rows, two ways up to 512) and the MFMA shape (16 x 16 x 32 above
    512 rows) are fixed by N and K, the tile shape by the number of tiles -- a 2048-row shard and the 16384-row matrix run
    different tiles (above 512 rows: 256 x 128 against 128 x 128 workgroup tiles) and must agree bit for bit."""
    M, K = 16384, 2048
    g = torch.Generator(device="cuda")
    g.manual_seed(3 + N)
    w = torch.randn((M, K), generator=g, device="cuda").half()
    x = torch.randn((N, K), generator=g, device="cuda")
    rows = w.view(torch.uint8).view(M, -1)
    W = dev.Weight.from_device(1, rows, K)
    full = dev.mul_mat(W, x)
    ref = x.half().double() @ w.double().T
    err = (full.double() - ref).abs()
    assert (err.max() / ref.pow(2).mean().sqrt()).item() < 1e-4
    for (r0, r1) in ((0, 2048), (9000, 9700)):
        Ws = dev.Weight.from_device(1, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1])
        Ws.free()
    W.free()


@pytest.mark.parametrize("t,kernel", [(7, 0), (3, 2)])
def test_min_term_types_tall_matrix_and_its_shards_add_in_one_order(dev, t, kernel):
    """Q5_1 (and Q4_1 when forced onto the f16 kernel) above 512 src1 rows: the 8-tile form added the min term per block on the VALU, the
    2-tile form per pair of blocks on the matrix pipe -- the same terms in another order -- and which form runs follows M.  A 26000-row
    matrix and its shard differed in the last bits (tools/sweep_parity.py with row shards, r3); the order now follows the K split, i.e. N."""
    from ggmlsharp_amd._lib import lib
    M, K, N = 26000, 1024, 600
    g = torch.Generator(device="cuda")
    g.manual_seed(t)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    rows = dev.quantize_rows(t, w)
    lib().ggml_hip_debug_force_gemm(kernel)
    try:
        W = dev.Weight.from_device(t, rows, K)
        full = dev.mul_mat(W, x)
        for (r0, r1) in ((0, 4000), (25000, 26000)):
            Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
            assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, r0, r1)
            Ws.free()
        W.free()
    finally:
        lib().ggml_hip_debug_force_gemm(0)


@pytest.mark.parametrize("t", [Q4_0, 3, 4, Q5_0, 7, Q8_0])
@pytest.mark.parametrize("N", [300, 512])
def test_k3p_forms_tall_matrix_and_its_shards_are_bitwise_slices(dev, t, N):
    """257..512 src1 rows, K >= 2048 (gemm_qmp.hip): eight K ranges per workgroup whatever M -- a vocabulary-sized matrix (persistent
    workgroups: more than four rounds of tiles), a 4000-row shard (one dispatch round) and a ragged shard compute the same bits.
    r4: Q5_1 (min term per pair of k-blocks on the matrix pipe) and Q4_1 run the form too; r5: Q4_2 (two K = 16 products and two
    scale-accumulates per k-block)."""
    M, K = 26000, 2048
    g = torch.Generator(device="cuda")
    g.manual_seed(100 * t + N)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    rows = dev.quantize_rows(t, w)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    _check_fp64(dev, t, rows, x, full, K)
    for (r0, r1) in ((0, 4000), (25000, 26000), (12345, 12345 + 777)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, N, r0, r1)
        Ws.free()
    W.free()


@pytest.mark.parametrize("K,N", [(4096, 128), (4096, 65), (11008, 100), (2048 + 64, 128), (2048, 96), (22016, 96), (4096, 256), (11008, 200), (4096, 512), (4096, 48), (11008, 33)])
def test_k3s_and_k3p_mx_compute_the_same_bits(dev, K, N):
    """r5: Q4_0's stage-free forms on the MX cores -- K3s (pairs of k-blocks per operand set) and K3p (one k-block per trip) -- are one tree as well: the same
    eight K ranges of an even number of k-blocks, acc += (sumi * d1) * d0 block by block, the eight sums in wave order.  Between 33 and 512 src1 rows the
    plan picks by M; a tall matrix (K3p) and its short shards (K3s) agree BIT FOR BIT, the short form meets fp64 and the oracle sample.  K with an odd
    number of k-blocks per eighth (11008), a ragged last range (2112), the smallest K of the forms (2048), sliced scale tables on the K3p side (22016)."""
    from ggmlsharp_amd import _lib
    import ctypes as C
    t = Q4_0
    M = 16384 if K <= 11008 else 12288
    pa, pb = _lib.ggml_hip_mm_plan_t(), _lib.ggml_hip_mm_plan_t()
    assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(pa)) == 0 and _lib.lib().ggml_hip_mm_plan(t, 1024, K, N, C.byref(pb)) == 0
    assert (pa.family, pb.family) == (5, 3) and pa.tree_id == pb.tree_id, (pa.family, pb.family)     # 5 = K3p-MX, 3 = K3s-MX
    rows, x, w = _make(dev, t, M, K, N, seed=3 * K + N + t, keep_w=True)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((0, 1024), (5000, 5000 + 2000), (M - 700, M), (777, 777 + 333)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        pl = _lib.ggml_hip_mm_plan_t()
        assert _lib.lib().ggml_hip_mm_plan(t, r1 - r0, K, N, C.byref(pl)) == 0 and pl.family in (3, 5) and (r0 != 0 or pl.family == 3)
        part = dev.mul_mat(Ws, x)
        assert torch.equal(part, full[:, r0:r1]), (N, K, r0, r1)
        if r0 == 0:
            _check_fp64(dev, t, rows[r0:r1], x, part, K)
            _check_oracle_sample(t, rows[r0:r1], w[r0:r1], x, part, K, seed=K + N)
        Ws.free()
    W.free()


@pytest.mark.parametrize("t", [Q8_0, Q5_0, 7, 4, 3])
@pytest.mark.parametrize("K,N", [(4096, 128), (4096, 65), (11008, 100), (2048 + 64, 256), (4096, 200), (22016, 96), (4096, 512), (4096, 48)])
def test_k3s_and_k3p_int8_compute_the_same_bits(dev, t, K, N):
    """r5: between 33 and 512 src1 rows the plan picks K3s-int8 or K3p-int8 by M -- allowed because the two families are one
    summation tree: the same eight K ranges (an even number of k-blocks per wave), a range's min-term chunks and blocks in the same order with the
    same statement, the eight sums added in wave order.  Here both really run: a tall matrix (K3p) and its short shards (K3s) agree BIT FOR BIT; the
    short form also meets fp64 and the oracle sample.  Q8_0, Q5_0, the min-term types Q5_1 and Q4_1 (from 65 rows on this pair; its MX form below) and the two-scale type Q4_2; K with an odd number of
    k-blocks per eighth (11008: 43 -> 44), a ragged last range (2112) and sliced scale tables on the K3p side (22016)."""
    from ggmlsharp_amd import _lib
    import ctypes as C
    if t == 3 and (N <= 64 or (K >= 11008 and N <= 128)):
        pytest.skip("Q4_1 keeps its MX batched-decode form up to 64 rows (behind K >= 11008: up to 128)")
    M = 16384 if K <= 11008 else 12288
    pa, pb = _lib.ggml_hip_mm_plan_t(), _lib.ggml_hip_mm_plan_t()
    assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(pa)) == 0 and _lib.lib().ggml_hip_mm_plan(t, 1024, K, N, C.byref(pb)) == 0
    assert (pa.family, pb.family) == (6, 4) and pa.tree_id == pb.tree_id, (pa.family, pb.family)     # 6 = K3p-int8, 4 = K3s-int8
    rows, x, w = _make(dev, t, M, K, N, seed=3 * K + N + t, keep_w=True)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((0, 1024), (5000, 5000 + 2000), (M - 700, M), (777, 777 + 333)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        pl = _lib.ggml_hip_mm_plan_t()
        assert _lib.lib().ggml_hip_mm_plan(t, r1 - r0, K, N, C.byref(pl)) == 0 and pl.family in (4, 6) and (r0 != 0 or pl.family == 4)   # (a 2000-row shard at 512 src1 rows is K3p again)
        part = dev.mul_mat(Ws, x)
        assert torch.equal(part, full[:, r0:r1]), (t, N, K, r0, r1)
        if r0 == 0:
            _check_fp64(dev, t, rows[r0:r1], x, part, K)
            _check_oracle_sample(t, rows[r0:r1], w[r0:r1], x, part, K, seed=K + N)
        Ws.free()
    W.free()


@pytest.mark.parametrize("t", [Q4_0, 3, Q8_0, Q5_0, 7, 4])
@pytest.mark.parametrize("K,N", [(1024, 16), (1024, 64), (1280, 33), (1536, 32), (1792, 9), (2016, 24)])
def test_batched_decode_forms_behind_a_short_K(dev, t, K, N):
    """r5: the batched-decode forms from K = 1024 (a small model's hidden size; it was 2048) up to 64 src1 rows: four to eight k-blocks per wave, slots
    past a wave's range repeating a valid block under a zero table row.  K with an odd number of k-blocks per eighth (1280: 5 -> 6) and a ragged last range
    (2016: 63 k-blocks).  fp64 evaluation of the block arithmetic, the oracle sample, and row shards -- 16-row tiles, one and several 32-row tiles per
    workgroup -- are the bitwise slices of an 18000-row matrix."""
    from ggmlsharp_amd import _lib
    import ctypes as C
    if t in (7, 4) and N < 9:
        pytest.skip("this type's mat-vec serves up to 8 rows")
    M = 18000
    pl = _lib.ggml_hip_mm_plan_t()
    assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(pl)) == 0 and pl.family in (3, 4), (t, K, N, pl.family)
    rows, x, w = _make(dev, t, M, K, N, seed=K + 7 * N + t, keep_w=True)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((0, 3000), (3000, 3000 + 4096), (9000, 9000 + 777), (M - 100, M)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        part = dev.mul_mat(Ws, x)
        assert torch.equal(part, full[:, r0:r1]), (t, K, N, r0, r1)
        if r0 == 0:
            _check_fp64(dev, t, rows[r0:r1], x, part, K)
            _check_oracle_sample(t, rows[r0:r1], w[r0:r1], x, part, K, seed=K + N)
        Ws.free()
    W.free()


@pytest.mark.parametrize("t", [Q4_0, Q8_0, 7, 4])
def test_k3s_and_k3p_agree_on_zero_rows_and_zero_blocks(dev, t):
    """The two families pad their K ranges differently (K3s repeats a valid block under a zero table row, K3p reads zero planes past the end), so the
    claim "the same bits" leans on x + 0 = x and on sums that never become -0.  Inputs that reach for the corners: src1 rows that are all zero (d = 0,
    every term 0 * d0), weight rows that are all zero, a K with a ragged last range, negative-only data; K3p on the tall matrix, K3s on its shards: bit
    for bit, and the all-zero rows / columns give +0.0 exactly (sign bit clear)."""
    from ggmlsharp_amd import _lib
    import ctypes as C
    M, K, N = 16384, 2048 + 96, 96
    g = torch.Generator(device="cuda")
    g.manual_seed(77 + t)
    w = -torch.rand((M, K), generator=g, device="cuda") - 0.01          # negative-only weights
    x = torch.randn((N, K), generator=g, device="cuda")
    w[5::97] = 0.0
    x[3::11] = 0.0
    x[:, 1024:1056] = 0.0                                                # a zero k-block in every src1 row
    rows = dev.quantize_rows(t, w)
    pa, pb = _lib.ggml_hip_mm_plan_t(), _lib.ggml_hip_mm_plan_t()
    assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(pa)) == 0 and _lib.lib().ggml_hip_mm_plan(t, 1000, K, N, C.byref(pb)) == 0
    assert pa.family in (5, 6) and pb.family in (3, 4) and pa.tree_id == pb.tree_id
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    assert torch.isfinite(full).all()
    zero_bits = full[3::11].view(torch.int32)
    assert int((zero_bits != 0).sum()) == 0, "an all-zero src1 row must give +0.0 exactly"
    if t in (Q4_0, Q8_0):                                                # (the min-term types' zero rows keep their min term; Q4_2's scales are its own)
        assert int((full[:, 5::97].view(torch.int32) != 0).sum()) == 0
    for (r0, r1) in ((0, 1000), (4000, 4000 + 900), (M - 333, M)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x).view(torch.int32), full[:, r0:r1].contiguous().view(torch.int32)), (t, r0, r1)
        Ws.free()
    _check_fp64(dev, t, rows[:1000], x, full[:, :1000].contiguous(), K)
    W.free()


@pytest.mark.parametrize("t,N,K", [(Q8_0, 192, 4096), (Q5_0, 129, 4096), (7, 256, 4096), (3, 300, 2048), (Q8_0, 512, 11008), (7, 200, 22016), (Q5_0, 160, 2048 + 64),
                                   (4, 129, 4096), (4, 512, 11008), (4, 200, 22016),
                                   (Q4_0, 512, 4096), (Q4_0, 257, 2048 + 64), (Q4_0, 400, 22016)])
def test_k3p_64_row_wave_tiles_are_bitwise_the_128_row_form(dev, t, N, K):
    """r5: K3p (both kernels: MX for Q4_0, int8 for the others) runs 64-row wave tiles (two m-tiles per wave) where a grid of 128-row tiles leaves CUs idle -- 4096 rows at 129..256
    src1 rows were 96..128 workgroups.  Geometry on K3p's tree (the same eight K ranges, block order, statement, wave-order sum; the min-term
    chunks go to the same waves): an 8192-row matrix (128-row tiles) and its shards of 4096 / 2048 / ragged rows (64-row tiles) agree bit for
    bit; the plan's tree_id is one; fp64 and the oracle sample hold for the 64-row form.  One scale table and sliced ones (K = 22016)."""
    from ggmlsharp_amd import _lib
    import ctypes as C
    pa, pb = _lib.ggml_hip_mm_plan_t(), _lib.ggml_hip_mm_plan_t()
    for M in (8192, 12288, 16384, 32768):                    # the smallest matrix of the list whose grid the plan gives 128-row tiles
        assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(pa)) == 0
        if pa.tile_m == 128:
            break
    # (short matrices run K3s up to 512 src1 rows -- the same tree, test_k3s_and_k3p_*_compute_the_same_bits)
    for Ms in (2048, 3072, 4096):                            # the smallest shard the plan gives K3p at all (192 workgroups of 64 rows; Q4_1 has no K3s on this arithmetic: 2048)
        assert _lib.lib().ggml_hip_mm_plan(t, Ms, K, N, C.byref(pb)) == 0
        if pb.family == pa.family:
            break
    assert pa.family == pb.family and pa.family in (5, 6) and pa.tree_id == pb.tree_id and (pa.tile_m, pb.tile_m) == (128, 64), (pa.family, pa.tile_m, pb.tile_m)
    rows, x, w = _make(dev, t, M, K, N, seed=K + N + t, keep_w=True)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((0, Ms), (Ms, Ms + 2000), (M - 1000, M), (777, 777 + 333)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        part = dev.mul_mat(Ws, x)
        assert torch.equal(part, full[:, r0:r1]), (t, N, K, r0, r1)
        if r0 == 0:
            _check_fp64(dev, t, rows[r0:r1], x, part, K)
            _check_oracle_sample(t, rows[r0:r1], w[r0:r1], x, part, K, seed=K + N)
        Ws.free()
    W.free()


@pytest.mark.parametrize("t", [Q4_0, 3, 4, Q5_0, 7, Q8_0])
@pytest.mark.parametrize("K", [20512, 28672, 60000 // 32 * 32])
def test_k3p_beyond_one_scale_table_slices_refill_inside_the_K_loop(dev, t, K):
    """K > 20480 (a 70B model's ffn-down at prompt sizes): the eight waves' scale tables no longer fit the 160 KB of LDS whole; the K loop
    goes through them in two to four slices (gemm_qmp.hip SLICED; it was the staged forms' territory up to round 3).  The ragged first
    case is one k-block past the old limit; fp64 evaluation of the same block arithmetic, and row shards are the bitwise slices."""
    M, N = 3000, 300 if t != 3 else 320                    # (Q4_1 runs the form from 257 rows)
    g = torch.Generator(device="cuda")
    g.manual_seed(7 * t + K)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    rows = dev.quantize_rows(t, w)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    _check_fp64(dev, t, rows, x, full, K)
    for (r0, r1) in ((0, 1000), (2100, 2100 + 777)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, K, r0, r1)
        Ws.free()
    W.free()


@pytest.mark.parametrize("t,K,N", [(4, 4096, 9), (4, 4096, 16), (4, 2048, 128), (4, 4096, 100), (Q8_0, 11008, 100), (Q8_0, 11008, 128), (Q5_0, 13824, 96),
                                   (7, 11008, 128), (Q4_0, 11008, 128), (3, 11008, 96)])
def test_batched_decode_forms_beyond_their_round_3_ranges(dev, t, K, N):
    """The stage-free batched-decode forms (gemm_q8s.hip, gemm_qmx.hip K3s) where the end of round 4 put them (plan.cpp k3_stage_free):
    the two-scale type Q4_2 from 9 rows (up to 256 in r4; r5: 128, K3p beyond), every other type up to 128 rows behind K >= 11008 -- three and more column tiles per weight
    tile.  fp64 evaluation of the block arithmetic; a row shard is the bitwise slice (the form is chosen by type, K and N alone)."""
    import ctypes as C
    from ggmlsharp_amd import _lib
    M = 3000
    pl = _lib.ggml_hip_mm_plan_t()
    assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(pl)) == 0 and pl.family in (3, 4), (t, K, N, pl.family)   # 3 / 4 = K3s MX / int8
    g = torch.Generator(device="cuda")
    g.manual_seed(31 * t + K + N)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda") * 2
    rows = dev.quantize_rows(t, w)
    W = dev.Weight.from_device(t, rows, K)
    full = dev.mul_mat(W, x)
    _check_fp64(dev, t, rows, x, full, K)
    for (r0, r1) in ((0, 1000), (2100, 2100 + 777)):
        Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, K, N, r0, r1)
        Ws.free()
    W.free()


@pytest.mark.parametrize("N", [128, 512])
def test_dense_f16_vocabulary_sized_matrix_and_its_shards_share_one_tree(dev, N):
    """F16, up to 512 src1 rows: a 32000-row matrix used to reach the unsplit 256 x 128 form (384 tiles and more) while its 4000-row
    shards ran the K-split forms -- found in round 3, the F16 twin of the Q4_0 case config 5's eight-slot test caught."""
    M, K = 32000, 1024
    g = torch.Generator(device="cuda")
    g.manual_seed(5 + N)
    w = torch.randn((M, K), generator=g, device="cuda").half()
    x = torch.randn((N, K), generator=g, device="cuda")
    rows = w.view(torch.uint8).view(M, -1)
    W = dev.Weight.from_device(1, rows, K)
    full = dev.mul_mat(W, x)
    for (r0, r1) in ((4000, 8000), (31000, 32000)):
        Ws = dev.Weight.from_device(1, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (N, r0, r1)
        Ws.free()
    W.free()


def test_dense_f32_split_form_is_tight_and_shards_are_bitwise_slices(dev):
    """F32 weights above 256 src1 rows: every operand as three bf16 pieces, six bf16 MFMAs per product, a fresh accumulator per k-step
    joined by a rounded add (dense16.hip K10d).  Tighter than the f32 fma chain it replaces (max 1.5e-5 of the rms at K = 4096), and a row
    shard is the bitwise slice of the unsplit product (one tile form, chosen by N alone)."""
    M, K, N = 3000, 4096 + 24, 700
    g = torch.Generator(device="cuda")
    g.manual_seed(11)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda") * 3
    rows = w.view(torch.uint8).view(M, -1)
    W = dev.Weight.from_device(0, rows, K)
    full = dev.mul_mat(W, x)
    ref = x.double() @ w.double().T
    err = (full.double() - ref).abs()
    assert (err.max() / ref.pow(2).mean().sqrt()).item() < 8e-6
    for (r0, r1) in ((0, 1000), (1111, 1300), (2990, 3000)):
        Ws = dev.Weight.from_device(0, rows, K, row_begin=r0, row_end=r1)
        assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1])
        Ws.free()
    assert np.array_equal(W.download(), w.cpu().numpy().view(np.uint8).reshape(-1))      # the row-major copy still round-trips
    W.free()


def test_dense_f32_split_form_keeps_infinities_nans_and_tiny_values(dev):
    """the three-piece split of K10d used to turn an infinite operand into NaN (inf - inf in the remainder pieces) where the
    reference's f32 product gives +-inf.  An infinite weight, an infinite activation, a NaN (payload in the low mantissa bits) and
    operands at the bottom of the normal range, at more than 256 src1 rows (the split form), against torch's f32 product."""
    M, K, N = 256, 512, 300
    g = torch.Generator(device="cuda")
    g.manual_seed(3)
    w = torch.randn((M, K), generator=g, device="cuda")
    x = torch.randn((N, K), generator=g, device="cuda")
    w[3, 7] = float("inf")                                     # column 3 of dst: +-inf by the sign of x[:, 7]
    x[5, 9] = float("-inf")                                    # row 5 of dst: -+inf by the sign of w[:, 9]
    x[11, 0] = torch.tensor([0x7F800001], dtype=torch.int32, device="cuda").view(torch.float32)[0]   # a NaN whose payload is in the low bits
    w[20] = w[20] * 1e-38
    x[21] = x[21] * 1e-30
    W = dev.Weight.from_device(0, w.view(torch.uint8).view(M, -1), K)
    got = dev.mul_mat(W, x)
    W.free()
    ref = x.double() @ w.double().T
    assert torch.isnan(got[11]).all()
    inf_ref = torch.isinf(ref)
    fin = torch.isfinite(ref)
    assert inf_ref[:, 3].sum() > 200 and inf_ref[5].sum() > 200
    ok_inf = inf_ref & torch.isinf(got) & (torch.sign(got.double()) == torch.sign(ref))
    assert torch.equal(ok_inf, inf_ref), "an infinite product did not come out as the same infinity"
    mask = fin.clone()
    mask[11] = False
    # finite outputs: the usual bound; rows / columns scaled down to the denormal border: nothing blows up (flush-to-zero of the pieces is allowed)
    err = (got.double() - ref).abs()[mask]
    rms = ref[mask & (ref.abs() > 1e-20)].pow(2).mean().sqrt()
    assert (err.max() / rms).item() < 1e-5
    assert torch.isfinite(got[21][fin[21]]).all() and torch.isfinite(got[:, 20][fin[:, 20]]).all()


def test_fullsize_byte_roundtrips(dev):
    M, K = 4096, 4096
    for t in (Q4_0, Q5_0, Q8_0):
        rows, _ = _make(dev, t, M, K, 1, seed=t)
        W = dev.Weight.from_device(t, rows, K)
        assert np.array_equal(W.download(), rows.cpu().numpy().reshape(-1))
        W.free()
    rows, _ = _make(dev, Q8_0, 512, K, 1, seed=9)
    y = dev.dequantize_rows(Q8_0, rows, K)
    again = dev.dequantize_rows(Q8_0, dev.quantize_rows(Q8_0, y), K)
    assert torch.allclose(again, y, rtol=0, atol=float(y.abs().max()) * 2 ** -20)


def test_short_wide_shard_runs_the_one_tile_form_with_the_unsplit_bits(dev):
    """A 512-row shard against thousands of src1 rows (the multi-GPU strong-scaling piece) takes 64 x 64 tiles of 1-tile waves
    (two waves per SIMD instead of one); K loop and per-element order are the unsplit matrix's: bitwise its columns."""
    M, K, N = 4096, 512, 3100
    for t in (Q4_0, 3):                                 # Q4_0 (the one-tile form), Q4_1 (stays on the 128 x 64 form)
        rows, x = _make(dev, t, M, K, N, seed=11)
        W = dev.Weight.from_device(t, rows, K)
        full = dev.mul_mat(W, x)
        for (r0, r1) in ((0, 512), (1536, 2048), (3600, 4096)):
            Ws = dev.Weight.from_device(t, rows, K, row_begin=r0, row_end=r1)
            assert torch.equal(dev.mul_mat(Ws, x), full[:, r0:r1]), (t, r0, r1)


@pytest.mark.parametrize("t", [Q4_0, 3, Q5_0, Q8_0])
def test_scratch_contents_never_reach_the_result(dev, t):
    """The work buffer is the caller's scratch: whatever it held before -- here every byte 0xFF, i.e. NaN where a kernel would read a
    float -- must not show in dst.  K that is not a whole number of 4-block stages leaves padded k-blocks in the planes, which a
    kernel either gets zero-filled from INIT or must not read (the int8 image's are not written)."""
    for (M, K, N) in ((130, 2048 + 64, 6), (300, 4096 + 64, 20), (96, 2048 + 32, 64), (200, 2048 + 96, 200), (64, 11008, 33), (128, 96, 12)):
        rows, x = _make(dev, t, M, K, N, seed=3 + t + N)
        W = dev.Weight.from_device(t, rows, K)
        ref = dev.mul_mat(W, x, work=torch.zeros_like(dev.alloc_work(t, K, N)))
        work = dev.alloc_work(t, K, N)
        work.fill_(0xFF)
        got = dev.mul_mat(W, x, work=work)
        assert torch.isfinite(got).all(), (t, M, K, N)
        assert torch.equal(got, ref), (t, M, K, N)
        W.free()
