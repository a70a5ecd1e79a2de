"""The grouped route of expert-routed products (include/ggml_hip_ext.h ggml_hip_mul_mat_id_grouped_*; csrc/moe.cpp, moe.hip's routing
kernels, the grouped K3s wrappers of gemm_q8s.hip / gemm_qmx.hip, plan.cpp plan_mul_mat_id_grouped): the ids are read on the device alone,
the pairs are sorted by expert there into segments padded to 32-row column tiles, and ONE launch runs every tile against its expert.

The checker for BITS is the library's own single-expert entry, code this feature does not touch: the summation tree is fixed by (type, K)
alone -- the tree of ggml_hip_mm_plan(type, M, K, 32) -- so pair p's M outputs == the row that ggml_hip_mul_mat_dev(expert ids[p], a batch
of 32 rows holding p's src1 row at any position, N = 32) returns for it, bit for bit.  One case per kernel family is also held against the
oracle under THE mul_mat tolerance (oracle_lib.assert_mul_mat_close), so a routing error that is consistent on both sides cannot hide.

Shapes: 8 experts, 70 tokens x 2 slots (P = 140; the bound is 140 + 31 * 8 = 388 rows: 12 column tiles), (M, K) = (96, 1024) and
(80, 1120) -- M no multiple of 32, 35 k-blocks over eight waves; the geometry test adds the sizes at which the plan takes two and four
weight tiles per workgroup (more than 256 / 512 tile groups under the bound) and a K whose ranges rotate through the slots."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, F16, Q4_0, Q4_1, Q4_2, Q5_0, Q5_1, Q8_0 = 0, 1, 2, 3, 4, 6, 7, 8
Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_NL, IQ4_XS, BF16 = 110, 111, 112, 113, 114, 120, 123, 130
ALL_TYPES = (Q4_0, Q4_1, Q4_2, Q5_0, Q5_1, Q8_0, F16, F32, BF16, Q5_K, Q4_K, Q6_K, Q3_K, Q2_K, IQ4_NL, IQ4_XS)
SERVED = (Q8_0, Q5_0, IQ4_NL, Q4_0)
K3S_MX, K3S_I8 = 3, 4
NEW_SYMBOLS = ("ggml_hip_mul_mat_id_grouped_serves", "ggml_hip_mul_mat_id_grouped_serves_for", "ggml_hip_mul_mat_id_grouped_work_size",
               "ggml_hip_mul_mat_id_grouped_work_size_for", "ggml_hip_mul_mat_id_grouped_dev")
N_EXPERT, N_TOKENS, N_USED = 8, 70, 2
P = N_TOKENS * N_USED
SHAPES = ((96, 1024), (80, 1120))


# ---------------------------------------------------------------- CPU
def test_the_five_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name


def _plan(t, M, K, N):
    out = _lib.ggml_hip_mm_plan_t()
    rc = _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(out))
    return out if rc == 0 else None


@pytest.mark.parametrize("t", ALL_TYPES)
def test_served_exactly_where_the_type_is_one_of_the_four_and_the_plan_at_32_rows_is_k3s(t):
    L = _lib.lib()
    ones = 0
    for K in (256, 992, 1024, 4096, 32768, 36864):
        for M in (96, 4096):
            pl = _plan(t, M, K, 32)                             # (None: no such product, e.g. a k-quant behind a K that is no multiple of 256)
            want = int(t in SERVED and pl is not None and pl.family in (K3S_I8, K3S_MX))
            assert L.ggml_hip_mul_mat_id_grouped_serves_for(t, M, K) == want, (t, M, K)
            assert (L.ggml_hip_mul_mat_id_grouped_work_size_for(t, M, K, 8, 70, 2) > 0) == bool(want), (t, M, K)
            ones += want
    assert (ones > 0) == (t in SERVED)
    if t in SERVED:                                             # today: K / 32 in 32 .. 1024
        assert [L.ggml_hip_mul_mat_id_grouped_serves_for(t, 96, K) for K in (256, 992, 1024, 4096, 32768, 36864)] == [0, 0, 1, 1, 1, 0]


@pytest.mark.parametrize("t", SERVED)
def test_the_tree_at_32_rows_is_no_function_of_m(t):
    """the structural reason a set of row shards computes a column slice"""
    for K in (1024, 1120, 4096, 32768):
        trees = {_plan(t, M, K, 32).tree_id for M in (16, 96, 4096, 32000)}
        assert len(trees) == 1, (t, K, trees)


def test_the_work_size_covers_its_pieces_and_follows_p_alone():
    L = _lib.lib()
    ws = L.ggml_hip_mul_mat_id_grouped_work_size_for
    for t in SERVED:
        for M, K in SHAPES + ((4096, 4096),):
            for ne in (2, 8, 128, 1024):
                assert ws(t, M, K, ne, 0, 2) == 0
                last = 0
                for p in (1, 2, 31, 32, 33, 140, 1024, 4096):
                    got = ws(t, M, K, ne, p, 1)
                    assert got >= last > -1, (t, M, K, ne, p)                                   # monotone in P
                    assert got >= L.ggml_hip_mul_mat_work_size(t, K, p) + 4 * p * M, (t, M, K, ne, p)     # the image of P rows + the results
                    last = got
                assert ws(t, M, K, ne, 70, 2) == ws(t, M, K, ne, 140, 1) == ws(t, M, K, ne, 35, 4) == ws(t, M, K, ne, 5, 28)
            assert ws(t, M, K, 8, 70, 2) <= ws(t, M, K, 128, 70, 2)                             # (the padding bound grows with n_expert)
    assert ws(Q8_0, 96, 1024, 8, (1 << 20) + 1, 1) == 0 and ws(Q8_0, 96, 1024, 8, 1 << 19, 2) > 0    # P up to 2^20
    assert L.ggml_hip_mul_mat_id_grouped_work_size(None, 70, 2) == 0
    assert L.ggml_hip_mul_mat_id_grouped_serves(None) == _lib.ERR_ARG


def test_the_two_routes_answer_as_before_on_the_served_shapes():
    L = _lib.lib()
    for t in SERVED:
        for M, K in SHAPES + ((4096, 4096),):
            for n_tokens in (1, 4, 5, 70, 512):
                assert L.ggml_hip_mul_mat_id_route_for(t, M, K, 8, n_tokens, 2) in (1, 2), (t, M, K, n_tokens)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


_CACHE = {}


def _rows(dev, t, M, K, seed):
    """M rows of K in type t's format on the device (module-wide cache: computed once, never written)"""
    key = ("w", t, M, K, seed)
    if key not in _CACHE:
        torch = dev.torch
        g = torch.Generator(device="cuda")
        g.manual_seed(1000 * seed + t)
        _CACHE[key] = dev.quantize_rows(t, torch.randn((M, K), generator=g, device="cuda")).contiguous()
    return _CACHE[key]


def _experts(dev, t, M, K, r0=0, r1=None, n_expert=N_EXPERT):
    return [dev.Weight.from_device(t, _rows(dev, t, M, K, e), K, row_begin=r0, row_end=r1) for e in range(n_expert)]


def _x(dev, shape, seed):
    g = dev.torch.Generator(device="cuda")
    g.manual_seed(seed)
    return dev.torch.randn(shape, generator=g, device="cuda")


def _routing():
    """70 tokens x 2 slots over 8 experts, built on purpose: expert 0 no pair, 1 exactly 32, 2 thirty-three, 3 one, 4..7 the other 74 at random"""
    rng = np.random.default_rng(17)
    flat = np.concatenate([np.full(32, 1), np.full(33, 2), np.full(1, 3), rng.integers(4, 8, P - 66)]).astype(np.int32)
    rng.shuffle(flat)
    counts = np.bincount(flat, minlength=N_EXPERT)
    assert counts[0] == 0 and counts[1] == 32 and counts[2] == 33 and counts[3] == 1 and counts[4:].min() > 0
    return flat.reshape(N_TOKENS, N_USED)


IDS_A = _routing()
IDS_B = ((IDS_A + 3) % N_EXPERT).astype(np.int32)                # another routing: the empty expert is 3, the one-pair expert 6


def _same_bits(dev, a, b):
    return a.shape == b.shape and dev.torch.equal(a.contiguous().view(dev.torch.int32), b.contiguous().view(dev.torch.int32))


def _want(dev, ws, ids, rows, reverse=()):
    """[P, M]: every expert's pairs (ascending p) cut into batches of 32, the last padded with zero rows, one N = 32 ggml_hip_mul_mat_dev call
    per batch; the experts in `reverse` with the rows of each batch in reverse order.  A pair whose id is outside the set: +0.0f."""
    torch = dev.torch
    flat = np.asarray(ids).reshape(-1)
    out = torch.zeros((len(flat), ws[0].M), device="cuda")
    for e in range(len(ws)):
        pairs = np.nonzero(flat == e)[0]
        for b0 in range(0, len(pairs), 32):
            chunk = pairs[b0:b0 + 32]
            slot = np.arange(len(chunk))[::-1] + (32 - len(chunk)) if e in reverse else np.arange(len(chunk))
            batch = torch.zeros((32, rows.shape[1]), device="cuda")
            batch[torch.from_numpy(slot.copy()).cuda()] = rows[torch.from_numpy(chunk).cuda()]
            res = dev.mul_mat(ws[e], batch)
            out[torch.from_numpy(chunk).cuda()] = res[torch.from_numpy(slot.copy()).cuda()]
    return out


def _pair_rows(x, n_used):
    """[P, K]: the src1 row of every pair (x: [n_tokens, K] one row per token, or [n_tokens, n_used, K])"""
    return x.repeat_interleave(n_used, dim=0) if x.dim() == 2 else x.reshape(-1, x.shape[-1])


def _case(dev, t, M, K):
    """the experts, the set, the src1 rows and the reference of the clean routing IDS_A: built once per (type, shape), never written"""
    key = ("case", t, M, K)
    if key not in _CACHE:
        ws = _experts(dev, t, M, K)
        x = _x(dev, (N_TOKENS, K), 100 + M)
        _CACHE[key] = (ws, dev.ExpertSet(ws), x, _want(dev, ws, IDS_A, _pair_rows(x, N_USED)))
    return _CACHE[key]


@pytest.mark.gpu
@pytest.mark.parametrize("M,K", SHAPES)
@pytest.mark.parametrize("t", SERVED)
def test_every_pair_is_bitwise_its_experts_own_call_at_32_rows(dev, t, M, K):
    torch = dev.torch
    L = _lib.lib()
    ws, es, x, want = _case(dev, t, M, K)
    assert es.grouped_serves() == 1 == L.ggml_hip_mul_mat_id_grouped_serves_for(t, M, K)
    assert es.grouped_work_size(N_TOKENS, N_USED) == L.ggml_hip_mul_mat_id_grouped_work_size_for(t, M, K, N_EXPERT, N_TOKENS, N_USED) > 0
    assert es.route(N_TOKENS, N_USED) == 2                        # (the two routes answer as before)
    got = dev.mul_mat_id_grouped(es, torch.from_numpy(IDS_A).cuda(), x)
    torch.cuda.synchronize()
    assert _same_bits(dev, got.reshape(P, M), want), (t, M, K)
    # the position inside the batch takes no part: the 33-pair expert's batches in reverse order
    assert _same_bits(dev, _want(dev, ws, IDS_A, _pair_rows(x, N_USED), reverse=(2,)), want), (t, M, K)
    # one row per slot (the down projection)
    xs = _x(dev, (N_TOKENS, N_USED, K), 200 + M)
    got = dev.mul_mat_id_grouped(es, torch.from_numpy(IDS_A).cuda(), xs)
    torch.cuda.synchronize()
    assert _same_bits(dev, got.reshape(P, M), _want(dev, ws, IDS_A, _pair_rows(xs, N_USED))), (t, M, K)


@pytest.mark.gpu
@pytest.mark.parametrize("t,M,K", ((Q8_0, 704, 1024), (Q5_0, 704, 1024), (Q4_0, 704, 1024), (Q8_0, 1400, 1024), (Q5_0, 1400, 1024), (Q4_0, 1400, 1024),
                                   (Q8_0, 96, 8192), (Q4_0, 96, 8192), (Q8_0, 704, 8192), (Q4_0, 704, 8192)))
def test_the_other_geometries_compute_the_same_bits(dev, t, M, K):
    """12 column tiles under the bound: 704 rows are 264 tile groups (two weight tiles per workgroup), 1400 rows 528 (four); K = 8192 is 32
    k-blocks per wave, which rotate through the slots"""
    torch = dev.torch
    ws = _experts(dev, t, M, K)
    es = dev.ExpertSet(ws)
    x = _x(dev, (N_TOKENS, K), 300 + M)
    got = dev.mul_mat_id_grouped(es, torch.from_numpy(IDS_A).cuda(), x)
    torch.cuda.synchronize()
    assert _same_bits(dev, got.reshape(P, M), _want(dev, ws, IDS_A, _pair_rows(x, N_USED))), (t, M, K)
    es.free()


@pytest.mark.gpu
@pytest.mark.parametrize("t", (Q8_0, Q4_0))
def test_one_case_per_kernel_family_against_the_oracle_under_the_library_tolerance(dev, t):
    torch = dev.torch
    M, K = SHAPES[0]
    ws, es, x, _ = _case(dev, t, M, K)
    got = dev.mul_mat_id_grouped(es, torch.from_numpy(IDS_A).cuda(), x).cpu().numpy().reshape(P, M)
    xh, flat = x.cpu().numpy(), IDS_A.reshape(-1)
    ref = np.zeros_like(got)
    for e in range(N_EXPERT):
        pairs = np.nonzero(flat == e)[0]
        if len(pairs):
            wq = _rows(dev, t, M, K, e).cpu().numpy()
            ref[pairs] = O.mul_mat(t, wq, xh[pairs // N_USED], M, K, len(pairs), nth=2)[0, 0]
    O.assert_mul_mat_close(got, ref, K, f"mul_mat_id grouped type {t}")      # THE mul_mat tolerance (tests/oracle_lib.py)


def _call(dev, es, ids_d, n_tokens, n_used, x_ptr, ld1_token, ld1_slot, out_ptr, ldd, work_ptr, work_bytes):
    return _lib.lib().ggml_hip_mul_mat_id_grouped_dev(es.handle, C.c_void_p(ids_d.data_ptr()) if ids_d is not None else None, n_tokens, n_used,
                                                      C.c_void_p(x_ptr), ld1_token, ld1_slot, C.c_void_p(out_ptr), ldd, C.c_void_p(work_ptr) if work_ptr else None,
                                                      work_bytes, C.c_void_p(dev.torch.cuda.current_stream().cuda_stream))


GUARD = 256      # floats


def _is_nan_bits(dev, a):
    return bool((a.view(dev.torch.int32) == 0x7FC00000).all())


@pytest.mark.gpu
@pytest.mark.parametrize("t", (Q8_0, Q4_0))
def test_ids_outside_the_set_give_zero_rows_and_touch_nothing_else(dev, t):
    torch = dev.torch
    M, K = SHAPES[1]
    ws, es, x, want = _case(dev, t, M, K)
    bad = IDS_A.copy().reshape(-1)
    where = (5, 64, 139)
    bad[list(where)] = (-1, N_EXPERT, 2 ** 30)
    nbytes = es.grouped_work_size(N_TOKENS, N_USED)
    assert nbytes % 4 == 0
    nan = torch.tensor(0x7FC00000, dtype=torch.int32, device="cuda").view(torch.float32)
    dst = nan.repeat(GUARD + P * M + GUARD)
    work = nan.repeat(nbytes // 4 + GUARD)
    rc = _call(dev, es, torch.from_numpy(bad).cuda(), N_TOKENS, N_USED, x.data_ptr(), x.stride(0), 0, dst.data_ptr() + 4 * GUARD, M, work.data_ptr(), nbytes)
    torch.cuda.synchronize()
    assert rc == 0
    got = dst[GUARD:GUARD + P * M].reshape(P, M)
    off = torch.zeros(P, dtype=torch.bool, device="cuda")
    off[list(where)] = True
    assert (got[off].view(torch.int32) == 0).all()                 # +0.0f: the bits, not the value
    assert _same_bits(dev, got[~off], want[~off])                  # every other row as in the clean run
    assert _is_nan_bits(dev, dst[:GUARD]) and _is_nan_bits(dev, dst[GUARD + P * M:]) and _is_nan_bits(dev, work[nbytes // 4:])


@pytest.mark.gpu
def test_strides_a_row_per_slot_and_padded_dst_rows(dev):
    torch = dev.torch
    t = Q8_0
    M, K = SHAPES[0]
    ws, es, _, _ = _case(dev, t, M, K)
    ld1_token, ldd = N_USED * K + 4, M + 4
    xbuf = _x(dev, (N_TOKENS, ld1_token), 41)
    rows = xbuf[:, :N_USED * K].reshape(P, K)
    nan = torch.tensor(0x7FC00000, dtype=torch.int32, device="cuda").view(torch.float32)
    dst = nan.repeat(P * ldd).reshape(P, ldd)
    work = torch.empty(es.grouped_work_size(N_TOKENS, N_USED), dtype=torch.uint8, device="cuda")
    rc = _call(dev, es, torch.from_numpy(IDS_A).cuda(), N_TOKENS, N_USED, xbuf.data_ptr(), ld1_token, K, dst.data_ptr(), ldd, work.data_ptr(), work.numel())
    torch.cuda.synchronize()
    assert rc == 0
    assert _same_bits(dev, dst[:, :M], _want(dev, ws, IDS_A, rows.contiguous()))
    assert _is_nan_bits(dev, dst[:, M:])                            # the padding columns of dst are untouched


@pytest.mark.gpu
@pytest.mark.parametrize("t", (Q8_0, Q4_0))
def test_a_set_of_row_shards_is_the_bitwise_column_slice(dev, t):
    torch = dev.torch
    M, K = SHAPES[0]
    _, es, x, _ = _case(dev, t, M, K)
    shard = dev.ExpertSet(_experts(dev, t, M, K, 32, 80))
    assert shard.M == 48 and shard.grouped_serves() == 1
    ids_d = torch.from_numpy(IDS_A).cuda()
    a, b = dev.mul_mat_id_grouped(es, ids_d, x), dev.mul_mat_id_grouped(shard, ids_d, x)
    torch.cuda.synchronize()
    assert _same_bits(dev, a[..., 32:80], b), t
    shard.free()


@pytest.mark.gpu
@pytest.mark.parametrize("t", (Q8_0, Q4_0))
def test_a_captured_call_follows_the_ids_of_each_replay(dev, t):
    torch = dev.torch
    M, K = SHAPES[0]
    ws, es, x, want_a = _case(dev, t, M, K)
    ids_d = torch.from_numpy(IDS_A).cuda()
    out = torch.zeros((N_TOKENS, N_USED, M), device="cuda")
    work = torch.empty(es.grouped_work_size(N_TOKENS, N_USED), dtype=torch.uint8, device="cuda")
    eager_b = dev.mul_mat_id_grouped(es, torch.from_numpy(IDS_B).cuda(), x).reshape(P, M).clone()
    torch.cuda.synchronize()
    assert _same_bits(dev, eager_b, _want(dev, ws, IDS_B, _pair_rows(x, N_USED))) and not _same_bits(dev, eager_b, want_a)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                   # (a first call outside the capture: the kernels' attributes are set)
        dev.mul_mat_id_grouped(es, ids_d, x, out=out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # captures on a side stream: one chain of launches
        rc = _call(dev, es, ids_d, N_TOKENS, N_USED, x.data_ptr(), x.stride(0), 0, out.data_ptr(), M, work.data_ptr(), work.numel())
    assert rc == 0                                                  # (and the capture ended valid: the graph replays below)
    for ids, want in ((IDS_A, want_a), (IDS_B, eager_b), (IDS_A, want_a)):
        ids_d.copy_(torch.from_numpy(ids).cuda())
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(dev, out.reshape(P, M), want), t
    del graph


@pytest.mark.gpu
def test_refusals_return_their_code_and_launch_nothing(dev):
    torch = dev.torch
    M, K = SHAPES[0]
    ids_d = torch.from_numpy(IDS_A).cuda()
    _, es, x, want = _case(dev, Q8_0, M, K)
    out = torch.full((N_TOKENS, N_USED, M), 7.0, device="cuda")
    work = torch.full((es.grouped_work_size(N_TOKENS, N_USED),), 9, dtype=torch.uint8, device="cuda")
    args = (N_TOKENS, N_USED, x.data_ptr(), x.stride(0), 0, out.data_ptr(), M)
    q51 = dev.ExpertSet(_experts(dev, Q5_1, M, K, n_expert=2))
    assert q51.grouped_serves() == 0 and q51.grouped_work_size(N_TOKENS, N_USED) == 0
    assert _call(dev, q51, ids_d, *args, work.data_ptr(), work.numel()) == _lib.ERR_TYPE
    short = dev.ExpertSet(_experts(dev, Q8_0, M, 512, n_expert=2))
    x512 = _x(dev, (N_TOKENS, 512), 61)
    assert short.grouped_serves() == 0 and short.grouped_work_size(N_TOKENS, N_USED) == 0
    assert _call(dev, short, ids_d, N_TOKENS, N_USED, x512.data_ptr(), 512, 0, out.data_ptr(), M, work.data_ptr(), work.numel()) == _lib.ERR_SHAPE
    assert _call(dev, es, ids_d, *args, work.data_ptr(), work.numel() - 1) == _lib.ERR_ARG          # a short work buffer
    assert _call(dev, es, ids_d, *args, None, 0) == _lib.ERR_ARG
    assert _call(dev, es, None, *args, work.data_ptr(), work.numel()) == _lib.ERR_ARG               # the ids are read on the device
    assert _call(dev, es, ids_d, N_TOKENS, 0, *args[2:], work.data_ptr(), work.numel()) == _lib.ERR_ARG
    assert _call(dev, es, ids_d, 1 << 20, 2, *args[2:], work.data_ptr(), work.numel()) == _lib.ERR_SHAPE     # more than 2^20 pairs
    assert _call(dev, es, ids_d, N_TOKENS, N_USED, x.data_ptr() + 4, x.stride(0), 0, out.data_ptr(), M, work.data_ptr(), work.numel()) == _lib.ERR_SHAPE
    assert _call(dev, es, ids_d, N_TOKENS, N_USED, x.data_ptr(), x.stride(0), 0, out.data_ptr(), M - 1, work.data_ptr(), work.numel()) == _lib.ERR_SHAPE
    assert _call(dev, es, ids_d, 0, N_USED, *args[2:], work.data_ptr(), work.numel()) == 0          # no tokens: nothing to do, nothing written
    torch.cuda.synchronize()
    assert (out == 7.0).all() and (work == 9).all()                 # nothing was launched
    assert _call(dev, es, ids_d, *args, work.data_ptr(), work.numel()) == 0                         # (the same arguments in order do run)
    torch.cuda.synchronize()
    assert _same_bits(dev, out.reshape(P, M), want)
    q51.free()
    short.free()
