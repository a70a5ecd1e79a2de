"""Expert-routed products (include/ggml_hip_ext.h ggml_hip_expert_set_* / ggml_hip_mul_mat_id_*; csrc/moe.cpp, moe.hip, gemv.hip's by-id
kernel): upstream's ggml_mul_mat_id for a mixture-of-experts layer.

The checker for BITS is the library's own single-expert entry, ggml_hip_mul_mat_dev -- code this feature does not touch:
  route 1 (the by-id mat-vec): pair p's M outputs == ggml_hip_mul_mat_dev(expert ids[p], the row of p, N = 1), bit for bit;
  route 2 (the batch route):   pair p's outputs == its row of ggml_hip_mul_mat_dev(expert e, e's gathered batch in ascending p, N = count_e).
One case per route is also held against the oracle under THE mul_mat tolerance (oracle_lib.assert_mul_mat_close), so a routing error that
is consistent on both sides cannot hide.

CPU tests: the symbols, and the route / work size answered without a device through the twins ggml_hip_mul_mat_id_route_for /
_work_size_for (type, M, K, n_expert, n_tokens, n_used) -- the set's own entries are the same function of the set's type, M and K and are
held against the twins in the GPU tests.  The rule: route 1 exactly where ggml_hip_mm_plan(type, M, K, N = 1) is the fused mat-vec and
n_tokens <= 4; never a function of n_expert or n_used."""
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
SUPER = (Q2_K, Q3_K, Q4_K, Q5_K, Q6_K, IQ4_XS)           # super-blocks of 256
GEMV_FUSED = 1
NEW_SYMBOLS = ("ggml_hip_expert_set_create", "ggml_hip_expert_set_free", "ggml_hip_mul_mat_id_route", "ggml_hip_mul_mat_id_work_size",
               "ggml_hip_mul_mat_id_route_for", "ggml_hip_mul_mat_id_work_size_for", "ggml_hip_mul_mat_id_dev")


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    assert "typedef struct ggml_hip_expert_set ggml_hip_expert_set;" in hdr
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name


def _plan_family(t, M, K, N):
    out = _lib.ggml_hip_mm_plan_t()
    assert _lib.lib().ggml_hip_mm_plan(t, M, K, N, C.byref(out)) == 0, (t, M, K, N)
    return out.family


@pytest.mark.parametrize("t", ALL_TYPES)
def test_route_1_exactly_where_the_plan_at_one_row_is_the_fused_mat_vec_and_at_most_four_tokens(t):
    L = _lib.lib()
    ones = 0
    for K in (256, 2048, 4096, 4128, 32768, 36864):
        if t in SUPER and K % 256:
            assert L.ggml_hip_mul_mat_id_route_for(t, 96, K, 8, 1, 2) == _lib.ERR_SHAPE
            continue
        for M in (96, 4096):
            fused = _plan_family(t, M, K, 1) == GEMV_FUSED
            for n_tokens in range(1, 7):
                want = 1 if fused and n_tokens <= 4 else 2
                got = {L.ggml_hip_mul_mat_id_route_for(t, M, K, ne, n_tokens, nu) for ne in (2, 8, 128, 1024) for nu in (1, 2, 8, 64)}
                assert got == {want}, (t, M, K, n_tokens, got, want)      # never a function of n_expert or n_used
                ones += want == 1
                ws = {L.ggml_hip_mul_mat_id_work_size_for(t, M, K, ne, n_tokens, 2) for ne in (2, 1024)}
                assert len(ws) == 1 and (ws == {0}) == (want == 1), (t, M, K, n_tokens, ws)
    # the types the by-id mat-vec serves, and those it never does
    by_id = t in (Q4_0, Q4_1, Q4_2, Q5_0, Q5_1, Q8_0, IQ4_NL, Q5_K, Q4_K, Q6_K, Q3_K, IQ4_XS)
    assert (ones > 0) == by_id, (t, ones)
    if t in (Q5_K, Q4_K, Q6_K, Q3_K, IQ4_XS):
        assert L.ggml_hip_mul_mat_id_route_for(t, 96, 32768, 8, 4, 2) == 1 and L.ggml_hip_mul_mat_id_route_for(t, 96, 36864, 8, 4, 2) == 2


def test_the_batch_routes_work_size_covers_its_pieces_and_bad_arguments_are_refused():
    L = _lib.lib()
    for t in (Q4_0, Q2_K, F16, F32):
        M, K, n_tokens, n_used = 96, 2048, 70, 2
        P = n_tokens * n_used
        need = 4 * P * K + 4 * P * M + L.ggml_hip_mul_mat_work_size(t, K, P)    # gathered rows, sorted results, one expert taking every pair
        ws = L.ggml_hip_mul_mat_id_work_size_for(t, M, K, 8, n_tokens, n_used)
        assert need <= ws <= need + 4096, (t, ws, need)
        assert L.ggml_hip_mul_mat_id_work_size_for(t, M, K, 8, 0, n_used) == 0
    assert L.ggml_hip_mul_mat_id_route_for(Q4_0, 96, 2048, 8, -1, 2) == _lib.ERR_ARG
    assert L.ggml_hip_mul_mat_id_route_for(Q4_0, 96, 2048, 8, 4, 0) == _lib.ERR_ARG
    assert L.ggml_hip_mul_mat_id_route_for(Q4_0, 96, 2040, 8, 4, 2) == _lib.ERR_SHAPE
    assert L.ggml_hip_mul_mat_id_route_for(9, 96, 2048, 8, 4, 2) == _lib.ERR_TYPE          # Q8_1: no weight type
    assert L.ggml_hip_mul_mat_id_route(None, 4, 2) == _lib.ERR_ARG and L.ggml_hip_mul_mat_id_work_size(None, 4, 2) == 0


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


_WEIGHTS = {}


def _rows(dev, t, M, K, seed):
    """M rows of K in type t's format on the device, and the same bytes on the host (module-wide cache: computed once, never written)"""
    key = (t, M, K, seed)
    if key not in _WEIGHTS:
        torch = dev.torch
        g = torch.Generator(device="cuda")
        g.manual_seed(1000 * seed + t)
        w = torch.randn((M, K), generator=g, device="cuda")
        rows = w if t == F32 else w.half() if t == F16 else dev.quantize_rows(t, w)
        _WEIGHTS[key] = rows.contiguous()
    return _WEIGHTS[key]


def _experts(dev, t, n_expert, M, K, r0=0, r1=None):
    return [dev.Weight.from_device(t, _rows(dev, t, M, K, e), K, row_begin=r0, row_end=r1) for e in range(n_expert)]


def _x(dev, shape, seed):
    g = dev.torch.Generator(device="cuda")
    g.manual_seed(seed)
    return dev.torch.randn(shape, generator=g, device="cuda")


def _singles(dev, ws, ids, x):
    """[n_tokens, n_used, M] from one N = 1 ggml_hip_mul_mat_dev call per pair (x: [n_tokens, K] or [n_tokens, n_used, K])"""
    torch = dev.torch
    n_tokens, n_used = ids.shape
    out = torch.empty((n_tokens, n_used, ws[0].M), device="cuda")
    for t in range(n_tokens):
        for s in range(n_used):
            row = x[t] if x.dim() == 2 else x[t, s]
            out[t, s] = dev.mul_mat(ws[int(ids[t, s])], row.reshape(1, -1))[0]
    return out


def _batches(dev, ws, ids, x):
    """[n_tokens, n_used, M] from one ggml_hip_mul_mat_dev call per non-empty expert on its pairs' rows, ascending p"""
    torch = dev.torch
    n_tokens, n_used = ids.shape
    flat = ids.reshape(-1)
    out = torch.full((n_tokens * n_used, ws[0].M), float("nan"), device="cuda")
    for e in range(len(ws)):
        pairs = np.nonzero(flat == e)[0]
        if not len(pairs):
            continue
        rows = [x[p // n_used] if x.dim() == 2 else x[p // n_used, p % n_used] for p in pairs]
        out[torch.from_numpy(pairs).cuda()] = dev.mul_mat(ws[e], torch.stack(rows).contiguous())
    return out.reshape(n_tokens, n_used, -1)


def _same_bits(dev, a, b):
    return dev.torch.equal(a.view(dev.torch.int32), b.view(dev.torch.int32))


IDS_R1 = np.array([[1, 1, 4], [0, 4, 2], [3, 1, 1], [2, 0, 3]], np.int32)       # an expert twice in a token and again across tokens
IDS_R1_WIDE = np.array([[1, 1], [0, 4], [4, 2], [3, 1]], np.int32)


@pytest.mark.gpu
@pytest.mark.parametrize("t", (Q4_0, Q4_1, Q5_0, Q5_1, Q4_2, Q8_0, IQ4_NL, Q5_K, Q4_K, Q6_K, Q3_K, IQ4_XS))
def test_route_1_is_bitwise_the_single_calls(dev, t):
    """(M, K): 40 x 256 a ragged last row tile and a partial chunk, 64 x 4096 the single-chunk look-ahead form, 48 x 4128 / 4352 a second
    chunk, 528 x 1024 with 8 pairs 264 row tiles in a grid capped at 256 workgroups: workgroups walk several tiles of their pair"""
    torch = dev.torch
    shapes = ((40, 256), (64, 4096), (48, 4352)) if t in SUPER else ((40, 256), (64, 4096), (48, 4128), (528, 1024))
    for M, K in shapes:
        ws = _experts(dev, t, 5, M, K)
        es = dev.ExpertSet(ws)
        cases = [(IDS_R1_WIDE, 4)] if M == 528 else [(IDS_R1[:1], 1), (IDS_R1, 4)]
        for ids, n_tokens in cases:
            n_used = ids.shape[1]
            assert es.route(n_tokens, n_used) == 1 == _lib.lib().ggml_hip_mul_mat_id_route_for(t, M, K, 5, n_tokens, n_used)
            assert es.work_size(n_tokens, n_used) == 0
            ids_d = torch.from_numpy(ids).cuda()
            for per_slot in (False, True):
                x = _x(dev, (n_tokens, n_used, K) if per_slot else (n_tokens, K), 7 + M)
                got = dev.mul_mat_id(es, ids_d, x)
                torch.cuda.synchronize()
                assert _same_bits(dev, got, _singles(dev, ws, ids, x)), (t, M, K, n_tokens, per_slot)
        es.free()


@pytest.mark.gpu
def test_route_1_reads_the_ids_on_the_device_a_captured_call_follows_them(dev):
    torch = dev.torch
    t, M, K = Q4_0, 64, 4096
    ws = _experts(dev, t, 5, M, K)
    es = dev.ExpertSet(ws)
    ids_a, ids_b = IDS_R1, np.ascontiguousarray(IDS_R1[::-1, ::-1])
    ids_d = torch.from_numpy(ids_a).cuda()
    x = _x(dev, (4, K), 11)
    out = torch.zeros((4, 3, M), device="cuda")
    work = torch.empty(16, dtype=torch.uint8, device="cuda")
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        dev.mul_mat_id(es, ids_d, x, out=out, work=work)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        dev.mul_mat_id(es, ids_d, x, out=out, work=work)
    want_a, want_b = _singles(dev, ws, ids_a, x), _singles(dev, ws, ids_b, x)
    assert not _same_bits(dev, want_a, want_b)
    for ids, want in ((ids_a, want_a), (ids_b, want_b), (ids_a, want_a)):
        ids_d.copy_(torch.from_numpy(ids).cuda())
        out.zero_()
        graph.replay()
        torch.cuda.synchronize()
        assert _same_bits(dev, out, want)
    del graph
    es.free()


def _routing_r2():
    """70 tokens x 2 slots over 8 experts: expert 0 no pair, 1 one, 2 four, 3 twenty (5..32), 4 seventy (> 64), 5..7 fifteen each"""
    counts = (0, 1, 4, 20, 70, 15, 15, 15)
    flat = np.concatenate([np.full(c, e, np.int32) for e, c in enumerate(counts)])
    np.random.default_rng(5).shuffle(flat)
    return flat.reshape(70, 2), counts


@pytest.mark.gpu
@pytest.mark.parametrize("t", (Q4_0, Q8_0, Q5_1, Q6_K, Q2_K, F16, BF16, F32))
def test_route_2_is_bitwise_the_gathered_single_expert_calls(dev, t):
    torch = dev.torch
    M, K = 96, 2048
    ws = _experts(dev, t, 8, M, K)
    es = dev.ExpertSet(ws)
    ids, counts = _routing_r2()
    assert tuple(np.bincount(ids.reshape(-1), minlength=8)) == counts
    assert es.route(70, 2) == 2 == _lib.lib().ggml_hip_mul_mat_id_route_for(t, M, K, 8, 70, 2)
    assert es.work_size(70, 2) == _lib.lib().ggml_hip_mul_mat_id_work_size_for(t, M, K, 8, 70, 2) > 0
    ids_d = torch.from_numpy(ids).cuda()
    x = _x(dev, (70, K), 21)
    want = _batches(dev, ws, ids, x)
    for h_ids in (ids, None):
        got = dev.mul_mat_id(es, ids_d, x, h_ids=h_ids)
        torch.cuda.synchronize()
        assert _same_bits(dev, got, want), (t, h_ids is None)
    xs = _x(dev, (70, 2, K), 22)                                 # the down projection: a row per slot
    got = dev.mul_mat_id(es, ids_d, xs, h_ids=ids)
    torch.cuda.synchronize()
    assert _same_bits(dev, got, _batches(dev, ws, ids, xs)), t
    if t in (Q2_K, F16):                                          # types that never take route 1: a decode-sized call is the batch route too
        ids3 = np.array([[4, 4], [1, 7], [4, 3]], np.int32)
        assert es.route(3, 2) == 2
        x3 = _x(dev, (3, K), 23)
        for h_ids in (ids3, None):
            got = dev.mul_mat_id(es, torch.from_numpy(ids3).cuda(), x3, h_ids=h_ids)
            torch.cuda.synchronize()
            assert _same_bits(dev, got, _batches(dev, ws, ids3, x3)), (t, h_ids is None)
    es.free()


@pytest.mark.gpu
def test_one_case_per_route_against_the_oracle_under_the_library_tolerance(dev):
    torch = dev.torch
    for t, M, K, ids, n_expert in ((Q4_0, 64, 4096, IDS_R1, 5), (Q8_0, 96, 2048, _routing_r2()[0], 8)):
        n_tokens, n_used = ids.shape
        ws = _experts(dev, t, n_expert, M, K)
        es = dev.ExpertSet(ws)
        assert es.route(n_tokens, n_used) == (1 if n_tokens == 4 else 2)
        x = _x(dev, (n_tokens, K), 31)
        got = dev.mul_mat_id(es, torch.from_numpy(ids).cuda(), x, h_ids=ids).cpu().numpy().reshape(-1, M)
        xh, flat = x.cpu().numpy(), ids.reshape(-1)
        ref = np.zeros_like(got)
        for e in range(n_expert):
            pairs = np.nonzero(flat == e)[0]
            if len(pairs):
                wq = _rows(dev, t, M, K, e).cpu().numpy()
                ref[pairs] = O.mul_mat(t, wq, xh[pairs // n_used], M, K, len(pairs), nth=2)[0, 0]
        O.assert_mul_mat_close(got, ref, K, f"mul_mat_id type {t} route {es.route(n_tokens, n_used)}")   # THE mul_mat tolerance (tests/oracle_lib.py)
        es.free()


@pytest.mark.gpu
@pytest.mark.parametrize("t", (Q4_0, Q6_K))
def test_a_set_of_row_shards_is_the_bitwise_column_slice_on_both_routes(dev, t):
    torch = dev.torch
    M, K = 96, 2048
    whole, shard = dev.ExpertSet(_experts(dev, t, 8, M, K)), dev.ExpertSet(_experts(dev, t, 8, M, K, 16, 80))
    assert shard.M == 64
    for ids in (np.array([[1, 1, 4], [0, 4, 2], [7, 1, 1], [2, 0, 3]], np.int32), _routing_r2()[0]):
        n_tokens, n_used = ids.shape
        assert whole.route(n_tokens, n_used) == shard.route(n_tokens, n_used) == (1 if n_tokens == 4 else 2)
        x = _x(dev, (n_tokens, K), 41)
        ids_d = torch.from_numpy(ids).cuda()
        a, b = dev.mul_mat_id(whole, ids_d, x, h_ids=ids), dev.mul_mat_id(shard, ids_d, x, h_ids=ids)
        torch.cuda.synchronize()
        assert _same_bits(dev, a[..., 16:80].contiguous(), b), (t, n_tokens)
    whole.free()
    shard.free()


def _call(dev, es, d_ids, h_ids, n_tokens, n_used, x, out, work, work_bytes=None):
    vp = lambda a: C.c_void_p(a.data_ptr()) if a is not None else None
    hp = h_ids.ctypes.data_as(C.c_void_p) if h_ids is not None else None
    return _lib.lib().ggml_hip_mul_mat_id_dev(es.handle, vp(d_ids), hp, n_tokens, n_used, vp(x), x.stride(0), 0, vp(out), out.stride(1), vp(work),
                                              work.numel() if work_bytes is None else work_bytes, C.c_void_p(dev.torch.cuda.current_stream().cuda_stream))


@pytest.mark.gpu
def test_ids_outside_the_set_are_not_a_fault(dev):
    torch = dev.torch
    t, M, K = Q4_0, 96, 2048
    ws = _experts(dev, t, 5, M, K)
    es = dev.ExpertSet(ws)
    # route 1: the ids are only known on the device -- those pairs are +0.0f, the others unchanged bit for bit
    good = IDS_R1.copy()
    bad = good.copy()
    bad[0, 1], bad[2, 0], bad[3, 2] = -1, 5, 2 ** 31 - 1
    x = _x(dev, (4, K), 51)
    want = _singles(dev, ws, good, x)
    out = torch.full((4, 3, M), float("nan"), device="cuda")
    dev.mul_mat_id(es, torch.from_numpy(bad).cuda(), x, out=out)
    torch.cuda.synchronize()
    off = torch.from_numpy((bad < 0) | (bad >= 5)).cuda()
    assert (out[off].view(torch.int32) == 0).all() and int(off.sum()) == 3
    assert _same_bits(dev, out[~off], want[~off])
    # route 2 with the ids on the host: refused before anything is launched, dst untouched
    ids = np.tile(np.array([[0, 1]], np.int32), (6, 1))
    ids[4, 1] = 5
    x6 = _x(dev, (6, K), 52)
    out = torch.full((6, 2, M), 7.0, device="cuda")
    work = torch.empty(es.work_size(6, 2), dtype=torch.uint8, device="cuda")
    assert es.route(6, 2) == 2
    assert _call(dev, es, torch.from_numpy(ids).cuda(), ids, 6, 2, x6, out, work) == _lib.ERR_ARG
    assert b"ids[9]" in _lib.lib().ggml_hip_last_error()
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    # ... and with the ids on the device alone: that pair is +0.0f, the others are the batch route's bits
    got = dev.mul_mat_id(es, torch.from_numpy(ids).cuda(), x6, out=out, work=work)
    torch.cuda.synchronize()
    ok = ids.copy()
    ok[4, 1] = 1
    want = _batches(dev, ws, np.delete(ok.reshape(-1), 9).reshape(1, -1).T.reshape(-1, 1),
                    torch.stack([x6[p // 2] for p in range(12) if p != 9]))
    assert (got[4, 1].view(torch.int32) == 0).all()
    keep = torch.tensor([p for p in range(12) if p != 9], device="cuda")
    assert _same_bits(dev, got.reshape(12, M)[keep], want.reshape(11, M))
    es.free()


@pytest.mark.gpu
def test_refusals(dev):
    torch = dev.torch
    L = _lib.lib()
    M, K = 96, 2048
    q4, q8, tall = _experts(dev, Q4_0, 2, M, K), _experts(dev, Q8_0, 2, M, K), _experts(dev, Q4_0, 1, 128, K)

    def create(ws, n=None):
        hw = (C.c_void_p * len(ws))(*[w.handle for w in ws])
        h = C.c_void_p(1)
        rc = L.ggml_hip_expert_set_create(hw, len(ws) if n is None else n, None, C.byref(h))
        assert rc == 0 or not h.value
        if rc == 0:
            L.ggml_hip_expert_set_free(h)
        return rc

    assert create(q4) == 0
    assert create([q4[0], q8[0]]) == _lib.ERR_ARG                   # mixed types
    assert create([q4[0], tall[0]]) == _lib.ERR_SHAPE               # mixed M
    assert create(q4, 1) == _lib.ERR_ARG                            # n_expert = 1
    assert create(q4 * 600) == _lib.ERR_ARG                         # n_expert = 1200
    assert L.ggml_hip_expert_set_create(None, 2, None, C.byref(C.c_void_p())) == _lib.ERR_ARG
    es = dev.ExpertSet(q4)
    ids = np.array([[0, 1]] * 6, np.int32)
    ids_d = torch.from_numpy(ids).cuda()
    x = _x(dev, (6, K), 61)
    out = torch.full((6, 2, M), 7.0, device="cuda")
    work = torch.empty(es.work_size(6, 2), dtype=torch.uint8, device="cuda")
    assert _call(dev, es, None, None, 6, 2, x, out, work) == _lib.ERR_ARG                  # null ids (batch route)
    assert _call(dev, es, None, None, 4, 2, x, out, work) == _lib.ERR_ARG                  # null ids (by-id route)
    assert _call(dev, es, None, ids, 4, 2, x, out, work) == _lib.ERR_ARG                   # the by-id route reads them on the device
    assert _call(dev, es, ids_d, ids, 6, 2, x, out, work, work.numel() - 1) == _lib.ERR_ARG   # short work buffer
    assert _call(dev, es, ids_d, ids, 6, 2, x, out, None, 0) == _lib.ERR_ARG
    assert _call(dev, es, ids_d, ids, 6, 0, x, out, work) == _lib.ERR_ARG
    assert _call(dev, es, ids_d, ids, 0, 2, x, out, work) == 0                             # no tokens: nothing to do, nothing written
    torch.cuda.synchronize()
    assert (out == 7.0).all()
    assert _call(dev, es, ids_d, ids, 6, 2, x, out, work) == 0                             # (the same arguments in order do run)
    torch.cuda.synchronize()
    assert _same_bits(dev, out, _batches(dev, q4, ids, x))
    # the batch route inside a capture needs the ids on the host: refused, and the capture goes on
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):
        rc_dev = _call(dev, es, ids_d, None, 6, 2, x, out, work)
        rc_host = _call(dev, es, ids_d, ids, 6, 2, x, out, work)
    assert rc_dev == _lib.ERR_ARG and rc_host == 0
    out.fill_(7.0)
    graph.replay()
    torch.cuda.synchronize()
    assert _same_bits(dev, out, _batches(dev, q4, ids, x))
    del graph
    es.free()


@pytest.mark.gpu
def test_a_set_over_two_devices_is_refused(dev):
    L = _lib.lib()
    if L.ggml_hip_n_slots() < 2 or L.ggml_hip_slot_device(0) == L.ggml_hip_slot_device(1):
        pytest.skip("one device slot")
    rows = _rows(dev, Q4_0, 96, 2048, 0).cpu().numpy()
    ws = []
    for g in (0, 1):
        assert L.ggml_hip_bind_thread(g) == 0
        ws.append(dev.Weight.from_host(Q4_0, rows, 2048))
    L.ggml_hip_bind_thread(-1)
    hw = (C.c_void_p * 2)(*[w.handle for w in ws])
    assert L.ggml_hip_expert_set_create(hw, 2, None, C.byref(C.c_void_p())) == _lib.ERR_ARG
