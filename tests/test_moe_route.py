"""The ends of a mixture-of-experts block (include/ggml_hip_ext.h ggml_hip_moe_route_dev, ggml_hip_moe_combine_dev,
ggml_hip_silu_mul_rows_dev; csrc/moe_route.hip, moe.cpp): router logits -> expert ids and gate weights on the device, the weighted sum of a
token's pair rows, the SwiGLU pair on device rows.

The yardsticks are the header's statements restated in numpy below:
  ids      exact: a stable sort by (NaN last, larger logit first, smaller index first); -0.0 == +0.0;
  weights  a float64 restatement on the same f32 logits, relative error <= 2^-18.  Derivation: l - lmax is rounded at magnitude up to 16
           (half an ulp = 2^-21 relative in the exponential), expf is within 1 ulp (2^-23), both once in the numerator and once in the sum;
           at most eleven further roundings of 2^-24 (the reduction, the divisions, the scale): about 1.9e-6 < 2^-18 = 3.8e-6;
  combine  exact: the float32 restatement, one rounding per product and per sum, ascending slots;
  silu_mul exact: the oracle's silu (GGML_SILU_FP16) and a float32 product -- what the silu_mul seam is held to (tests/test_fused.py).
Shapes are the smallest at which each mechanism can go wrong: fewer experts than lanes, one per lane, one past, sixteen per lane; one
token, a partial workgroup of tokens (5), several workgroups (70); row lengths below, at and past one vector and one workgroup.
The router kernel is picked by size (launch_moe_topk: 1, 2, 4, 8 or 16 experts per lane): the expert counts stand on both edges of every
rung (64 | 65, 128 | 129, 256 | 257, 512 | 513, 1024), ids and weights alike, and test_the_cases_reach_every_form_of_the_router counts
them.  The combine's slot loop is unrolled by four: n_used - 1 is a whole number of bodies (5, 9), leaves 1, 2 or 3 (6, 3, 64), and 64 is
the contract's maximum."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import oracle_lib as O
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32, Q8_0 = 0, 8
NEW_SYMBOLS = ("ggml_hip_moe_route_dev", "ggml_hip_moe_combine_dev", "ggml_hip_silu_mul_rows_dev")
SENTINEL = 0x7FC00123                                               # a NaN no kernel here produces


# ---------------------------------------------------------------- CPU
def test_the_three_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name


# ---------------------------------------------------------------- the numpy restatements
def np_route_ids(logits, n_used):
    """[T, n_used] int32: rank order under (a NaN after every number, larger logit first, smaller index first)"""
    l = np.asarray(logits, np.float32)
    isn = np.isnan(l)
    idx = np.broadcast_to(np.arange(l.shape[1]), l.shape)
    with np.errstate(invalid="ignore"):
        order = np.lexsort((idx, -np.where(isn, np.float32(0), l), isn), axis=1)       # (the last key is the primary one; -0.0 == 0.0)
    return order[:, :n_used].astype(np.int32)


def np_route_weights(logits, ids, gating, normalize, scale):
    """[T, n_used] float64, from the same f32 logits"""
    l = np.asarray(logits, np.float32).astype(np.float64)
    sel = np.take_along_axis(l, ids.astype(np.int64), axis=1)
    if gating == 0:
        lmax = sel[:, :1]
        w = np.exp(sel - lmax) / np.exp(l - lmax).sum(axis=1, keepdims=True)
    else:
        w = 1.0 / (1.0 + np.exp(-sel))
    if normalize:
        w = w / w.sum(axis=1, keepdims=True)
    return w * float(np.float32(scale))


def np_combine(y, w, addend=None):
    """y f32 [T, n_used, M], w f32 [T, n_used] -> f32 [T, M]: every product and every sum one binary32 rounding, ascending slots"""
    y, w = np.asarray(y, np.float32), np.asarray(w, np.float32)
    acc = w[:, 0, None] * y[:, 0, :]
    for s in range(1, y.shape[1]):
        acc = acc + w[:, s, None] * y[:, s, :]
    if addend is not None:
        acc = acc + np.asarray(addend, np.float32)
    assert acc.dtype == np.float32
    return acc


def test_the_restatements_on_rows_worked_by_hand():
    nan, inf = np.float32("nan"), np.float32("inf")
    rows = np.array([[1, 3, 3, 2, 3, 0], [nan, -inf, nan, -inf, 5, nan], [0.0, -0.0, -1, 0.0, -0.0, -2], [nan] * 6], np.float32)
    assert np_route_ids(rows, 4).tolist() == [[1, 2, 4, 3], [4, 1, 3, 0], [0, 1, 3, 4], [0, 1, 2, 3]]
    l = np.array([[0.0, np.log(3.0), -50.0]], np.float32)
    ids = np_route_ids(l, 2)
    assert ids.tolist() == [[1, 0]]
    assert np.allclose(np_route_weights(l, ids, 0, 0, 1.0), [[0.75, 0.25]], rtol=1e-6)
    assert np.allclose(np_route_weights(l, ids, 0, 1, 2.0), [[1.5, 0.5]], rtol=1e-6)
    assert np.allclose(np_route_weights(l, ids, 1, 0, 1.0), [[0.75, 0.5]], rtol=1e-6)
    y = np.array([[[1.0, 2.0], [10.0, 20.0]]], np.float32)
    assert np_combine(y, np.array([[0.5, 0.25]], np.float32), np.array([[1.0, 1.0]], np.float32)).tolist() == [[4.0, 7.0]]


# ---------------------------------------------------------------- the router's cases, and the kernel forms they select
IDS_EXPERTS = (2, 8, 60, 64, 65, 128, 129, 256, 257, 384, 512, 513, 1024)
SPECIAL_CASES = ((8, 4), (130, 8), (384, 8), (512, 64), (1024, 64))                    # (n_expert, n_used)
WEIGHT_CASES = ((8, 2), (60, 8), (65, 8), (128, 8), (129, 8), (256, 8), (257, 8), (384, 8), (512, 64), (513, 1), (1024, 64))
ROUTER_RUNGS = (1, 2, 4, 8, 16)


def _router_form(n_expert):
    """launch_moe_topk's ladder restated: the experts a lane holds"""
    npl = -(-n_expert // 64)
    return next(N for N in ROUTER_RUNGS if npl <= N)


def test_the_cases_reach_every_form_of_the_router():
    """A RESTATEMENT of launch_moe_topk's ladder (csrc/moe_route.hip): npl = ceil(n_expert / 64) rounded up to 1, 2, 4, 8, 16.  A change to
    the ladder there changes _router_form here.  The ids and the weights are each checked in all five forms, the ids on both edges of every
    rung past the first (64 N experts fill it, 32 N + 1 enter it); the special rows run in every form with more than two registers."""
    assert {_router_form(e) for e in IDS_EXPERTS} == set(ROUTER_RUNGS)
    assert {_router_form(e) for e, _ in WEIGHT_CASES} == set(ROUTER_RUNGS)
    for N in ROUTER_RUNGS[1:]:
        assert 64 * N in IDS_EXPERTS and 32 * N + 1 in IDS_EXPERTS, N
        assert _router_form(64 * N) == _router_form(32 * N + 1) == N
    for N in (4, 8):                                                  # the two rungs between the small shapes and 1024, weights on both edges
        assert {64 * N, 32 * N + 1} <= {e for e, _ in WEIGHT_CASES}, N
    assert {_router_form(e) for e, _ in SPECIAL_CASES} >= {1, 4, 8, 16}
    assert all(u <= e and u <= 64 for e, u in SPECIAL_CASES + WEIGHT_CASES)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


def _stream(dev):
    return C.c_void_p(dev.torch.cuda.current_stream().cuda_stream)


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _sentinel(dev, n):
    torch = dev.torch
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def _keeps_sentinel(dev, a):
    return bool((a.view(dev.torch.int32) == SENTINEL).all())


GUARD = 64       # elements


def _route(dev, logits_np, ld, n_used, gating, normalize, scale):
    """the entry on logits placed ld apart; the outputs sit between guards, which must keep their sentinel.  -> (ids, weights) numpy"""
    torch = dev.torch
    T, E = logits_np.shape
    buf = np.full((T, ld), np.float32(777.0), np.float32)            # (the padding columns hold a LARGER value than any logit: never read)
    buf[:, :E] = logits_np
    d_l = torch.from_numpy(buf).cuda()
    ids = _sentinel(dev, GUARD + T * n_used + GUARD)
    wts = _sentinel(dev, GUARD + T * n_used + GUARD)
    rc = _lib.lib().ggml_hip_moe_route_dev(_p(d_l.data_ptr()), ld, T, E, n_used, gating, normalize, scale, _p(ids.data_ptr() + 4 * GUARD),
                                           _p(wts.data_ptr() + 4 * GUARD), _stream(dev))
    assert rc == 0, _lib.lib().ggml_hip_last_error()
    torch.cuda.synchronize()
    for b in (ids, wts):
        assert _keeps_sentinel(dev, b[:GUARD]) and _keeps_sentinel(dev, b[GUARD + T * n_used:])
    body = slice(GUARD, GUARD + T * n_used)
    return ids[body].cpu().numpy().reshape(T, n_used), wts[body].view(torch.float32).cpu().numpy().reshape(T, n_used)


@pytest.mark.gpu
@pytest.mark.parametrize("n_expert", IDS_EXPERTS)
def test_the_ids_are_exact(dev, n_expert):
    rng = np.random.default_rng(n_expert)
    for n_tokens in (1, 5, 70):
        logits = rng.standard_normal((n_tokens, n_expert)).astype(np.float32)
        for n_used in sorted({min(u, n_expert) for u in (1, 2, 8, 64)}):
            want = np_route_ids(logits, n_used)
            for gating in (0, 1):
                for ld in (n_expert, n_expert + 3):
                    got, _ = _route(dev, logits, ld, n_used, gating, 1, 1.0)
                    assert np.array_equal(got, want), (n_expert, n_tokens, n_used, gating, ld)


def _special_rows(n_expert, n_used, rng):
    """name -> one row of logits.  Every one is data to the kernel, never an address."""
    nan, inf = np.float32("nan"), np.float32("inf")
    base = rng.standard_normal(n_expert).astype(np.float32)
    rows = {"all equal": np.full(n_expert, 1.5, np.float32)}
    perm = rng.permutation(n_expert)                                 # n_used - 1 times the largest value, then a tie of three across the boundary
    r = base.copy()
    r[perm[:n_used - 1]] = 10.0
    r[perm[n_used - 1:n_used + 2]] = 9.0
    rows["repeats straddle the boundary"] = r
    r = np.where(base > 0, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    r[n_expert // 2] = -1.0
    rows["zeros of both signs"] = r
    r = np.full(n_expert, -inf, np.float32)                          # two finite logits, fewer than n_used: the -inf follow by index
    r[n_expert - 1], r[1] = 0.25, -3.0
    rows["-inf but a few"] = r
    r = base.copy()
    r[rng.permutation(n_expert)[:max(1, n_expert // 3)]] = nan
    rows["NaNs scattered"] = r
    r = base.copy()
    r[0] = nan
    rows["NaN at index 0"] = r
    r = np.full(n_expert, nan, np.float32)                           # two numbers, one of them -inf: then the NaNs, in index order
    r[n_expert - 1], r[1] = 2.0, -inf
    rows["NaNs are reached"] = r
    rows["all NaN"] = np.full(n_expert, nan, np.float32)
    r = base.copy()
    r[n_expert - 2] = inf
    rows["+inf at one index"] = r
    r = base.copy()                                                  # lane 5 holds experts 5 + 64 j: every round takes one of ITS registers, in a shuffled order
    own = 5 + 64 * np.arange(min(n_used, (n_expert - 5 + 63) // 64))
    r[own] = np.float32(10.0) + rng.permutation(len(own)).astype(np.float32)
    rows["one lane owns every winner"] = r
    r = base.copy()                                                  # the n_used largest from n_expert - 1 downwards: the highest registers, the last lanes
    r[n_expert - 1 - np.arange(n_used)] = np.float32(10.0) + np.float32(0.25) * rng.permutation(n_used).astype(np.float32)
    rows["the last registers"] = r
    return rows


@pytest.mark.gpu
@pytest.mark.parametrize("n_expert,n_used", SPECIAL_CASES)
def test_the_special_rows_are_exact_on_ids(dev, n_expert, n_used):
    rng = np.random.default_rng(1000 + n_expert)
    n_tokens, where = 70, (0, 37, 69)
    for name, row in _special_rows(n_expert, n_used, rng).items():
        logits = rng.standard_normal((n_tokens, n_expert)).astype(np.float32)
        logits[list(where)] = row
        want = np_route_ids(logits, n_used)
        if name == "all equal":
            assert all(want[t].tolist() == list(range(n_used)) for t in where)
        for gating in (0, 1):
            got, _ = _route(dev, logits, n_expert + 3, n_used, gating, 1, 1.0)
            assert np.array_equal(got, want), (name, gating)
            for t in where:
                assert len(set(got[t].tolist())) == n_used and got[t].min() >= 0 and got[t].max() < n_expert, (name, gating, t)


@pytest.mark.gpu
@pytest.mark.parametrize("n_expert,n_used", WEIGHT_CASES)
def test_the_weights_are_within_the_derived_bound_of_the_float64_restatement(dev, n_expert, n_used):
    rng = np.random.default_rng(2000 + n_expert)
    logits = rng.uniform(-8.0, 8.0, (70, n_expert)).astype(np.float32)
    ids = np_route_ids(logits, n_used)
    for gating in (0, 1):
        for normalize in (0, 1):
            for scale in (1.0, 2.5):
                got_ids, got = _route(dev, logits, n_expert, n_used, gating, normalize, scale)
                assert np.array_equal(got_ids, ids)
                want = np_route_weights(logits, ids, gating, normalize, scale)
                rel = float(np.max(np.abs(got.astype(np.float64) - want) / want))
                print(f"n_expert {n_expert} n_used {n_used} gating {gating} normalize {normalize} scale {scale}: max relative error {rel:.3e}")
                assert rel <= 2.0 ** -18, (gating, normalize, scale, rel)
                if normalize == 1 and scale == 1.0:
                    off = float(np.max(np.abs(got.astype(np.float64).sum(axis=1) - 1.0)))
                    assert off <= n_used * 2.0 ** -23, (gating, off)


def _place(dev, rows2d, ld, off):
    """rows ld apart behind a base `off` floats past the allocation's start; everything around them holds the sentinel"""
    n, M = rows2d.shape
    host = np.full(off + n * ld + GUARD, SENTINEL, np.int32).view(np.float32)
    host[off:off + n * ld].reshape(n, ld)[:, :M] = rows2d
    return dev.torch.from_numpy(host).cuda()


def _combine(dev, d_y, d_w, T, U, M, ld, off, mode, add_np):
    """the entry on placed pair rows; mode 0 no addend, 1 an addend of its own, 2 dst IS the addend.  -> dst [T, M] numpy"""
    torch = dev.torch
    d_add = _place(dev, add_np, ld, off) if mode else None
    d_dst = d_add if mode == 2 else _sentinel(dev, off + T * ld + GUARD).view(torch.float32)
    rc = _lib.lib().ggml_hip_moe_combine_dev(_p(d_y.data_ptr() + 4 * off), ld, _p(d_w.data_ptr()), T, U, M,
                                             _p(d_add.data_ptr() + 4 * off) if mode else None, ld if mode else 0,
                                             _p(d_dst.data_ptr() + 4 * off), ld, _stream(dev))
    assert rc == 0, _lib.lib().ggml_hip_last_error()
    torch.cuda.synchronize()
    body = d_dst[off:off + T * ld].reshape(T, ld)
    assert _keeps_sentinel(dev, d_dst[:off]) and _keeps_sentinel(dev, d_dst[off + T * ld:]) and _keeps_sentinel(dev, body[:, M:])
    return body[:, :M].cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("M", (1, 7, 96, 4100))
def test_the_combine_is_bit_exact(dev, M):
    rng = np.random.default_rng(3000 + M)
    for n_tokens in (1, 70):
        for n_used in (1, 2, 8) + ((3, 5, 6, 9, 64) if M in (7, 4100) else ()):     # (the vector form's slot loop is unrolled by four)
            y = rng.standard_normal((n_tokens, n_used, M)).astype(np.float32)
            y[n_tokens // 2, n_used - 1] = 0.0                       # a pair row of +0.0f: what an id outside the set leaves
            if n_tokens > 1:
                y[0, :] = 0.0
            w = rng.uniform(0.0, 1.0, (n_tokens, n_used)).astype(np.float32)
            add = rng.standard_normal((n_tokens, M)).astype(np.float32)
            want = (np_combine(y, w), np_combine(y, w, add), np_combine(y, w, add))
            for pad, off in ((0, 0), (4, 0), (1, 0), (0, 1), (4, 1)):      # (a stride of M + 1, or a base 4 bytes on: the one-by-one form)
                d_y, d_w = _place(dev, y.reshape(-1, M), M + pad, off), dev.torch.from_numpy(w).cuda()
                for mode in (0, 1, 2):
                    got = _combine(dev, d_y, d_w, n_tokens, n_used, M, M + pad, off, mode, add)
                    assert np.array_equal(got.view(np.int32), want[mode].view(np.int32)), (M, n_tokens, n_used, pad, off, mode)


@pytest.mark.gpu
@pytest.mark.parametrize("nrows,k", ((3, 100), (70, 1024)))
def test_silu_mul_rows_is_bitwise_the_oracle_pair(dev, nrows, k):
    torch = dev.torch
    rng = np.random.default_rng(nrows)
    a, b = (3.0 * rng.standard_normal((nrows, k))).astype(np.float32), rng.standard_normal((nrows, k)).astype(np.float32)
    want_s = O.eltwise("silu", a)
    want_y = O.eltwise("mul", want_s, b)
    da, db = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
    s = _sentinel(dev, nrows * k + GUARD).view(torch.float32)
    y = _sentinel(dev, nrows * k + GUARD).view(torch.float32)
    dev.silu_mul_rows(da, db, silu=s[:nrows * k].view(nrows, k), out=y[:nrows * k].view(nrows, k))
    y2 = dev.silu_mul_rows(da, db)                                   # d_silu = NULL
    torch.cuda.synchronize()
    assert np.array_equal(s[:nrows * k].cpu().numpy().view(np.int32), want_s.reshape(-1).view(np.int32))
    assert np.array_equal(y[:nrows * k].cpu().numpy().view(np.int32), want_y.reshape(-1).view(np.int32))
    assert np.array_equal(y2.cpu().numpy().view(np.int32), want_y.view(np.int32))
    assert _keeps_sentinel(dev, s[nrows * k:]) and _keeps_sentinel(dev, y[nrows * k:])


@pytest.mark.gpu
def test_refusals_return_their_code_and_launch_nothing(dev):
    torch = dev.torch
    L = _lib.lib()
    T, E, U, M = 5, 8, 2, 12
    lg = torch.zeros((T, E), device="cuda")
    ids, wts = _sentinel(dev, T * U), _sentinel(dev, T * U)
    st = _stream(dev)

    def route(d_l=lg.data_ptr(), ld=E, n_tokens=T, n_expert=E, n_used=U, gating=0, d_ids=ids.data_ptr(), d_w=wts.data_ptr()):
        return L.ggml_hip_moe_route_dev(_p(d_l), ld, n_tokens, n_expert, n_used, gating, 1, 1.0, _p(d_ids), _p(d_w), st)

    assert route(n_expert=0) == route(n_expert=1025, ld=1025) == _lib.ERR_SHAPE
    assert route(n_used=0) == route(n_used=9) == route(n_expert=128, ld=128, n_used=65) == _lib.ERR_SHAPE
    assert route(n_tokens=(1 << 19) + 1) == _lib.ERR_SHAPE                                     # more than 2^20 pairs
    assert route(d_l=None) == route(d_ids=None) == route(d_w=None) == _lib.ERR_ARG
    assert route(ld=E - 1) == route(gating=2) == route(gating=-1) == route(n_tokens=-1) == _lib.ERR_ARG
    assert route(n_tokens=0) == 0
    y = torch.zeros((T * U, M), device="cuda")
    w = torch.zeros((T, U), device="cuda")
    add = torch.zeros((T, M), device="cuda")
    dst = _sentinel(dev, T * M)

    def combine(d_y=y.data_ptr(), ldy=M, d_w=w.data_ptr(), n_tokens=T, n_used=U, m=M, d_add=add.data_ptr(), ld_add=M, d_dst=dst.data_ptr(), ldd=M):
        return L.ggml_hip_moe_combine_dev(_p(d_y), ldy, _p(d_w), n_tokens, n_used, m, _p(d_add), ld_add, _p(d_dst), ldd, st)

    assert combine(ldy=M - 1) == combine(ldd=M - 1) == combine(ld_add=M - 1) == combine(m=0) == _lib.ERR_SHAPE
    assert combine(n_used=0) == combine(n_used=65) == combine(n_tokens=(1 << 19) + 1) == _lib.ERR_SHAPE
    assert combine(d_y=None) == combine(d_w=None) == combine(d_dst=None) == combine(n_tokens=-1) == _lib.ERR_ARG
    assert combine(n_tokens=0) == 0
    sm = _sentinel(dev, T * M)
    assert L.ggml_hip_silu_mul_rows_dev(None, _p(add.data_ptr()), None, _p(sm.data_ptr()), T, M, st) == _lib.ERR_ARG
    assert L.ggml_hip_silu_mul_rows_dev(_p(add.data_ptr()), None, None, _p(sm.data_ptr()), T, M, st) == _lib.ERR_ARG
    assert L.ggml_hip_silu_mul_rows_dev(_p(add.data_ptr()), _p(add.data_ptr()), None, None, T, M, st) == _lib.ERR_ARG
    assert L.ggml_hip_silu_mul_rows_dev(_p(add.data_ptr()), _p(add.data_ptr()), None, _p(sm.data_ptr()), 0, M, st) == 0
    torch.cuda.synchronize()
    assert all(_keeps_sentinel(dev, b) for b in (ids, wts, dst, sm))          # nothing was launched
    assert route() == 0 and combine(d_add=None, ld_add=0) == 0                # (the same arguments in order do run)
    torch.cuda.synchronize()
    assert ids.cpu().numpy().reshape(T, U).tolist() == [[0, 1]] * T and (dst.view(torch.float32) == 0).all()


# ---------------------------------------------------------------- the whole block, captured
N_EXPERT, N_TOKENS, N_USED, HIDDEN, FFN = 8, 70, 2, 1024, 1024


class _Block:
    """router F32 [HIDDEN -> N_EXPERT], gate / up [HIDDEN -> FFN] and down [FFN -> HIDDEN] Q8_0 expert sets, and one set of buffers"""

    def __init__(self, dev):
        torch = dev.torch
        g = torch.Generator(device="cuda")
        g.manual_seed(4242)
        rnd = lambda *shape: torch.randn(shape, generator=g, device="cuda")   # noqa: E731
        self.router = dev.Weight.from_device(F32, rnd(N_EXPERT, HIDDEN).contiguous(), HIDDEN)
        self.sets = []
        for (m, k) in ((FFN, HIDDEN), (FFN, HIDDEN), (HIDDEN, FFN)):
            ws = [dev.Weight.from_device(Q8_0, dev.quantize_rows(Q8_0, rnd(m, k) * 0.05).contiguous(), k) for _ in range(N_EXPERT)]
            self.sets.append(dev.ExpertSet(ws))
        assert all(s.grouped_serves() == 1 for s in self.sets)
        self.work_r = dev.alloc_work(F32, HIDDEN, N_TOKENS)
        self.work_g = torch.empty(max(s.grouped_work_size(N_TOKENS, N_USED) for s in self.sets), dtype=torch.uint8, device="cuda")

    def buffers(self, dev):
        torch = dev.torch
        z = lambda *shape, dt=torch.float32: torch.zeros(shape, dtype=dt, device="cuda")   # noqa: E731
        return dict(logits=z(N_TOKENS, N_EXPERT), ids=z(N_TOKENS, N_USED, dt=torch.int32), wts=z(N_TOKENS, N_USED), gate=z(N_TOKENS, N_USED, FFN),
                    up=z(N_TOKENS, N_USED, FFN), h=z(N_TOKENS, N_USED, FFN), down=z(N_TOKENS, N_USED, HIDDEN), out=z(N_TOKENS, HIDDEN))

    def run(self, dev, x, b):
        """router product -> route -> grouped gate and up (one src1 row per token) -> silu_mul_rows -> grouped down (a row per slot) -> combine + x"""
        dev.mul_mat(self.router, x, out=b["logits"], work=self.work_r)
        dev.moe_route(b["logits"], N_USED, gating=0, normalize=True, scale=1.0, ids=b["ids"], weights=b["wts"])
        dev.mul_mat_id_grouped(self.sets[0], b["ids"], x, out=b["gate"], work=self.work_g)
        dev.mul_mat_id_grouped(self.sets[1], b["ids"], x, out=b["up"], work=self.work_g)
        dev.silu_mul_rows(b["gate"].view(-1, FFN), b["up"].view(-1, FFN), out=b["h"].view(-1, FFN))
        dev.mul_mat_id_grouped(self.sets[2], b["ids"], b["h"], out=b["down"], work=self.work_g)
        dev.moe_combine(b["down"], b["wts"], addend=x, out=b["out"])


@pytest.mark.gpu
def test_the_whole_block_is_captured_and_replayed_with_other_tokens(dev):
    torch = dev.torch
    blk = _Block(dev)
    g = torch.Generator(device="cuda")
    g.manual_seed(77)
    x1, x2 = torch.randn((N_TOKENS, HIDDEN), generator=g, device="cuda"), torch.randn((N_TOKENS, HIDDEN), generator=g, device="cuda")
    eager1, eager2, b = blk.buffers(dev), blk.buffers(dev), blk.buffers(dev)
    blk.run(dev, x1, eager1)
    blk.run(dev, x2, eager2)
    torch.cuda.synchronize()
    assert not torch.equal(eager1["ids"], eager2["ids"])                   # the second batch is routed differently
    x = x1.clone()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                                          # (a first run outside the capture: the kernels' attributes are set)
        blk.run(dev, x, b)
    torch.cuda.current_stream().wait_stream(side)
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                          # captures on a side stream: one chain of launches
        blk.run(dev, x, b)
    for xs, eager in ((x1, eager1), (x2, eager2), (x1, eager1)):
        x.copy_(xs)
        b["out"].zero_()
        b["ids"].zero_()
        graph.replay()
        torch.cuda.synchronize()
        # (a) the replay is bitwise the same sequence run eagerly on that batch
        for name in ("logits", "ids", "wts", "gate", "up", "h", "down", "out"):
            assert torch.equal(b[name].view(torch.int32), eager[name].view(torch.int32)), name
        # (b) stage by stage on the device's own intermediates
        ids = b["ids"].cpu().numpy()
        assert np.array_equal(ids, np_route_ids(b["logits"].cpu().numpy(), N_USED))
        want = np_combine(b["down"].cpu().numpy(), b["wts"].cpu().numpy(), xs.cpu().numpy())
        assert np.array_equal(b["out"].cpu().numpy().view(np.int32), want.view(np.int32))
    del graph
    for s in blk.sets:
        s.free()
