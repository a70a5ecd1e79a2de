"""The rotary embedding on the device (include/ggml_hip_ext.h ROPE: ggml_hip_rope_table, ggml_hip_rope_dev, ggml_hip_rope_kv_store_dev;
csrc/rope.hip, rope.cpp).

Yardsticks (tests/np_rope.py): the header's table formulas in float64, the exact float64 rotation, and a numpy model of the float32
statement.  The bar per element is 4 * 2^-24 * mscale * (|x0| + |x1|), derived in np_rope's docstring, never measured from the kernels.
Bits: position 0 returns the input's values; elements beyond n_dims, the padding between rows and heads, and everything around a cache row
are untouched; a row's bits do not depend on the launch around it; the fused rotate-and-store equals rope then kv_store bit for bit.
Shapes: (D, n_dims) in {(64, 64), (128, 128), (128, 64), (64, 32), (12, 6)} -- whole and partial rotation, and (12, 6) on the
one-element-at-a-time path; n_head 1 / 4; n_tokens 1 / 3 / 130 (one token, a workgroup of several, more than one workgroup)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_attention as A
import np_rope as R
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, Q8_0 = A.F16, A.Q8_0
NEW_SYMBOLS = ("ggml_hip_rope_table", "ggml_hip_rope_dev", "ggml_hip_rope_kv_store_dev")


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _rp(p):
    return _lib.ggml_hip_rope_params_t(p["n_dims"], p["mode"], p["n_ctx_orig"], p["freq_base"], p["freq_scale"], p["ext_factor"], p["attn_factor"],
                                       p["beta_fast"], p["beta_slow"])


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name
    assert "ggml_hip_rope_params_t" in hdr and "ggml_hip_rope_params_t" in cs
    assert C.sizeof(_lib.ggml_hip_rope_params_t) == 36


def _table(p):
    eff = np.zeros(p["n_dims"] // 2, np.float64)
    ms = C.c_double()
    rc = _lib.lib().ggml_hip_rope_table(C.byref(_rp(p)), eff.ctypes.data_as(C.POINTER(C.c_double)), C.byref(ms))
    return rc, eff, ms.value


@pytest.mark.parametrize("name", ["plain", "scaled", "yarn"])
@pytest.mark.parametrize("n_dims", [6, 64, 128])
def test_the_table_is_the_headers_formulas(name, n_dims):
    """within 2^-48 relative: a formula mistake is >= 1e-3, the slack covers a few roundings and two libm calls"""
    p = R.params(n_dims, **R.PARAM_SETS[name])
    rc, eff, ms = _table(p)
    want, want_ms = R.table(p)
    assert rc == 0
    rel = np.abs(eff - want) / want
    print(name, n_dims, "worst relative", rel.max(), "mscale", ms, want_ms)
    assert rel.max() <= 2.0 ** -48 and abs(ms - want_ms) <= 2.0 ** -48 * want_ms
    if p["ext_factor"] == 0.0:
        assert ms == p["attn_factor"]
        assert _table(dict(p, attn_factor=float(np.float32(0.7))))[2] == float(np.float32(0.7))      # exactly, whatever freq_scale is
    else:
        assert ms > 1.0 and eff[0] == want[0] == 1.0                                 # YaRN: pair 0 extrapolates (mix = 1) ...
        if n_dims >= 64:                                                             # ... and a pair beyond `high` interpolates (mix = 0)
            assert abs(eff[-1] / (p["freq_base"] ** (-2.0 * (n_dims // 2 - 1) / n_dims)) - p["freq_scale"]) < 1e-12


GOOD = R.params(64, R.NORMAL)


def _rope_rc(p=GOOD, x=0x1000, ldx=(512, 128), n_head=4, D=128, n_tokens=2, pos=None, dst=0x1000, ldd=(512, 128)):
    return _lib.lib().ggml_hip_rope_dev(C.byref(_rp(p)), _p(x), ldx[0], ldx[1], n_head, D, n_tokens, _p(pos), 0, None, None, _p(dst), ldd[0], ldd[1], None)


def _fused_rc(p=GOOD, kv_type=F16, x=0x1000, ldx=(256, 128), n_head_kv=2, D=128, n_tokens=2, cache=0x1000, nb=(512, 256), n_pos_max=8):
    return _lib.lib().ggml_hip_rope_kv_store_dev(C.byref(_rp(p)), kv_type, _p(x), ldx[0], ldx[1], n_head_kv, D, n_tokens, None, _p(cache), nb[0], nb[1],
                                                 n_pos_max, 0, None, None)


def test_what_is_not_served_is_refused_before_anything_is_launched():
    """every call below carries pointers that are not device memory: a launch would fault, a refusal returns its code"""
    E = _lib
    nan, inf = float("nan"), float("inf")
    for rc in (_rope_rc, _fused_rc):
        for mode in (1, 3, 8, 24, -1):                                         # mrope, vision, anything else
            assert rc(p=dict(GOOD, mode=mode)) == E.ERR_ARG
        assert rc(p=dict(GOOD, n_dims=63)) == E.ERR_SHAPE and rc(p=dict(GOOD, n_dims=0)) == E.ERR_SHAPE
        assert rc(p=dict(GOOD, n_dims=130)) == E.ERR_SHAPE                      # n_dims > D
        assert rc(D=260, ldx=(2080, 260)) == E.ERR_SHAPE and rc(D=126) == E.ERR_SHAPE
        assert rc(x=0x1004) == E.ERR_SHAPE and rc(x=None) == E.ERR_ARG
        assert rc(ldx=(514, 128)) == E.ERR_SHAPE and rc(ldx=(512, 130)) == E.ERR_SHAPE and rc(ldx=(512, 124)) == E.ERR_SHAPE
        assert rc(p=dict(GOOD, freq_base=1.0)) == E.ERR_ARG and rc(p=dict(GOOD, freq_scale=0.0)) == E.ERR_ARG
        for k in ("freq_base", "freq_scale", "ext_factor", "attn_factor", "beta_fast", "beta_slow"):
            assert rc(p=dict(GOOD, **{k: nan})) == E.ERR_ARG and rc(p=dict(GOOD, **{k: inf})) == E.ERR_ARG, k
        assert rc(n_tokens=-1) == E.ERR_ARG
        assert rc(n_tokens=0, x=None) == 0                                      # an empty batch: OK, nothing written
    assert _rope_rc(n_head=0) == E.ERR_SHAPE and _rope_rc(n_head=65536) == E.ERR_SHAPE
    assert _rope_rc(dst=0x1008) == E.ERR_SHAPE and _rope_rc(ldd=(512, 126)) == E.ERR_SHAPE and _rope_rc(ldd=(510, 128)) == E.ERR_SHAPE
    assert _rope_rc(dst=None) == E.ERR_ARG
    for t in (0, 2, 7, 9, _lib.BF16):
        assert _fused_rc(kv_type=t) == E.ERR_TYPE
    assert _fused_rc(kv_type=Q8_0, D=48, p=R.params(32), ldx=(96, 48), nb=(256, 128)) == E.ERR_SHAPE     # Q8_0 rows are whole blocks of 32
    assert _fused_rc(kv_type=F16, D=48, p=R.params(32), ldx=(96, 48), nb=(256, 128), n_tokens=0) == 0  # (the same shape is an F16 row)
    assert _fused_rc(nb=(512, 128)) == E.ERR_SHAPE and _fused_rc(nb=(128, 512)) == E.ERR_SHAPE           # below the 256 bytes of a row
    assert _fused_rc(nb=(520, 256)) == E.ERR_SHAPE and _fused_rc(nb=(512, 264)) == E.ERR_SHAPE
    assert _fused_rc(kv_type=Q8_0, nb=(512, 128)) == E.ERR_SHAPE                                         # 144-byte rows
    assert _fused_rc(cache=0x1008) == E.ERR_SHAPE and _fused_rc(cache=None) == E.ERR_ARG
    assert _table(dict(GOOD, mode=1))[0] == E.ERR_ARG and _table(dict(GOOD, n_dims=7))[0] == E.ERR_SHAPE
    assert _table(dict(GOOD, ext_factor=1.0, n_ctx_orig=0))[0] == E.ERR_ARG


def test_the_model_constant_is_what_the_model_measures():
    """the numpy model of the float32 statement against the f64 reference on the GPU sweep: its worst statistic is the recorded constant
    (rounded up), and it sits below the derived bar of the kernels"""
    worst = {R.NORMAL: 0.0, R.NEOX: 0.0}
    for case in R.cases():
        x, pos, ff = R.inputs(case)
        p = R.case_params(case)
        worst[case[2]] = max(worst[case[2]], R.statistic(p, x, R.model(p, x, pos, ff), R.case_reference(case)))
    print("model worst", worst, "recorded", R.MODEL_WORST)
    w = max(worst.values())
    assert R.MODEL_WORST / 1.25 <= w <= R.MODEL_WORST < R.BAR, (worst, R.MODEL_WORST)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


PAD_X, PAD_Y = -3.0, -7.0


def _rope(dev, p, x, pos=None, pos0=0, d_pos0=None, ff=None, pad=(0, 0), in_place=False):
    """the entry on x f32 [n_tokens, n_head, D] (numpy) -> numpy; pad: extra elements (between heads, between tokens) in the strides of x and
    dst, checked untouched"""
    torch = dev.torch
    n_tokens, n_head, D = x.shape
    ph, pt = pad

    def padded(fill):
        buf = torch.full((n_tokens, n_head * (D + ph) + pt), fill, device="cuda")
        return buf, buf[:, :n_head * (D + ph)].view(n_tokens, n_head, D + ph)[:, :, :D]

    xbuf, xv = padded(PAD_X)
    xv.copy_(torch.from_numpy(np.ascontiguousarray(x)))
    ybuf, yv = (xbuf, xv) if in_place else padded(PAD_Y)
    before = xbuf.clone()
    d_pos = torch.from_numpy(np.asarray(pos, np.int32)).cuda() if pos is not None else None
    d_p0 = torch.tensor([d_pos0], dtype=torch.int32, device="cuda") if d_pos0 is not None else None
    d_ff = torch.from_numpy(ff).cuda() if ff is not None else None
    dev.rope(_rp(p), xv, pos=d_pos, pos0=pos0, d_pos0=d_p0, freq_factors=d_ff, out=yv)
    torch.cuda.synchronize()
    got = yv.cpu().numpy()
    mask = torch.ones_like(ybuf, dtype=torch.bool)
    mask[:, :n_head * (D + ph)].view(n_tokens, n_head, D + ph)[:, :, :D] = False
    assert bool((ybuf[mask] == (PAD_X if in_place else PAD_Y)).all()), "padding written"
    if not in_place:
        assert torch.equal(xbuf.view(torch.int32), before.view(torch.int32)), "source written"       # (bits: x may hold a NaN)
    return got


@pytest.mark.gpu
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("D,n_dims", R.SHAPES)
def test_every_case_of_the_sweep_is_inside_the_derived_bar(dev, D, n_dims, mode):
    worst = 0.0
    for i, case in enumerate(R.cases(D, n_dims, mode)):
        x, pos, ff = R.inputs(case)
        p = R.case_params(case)
        got = _rope(dev, p, x, pos=pos, ff=ff, pad=(4 * (i % 3), 8 * (i % 2)))
        st = R.statistic(p, x, got, R.case_reference(case))
        worst = max(worst, st)
        assert np.isfinite(got).all() and st <= R.BAR, (case, st, R.BAR)
    print((D, n_dims, mode), "worst statistic", worst, "bar", R.BAR, "model", R.MODEL_WORST)


@pytest.mark.gpu
@pytest.mark.parametrize("mode", R.MODES)
def test_exact_cases_position_zero_and_everything_that_is_not_rotated(dev, mode):
    rng = np.random.default_rng(3)
    for D, n_dims in R.SHAPES:
        p = R.params(n_dims, mode)
        x = rng.uniform(-1, 1, (5, 3, D)).astype(np.float32)
        x[0, 0, :4] = [0.0, -0.0, 1.0e-40, -2.5]                           # (a zero's sign may change at position 0: values, not bits)
        got = _rope(dev, p, x, pos=np.zeros(5, np.int32), pad=(4, 12))
        assert np.array_equal(got, x), (D, n_dims)
        got = _rope(dev, p, x, pos0=0, pad=(8, 0))[0]
        assert np.array_equal(got, x[0]), (D, n_dims)
        # beyond n_dims: bit for bit, NaN payloads and both zeros included, at a position that rotates (the padding is checked by _rope)
        if n_dims < D:
            x[1, 1, n_dims:n_dims + 3] = np.array([0x7FC01234, 0x80000000, 0x00000001], np.uint32).view(np.float32)
            for in_place in (False, True):
                got = _rope(dev, p, x, pos=np.array([5, 77, 4095, 1, 2], np.int32), pad=(4, 4), in_place=in_place)
                assert np.array_equal(got[..., n_dims:].view(np.uint32), x[..., n_dims:].view(np.uint32)), (D, n_dims, in_place)
                assert not np.array_equal(got[..., :n_dims], x[..., :n_dims])


@pytest.mark.gpu
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("D,n_dims", [(128, 128), (128, 64), (12, 6)])
def test_a_row_does_not_depend_on_the_launch_around_it(dev, D, n_dims, mode):
    """n_head, the strides, n_tokens, in place against out of place, and where the position comes from (d_pos, d_pos0, pos0)"""
    rng = np.random.default_rng([D, n_dims, mode])
    p = R.params(n_dims, mode, **R.PARAM_SETS["yarn"])
    n_tokens, n_head, p0 = 130, 4, 4000
    x = rng.uniform(-1, 1, (n_tokens, n_head, D)).astype(np.float32)
    ff = rng.uniform(1.0, 8.0, n_dims // 2).astype(np.float32)
    pos = np.arange(p0, p0 + n_tokens, dtype=np.int32)
    base = _rope(dev, p, x, pos=pos, ff=ff)
    same = lambda got, want, what: np.array_equal(got.view(np.uint32), want.view(np.uint32)) or pytest.fail("%s: %s" % (what, (D, n_dims, mode)))
    same(_rope(dev, p, x, pos0=p0, ff=ff), base, "pos0")
    same(_rope(dev, p, x, pos0=99, d_pos0=p0, ff=ff), base, "d_pos0")
    same(_rope(dev, p, x, pos=pos, ff=ff, pad=(8, 20)), base, "strides")
    same(_rope(dev, p, x, pos=pos, ff=ff, in_place=True), base, "in place")
    same(_rope(dev, p, x, pos=pos, ff=ff, pad=(4, 0), in_place=True), base, "in place, padded")
    same(_rope(dev, p, x[:, 2:3], pos=pos, ff=ff), base[:, 2:3], "n_head")
    for t in (0, 7, 129):
        same(_rope(dev, p, x[t:t + 1], pos=pos[t:t + 1], ff=ff), base[t:t + 1], "n_tokens")
        same(_rope(dev, p, x[t:t + 1, 1:2], pos0=p0 + t, ff=ff), base[t:t + 1, 1:2], "one row, pos0")
    same(_rope(dev, p, x[3:8], pos0=99, d_pos0=p0 + 3, ff=ff), base[3:8], "a few tokens, d_pos0")
    # shuffled positions follow the array, token by token
    perm = rng.permutation(n_tokens)
    same(_rope(dev, p, x[perm], pos=pos[perm], ff=ff), base[perm], "d_pos order")


class KCache:
    """one side of a cache as a padded device buffer of 0xA5 bytes.  layout 0: position-major (nb_head < nb_pos), 1: head-major (nb_head >
    nb_pos), 2: position-major with the heads as close as 16-byte alignment lets them be (D = 64 Q8_0: 72-byte rows, heads 80 bytes apart)"""

    def __init__(self, dev, kv_type, D, n_head_kv, n_pos, layout):
        rb = A.row_bytes(kv_type, D)
        up16 = lambda n: (n + 15) // 16 * 16
        if layout == 0:
            self.nb_head = up16(rb) + 16
            self.nb_pos = n_head_kv * self.nb_head + 32
        elif layout == 1:
            self.nb_pos = up16(rb) + 16
            self.nb_head = n_pos * self.nb_pos + 48
        else:
            self.nb_head = up16(rb)
            self.nb_pos = n_head_kv * self.nb_head
        self.rb, self.n_pos, self.n_head_kv = rb, n_pos, n_head_kv
        self.size = n_pos * self.nb_pos + n_head_kv * self.nb_head
        self.buf = dev.torch.full((self.size,), 0xA5, dtype=dev.torch.uint8, device="cuda")


def _unfused(dev, rp, kv_type, xv, cache, pos0, d_p0, d_ff):
    tmp = dev.rope(rp, xv, pos0=pos0, d_pos0=d_p0, freq_factors=d_ff)
    for hk in range(xv.shape[1]):
        dev.kv_store(kv_type, tmp[:, hk], cache.buf[hk * cache.nb_head:], cache.nb_pos, cache.n_pos, pos0=pos0, d_pos0=d_p0)
    return tmp


@pytest.mark.gpu
@pytest.mark.parametrize("mode", R.MODES)
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
@pytest.mark.parametrize("D,n_dims", [(64, 32), (64, 64), (128, 128), (64, 20)])       # (64, 20): the one-element-at-a-time path
def test_the_fused_store_is_rope_then_kv_store_bit_for_bit(dev, D, n_dims, kv_type, mode):
    torch = dev.torch
    rng = np.random.default_rng([D, n_dims, kv_type, mode])
    n_tokens, n_head_kv, n_pos = 5, 3, 12
    p = R.params(n_dims, mode, **R.PARAM_SETS["scaled"])
    x = rng.uniform(-1, 1, (n_tokens, n_head_kv, D)).astype(np.float32)
    x[1, 1, :32] = 0.0                                                         # an all-zero Q8_0 block (rotated zeros)
    xbuf = torch.zeros((n_tokens, n_head_kv, D + 4), device="cuda")
    xv = xbuf[:, :, :D]
    xv.copy_(torch.from_numpy(x))
    ff = torch.from_numpy(rng.uniform(1.0, 8.0, n_dims // 2).astype(np.float32)).cuda()
    for layout in (0, 1, 2):
        if layout == 2:
            assert (D, kv_type) != (64, Q8_0) or KCache(dev, kv_type, D, n_head_kv, n_pos, 2).nb_head == 80
        for p0 in (0, 3, n_pos - 2, -3, n_pos, -100):                          # inside, clipped at either end, wholly outside
            for on_device in (False, True):
                for d_ff in (None, ff):
                    fused, plain = KCache(dev, kv_type, D, n_head_kv, n_pos, layout), KCache(dev, kv_type, D, n_head_kv, n_pos, layout)
                    d_p0 = torch.tensor([p0], dtype=torch.int32, device="cuda") if on_device else None
                    host_p0 = 12345 if on_device else p0
                    dev.rope_kv_store(_rp(p), kv_type, xv, fused.buf, fused.nb_pos, fused.nb_head, n_pos, pos0=host_p0, d_pos0=d_p0, freq_factors=d_ff)
                    tmp = _unfused(dev, _rp(p), kv_type, xv, plain, host_p0, d_p0, d_ff)
                    torch.cuda.synchronize()
                    what = (D, n_dims, kv_type, mode, layout, p0, on_device, d_ff is not None)
                    assert torch.equal(fused.buf, plain.buf), what
                    # what the unfused pair wrote is where it belongs and nowhere else: the expected image from the rotated rows
                    want = np.full(fused.size, 0xA5, np.uint8)
                    rows = A.encode_rows(kv_type, tmp.cpu().numpy())
                    for t in range(n_tokens):
                        for hk in range(n_head_kv):
                            if 0 <= p0 + t < n_pos:
                                o = (p0 + t) * fused.nb_pos + hk * fused.nb_head
                                want[o:o + fused.rb] = rows[t, hk]
                    assert np.array_equal(fused.buf.cpu().numpy(), want), what


@pytest.mark.gpu
def test_a_captured_decode_step_rotates_stores_and_attends_by_two_device_integers(dev):
    """rope(q), rope_kv_store(k), kv_store(v), attention captured ONCE (hidden 1024: 8 heads of 128 over 2 kv heads, a Q8_0 cache); positions
    from one device int32, n_kv from another; replayed at positions 127, 128, 129 (across the chunk boundary).  Each replay equals the same
    four calls run eagerly with HOST positions bit for bit.  Against numpy: the K row the step wrote is the np_rope reference up to the Q8_0
    step (half a quantum of its block plus the rope bar), and the output is within TOL_DECODE of np_attention's reference for the np_rope
    reference of q over the cache as it stands (the way test_attention.py holds its layer test)."""
    torch = dev.torch
    D, n_head, n_head_kv, n_max, start = 128, 8, 2, 2 * A.CHUNK, A.CHUNK - 1
    rng = np.random.default_rng(41)
    p = R.params(D, R.NEOX, **R.PARAM_SETS["scaled"])
    rp = _rp(p)
    rb = A.row_bytes(Q8_0, D)
    nb_head, nb_pos = rb, n_head_kv * rb
    hist = rng.uniform(-1, 1, (2, start, n_head_kv, D)).astype(np.float32)
    kc = torch.full((n_max * nb_pos,), 0xFF, dtype=torch.uint8, device="cuda")
    vc = kc.clone()
    for c, h in ((kc, hist[0]), (vc, hist[1])):
        c[:start * nb_pos] = torch.from_numpy(A.encode_rows(Q8_0, h).reshape(-1)).cuda()
    q = torch.zeros((1, n_head, D), device="cuda")
    k = torch.zeros((1, n_head_kv, D), device="cuda")
    v = torch.zeros((1, n_head_kv, D), device="cuda")
    out = torch.zeros((1, n_head, D), device="cuda")
    work = torch.empty(dev.attn_work_size(Q8_0, D, n_head, n_head_kv, 1, n_max), dtype=torch.uint8, device="cuda")
    d_pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")

    def step(kcache, vcache, o, dp, dn, host_pos=0):
        qr = dev.rope(rp, q, pos0=host_pos, d_pos0=dp, out=step.qr)
        dev.rope_kv_store(rp, Q8_0, k, kcache, nb_pos, nb_head, n_max, pos0=host_pos, d_pos0=dp)
        dev.kv_store(Q8_0, v.view(1, n_head_kv * D), vcache, nb_pos, n_max, pos0=host_pos, d_pos0=dp)
        dev.attention(Q8_0, qr, kcache, vcache, nb_pos, nb_head, n_head_kv, host_pos + 1 if dn is None else 0, d_n_kv=dn, n_kv_max=n_max, out=o, work=work)

    step.qr = torch.zeros_like(q)
    d_pos.fill_(start)
    d_n.fill_(start + 1)
    step(kc.clone(), vc.clone(), torch.zeros_like(out), d_pos, d_n)            # (a first call outside the capture, on copies: one-time kernel attributes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(kc, vc, out, d_pos, d_n)
    torch.cuda.current_stream().wait_stream(s)
    fk, fv = kc.clone(), vc.clone()                                            # the eager calls keep a cache of their own
    for i in range(3):
        pos = start + i
        for t, shape in ((q, (1, n_head, D)), (k, (1, n_head_kv, D)), (v, (1, n_head_kv, D))):
            t.copy_(torch.from_numpy(rng.uniform(-1, 1, shape).astype(np.float32)))
        d_pos.fill_(pos)
        d_n.fill_(pos + 1)
        g.replay()
        torch.cuda.synchronize()
        got, got_q = out.clone(), step.qr.clone()
        fresh = torch.zeros_like(out)
        step(fk, fv, fresh, None, None, host_pos=pos)
        torch.cuda.synchronize()
        assert torch.equal(got, fresh) and torch.equal(got_q, step.qr) and torch.equal(kc, fk) and torch.equal(vc, fv), i
        # against numpy
        P = np.array([pos])
        q_ref, k_ref = R.reference(p, q.cpu().numpy(), P), R.reference(p, k.cpu().numpy(), P)
        assert R.statistic(p, q.cpu().numpy(), got_q.cpu().numpy(), q_ref) <= R.BAR
        n = pos + 1
        Kd = A.decode_rows(Q8_0, kc.cpu().numpy()[:n * nb_pos].reshape(n, n_head_kv, rb), D)
        Vd = A.decode_rows(Q8_0, vc.cpu().numpy()[:n * nb_pos].reshape(n, n_head_kv, rb), D)
        quantum = np.abs(k_ref[0]).reshape(n_head_kv, D // 32, 32).max(axis=-1, keepdims=True) / 127.0
        slack = quantum * (0.5 + 2.0 ** -14) + R.BAR * R.U * 2.0     # (v * id is good to 127 * 3 * 2^-24 quanta; |x0| + |x1| <= 2)
        assert (np.abs(Kd[pos].reshape(n_head_kv, D // 32, 32) - k_ref[0].reshape(n_head_kv, D // 32, 32)) <= slack).all(), i
        assert np.array_equal(Vd[pos], A.decode_rows(Q8_0, A.encode_rows(Q8_0, v.cpu().numpy()[0]), D))
        ref = A.reference(q_ref, Kd, Vd, n, True, 1.0 / np.sqrt(D))
        stat = A.statistic(got.cpu().numpy(), ref, Vd)
        print("position", pos, "attention statistic", stat, "bar", A.TOL_DECODE)
        assert stat <= A.TOL_DECODE, (i, stat)
