"""The attention options over either KV cache: a sliding window, attention sinks, a logit soft-cap (include/ggml_hip_ext.h, ATTENTION OPTIONS:
ggml_hip_attn_ex_plan, ggml_hip_attn_ex_dev, ggml_hip_attn_paged_ex_plan, ggml_hip_attn_paged_ex_dev; csrc/attn.hip, attn.cpp, plan.cpp
plan_attn_ex).

Yardsticks (tests/np_attention_ex.py): the float64 attention over the DEQUANTIZED cache under the options, never the library; the statistic
max |dst - ref| / max |V|; the bar per form is 4 x what the numpy model of the header's arithmetic measures on this sweep (TOL_DECODE_EX,
TOL_PROMPT_EX; both recomputed on the CPU here).  The sweep's inputs are shaped so that every option that can act moves dst by at least
100 x its bar (checked on the CPU): a kernel that ignores an option cannot pass.  The header's CONSEQUENCES are held to bits: everything off
is the base entry; a window >= n_kv is no window; sinks of -inf are no sinks; a windowed call is the windowed (for n_q = 1: the BASE) call on the
cache advanced by whole chunks; the base invariances; a paged sequence is the contiguous _ex call, with the table entries below the window
holding anything.
Shapes: chunk = 128; n_kv in {1, 129, 379}; n_q 1, 3 (DECODE), 9, 130 (PROMPT: the smallest, and two query tiles); W in {1, 5, 123, 128, 200}
(inside a chunk, a whole chunk, across two); D 64 / 128; heads (4, 2), (8, 1); both cache types; both layouts; buffers pre-filled with 0xFF."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_attention as A
import np_attention_ex as X
import test_attention as T                                           # Cache: the padded 0xFF-filled device cache of the base tests
import test_attention_paged as P                                     # Pool, _geometry: the 0xFF-filled page pool of the paged tests
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, Q8_0 = A.F16, A.Q8_0
NEW_SYMBOLS = ("ggml_hip_attn_ex_plan", "ggml_hip_attn_ex_dev", "ggml_hip_attn_paged_ex_plan", "ggml_hip_attn_paged_ex_dev")
DECODE, PROMPT = 1, 2
PAGE = A.CHUNK
NINF = float("-inf")


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _last_error():
    return _lib.lib().ggml_hip_last_error().decode(errors="replace")


def _opts(window=0, softcap=0.0, sinks=None, reserved=0):
    return _lib.ggml_hip_attn_opts_t(sinks, window, softcap, reserved)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    exports = open(os.path.join(ROOT, "ggmlsharp_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ggml_hip_\*;", exports)            # the export list is the ggml_hip_ prefix
    assert re.search(r"typedef struct ggml_hip_attn_opts_t\s*\{", hdr)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name
    assert not hasattr(L, "ggml_hip_attn_ex_work_size") and not hasattr(L, "ggml_hip_attn_paged_ex_work_size")      # the base work sizes serve


def _plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max):
    out = _lib.ggml_hip_attn_plan_t()
    return _lib.lib().ggml_hip_attn_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, C.byref(out)), out


def _plan_ex(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, opts):
    out = _lib.ggml_hip_attn_plan_t()
    return _lib.lib().ggml_hip_attn_ex_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, None if opts is None else C.byref(opts), C.byref(out)), out


def _plan_paged_ex(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, opts):
    out = _lib.ggml_hip_attn_plan_t()
    return _lib.lib().ggml_hip_attn_paged_ex_plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, None if opts is None else C.byref(opts), C.byref(out)), out


def _fields(p):
    return (p.form, p.chunk, p.q_tile, p.launches, p.n_chunks, p.workgroups)


def _attn_rc(opts, causal=1, n_q=1, work_bytes=1 << 30, ptr=0x1000):
    o = None if opts is None else C.byref(opts)
    return _lib.lib().ggml_hip_attn_ex_dev(F16, _p(ptr), 512, 128, _p(ptr), _p(ptr), 512, 256, 4, 2, 128, n_q, 16, None, 16, causal, 0.125, o, _p(ptr), 512, 128,
                                           _p(0x1000), work_bytes, None)


def _paged_rc(opts, causal=1, n_q=1, work_bytes=1 << 30, ptr=0x1000):
    o = None if opts is None else C.byref(opts)
    nb = P._geometry(F16, 128, 2, 0)
    return _lib.lib().ggml_hip_attn_paged_ex_dev(F16, _p(ptr), 512, 128, _p(ptr), _p(ptr), nb[0], nb[1], nb[2], 4, _p(0x1000), 2, _p(0x1000), 1, 2, 4, 2, 128, n_q, 256,
                                                 causal, 0.125, o, _p(ptr), 512, 128, _p(0x1000), work_bytes, None)


def test_every_new_refusal_is_decided_before_anything_is_launched():
    """every call below carries pointers that are not device memory: a launch would fault, a refusal returns its code"""
    E = _lib
    bad = [_opts(window=-1), _opts(window=-(1 << 40)), _opts(softcap=-1.0), _opts(softcap=float("inf")), _opts(softcap=float("nan")), _opts(softcap=-0.5, window=4),
           _opts(sinks=0x1002), _opts(sinks=0x1001, window=3), _opts(reserved=1), _opts(reserved=-1, window=5)]
    for rc_of in (_attn_rc, _paged_rc):
        for o in bad:
            assert rc_of(o) == E.ERR_ARG, (rc_of.__name__, o.window, o.logit_softcap, o.d_sinks, o.reserved)
        assert rc_of(_opts(window=1), causal=0) == E.ERR_ARG and rc_of(_opts(window=1 << 40), causal=0) == E.ERR_ARG      # a window needs causal
        # the base entry's rules stand behind the new ones: alignment, the work buffer, an empty batch
        for o in (None, _opts(), _opts(window=5, softcap=0.5, sinks=0x1000), _opts(window=1 << 40)):
            assert rc_of(o, ptr=0x1004) == E.ERR_SHAPE
            assert rc_of(o, work_bytes=64) == E.ERR_ARG
            assert rc_of(o, n_q=0) == 0
        assert rc_of(_opts(softcap=1.0), causal=0, n_q=0) == 0 and rc_of(_opts(sinks=0x1000), causal=0, n_q=0) == 0       # only the window needs causal
    for o in bad:
        assert _plan_ex(F16, 128, 4, 2, 1, 4096, o)[0] == E.ERR_ARG and _plan_paged_ex(F16, 128, 4, 2, 2, 1, 4096, o)[0] == E.ERR_ARG
    assert _plan_ex(F16, 96, 4, 2, 1, 16, _opts(window=4))[0] == E.ERR_SHAPE and _plan_ex(2, 128, 4, 2, 1, 16, None)[0] == E.ERR_TYPE
    assert _plan_paged_ex(F16, 128, 4, 2, 0, 1, 128, _opts(window=4))[0] == E.ERR_SHAPE and _plan_paged_ex(F16, 128, 4, 2, 4097, 1, 128, None)[0] == E.ERR_SHAPE
    # the work size the _ex entries ask for IS the base entry's: one byte less than it is refused, by the base function's name
    L = _lib.lib()
    need = L.ggml_hip_attn_work_size(F16, 128, 4, 2, 1, 16)
    assert need > 0 and _attn_rc(_opts(window=4), work_bytes=need - 1) == E.ERR_ARG and "ggml_hip_attn_work_size" in _last_error()
    need = L.ggml_hip_attn_paged_work_size(F16, 128, 4, 2, 2, 1, 256)
    assert need > 0 and _paged_rc(_opts(window=4), work_bytes=need - 1) == E.ERR_ARG and "ggml_hip_attn_paged_work_size" in _last_error()


def test_null_and_all_off_options_plan_like_the_base_entries():
    for kv_type in (F16, Q8_0):
        for D in (64, 128):
            for n_head, n_head_kv in ((4, 2), (8, 1), (32, 8)):
                for n_q in (0, 1, 3, 8, 9, 130, 4096):
                    for n_kv_max in (0, 1, 128, 129, 5000, 1 << 20):
                        rc, base = _plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max)
                        assert rc == 0
                        for o in (None, _opts(), _opts(softcap=0.5), _opts(sinks=0x1000), _opts(softcap=30.0, sinks=0x1000)):      # no window: the base grid
                            rc, p = _plan_ex(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, o)
                            assert rc == 0 and _fields(p) == _fields(base), (n_q, n_kv_max)
                        for n_seq in (1, 3, 32):
                            pb = _lib.ggml_hip_attn_plan_t()
                            assert _lib.lib().ggml_hip_attn_paged_plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, C.byref(pb)) == 0
                            for o in (None, _opts()):
                                rc, p = _plan_paged_ex(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, o)
                                assert rc == 0 and _fields(p) == _fields(pb), (n_seq, n_q, n_kv_max)


def test_the_windowed_decode_grid_follows_the_window_and_nothing_else_moves():
    cdiv = lambda a, b: (a + b - 1) // b
    for kv_type, D, n_head, n_head_kv in ((F16, 128, 32, 8), (Q8_0, 64, 8, 1), (F16, 64, 4, 2)):
        for n_q in (1, 3, 8, 9, 130):
            for W in (1, 5, 127, 128, 129, 1024, 4096, 1 << 20, 1 << 40):
                for n_kv_max in (0, 1, 128, 129, 1000, 4096, 1 << 20):
                    _, base = _plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max)
                    rc, p = _plan_ex(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, _opts(window=W, softcap=0.5))
                    assert rc == 0 and (p.form, p.chunk, p.q_tile, p.launches) == (base.form, base.chunk, base.q_tile, base.launches)
                    if p.form == DECODE:
                        want = min(cdiv(n_kv_max, PAGE), cdiv(W + n_q - 1, PAGE) + 1)
                        assert p.n_chunks == want and p.workgroups == want * n_head_kv, (n_q, W, n_kv_max, p.n_chunks, want)
                        if W >= n_kv_max:
                            assert _fields(p) == _fields(base)
                    else:
                        assert _fields(p) == _fields(base)                     # the PROMPT plan is unchanged by the options
                    for n_seq in (1, 2, 32):
                        rc, pp = _plan_paged_ex(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, _opts(window=W))
                        assert rc == 0 and _fields(pp)[:5] == _fields(p)[:5] and pp.workgroups == n_seq * p.workgroups
        a, b = (_plan_ex(kv_type, D, n_head, n_head_kv, 1, n, _opts(window=1024))[1] for n in (4096, 1 << 20))
        assert _fields(a) == _fields(b) and a.n_chunks == 9                   # past the window the grid does not grow with n_kv_max
    # the work-size functions are untouched: still the base plan's partials, whatever window a caller has in mind
    L = _lib.lib()
    for n_kv_max in (128, 4096, 1 << 16):
        w = L.ggml_hip_attn_work_size(F16, 128, 8, 2, 3, n_kv_max)
        assert w >= 3 * 8 * cdiv(n_kv_max, PAGE) * 132 * 4 and w == L.ggml_hip_attn_paged_work_size(F16, 128, 8, 2, 1, 3, n_kv_max)


def test_the_numpy_model_honours_the_consequences_exactly():
    """1: everything off is np_attention's functions; 2: a window >= n_kv is no window; 3: sinks of -inf are no sinks -- reference and both models"""
    for form, model, base_model in (("decode", X.model_decode, A.model_decode), ("prompt", X.model_prompt, A.model_prompt)):
        for shape in [s for s in X.shapes(form) if s[:4] in ((64, 4, 2, Q8_0), (128, 8, 1, F16))]:
            D, n_head, _, _, n_q, n_kv = shape
            q, _, _, Kd, Vd = X.inputs(shape)
            sc = 1.0 / np.sqrt(D)
            off = model(q, Kd, Vd, n_kv, True, sc)
            assert np.array_equal(bits(off), bits(base_model(q, Kd, Vd, n_kv, True, sc)))
            assert np.array_equal(X.reference(q, Kd, Vd, n_kv, True, sc), A.reference(q, Kd, Vd, n_kv, True, sc))
            for W in (n_kv, n_kv + 1, 1 << 40):
                assert np.array_equal(bits(model(q, Kd, Vd, n_kv, True, sc, window=W)), bits(off)), (shape, W)
                assert np.array_equal(X.reference(q, Kd, Vd, n_kv, True, sc, window=W), X.reference(q, Kd, Vd, n_kv, True, sc))
            none = np.full(n_head, NINF, np.float32)
            assert np.array_equal(bits(model(q, Kd, Vd, n_kv, True, sc, sinks=none)), bits(off)), shape
            capped = model(q, Kd, Vd, n_kv, True, sc, window=5, softcap=0.5)
            assert np.array_equal(bits(model(q, Kd, Vd, n_kv, True, sc, window=5, softcap=0.5, sinks=none)), bits(capped)), shape
            assert np.allclose(X.reference(q, Kd, Vd, n_kv, True, sc, sinks=none), X.reference(q, Kd, Vd, n_kv, True, sc), rtol=1e-15, atol=0)


_MODEL = {}


def _model_sweep(form):
    """(the model's worst statistic, the smallest distance of an acting variant from the unvaried reference, its case) on the sweep, computed once"""
    if form not in _MODEL:
        fn = X.model_decode if form == "decode" else X.model_prompt
        worst, least, who = 0.0, np.inf, None
        for shape in X.shapes(form):
            q, _, _, Kd, Vd = X.inputs(shape)
            for v in X.variants(shape[1]):
                ref = X.case_reference(shape, v)
                worst = max(worst, A.statistic(fn(q, Kd, Vd, shape[5], True, 1.0 / np.sqrt(shape[0]), *v), ref, Vd))
                if X.can_act(shape, v):
                    d = A.statistic(X.case_reference(shape), ref, Vd)
                    if d < least:
                        least, who = d, (shape, v[0], v[1], v[2] is not None)
        _MODEL[form] = (worst, least, who)
    return _MODEL[form]


@pytest.mark.parametrize("form", ["decode", "prompt"])
def test_the_ex_model_constants_are_what_the_model_measures(form):
    rec = X.MODEL_WORST_DECODE_EX if form == "decode" else X.MODEL_WORST_PROMPT_EX
    worst = _model_sweep(form)[0]
    print(form, "model worst", worst, "recorded", rec)
    assert rec / 1.25 <= worst <= rec, (form, worst, rec)
    tol, base_rec, base_tol = ((X.TOL_DECODE_EX, A.MODEL_WORST_DECODE, A.TOL_DECODE) if form == "decode" else (X.TOL_PROMPT_EX, A.MODEL_WORST_PROMPT, A.TOL_PROMPT))
    assert tol == (4 * rec if rec > base_rec else base_tol)


@pytest.mark.parametrize("form", ["decode", "prompt"])
def test_every_variant_case_differs_from_the_unvaried_reference(form):
    """a condition on the INPUTS: wherever an option can act at all, the varied f64 reference is at least 100 bars away from the unvaried one"""
    tol = X.TOL_DECODE_EX if form == "decode" else X.TOL_PROMPT_EX
    _, least, who = _model_sweep(form)
    print(form, "smallest distance", least, "at", who, "100 bars", 100 * tol)
    assert least >= 100 * tol, (form, least, who)
    acting = sum(X.can_act(s, v) for s in X.shapes(form) for v in X.variants(s[1]))
    assert acting >= 0.75 * len(X.shapes(form)) * len(X.variants(4))           # (the rest: n_kv = 1, or a window no row reaches)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


_CACHES = {}


def _cache(dev, shape, layout, heads=None):
    """the 0xFF-filled device cache of a shape's rows, built once per (shape, layout, head slice)"""
    key = (shape, layout, None if heads is None else (heads.start, heads.stop))
    if key not in _CACHES:
        D, n_head, n_head_kv, kv_type, _, n_kv = shape
        _, Kraw, Vraw, _, _ = X.inputs(shape)
        if heads is not None:
            G = n_head // n_head_kv
            Kraw, Vraw = Kraw[:, heads.start // G:heads.stop // G], Vraw[:, heads.start // G:heads.stop // G]
        _CACHES[key] = T.Cache(dev, kv_type, D, Kraw.shape[1], n_kv + 700, layout, Kraw, Vraw)
    return _CACHES[key]


def run(dev, shape, variant=(0, 0.0, None), layout=0, entry="py", causal=True, n_kv=None, n_kv_max=None, device_n_kv=False, pad=0, heads=None, rows=None,
        advance=0, q=None):
    """one contiguous call on a shape of the sweep -> numpy [n_q, n_head, D].  entry: "py" device.attention with the keyword options (the base
    entry when all are off), "ex" ggml_hip_attn_ex_dev with an options struct whatever it holds, "null" the same with opts = NULL.
    advance: the cache pointers moved forward by this many positions (n_kv is then the caller's); pad / heads / rows / n_kv as test_attention._run"""
    torch = dev.torch
    D, n_head, n_head_kv, kv_type, n_q, case_n_kv = shape
    window, softcap, sinks = variant
    q = X.inputs(shape)[0] if q is None else q
    n_kv = case_n_kv if n_kv is None else n_kv
    cache = _cache(dev, shape, layout, heads)
    if heads is not None:
        q = q[:, heads]
        sinks = None if sinks is None else sinks[heads]
        n_head, n_head_kv = q.shape[1], cache.n_head_kv
    if rows is not None:
        q = q[rows]
        n_q = q.shape[0]
    n_kv_max = n_kv if n_kv_max is None else n_kv_max
    qd = torch.zeros((n_q, n_head, D + pad), device="cuda")
    qd[:, :, :D] = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    out = torch.full((n_q, n_head, D + pad), -7.0, device="cuda")
    d_n = torch.tensor([n_kv], dtype=torch.int32, device="cuda") if device_n_kv else None
    d_s = None if sinks is None else torch.from_numpy(np.ascontiguousarray(sinks)).cuda()
    k, v = cache.k[advance * cache.nb_pos:], cache.v[advance * cache.nb_pos:]
    if entry == "py":
        dev.attention(kv_type, qd[:, :, :D], k, v, cache.nb_pos, cache.nb_head, n_head_kv, 0 if device_n_kv else n_kv, d_n_kv=d_n, n_kv_max=n_kv_max,
                      causal=causal, out=out[:, :, :D], window=window, softcap=softcap, sinks=d_s)
    else:
        work = torch.empty(max(dev.attn_work_size(kv_type, D, n_head, n_head_kv, n_q, n_kv_max), 16), dtype=torch.uint8, device="cuda")
        o = _opts(window, softcap, None if d_s is None else d_s.data_ptr())
        rc = _lib.lib().ggml_hip_attn_ex_dev(kv_type, _p(qd.data_ptr()), qd.stride(0), qd.stride(1), _p(k.data_ptr()), _p(v.data_ptr()), cache.nb_pos, cache.nb_head,
                                             n_head, n_head_kv, D, n_q, 0 if device_n_kv else n_kv, None if d_n is None else _p(d_n.data_ptr()), n_kv_max,
                                             int(causal), 1.0 / float(np.sqrt(np.float64(D))), None if entry == "null" else C.byref(o), _p(out.data_ptr()),
                                             out.stride(0), out.stride(1), _p(work.data_ptr()), work.numel(), _p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, _last_error()
    torch.cuda.synchronize()
    if pad:
        assert bool((out[:, :, D:] == -7.0).all())
    return out[:, :, :D].cpu().numpy()


SWEEP = [(D, nh, nhk, t) for D in (64, 128) for nh, nhk in X.HEADS for t in (F16, Q8_0)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["decode", "prompt"])
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_every_case_of_the_sweep_is_inside_four_times_the_model(dev, form, D, n_head, n_head_kv, kv_type):
    tol = X.TOL_DECODE_EX if form == "decode" else X.TOL_PROMPT_EX
    i = 0
    for shape in (s for s in X.shapes(form) if s[:4] == (D, n_head, n_head_kv, kv_type)):
        rc, p = _plan_ex(kv_type, D, n_head, n_head_kv, shape[4], shape[5], _opts(window=5))
        assert rc == 0 and p.form == (DECODE if form == "decode" else PROMPT)
        Vd = X.inputs(shape)[4]
        for v in X.variants(n_head):
            got = run(dev, shape, v, layout=i % 2, pad=4 * (i % 3))
            st = A.statistic(got, X.case_reference(shape, v), Vd)
            print(form, shape, v[0], v[1], v[2] is not None, "statistic", st, "bar", tol)
            assert np.isfinite(got).all() and st <= tol, (shape, v[0], v[1], v[2] is not None, st, tol)
            i += 1


@pytest.mark.gpu
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_consequences_1_to_3_hold_to_the_bit(dev, D, n_head, n_head_kv, kv_type):
    none = np.full(n_head, NINF, np.float32)
    sinks = X.sinks_of(n_head)
    for n_q in (1, 3, 9, 130):
        for n_kv in (1, 379):
            shape = (D, n_head, n_head_kv, kv_type, n_q, n_kv)
            for causal in (False, True):
                base = run(dev, shape, causal=causal)                                   # ggml_hip_attn_dev
                assert np.array_equal(bits(base), bits(run(dev, shape, entry="null", causal=causal))), ("1: opts = NULL", shape, causal)
                assert np.array_equal(bits(base), bits(run(dev, shape, entry="ex", causal=causal))), ("1: everything off", shape, causal)
                assert np.array_equal(bits(base), bits(run(dev, shape, (0, 0.0, none), entry="ex", causal=causal))), ("3: sinks -inf", shape, causal)
            for W in (n_kv, n_kv + 1, 1 << 40):
                assert np.array_equal(bits(base), bits(run(dev, shape, (W, 0.0, None), entry="ex"))), ("2: window >= n_kv", shape, W)
                some = run(dev, shape, (0, X.SOFTCAP, sinks))
                assert np.array_equal(bits(some), bits(run(dev, shape, (W, X.SOFTCAP, sinks)))), ("2: under sinks and a cap", shape, W)
            capped = run(dev, shape, (123, X.SOFTCAP, None))
            assert np.array_equal(bits(capped), bits(run(dev, shape, (123, X.SOFTCAP, none)))), ("3: under a window and a cap", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_consequence_4_translation_by_whole_chunks(dev, D, n_head, n_head_kv, kv_type):
    W = 123
    # n_q = 1, n_kv = 379: n_kv - W = 256, so the windowed call IS the base entry on the cache advanced by 256 positions with n_kv' = W
    shape = (D, n_head, n_head_kv, kv_type, 1, 379)
    for layout in (0, 1):
        got = run(dev, shape, (W, 0.0, None), layout=layout)
        assert np.array_equal(bits(got), bits(run(dev, shape, layout=layout, advance=256, n_kv=W))), ("the base entry on the advanced cache", shape, layout)
        assert np.array_equal(bits(got), bits(run(dev, shape, (W, 0.0, None), layout=layout, advance=128, n_kv=379 - 128))), ("one chunk", shape, layout)
    # n_q = 3 (DECODE) and 130 (PROMPT) translated by one chunk, sinks and the cap on: lo_0 = 379 - n_q + 1 - W is 254 / 127
    sinks = X.sinks_of(n_head)
    for n_q, Wq in ((3, 123), (130, 100)):                           # (lo_0 = 254; lo_0 = 150: both in chunk 1)
        shape = (D, n_head, n_head_kv, kv_type, n_q, 379)
        v = (Wq, X.SOFTCAP, sinks)
        got = run(dev, shape, v)
        assert np.array_equal(bits(got), bits(run(dev, shape, v, advance=128, n_kv=379 - 128))), ("one chunk", shape)
        assert np.array_equal(bits(got), bits(run(dev, shape, v, layout=1, advance=128, n_kv=379 - 128, n_kv_max=1000, device_n_kv=True))), ("one chunk, n_kv on the device", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
@pytest.mark.parametrize("D", [64, 128])
def test_exact_cases_half_of_v_and_no_visible_position(dev, D, kv_type):
    for n_head, n_head_kv in X.HEADS:
        G = n_head // n_head_kv
        zero_sinks = np.zeros(n_head, np.float32)
        # q = 0, sink = 0, one visible position: s = 0 = sink, p = 1, L = 1 + 1 -- dst = deq(V_j) / 2 bit for bit in DECODE
        for n_q in (1, 3):
            shape = (D, n_head, n_head_kv, kv_type, n_q, 379)
            Vd = X.inputs(shape)[4]
            q0 = np.zeros((n_q, n_head, D), np.float32)
            got = run(dev, shape, (1, 0.0, zero_sinks), q=q0)                           # W = 1: row t sees position 379 - n_q + t alone
            for t in range(n_q):
                for h in range(n_head):
                    assert np.array_equal(bits(got[t, h]), bits(Vd[379 - n_q + t, h // G] / np.float32(2))), ("half of V", shape, t, h)
            got = run(dev, shape, (1, X.SOFTCAP, zero_sinks), q=q0)                     # tanhf(0) = 0: the cap changes nothing here
            assert np.array_equal(bits(got[n_q - 1, 0]), bits(Vd[378, 0] / np.float32(2)))
        # no visible position writes +0.0f with sinks given: n_kv = 0 on the device over a cache that has room, both forms; and the rows above
        # the cache's first position when n_q > n_kv
        for n_q in (1, 3, 9, 130):
            shape = (D, n_head, n_head_kv, kv_type, n_q, 379)
            for v in ((0, 0.0, X.sinks_of(n_head)), (5, X.SOFTCAP, X.sinks_of(n_head))):
                got = run(dev, shape, v, n_kv=0, n_kv_max=300, device_n_kv=True)
                assert np.array_equal(bits(got), np.zeros_like(bits(got))), ("n_kv = 0", shape, v[0])
            if n_q > 1:
                got = run(dev, shape, (5, 0.0, X.sinks_of(n_head)), n_kv=1)             # only the last row sees position 0
                assert np.array_equal(bits(got[:-1]), np.zeros_like(bits(got[:-1]))) and np.abs(got[-1]).max() > 0, ("n_kv = 1", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
@pytest.mark.parametrize("D", [64, 128])
def test_a_windowed_sinked_row_does_not_depend_on_the_launch_around_it(dev, D, kv_type):
    """consequence 5: the base invariances, for a call with a window across two chunks, sinks and a cap"""
    n_kv, n_head, n_head_kv = 379, 8, 1
    sinks = X.sinks_of(n_head)
    for n_q in (3, 9):
        shape = (D, n_head, n_head_kv, kv_type, n_q, n_kv)
        v = (200, X.SOFTCAP, sinks)
        base = run(dev, shape, v)
        assert np.array_equal(bits(base), bits(run(dev, shape, v, layout=1, pad=8))), (n_q, "strides")
        assert np.array_equal(bits(base), bits(run(dev, shape, v, n_kv_max=n_kv + 700))), (n_q, "n_kv_max")
        assert np.array_equal(bits(base), bits(run(dev, shape, v, n_kv_max=n_kv + 700, device_n_kv=True))), (n_q, "d_n_kv")
        if n_q <= A.DECODE_MAX_Q:
            for t in range(n_q):                                     # the row alone sees the same positions with n_kv - (n_q - 1 - t) in the cache
                alone = run(dev, shape, v, rows=slice(t, t + 1), n_kv=n_kv - (n_q - 1 - t), n_kv_max=n_kv)
                assert np.array_equal(bits(base[t:t + 1]), bits(alone)), ("n_q", t)
    v = (200, 0.0, X.sinks_of(4))                                    # n_head: the first kv group alone, with its two sinks
    for n_q in (3, 9):
        shape = (D, 4, 2, kv_type, n_q, n_kv)
        assert np.array_equal(bits(run(dev, shape, v)[:, :2]), bits(run(dev, shape, v, heads=slice(0, 2)))), (n_q, "n_head")


# ---- paged ----
LENGTHS = (379, 0, 129, 1)
TABLE = ((11, 8, 5), (), (10, 7), (9,))
FREE_PAGE = 0                                                        # a page of the pool no sequence holds: 0xFF bytes


def paged(dev, cfg, n_q, variant, table=TABLE, garbage=P.GARBAGE, lens=LENGTHS, n_kv_max=None, len_bias=0):
    """one paged _ex call over the sequences of LENGTHS (the sweep's rows for those n_kv) -> numpy [n_seq, n_q, n_head, D]"""
    torch = dev.torch
    kv_type, D, n_head, n_head_kv, layout = cfg
    window, softcap, sinks = variant
    pool = P.Pool(kv_type, D, n_head_kv, layout)
    qs = []
    for n, pages in zip(LENGTHS, TABLE):                              # (the rows always lie where TABLE says; `table` is what the call is told)
        shape = (D, n_head, n_head_kv, kv_type, n_q, max(n, 1))
        qs.append(X.inputs(shape)[0])
        if n:
            pool.put(0, pages, X.inputs(shape)[1], n)
            pool.put(1, pages, X.inputs(shape)[2], n)
    n_kv_max = max(max(LENGTHS), 1) if n_kv_max is None else n_kv_max
    pc = pool.cache(dev, table, [n - len_bias for n in lens], n_kv_max, None, garbage)
    q = torch.from_numpy(np.concatenate(qs)).cuda()
    d_s = None if sinks is None else torch.from_numpy(sinks).cuda()
    out = dev.attn_paged(pc, q, n_head_kv, len_bias=len_bias, window=window, softcap=softcap, sinks=d_s)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(LENGTHS), n_q, n_head, D)


_CONTIG = {}


def contiguous_ex(dev, cfg, n, n_q, variant):
    kv_type, D, n_head, n_head_kv, _ = cfg
    key = (cfg[:4], n, n_q, X._vkey(variant))
    if key not in _CONTIG:
        _CONTIG[key] = np.zeros((n_q, n_head, D), np.float32) if n == 0 else run(dev, (D, n_head, n_head_kv, kv_type, n_q, n), variant)
    return _CONTIG[key]


def c_lo(n_kv, n_q, W):
    return X.window_lo(A.visible(0, n_kv, n_q, True), W) // PAGE


PAGED_SWEEP = [(t, D, nh, nhk, layout) for t in (F16, Q8_0) for D in (64, 128) for nh, nhk in X.HEADS for layout in (0, 1)]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", PAGED_SWEEP)
def test_every_paged_sequence_equals_the_contiguous_ex_entry_whatever_lies_below_the_window(dev, cfg):
    kv_type, D, n_head, n_head_kv, _ = cfg
    sinks = X.sinks_of(n_head)
    for n_q in (1, 3, 9, 130):
        rc, p = _plan_paged_ex(kv_type, D, n_head, n_head_kv, len(LENGTHS), n_q, max(LENGTHS), _opts(window=100))
        assert rc == 0 and p.form == (DECODE if n_q <= A.DECODE_MAX_Q else PROMPT)
        for v in ((100, X.SOFTCAP, sinks), (0, 0.0, sinks), (200, 0.0, None)):
            want = [contiguous_ex(dev, cfg, n, n_q, v) for n in LENGTHS]
            got = paged(dev, cfg, n_q, v)
            for b, n in enumerate(LENGTHS):
                assert np.array_equal(bits(got[b]), bits(want[b])), (cfg, n_q, v[0], b, n)
            if v[0] == 0:
                continue
            lo = c_lo(379, n_q, v[0])                                # the first sequence's first needed chunk: 2, 2, 2, 1 at W = 100
            if lo == 0:
                continue
            # the table entries below c_lo hold anything: invalid ids (the id check stands before the address: a wrong scan gives zeros), a page of 0xFF
            for junk in (-1, P.N_PAGES, 1 << 30, FREE_PAGE):
                row = tuple(junk if c < lo else pg for c, pg in enumerate(TABLE[0]))
                got = paged(dev, cfg, n_q, v, table=(row,) + TABLE[1:])
                for b, n in enumerate(LENGTHS):
                    assert np.array_equal(bits(got[b]), bits(want[b])), (cfg, n_q, v[0], "below the window", junk, b)
            # an invalid id INSIDE the window still zeroes that sequence, and that one only
            for where in range(lo, 3):
                row = list(TABLE[0])
                row[where] = P.N_PAGES
                got = paged(dev, cfg, n_q, v, table=(tuple(row),) + TABLE[1:])
                assert np.array_equal(bits(got[0]), np.zeros_like(bits(got[0]))), (cfg, n_q, v[0], "inside the window", where)
                for b in (1, 2, 3):
                    assert np.array_equal(bits(got[b]), bits(want[b])), (cfg, n_q, v[0], "inside the window", where, b)
        assert c_lo(379, 1, 100) == 2 and c_lo(379, 130, 100) == 1


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_paged_windowed_sequence_does_not_depend_on_the_call_around_it(dev, kv_type):
    cfg = (kv_type, 128, 8, 1, 0)
    v = (100, X.SOFTCAP, X.sinks_of(8))
    for n_q in (3, 9):
        base = paged(dev, cfg, n_q, v)
        assert np.array_equal(bits(base), bits(paged(dev, cfg, n_q, v, n_kv_max=379 + 700))), (n_q, "n_kv_max")
        assert np.array_equal(bits(base), bits(paged(dev, cfg, n_q, v, len_bias=5))), (n_q, "len_bias against a shifted d_len")
        assert np.array_equal(bits(base), bits(paged(dev, (kv_type, 128, 8, 1, 1), n_q, v))), (n_q, "the order of nb_pos and nb_head")
        assert np.array_equal(bits(base), bits(paged(dev, cfg, n_q, v, garbage=1 << 30))), (n_q, "the unneeded entries")


# ---- captured steps ----
def _capture(torch, fn):
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            fn()
    torch.cuda.current_stream().wait_stream(s)
    return g


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_captured_windowed_decode_step_follows_c_lo_between_replays(dev, kv_type):
    """rope(q) -> rope_kv_store(k) -> kv_store(v) -> windowed attention with sinks, n_kv and the position on the device, W = 130, captured ONCE; replayed
    at n_kv = 200, 258, 386, which carry c_lo = (n_kv - 130) // 128 from 0 to 1 to 2; every replay equals an uncaptured call bit for bit"""
    torch = dev.torch
    D, n_head, n_head_kv, n_max, W = 128, 8, 2, 4 * PAGE, 130
    rp = dev.rope_params(D, mode=2)
    rb = A.row_bytes(kv_type, D)
    nb_head, nb_pos = rb, n_head_kv * rb
    rng = np.random.default_rng(41)
    hist = rng.uniform(-1, 1, (2, n_max, n_head_kv, D)).astype(np.float32)
    mk = lambda side: torch.from_numpy(A.encode_rows(kv_type, hist[side]).reshape(-1)).cuda()
    kc, vc, fk, fv = mk(0), mk(1), mk(0), mk(1)
    sinks = torch.from_numpy(X.sinks_of(n_head) - 2.0).cuda()       # 0 .. 1: about the scores of these inputs
    q = torch.zeros((1, n_head, D), device="cuda")
    k_new = torch.zeros((1, n_head_kv, D), device="cuda")
    v_new = torch.zeros((1, n_head_kv, D), device="cuda")
    q_rot, out = torch.zeros_like(q), torch.zeros_like(q)
    work = torch.empty(dev.attn_work_size(kv_type, D, n_head, n_head_kv, 1, n_max), dtype=torch.uint8, device="cuda")
    d_pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")

    def step(k, v, o, on_device, pos=0):
        dp, dn = (d_pos, d_n) if on_device else (None, None)
        dev.rope(rp, q, pos0=pos, d_pos0=dp, out=q_rot)
        dev.rope_kv_store(rp, kv_type, k_new, k, nb_pos, nb_head, n_max, pos0=pos, d_pos0=dp)
        dev.kv_store(kv_type, v_new.reshape(1, n_head_kv * D), v, nb_pos, n_max, pos0=pos, d_pos0=dp)
        dev.attention(kv_type, q_rot, k, v, nb_pos, nb_head, n_head_kv, 0 if on_device else pos + 1, d_n_kv=dn, n_kv_max=n_max, out=o, work=work, window=W,
                      sinks=sinks)

    d_pos.fill_(199)
    d_n.fill_(200)
    step(kc.clone(), vc.clone(), torch.zeros_like(out), True)        # (a first call outside the capture, on copies: one-time kernel attributes)
    g = _capture(torch, lambda: step(kc, vc, out, True))
    seen = []
    for n_kv in (200, 258, 386):
        for t in (q, k_new, v_new):
            t.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(t.shape)).astype(np.float32)))
        d_pos.fill_(n_kv - 1)
        d_n.fill_(n_kv)
        g.replay()
        torch.cuda.synchronize()
        got = out.clone()
        fresh = torch.zeros_like(out)
        step(fk, fv, fresh, False, pos=n_kv - 1)
        torch.cuda.synchronize()
        assert torch.equal(got, fresh) and torch.equal(kc, fk) and torch.equal(vc, fv), (kv_type, n_kv)
        assert bool(torch.isfinite(got).all()) and float(got.abs().max()) > 0
        seen.append(c_lo(n_kv, 1, W))
    assert seen == [0, 1, 2]
    rc, p = _plan_ex(kv_type, D, n_head, n_head_kv, 1, n_max, _opts(window=W))
    assert rc == 0 and p.n_chunks == 3 and p.n_chunks < (n_max + PAGE - 1) // PAGE    # the captured grid is the window's, not n_kv_max's


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_captured_paged_windowed_step_crosses_a_page_boundary_and_frees_the_pages_behind(dev, kv_type):
    """the paged twin: rope(q, d_pos = d_len) -> rope_kv_store_paged(k) -> kv_store_paged(v) -> attn_paged(len_bias = 1, W = 130, sinks), captured ONCE
    for three sequences and replayed three times with d_len + 1 in between.  One sequence steps 256 -> 257 -> 258 positions onto its next page and its
    c_lo goes 0 -> 0 -> 1: from then on its first table entry is overwritten with an invalid id, as a host that recycled the page would.  Every replay
    equals the uncaptured contiguous _ex calls of each sequence bit for bit."""
    torch = dev.torch
    D, n_head, n_head_kv, n_seq, n_max, W = 128, 8, 2, 3, 4 * PAGE, 130
    start = (255, 5, 400)                                            # n_kv after the store: 256, 257, 258 / 6 .. 8 / 401 .. 403 (c_lo 2)
    table = ((4, 2, 3, P.GARBAGE), (7, P.GARBAGE, P.GARBAGE, P.GARBAGE), (-1, 1 << 30, 6, 10))      # the third sequence's first two pages are gone already
    rp = dev.rope_params(D, mode=2)
    rb = A.row_bytes(kv_type, D)
    rng = np.random.default_rng(43)
    hist = [rng.uniform(-1, 1, (2, n, n_head_kv, D)).astype(np.float32) for n in start]
    pool = P.Pool(kv_type, D, n_head_kv, 0)
    for h, n, pages in zip(hist, start, table):
        pool.put(0, pages, A.encode_rows(kv_type, h[0]), n)
        pool.put(1, pages, A.encode_rows(kv_type, h[1]), n)
    pc = pool.cache(dev, table, start, n_max)
    warm = pool.cache(dev, table, start, n_max)
    c_nb_head, c_nb_pos = rb, n_head_kv * rb
    fresh_kv = []
    for h, n in zip(hist, start):
        bufs = []
        for side in (0, 1):
            buf = torch.full((n_max * c_nb_pos,), 0xFF, dtype=torch.uint8, device="cuda")
            buf[:n * c_nb_pos] = torch.from_numpy(A.encode_rows(kv_type, h[side]).reshape(-1)).cuda()
            bufs.append(buf)
        fresh_kv.append(bufs)
    sinks = torch.from_numpy(X.sinks_of(n_head) - 2.0).cuda()
    q = torch.zeros((n_seq, n_head, D), device="cuda")
    k_new = torch.zeros((n_seq, n_head_kv, D), device="cuda")
    v_new = torch.zeros((n_seq, n_head_kv, D), device="cuda")
    q_rot, out = torch.zeros_like(q), torch.zeros_like(q)
    work = torch.empty(dev.attn_paged_work_size(kv_type, D, n_head, n_head_kv, n_seq, 1, n_max), dtype=torch.uint8, device="cuda")

    def step(cache, o):
        dev.rope(rp, q, pos=cache.d_len, out=q_rot)
        dev.rope_kv_store_paged(rp, cache, k_new, cache.k)
        dev.kv_store_paged(cache, v_new, cache.v)
        dev.attn_paged(cache, q_rot, n_head_kv, len_bias=1, out=o, work=work, window=W, sinks=sinks)

    step(warm, torch.zeros_like(out))
    g = _capture(torch, lambda: step(pc, out))
    for i in range(3):
        for t in (q, k_new, v_new):
            t.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(t.shape)).astype(np.float32)))
        if c_lo(start[0] + i + 1, 1, W) == 1:
            pc.pages[0, 0] = -1                                      # the page slid out of the window: the host recycled it
        g.replay()
        torch.cuda.synchronize()
        for b in range(n_seq):
            pos = start[b] + i
            kc, vc = fresh_kv[b]
            qb = dev.rope(rp, q[b:b + 1], pos0=pos)
            dev.rope_kv_store(rp, kv_type, k_new[b:b + 1], kc, c_nb_pos, c_nb_head, n_max, pos0=pos)
            dev.kv_store(kv_type, v_new[b:b + 1].reshape(1, n_head_kv * D), vc, c_nb_pos, n_max, pos0=pos)
            fresh = dev.attention(kv_type, qb, kc, vc, c_nb_pos, c_nb_head, n_head_kv, pos + 1, n_kv_max=n_max, window=W, sinks=sinks)
            torch.cuda.synchronize()
            assert torch.equal(out[b:b + 1], fresh), (kv_type, i, b)
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
        pc.d_len.add_(1)
    torch.cuda.synchronize()
    assert [c_lo(start[0] + i + 1, 1, W) for i in range(3)] == [0, 0, 1] and int(pc.pages[0, 0]) == -1
