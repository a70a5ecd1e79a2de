"""Attention with a mask tensor and ALiBi slopes over the contiguous, the paged and the ragged KV cache (include/ggml_hip_ext.h, ATTENTION WITH A
MASK TENSOR AND ALiBi SLOPES: ggml_hip_alibi_slopes, ggml_hip_attn_bias_dev, ggml_hip_attn_paged_bias_dev, ggml_hip_attn_paged_ragged_bias_dev;
csrc/attn.hip, attn.cpp).

Yardsticks (tests/np_attention_bias.py): the float64 attention over the DEQUANTIZED cache under the mask, never the library; the statistic
max |dst - ref| / max |V|; the bar per form is 4 x what the numpy model of the header's arithmetic measures on this sweep, or np_attention_ex's bar
where that is larger (TOL_DECODE_BIAS, TOL_PROMPT_BIAS; recomputed on the CPU here).  The sweep's inputs are peaked so that every mask that can act
moves dst by at least 100 x its bar (checked on the CPU): a kernel that ignores the mask cannot pass.  The header's CONSEQUENCES are held to bits.
Shapes: chunk = 128; n_kv in {1, 129, 379}; n_q 1, 3 (DECODE), 9, 140 (PROMPT: the smallest, and two query tiles); D 64 / 128; heads (4, 2), (8, 1);
both cache types; both layouts; caches, pools and the mask's slack pre-filled with 0xFF bytes (NaNs in every format)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_attention as A
import np_attention_bias as B
import test_attention as T                                           # Cache: the padded 0xFF-filled device cache of the base tests
import test_attention_paged as P                                     # Pool, _geometry: the 0xFF-filled page pool of the paged tests
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, Q8_0 = A.F16, A.Q8_0
NEW_SYMBOLS = ("ggml_hip_alibi_slopes", "ggml_hip_attn_bias_dev", "ggml_hip_attn_paged_bias_dev", "ggml_hip_attn_paged_ragged_bias_dev")
PAGE = A.CHUNK
NINF = B.NINF


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _last_error():
    return _lib.lib().ggml_hip_last_error().decode(errors="replace")


def _opts(window=0, softcap=0.0, sinks=None, reserved=0):
    return _lib.ggml_hip_attn_opts_t(sinks, window, softcap, reserved)


def _bias(mask=None, ld=0, slopes=None):
    return _lib.ggml_hip_attn_bias_t(mask, ld, slopes)


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def _tol(form):
    return B.TOL_DECODE_BIAS if form == "decode" else B.TOL_PROMPT_BIAS


def _call_kw(kw):
    """a variant's keywords as reference / model take them: (causal, the rest)"""
    kw = dict(kw)
    return kw.pop("causal"), kw


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    exports = open(os.path.join(ROOT, "ggmlsharp_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ggml_hip_\*;", exports)            # the export list is the ggml_hip_ prefix
    assert re.search(r"typedef struct ggml_hip_attn_bias_t\s*\{", hdr) and re.search(r"struct ggml_hip_attn_bias_t\b", cs)
    assert C.sizeof(_lib.ggml_hip_attn_bias_t) == 24
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name
    for name in ("ggml_hip_attn_bias_plan", "ggml_hip_attn_bias_work_size", "ggml_hip_attn_paged_bias_work_size"):      # the existing plans and sizes serve
        assert not hasattr(L, name), name


def _ulps(a, b):
    a, b = np.asarray(a, np.float32).view(np.int32).astype(np.int64), np.asarray(b, np.float32).view(np.int32).astype(np.int64)
    return int(np.abs(a - b).max())


def test_the_alibi_slopes_are_upstreams_rule():
    L = _lib.lib()
    for n_head in (1, 8, 12, 16, 40):
        for max_bias in (0.0, 8.0):
            got = np.full(n_head + 1, -3.0, np.float32)
            assert L.ggml_hip_alibi_slopes(n_head, max_bias, got.ctypes.data_as(C.c_void_p)) == 0
            want = B.alibi_slopes(n_head, max_bias)
            assert got[n_head] == -3.0                               # (nothing behind the vector is written)
            if max_bias == 0:
                assert np.array_equal(bits(got[:n_head]), bits(np.ones(n_head, np.float32)))
            else:
                assert _ulps(got[:n_head], want) <= 4, (n_head, got[:n_head], want)       # (two different powf: a few ulp)
                assert (np.diff(got[:min(n_head, 1 << int(np.log2(n_head)))]) < 0).all() and 0 < got[:n_head].min() and got[:n_head].max() < 1
    # the exact powers of two of the textbook cases: 8 heads, max_bias 8 -> 2^-1 .. 2^-8
    got = np.zeros(8, np.float32)
    assert L.ggml_hip_alibi_slopes(8, 8.0, got.ctypes.data_as(C.c_void_p)) == 0
    assert _ulps(got, 2.0 ** -np.arange(1, 9)) <= 4
    E = _lib
    assert L.ggml_hip_alibi_slopes(0, 8.0, got.ctypes.data_as(C.c_void_p)) == E.ERR_ARG and L.ggml_hip_alibi_slopes(8, 8.0, None) == E.ERR_ARG
    assert L.ggml_hip_alibi_slopes(8, -1.0, got.ctypes.data_as(C.c_void_p)) == E.ERR_ARG
    assert L.ggml_hip_alibi_slopes(8, float("nan"), got.ctypes.data_as(C.c_void_p)) == E.ERR_ARG


def _attn_rc(bias, opts=None, causal=1, n_q=1, work_bytes=1 << 30, ptr=0x1000, n_kv_max=16):
    o = None if opts is None else C.byref(opts)
    b = None if bias is None else C.byref(bias)
    return _lib.lib().ggml_hip_attn_bias_dev(F16, _p(ptr), 512, 128, _p(ptr), _p(ptr), 512, 256, 4, 2, 128, n_q, 16, None, n_kv_max, causal, 0.125, o, b, _p(ptr),
                                             512, 128, _p(0x1000), work_bytes, None)


def _paged_rc(bias, opts=None, causal=1, n_q=1, work_bytes=1 << 30, ptr=0x1000, n_kv_max=16):
    o = None if opts is None else C.byref(opts)
    b = None if bias is None else C.byref(bias)
    nb = P._geometry(F16, 128, 2, 0)
    return _lib.lib().ggml_hip_attn_paged_bias_dev(F16, _p(ptr), 512, 128, _p(ptr), _p(ptr), nb[0], nb[1], nb[2], 4, _p(0x1000), 2, _p(0x1000), 1, 2, 4, 2, 128, n_q,
                                                   n_kv_max, causal, 0.125, o, b, _p(ptr), 512, 128, _p(0x1000), work_bytes, None)


def _ragged_rc(bias, opts=None, causal=1, n_q=1, work_bytes=1 << 30, ptr=0x1000, n_kv_max=16):
    o = None if opts is None else C.byref(opts)
    b = None if bias is None else C.byref(bias)
    nb = P._geometry(F16, 128, 2, 0)
    n_tokens_max = 16 if n_q else 0                                  # (n_q = 0: the empty batch)
    return _lib.lib().ggml_hip_attn_paged_ragged_bias_dev(F16, _p(ptr), 512, 128, _p(ptr), _p(ptr), nb[0], nb[1], nb[2], 4, _p(0x1000), 2, _p(0x1000), 1, 0, 2,
                                                          _p(0x1000), n_tokens_max, n_tokens_max, 4, 2, 128, n_kv_max, causal, 0.125, o, b, _p(ptr), 512, 128,
                                                          _p(0x1000), work_bytes, None)


def test_every_new_refusal_is_decided_before_anything_is_launched():
    """every call below carries pointers that are not device memory: a launch would fault, a refusal returns its code"""
    E = _lib
    for rc_of in (_attn_rc, _paged_rc, _ragged_rc):
        name = rc_of.__name__
        # the mask's shape: ld_mask below n_kv_max, not a multiple of 8, a base that is not 16-byte aligned
        assert rc_of(_bias(0x1000, 8), n_kv_max=16) == E.ERR_SHAPE and "ld_mask" in _last_error(), name
        assert rc_of(_bias(0x1000, 20)) == E.ERR_SHAPE and rc_of(_bias(0x1000, 0)) == E.ERR_SHAPE and rc_of(_bias(0x1000, -16)) == E.ERR_SHAPE, name
        assert rc_of(_bias(0x1008, 16)) == E.ERR_SHAPE and rc_of(_bias(0x1002, 16, 0x1000)) == E.ERR_SHAPE, name
        # the slopes: misaligned, or without a mask
        assert rc_of(_bias(0x1000, 16, 0x1002)) == E.ERR_ARG and rc_of(_bias(None, 16, 0x1002)) == E.ERR_ARG, name
        assert rc_of(_bias(None, 16, 0x1000)) == E.ERR_ARG and "nothing to multiply" in _last_error(), name
        # the options' refusals stand in front, the base entry's rules behind
        for o in (_opts(window=-1), _opts(softcap=-1.0), _opts(sinks=0x1002), _opts(reserved=1)):
            assert rc_of(_bias(0x1000, 16), opts=o) == E.ERR_ARG, name
        assert rc_of(_bias(0x1000, 16), opts=_opts(window=1), causal=0) == E.ERR_ARG, name
        for b in (None, _bias(), _bias(None, 3), _bias(0x1000, 16), _bias(0x1000, 24, 0x1000)):
            for o in (None, _opts(), _opts(window=5, softcap=0.5, sinks=0x1000)):
                assert rc_of(b, opts=o, ptr=0x1004) == E.ERR_SHAPE, name
                assert rc_of(b, opts=o, work_bytes=64) == E.ERR_ARG, name
                assert rc_of(b, opts=o, n_q=0) == 0, name
    # the work size the entries ask for IS the base entry's: one byte less than it is refused, by the base function's name
    L = _lib.lib()
    need = L.ggml_hip_attn_work_size(F16, 128, 4, 2, 1, 16)
    assert need > 0 and _attn_rc(_bias(0x1000, 16), work_bytes=need - 1) == E.ERR_ARG and "ggml_hip_attn_work_size" in _last_error()
    need = L.ggml_hip_attn_paged_work_size(F16, 128, 4, 2, 2, 1, 16)
    assert need > 0 and _paged_rc(_bias(0x1000, 16), work_bytes=need - 1) == E.ERR_ARG and "ggml_hip_attn_paged_work_size" in _last_error()
    need = L.ggml_hip_attn_paged_ragged_work_size(F16, 128, 4, 2, 2, 16, 16, 16)
    assert need > 0 and _ragged_rc(_bias(0x1000, 16), work_bytes=need - 1) == E.ERR_ARG and "ggml_hip_attn_paged_ragged_work_size" in _last_error()


def test_the_numpy_model_without_a_mask_is_np_attention_ex_and_a_zero_mask_changes_nothing():
    for form, model in (("decode", B.model_decode), ("prompt", B.model_prompt)):
        for shape in [s for s in B.shapes(form) if s[:4] in ((64, 4, 2, Q8_0), (128, 8, 1, F16))]:
            D, n_head, _, _, n_q, n_kv = shape
            q, _, _, Kd, Vd = B.inputs(shape)
            sc = 1.0 / np.sqrt(D)
            zero = np.zeros((n_q, n_kv), np.float16)
            for kw in (dict(), dict(window=B.WINDOW, softcap=B.SOFTCAP, sinks=B.sinks_of(n_head))):
                off = model(q, Kd, Vd, n_kv, True, sc, **kw)
                assert np.array_equal(bits(off), bits(model(q, Kd, Vd, n_kv, True, sc, mask=zero, **kw))), (shape, sorted(kw))
                assert np.array_equal(bits(off), bits(model(q, Kd, Vd, n_kv, True, sc, mask=zero, slopes=np.ones(n_head, np.float32), **kw))), shape
                assert np.allclose(B.reference(q, Kd, Vd, n_kv, True, sc, mask=zero, **kw), B.reference(q, Kd, Vd, n_kv, True, sc, **kw), rtol=1e-14, atol=0)
            # the causal pattern written into the mask IS causal attention
            assert np.array_equal(bits(model(q, Kd, Vd, n_kv, False, sc, mask=B.causal_mask(n_q, n_kv))), bits(model(q, Kd, Vd, n_kv, True, sc))), shape


_MODEL = {}


def _model_sweep(form):
    """(the model's worst statistic, the smallest distance of an acting case from its unmasked reference, that case, the acting cases) on the sweep, once"""
    if form not in _MODEL:
        fn = B.model_decode if form == "decode" else B.model_prompt
        worst, least, who, acting = 0.0, np.inf, None, 0
        for shape in B.shapes(form):
            q, _, _, Kd, Vd = B.inputs(shape)
            for name in B.VARIANTS:
                causal, kw = _call_kw(B.variant(shape, name))
                ref = B.case_reference(shape, name)
                worst = max(worst, A.statistic(fn(q, Kd, Vd, shape[5], causal, 1.0 / np.sqrt(shape[0]), **kw), ref, Vd))
                if B.can_act(shape, B.variant(shape, name)):
                    acting += 1
                    d = A.statistic(B.unmasked_reference(shape, name), ref, Vd)
                    if d < least:
                        least, who = d, (shape, name)
        _MODEL[form] = (worst, least, who, acting)
    return _MODEL[form]


@pytest.mark.parametrize("form", ["decode", "prompt"])
def test_the_bias_model_constants_are_what_the_model_measures(form):
    rec = B.MODEL_WORST_DECODE_BIAS if form == "decode" else B.MODEL_WORST_PROMPT_BIAS
    worst = _model_sweep(form)[0]
    print(form, "model worst", worst, "recorded", rec)
    assert rec / 1.25 <= worst <= rec, (form, worst, rec)
    ex_tol = B.X.TOL_DECODE_EX if form == "decode" else B.X.TOL_PROMPT_EX
    assert _tol(form) == max(4 * rec, ex_tol)


@pytest.mark.parametrize("form", ["decode", "prompt"])
def test_every_mask_case_differs_from_the_unmasked_reference(form):
    """a condition on the INPUTS: wherever the mask can act at all, the masked f64 reference is at least 100 bars away from the unmasked one"""
    _, least, who, acting = _model_sweep(form)
    print(form, "smallest distance", least, "at", who, "100 bars", 100 * _tol(form))
    assert least >= 100 * _tol(form), (form, least, who)
    assert acting >= 0.8 * len(B.shapes(form)) * len(B.VARIANTS)      # (the rest: n_kv = 1 under a finite mask, chunk [128, 256) of a shorter cache)


TREE_PARENTS = (-1, 0, 0, 1, 2)
TREE_COMMITTED = PAGE + 1


def tree_mask():
    """draft i sits at position 129 + i and sees the committed cache and its own ancestors among the drafts (itself included)"""
    n = len(TREE_PARENTS)
    m = np.zeros((n, TREE_COMMITTED + n), np.float16)
    anc = []
    for i in range(n):
        a, k = [], i
        while k >= 0:
            a.append(k)
            k = TREE_PARENTS[k]
        anc.append(sorted(a))
        m[i, TREE_COMMITTED:] = NINF
        m[i, [TREE_COMMITTED + k for k in a]] = 0
    return m, anc


def tree_reference(shape):
    """per draft row: float64 causal attention of that row alone over a cache that holds only the committed positions and the row's ancestors"""
    D, n_head, _, _, n_q, n_kv = shape
    q, _, _, Kd, Vd = B.inputs(shape)
    _, anc = tree_mask()
    out = np.zeros((n_q, n_head, D), np.float64)
    for i in range(n_q):
        keep = list(range(TREE_COMMITTED)) + [TREE_COMMITTED + k for k in anc[i]]
        out[i] = A.reference(q[i:i + 1], Kd[keep], Vd[keep], len(keep), True, 1.0 / np.sqrt(D))[0]
    return out


def test_the_draft_tree_is_not_a_chain():
    """the tree's reference is the masked reference, and it lies far from plain causal attention over the five drafts as a chain"""
    assert tree_mask()[1] == [[0], [0, 1], [0, 2], [0, 1, 3], [0, 2, 4]]
    for shape in ((64, 4, 2, F16, 5, TREE_COMMITTED + 5), (128, 8, 1, Q8_0, 5, TREE_COMMITTED + 5)):
        q, _, _, Kd, Vd = B.inputs(shape)
        sc = 1.0 / np.sqrt(shape[0])
        want = tree_reference(shape)
        assert np.allclose(B.reference(q, Kd, Vd, shape[5], True, sc, mask=tree_mask()[0]), want, rtol=1e-12, atol=1e-15)
        assert A.statistic(A.reference(q, Kd, Vd, shape[5], True, sc), want, Vd) >= 100 * B.TOL_DECODE_BIAS


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
        _, Kraw, Vraw, _, _ = B.inputs(shape)
        if heads is not None:
            G = n_head // n_head_kv
            Kraw, Vraw = Kraw[:, heads.start // G:heads.stop // G], Vraw[:, heads.start // G:heads.stop // G]
        _CACHES[key] = T.Cache(dev, kv_type, D, Kraw.shape[1], n_kv + 700, layout, Kraw, Vraw)
    return _CACHES[key]


def dev_mask(dev, mask, ld=None):
    """a mask [rows, n] as a device f16 tensor [rows, ld] (ld: n rounded up to 8 by default), everything behind column n 0xFFFF -- a NaN"""
    rows, n = mask.shape
    ld = (n + 7) // 8 * 8 if ld is None else ld
    host = np.full((rows, ld), 0xFFFF, np.uint16)
    host[:, :n] = np.ascontiguousarray(mask, np.float16).view(np.uint16)
    return dev.torch.from_numpy(host.view(np.float16)).cuda()


TAIL = 256


def run(dev, shape, kw=None, layout=0, entry="bias", n_kv=None, n_kv_max=None, device_n_kv=False, pad=0, heads=None, ld=None, **more):
    """one contiguous call on a shape of the sweep -> numpy [n_q, n_head, D].  kw: causal / window / softcap / sinks / mask / slopes (a variant of
    np_attention_bias, or keywords given directly).  entry: "bias" ggml_hip_attn_bias_dev with a bias struct whatever it holds, "null" the same with
    bias = NULL, "ex" ggml_hip_attn_ex_dev (mask and slopes must be None).  The work buffer is followed by TAIL bytes that must stay as they were."""
    torch = dev.torch
    kw = dict(dict(causal=True, window=0, softcap=0.0, sinks=None, mask=None, slopes=None), **(kw or {}))
    kw.update(more)
    D, n_head, n_head_kv, kv_type, n_q, case_n_kv = shape
    q = B.inputs(shape)[0]
    n_kv = case_n_kv if n_kv is None else n_kv
    cache = _cache(dev, shape, layout, heads)
    sinks, slopes = kw["sinks"], kw["slopes"]
    if heads is not None:
        q = q[:, heads]
        sinks = None if sinks is None else sinks[heads]
        slopes = None if slopes is None else slopes[heads]
        n_head, n_head_kv = q.shape[1], cache.n_head_kv
    n_kv_max = n_kv if n_kv_max is None else n_kv_max
    qd = torch.zeros((n_q, n_head, D + pad), device="cuda")
    qd[:, :, :D] = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    out = torch.full((n_q, n_head, D + pad), -7.0, device="cuda")
    d_n = torch.tensor([n_kv], dtype=torch.int32, device="cuda") if device_n_kv else None
    d_s = None if sinks is None else torch.from_numpy(np.ascontiguousarray(sinks)).cuda()
    d_sl = None if slopes is None else torch.from_numpy(np.ascontiguousarray(slopes)).cuda()
    d_m = None if kw["mask"] is None else dev_mask(dev, kw["mask"], max((n_kv_max + 7) // 8 * 8, 8) if ld is None else ld)
    need = dev.attn_work_size(kv_type, D, n_head, n_head_kv, n_q, n_kv_max)
    work = torch.full((need + TAIL,), 0xA5, dtype=torch.uint8, device="cuda")
    o = _opts(kw["window"], kw["softcap"], None if d_s is None else d_s.data_ptr())
    args = [kv_type, _p(qd.data_ptr()), qd.stride(0), qd.stride(1), _p(cache.k.data_ptr()), _p(cache.v.data_ptr()), cache.nb_pos, cache.nb_head, n_head, n_head_kv,
            D, n_q, 0 if device_n_kv else n_kv, None if d_n is None else _p(d_n.data_ptr()), n_kv_max, int(kw["causal"]), 1.0 / float(np.sqrt(np.float64(D))), C.byref(o)]
    tail = [_p(out.data_ptr()), out.stride(0), out.stride(1), _p(work.data_ptr()), need, _p(torch.cuda.current_stream().cuda_stream)]
    if entry == "ex":
        assert d_m is None and d_sl is None
        rc = _lib.lib().ggml_hip_attn_ex_dev(*args, *tail)
    else:
        b = _bias(None if d_m is None else d_m.data_ptr(), 0 if d_m is None else d_m.stride(0), None if d_sl is None else d_sl.data_ptr())
        rc = _lib.lib().ggml_hip_attn_bias_dev(*args, None if entry == "null" else C.byref(b), *tail)
    assert rc == 0, _last_error()
    torch.cuda.synchronize()
    assert bool((work[need:] == 0xA5).all()), "the bytes behind the work buffer"
    if pad:
        assert bool((out[:, :, D:] == -7.0).all()), "the columns between the rows of dst"
    return out[:, :, :D].cpu().numpy()


SWEEP = [(D, nh, nhk, t) for D in (64, 128) for nh, nhk in B.HEADS for t in (F16, Q8_0)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["decode", "prompt"])
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_every_case_of_the_sweep_is_inside_four_times_the_model(dev, form, D, n_head, n_head_kv, kv_type):
    tol = _tol(form)
    i = 0
    for shape in (s for s in B.shapes(form) if s[:4] == (D, n_head, n_head_kv, kv_type)):
        Vd = B.inputs(shape)[4]
        for name in B.VARIANTS:
            kw = B.variant(shape, name)
            slack = i % 4 == 3                                       # every fourth case reads n_kv on the device, with 700 rows of 0xFF behind it
            got = run(dev, shape, kw, layout=i % 2, pad=4 * (i % 3), n_kv_max=shape[5] + 700 if slack else None, device_n_kv=slack)
            st = A.statistic(got, B.case_reference(shape, name), Vd)
            print(form, shape, name, "statistic", st, "bar", tol)
            assert np.isfinite(got).all() and st <= tol, (shape, name, st, tol)
            if name == "row":                                        # the hidden row is +0.0f, the others are the call without a mask
                t = shape[4] // 2
                assert np.array_equal(bits(got[t]), np.zeros_like(bits(got[t]))), (shape, "the hidden row")
                plain = run(dev, shape, entry="ex", layout=i % 2)
                keep = [r for r in range(shape[4]) if r != t]
                assert np.array_equal(bits(got[keep]), bits(plain[keep])), (shape, "the other rows")
            i += 1


@pytest.mark.gpu
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_no_bias_and_a_zero_mask_give_the_ex_entrys_bits(dev, D, n_head, n_head_kv, kv_type):
    """consequences 1 and 2: bias NULL / empty, a mask of +0.0, slopes NULL against slopes of 1.0f"""
    ones = np.ones(n_head, np.float32)
    for n_q in (1, 3, 9, 140):
        for n_kv in (1, 379):
            shape = (D, n_head, n_head_kv, kv_type, n_q, n_kv)
            zero = np.zeros((n_q, n_kv), np.float16)
            for opt in (dict(), dict(window=B.WINDOW, softcap=B.SOFTCAP, sinks=B.sinks_of(n_head))):
                for causal in (False, True) if not opt else (True,):
                    ex = run(dev, shape, entry="ex", causal=causal, **opt)
                    assert np.array_equal(bits(ex), bits(run(dev, shape, entry="null", causal=causal, **opt))), ("1: bias = NULL", shape, causal)
                    assert np.array_equal(bits(ex), bits(run(dev, shape, entry="bias", causal=causal, **opt))), ("1: both pointers NULL", shape, causal)
                    assert np.array_equal(bits(ex), bits(run(dev, shape, causal=causal, mask=zero, **opt))), ("2: a zero mask", shape, causal)
                    assert np.array_equal(bits(ex), bits(run(dev, shape, causal=causal, mask=zero, slopes=ones, **opt))), ("2: and slopes of 1", shape, causal)
            kw = B.variant(shape, "random")
            assert np.array_equal(bits(run(dev, shape, kw)), bits(run(dev, shape, kw, slopes=ones))), ("2: slopes NULL are slopes of 1", shape)


@pytest.mark.gpu
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_the_causal_pattern_in_the_mask_is_the_causal_flag(dev, D, n_head, n_head_kv, kv_type):
    """consequence 3, both forms: chunks above the diagonal are fully hidden for some rows (n_q = 3 over 129 positions: rows 0 and 1 see chunk 0 alone)"""
    for n_q, n_kv in ((1, 379), (3, 129), (3, 379), (9, 129), (140, 379), (140, 129)):
        shape = (D, n_head, n_head_kv, kv_type, n_q, n_kv)
        assert (B.inputs(shape)[4] != 0).all()                       # (V holds no zeros: the sign of a zero cannot decide)
        want = run(dev, shape, entry="ex", causal=True)
        got = run(dev, shape, causal=False, mask=B.causal_mask(n_q, n_kv))
        assert np.array_equal(bits(got), bits(want)), shape
        opt = dict(softcap=B.SOFTCAP, sinks=B.sinks_of(n_head))
        assert np.array_equal(bits(run(dev, shape, causal=False, mask=B.causal_mask(n_q, n_kv), **opt)), bits(run(dev, shape, entry="ex", causal=True, **opt))), shape


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
@pytest.mark.parametrize("D", [64, 128])
def test_a_masked_row_does_not_depend_on_the_launch_around_it(dev, D, kv_type):
    """consequence 4, the contiguous part: strides, n_kv_max, where n_kv comes from, ld_mask, and -- without slopes -- n_head"""
    n_kv = 379
    for n_q in (3, 9):
        shape = (D, 8, 1, kv_type, n_q, n_kv)
        for name in ("random+slopes", "random+options"):
            kw = B.variant(shape, name)
            base = run(dev, shape, kw)
            assert np.array_equal(bits(base), bits(run(dev, shape, kw, layout=1, pad=8))), (n_q, name, "strides")
            assert np.array_equal(bits(base), bits(run(dev, shape, kw, n_kv_max=n_kv + 700))), (n_q, name, "n_kv_max")
            assert np.array_equal(bits(base), bits(run(dev, shape, kw, n_kv_max=n_kv + 700, device_n_kv=True))), (n_q, name, "d_n_kv")
            assert np.array_equal(bits(base), bits(run(dev, shape, kw, ld=1536))), (n_q, name, "ld_mask")
        shape = (D, 4, 2, kv_type, n_q, n_kv)
        kw = B.variant(shape, "random")
        assert np.array_equal(bits(run(dev, shape, kw)[:, :2]), bits(run(dev, shape, kw, heads=slice(0, 2)))), (n_q, "n_head")
        kw = B.variant(shape, "alibi")                               # with slopes: the first kv group with its own two slopes
        assert np.array_equal(bits(run(dev, shape, kw)[:, :2]), bits(run(dev, shape, kw, heads=slice(0, 2)))), (n_q, "n_head, its slopes")


# ---- paged ----
LENGTHS = (379, 0, 129, 1)
TABLE = ((11, 8, 5), (), (10, 7), (9,))
OTHER_TABLE = ((2, 6, 1), (), (0, 3), (4,))


def _seq_shape(cfg, n_q, n):
    kv_type, D, n_head, n_head_kv, _ = cfg
    return (D, n_head, n_head_kv, kv_type, n_q, max(n, 1))


def paged(dev, cfg, n_q, name, table=TABLE, n_kv_max=None, ld=None, len_bias=0):
    """one paged bias call over the sequences of LENGTHS, each under ITS OWN variant `name` (its mask rows stacked) -> numpy [n_seq, n_q, n_head, D]"""
    torch = dev.torch
    kv_type, D, n_head, n_head_kv, layout = cfg
    pool = P.Pool(kv_type, D, n_head_kv, layout)
    n_kv_max = max(LENGTHS) if n_kv_max is None else n_kv_max
    ld = (n_kv_max + 7) // 8 * 8 if ld is None else ld
    qs, mask = [], np.full((len(LENGTHS) * n_q, ld), 0xFFFF, np.uint16).view(np.float16)
    kw = None
    for b, (n, pages) in enumerate(zip(LENGTHS, table)):
        shape = _seq_shape(cfg, n_q, n)
        qs.append(B.inputs(shape)[0])
        if n:
            pool.put(0, pages, B.inputs(shape)[1], n)
            pool.put(1, pages, B.inputs(shape)[2], n)
            kw = B.variant(shape, name)
            mask[b * n_q:(b + 1) * n_q, :n] = kw["mask"]
    pc = pool.cache(dev, table, [n - len_bias for n in LENGTHS], n_kv_max)
    q = torch.from_numpy(np.concatenate(qs)).cuda()
    d_s = None if kw["sinks"] is None else torch.from_numpy(kw["sinks"]).cuda()
    d_sl = None if kw["slopes"] is None else torch.from_numpy(kw["slopes"]).cuda()
    out = dev.attn_paged(pc, q, n_head_kv, len_bias=len_bias, causal=kw["causal"], window=kw["window"], softcap=kw["softcap"], sinks=d_s,
                         mask=torch.from_numpy(mask).cuda(), slopes=d_sl)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(LENGTHS), n_q, n_head, D)


PAGED_SWEEP = [(t, D, nh, nhk, (D // 64 + nh // 8 + t) % 2) for t in (F16, Q8_0) for D in (64, 128) for nh, nhk in B.HEADS]


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", PAGED_SWEEP)
def test_every_paged_sequence_equals_the_contiguous_bias_entry_and_is_inside_the_tolerance(dev, cfg):
    for n_q in (1, 3, 9, 140):
        form = "decode" if n_q <= A.DECODE_MAX_Q else "prompt"
        for name in B.VARIANTS:
            got = paged(dev, cfg, n_q, name)
            for b, n in enumerate(LENGTHS):
                if n == 0:
                    assert np.array_equal(bits(got[b]), np.zeros_like(bits(got[b]))), (cfg, n_q, name, "the empty sequence")
                    continue
                shape = _seq_shape(cfg, n_q, n)
                want = run(dev, shape, B.variant(shape, name))
                assert np.array_equal(bits(got[b]), bits(want)), (cfg, n_q, name, b, n)
                st = A.statistic(got[b], B.case_reference(shape, name), B.inputs(shape)[4])
                assert st <= _tol(form), (cfg, n_q, name, b, st)
        base = paged(dev, cfg, n_q, "random+slopes")
        assert np.array_equal(bits(base), bits(paged(dev, cfg, n_q, "random+slopes", table=OTHER_TABLE))), (cfg, n_q, "the page assignment")
        assert np.array_equal(bits(base), bits(paged(dev, cfg, n_q, "random+slopes", n_kv_max=379 + 700, ld=1280))), (cfg, n_q, "n_kv_max and ld_mask")
        assert np.array_equal(bits(base), bits(paged(dev, cfg, n_q, "random+slopes", len_bias=n_q))), (cfg, n_q, "len_bias against a shifted d_len")


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_an_invalid_needed_page_id_still_zeroes_its_sequence_alone_under_a_mask(dev, kv_type):
    cfg = (kv_type, 128, 8, 1, 0)
    for n_q in (3, 9):
        want = paged(dev, cfg, n_q, "random")
        bad = ((11, P.N_PAGES, 5),) + TABLE[1:]
        got = paged(dev, cfg, n_q, "random", table=bad)
        assert np.array_equal(bits(got[0]), np.zeros_like(bits(got[0]))), n_q
        assert np.array_equal(bits(got[1:]), bits(want[1:])), n_q


# ---- ragged, and the draft tree ----
def ragged(dev, cfg, seqs, n_tokens_max, n_kv_max=512):
    """one ragged bias call.  seqs: per sequence (shape or None for an idle slot, variant keywords or None, pages); the sequence's n_kv is its shape's,
    d_len = n_kv - n_q with add_q = 1.  Options and slopes are the first masked sequence's.  -> (dst [n_tokens_max, n_head, D] over a poisoned buffer, q_start)"""
    torch = dev.torch
    kv_type, D, n_head, n_head_kv, layout = cfg
    pool = P.Pool(kv_type, D, n_head_kv, layout)
    ld = (n_kv_max + 7) // 8 * 8
    q = np.full((n_tokens_max, n_head, D), 3.0, np.float32)
    mask = np.full((n_tokens_max, ld), 0xFFFF, np.uint16).view(np.float16)
    q_start, lens, table, opt = [0], [], [], None
    for shape, kw, pages in seqs:
        n_q, n_kv = (0, 0) if shape is None else (shape[4], shape[5])
        r0 = q_start[-1]
        q_start.append(r0 + n_q)
        lens.append(n_kv - n_q)
        table.append(pages)
        if shape is None:
            continue
        q[r0:r0 + n_q] = B.inputs(shape)[0]
        pool.put(0, pages, B.inputs(shape)[1], n_kv)
        pool.put(1, pages, B.inputs(shape)[2], n_kv)
        mask[r0:r0 + n_q, :n_kv] = np.zeros((n_q, n_kv), np.float16) if kw is None else kw["mask"]
        opt = kw if opt is None and kw is not None else opt
    pc = pool.cache(dev, table, lens, n_kv_max)
    d_s = None if opt["sinks"] is None else torch.from_numpy(opt["sinks"]).cuda()
    d_sl = None if opt["slopes"] is None else torch.from_numpy(opt["slopes"]).cuda()
    dst = torch.full((n_tokens_max, n_head, D), -777.25, device="cuda")
    dev.attn_paged_ragged(pc, torch.tensor(q_start, dtype=torch.int32, device="cuda"), torch.from_numpy(q).cuda(), n_head_kv, add_q=True, out=dst,
                          causal=opt["causal"], window=opt["window"], softcap=opt["softcap"], sinks=d_s, mask=torch.from_numpy(mask).cuda(), slopes=d_sl)
    torch.cuda.synchronize()
    return dst.cpu().numpy(), q_start


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", PAGED_SWEEP)
def test_every_ragged_sequence_equals_the_bias_entry_for_it_alone(dev, cfg):
    """consequence 4, the ragged part: a DECODE sequence, a PROMPT sequence of two tiles, an idle slot and a single row in one call, each under its own
    mask rows; a sequence's rows are the contiguous bias entry's (which the paged entry equals per sequence), rows of no sequence are not written"""
    kv_type, D, n_head, n_head_kv, _ = cfg
    for name in ("random+slopes", "random+options", "chunk0"):
        shapes = [(D, n_head, n_head_kv, kv_type, 3, 379), (D, n_head, n_head_kv, kv_type, 140, 379), None, (D, n_head, n_head_kv, kv_type, 1, 129)]
        seqs = [(s, None if s is None else B.variant(s, name), pages) for s, pages in zip(shapes, ((11, 8, 5), (2, 6, 1), (), (10, 7)))]
        got, q_start = ragged(dev, cfg, seqs, 150)
        for b, s in enumerate(shapes):
            if s is not None:
                want = run(dev, s, B.variant(s, name))
                assert np.array_equal(bits(got[q_start[b]:q_start[b + 1]]), bits(want)), (cfg, name, b)
        assert (got[q_start[-1]:] == np.float32(-777.25)).all(), (cfg, name, "rows of no sequence")


@pytest.mark.gpu
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_a_draft_tree_sees_the_committed_cache_and_its_ancestors(dev, D, n_head, n_head_kv, kv_type):
    shape = (D, n_head, n_head_kv, kv_type, 5, TREE_COMMITTED + 5)
    mask, _ = tree_mask()
    want = tree_reference(shape)
    Vd = B.inputs(shape)[4]
    got = run(dev, shape, mask=mask)
    st = A.statistic(got, want, Vd)
    print(shape, "tree statistic", st, "bar", B.TOL_DECODE_BIAS)
    assert st <= B.TOL_DECODE_BIAS, (shape, st)
    # the same through the ragged entry, beside a plain decoding sequence and an idle slot
    cfg = (kv_type, D, n_head, n_head_kv, 0)
    plain = (D, n_head, n_head_kv, kv_type, 1, 379)
    rows, q_start = ragged(dev, cfg, [(plain, None, (11, 8, 5)), (None, None, ()), (shape, dict(B.variant(shape, "row"), mask=mask), (3, 9))], 8)
    assert q_start == [0, 1, 1, 6]
    assert np.array_equal(bits(rows[1:6]), bits(got)), (shape, "the tree in a ragged batch")
    assert A.statistic(rows[1:6], want, Vd) <= B.TOL_DECODE_BIAS
    assert np.array_equal(bits(rows[:1]), bits(run(dev, plain, entry="ex"))), (shape, "the plain sequence beside it: a zero mask row")
    assert (rows[6:] == np.float32(-777.25)).all()


# ---- a captured step ----
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
def test_a_captured_masked_decode_step_follows_the_mask_between_replays(dev, kv_type):
    """rope(q) -> rope_kv_store(k) -> kv_store(v) -> attention under a mask with ALiBi slopes, n_kv and the position on the device, captured ONCE; replayed
    at n_kv = 127, 128, 129 (onto the second chunk) with the mask's contents rewritten in between; every replay equals an uncaptured call bit for bit"""
    torch = dev.torch
    D, n_head, n_head_kv, n_max = 128, 8, 2, 4 * PAGE
    rp = dev.rope_params(D, mode=2)
    rb = A.row_bytes(kv_type, D)
    nb_head, nb_pos = rb, n_head_kv * rb
    rng = np.random.default_rng(47)
    hist = rng.uniform(-1, 1, (2, n_max, n_head_kv, D)).astype(np.float32)
    mk = lambda side: torch.from_numpy(A.encode_rows(kv_type, hist[side]).reshape(-1)).cuda()
    kc, vc, fk, fv = mk(0), mk(1), mk(0), mk(1)
    slopes = torch.from_numpy(dev.alibi_slopes(n_head, 8.0)).cuda()
    mask = torch.zeros((1, n_max), dtype=torch.float16, device="cuda")
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
        dev.attention(kv_type, q_rot, k, v, nb_pos, nb_head, n_head_kv, 0 if on_device else pos + 1, d_n_kv=dn, n_kv_max=n_max, out=o, work=work, mask=mask,
                      slopes=slopes)

    d_pos.fill_(126)
    d_n.fill_(127)
    step(kc.clone(), vc.clone(), torch.zeros_like(out), True)        # (a first call outside the capture, on copies: one-time kernel attributes)
    g = _capture(torch, lambda: step(kc, vc, out, True))
    seen = []
    for n_kv in (127, 128, 129):
        for t in (q, k_new, v_new):
            t.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(t.shape)).astype(np.float32)))
        m = rng.uniform(-4, 0, (1, n_max)).astype(np.float16)
        m[rng.uniform(0, 1, (1, n_max)) < 0.3] = NINF
        if n_kv == 129:
            m[0, :PAGE] = NINF                                       # the whole first chunk hidden: the step lives on position 128 alone
            m[0, PAGE] = np.float16(-1.5)
        mask.copy_(torch.from_numpy(m))
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
        seen.append(got.cpu().numpy())
    assert not np.array_equal(seen[0], seen[1]) and not np.array_equal(seen[1], seen[2])
