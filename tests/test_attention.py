"""Attention over an F16 or Q8_0 KV cache on the device (include/ggml_hip_ext.h ggml_hip_kv_store_dev, ggml_hip_attn_dev, ggml_hip_attn_plan,
ggml_hip_attn_work_size; csrc/attn.hip, attn.cpp, plan.cpp plan_attn).

Yardsticks (tests/np_attention.py): the float64 attention over the DEQUANTIZED cache, never the library; the statistic of a case is
max |dst - ref| / max |V| and the bar per form is 4 x what the numpy model of the header's arithmetic measures on the same sweep
(TOL_DECODE, TOL_PROMPT).  kv_store is held to bits: the oracle's quantize_row_q8_0, numpy's astype(float16).
Exact cases: one visible position returns the V row the form works on bit for bit -- deq(V_0), and in the PROMPT form over a Q8_0 cache
f16(deq(V_0)), because that form dequantizes a row to f16 while staging it (the header says so); no visible position returns +0.0f.
V constant over the positions is NOT exact in either form (the header says why) and is held to the tolerance.
Shapes: chunk = 128 positions; n_kv in {1, 31, 128, 129, 379}; n_q 1 / 3 (DECODE), 9 and 379 (PROMPT: the smallest, and one that is no
multiple of the 128-row query tile and spans three chunks causally); heads (4, 4), (4, 2), (8, 1); both layouts of the cache."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_attention as A
import oracle_lib as O
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, Q8_0 = A.F16, A.Q8_0
NEW_SYMBOLS = ("ggml_hip_kv_store_dev", "ggml_hip_attn_dev", "ggml_hip_attn_plan", "ggml_hip_attn_work_size")
DECODE, PROMPT = 1, 2


def _p(x):
    return None if x is None else C.c_void_p(int(x))


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


def _plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max):
    out = _lib.ggml_hip_attn_plan_t()
    rc = _lib.lib().ggml_hip_attn_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, C.byref(out))
    return rc, out


def test_the_form_follows_n_q_alone_and_the_chunk_never_moves():
    for n_q in (1, 2, 3, 8, 9, 10, 127, 128, 129, 379, 4096):
        seen = set()
        for kv_type in (F16, Q8_0):
            for D in (64, 128):
                for n_head, n_head_kv in ((4, 4), (4, 2), (8, 1), (32, 8), (16, 1), (64, 8)):
                    for n_kv_max in (0, 1, 127, 128, 129, 5000, 1 << 20):
                        rc, p = _plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max)
                        assert rc == 0
                        seen.add((p.form, p.chunk))
                        assert p.n_chunks == (n_kv_max + p.chunk - 1) // p.chunk
                        assert p.launches == (2 if p.form == DECODE else 1)
        assert seen == {(DECODE if n_q <= A.DECODE_MAX_Q else PROMPT, A.CHUNK)}, (n_q, seen)


def test_the_work_size_is_monotone_and_zero_for_an_empty_batch():
    L = _lib.lib()
    for kv_type in (F16, Q8_0):
        for D in (64, 128):
            for n_q in (1, 3, 8):
                last = 0
                for n_kv_max in (1, 128, 129, 1000, 1001, 40000):
                    w = L.ggml_hip_attn_work_size(kv_type, D, 8, 2, n_q, n_kv_max)
                    assert w >= last and w > 0
                    last = w
            assert L.ggml_hip_attn_work_size(kv_type, D, 8, 2, 0, 4096) == 0
            assert L.ggml_hip_attn_work_size(kv_type, D, 8, 2, 64, 4096) == 0      # the PROMPT form keeps its state in registers


def _attn_rc(kv_type=F16, D=128, n_head=4, n_head_kv=2, n_q=1, n_kv=16, n_kv_max=16, ldq=(512, 128), ldd=(512, 128), nb=(512, 256), ptr=0x1000, mask=None,
             max_bias=0.0, softcap=0.0, sinks=None, work=0x1000, work_bytes=1 << 30, d_n_kv=None):
    return _lib.lib().ggml_hip_attn_dev(kv_type, _p(ptr), ldq[0], ldq[1], _p(ptr), _p(ptr), nb[0], nb[1], n_head, n_head_kv, D, n_q, n_kv, d_n_kv, n_kv_max, 1,
                                        0.125, mask, max_bias, softcap, sinks, _p(ptr), ldd[0], ldd[1], _p(work), work_bytes, None)


def test_what_is_not_served_is_refused_before_anything_is_launched():
    """every call below carries pointers that are not device memory: a launch would fault, a refusal returns its code"""
    E = _lib
    assert _attn_rc(D=96) == E.ERR_SHAPE and _attn_rc(D=256) == E.ERR_SHAPE
    assert _attn_rc(n_head=6, n_head_kv=4) == E.ERR_SHAPE                       # G not an integer
    assert _attn_rc(n_head=34, n_head_kv=2) == E.ERR_SHAPE                      # G = 17
    for t in (0, 2, 7, 9, _lib.BF16):
        assert _attn_rc(kv_type=t) == E.ERR_TYPE
    assert _attn_rc(ldq=(514, 128)) == E.ERR_SHAPE and _attn_rc(ldq=(512, 130)) == E.ERR_SHAPE and _attn_rc(ldd=(512, 126)) == E.ERR_SHAPE
    assert _attn_rc(nb=(520, 256)) == E.ERR_SHAPE and _attn_rc(nb=(512, 264)) == E.ERR_SHAPE and _attn_rc(nb=(512, 128)) == E.ERR_SHAPE
    assert _attn_rc(ptr=0x1004) == E.ERR_SHAPE
    assert _attn_rc(mask=_p(0x1000)) == E.ERR_ARG and _attn_rc(max_bias=8.0) == E.ERR_ARG and _attn_rc(softcap=30.0) == E.ERR_ARG
    assert _attn_rc(sinks=_p(0x1000)) == E.ERR_ARG
    assert _attn_rc(n_kv=17) == E.ERR_ARG and _attn_rc(n_kv=-1) == E.ERR_ARG
    assert _attn_rc(work=None) == E.ERR_ARG and _attn_rc(work_bytes=64) == E.ERR_ARG
    assert _attn_rc(n_q=0, work=None) == 0                                      # an empty batch: OK, nothing written
    rc, _ = _plan(F16, 96, 4, 4, 1, 16)
    assert rc == E.ERR_SHAPE
    rc, _ = _plan(Q8_0 + 1, 128, 4, 4, 1, 16)
    assert rc == E.ERR_TYPE
    L = _lib.lib()
    st = lambda **k: L.ggml_hip_kv_store_dev(k.get("t", F16), _p(k.get("src", 0x1000)), k.get("ld", 128), 1, k.get("n", 128), _p(k.get("c", 0x1000)),
                                             k.get("nb", 256), 8, 0, None, None)
    assert st(t=2) == E.ERR_TYPE and st(ld=130) == E.ERR_SHAPE and st(ld=64) == E.ERR_SHAPE and st(nb=250) == E.ERR_SHAPE and st(nb=128) == E.ERR_SHAPE
    assert st(t=Q8_0, n=48, ld=48) == E.ERR_SHAPE and st(src=0x1004) == E.ERR_SHAPE and st(c=0x1008) == E.ERR_SHAPE and st(src=None) == E.ERR_ARG


def test_the_q8_0_restatement_is_the_oracle():
    rng = np.random.default_rng(5)
    x = rng.uniform(-1, 1, (7, 128)).astype(np.float32)
    x[3, :32] = 0.0
    assert np.array_equal(A.quantize_q8_0(x), np.asarray(O.quantize_row(Q8_0, x)).reshape(7, -1))


def test_the_model_constants_are_what_the_model_measures():
    """the numpy model of each form against the f64 reference on the whole sweep: its worst statistic is the recorded constant (rounded up)"""
    for form, fn, rec in (("decode", A.model_decode, A.MODEL_WORST_DECODE), ("prompt", A.model_prompt, A.MODEL_WORST_PROMPT)):
        worst = 0.0
        for case in A.cases(form):
            q, _, _, Kd, Vd = A.inputs(case)
            worst = max(worst, A.statistic(fn(q, Kd, Vd, case[5], True, 1.0 / np.sqrt(case[0])), A.case_reference(case), Vd))
        print(form, "model worst", worst, "recorded", rec)
        assert rec / 1.25 <= worst <= rec, (form, worst, rec)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


def _up16(n):
    return (n + 15) // 16 * 16


class Cache:
    """K and V bytes [n_kv, n_head_kv, row_bytes] in a padded device buffer of 0xFF bytes (NaNs in both formats), room for n_alloc positions.
    layout 0: position-major (nb_head < nb_pos), 1: head-major (nb_head > nb_pos); padding between heads and between positions in both."""

    def __init__(self, dev, kv_type, D, n_head_kv, n_alloc, layout, Kraw=None, Vraw=None):
        torch = dev.torch
        rb = A.row_bytes(kv_type, D)
        if layout == 0:
            self.nb_head = _up16(rb) + 16
            self.nb_pos = n_head_kv * self.nb_head + 32
        else:
            self.nb_pos = _up16(rb) + 16
            self.nb_head = n_alloc * self.nb_pos + 48
        self.kv_type, self.D, self.n_head_kv, self.n_alloc, self.rb = kv_type, D, n_head_kv, n_alloc, rb
        self.size = max(n_alloc, 1) * self.nb_pos + n_head_kv * self.nb_head
        self.host = [np.full(self.size, 0xFF, np.uint8), np.full(self.size, 0xFF, np.uint8)]
        for buf, raw in zip(self.host, (Kraw, Vraw)):
            if raw is not None:
                for j in range(raw.shape[0]):
                    for hk in range(n_head_kv):
                        o = j * self.nb_pos + hk * self.nb_head
                        buf[o:o + rb] = raw[j, hk]
        self.k = torch.from_numpy(self.host[0]).cuda()
        self.v = torch.from_numpy(self.host[1]).cuda()


def _run(dev, case, layout=0, causal=True, n_kv_max=None, device_n_kv=False, pad=0, heads=None, rows=None, n_kv=None, cache=None, V=None):
    """the entry on a case of the sweep -> numpy [n_q, n_head, D].  pad: extra elements in the strides of q and dst; heads: run only these
    query heads (a slice, whole kv groups); rows: only these query rows as a batch of their own (n_kv is then the caller's)"""
    torch = dev.torch
    D, n_head, n_head_kv, kv_type, n_q, case_n_kv = case
    q, Kraw, Vraw, _, _ = A.inputs(case)
    n_kv = case_n_kv if n_kv is None else n_kv
    if V is not None:
        Vraw = V
    G = n_head // n_head_kv
    if heads is not None:
        q = q[:, heads]
        Kraw, Vraw = Kraw[:, heads.start // G:heads.stop // G], Vraw[:, heads.start // G:heads.stop // G]
        n_head, n_head_kv = q.shape[1], Kraw.shape[1]
    if rows is not None:
        q = q[rows]
        n_q = q.shape[0]
    n_kv_max = n_kv if n_kv_max is None else n_kv_max
    if cache is None:
        cache = Cache(dev, kv_type, D, n_head_kv, max(n_kv_max, Kraw.shape[0]), layout, Kraw, Vraw)
    qd = torch.zeros((n_q, n_head, D + pad), device="cuda")
    qd[:, :, :D] = torch.from_numpy(np.ascontiguousarray(q)).cuda()
    out = torch.full((n_q, n_head, D + pad), -7.0, device="cuda")
    d_n = torch.tensor([n_kv], dtype=torch.int32, device="cuda") if device_n_kv else None
    dev.attention(kv_type, qd[:, :, :D], cache.k, cache.v, cache.nb_pos, cache.nb_head, n_head_kv, 0 if device_n_kv else n_kv, d_n_kv=d_n, n_kv_max=n_kv_max,
                  causal=causal, out=out[:, :, :D])
    torch.cuda.synchronize()
    if pad:
        assert bool((out[:, :, D:] == -7.0).all())
    return out[:, :, :D].cpu().numpy()


SWEEP = [(D, nh, nhk, t) for D in (64, 128) for nh, nhk in A.HEADS for t in (F16, Q8_0)]


@pytest.mark.gpu
@pytest.mark.parametrize("form", ["decode", "prompt"])
@pytest.mark.parametrize("D,n_head,n_head_kv,kv_type", SWEEP)
def test_every_case_of_the_sweep_is_inside_four_times_the_model(dev, form, D, n_head, n_head_kv, kv_type):
    tol = A.TOL_DECODE if form == "decode" else A.TOL_PROMPT
    worst = 0.0
    for i, case in enumerate(c for c in A.cases(form) if c[:4] == (D, n_head, n_head_kv, kv_type)):
        rc, p = _plan(kv_type, D, n_head, n_head_kv, case[4], case[5])
        assert rc == 0 and p.form == (DECODE if form == "decode" else PROMPT)
        got = _run(dev, case, layout=i % 2, pad=4 * (i % 3))
        st = A.statistic(got, A.case_reference(case), A.inputs(case)[4])
        print(form, case, "statistic", st, "bar", tol)
        worst = max(worst, st)
        assert np.isfinite(got).all() and st <= tol, (case, st, tol)


def _staged(form, kv_type, Vd):
    """the V values a form works on: deq(V); the PROMPT form over a Q8_0 cache rounds them to f16 while staging"""
    return Vd.astype(np.float16).astype(np.float32) if (form == "prompt" and kv_type == Q8_0) else Vd


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
@pytest.mark.parametrize("D", [64, 128])
def test_exact_cases_one_visible_position_and_none(dev, D, kv_type):
    for n_head, n_head_kv in A.HEADS:
        G = n_head // n_head_kv
        for form, n_qs in (("decode", (1, 3)), ("prompt", (A.PROMPT_MIN_Q,))):
            for n_q in n_qs:
                # n_kv = 1: every row that sees anything sees position 0 alone (causal: the last row only; not causal: all of them)
                case = (D, n_head, n_head_kv, kv_type, n_q, 1)
                Vd = _staged(form, kv_type, A.inputs(case)[4])
                for causal in (True, False):
                    got = _run(dev, case, causal=causal, layout=1)
                    for t in range(n_q):
                        for h in range(n_head):
                            want = Vd[0, h // G] if A.visible(t, 1, n_q, causal) else np.zeros(D, np.float32)
                            assert np.array_equal(got[t, h].view(np.uint32), want.view(np.uint32)), (case, causal, t, h)
                # no visible position at all: d_n_kv = 0 over a cache that has room
                got = _run(dev, case, n_kv=0, n_kv_max=300, device_n_kv=True)
                assert np.array_equal(got.view(np.uint32), np.zeros_like(got).view(np.uint32)), case
        # causal row t = 0 at n_kv = n_q sees position 0 alone, in both forms
        for form, n_q in (("decode", 3), ("prompt", 3 * A.CHUNK - 5)):
            case = (D, n_head, n_head_kv, kv_type, n_q, n_q) if form == "prompt" else None
            if case is None:
                base = (D, n_head, n_head_kv, kv_type, 3, A.CHUNK + 1)
                got = _run(dev, base, n_kv=3, n_kv_max=A.CHUNK + 1)
                Vd = A.inputs(base)[4]
            else:
                got = _run(dev, case)
                Vd = _staged(form, kv_type, A.inputs(case)[4])
            for h in range(n_head):
                assert np.array_equal(got[0, h].view(np.uint32), Vd[0, h // G].view(np.uint32)), (form, D, kv_type, h)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_v_that_is_constant_over_the_positions_comes_back_inside_the_tolerance(dev, kv_type):
    """not exact in either form (the header: a and l round independently), so held to the form's tolerance against the constant itself"""
    D = 128
    for form, n_q, n_kv in (("decode", 3, 3 * A.CHUNK - 5), ("prompt", A.PROMPT_MIN_Q, 3 * A.CHUNK - 5)):
        case = (D, 4, 2, kv_type, n_q, n_kv)
        const = (np.arange(2 * D, dtype=np.float32).reshape(2, D) - 100.0) / 128.0        # f16-exact values; a Q8_0 cache keeps its own rounding of them
        Vraw = A.encode_rows(kv_type, np.broadcast_to(const, (n_kv, 2, D)))
        Vd = A.decode_rows(kv_type, Vraw, D)                                            # what the cache holds, whatever the format kept of it
        got = _run(dev, case, V=Vraw)
        want = _staged(form, kv_type, Vd)[0]
        st = np.abs(got.astype(np.float64) - want[None, np.arange(4) // 2]).max() / np.abs(Vd).max()
        print(form, kv_type, "constant V statistic", st)
        assert st <= (A.TOL_DECODE if form == "decode" else A.TOL_PROMPT), (form, st)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
@pytest.mark.parametrize("D", [64, 128])
def test_a_row_does_not_depend_on_the_launch_around_it(dev, D, kv_type):
    torch = dev.torch
    n_kv = 3 * A.CHUNK - 5
    for form, n_q in (("decode", 3), ("prompt", A.PROMPT_MIN_Q)):
        case = (D, 8, 2, kv_type, n_q, n_kv)
        base = _run(dev, case)
        assert np.array_equal(base, _run(dev, case, layout=1, pad=8)), (form, "strides")
        assert np.array_equal(base, _run(dev, case, n_kv_max=n_kv + 700)), (form, "n_kv_max")
        assert np.array_equal(base, _run(dev, case, n_kv_max=n_kv + 700, device_n_kv=True)), (form, "d_n_kv")
        assert np.array_equal(base[:, :4], _run(dev, case, heads=slice(0, 4))), (form, "n_head")
        if form == "decode":
            for t in range(n_q):                                    # the row alone sees the same positions with n_kv - (n_q - 1 - t) in the cache
                alone = _run(dev, case, rows=slice(t, t + 1), n_kv=n_kv - (n_q - 1 - t), n_kv_max=n_kv)
                assert np.array_equal(base[t:t + 1], alone), (form, "n_q", t)
        # heads that share a kv head, given identical q rows, give identical outputs
        q = A.inputs(case)[0]
        saved = q.copy()
        try:
            q[:, 1:4] = q[:, 0:1]
            same = _run(dev, case)
            for h in range(1, 4):
                assert np.array_equal(same[:, 0], same[:, h]), (form, "shared kv head", h)
        finally:
            q[:] = saved


@pytest.mark.gpu
def test_kv_store_bits_surroundings_and_the_position_on_the_device(dev):
    torch = dev.torch
    rng = np.random.default_rng(11)
    for kv_type in (F16, Q8_0):
        for D, n_head_kv in ((64, 1), (128, 2), (128, 3)):
            row_elems, n_rows, n_pos = n_head_kv * D, 5, 12
            rb = A.row_bytes(kv_type, row_elems)
            nb_pos = _up16(rb) + 32
            x = rng.uniform(-1, 1, (n_rows, row_elems)).astype(np.float32)
            x[0, :8] = [6.0e-8, -6.0e-8, 65520.0, -1.0e6, 0.0, -0.0, 65504.0, 2.98e-8]       # subnormals, overflow to inf, both zeros, the f16 maximum, half the least subnormal
            x[1, 32:64] = 0.0                                                                # an all-zero Q8_0 block
            xs = torch.zeros((n_rows, row_elems + 4), device="cuda")
            xs[:, :row_elems] = torch.from_numpy(x).cuda()
            with np.errstate(over="ignore"):
                want_rows = (np.asarray(O.quantize_row(Q8_0, x)).reshape(n_rows, -1) if kv_type == Q8_0
                             else x.astype(np.float16).view(np.uint8).reshape(n_rows, -1))
            assert np.array_equal(want_rows, A.encode_rows(kv_type, x))
            def expect(p0):
                buf = np.full(n_pos * nb_pos, 0xA5, np.uint8)
                for i in range(n_rows):
                    if 0 <= p0 + i < n_pos:
                        buf[(p0 + i) * nb_pos:(p0 + i) * nb_pos + rb] = want_rows[i]
                return buf
            for p0 in (0, 3, n_pos - 2, -3, n_pos, -100):            # inside, clipped at either end, wholly outside
                for on_device in (False, True):
                    cache = torch.full((n_pos * nb_pos,), 0xA5, dtype=torch.uint8, device="cuda")
                    d_p = torch.tensor([p0], dtype=torch.int32, device="cuda") if on_device else None
                    dev.kv_store(kv_type, xs[:, :row_elems], cache, nb_pos, n_pos, pos0=(12345 if on_device else p0), d_pos0=d_p)
                    torch.cuda.synchronize()
                    assert np.array_equal(cache.cpu().numpy(), expect(p0)), (kv_type, D, n_head_kv, p0, on_device)
            # a captured call follows the position it finds on the device
            cache = torch.full((n_pos * nb_pos,), 0xA5, dtype=torch.uint8, device="cuda")
            d_p = torch.tensor([1], dtype=torch.int32, device="cuda")
            one = xs[:1, :row_elems]
            s = torch.cuda.Stream()
            s.wait_stream(torch.cuda.current_stream())
            with torch.cuda.stream(s):
                g = torch.cuda.CUDAGraph()
                with torch.cuda.graph(g, stream=s):
                    dev.kv_store(kv_type, one, cache, nb_pos, n_pos, d_pos0=d_p)
            torch.cuda.current_stream().wait_stream(s)
            want = np.full(n_pos * nb_pos, 0xA5, np.uint8)
            for p0 in (4, 9):
                d_p.fill_(p0)
                g.replay()
                torch.cuda.synchronize()
                want[p0 * nb_pos:p0 * nb_pos + rb] = want_rows[0]
                assert np.array_equal(cache.cpu().numpy(), want), (kv_type, D, p0)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_captured_decode_step_follows_the_cache_as_it_grows(dev, kv_type):
    """kv_store at d_pos0, attention with d_n_kv, captured ONCE; replayed for three successive positions with the two device integers
    rewritten in between; every replay equals a fresh uncaptured call bit for bit"""
    torch = dev.torch
    D, n_head, n_head_kv, n_max = 128, 8, 2, 2 * A.CHUNK + 40
    start = 2 * A.CHUNK - 1                                          # the three steps cross a chunk boundary
    rng = np.random.default_rng(21)
    hist = rng.uniform(-1, 1, (2, start, n_head_kv, D)).astype(np.float32)
    cache = Cache(dev, kv_type, D, n_head_kv, n_max, 0, A.encode_rows(kv_type, hist[0]), A.encode_rows(kv_type, hist[1]))
    assert cache.nb_head >= A.row_bytes(kv_type, D)
    kv_new = torch.zeros((2, n_head_kv, D), device="cuda")
    q = torch.zeros((1, n_head, D), device="cuda")
    out = torch.zeros((1, n_head, D), device="cuda")
    work = torch.empty(dev.attn_work_size(kv_type, D, n_head, n_head_kv, 1, n_max), dtype=torch.uint8, device="cuda")
    d_pos = torch.zeros(1, dtype=torch.int32, device="cuda")
    d_n = torch.zeros(1, dtype=torch.int32, device="cuda")

    def step(kc, vc, o, dp, dn, host_pos=None):
        for hk in range(n_head_kv):                                  # (the heads of a position are padded apart: one store per head and side)
            for side, c in ((0, kc), (1, vc)):
                dev.kv_store(kv_type, kv_new[side, hk:hk + 1], c[hk * cache.nb_head:], cache.nb_pos, n_max, pos0=host_pos or 0, d_pos0=dp)
        dev.attention(kv_type, q, kc, vc, cache.nb_pos, cache.nb_head, n_head_kv, (host_pos + 1) if dn is None else 0, d_n_kv=dn, n_kv_max=n_max, out=o, work=work)

    d_pos.fill_(start)
    d_n.fill_(start + 1)
    step(cache.k.clone(), cache.v.clone(), torch.zeros_like(out), d_pos, d_n)      # (a first call outside the capture, on copies: one-time kernel attributes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(cache.k, cache.v, out, d_pos, d_n)
    torch.cuda.current_stream().wait_stream(s)
    fk, fv = cache.k.clone(), cache.v.clone()                        # the fresh calls keep a cache of their own
    for i in range(3):
        pos = start + i
        kv_new.copy_(torch.from_numpy(rng.uniform(-1, 1, (2, n_head_kv, D)).astype(np.float32)))
        q.copy_(torch.from_numpy(rng.uniform(-1, 1, (1, n_head, D)).astype(np.float32)))
        d_pos.fill_(pos)
        d_n.fill_(pos + 1)
        g.replay()
        fresh = torch.zeros_like(out)
        step(fk, fv, fresh, None, None, host_pos=pos)
        torch.cuda.synchronize()
        assert torch.equal(out, fresh) and torch.equal(cache.k, fk) and torch.equal(cache.v, fv), (kv_type, i)
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0


@pytest.mark.gpu
def test_a_decoder_layers_attention_half_as_device_entries(dev):
    """q / k / v through mul_mat_multi_dev -> kv_store -> attention -> the output projection with the add epilogue: hidden 1024, 8 heads of 128,
    2 kv heads, Q8_0 weights, a Q8_0 cache.  The attention output against the f64 reference under TOL_DECODE, everything else against the
    library's own single calls, bitwise."""
    torch = dev.torch
    L, check = _lib.lib(), _lib.check
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, n_head, n_head_kv, D, n_past, n_max = 1024, 8, 2, 128, A.CHUNK + 7, 2 * A.CHUNK
    rng = np.random.default_rng(31)
    mk = lambda M, K: dev.Weight.from_host(Q8_0, O.quantize_row(Q8_0, (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)), K)
    Wq, Wk, Wv, Wo = mk(n_head * D, H), mk(n_head_kv * D, H), mk(n_head_kv * D, H), mk(H, n_head * D)
    hist = rng.uniform(-1, 1, (2, n_past, n_head_kv, D)).astype(np.float32)
    rb = A.row_bytes(Q8_0, D)
    nb_head, nb_pos = rb, n_head_kv * rb                             # the heads of a position back to back: one store per side (144-byte rows)
    kc = torch.full((n_max * nb_pos,), 0xFF, dtype=torch.uint8, device="cuda")
    vc = kc.clone()
    for c, hraw in ((kc, A.encode_rows(Q8_0, hist[0])), (vc, A.encode_rows(Q8_0, hist[1]))):
        c[:n_past * nb_pos] = torch.from_numpy(hraw.reshape(-1)).cuda()
    x = torch.from_numpy(rng.uniform(-1, 1, (1, H)).astype(np.float32)).cuda()
    resid = torch.from_numpy(rng.uniform(-1, 1, (1, H)).astype(np.float32)).cuda()
    qkv = [torch.empty((1, w.M), device="cuda") for w in (Wq, Wk, Wv)]
    hw = (C.c_void_p * 3)(Wq.handle, Wk.handle, Wv.handle)
    dp = (C.c_void_p * 3)(*[o.data_ptr() for o in qkv])
    ld = (C.c_int64 * 3)(*[o.stride(0) for o in qkv])
    check(L.ggml_hip_mul_mat_multi_dev(hw, 3, _p(x.data_ptr()), H, 1, dp, ld, None, 0, None, None, st), "q / k / v")
    for o, w in zip(qkv, (Wq, Wk, Wv)):
        assert torch.equal(o, dev.mul_mat(w, x))
    d_pos = torch.tensor([n_past], dtype=torch.int32, device="cuda")
    d_n = torch.tensor([n_past + 1], dtype=torch.int32, device="cuda")
    dev.kv_store(Q8_0, qkv[1], kc, nb_pos, n_max, d_pos0=d_pos)
    dev.kv_store(Q8_0, qkv[2], vc, nb_pos, n_max, d_pos0=d_pos)
    for c, o in ((kc, qkv[1]), (vc, qkv[2])):
        assert torch.equal(c[n_past * nb_pos:(n_past + 1) * nb_pos], dev.quantize_rows(Q8_0, o).reshape(-1))
    att = dev.attention(Q8_0, qkv[0].view(1, n_head, D), kc, vc, nb_pos, nb_head, n_head_kv, 0, d_n_kv=d_n, n_kv_max=n_max)
    work = dev.alloc_work(Q8_0, n_head * D, 1)
    prod, out = torch.empty((1, H), device="cuda"), torch.empty((1, H), device="cuda")
    a2 = att.view(1, n_head * D)
    check(L.ggml_hip_mul_mat_epilogue_dev(Wo.handle, _p(a2.data_ptr()), 1, n_head * D, _p(prod.data_ptr()), H, _p(work.data_ptr()), work.numel(), 1,
                                          _p(resid.data_ptr()), H, _p(out.data_ptr()), H, 1.0, st), "output projection + residual")
    torch.cuda.synchronize()
    single = dev.mul_mat(Wo, a2)
    assert torch.equal(prod, single) and torch.equal(out, single + resid)
    Kd = A.decode_rows(Q8_0, kc.cpu().numpy()[:(n_past + 1) * nb_pos].reshape(n_past + 1, n_head_kv, rb), D)
    Vd = A.decode_rows(Q8_0, vc.cpu().numpy()[:(n_past + 1) * nb_pos].reshape(n_past + 1, n_head_kv, rb), D)
    ref = A.reference(qkv[0].cpu().numpy().reshape(1, n_head, D), Kd, Vd, n_past + 1, True, 1.0 / np.sqrt(D))
    stat = A.statistic(att.cpu().numpy(), ref, Vd)
    print("layer attention statistic", stat, "bar", A.TOL_DECODE)
    assert stat <= A.TOL_DECODE
    for w in (Wq, Wk, Wv, Wo):
        w.free()
