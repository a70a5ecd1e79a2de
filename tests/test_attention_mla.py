"""MLA: latent attention over a latent KV cache (include/ggml_hip_ext.h, section MLA: ggml_hip_attn_mla_dev, ggml_hip_attn_mla_paged_dev, their plans
and work sizes, ggml_hip_kv_store_latent_paged_dev; csrc/mla.hip, mla.cpp, plan.cpp plan_attn_mla).

Yardsticks (tests/np_attention_mla.py): the float64 reference on the dequantized cache, and the numpy model of the header's statement whose worst
statistic over the CPU sweep, per form, is recorded there; the kernels are held to 4 x it.  The contracts are held to bits (uint32): one visible
position returns the staged V row; a row's bits follow its own q row, the cache bytes below its vis, scale, the cache type and the form only; paged
equals contiguous; the latent store equals ggml_hip_kv_store_dev at row_elems = 576.  The span is read from the plan, never from a literal.
Shapes: n_head in {1, 16, 24, 128} (24: rows of different tokens and a partial last tile share a workgroup; 128 against the reference only), both cache
types, n_q in {1, 3, 8} (SPLIT) and {9, 70} (WALK), n_kv in {1, 31, 128, 129, 379, 128 span + 1, 256 span + 37} (n_kv < n_q included), causal on and off.
The step, chunk and span edges, the other n_q and head counts, explicit scales, steep scores and planted keys: tests/test_attention_mla_edges.py."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_attention as A
import np_attention_mla as M
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, Q8_0 = A.F16, A.Q8_0
DK, DV = M.D_K, M.D_V
NEW_SYMBOLS = ("ggml_hip_attn_mla_plan", "ggml_hip_attn_mla_work_size", "ggml_hip_attn_mla_paged_plan", "ggml_hip_attn_mla_paged_work_size",
               "ggml_hip_attn_mla_dev", "ggml_hip_attn_mla_paged_dev", "ggml_hip_kv_store_latent_paged_dev")
NEW_WRAPPERS = ("attn_mla_plan", "attn_mla_work_size", "attention_mla", "attn_mla_paged", "kv_store_latent_paged", "LatentCache")
PAGE = M.CHUNK
SENTINEL = np.float32(3.0e38)


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _up16(n):
    return (n + 15) // 16 * 16


def _plan(kv_type, n_head, n_q, n_kv_max, n_seq=None, dk=DK, dv=DV):
    out = _lib.ggml_hip_attn_mla_plan_t()
    L = _lib.lib()
    if n_seq is None:
        return L.ggml_hip_attn_mla_plan(kv_type, dk, dv, n_head, n_q, n_kv_max, C.byref(out)), out
    return L.ggml_hip_attn_mla_paged_plan(kv_type, dk, dv, n_head, n_seq, n_q, n_kv_max, C.byref(out)), out


def span():
    """MLA_SPAN, from the plan"""
    rc, p = _plan(F16, 1, 1, 1)
    assert rc == 0 and p.span in (1, 2, 4, 8)
    return p.span


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    dev_src = open(os.path.join(ROOT, "ggmlsharp_amd", "device.py")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert name in dev_src, name
    for name in NEW_WRAPPERS:
        assert re.search(r"^(def|class) %s\b" % name, dev_src, flags=re.M), name
    assert C.sizeof(_lib.ggml_hip_attn_mla_plan_t) == 56


def test_the_plan_follows_its_statement():
    S = span()
    for kv_type in (F16, Q8_0):
        for n_head in (1, 16, 24, 128, 256):
            for n_kv_max in (0, 1, 128 * S, 128 * S + 1, 5000, 32768):
                n_spans = (n_kv_max + 128 * S - 1) // (128 * S)
                for n_q in (1, 3, 8, 9, 70, 2048):
                    for n_seq in (None, 1, 4, 32):
                        rc, p = _plan(kv_type, n_head, n_q, n_kv_max, n_seq)
                        ns = 1 if n_seq is None else n_seq
                        tiles = (n_q * n_head + p.q_tile - 1) // p.q_tile
                        assert rc == 0 and p.form == (M.SPLIT if n_q <= M.SPLIT_MAX_Q else M.WALK)         # the form from n_q alone
                        assert (p.chunk, p.span, p.q_tile, p.step, p.n_spans) == (128, S, 64, M.STEP, n_spans)
                        if p.form == M.SPLIT:
                            assert (p.launches, p.workgroups, p.merge_workgroups) == (2, tiles * n_spans * ns, ns * n_q * n_head)
                            assert p.work_bytes == (ns * n_q * n_head * n_spans * (DV + 4) * 4 + 255) // 256 * 256 + 256 if n_spans else p.work_bytes == 0
                        else:
                            assert (p.launches, p.workgroups, p.merge_workgroups, p.work_bytes) == (1, tiles * ns, 0, 0)
                        W = _lib.lib().ggml_hip_attn_mla_work_size(kv_type, DK, DV, n_head, n_q, n_kv_max) if n_seq is None else \
                            _lib.lib().ggml_hip_attn_mla_paged_work_size(kv_type, DK, DV, n_head, n_seq, n_q, n_kv_max)
                        assert W == p.work_bytes
    rc, p = _plan(F16, 16, 0, 4096)
    assert rc == 0 and p.form == 0 and p.span == S and p.work_bytes == 0


def test_the_work_size_is_monotone():
    W = _lib.lib().ggml_hip_attn_mla_paged_work_size
    for kv_type in (F16, Q8_0):
        last_h = 0
        for n_head in (1, 16, 128, 256):
            last_q = 0
            for n_q in (1, 3, 8):
                last_s = 0
                for n_seq in (1, 2, 32, 4096):
                    last = 0
                    for n_kv_max in (1, 128, 129, 1000, 1001, 40000):
                        w = W(kv_type, DK, DV, n_head, n_seq, n_q, n_kv_max)
                        assert w >= last and w > 0
                        last = w
                    assert last >= last_s
                    last_s = last
                assert last_s >= last_q
                last_q = last_s
            assert last_q >= last_h
            last_h = last_q
        assert W(kv_type, DK, DV, 16, 4, 0, 4096) == 0 and W(kv_type, DK, DV, 16, 0, 1, 4096) == 0 and W(kv_type, DK, DV, 16, 4, 9, 4096) == 0
        assert W(kv_type, 512, DV, 16, 4, 1, 4096) == 0


def _rc(kv_type=F16, ptr=0x1000, ldq=(16 * DK, DK), cache=0x1000, nb_pos=1152, n_head=16, dk=DK, dv=DV, n_q=1, n_kv=256, d_n_kv=None, n_kv_max=256,
        dst=0x1000, ldd=(16 * DV, DV), work=0x1000, work_bytes=1 << 30):
    return _lib.lib().ggml_hip_attn_mla_dev(kv_type, _p(ptr), ldq[0], ldq[1], _p(cache), nb_pos, n_head, dk, dv, n_q, n_kv, _p(d_n_kv), n_kv_max, 1, 0.125,
                                            _p(dst), ldd[0], ldd[1], _p(work), work_bytes, None)


def _rc_paged(kv_type=F16, ptr=0x1000, ldq=(16 * DK, DK), pool=0x1000, nb_page=128 * 1152, nb_pos=1152, n_pages=4, pages=0x1000, ld_pages=2, d_len=0x1000,
              n_seq=2, n_head=16, dk=DK, dv=DV, n_q=1, n_kv_max=256, dst=0x1000, ldd=(16 * DV, DV), work=0x1000, work_bytes=1 << 30):
    return _lib.lib().ggml_hip_attn_mla_paged_dev(kv_type, _p(ptr), ldq[0], ldq[1], _p(pool), nb_page, nb_pos, n_pages, _p(pages), ld_pages, _p(d_len), 1, n_seq,
                                                  n_head, dk, dv, n_q, n_kv_max, 1, 0.125, _p(dst), ldd[0], ldd[1], _p(work), work_bytes, None)


def _rc_store(kv_type=F16, src=0x1000, ld=DK, n_seq=2, n_q=1, pool=0x1000, nb_page=128 * 1152, nb_pos=1152, n_pages=4, pages=0x1000, ld_pages=2, d_len=0x1000,
              n_kv_max=256):
    return _lib.lib().ggml_hip_kv_store_latent_paged_dev(kv_type, _p(src), ld, n_seq, n_q, _p(pool), nb_page, nb_pos, n_pages, _p(pages), ld_pages, _p(d_len),
                                                         n_kv_max, None)


def test_what_is_not_served_is_refused_before_anything_is_launched():
    """every call below carries pointers that are not device memory: a launch would fault, a refusal returns its code.  Each call breaks ONE stated host rule."""
    E = _lib
    for rc in (_rc, _rc_paged):
        for t in (0, 2, 7, 9, _lib.BF16):
            assert rc(kv_type=t) == E.ERR_TYPE
        assert rc(dk=512) == E.ERR_SHAPE and rc(dv=576) == E.ERR_SHAPE and rc(dk=128, dv=128) == E.ERR_SHAPE and rc(dk=192, dv=128) == E.ERR_SHAPE
        assert rc(n_head=0) == E.ERR_SHAPE and rc(n_head=257) == E.ERR_SHAPE
        assert rc(ldq=(16 * DK + 2, DK)) == E.ERR_SHAPE and rc(ldq=(16 * DK, DK + 2)) == E.ERR_SHAPE and rc(ldq=(16 * DK, DK - 4)) == E.ERR_SHAPE
        assert rc(ldd=(16 * DV, DV - 4)) == E.ERR_SHAPE and rc(ldd=(16 * DV + 1, DV)) == E.ERR_SHAPE
        assert rc(n_q=2, ldq=(DK - 4, DK)) == E.ERR_SHAPE and rc(n_q=2, ldd=(DV - 4, DV)) == E.ERR_SHAPE
        assert rc(nb_pos=1136) == E.ERR_SHAPE and rc(nb_pos=1160) == E.ERR_SHAPE and rc(kv_type=Q8_0, nb_pos=640) == E.ERR_SHAPE
        assert rc(work=None) == E.ERR_ARG and rc(work_bytes=1024) == E.ERR_ARG
        assert rc(ptr=None) == E.ERR_ARG and rc(dst=None) == E.ERR_ARG and rc(ptr=0x1008) == E.ERR_SHAPE
        assert rc(n_q=-1) == E.ERR_ARG and rc(n_kv_max=-1) == E.ERR_ARG and rc(n_kv_max=(1 << 24) + 1) == E.ERR_SHAPE and rc(n_q=(1 << 20) + 1) == E.ERR_SHAPE
        assert rc(n_q=0) == 0                                         # nothing to do, after every shape check
    assert _rc(n_kv=257) == E.ERR_ARG and _rc(n_kv=-1) == E.ERR_ARG and _rc(cache=None) == E.ERR_ARG and _rc(d_n_kv=0x1002) == E.ERR_SHAPE
    for rc in (_rc_paged, _rc_store):
        assert rc(pages=None) == E.ERR_ARG and rc(d_len=None) == E.ERR_ARG and rc(n_pages=0) == E.ERR_ARG
        assert rc(n_seq=0) == E.ERR_SHAPE and rc(n_seq=4097) == E.ERR_SHAPE and rc(ld_pages=1) == E.ERR_SHAPE
        assert rc(nb_page=128 * 1152 - 16) == E.ERR_SHAPE and rc(nb_page=128 * 1152 + 4) == E.ERR_SHAPE and rc(pool=None) == E.ERR_ARG
        assert rc(pages=0x1002) == E.ERR_SHAPE
    assert _rc_paged(n_seq=4096, n_q=512) == E.ERR_SHAPE             # n_seq * n_q above 2^20
    assert _rc_store(kv_type=2) == E.ERR_TYPE and _rc_store(ld=DK + 2) == E.ERR_SHAPE and _rc_store(ld=DK - 4) == E.ERR_SHAPE and _rc_store(src=None) == E.ERR_ARG
    assert _rc_store(nb_pos=1136) == E.ERR_SHAPE and _rc_store(kv_type=Q8_0, nb_pos=640) == E.ERR_SHAPE and _rc_store(pool=0x1008) == E.ERR_SHAPE
    assert _rc_store(n_q=-1) == E.ERR_ARG and _rc_store(n_q=0) == 0
    for bad in ((F16, 128, 128), (2, DK, DV)):
        rc, _ = _plan(bad[0], 16, 1, 256, dk=bad[1], dv=bad[2])
        assert rc == (E.ERR_TYPE if bad[0] == 2 else E.ERR_SHAPE)
    assert _plan(F16, 257, 1, 256)[0] == E.ERR_SHAPE and _plan(F16, 16, 1, 256, n_seq=0)[0] == E.ERR_SHAPE
    assert _lib.lib().ggml_hip_attn_mla_plan(F16, DK, DV, 16, 1, 256, None) == E.ERR_ARG


def _model_worst(form, S, mutant=None, n_heads=M.N_HEADS):
    worst = 0.0
    for case in M.cases(form, S, n_heads):
        kv_type, n_head, n_q, n_kv, causal = case
        ref, V = M.case_reference(case)
        got = M.model(M.queries(n_head, n_q), M.cache_rows(kv_type, n_kv)[1], n_kv, causal, M.SCALE, S, mutant=mutant)
        worst = max(worst, A.statistic(got, ref, V))
    return worst


def test_the_model_constants_are_what_the_model_measures():
    """the numpy model of each form against the f64 reference on the whole CPU sweep: its worst statistic is the recorded constant (rounded up)"""
    S = span()
    for form, rec in ((M.SPLIT, M.MODEL_WORST_SPLIT), (M.WALK, M.MODEL_WORST_WALK)):
        worst = _model_worst(form, S)
        print("form", form, "model worst", worst, "recorded", rec)
        assert rec / 1.25 <= worst <= rec, (form, worst, rec)


def test_the_bar_sees_the_four_mutants():
    """each wrong statement exceeds the tolerance of its form at least 100-fold on the sweep's inputs (the merge exists in SPLIT only)"""
    S = span()
    for form, tol in ((M.SPLIT, M.TOL_SPLIT), (M.WALK, M.TOL_WALK)):
        for mutant in M.MUTANTS:
            if mutant == "merge_no_b" and form == M.WALK:
                continue
            worst = _model_worst(form, S, mutant, n_heads=(16,))
            print("form", form, "mutant", mutant, "worst", worst, "bar", tol)
            assert worst >= 100 * tol, (form, mutant, worst, tol)


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def contiguous_cache(dev, kv_type, n, tag="c", n_alloc=None, pad=0):
    """a contiguous cache of n seeded positions (nb_pos = row bytes rounded up to 16, + pad), 0xFF (NaN) bytes everywhere else -> (tensor, nb_pos)"""
    rb = M.row_bytes(kv_type)
    nb_pos = _up16(rb) + pad
    buf = np.full((max(n if n_alloc is None else n_alloc, 1), nb_pos), 0xFF, np.uint8)
    buf[:n, :rb] = M.cache_rows(kv_type, n, tag)[0]
    return dev.torch.from_numpy(buf.reshape(-1)).cuda(), nb_pos


_GOT = {}


def run(dev, case, tag="c", qtag="q"):
    """ggml_hip_attn_mla_dev on a sweep case, computed once -> numpy [n_q, n_head, 512]"""
    key = (case, tag, qtag)
    if key not in _GOT:
        torch = dev.torch
        kv_type, n_head, n_q, n_kv, causal = case
        cache, nb_pos = contiguous_cache(dev, kv_type, n_kv, tag)
        q = torch.from_numpy(M.queries(n_head, n_q, qtag)).cuda()
        out = dev.attention_mla(kv_type, q, cache, nb_pos, n_kv, M.SCALE, causal=causal)
        torch.cuda.synchronize()
        _GOT[key] = out.cpu().numpy()
    return _GOT[key]


@pytest.mark.gpu
@pytest.mark.parametrize("form", [M.SPLIT, M.WALK])
@pytest.mark.parametrize("n_head", [1, 16, 24, 128])
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_the_sweep_is_inside_the_tolerance_of_the_f64_reference(dev, kv_type, n_head, form):
    S = span()
    tol = M.TOL_SPLIT if form == M.SPLIT else M.TOL_WALK
    worst = 0.0
    for case in M.cases(form, S, (n_head,)):
        if case[0] != kv_type:
            continue
        rc, p = _plan(kv_type, n_head, case[2], case[3])
        assert rc == 0 and p.form == form
        got = run(dev, case)
        assert np.isfinite(got).all(), case
        ref, V = M.case_reference(case)
        st = A.statistic(got, ref, V)
        worst = max(worst, st)
        print(case, "statistic", st, "bar", tol)
        assert st <= tol, (case, st, tol)
    print("kv_type", kv_type, "n_head", n_head, "form", form, "worst", worst, "bar", tol)


def staged_v(kv_type, n, tag="c"):
    """the staged V rows: deq for F16, f16(deq) for Q8_0 -> f32 [n, 512]"""
    deq = M.cache_rows(kv_type, n, tag)[1][:, :DV]
    return deq if kv_type == F16 else M._h(deq)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_one_visible_position_returns_the_staged_v_row_bit_for_bit(dev, kv_type):
    v0 = staged_v(kv_type, 1)[0]
    for n_head in (1, 24):
        for n_q in (1, 3, 9, 70):
            got = run(dev, (kv_type, n_head, n_q, 1, False))         # every row sees position 0 alone
            assert np.array_equal(bits(got), bits(np.broadcast_to(v0, got.shape))), (n_head, n_q)
            got = run(dev, (kv_type, n_head, n_q, 1, True))          # the last token does, the others see nothing: +0.0f
            assert np.array_equal(bits(got[-1]), bits(np.broadcast_to(v0, got[-1].shape))) and not bits(got[:-1]).any(), (n_head, n_q)
        for n in (3, 8, 9, 70):                                       # n_q = n_kv, causal: row 0 sees position 0 alone inside a longer cache
            got = run(dev, (kv_type, n_head, n, n, True))
            assert np.array_equal(bits(got[0]), bits(np.broadcast_to(v0, got[0].shape))), (n_head, n)


def call_padded(dev, case, n_kv_max=None, device_n_kv=False, pad=True, tag="c"):
    """the same call through padded strides: 3.0e38 in every gap of q and dst and around the work buffer; every input is compared after the call"""
    torch = dev.torch
    kv_type, n_head, n_q, n_kv, causal = case
    n_kv_max = n_kv if n_kv_max is None else n_kv_max
    hp, dp = (1, 8) if pad else (0, 0)
    cache, nb_pos = contiguous_cache(dev, kv_type, n_kv, tag, n_alloc=n_kv_max, pad=48 if pad else 0)
    cache0 = cache.clone()
    q_host = np.full((n_q, n_head + hp, DK + dp), SENTINEL, np.float32)
    q_host[:, :n_head, :DK] = M.queries(n_head, n_q)
    q_big = torch.from_numpy(q_host).cuda()
    dst_big = torch.full((n_q, n_head + hp, DV + dp), float(SENTINEL), dtype=torch.float32, device="cuda")
    need = dev.attn_mla_work_size(kv_type, n_head, n_q, n_kv_max)
    guard = 512
    work_big = torch.full((need + 2 * guard,), 0xA5, dtype=torch.uint8, device="cuda")
    d_n_kv = torch.tensor([n_kv], dtype=torch.int32, device="cuda") if device_n_kv else None
    out = dev.attention_mla(kv_type, q_big[:, :n_head, :DK], cache, nb_pos, -5 if device_n_kv else n_kv, M.SCALE, d_n_kv=d_n_kv, n_kv_max=n_kv_max, causal=causal,
                            out=dst_big[:, :n_head, :DV], work=work_big[guard:guard + max(need, 16)])
    torch.cuda.synchronize()
    assert torch.equal(q_big.cpu(), torch.from_numpy(q_host)) and torch.equal(cache, cache0)
    d = dst_big.cpu().numpy()
    assert (d[:, n_head:, :] == SENTINEL).all() and (d[:, :, DV:] == SENTINEL).all(), "a gap of dst was written"
    w = work_big.cpu().numpy()
    assert (w[:guard] == 0xA5).all() and (w[guard + max(need, 16):] == 0xA5).all(), "the work buffer's guards were written"
    return out.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_rows_bits_follow_its_own_inputs_only(dev, kv_type):
    S = span()
    long_kv = 2 * PAGE * S + 37
    for n_q in (3, 8, 9, 70):
        for n_kv in (129, long_kv):
            case = (kv_type, 24, n_q, n_kv, True)
            base = run(dev, case)
            assert np.array_equal(bits(call_padded(dev, case)), bits(base)), ("padded strides", case)
            assert np.array_equal(bits(call_padded(dev, case, n_kv_max=n_kv + 700, pad=False)), bits(base)), ("n_kv_max", case)
            assert np.array_equal(bits(call_padded(dev, case, n_kv_max=n_kv + 131, device_n_kv=True, pad=False)), bits(base)), ("device n_kv", case)
    # head h of a 24-head call against the same rows alone at n_head = 1
    torch = dev.torch
    for n_q in (3, 9):
        case = (kv_type, 24, n_q, long_kv, True)
        base = run(dev, case)
        cache, nb_pos = contiguous_cache(dev, kv_type, long_kv)
        for h in (0, 7, 23):
            q1 = torch.from_numpy(np.ascontiguousarray(M.queries(24, n_q)[:, h:h + 1])).cuda()
            one = dev.attention_mla(kv_type, q1, cache, nb_pos, long_kv, M.SCALE).cpu().numpy()
            assert np.array_equal(bits(one[:, 0]), bits(base[:, h])), ("n_head", n_q, h)
    # rows of equal vis across two n_q of one form: the last rows of the longer call, causal; every row, not causal
    for small, big in ((3, 8), (9, 70)):
        for causal in (True, False):
            for n_kv in (129, long_kv):
                want = run(dev, (kv_type, 16, big, n_kv, causal))
                qs = M.queries(16, big)[big - small:] if causal else M.queries(16, big)[:small]
                cache, nb_pos = contiguous_cache(dev, kv_type, n_kv)
                got = dev.attention_mla(kv_type, torch.from_numpy(np.ascontiguousarray(qs)).cuda(), cache, nb_pos, n_kv, M.SCALE, causal=causal).cpu().numpy()
                assert np.array_equal(bits(got), bits(want[big - small:] if causal else want[:small])), ("n_q", small, big, causal, n_kv)


class Pool:
    """the host image of a latent pool: n_pages pages of 0xFF bytes (F16 NaN halves, Q8_0 d = NaN), rows put where a table says"""

    def __init__(self, kv_type, n_pages, slack=0, fill=0xFF):
        self.kv_type, self.n_pages, self.rb = kv_type, n_pages, M.row_bytes(kv_type)
        self.nb_pos = _up16(self.rb) + 16
        self.nb_page = _up16((PAGE - 1) * self.nb_pos + self.rb) + slack
        self.host = np.full(n_pages * self.nb_page, fill, np.uint8)

    def put(self, pages, raw, j_from=0):
        for j in range(j_from, raw.shape[0]):
            page = pages[j // PAGE]
            if 0 <= page < self.n_pages:
                o = page * self.nb_page + (j % PAGE) * self.nb_pos
                self.host[o:o + self.rb] = raw[j]

    def cache(self, dev, table, lens, n_kv_max, ld_pages=None, garbage=-7):
        torch = dev.torch
        ld_pages = max((n_kv_max + PAGE - 1) // PAGE, 1) if ld_pages is None else ld_pages
        tab = np.full((len(table), ld_pages), garbage, np.int32)
        for b, pages in enumerate(table):
            tab[b, :len(pages)] = pages
        return dev.LatentCache(self.kv_type, torch.from_numpy(self.host).cuda(), self.nb_page, self.nb_pos, self.n_pages, torch.from_numpy(tab).cuda(),
                               torch.tensor(list(lens), dtype=torch.int32, device="cuda"), n_kv_max)


def paged(dev, kv_type, n_head, n_q, causal, lens, table, n_pages, slack=0, ld_pages=None, n_kv_max=None, len_bias=0):
    """one paged call: every sequence holds the first lens[b] rows of the cache tagged "c" (so a first page can be shared) and asks the same queries"""
    torch = dev.torch
    pool = Pool(kv_type, n_pages, slack)
    for n, pages in zip(lens, table):
        pool.put(pages, M.cache_rows(kv_type, n)[0])
    n_kv_max = max(max(lens), 1) if n_kv_max is None else n_kv_max
    lc = pool.cache(dev, table, [n - len_bias for n in lens], n_kv_max, ld_pages)
    q = torch.from_numpy(np.concatenate([M.queries(n_head, n_q)] * len(lens))).cuda()
    out = dev.attn_mla_paged(lc, q, M.SCALE, len_bias=len_bias, causal=causal)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(lens), n_q, n_head, DV)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_paged_equals_contiguous_bit_for_bit(dev, kv_type):
    S = span()
    lens = (0, 1, 129, 2 * PAGE * S + 37)
    n_long = (lens[3] + PAGE - 1) // PAGE
    long_pages = tuple(2 * n_long + 3 - 2 * c for c in range(n_long))            # descending, every other page: the pages between stay NaN
    shared = long_pages[0]
    table = ((), (1,), (shared, 0), long_pages)                                  # sequences 2 and 3 share their first page
    n_pages = 2 * n_long + 5
    for n_q in (3, 9):
        for causal in (True, False):
            want = [np.zeros((n_q, 16, DV), np.float32) if n == 0 else run(dev, (kv_type, 16, n_q, n, causal)) for n in lens]
            got = paged(dev, kv_type, 16, n_q, causal, lens, table, n_pages)
            for b in range(4):
                assert np.array_equal(bits(got[b]), bits(want[b])), ("paged", n_q, causal, b)
            for what, kw in (("nb_page", dict(slack=80)), ("ld_pages", dict(ld_pages=n_long + 6)), ("n_kv_max", dict(n_kv_max=lens[3] + 700)), ("len_bias", dict(len_bias=5))):
                if not causal:
                    continue                                          # (one pass over the variants per form is enough)
                got = paged(dev, kv_type, 16, n_q, causal, lens, table, n_pages, **kw)
                for b in range(4):
                    assert np.array_equal(bits(got[b]), bits(want[b])), (what, n_q, causal, b)
            # an invalid page id among sequence 3's needed entries: its rows are +0.0f, the others as before
            for bad in (-1, n_pages):
                broken = (table[0], table[1], table[2], long_pages[:2] + (bad,) + long_pages[3:])
                got = paged(dev, kv_type, 16, n_q, causal, lens, broken, n_pages)
                assert not bits(got[3]).any(), ("invalid id", n_q, causal, bad)
                for b in range(3):
                    assert np.array_equal(bits(got[b]), bits(want[b])), ("beside an invalid id", n_q, causal, b)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_the_latent_store_writes_the_bytes_of_kv_store_and_nothing_else(dev, kv_type):
    torch = dev.torch
    n_q, n_kv_max, n_pages = 5, 300, 7
    lens = (0, 126, 297, 40, 200)                                    # 126: crosses onto its second page; 297: its last two tokens lie beyond n_kv_max
    table = ((6,), (2, 4), (5, 1, 0), (-1,), (3, 9))                 # sequence 3: an invalid id, nothing written; sequence 4: its second page invalid
    rng = np.random.default_rng([kv_type, 576, 5])
    x = rng.uniform(-1, 1, (len(lens) * n_q, DK + 8)).astype(np.float32)
    x[:, DK:] = SENTINEL
    pool = Pool(kv_type, n_pages, fill=0xA5)
    lc = pool.cache(dev, table, lens, n_kv_max, garbage=-3)
    xd = torch.from_numpy(x).cuda()
    dev.kv_store_latent_paged(lc, xd[:, :DK])
    # the expectation: ggml_hip_kv_store_dev(row_elems = 576) of the same rows into a contiguous cache, its bytes put where the table says
    rb = M.row_bytes(kv_type)
    flat = torch.full((len(lens) * n_q * _up16(rb),), 0, dtype=torch.uint8, device="cuda")
    dev.kv_store(kv_type, xd[:, :DK], flat, _up16(rb), len(lens) * n_q)
    torch.cuda.synchronize()
    raw = flat.cpu().numpy().reshape(len(lens) * n_q, _up16(rb))[:, :rb]
    assert np.array_equal(raw, A.encode_rows(kv_type, x[:, :DK])), "kv_store itself"
    for b, (n, pages) in enumerate(zip(lens, table)):
        for t in range(n_q):
            pos = n + t
            if pos < n_kv_max and 0 <= pages[pos // PAGE] < n_pages:
                o = pages[pos // PAGE] * pool.nb_page + (pos % PAGE) * pool.nb_pos
                pool.host[o:o + rb] = raw[b * n_q + t]
    assert np.array_equal(lc.pool.cpu().numpy(), pool.host), "the pool differs from the host-built image"
    assert torch.equal(xd.cpu(), torch.from_numpy(x))


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_captured_decode_step_follows_the_lengths(dev, kv_type):
    """latent store, then SPLIT attention, captured once and replayed three times with d_len + 1 in between; sequence 0 crosses onto a new page and into a
    new span.  Each replay is bit for bit the eager contiguous call on the rows the sequence then holds."""
    torch = dev.torch
    S = span()
    n_head, n_seq = 16, 2
    start = (PAGE * S - 1, 5)
    n_kv_max = PAGE * S + 130
    n_tab = (n_kv_max + PAGE - 1) // PAGE
    table = (tuple(3 + 2 * c for c in reversed(range(n_tab))), (2,))         # descending, every other page
    n_pages = 3 + 2 * n_tab + 1
    pool = Pool(kv_type, n_pages)
    held = [M.cache_rows(kv_type, start[b], "g%d" % b) for b in range(n_seq)]
    for b in range(n_seq):
        pool.put(table[b], held[b][0])
    lc = pool.cache(dev, table, start, n_kv_max)
    warm = pool.cache(dev, table, start, n_kv_max)
    rng = np.random.default_rng([kv_type, 99])
    x = torch.zeros((n_seq, DK), device="cuda")
    q = torch.zeros((n_seq, n_head, DK), device="cuda")
    out = torch.zeros((n_seq, n_head, DV), device="cuda")
    work = torch.empty(dev.attn_mla_work_size(kv_type, n_head, 1, n_kv_max, n_seq), dtype=torch.uint8, device="cuda")

    def step(cache, o):
        dev.kv_store_latent_paged(cache, x)
        dev.attn_mla_paged(cache, q, M.SCALE, len_bias=1, out=o, work=work)

    step(warm, torch.zeros_like(out))                                # (a first call outside the capture, on a copy: one-time kernel attributes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(lc, out)
    torch.cuda.current_stream().wait_stream(s)
    rows = [np.array(h[0]) for h in held]                            # the raw rows every sequence holds, grown by the eager store below
    for i in range(3):
        x.copy_(torch.from_numpy(rng.uniform(-1, 1, (n_seq, DK)).astype(np.float32)))
        q.copy_(torch.from_numpy(rng.uniform(-1, 1, (n_seq, n_head, DK)).astype(np.float32)))
        g.replay()
        torch.cuda.synchronize()
        got = out.cpu().numpy()
        for b in range(n_seq):
            n = start[b] + i + 1
            rb = M.row_bytes(kv_type)
            fresh = torch.full((n * _up16(rb),), 0xFF, dtype=torch.uint8, device="cuda")
            fresh.view(n, _up16(rb))[:n - 1, :rb] = torch.from_numpy(rows[b]).cuda()
            dev.kv_store(kv_type, x[b:b + 1], fresh, _up16(rb), n, pos0=n - 1)
            want = dev.attention_mla(kv_type, q[b:b + 1], fresh, _up16(rb), n, M.SCALE).cpu().numpy()
            assert np.array_equal(bits(got[b]), bits(want[0])), ("replay", i, "sequence", b)
            rows[b] = fresh.view(n, _up16(rb))[:, :rb].cpu().numpy()
        lc.d_len += 1
    torch.cuda.synchronize()


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_the_python_face_runs_the_recipe(dev, kv_type):
    """rope in place on the 64-column view of a [n_tok][576] buffer, store, attend -- bit for bit the raw entries on contiguous copies, and inside the tolerance"""
    torch = dev.torch
    L = _lib.lib()
    n_tok, n_head = 70, 16
    rng = np.random.default_rng([kv_type, 576, 7])
    x_host = rng.uniform(-1, 1, (n_tok, DK)).astype(np.float32)
    q_host = M.queries(n_head, n_tok, "face")
    rp = dev.rope_params(64, mode=2, freq_base=10000.0)
    # the Python face: one sequence in a paged cache
    x = torch.from_numpy(x_host).cuda()
    pe = x[:, DV:].unsqueeze(1)                                      # [n_tok, 1, 64], token stride 576
    dev.rope(rp, pe, pos0=0, out=pe)
    pool = Pool(kv_type, 3)
    lc = pool.cache(dev, ((2,),), (0,), n_tok)
    dev.kv_store_latent_paged(lc, x)
    q = torch.from_numpy(q_host).cuda()
    face = dev.attn_mla_paged(lc, q, M.SCALE, len_bias=n_tok).cpu().numpy()
    # the raw entries on contiguous copies
    pe2 = torch.from_numpy(np.ascontiguousarray(x_host[:, DV:])).cuda()
    assert L.ggml_hip_rope_dev(C.byref(rp), _p(pe2.data_ptr()), 64, 64, 1, 64, n_tok, None, 0, None, None, _p(pe2.data_ptr()), 64, 64, dev._stream()) == 0
    x2 = torch.from_numpy(x_host).cuda()
    x2[:, DV:] = pe2
    assert torch.equal(x2, x), "the rotation through the strided view"
    rb = M.row_bytes(kv_type)
    cache = torch.full((n_tok * _up16(rb),), 0xFF, dtype=torch.uint8, device="cuda")
    assert L.ggml_hip_kv_store_dev(kv_type, _p(x2.data_ptr()), DK, n_tok, DK, _p(cache.data_ptr()), _up16(rb), n_tok, 0, None, dev._stream()) == 0
    dst = torch.empty((n_tok, n_head, DV), dtype=torch.float32, device="cuda")
    need = L.ggml_hip_attn_mla_work_size(kv_type, DK, DV, n_head, n_tok, n_tok)
    work = torch.empty(max(need, 16), dtype=torch.uint8, device="cuda")
    assert L.ggml_hip_attn_mla_dev(kv_type, _p(q.data_ptr()), n_head * DK, DK, _p(cache.data_ptr()), _up16(rb), n_head, DK, DV, n_tok, n_tok, None, n_tok, 1,
                                   C.c_float(M.SCALE), _p(dst.data_ptr()), n_head * DV, DV, _p(work.data_ptr()), work.numel(), dev._stream()) == 0
    torch.cuda.synchronize()
    assert np.array_equal(bits(face), bits(dst.cpu().numpy()))
    deq = A.decode_rows(kv_type, cache.cpu().numpy().reshape(n_tok, _up16(rb))[:, :rb], DK)
    ref = M.reference(q_host, deq, n_tok, True, M.SCALE)
    st = A.statistic(face, ref, deq[:, :DV])
    print("the recipe: statistic", st, "bar", M.TOL_WALK)
    assert st <= M.TOL_WALK
