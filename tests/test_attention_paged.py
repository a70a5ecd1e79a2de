"""Paged, multi-sequence attention and KV store (include/ggml_hip_ext.h, PAGED ATTENTION: ggml_hip_kv_store_paged_dev,
ggml_hip_rope_kv_store_paged_dev, ggml_hip_attn_paged_dev, ggml_hip_attn_paged_plan, ggml_hip_attn_paged_work_size; csrc/attn.hip, rope.hip,
attn.cpp, rope.cpp, plan.cpp plan_attn_paged).

Yardsticks.  page = chunk = 128 positions, so a paged call is, per sequence, BIT FOR BIT ggml_hip_attn_dev on a contiguous copy of the same
row bytes: that is the main yardstick and it needs no tolerance.  Independently of the library the same outputs are held to the float64
reference of tests/np_attention.py under its TOL_DECODE / TOL_PROMPT; no new tolerance is introduced.  The stores are held to bytes: the
whole pool downloaded equals a host-built image.
Shapes: a pool of 12 pages filled with 0xFF bytes (F16 NaN halves, Q8_0 d = NaN) except the rows a sequence holds; page assignments
descending and interleaved between the sequences; sequences of lengths {0, 1, 129, 379} in one call; D 64 / 128, heads (4, 2) and (8, 1),
both cache types, both nb_pos / nb_head orders; n_q 1, 3 (DECODE), 9 and 130 (PROMPT: the smallest, and two query tiles)."""
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
NEW_SYMBOLS = ("ggml_hip_kv_store_paged_dev", "ggml_hip_rope_kv_store_paged_dev", "ggml_hip_attn_paged_dev", "ggml_hip_attn_paged_plan",
               "ggml_hip_attn_paged_work_size")
DECODE, PROMPT = 1, 2
PAGE = A.CHUNK
N_PAGES = 12
LENGTHS = (379, 0, 129, 1)                                          # the sequences of the common batch, by slot
TABLE = ((11, 8, 5), (), (10, 7), (9,))                             # their pages: descending, interleaved between the sequences
GARBAGE = -7                                                        # what every unneeded table entry holds


def _p(x):
    return None if x is None else C.c_void_p(int(x))


def _up16(n):
    return (n + 15) // 16 * 16


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    exports = open(os.path.join(ROOT, "ggmlsharp_amd", "csrc", "exports.map")).read()
    assert re.search(r"global:\s*ggml_hip_\*;", exports)
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name


def _plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max):
    out = _lib.ggml_hip_attn_plan_t()
    rc = _lib.lib().ggml_hip_attn_paged_plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, C.byref(out))
    return rc, out


def test_the_paged_plan_is_the_contiguous_plan_with_a_sequence_dimension():
    L = _lib.lib()
    for n_q in (1, 8, 9, 128, 129, 379):
        for kv_type in (F16, Q8_0):
            for D in (64, 128):
                for n_head, n_head_kv in ((4, 2), (8, 1), (32, 8)):
                    for n_kv_max in (0, 1, 128, 129, 5000):
                        one = _lib.ggml_hip_attn_plan_t()
                        assert L.ggml_hip_attn_plan(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, C.byref(one)) == 0
                        for n_seq in (1, 2, 3, 32, 1000, 4096):
                            rc, p = _plan(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max)
                            if n_seq * n_q > (1 << 20):
                                assert rc == _lib.ERR_SHAPE                     # the stated bound on n_seq * n_q
                                continue
                            assert rc == 0
                            assert (p.form, p.chunk, p.q_tile, p.launches, p.n_chunks) == (one.form, one.chunk, one.q_tile, one.launches, one.n_chunks)
                            assert p.form == (DECODE if n_q <= A.DECODE_MAX_Q else PROMPT) and p.chunk == PAGE
                            assert p.workgroups == n_seq * one.workgroups      # workgroups scale with n_seq
    assert _plan(F16, 128, 4, 2, 0, 1, 128)[0] == _lib.ERR_SHAPE and _plan(F16, 128, 4, 2, 4097, 1, 128)[0] == _lib.ERR_SHAPE
    assert _plan(F16, 96, 4, 2, 2, 1, 128)[0] == _lib.ERR_SHAPE and _plan(2, 128, 4, 2, 2, 1, 128)[0] == _lib.ERR_TYPE


def test_the_work_size_is_monotone_and_zero_for_an_empty_batch_and_for_prompt():
    W = _lib.lib().ggml_hip_attn_paged_work_size
    for kv_type in (F16, Q8_0):
        for D in (64, 128):
            last_q = 0
            for n_q in (1, 3, 8):
                last_s = 0
                for n_seq in (1, 2, 16, 4096):
                    last = 0
                    for n_kv_max in (1, 128, 129, 1000, 1001, 40000):
                        w = W(kv_type, D, 8, 2, n_seq, n_q, n_kv_max)
                        assert w >= last and w > 0
                        assert w >= n_seq * n_q * 8 * ((n_kv_max + PAGE - 1) // PAGE) * (D + 4) * 4
                        last = w
                    assert last >= last_s
                    last_s = last
                w = W(kv_type, D, 8, 2, 16, n_q, 1000)
                assert w >= last_q
                last_q = w
            assert W(kv_type, D, 8, 2, 16, 0, 4096) == 0 and W(kv_type, D, 8, 2, 0, 1, 4096) == 0
            assert W(kv_type, D, 8, 2, 16, 9, 4096) == 0 and W(kv_type, D, 8, 2, 4, 512, 4096) == 0      # PROMPT keeps its state in registers


def _geometry(kv_type, D, n_head_kv, layout, slack=0):
    """(nb_page, nb_pos, nb_head) of a page: layout 0 position-major (nb_head < nb_pos), 1 head-major; padding between rows in both"""
    rb = A.row_bytes(kv_type, D)
    if layout == 0:
        nb_head = _up16(rb) + 16
        nb_pos = n_head_kv * nb_head + 32
    else:
        nb_pos = _up16(rb) + 16
        nb_head = PAGE * nb_pos + 48
    span = (PAGE - 1) * nb_pos + (n_head_kv - 1) * nb_head + rb
    return _up16(span) + slack, nb_pos, nb_head


def _attn_rc(kv_type=F16, D=128, n_head=4, n_head_kv=2, n_seq=2, n_q=1, n_kv_max=256, ldq=(512, 128), ldd=(512, 128), nb=None, n_pages=4, ld_pages=2,
             ptr=0x1000, pages=0x1000, d_len=0x1000, mask=None, max_bias=0.0, softcap=0.0, sinks=None, work=0x1000, work_bytes=1 << 30):
    g = _geometry(F16, 128, 2, 0)
    nb = g if nb is None else nb
    return _lib.lib().ggml_hip_attn_paged_dev(kv_type, _p(ptr), ldq[0], ldq[1], _p(ptr), _p(ptr), nb[0], nb[1], nb[2], n_pages, _p(pages), ld_pages, _p(d_len), 1,
                                              n_seq, n_head, n_head_kv, D, n_q, n_kv_max, 1, 0.125, mask, max_bias, softcap, sinks, _p(ptr), ldd[0], ldd[1],
                                              _p(work), work_bytes, None)


def test_what_is_not_served_is_refused_before_anything_is_launched():
    """every call below carries pointers that are not device memory: a launch would fault, a refusal returns its code"""
    E = _lib
    nb_page, nb_pos, nb_head = _geometry(F16, 128, 2, 0)
    for t in (0, 2, 7, 9, _lib.BF16):
        assert _attn_rc(kv_type=t) == E.ERR_TYPE
    assert _attn_rc(D=96) == E.ERR_SHAPE and _attn_rc(D=256) == E.ERR_SHAPE
    assert _attn_rc(n_head=6, n_head_kv=4) == E.ERR_SHAPE and _attn_rc(n_head=34, n_head_kv=2) == E.ERR_SHAPE
    assert _attn_rc(ldq=(514, 128)) == E.ERR_SHAPE and _attn_rc(ldq=(512, 130)) == E.ERR_SHAPE and _attn_rc(ldd=(512, 126)) == E.ERR_SHAPE
    assert _attn_rc(nb=(nb_page, nb_pos + 8, nb_head)) == E.ERR_SHAPE and _attn_rc(nb=(nb_page, nb_pos, 128)) == E.ERR_SHAPE
    assert _attn_rc(nb=(nb_page - 16, nb_pos, nb_head)) == E.ERR_SHAPE          # a page shorter than its rows span
    assert _attn_rc(nb=(nb_page + 8, nb_pos, nb_head)) == E.ERR_SHAPE           # a page that is no multiple of 16
    assert _attn_rc(nb=(PAGE * 256, 256, 256)) == E.ERR_SHAPE                   # two kv heads do not fit rows 256 apart in both directions
    assert _attn_rc(ld_pages=1) == E.ERR_SHAPE and _attn_rc(n_kv_max=257, ld_pages=2) == E.ERR_SHAPE
    assert _attn_rc(d_len=None) == E.ERR_ARG and _attn_rc(pages=None) == E.ERR_ARG
    assert _attn_rc(n_pages=0) == E.ERR_ARG and _attn_rc(n_pages=-3) == E.ERR_ARG
    assert _attn_rc(mask=_p(0x1000)) == E.ERR_ARG and _attn_rc(max_bias=8.0) == E.ERR_ARG and _attn_rc(softcap=30.0) == E.ERR_ARG
    assert _attn_rc(sinks=_p(0x1000)) == E.ERR_ARG
    assert _attn_rc(work=None) == E.ERR_ARG and _attn_rc(work_bytes=64) == E.ERR_ARG
    assert _attn_rc(n_seq=0) == E.ERR_SHAPE and _attn_rc(n_seq=4097) == E.ERR_SHAPE and _attn_rc(n_seq=-1) == E.ERR_SHAPE
    assert _attn_rc(n_seq=4096, n_q=257, ldq=(512, 128)) == E.ERR_SHAPE         # n_seq * n_q above 2^20
    assert _attn_rc(ptr=0x1004) == E.ERR_SHAPE
    assert _attn_rc(n_q=0, work=None) == 0                                      # an empty batch: OK, nothing written
    L = _lib.lib()

    def st(kv_type=F16, D=128, nb=(nb_page, nb_pos, nb_head), ld=(256, 128), n_seq=2, n_pages=4, ld_pages=2, pages=0x1000, d_len=0x1000, src=0x1000, pool=0x1000, rope=False):
        tail = (n_seq, 1) + ((None,) if rope else ()) + (_p(pool), nb[0], nb[1], nb[2], n_pages, _p(pages), ld_pages, _p(d_len), 256, None)
        if rope:
            rp = _lib.ggml_hip_rope_params_t(64, 0, 0, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
            return L.ggml_hip_rope_kv_store_paged_dev(C.byref(rp), kv_type, _p(src), ld[0], ld[1], 2, D, *tail)
        return L.ggml_hip_kv_store_paged_dev(kv_type, _p(src), ld[0], ld[1], 2, D, *tail)

    for rope in (False, True):
        assert st(rope=rope, kv_type=2) == E.ERR_TYPE and st(rope=rope, kv_type=Q8_0, D=48, ld=(96, 48)) == E.ERR_SHAPE
        assert st(rope=rope, ld=(256, 130)) == E.ERR_SHAPE and st(rope=rope, ld=(256, 64)) == E.ERR_SHAPE
        assert st(rope=rope, nb=(nb_page - 16, nb_pos, nb_head)) == E.ERR_SHAPE and st(rope=rope, nb=(nb_page + 4, nb_pos, nb_head)) == E.ERR_SHAPE
        assert st(rope=rope, nb=(nb_page, nb_pos, 250)) == E.ERR_SHAPE and st(rope=rope, ld_pages=1) == E.ERR_SHAPE
        assert st(rope=rope, d_len=None) == E.ERR_ARG and st(rope=rope, pages=None) == E.ERR_ARG and st(rope=rope, n_pages=0) == E.ERR_ARG
        assert st(rope=rope, n_seq=0) == E.ERR_SHAPE and st(rope=rope, n_seq=4097) == E.ERR_SHAPE
        assert st(rope=rope, src=None) == E.ERR_ARG and st(rope=rope, pool=0x1008) == E.ERR_SHAPE


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


_SEQ, _Q, _CONTIG, _REF = {}, {}, {}, {}


def seq_rows(kv_type, D, n_head_kv, tag, n):
    """the cache bytes of a sequence, computed once: (Kraw, Vraw) uint8 [n, n_head_kv, row_bytes], values in [-1, 1]"""
    key = (kv_type, D, n_head_kv, tag, n)
    if key not in _SEQ and n == 0:
        _SEQ[key] = (np.zeros((0, n_head_kv, A.row_bytes(kv_type, D)), np.uint8),) * 2
    if key not in _SEQ:
        rng = np.random.default_rng([kv_type, D, n_head_kv, n] + [ord(c) for c in str(tag)])
        K = rng.uniform(-1, 1, (n, n_head_kv, D)).astype(np.float32)
        V = rng.uniform(-1, 1, (n, n_head_kv, D)).astype(np.float32)
        _SEQ[key] = (A.encode_rows(kv_type, K), A.encode_rows(kv_type, V))
    return _SEQ[key]


def queries(D, n_head, tag, n_q):
    key = (D, n_head, tag, n_q)
    if key not in _Q:
        rng = np.random.default_rng([D, n_head, n_q, 77] + [ord(c) for c in str(tag)])
        _Q[key] = rng.uniform(-1, 1, (n_q, n_head, D)).astype(np.float32)
    return _Q[key]


class Pool:
    """host images of the K and V pools: n_pages pages of 0xFF bytes, rows put where a table says"""

    def __init__(self, kv_type, D, n_head_kv, layout, n_pages=N_PAGES, slack=0):
        self.kv_type, self.D, self.n_head_kv, self.n_pages = kv_type, D, n_head_kv, n_pages
        self.rb = A.row_bytes(kv_type, D)
        self.nb_page, self.nb_pos, self.nb_head = _geometry(kv_type, D, n_head_kv, layout, slack)
        self.host = [np.full(n_pages * self.nb_page, 0xFF, np.uint8), np.full(n_pages * self.nb_page, 0xFF, np.uint8)]

    def offsets(self, page, jj):
        """byte offsets [len(jj), n_head_kv, rb] of the rows (position-in-page jj, every kv head) of a page"""
        return (page * self.nb_page + np.asarray(jj)[:, None, None] * self.nb_pos + np.arange(self.n_head_kv)[None, :, None] * self.nb_head
                + np.arange(self.rb)[None, None, :])

    def put(self, side, pages, raw, n):
        """rows 0 .. n-1 of raw [>= n, n_head_kv, rb] into the pages of a table row (entries outside the pool are skipped)"""
        for c, page in enumerate(pages):
            j0, j1 = c * PAGE, min(n, c * PAGE + PAGE)
            if j1 > j0 and 0 <= page < self.n_pages:
                self.host[side][self.offsets(page, np.arange(j1 - j0))] = raw[j0:j1]

    def cache(self, dev, table, lens, n_kv_max, ld_pages=None, garbage=GARBAGE):
        torch = dev.torch
        ld_pages = max((n_kv_max + PAGE - 1) // PAGE, 1) if ld_pages is None else ld_pages
        tab = np.full((len(table), ld_pages), garbage, np.int32)
        for b, pages in enumerate(table):
            tab[b, :len(pages)] = pages
        return dev.PagedCache(self.kv_type, torch.from_numpy(self.host[0]).cuda(), torch.from_numpy(self.host[1]).cuda(), self.nb_page, self.nb_pos, self.nb_head,
                              self.n_pages, torch.from_numpy(tab).cuda(), torch.tensor(list(lens), dtype=torch.int32, device="cuda"), n_kv_max)


def paged(dev, cfg, tags, lens, table, n_q, causal, n_pages=N_PAGES, ld_pages=None, slack=0, n_kv_max=None, len_bias=0, garbage=GARBAGE, layout=None):
    """one paged call over sequences (tag, length) laid out by `table` -> numpy [n_seq, n_q, n_head, D]"""
    torch = dev.torch
    kv_type, D, n_head, n_head_kv, cfg_layout = cfg
    pool = Pool(kv_type, D, n_head_kv, cfg_layout if layout is None else layout, n_pages, slack)
    for tag, n, pages in zip(tags, lens, table):
        Kraw, Vraw = seq_rows(kv_type, D, n_head_kv, tag, n)
        pool.put(0, pages, Kraw, n)
        pool.put(1, pages, Vraw, n)
    n_kv_max = max(max(lens), 1) if n_kv_max is None else n_kv_max
    pc = pool.cache(dev, table, [n - len_bias for n in lens], n_kv_max, ld_pages, garbage)
    q = torch.from_numpy(np.concatenate([queries(D, n_head, tag, n_q) for tag in tags])).cuda()
    out = dev.attn_paged(pc, q, n_head_kv, len_bias=len_bias, causal=causal)
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(len(tags), n_q, n_head, D)


def contiguous(dev, cfg, tag, n, n_q, causal):
    """ggml_hip_attn_dev for one sequence on a contiguous cache of the same row bytes, computed once -> numpy [n_q, n_head, D]"""
    torch = dev.torch
    kv_type, D, n_head, n_head_kv, _ = cfg
    key = (kv_type, D, n_head, n_head_kv, tag, n, n_q, causal)
    if key not in _CONTIG:
        rb = A.row_bytes(kv_type, D)
        nb_head = _up16(rb)
        nb_pos = n_head_kv * nb_head
        bufs = []
        for raw in seq_rows(kv_type, D, n_head_kv, tag, n):
            buf = np.full((n, n_head_kv, nb_head), 0xFF, np.uint8)
            buf[:, :, :rb] = raw
            bufs.append(torch.from_numpy(buf.reshape(-1)).cuda())
        q = torch.from_numpy(queries(D, n_head, tag, n_q)).cuda()
        out = dev.attention(kv_type, q, bufs[0], bufs[1], nb_pos, nb_head, n_head_kv, n, causal=causal)
        torch.cuda.synchronize()
        _CONTIG[key] = out.cpu().numpy()
    return _CONTIG[key]


def reference(cfg, tag, n, n_q, causal):
    """the float64 reference over the dequantized rows, computed once -> (ref [n_q, n_head, D], Vd)"""
    kv_type, D, n_head, n_head_kv, _ = cfg
    key = (kv_type, D, n_head, n_head_kv, tag, n, n_q, causal)
    if key not in _REF:
        Kraw, Vraw = seq_rows(kv_type, D, n_head_kv, tag, n)
        Kd, Vd = A.decode_rows(kv_type, Kraw, D), A.decode_rows(kv_type, Vraw, D)
        _REF[key] = (A.reference(queries(D, n_head, tag, n_q), Kd, Vd, n, causal, 1.0 / np.sqrt(D)), Vd)
    return _REF[key]


def bits(x):
    return np.ascontiguousarray(x).view(np.uint32)


def expect_sequence(dev, cfg, tag, n, n_q, causal):
    """what a sequence's rows must be, bit for bit: +0.0f for an empty sequence, the contiguous entry otherwise"""
    kv_type, D, n_head, n_head_kv, _ = cfg
    return np.zeros((n_q, n_head, D), np.float32) if n == 0 else contiguous(dev, cfg, tag, n, n_q, causal)


_BATCH = {}


def common_batch(dev, cfg, n_q, causal):
    key = (cfg, n_q, causal)
    if key not in _BATCH:
        _BATCH[key] = paged(dev, cfg, ["s%d" % n for n in LENGTHS], LENGTHS, TABLE, n_q, causal)
    return _BATCH[key]


SWEEP = [(t, D, nh, nhk, layout) for t in (F16, Q8_0) for D in (64, 128) for nh, nhk in ((4, 2), (8, 1)) for layout in (0, 1)]
N_QS = (1, 3, 9, 130)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SWEEP)
def test_every_sequence_equals_the_contiguous_entry_bit_for_bit(dev, cfg):
    for n_q in N_QS:
        rc, p = _plan(cfg[0], cfg[1], cfg[2], cfg[3], len(LENGTHS), n_q, max(LENGTHS))
        assert rc == 0 and p.form == (DECODE if n_q <= A.DECODE_MAX_Q else PROMPT)
        for causal in (True, False):
            got = common_batch(dev, cfg, n_q, causal)
            for b, n in enumerate(LENGTHS):
                want = expect_sequence(dev, cfg, "s%d" % n, n, n_q, causal)
                assert np.array_equal(bits(got[b]), bits(want)), (cfg, n_q, causal, b, n)


@pytest.mark.gpu
@pytest.mark.parametrize("cfg", SWEEP)
def test_every_sequence_is_inside_the_tolerance_of_the_f64_reference(dev, cfg):
    for n_q in N_QS:
        tol = A.TOL_DECODE if n_q <= A.DECODE_MAX_Q else A.TOL_PROMPT
        for causal in (True, False):
            got = common_batch(dev, cfg, n_q, causal)
            assert np.isfinite(got).all()
            for b, n in enumerate(LENGTHS):
                if n == 0:
                    assert np.array_equal(bits(got[b]), np.zeros_like(bits(got[b])))
                    continue
                ref, Vd = reference(cfg, "s%d" % n, n, n_q, causal)
                st = A.statistic(got[b], ref, Vd)
                print(cfg, "n_q", n_q, "causal", causal, "n_kv", n, "statistic", st, "bar", tol)
                assert st <= tol, (cfg, n_q, causal, n, st, tol)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_sequences_bits_do_not_depend_on_the_call_around_it(dev, kv_type):
    cfg = (kv_type, 128, 8, 2, 0)
    tags = ["s%d" % n for n in LENGTHS]
    for n_q in (3, 9):
        base = common_batch(dev, cfg, n_q, True)

        def same(got, what):
            for b in range(len(LENGTHS)):
                assert np.array_equal(bits(got[b]), bits(base[b])), (what, "sequence", b, "n_q", n_q)

        same(paged(dev, cfg, tags, LENGTHS, ((0, 1, 2), (), (3, 4), (5,)), n_q, True), "the page assignment")
        same(paged(dev, cfg, tags, LENGTHS, ((16, 8, 5), (), (10, 13), (0,)), n_q, True, n_pages=17), "n_pages")
        same(paged(dev, cfg, tags, LENGTHS, TABLE, n_q, True, ld_pages=7), "ld_pages")
        same(paged(dev, cfg, tags, LENGTHS, TABLE, n_q, True, slack=80), "nb_page")
        same(paged(dev, cfg, tags, LENGTHS, TABLE, n_q, True, layout=1), "the order of nb_pos and nb_head")
        same(paged(dev, cfg, tags, LENGTHS, TABLE, n_q, True, n_kv_max=max(LENGTHS) + 700), "n_kv_max")
        same(paged(dev, cfg, tags, LENGTHS, TABLE, n_q, True, len_bias=5), "len_bias against a shifted d_len")
        for b, n in enumerate(LENGTHS):                              # alone, and in another slot of the reversed batch
            alone = paged(dev, cfg, [tags[b]], [n], [TABLE[b]], n_q, True)
            assert np.array_equal(bits(alone[0]), bits(base[b])), ("n_seq", b, n_q)
        rev = paged(dev, cfg, tags[::-1], LENGTHS[::-1], TABLE[::-1], n_q, True)
        same(rev[::-1], "the slot")


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_shared_prefix_page_gives_the_bits_of_private_copies(dev, kv_type):
    torch = dev.torch
    cfg = (kv_type, 128, 4, 2, 1)
    _, D, n_head, n_head_kv, layout = cfg
    lens = (129, 200)
    rows = [list(seq_rows(kv_type, D, n_head_kv, "p%d" % n, n)) for n in lens]
    for side in (0, 1):                                             # the second sequence starts with the first one's first page
        rows[1][side] = rows[1][side].copy()
        rows[1][side][:PAGE] = rows[0][side][:PAGE]
    for n_q in (3, 9):
        outs = []
        for table in (((6, 2), (6, 9)), ((6, 2), (4, 9))):
            pool = Pool(kv_type, D, n_head_kv, layout)
            for (Kraw, Vraw), n, pages in zip(rows, lens, table):
                pool.put(0, pages, Kraw, n)
                pool.put(1, pages, Vraw, n)
            pc = pool.cache(dev, table, lens, max(lens))
            q = torch.from_numpy(np.concatenate([queries(D, n_head, "p%d" % n, n_q) for n in lens])).cuda()
            outs.append(dev.attn_paged(pc, q, n_head_kv).cpu().numpy())
        assert np.array_equal(bits(outs[0]), bits(outs[1])), (kv_type, n_q)
        assert np.isfinite(outs[0]).all() and np.abs(outs[0]).max() > 0


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_an_invalid_needed_page_id_zeroes_its_sequence_and_no_other(dev, kv_type):
    cfg = (kv_type, 64, 4, 2, 0)
    tags = ["s%d" % n for n in LENGTHS]
    for n_q in (3, 9, 130):
        base = common_batch(dev, cfg, n_q, True)
        for bad in (-1, N_PAGES, 1 << 30, -(1 << 31)):
            for where in (0, 1, 2):
                row = list(TABLE[0])
                row[where] = bad
                got = paged(dev, cfg, tags, LENGTHS, (tuple(row),) + TABLE[1:], n_q, True)
                assert np.array_equal(bits(got[0]), np.zeros_like(bits(got[0]))), (n_q, bad, where)
                for b in (1, 2, 3):
                    assert np.array_equal(bits(got[b]), bits(base[b])), (n_q, bad, where, b)
        for garbage in (0, N_PAGES, 1 << 30, -1):                   # what the unneeded entries hold changes nothing
            got = paged(dev, cfg, tags, LENGTHS, TABLE, n_q, True, ld_pages=5, garbage=garbage)
            assert np.array_equal(bits(got), bits(base)), (n_q, garbage)


def _store_rows(dev, kv_type, x):
    """the bytes ggml_hip_kv_store_dev writes for the f32 rows x [..., D] -> uint8 [..., row_bytes]"""
    torch = dev.torch
    D = x.shape[-1]
    rb = A.row_bytes(kv_type, D)
    flat = np.ascontiguousarray(x.reshape(-1, D))
    nb = _up16(rb)
    cache = torch.zeros(flat.shape[0] * nb, dtype=torch.uint8, device="cuda")
    dev.kv_store(kv_type, torch.from_numpy(flat).cuda(), cache, nb, flat.shape[0])
    torch.cuda.synchronize()
    got = cache.cpu().numpy().reshape(flat.shape[0], nb)[:, :rb]
    assert np.array_equal(got, A.encode_rows(kv_type, flat))
    return got.reshape(x.shape[:-1] + (rb,))


def _store_image(pool, side, want, lens, table, n_kv_max):
    """the pool after a paged store of want [n_seq, n_q, n_head_kv, rb]: a token outside [0, n_kv_max) or on a page outside the pool writes nothing"""
    img = pool.host[side].copy()
    for b, (n, pages) in enumerate(zip(lens, table)):
        for t in range(want.shape[1]):
            pos = n + t
            if not 0 <= pos < n_kv_max:
                continue
            page = pages[pos // PAGE]
            if 0 <= page < pool.n_pages:
                img[pool.offsets(page, [pos % PAGE])] = want[b, t][None]
    return img


@pytest.mark.gpu
@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_the_paged_store_writes_kv_stores_bytes_and_nothing_else(dev, kv_type, layout):
    torch = dev.torch
    rng = np.random.default_rng(11)
    n_q = 3
    full = ((11, 8, 5), (3, GARBAGE, GARBAGE), (10, 7, GARBAGE), (9, GARBAGE, GARBAGE))
    for D, n_head_kv in ((64, 2), (128, 1), (128, 3)):
        x = rng.uniform(-1, 1, (len(LENGTHS), n_q, n_head_kv, D)).astype(np.float32)
        x[0, 0, 0, :8] = [6.0e-8, -6.0e-8, 65520.0, -1.0e6, 0.0, -0.0, 65504.0, 2.98e-8]      # subnormals, overflow to inf, both zeros, the f16 maximum
        x[2, 1, 0, 32:64] = 0.0                                                               # an all-zero Q8_0 block
        want = _store_rows(dev, kv_type, x)
        xs = torch.zeros((len(LENGTHS) * n_q, n_head_kv, D + 4), device="cuda")              # padded strides
        xs[:, :, :D] = torch.from_numpy(x.reshape(-1, n_head_kv, D)).cuda()
        cases = [(full, 384), (full, 381), (full, 130), (full, 2),                            # every token inside; tokens past n_kv_max dropped
                 (((11, 8, -1),) + full[1:], 384), (((11, 8, N_PAGES),) + full[1:], 384), (full[:2] + ((10, 1 << 30, 0),) + full[3:], 384)]
        for table, n_kv_max in cases:
            pool = Pool(kv_type, D, n_head_kv, layout)
            for side in (0, 1):
                pool.host[side][:] = rng.integers(0, 256, pool.host[side].size, dtype=np.uint8)
            pc = pool.cache(dev, table, LENGTHS, n_kv_max, ld_pages=3)
            dev.kv_store_paged(pc, xs[:, :, :D], pc.k)
            torch.cuda.synchronize()
            assert np.array_equal(pc.k.cpu().numpy(), _store_image(pool, 0, want, LENGTHS, table, n_kv_max)), (kv_type, layout, D, n_head_kv, table, n_kv_max)
            assert np.array_equal(pc.v.cpu().numpy(), pool.host[1])
        # lengths on the device that are out of range: only the first sequence's last token (position -2 + 2 = 0) is written
        wild = (-2, 384, 1 << 30, -(1 << 31))
        pool = Pool(kv_type, D, n_head_kv, layout)
        pc = pool.cache(dev, full, wild, 384, ld_pages=3)
        dev.kv_store_paged(pc, xs[:, :, :D], pc.k)
        torch.cuda.synchronize()
        img = _store_image(pool, 0, want, wild, full, 384)
        assert np.array_equal(pc.k.cpu().numpy(), img) and int((img != pool.host[0]).sum()) > 0


@pytest.mark.gpu
@pytest.mark.parametrize("mode", [0, 2])
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_the_fused_store_is_rope_then_the_paged_store_byte_for_byte(dev, kv_type, mode):
    torch = dev.torch
    rng = np.random.default_rng(13)
    n_q, lens = 4, (126, 0, 379, 254)                               # tokens on both sides of a page boundary: 126 .. 129 and 254 .. 257
    table = ((11, 8, 5), (3, GARBAGE, GARBAGE), (10, 7, 2), (9, 6, 4))
    for D, n_head_kv, n_dims, layout in ((64, 2, 64, 0), (128, 2, 128, 1), (128, 1, 64, 0), (64, 1, 30, 1)):
        rp = dev.rope_params(n_dims, mode=mode, freq_base=10000.0)
        x = torch.from_numpy(rng.uniform(-1, 1, (len(lens) * n_q, n_head_kv, D)).astype(np.float32)).cuda()
        pos = torch.tensor([n + t for n in lens for t in range(n_q)], dtype=torch.int32, device="cuda")
        pool = Pool(kv_type, D, n_head_kv, layout)
        two = pool.cache(dev, table, lens, 384, ld_pages=3)
        fused = pool.cache(dev, table, lens, 384, ld_pages=3)
        dev.kv_store_paged(two, dev.rope(rp, x, pos=pos), two.k)
        dev.rope_kv_store_paged(rp, fused, x, fused.k)
        torch.cuda.synchronize()
        assert torch.equal(two.k, fused.k), (kv_type, mode, D, n_head_kv, n_dims)
        assert int((fused.k.cpu() != torch.from_numpy(pool.host[0])).sum()) > 0 and torch.equal(fused.v.cpu(), torch.from_numpy(pool.host[1]))
        # a position past n_kv_max and an invalid page write nothing in the fused form either
        cut = pool.cache(dev, ((11, 8, -1), (3, 0, 0), (10, 7, 2), (9, N_PAGES, 4)), lens, 381, ld_pages=3)
        ref = pool.cache(dev, ((11, 8, -1), (3, 0, 0), (10, 7, 2), (9, N_PAGES, 4)), lens, 381, ld_pages=3)
        dev.kv_store_paged(ref, dev.rope(rp, x, pos=pos), ref.k)
        dev.rope_kv_store_paged(rp, cut, x, cut.k)
        torch.cuda.synchronize()
        assert torch.equal(ref.k, cut.k)


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_captured_batched_decode_step_follows_three_sequences_across_a_page_boundary(dev, kv_type):
    """rope(q, d_pos = d_len) -> rope_kv_store_paged(k) -> kv_store_paged(v) -> attn_paged(len_bias = 1), captured ONCE for three sequences and
    replayed three times with d_len + 1 in between; one sequence steps 127 -> 128 -> 129 onto its next page, which the table already names.
    Every replay equals the uncaptured contiguous calls of each sequence bit for bit."""
    torch = dev.torch
    D, n_head, n_head_kv, n_seq, n_max = 128, 8, 2, 3, 3 * PAGE
    start = (127, 5, 300)
    table = ((4, 2, GARBAGE), (7, GARBAGE, GARBAGE), (9, 1, 6))
    rp = dev.rope_params(D, mode=2)
    rb = A.row_bytes(kv_type, D)
    rng = np.random.default_rng(21)
    hist = [rng.uniform(-1, 1, (2, n, n_head_kv, D)).astype(np.float32) for n in start]
    pool = Pool(kv_type, D, n_head_kv, 0)
    for h, n, pages in zip(hist, start, table):
        pool.put(0, pages, A.encode_rows(kv_type, h[0]), n)
        pool.put(1, pages, A.encode_rows(kv_type, h[1]), n)
    pc = pool.cache(dev, table, start, n_max)
    warm = pool.cache(dev, table, start, n_max)
    c_nb_head, c_nb_pos = rb, n_head_kv * rb                         # the contiguous caches of the fresh calls: heads back to back
    fresh_kv = []
    for h, n in zip(hist, start):
        bufs = []
        for side in (0, 1):
            buf = torch.full((n_max * c_nb_pos,), 0xFF, dtype=torch.uint8, device="cuda")
            buf[:n * c_nb_pos] = torch.from_numpy(A.encode_rows(kv_type, h[side]).reshape(-1)).cuda()
            bufs.append(buf)
        fresh_kv.append(bufs)
    q = torch.zeros((n_seq, n_head, D), device="cuda")
    k_new = torch.zeros((n_seq, n_head_kv, D), device="cuda")
    v_new = torch.zeros((n_seq, n_head_kv, D), device="cuda")
    q_rot = torch.zeros_like(q)
    out = torch.zeros_like(q)
    work = torch.empty(dev.attn_paged_work_size(kv_type, D, n_head, n_head_kv, n_seq, 1, n_max), dtype=torch.uint8, device="cuda")

    def step(cache, o):
        dev.rope(rp, q, pos=cache.d_len, out=q_rot)
        dev.rope_kv_store_paged(rp, cache, k_new, cache.k)
        dev.kv_store_paged(cache, v_new, cache.v)
        dev.attn_paged(cache, q_rot, n_head_kv, len_bias=1, out=o, work=work)

    step(warm, torch.zeros_like(out))                                # (a first call outside the capture, on copies: one-time kernel attributes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(pc, out)
    torch.cuda.current_stream().wait_stream(s)
    for i in range(3):
        for t in (q, k_new, v_new):
            t.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(t.shape)).astype(np.float32)))
        g.replay()
        torch.cuda.synchronize()
        for b in range(n_seq):
            pos = start[b] + i
            kc, vc = fresh_kv[b]
            qb = dev.rope(rp, q[b:b + 1], pos0=pos)
            dev.rope_kv_store(rp, kv_type, k_new[b:b + 1], kc, c_nb_pos, c_nb_head, n_max, pos0=pos)
            dev.kv_store(kv_type, v_new[b:b + 1].reshape(1, n_head_kv * D), vc, c_nb_pos, n_max, pos0=pos)
            fresh = dev.attention(kv_type, qb, kc, vc, c_nb_pos, c_nb_head, n_head_kv, pos + 1, n_kv_max=n_max)
            torch.cuda.synchronize()
            assert torch.equal(out[b:b + 1], fresh), (kv_type, i, b)
        assert bool(torch.isfinite(out).all()) and float(out.abs().max()) > 0
        pc.d_len.add_(1)                                             # the host's part of the step
    torch.cuda.synchronize()
    assert pc.d_len.cpu().tolist() == [n + 3 for n in start]


@pytest.mark.gpu
def test_sixteen_sequences_behind_the_batched_projections(dev):
    """n_q = 1 for 16 sequences: hidden 1024, 8 heads of 128 over 2 kv heads, Q8_0 weights and a Q8_0 cache; q / k / v from ONE
    mul_mat_multi_work_dev call at 16 rows (mul_mat_multi_dev's form for a batch) -> two paged stores -> one paged attention.  Finite, inside TOL_DECODE of the f64 reference, and equal to the
    16 single-sequence calls on contiguous caches."""
    torch = dev.torch
    L, check = _lib.lib(), _lib.check
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    H, n_head, n_head_kv, D, n_seq = 1024, 8, 2, 128, 16
    lens = [(53 * i) % 300 for i in range(n_seq)]                    # 0 .. 299, one empty, several across a page boundary
    lens[5] = 127
    lens[9] = 128
    n_max = 3 * PAGE
    rng = np.random.default_rng(31)
    mk = lambda M, K: dev.Weight.from_host(Q8_0, O.quantize_row(Q8_0, (rng.standard_normal((M, K)) / np.sqrt(K)).astype(np.float32)), K)
    Wq, Wk, Wv = mk(n_head * D, H), mk(n_head_kv * D, H), mk(n_head_kv * D, H)
    rb = A.row_bytes(Q8_0, D)
    n_pages = 3 * n_seq
    perm = rng.permutation(n_pages)
    table = [tuple(int(p) for p in perm[3 * b:3 * b + 3]) for b in range(n_seq)]
    enc = lambda n: A.encode_rows(Q8_0, rng.uniform(-1, 1, (n, n_head_kv, D)).astype(np.float32)) if n else np.zeros((0, n_head_kv, rb), np.uint8)
    hist = [(enc(n), enc(n)) for n in lens]
    pool = Pool(Q8_0, D, n_head_kv, 0, n_pages=n_pages)
    for (Kraw, Vraw), n, pages in zip(hist, lens, table):
        pool.put(0, pages, Kraw, n)
        pool.put(1, pages, Vraw, n)
    pc = pool.cache(dev, table, lens, n_max)
    x = torch.from_numpy(rng.uniform(-1, 1, (n_seq, H)).astype(np.float32)).cuda()
    qkv = [torch.empty((n_seq, w.M), device="cuda") for w in (Wq, Wk, Wv)]
    hw = (C.c_void_p * 3)(Wq.handle, Wk.handle, Wv.handle)
    dp = (C.c_void_p * 3)(*[o.data_ptr() for o in qkv])
    ld = (C.c_int64 * 3)(*[o.stride(0) for o in qkv])
    mm_work = dev.alloc_work(Q8_0, H, n_seq)
    check(L.ggml_hip_mul_mat_multi_work_dev(hw, 3, _p(x.data_ptr()), H, n_seq, dp, ld, _p(mm_work.data_ptr()), mm_work.numel(), st), "q / k / v at 16 rows")
    q3, k3, v3 = qkv[0].view(n_seq, n_head, D), qkv[1].view(n_seq, n_head_kv, D), qkv[2].view(n_seq, n_head_kv, D)
    dev.kv_store_paged(pc, k3, pc.k)
    dev.kv_store_paged(pc, v3, pc.v)
    att = dev.attn_paged(pc, q3, n_head_kv, len_bias=1)
    torch.cuda.synchronize()
    got = att.cpu().numpy()
    assert np.isfinite(got).all()
    new_k, new_v = dev.quantize_rows(Q8_0, qkv[1]).cpu().numpy().reshape(n_seq, n_head_kv, rb), dev.quantize_rows(Q8_0, qkv[2]).cpu().numpy().reshape(n_seq, n_head_kv, rb)
    qh = qkv[0].cpu().numpy().reshape(n_seq, n_head, D)
    worst = 0.0
    for b, n in enumerate(lens):
        Kraw = np.concatenate([hist[b][0], new_k[b:b + 1]])
        Vraw = np.concatenate([hist[b][1], new_v[b:b + 1]])
        kc, vc = torch.from_numpy(Kraw.reshape(-1)).cuda(), torch.from_numpy(Vraw.reshape(-1)).cuda()
        single = dev.attention(Q8_0, q3[b:b + 1], kc, vc, n_head_kv * rb, rb, n_head_kv, n + 1)
        assert np.array_equal(bits(single.cpu().numpy()), bits(got[b:b + 1])), (b, n)
        Vd = A.decode_rows(Q8_0, Vraw, D)
        worst = max(worst, A.statistic(got[b:b + 1], A.reference(qh[b:b + 1], A.decode_rows(Q8_0, Kraw, D), Vd, n + 1, True, 1.0 / np.sqrt(D)), Vd))
    print("16 sequences: worst statistic", worst, "bar", A.TOL_DECODE)
    assert worst <= A.TOL_DECODE
    for w in (Wq, Wk, Wv):
        w.free()
