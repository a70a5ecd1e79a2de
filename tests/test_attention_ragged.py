"""Ragged paged attention and KV stores: a query count per sequence, read on the device (include/ggml_hip_ext.h, RAGGED PAGED ATTENTION:
ggml_hip_ragged_positions_dev, ggml_hip_kv_store_paged_ragged_dev, ggml_hip_rope_kv_store_paged_ragged_dev, ggml_hip_attn_paged_ragged_dev,
ggml_hip_attn_paged_ragged_plan, ggml_hip_attn_paged_ragged_work_size; csrc/attn.hip, rope.hip, attn.cpp, rope.cpp, plan.cpp plan_attn_ragged).

Yardstick.  The ragged kernels run the paged chunk bodies with each sequence's own n_q, so every sequence of a ragged call is BIT FOR BIT the
uniform paged entry called for it alone (n_seq = 1, n_q = n_q[b], the same table row, d_len[b], len_bias = n_q[b]); the stores write the
uniform stores' bytes.  No tolerance appears anywhere: every comparison is array_equal on bytes.  The uniform entries themselves are held to the
contiguous entry and to the float64 reference by tests/test_attention_paged.py and tests/test_attention_ex.py.
Shapes: D 64 / 128, F16 / Q8_0, heads (4, 2) and (8, 1), a pool of 16 pages in a shuffled assignment with sequences 0 and 6 sharing their first
page, n_kv_max 512, ONE batch of 8 sequences (BATCH below) that reaches an idle slot, DECODE at 1, 2, 3 and 8 rows (the 8 across a chunk edge),
the smallest PROMPT, a PROMPT of two tiles, and a sequence with an invalid needed page id."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import np_attention as A
import test_attention_paged as P                                     # Pool, _geometry, seq_rows, queries, bits: the page pool of the paged tests
from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F16, Q8_0 = A.F16, A.Q8_0
PAGE = A.CHUNK
NEW_SYMBOLS = ("ggml_hip_ragged_positions_dev", "ggml_hip_kv_store_paged_ragged_dev", "ggml_hip_rope_kv_store_paged_ragged_dev",
               "ggml_hip_attn_paged_ragged_dev", "ggml_hip_attn_paged_ragged_plan", "ggml_hip_attn_paged_ragged_work_size")
_p, bits = P._p, P.bits

# the batch: (n_q[b], d_len[b]) by slot; n_kv[b] = d_len[b] + n_q[b] (add_q = 1, len_bias = 0: behind a store)
BATCH = ((1, 200), (0, 50), (3, 0), (8, 125), (9, 119), (140, 0), (2, 383), (1, 0))
N_Q = tuple(n for n, _ in BATCH)
D_LEN = tuple(l for _, l in BATCH)
N_KV_MAX = 512
N_PAGES = 16
INVALID = 1 << 20                                                   # the page id sequence 7 needs and does not have
# shuffled pages; sequences 0 and 6 share page 13 (their first 128 positions); what a sequence does not need holds P.GARBAGE
TABLE = ((13, 4), (9,), (15,), (2, 11), (6,), (0, 8), (13, 3, 10, 7), (INVALID,))
N_TOKENS_MAX = sum(N_Q) + 6                                         # 164 rows in use, 6 beyond d_q_start[n_seq]
POISON = np.float32(-777.25)
OPTS = dict(window=200, softcap=30.0)                               # c_lo = (384 - 200) // 128 = 1 for sequence 6; the sinks are made per n_head


def q_start_of(n_qs):
    return np.concatenate([[0], np.cumsum(n_qs)]).astype(np.int32)


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


def _plan(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, window=0):
    out = _lib.ggml_hip_attn_ragged_plan_t()
    opts = _lib.ggml_hip_attn_opts_t(None, window, 0.0, 0)
    rc = _lib.lib().ggml_hip_attn_paged_ragged_plan(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, C.byref(opts), C.byref(out))
    return rc, out


def _most_tiles(n_max, s_max):
    """best[s][n]: the most PROMPT tiles s sequences can hold in n packed rows, by trying every row count for every sequence in turn: a sequence
    of k >= 9 rows has ceil(k / 128) tiles, any other (idle, DECODE, not present) has none"""
    tiles = np.array([(k + 127) // 128 if k >= 9 else 0 for k in range(n_max + 1)])
    best = [np.zeros(n_max + 1, np.int64)]
    for _ in range(s_max):
        prev = best[-1]
        best.append(np.array([max(tiles[k] + prev[n - k] for k in range(n + 1)) for n in range(n_max + 1)]))
    return best


def test_the_plan_is_four_launches_sized_by_the_bounds_alone():
    brute = _most_tiles(300, 4)
    for n_seq in (1, 2, 3, 4):
        for n in range(0, 301):
            rc, p = _plan(F16, 128, 4, 2, n_seq, n, min(n, 8 * n_seq), 512)
            assert rc == 0 and p.max_tiles == brute[n_seq][n], (n_seq, n, p.max_tiles, brute[n_seq][n])
    for kv_type in (F16, Q8_0):
        for D in (64, 128):
            for n_head, n_head_kv in ((4, 2), (8, 1), (32, 8)):
                for n_seq, n_tok in ((1, 9), (8, 170), (64, 2108), (4096, 1 << 20)):
                    n_dec = min(n_tok, 8 * n_seq)
                    for n_kv_max in (1, 128, 129, 512, 5000):
                        rc, p = _plan(kv_type, D, n_head, n_head_kv, n_seq, n_tok, n_dec, n_kv_max)
                        assert rc == 0 and (p.chunk, p.launches) == (PAGE, 4)
                        nc = (n_kv_max + PAGE - 1) // PAGE
                        P_, L_ = min(n_seq, n_tok // 9), n_tok - 9 * min(n_seq, n_tok // 9)
                        k_ = min(P_, L_ // 120)
                        assert p.n_chunks == nc and p.max_tiles == P_ + k_ + (L_ - 120 * k_) // 128
                        assert (p.decode_workgroups, p.merge_workgroups, p.prompt_workgroups) == (nc * n_head_kv * n_seq, n_dec * n_head, p.max_tiles * n_head)
                        assert p.index_bytes % 256 == 0 and p.index_bytes >= 16 * n_seq + 16 + 8 * p.max_tiles + 8 * n_dec
                        for W in (1, 100, 121, 122, 250, n_kv_max, n_kv_max + 1):     # the windowed chunk count is the _ex bound at 8 rows
                            rc, pw = _plan(kv_type, D, n_head, n_head_kv, n_seq, n_tok, n_dec, n_kv_max, window=W)
                            want = min(nc, (W + 7 + PAGE - 1) // PAGE + 1) if W < n_kv_max else nc
                            assert rc == 0 and pw.n_chunks == want and pw.decode_workgroups == want * n_head_kv * n_seq, (W, n_kv_max)
                            assert (pw.max_tiles, pw.merge_workgroups, pw.index_bytes) == (p.max_tiles, p.merge_workgroups, p.index_bytes)
    rc, p = _plan(F16, 128, 4, 2, 8, 0, 0, 512)
    assert rc == 0 and p.launches == 0 and p.chunk == PAGE          # an empty batch: nothing is launched
    rc, p = _plan(F16, 128, 4, 2, 8, 8, 0, 512)                     # bounds that leave a grid empty: that launch is not made
    assert rc == 0 and (p.launches, p.decode_workgroups, p.merge_workgroups, p.prompt_workgroups) == (1, 0, 0, 0)
    E = _lib
    assert _plan(2, 128, 4, 2, 8, 170, 64, 512)[0] == E.ERR_TYPE and _plan(F16, 96, 4, 2, 8, 170, 64, 512)[0] == E.ERR_SHAPE
    assert _plan(F16, 128, 4, 2, 0, 170, 64, 512)[0] == E.ERR_SHAPE and _plan(F16, 128, 4, 2, 4097, 170, 64, 512)[0] == E.ERR_SHAPE
    assert _plan(F16, 128, 4, 2, 8, -1, 0, 512)[0] == E.ERR_ARG and _plan(F16, 128, 4, 2, 8, (1 << 20) + 1, 64, 512)[0] == E.ERR_SHAPE
    assert _plan(F16, 128, 4096, 512, 8, 1 << 20, 64, 512)[0] == E.ERR_SHAPE            # n_tokens_max * n_head at 2^32
    assert _plan(F16, 128, 4, 2, 8, 170, 171, 512)[0] == E.ERR_ARG and _plan(F16, 128, 4, 2, 8, 170, -1, 512)[0] == E.ERR_ARG
    assert _plan(F16, 128, 4, 2, 8, 170, 64, 512, window=-1)[0] == E.ERR_ARG


def test_the_work_size_is_sized_by_the_decode_bound_and_monotone_in_every_bound():
    W = _lib.lib().ggml_hip_attn_paged_ragged_work_size
    for kv_type in (F16, Q8_0):
        for D in (64, 128):
            for n_head in (8, 32):
                rc, p = _plan(kv_type, D, n_head, 2, 64, 2108, 64, 4096)
                w = W(kv_type, D, n_head, 2, 64, 2108, 64, 4096)
                floats = 64 * n_head * 32 * (D + 4)
                assert rc == 0 and p.index_bytes + 4 * floats <= w <= p.index_bytes + 4 * floats + 512      # (the tables, the partials, alignment)
                assert w < 2108 * n_head * 32 * (D + 4) * 4 // 8                                   # a 2048-token prefill pays no partials
            last = 0
            for n_seq in (1, 2, 16, 64, 4096):
                w = W(kv_type, D, 8, 2, n_seq, 4096, 8, 1000)
                assert w >= last and w > 0
                last = w
            assert last > W(kv_type, D, 8, 2, 1, 4096, 8, 1000)
            last = 0
            for n_tok in (8, 9, 128, 129, 1000, 1 << 20):
                w = W(kv_type, D, 8, 2, 16, n_tok, 8, 1000)
                assert w >= last and w > 0
                last = w
            last = 0
            for n_dec in (0, 1, 8, 100, 128):
                w = W(kv_type, D, 8, 2, 16, 128, n_dec, 1000)
                assert w > last
                last = w
            last = 0
            for n_kv_max in (0, 1, 128, 129, 1000, 1001, 40000):
                w = W(kv_type, D, 8, 2, 16, 128, 128, n_kv_max)
                assert w >= last and w > 0
                last = w
            assert W(kv_type, D, 8, 2, 16, 0, 0, 4096) == 0 and W(kv_type, D, 8, 2, 0, 128, 8, 4096) == 0 and W(kv_type, D, 8, 2, 16, 128, 129, 4096) == 0


def _attn_rc(kv_type=F16, D=128, n_head=4, n_head_kv=2, n_seq=2, n_tokens_max=16, n_dec_rows_max=16, n_kv_max=256, ldq=(512, 128), ldd=(512, 128), nb=None,
             n_pages=4, ld_pages=2, ptr=0x1000, pages=0x1000, d_len=0x1000, q_start=0x1000, opts=None, causal=1, work=0x1000, work_bytes=1 << 30):
    g = P._geometry(F16, 128, 2, 0)
    nb = g if nb is None else nb
    return _lib.lib().ggml_hip_attn_paged_ragged_dev(kv_type, _p(ptr), ldq[0], ldq[1], _p(ptr), _p(ptr), nb[0], nb[1], nb[2], n_pages, _p(pages), ld_pages,
                                                     _p(d_len), 1, 0, n_seq, _p(q_start), n_tokens_max, n_dec_rows_max, n_head, n_head_kv, D, n_kv_max, causal,
                                                     0.125, None if opts is None else C.byref(opts), _p(ptr), ldd[0], ldd[1], _p(work), work_bytes, None)


def test_what_is_not_served_is_refused_before_anything_is_launched():
    """every call below carries pointers that are not device memory: a launch would fault, a refusal returns its code"""
    E = _lib
    L = _lib.lib()
    nb_page, nb_pos, nb_head = P._geometry(F16, 128, 2, 0)
    # ---- the new refusals
    assert _attn_rc(q_start=None) == E.ERR_ARG and _attn_rc(q_start=0x1002) == E.ERR_SHAPE
    assert _attn_rc(n_tokens_max=-1, n_dec_rows_max=0) == E.ERR_ARG and _attn_rc(n_tokens_max=(1 << 20) + 1) == E.ERR_SHAPE
    assert _attn_rc(n_tokens_max=1 << 20, n_head=4096, n_head_kv=512) == E.ERR_SHAPE     # n_tokens_max * n_head at 2^32
    assert _attn_rc(n_dec_rows_max=17) == E.ERR_ARG and _attn_rc(n_dec_rows_max=-1) == E.ERR_ARG
    assert _attn_rc(work=None) == E.ERR_ARG and _attn_rc(work_bytes=64) == E.ERR_ARG
    need = L.ggml_hip_attn_paged_ragged_work_size(F16, 128, 4, 2, 2, 16, 16, 256)
    assert need > 0 and _attn_rc(work_bytes=need - 1) == E.ERR_ARG
    assert _attn_rc(n_tokens_max=0, n_dec_rows_max=0, work=None) == 0                   # an empty batch: OK, nothing written
    # ---- the paged entries' refusals carry over
    for t in (0, 2, 7, 9, _lib.BF16):
        assert _attn_rc(kv_type=t) == E.ERR_TYPE
    assert _attn_rc(D=96) == E.ERR_SHAPE and _attn_rc(D=256) == E.ERR_SHAPE
    assert _attn_rc(n_head=6, n_head_kv=4) == E.ERR_SHAPE and _attn_rc(n_head=34, n_head_kv=2) == E.ERR_SHAPE
    assert _attn_rc(ldq=(514, 128)) == E.ERR_SHAPE and _attn_rc(ldq=(512, 130)) == E.ERR_SHAPE and _attn_rc(ldd=(512, 126)) == E.ERR_SHAPE
    assert _attn_rc(nb=(nb_page, nb_pos + 8, nb_head)) == E.ERR_SHAPE and _attn_rc(nb=(nb_page, nb_pos, 128)) == E.ERR_SHAPE
    assert _attn_rc(nb=(nb_page - 16, nb_pos, nb_head)) == E.ERR_SHAPE and _attn_rc(nb=(nb_page + 8, nb_pos, nb_head)) == E.ERR_SHAPE
    assert _attn_rc(ld_pages=1) == E.ERR_SHAPE and _attn_rc(n_kv_max=257, ld_pages=2) == E.ERR_SHAPE
    assert _attn_rc(d_len=None) == E.ERR_ARG and _attn_rc(pages=None) == E.ERR_ARG
    assert _attn_rc(n_pages=0) == E.ERR_ARG and _attn_rc(n_pages=-3) == E.ERR_ARG
    assert _attn_rc(n_seq=0) == E.ERR_SHAPE and _attn_rc(n_seq=4097) == E.ERR_SHAPE and _attn_rc(n_seq=-1) == E.ERR_SHAPE
    assert _attn_rc(ptr=0x1004) == E.ERR_SHAPE and _attn_rc(ptr=None) == E.ERR_ARG
    # ---- the option rules
    O = _lib.ggml_hip_attn_opts_t
    assert _attn_rc(opts=O(None, -1, 0.0, 0)) == E.ERR_ARG and _attn_rc(opts=O(None, 64, 0.0, 0), causal=0) == E.ERR_ARG
    assert _attn_rc(opts=O(None, 0, -1.0, 0)) == E.ERR_ARG and _attn_rc(opts=O(None, 0, float("inf"), 0)) == E.ERR_ARG
    assert _attn_rc(opts=O(0x1002, 0, 0.0, 0)) == E.ERR_ARG and _attn_rc(opts=O(None, 0, 0.0, 1)) == E.ERR_ARG

    def st(kv_type=F16, D=128, nb=(nb_page, nb_pos, nb_head), ld=(256, 128), n_seq=2, n_tokens_max=16, n_pages=4, ld_pages=2, pages=0x1000, d_len=0x1000,
           q_start=0x1000, src=0x1000, pool=0x1000, rope=False):
        tail = (_p(pool), nb[0], nb[1], nb[2], n_pages, _p(pages), ld_pages, _p(d_len), 256, None)
        if rope:
            rp = _lib.ggml_hip_rope_params_t(64, 0, 0, 10000.0, 1.0, 0.0, 1.0, 32.0, 1.0)
            return L.ggml_hip_rope_kv_store_paged_ragged_dev(C.byref(rp), kv_type, _p(src), ld[0], ld[1], 2, D, n_seq, _p(q_start), n_tokens_max, None, *tail)
        return L.ggml_hip_kv_store_paged_ragged_dev(kv_type, _p(src), ld[0], ld[1], 2, D, n_seq, _p(q_start), n_tokens_max, *tail)

    for rope in (False, True):
        assert st(rope=rope, q_start=None) == E.ERR_ARG and st(rope=rope, q_start=0x1001) == E.ERR_SHAPE
        assert st(rope=rope, n_tokens_max=-1) == E.ERR_ARG and st(rope=rope, n_tokens_max=(1 << 20) + 1) == E.ERR_SHAPE
        assert st(rope=rope, n_tokens_max=0, src=None) == 0
        assert st(rope=rope, kv_type=2) == E.ERR_TYPE and st(rope=rope, kv_type=Q8_0, D=48, ld=(96, 48)) == E.ERR_SHAPE
        assert st(rope=rope, ld=(256, 130)) == E.ERR_SHAPE and st(rope=rope, ld=(256, 64)) == E.ERR_SHAPE
        assert st(rope=rope, nb=(nb_page - 16, nb_pos, nb_head)) == E.ERR_SHAPE and st(rope=rope, nb=(nb_page + 4, nb_pos, nb_head)) == E.ERR_SHAPE
        assert st(rope=rope, nb=(nb_page, nb_pos, 250)) == E.ERR_SHAPE and st(rope=rope, ld_pages=1) == E.ERR_SHAPE
        assert st(rope=rope, d_len=None) == E.ERR_ARG and st(rope=rope, pages=None) == E.ERR_ARG and st(rope=rope, n_pages=0) == E.ERR_ARG
        assert st(rope=rope, n_seq=0) == E.ERR_SHAPE and st(rope=rope, n_seq=4097) == E.ERR_SHAPE
        assert st(rope=rope, src=None) == E.ERR_ARG and st(rope=rope, pool=0x1008) == E.ERR_SHAPE

    def pos(q_start=0x1000, d_len=0x1000, n_seq=2, n_tokens_max=16, d_pos=0x1000):
        return L.ggml_hip_ragged_positions_dev(_p(q_start), _p(d_len), n_seq, n_tokens_max, _p(d_pos), None)

    assert pos(q_start=None) == E.ERR_ARG and pos(d_len=None) == E.ERR_ARG and pos(d_pos=None) == E.ERR_ARG
    assert pos(q_start=0x1002) == E.ERR_SHAPE and pos(d_pos=0x1001) == E.ERR_SHAPE
    assert pos(n_seq=0) == E.ERR_SHAPE and pos(n_seq=4097) == E.ERR_SHAPE
    assert pos(n_tokens_max=-1) == E.ERR_ARG and pos(n_tokens_max=(1 << 20) + 1) == E.ERR_SHAPE and pos(n_tokens_max=0, d_pos=None) == 0


# ---------------------------------------------------------------- GPU
@pytest.fixture(scope="module")
def dev():
    torch = pytest.importorskip("torch")
    from ggmlsharp_amd import device
    device.init(0)
    device.torch = torch
    return device


SWEEP = [(t, D, nh, nhk, (D // 64 + nh // 8) % 2) for t in (F16, Q8_0) for D in (64, 128) for nh, nhk in ((4, 2), (8, 1))]
_POOL, _UNIFORM = {}, {}


def _rows(cfg, b):
    """the cache rows of sequence b: n_kv[b] positions; sequence 6 begins with sequence 0's first page (the shared prefix)"""
    kv_type, D, _, n_head_kv, _ = cfg
    n = D_LEN[b] + N_Q[b]
    K, V = P.seq_rows(kv_type, D, n_head_kv, "r%d" % b, n)
    if b == 6:
        K0, V0 = P.seq_rows(kv_type, D, n_head_kv, "r0", D_LEN[0] + N_Q[0])
        K, V = K.copy(), V.copy()
        K[:PAGE], V[:PAGE] = K0[:PAGE], V0[:PAGE]
    return K, V


def pool_of(cfg):
    """the host image of the pool with every sequence's n_kv[b] rows in its pages, built once per cfg"""
    if cfg not in _POOL:
        kv_type, D, _, n_head_kv, layout = cfg
        pool = P.Pool(kv_type, D, n_head_kv, layout, n_pages=N_PAGES)
        for b, pages in enumerate(TABLE):
            K, V = _rows(cfg, b)
            pool.put(0, pages, K, D_LEN[b] + N_Q[b])
            pool.put(1, pages, V, D_LEN[b] + N_Q[b])
        _POOL[cfg] = pool
    return _POOL[cfg]


def sinks_of(dev, n_head):
    return dev.torch.from_numpy(np.linspace(-1.0, 2.0, n_head).astype(np.float32)).cuda()


def opts_of(dev, cfg, on):
    return dict(OPTS, sinks=sinks_of(dev, cfg[2])) if on else {}


def uniform(dev, cfg, b, on):
    """what sequence b's rows must be: the uniform paged entry for it alone (the _ex entry when the options are on), computed once -> [n_q, n_head, D]"""
    key = (cfg, b, on)
    if key not in _UNIFORM:
        torch = dev.torch
        _, D, n_head, n_head_kv, _ = cfg
        if N_Q[b] == 0:                                              # an idle slot has no rows
            return np.zeros((0, n_head, D), np.float32)
        pc = pool_of(cfg).cache(dev, [TABLE[b]], [D_LEN[b]], N_KV_MAX)
        q = torch.from_numpy(P.queries(D, n_head, "r%d" % b, N_Q[b])).cuda()
        out = dev.attn_paged(pc, q, n_head_kv, len_bias=N_Q[b], **opts_of(dev, cfg, on))
        torch.cuda.synchronize()
        _UNIFORM[key] = out.cpu().numpy()
    return _UNIFORM[key]


def ragged(dev, cfg, on, order=tuple(range(len(BATCH))), n_dec_rows_max=None, q_start=None, table=TABLE, n_tokens_max=N_TOKENS_MAX):
    """one ragged call over the batch in `order` into a poisoned dst -> (dst [n_tokens_max, n_head, D], the q_start used)"""
    torch = dev.torch
    _, D, n_head, n_head_kv, _ = cfg
    qs = q_start_of([N_Q[b] for b in order]) if q_start is None else np.asarray(q_start, np.int32)
    pc = pool_of(cfg).cache(dev, [table[b] for b in order], [D_LEN[b] for b in order], N_KV_MAX)
    q = np.full((n_tokens_max, n_head, D), 3.0, np.float32)
    base = q_start_of([N_Q[b] for b in order])                       # (the rows hold the sequences' queries where the unmodified bounds put them)
    for i, b in enumerate(order):
        q[base[i]:base[i + 1]] = P.queries(D, n_head, "r%d" % b, N_Q[b])
    dst = torch.full((n_tokens_max, n_head, D), float(POISON), device="cuda")
    dev.attn_paged_ragged(pc, torch.from_numpy(qs).cuda(), torch.from_numpy(q).cuda(), n_head_kv, add_q=True, n_dec_rows_max=n_dec_rows_max, out=dst,
                          **opts_of(dev, cfg, on))
    torch.cuda.synchronize()
    return dst.cpu().numpy(), base


def poisoned(x):
    return np.array_equal(bits(x), np.full(x.shape, bits(POISON), np.uint32))


def zeros(x):
    return np.array_equal(bits(x), np.zeros(x.shape, np.uint32))


def check_batch(dev, cfg, on, got, base, order, zero=(), absent=()):
    """every sequence's rows are the uniform entry's bits -- +0.0f for those in `zero`, untouched for those in `absent` -- and no other row is written"""
    written = np.zeros(got.shape[0], bool)
    for i, b in enumerate(order):
        rows = got[base[i]:base[i + 1]]
        if b in absent:
            assert poisoned(rows), (cfg, on, "absent", b)
            continue
        written[base[i]:base[i + 1]] = True
        if b in zero:
            assert zeros(rows), (cfg, on, "zero", b)
        else:
            assert np.array_equal(bits(rows), bits(uniform(dev, cfg, b, on))), (cfg, on, "sequence", b)
    assert poisoned(got[~written]), (cfg, on, "a row of no present sequence was written")


@pytest.mark.gpu
@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("cfg", SWEEP)
def test_every_sequence_equals_the_uniform_paged_entry_bit_for_bit(dev, cfg, on):
    order = tuple(range(len(BATCH)))
    table = TABLE
    if on:                                                          # an entry below c_lo of sequence 6 is invalid and must not matter
        table = TABLE[:6] + ((INVALID,) + TABLE[6][1:],) + TABLE[7:]
    got, base = ragged(dev, cfg, on, table=table)
    check_batch(dev, cfg, on, got, base, order)
    assert zeros(got[base[7]:base[8]])                               # the invalid needed page id: zeros for sequence 7 alone
    for b in (0, 2, 3, 4, 5, 6):
        rows = got[base[b]:base[b + 1]]
        assert np.isfinite(rows).all() and np.abs(rows).max() > 0, (cfg, on, b)
    assert poisoned(got[sum(N_Q):])                                  # rows beyond d_q_start[n_seq]


@pytest.mark.gpu
@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_sequences_rows_keep_their_bits_in_a_permuted_batch_and_under_other_bounds(dev, kv_type, on):
    cfg = (kv_type, 128, 8, 1, 0)
    for order in ((5, 7, 3, 0, 6, 1, 4, 2), (7, 6, 5, 4, 3, 2, 1, 0)):
        got, base = ragged(dev, cfg, on, order=order)
        check_batch(dev, cfg, on, got, base, order)
    order = tuple(range(len(BATCH)))
    for n_tokens_max, n_dec in ((sum(N_Q), 15), (400, 64), (400, 400)):
        got, base = ragged(dev, cfg, on, n_tokens_max=n_tokens_max, n_dec_rows_max=n_dec)
        check_batch(dev, cfg, on, got, base, order)


@pytest.mark.gpu
@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_decode_sequence_that_does_not_fit_is_zero_and_the_others_are_served(dev, kv_type, on):
    """The DECODE rows of the batch are 1 + 3 + 8 + 2 + 1 = 15.  With n_dec_rows_max one short the slots go in ascending b, so the LAST DECODE
    sequence is the one that does not fit.  One short can never leave room for a later one (the rows before, the one that fails and the rows
    after sum to 15), so a second case, n_dec_rows_max = 6 in batch order, has the 8-row sequence fail at slot 4 and the later 2-row one fit there."""
    cfg = (kv_type, 64, 4, 2, 1)
    order = (7, 0, 6, 5, 3, 4, 1, 2)                                # the last DECODE sequence is the 3-row one
    got, base = ragged(dev, cfg, on, order=order, n_dec_rows_max=14)
    check_batch(dev, cfg, on, got, base, order, zero=(2,))
    order = (2, 0, 6, 5, 7, 4, 1, 3)                                # ... the 8-row one
    got, base = ragged(dev, cfg, on, order=order, n_dec_rows_max=14)
    check_batch(dev, cfg, on, got, base, order, zero=(3,))
    order = tuple(range(len(BATCH)))
    got, base = ragged(dev, cfg, on, n_dec_rows_max=6)              # slots: b0 at 0, b2 at 1, b3 (8 rows) does not fit, b6 at 4, b7 does not fit
    check_batch(dev, cfg, on, got, base, order, zero=(3, 7))
    got, base = ragged(dev, cfg, on, n_dec_rows_max=0)              # no slot at all: every DECODE sequence is zero, PROMPT untouched
    check_batch(dev, cfg, on, got, base, order, zero=(0, 2, 3, 6, 7))


@pytest.mark.gpu
@pytest.mark.parametrize("on", [False, True])
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_sequence_that_is_not_present_writes_nothing_and_the_others_keep_their_bits(dev, kv_type, on):
    cfg = (kv_type, 128, 4, 2, 0)
    order = tuple(range(len(BATCH)))
    base = q_start_of(N_Q)
    qs = base.copy()
    qs[8] = 100                                                     # sequence 7 = [163, 100): decreasing.  Present it writes zeros; absent, nothing
    got, _ = ragged(dev, cfg, on, q_start=qs)
    check_batch(dev, cfg, on, got, base, order, absent=(7,))
    qs = base.copy()
    qs[6] = N_TOKENS_MAX + 30                                       # sequence 5 ends beyond n_tokens_max, sequence 6 = [200, 163) decreases
    got, _ = ragged(dev, cfg, on, q_start=qs)
    check_batch(dev, cfg, on, got, base, order, absent=(5, 6))
    qs = base.copy()
    qs[0] = -1                                                      # a negative start
    got, _ = ragged(dev, cfg, on, q_start=qs)
    check_batch(dev, cfg, on, got, base, order, absent=(0,))


@pytest.mark.gpu
def test_ragged_positions_against_numpy(dev):
    torch = dev.torch
    d_len = torch.tensor(D_LEN, dtype=torch.int32, device="cuda")
    base = q_start_of(N_Q)
    bad = base.copy()
    bad[6] = N_TOKENS_MAX + 30
    neg = base.copy()
    neg[0] = -1
    for qs in (base, bad, neg):
        want = np.zeros(N_TOKENS_MAX, np.int32)
        for b in range(len(BATCH)):
            if 0 <= qs[b] <= qs[b + 1] <= N_TOKENS_MAX:
                want[qs[b]:qs[b + 1]] = D_LEN[b] + np.arange(qs[b + 1] - qs[b])
        out = torch.full((N_TOKENS_MAX,), -5, dtype=torch.int32, device="cuda")
        dev.ragged_positions(torch.from_numpy(qs).cuda(), d_len, N_TOKENS_MAX, out=out)
        torch.cuda.synchronize()
        assert np.array_equal(out.cpu().numpy(), want), qs
    assert want.max() > 0


STORE_KV_MAX = 384                                                  # sequence 6's second token falls at position 384 = n_kv_max: it writes nothing


@pytest.mark.gpu
@pytest.mark.parametrize("rope", [False, True])
@pytest.mark.parametrize("cfg", SWEEP)
def test_the_ragged_stores_write_the_uniform_stores_bytes_and_nothing_else(dev, cfg, rope):
    torch = dev.torch
    kv_type, D, _, n_head_kv, layout = cfg
    rng = np.random.default_rng([kv_type, D, n_head_kv, int(rope)])
    pool = P.Pool(kv_type, D, n_head_kv, layout, n_pages=N_PAGES)
    pool.host[0][:] = rng.integers(0, 256, pool.host[0].size, dtype=np.uint8)
    x = torch.zeros((N_TOKENS_MAX, n_head_kv, D + 4), device="cuda")[:, :, :D]                 # padded strides
    x.copy_(torch.from_numpy(rng.uniform(-1, 1, (N_TOKENS_MAX, n_head_kv, D)).astype(np.float32)))
    rp = dev.rope_params(D if D == 64 else 96, mode=2 if D == 128 else 0)
    base = q_start_of(N_Q)
    absent = base.copy()
    absent[6] = N_TOKENS_MAX + 30                                   # sequences 5 and 6 are not present: their rows are not stored

    def store(pc, *a):
        if rope:
            dev.rope_kv_store_paged(rp, pc, *a) if len(a) == 2 else dev.rope_kv_store_paged_ragged(rp, pc, *a)
        else:
            dev.kv_store_paged(pc, *a) if len(a) == 2 else dev.kv_store_paged_ragged(pc, *a)

    for qs, gone in ((base, ()), (absent, (5, 6))):
        one = pool.cache(dev, TABLE, D_LEN, STORE_KV_MAX, ld_pages=4)
        for b in range(len(BATCH)):                                  # the uniform stores, a sequence at a time, into one pool
            if N_Q[b] == 0 or b in gone:
                continue
            pc = dev.PagedCache(kv_type, one.k, one.v, one.nb_page, one.nb_pos, one.nb_head, N_PAGES, one.pages[b:b + 1], one.d_len[b:b + 1], STORE_KV_MAX)
            store(pc, x[base[b]:base[b + 1]], pc.k)
        rag = pool.cache(dev, TABLE, D_LEN, STORE_KV_MAX, ld_pages=4)
        store(rag, torch.from_numpy(qs).cuda(), x, rag.k)
        torch.cuda.synchronize()
        assert torch.equal(rag.k, one.k), (cfg, rope, gone)
        assert torch.equal(rag.v.cpu(), torch.from_numpy(pool.host[1]))
        got = rag.k.cpu().numpy()
        changed = np.flatnonzero((got != pool.host[0]).reshape(N_PAGES, -1).any(axis=1))
        want = {4, 15, 2, 11, 6, 0, 8, 10} - ({0, 8, 10} if gone else set())       # the pages the tokens of the present sequences fall on
        assert set(changed.tolist()) == want, (cfg, rope, gone, changed)   # page 7 (sequence 6's position 384) and sequence 7's invalid id: nothing


@pytest.mark.gpu
@pytest.mark.parametrize("kv_type", [F16, Q8_0])
def test_a_captured_ragged_step_follows_a_sequence_from_prefill_to_decode(dev, kv_type):
    """ragged_positions -> rope(q) -> rope_kv_store_paged_ragged(k) -> kv_store_paged_ragged(v) -> attn_paged_ragged(add_q = 1) on one stream,
    captured ONCE and replayed with two batches: in the second the former prefill sequence decodes one token and a former decode slot prefills 20.
    After each replay dst and both pools equal the eager uniform calls, a sequence at a time, for that batch."""
    torch = dev.torch
    D, n_head, n_head_kv, n_seq, n_max, n_tok = 128, 8, 2, 4, 3 * PAGE, 40
    batches = (((1, 100), (30, 0), (0, 40), (2, 130)), ((20, 101), (1, 30), (1, 40), (3, 132)))
    table = ((4, 2, P.GARBAGE), (7, P.GARBAGE, P.GARBAGE), (9, P.GARBAGE, P.GARBAGE), (5, 1, 6))
    rp = dev.rope_params(D, mode=2)
    rng = np.random.default_rng(23)
    pool = P.Pool(kv_type, D, n_head_kv, 0, n_pages=N_PAGES)
    for (_, n), pages in zip(batches[0], table):
        for side in (0, 1) if n else ():
            pool.put(side, pages, A.encode_rows(kv_type, rng.uniform(-1, 1, (n, n_head_kv, D)).astype(np.float32)), n)
    pc = pool.cache(dev, table, [n for _, n in batches[0]], n_max)
    warm = pool.cache(dev, table, [n for _, n in batches[0]], n_max)
    q_start = torch.from_numpy(q_start_of([n for n, _ in batches[0]])).cuda()
    q = torch.zeros((n_tok, n_head, D), device="cuda")
    k_new = torch.zeros((n_tok, n_head_kv, D), device="cuda")
    v_new = torch.zeros((n_tok, n_head_kv, D), device="cuda")
    pos, q_rot, out = torch.zeros(n_tok, dtype=torch.int32, device="cuda"), torch.zeros_like(q), torch.zeros_like(q)
    n_dec = min(n_tok, 8 * n_seq)
    work = torch.empty(dev.attn_paged_ragged_work_size(kv_type, D, n_head, n_head_kv, n_seq, n_tok, n_dec, n_max), dtype=torch.uint8, device="cuda")

    def step(cache, o):
        dev.ragged_positions(q_start, cache.d_len, n_tok, out=pos)
        dev.rope(rp, q, pos=pos, out=q_rot)
        dev.rope_kv_store_paged_ragged(rp, cache, q_start, k_new, cache.k)
        dev.kv_store_paged_ragged(cache, q_start, v_new, cache.v)
        dev.attn_paged_ragged(cache, q_start, q_rot, n_head_kv, add_q=True, n_dec_rows_max=n_dec, out=o, work=work)

    step(warm, torch.zeros_like(out))                                # (a first call outside the capture, on copies: one-time kernel attributes)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(pc, out)
    torch.cuda.current_stream().wait_stream(s)
    for batch in batches:
        n_qs, lens = [n for n, _ in batch], [n for _, n in batch]
        qs = q_start_of(n_qs)
        q_start.copy_(torch.from_numpy(qs))
        pc.d_len.copy_(torch.tensor(lens, dtype=torch.int32))
        for t in (q, k_new, v_new):
            t.copy_(torch.from_numpy(rng.uniform(-1, 1, tuple(t.shape)).astype(np.float32)))
        out.fill_(float(POISON))
        ek, ev = pc.k.clone(), pc.v.clone()                          # the pools before the step, for the eager calls
        g.replay()
        torch.cuda.synchronize()
        for b in range(n_seq):
            if n_qs[b] == 0:
                continue
            r0, r1 = int(qs[b]), int(qs[b + 1])
            one = dev.PagedCache(kv_type, ek, ev, pc.nb_page, pc.nb_pos, pc.nb_head, N_PAGES, pc.pages[b:b + 1], pc.d_len[b:b + 1], n_max)
            qb = dev.rope(rp, q[r0:r1], pos0=lens[b])
            dev.rope_kv_store_paged(rp, one, k_new[r0:r1], one.k)
            dev.kv_store_paged(one, v_new[r0:r1], one.v)
            eager = dev.attn_paged(one, qb, n_head_kv, len_bias=n_qs[b])
            torch.cuda.synchronize()
            assert torch.equal(out[r0:r1], eager), (kv_type, batch, b)
            assert bool(torch.isfinite(eager).all()) and float(eager.abs().max()) > 0
        assert torch.equal(pc.k, ek) and torch.equal(pc.v, ev), (kv_type, batch)
        assert poisoned(out[int(qs[-1]):].cpu().numpy())
