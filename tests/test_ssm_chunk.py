"""The chunked selective scan (include/ggml_hip_ext.h: ggml_hip_ssm_scan_chunked_ragged_dev, ggml_hip_ssm_scan_chunked_plan, ggml_hip_ssm_scan_chunked_work_size;
csrc/ssm_chunk.hip, ssm.cpp, plan.cpp plan_ssm_chunk).

Yardsticks (tests/np_ssm_chunk.py): the reference is np_ssm.scan_f64, the SEQUENTIAL statement in float64; the bar is derived there from u = 2^-24 for the
chunked form and never measured.  The kernels and the float32 model of the chunked statement are held to 1 x that bar for every row and every element of the
final state; five mutants of the form exceed it a hundredfold where they apply, and every mutant is shown to apply somewhere.  A sequence of at most
seq_max_tokens tokens is bit for bit ggml_hip_ssm_scan_ragged_dev's.  The bitwise contracts (i), (iii) and (ii') need no reference.

Q and seq_max_tokens are READ FROM THE PLAN, never written here: ONE ragged batch is built from them -- counts 0, 1, seq_max_tokens, seq_max_tokens + 1, Q - 1,
Q, Q + 1, 2 Q and 2 Q + Q / 2 + 3, an absent sequence, a short and a long sequence with slot ids -1 and n_slots, fresh sequences over NaN slots and continued
ones, and three rows nobody owns, filled with 3.0e38, directly behind the partial tail of the last sequence.  (ii') splits a sequence at the first two
multiples of Q above seq_max_tokens -- Q and 2 Q where seq_max_tokens < Q -- since both parts must be chunked for the contract to apply.
Shapes: the five below, the smallest at which a tile, a P tile, a group index or the state pass can go wrong; test_every_kernel_form_has_a_shape sweeps the
plan over every served (P, N) and holds the shapes' kernel forms to be exactly the reachable ones."""
import ctypes as C
import fnmatch
import functools
import os
import re

import numpy as np
import pytest

import np_ssm
import np_ssm_chunk as npc
import test_ssm as ts
from ggmlsharp_amd import _lib

ROOT = ts.ROOT
NEW_SYMBOLS = ("ggml_hip_ssm_scan_chunked_ragged_dev", "ggml_hip_ssm_scan_chunked_plan", "ggml_hip_ssm_scan_chunked_work_size")
SENTINEL, NAN_BYTES, GUARD, FAKE = ts.SENTINEL, ts.NAN_BYTES, ts.GUARD, ts.FAKE
OK, ERR_SHAPE, ERR_ARG = ts.OK, ts.ERR_SHAPE, ts.ERR_ARG
F, U = np.float32, np_ssm.U
_p, _up, _bits, _stream, Pool = ts._p, ts._up, ts._bits, ts._stream, ts.Pool
dev = ts.dev

# seed: A is drawn first, so it does not follow the batch; every shape has a head whose chunks decay below the binary32 exponential's underflow (the quotient
# mutant needs one) beside the head with A = 0, and "small" and "mamba2" a slowly decaying head too
SHAPES = {
    "small": dict(H=4, P=16, N=16, G=1, seed=318),                   # the smallest of everything: P tile 16, one block of N
    "mamba2": dict(H=4, P=64, N=128, G=2, seed=317),                 # the Mamba-2 head, two groups: P tile 64
    "n48": dict(H=2, P=48, N=48, G=1, seed=365),                     # P and N no powers of two: three P tiles of 16, three blocks of N over four waves
    "g3": dict(H=3, P=32, N=80, G=3, seed=336),                      # one head per group: P tile 32, five blocks of N
    "largest": dict(H=1, P=256, N=256, G=1, seed=343),               # every P tile of the largest head: four tiles of 64, sixteen blocks of N
}


def _plan(H, P, N, G, aps, n_seq, n_tokens_max):
    out = _lib.ggml_hip_ssm_chunk_plan_t()
    rc = _lib.lib().ggml_hip_ssm_scan_chunked_plan(H, P, N, G, aps, n_seq, n_tokens_max, C.byref(out))
    return rc, out


def _work_size(H, P, N, G, aps, n_seq, n_tokens_max):
    return int(_lib.lib().ggml_hip_ssm_scan_chunked_work_size(H, P, N, G, aps, n_seq, n_tokens_max))


@functools.lru_cache(maxsize=None)
def _q_and_smt():
    """Q and seq_max_tokens of the plan; the same for every shape the tests use, which test_the_batch_is_what_it_says asserts"""
    rc, p = _plan(4, 64, 128, 2, 0, 1, 1 << 20)
    assert rc == OK and p.form == 2
    return int(p.chunk), int(p.seq_max_tokens)


# ---------------------------------------------------------------- the batch, built from the plan's Q and seq_max_tokens
class Batch(ts.Batch):
    pass


@functools.lru_cache(maxsize=None)
def batch():
    Q, smt = _q_and_smt()
    counts = [None, 1, 0, smt, smt + 1, 3, Q - 1, Q, Q + 1, Q + 2, 2 * Q, 2 * Q + Q // 2 + 3]      # (None: not present)
    n_slots = 12
    slot = np.array([7, 2, 5, 0, 9, -1, 4, 11, 1, n_slots, 3, 6], np.int32)
    d_len = np.array([4, 7, 3, 0, 5, 2, 0, 6, 0, 1, 9, 0], np.int32)
    q = [-3, 0]
    for n in counts[1:]:
        q.append(q[-1] + n)
    k = Batch(q[-1] + 3, np.array(q, np.int32), d_len, slot, tuple(b for b in range(1, 12) if counts[b] and 0 <= slot[b] < n_slots),
              tuple(b for b in range(1, 12) if counts[b] and not 0 <= slot[b] < n_slots))
    k.counts, k.n_slots, k.Q, k.smt = counts, n_slots, Q, smt
    k.chunked = tuple(b for b in k.served if counts[b] > smt)
    k.short = tuple(b for b in k.served if counts[b] <= smt)
    return k


def test_the_batch_is_what_it_says():
    k = batch()
    Q, smt = k.Q, k.smt
    for s in SHAPES.values():
        rc, p = _plan(s["H"], s["P"], s["N"], s["G"], 0, k.n_seq, k.n_tokens_max)
        assert rc == OK and (p.form, p.chunk, p.seq_max_tokens) == (2, Q, smt)
    got = [int(k.q_start[b + 1] - k.q_start[b]) for b in range(1, k.n_seq)]
    assert got == [1, 0, smt, smt + 1, 3, Q - 1, Q, Q + 1, Q + 2, 2 * Q, 2 * Q + Q // 2 + 3] and k.q_start[0] < 0
    assert set(got) >= {0, 1, smt, smt + 1, Q - 1, Q, Q + 1, 2 * Q, 2 * Q + Q // 2 + 3}
    present = [b for b in range(k.n_seq) if 0 <= k.q_start[b] <= k.q_start[b + 1] <= k.n_tokens_max]
    assert present == list(range(1, k.n_seq)) and k.q_start[k.n_seq] == k.n_tokens_max - 3
    assert k.zeroed == (5, 9) and sorted(int(k.slot[b]) for b in k.zeroed) == [-1, k.n_slots]
    assert k.counts[5] <= smt < k.counts[9]                          # a slot id outside the pool in the sequential form and in the chunked form
    assert k.served == (1, 3, 4, 6, 7, 8, 10, 11) and len({int(k.slot[b]) for b in k.served}) == len(k.served)
    assert set(k.chunked) | set(k.short) == set(k.served) and len(k.chunked) >= 3 and len(k.short) >= 2
    for group in (k.chunked, k.short):                               # fresh and continued in both forms
        assert {bool(k.d_len[b]) for b in group} == {False, True}, group
    assert (k.counts[11] % Q) and k.q_start[12] + 3 == k.n_tokens_max  # the rows nobody owns lie directly behind a partial tail
    assert any(k.counts[b] > Q and k.counts[b] % Q == 0 for b in k.chunked) and any(k.counts[b] > 2 * Q for b in k.chunked)


# ---------------------------------------------------------------- the inputs and references, computed once
@functools.lru_cache(maxsize=None)
def case(name):
    s, k = SHAPES[name], batch()
    H, P, N, G, n = s["H"], s["P"], s["N"], s["G"], k.n_tokens_max
    rng = np.random.default_rng(s["seed"])
    c = dict(s, aps=False)
    c["A"] = (-np.exp(rng.uniform(-3.0, 2.5, H))).astype(F)
    if H > 1:
        c["A"][1] = F(0.0)                                           # one head that does not decay: a pure running sum
    c["x"] = rng.normal(0.0, 1.0, (n, H, P)).astype(F)
    c["dt"] = (2.0 * rng.normal(0.0, 1.0, (n, H)) - 1.0).astype(F)
    c["dt"][int(k.q_start[11]) + 70, 0] = F(25.0)                    # (the branch d > 20, in the second chunk of the longest sequence)
    c["B"] = rng.normal(0.0, 1.0, (n, G, N)).astype(F)
    c["C"] = rng.normal(0.0, 1.0, (n, G, N)).astype(F)
    c["D"] = rng.normal(0.0, 1.0, H).astype(F)
    c["dt_bias"] = (0.5 * rng.normal(0.0, 1.0, H)).astype(F)
    c["pool"] = rng.normal(0.0, 1.0, (k.n_slots, H, P, N)).astype(F)
    owned = np.zeros(n, bool)
    for b in k.served + k.zeroed:
        owned[slice(*k.rows(b))] = True
    for key in ("x", "dt", "B", "C"):
        c[key][~owned] = F(3.0e38)
    return c


def _seq_args(c, b, with_D=True, with_bias=True):
    return ts._seq_args(c, b, batch(), with_D, with_bias)


@functools.lru_cache(maxsize=None)
def ref(name, b, with_D=True, with_bias=True):
    """sequence b in float64: (y, h) of the SEQUENTIAL statement, the chunked bars (bar_y, bar_h), the least cs of a chunk, and the sequential bars"""
    a, kw = _seq_args(case(name), b, with_D, with_bias)
    y, h, sbar_y, sbar_h = np_ssm.scan_f64(*a, want_bar=True, **kw)
    yc, hc, bar_y, bar_h, cs_min = npc.chunk_f64(*a, Q=batch().Q, want_bar=True, **kw)
    return y, h, bar_y, bar_h, cs_min, sbar_y, sbar_h, yc, hc


# ---------------------------------------------------------------- CPU
def test_the_new_symbols_are_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    exports = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "ggmlsharp_amd", "csrc", "exports.map")).read(), flags=re.S)
    pats = re.search(r"global:([^;]*);", exports).group(1).split()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name
        assert any(fnmatch.fnmatchcase(name, p) for p in pats), name
    assert "ggml_hip_ssm_chunk_plan_t" in hdr and "ggml_hip_ssm_chunk_plan_t" in cs and C.sizeof(_lib.ggml_hip_ssm_chunk_plan_t) == 56
    assert C.sizeof(_lib.ggml_hip_ssm_plan_t) == 32                  # (the sequential plan's struct is untouched)


def _fields(p):
    return tuple(int(getattr(p, f[0])) for f in p._fields_)


def test_the_plan_and_the_work_size_are_functions_of_their_arguments():
    Q, smt = _q_and_smt()
    L = _lib.lib()
    seen = {}
    for rep in range(2):
        for a in ((4, 16, 16, 1, 0, 1, 500), (64, 64, 128, 8, 0, 65, 2112), (2, 48, 48, 1, 0, 9, 700), (1, 256, 256, 1, 0, 4096, 1 << 20), (3, 32, 80, 3, 0, 2, smt + 1)):
            rc, p = _plan(*a)
            H, P, N, G, aps, n_seq, ntm = a
            assert rc == OK and seen.setdefault(a, _fields(p)) == _fields(p)
            pt = 64 if P % 64 == 0 else 32 if P % 32 == 0 else 16
            assert (p.form, p.chunk, p.seq_max_tokens, p.launches, p.p_tile, p.p_tiles, p.kernel_state, p.kernel_out) == (2, Q, smt, 5, pt, P // pt, pt, pt)
            assert p.seqs_max == min(n_seq, ntm // (smt + 1)) and p.chunks_max == p.seqs_max + (ntm - p.seqs_max) // Q
            assert p.work_bytes == _work_size(*a) and p.work_bytes >= p.chunks_max * H * (P * N + 2 * Q) * 4 + 8 * p.chunks_max + 16 * p.seqs_max
            if rep == 0:
                assert L.ggml_hip_ssm_state_bytes(H, P, N) == H * P * N * 4
    # the shapes the chunked form does not serve, and a call no sequence of which can be chunked: form 1, one launch, no work buffer -- not refused
    for a in ((4, 16, 16, 1, 1, 3, 500), (4, 5, 48, 1, 0, 3, 500), (4, 24, 16, 1, 0, 3, 500), (4, 64, 128, 2, 0, 3, smt), (4, 64, 128, 2, 0, 3, 0)):
        rc, p = _plan(*a)
        assert rc == OK and _fields(p) == (1, Q, smt, 1, 0, 0, 0, 0, 0, 0, 0) and _work_size(*a) == 0, a
    # monotone in n_tokens_max (and in n_seq)
    for H, P, N, G in ((4, 16, 16, 1), (4, 64, 128, 2)):
        last = (0, 0, 0)
        for ntm in list(range(0, 4 * Q + 8)) + [1000, 4096, 1 << 16, 1 << 20]:
            rc, p = _plan(H, P, N, G, 0, 7, ntm)
            now = (int(p.chunks_max), int(p.seqs_max), int(p.work_bytes))
            assert rc == OK and all(x >= y for x, y in zip(now, last)), ntm
            assert _plan(H, P, N, G, 0, 8, ntm)[1].work_bytes >= p.work_bytes
            last = now
    # chunks_max and seqs_max bound every valid batch
    rng = np.random.default_rng(5)
    for _ in range(2000):
        n_seq = int(rng.integers(1, 40))
        if rng.integers(0, 2):                                      # sequences cut at random out of the rows
            ntm = int(rng.integers(0, 3000))
            n_q = np.diff(np.sort(rng.integers(0, ntm + 1, n_seq + 1)))
        else:                                                       # a few sequences just above the threshold or long, the rest idle or one token, no row to spare
            n_q = rng.integers(0, 2, n_seq)
            for j in rng.integers(0, n_seq, int(rng.integers(1, 5))):
                n_q[j] = int(rng.choice([smt + 1, smt + 2, Q + 1, 2 * Q, 2 * Q + 1, int(rng.integers(smt + 1, 6 * Q))]))
            ntm = int(n_q.sum()) + int(rng.integers(0, 2))
        rc, p = _plan(4, 16, 16, 1, 0, n_seq, ntm)
        long = n_q[n_q > smt]
        assert rc == OK and (long.size == 0 or p.form == 2)
        assert int(p.chunks_max) >= int(np.sum(-(-long // Q))) and int(p.seqs_max) >= long.size, (n_seq, ntm, n_q)
    # refused shapes: the sequential plan's, and the bounds of the batch
    for bad in ((0, 64, 128, 1, 0, 1, 100), (4, 0, 128, 1, 0, 1, 100), (4, 257, 128, 1, 0, 1, 100), (4, 64, 24, 1, 0, 1, 100), (4, 64, 272, 1, 0, 1, 100),
                (4, 64, 128, 3, 0, 1, 100), (4, 64, 128, 1, 0, 0, 100), (4, 64, 128, 1, 0, 4097, 100), (4, 64, 128, 1, 2, 1, 100), (4, 64, 128, 1, 0, 1, -1),
                (4, 64, 128, 1, 0, 1, (1 << 20) + 1)):
        assert _plan(*bad)[0] == ERR_SHAPE and _work_size(*bad) == 0, bad
    assert L.ggml_hip_ssm_scan_chunked_plan(4, 64, 128, 1, 0, 1, 100, None) == ERR_ARG


def _rc(**kw):
    """one call on pointers that are no device memory; every caller changes at least one argument into something a host check refuses"""
    assert kw
    a = dict(x=FAKE, ldx_tok=128, ldx_head=16, dt=FAKE, ld_dt=8, dt_bias=None, A=FAKE, a_ld=1, aps=0, B=FAKE, C=FAKE, ld_bc=32, D=None, n_head=8, P=16, N=16, G=2,
             n_seq=3, q_start=FAKE, n_tokens_max=300, len=FAKE, slot=FAKE, state=FAKE, nb_slot=8 * 16 * 16 * 4, n_slots=4, dst=FAKE, ldd_tok=128, ldd_head=16,
             work=FAKE, work_bytes=None)
    a.update(kw)
    if a["work_bytes"] is None:
        a["work_bytes"] = 1 << 40
    return _lib.lib().ggml_hip_ssm_scan_chunked_ragged_dev(
        _p(a["x"]), a["ldx_tok"], a["ldx_head"], _p(a["dt"]), a["ld_dt"], _p(a["dt_bias"]), _p(a["A"]), a["a_ld"], a["aps"], _p(a["B"]), _p(a["C"]), a["ld_bc"],
        _p(a["D"]), a["n_head"], a["P"], a["N"], a["G"], a["n_seq"], _p(a["q_start"]), a["n_tokens_max"], _p(a["len"]), _p(a["slot"]), _p(a["state"]), a["nb_slot"],
        a["n_slots"], _p(a["dst"]), a["ldd_tok"], a["ldd_head"], _p(a["work"]), a["work_bytes"], None)


def test_refusals_need_no_device():
    """every refusal of ggml_hip_ssm_scan_ragged_dev with its code, and the work buffer's (every call's pointers are no device memory: none may launch)"""
    rc = _rc
    ts._batch_refusals(rc, 8 * 16 * 16 * 4)
    assert rc(n_head=0) == ERR_SHAPE
    assert rc(n_head=(1 << 20) + 1) == ERR_SHAPE
    for P in (0, 257, -1):
        assert rc(P=P) == ERR_SHAPE, P
    for N in (0, 8, 24, 272):
        assert rc(N=N) == ERR_SHAPE, N
    for G in (0, 3, 16):
        assert rc(G=G) == ERR_SHAPE, G
    for aps in (2, -1):
        assert rc(aps=aps) == ERR_ARG, aps
    assert rc(ldx_head=15) == ERR_SHAPE
    assert rc(ldd_head=15) == ERR_SHAPE
    assert rc(ldx_tok=15) == ERR_SHAPE
    assert rc(ldd_tok=-8) == ERR_SHAPE
    assert rc(ld_dt=7) == ERR_SHAPE
    assert rc(a_ld=0) == ERR_SHAPE
    assert rc(aps=1, a_ld=15) == ERR_SHAPE
    assert rc(aps=1, a_ld=18) == ERR_SHAPE
    assert rc(aps=1, a_ld=16, A=FAKE + 4) == ERR_SHAPE
    assert rc(ld_bc=31) == ERR_SHAPE
    assert rc(ld_bc=34) == ERR_SHAPE
    for name in ("x", "dt", "A", "B", "C", "dst"):
        assert rc(**{name: None}) == ERR_ARG, name
    for name in ("B", "C"):
        assert rc(**{name: FAKE + 4}) == ERR_SHAPE, name
    for name in ("x", "dt", "dt_bias", "A", "D", "dst"):
        assert rc(**{name: FAKE + 2}) == ERR_SHAPE, name
    assert rc(N=32, ld_bc=64, nb_slot=8 * 16 * 16 * 4) == ERR_SHAPE
    need = _work_size(8, 16, 16, 2, 0, 3, 300)
    assert need > 0
    assert rc(work=None) == ERR_ARG
    assert rc(work_bytes=need - 1) == ERR_ARG
    assert rc(work_bytes=0) == ERR_ARG
    assert rc(work=None, work_bytes=0, n_tokens_max=0) == OK         # (no tokens: no work buffer, nothing launched)


def _ratio(got, want, bar):
    with np.errstate(all="ignore"):
        diff = np.abs(np.asarray(got, np.float64) - want)
        return float(np.where(np.isfinite(diff), diff / bar, np.inf).max())


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_the_float32_model_is_within_the_bar(name):
    k, c = batch(), case(name)
    for b in k.chunked:
        y, h, bar_y, bar_h, cs_min, sbar_y, sbar_h, yc, hc = ref(name, b)
        assert np.isfinite(bar_y).all() and np.isfinite(bar_h).all()
        # the chunked statement in float64 IS the sequential one: far inside either bar
        assert _ratio(yc, y, sbar_y) <= 1e-3 and _ratio(hc, h, sbar_h) <= 1e-3, (name, b)
        a, kw = _seq_args(c, b)
        y32, h32 = npc.chunk_f32(*a, Q=k.Q, **kw)
        ry, rh = _ratio(y32, y, bar_y), _ratio(h32, h, bar_h)
        print(f"{name} seq {b} ({k.counts[b]} tokens): model / bar  y {ry:.3f}  state {rh:.3f};  chunked bar / sequential bar  y median {float(np.median(bar_y / sbar_y)):.1f} "
              f"max {float((bar_y / sbar_y).max()):.1f}  state median {float(np.median(bar_h / sbar_h)):.1f} max {float((bar_h / sbar_h).max()):.1f};  least cs {cs_min:.0f}")
        assert ry <= 1.0 and rh <= 1.0, (name, b, ry, rh)


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_five_mutants_of_the_chunked_form_exceed_the_bar_a_hundredfold(name):
    k, c = batch(), case(name)
    applied = {m: 0 for m in npc.MUTANTS}
    for b in k.chunked:
        y, h, bar_y, bar_h, cs_min = ref(name, b)[:5]
        a, kw = _seq_args(c, b)
        T, Q = k.counts[b], k.Q
        for m in npc.MUTANTS:
            with np.errstate(all="ignore"):
                ym, hm = npc.chunk_f64(*a, Q=Q, mutant=m, **kw)
            ry, rh = _ratio(ym, y, bar_y), _ratio(hm, h, bar_h)
            ry2 = _ratio(ym[Q:], y[Q:], bar_y[Q:]) if T > Q else None
            print(f"{name} seq {b} ({T} tokens): {m} / bar  y {ry:.3g}  state {rh:.3g}  y from the second chunk {ry2}")
            if m == "mask_off_by_one":
                ok = ry >= 100.0
            elif m == "end_decay_on_h_in":                           # where H_in != 0 meets a row that is not its chunk's last: a continued sequence, or
                if k.d_len[b] == 0 and T <= Q + 1:                   # a second chunk of more than one token
                    continue
                ok = ry >= 100.0
            elif m == "no_decay_to_end":
                ok = rh >= 100.0 and (ry2 is None or ry2 >= 100.0)
            elif m == "tail_as_full":
                if T % Q == 0:                                       # (no partial tail: the statement itself)
                    continue
                ok = rh >= 100.0
            else:                                                    # quotient_decay: where a chunk's cs falls below the binary32 exponential's underflow
                if cs_min > npc.EXP_UNDERFLOW:
                    continue
                ok = ry >= 100.0
            assert ok, (name, b, m, ry, rh, ry2)
            applied[m] += 1
    assert all(applied.values()), applied                           # every mutant has a sequence where it applies


def _forms(shapes):
    k = batch()
    return {(int(p.p_tile), int(p.kernel_state), int(p.kernel_out)) for p in (_plan(s["H"], s["P"], s["N"], s["G"], 0, k.n_seq, k.n_tokens_max)[1] for s in shapes)}


def test_every_kernel_form_has_a_shape():
    """the state and out kernels are compiled once per P tile: the forms of SHAPES are the forms the plan hands out over every served (P, N), so a form added to
    the plan fails here until a shape reaches it.  Every shape but the first reaches something the others do not"""
    Q, smt = _q_and_smt()
    reachable = set()
    for P in range(16, 257, 16):
        for N in range(16, 257, 16):
            rc, p = _plan(2, P, N, 1, 0, 3, 1000)
            assert rc == OK and p.form == 2 and p.p_tile * p.p_tiles == P
            reachable.add((int(p.p_tile), int(p.kernel_state), int(p.kernel_out)))
    for P in list(range(1, 16)) + [17, 40, 100, 255]:
        assert _plan(2, P, 64, 1, 0, 3, 1000)[1].form == 1
    assert len(reachable) == 3 and _forms(SHAPES.values()) == reachable
    assert {s["P"] // _plan(s["H"], s["P"], s["N"], s["G"], 0, 3, 1000)[1].p_tile for s in SHAPES.values()} >= {1, 3, 4}      # one P tile, and more
    blocks = {s["N"] // 16 for s in SHAPES.values()}
    assert min(blocks) == 1 and any(b % 4 for b in blocks if b > 4) and max(blocks) == 16      # one wave works; waves with unequal blocks; the most
    assert any(s["G"] > 1 and s["H"] > s["G"] for s in SHAPES.values()) and any(s["G"] == s["H"] > 1 for s in SHAPES.values())


# ---------------------------------------------------------------- GPU
def _call(dev, c, q_start, d_len, slot, pool, n_tokens_max, row0=0, pad_head=0, pad_tok=0, pad_bc=0, pad_head_d=None, pad_tok_d=None, pad_dt=0, pad_a=0, with_D=True,
          with_bias=True, entry="chunked", work_fill=SENTINEL, work_shift=0, work_extra=0):
    """one call over rows [row0, row0 + n_tokens_max) of the case's packed inputs (tests/test_ssm.py _scan_call, with the work buffer): the paddings of every
    stride hold 3.0e38 (inputs) or the sentinel (dst).  entry "sequential": ggml_hip_ssm_scan_ragged_dev.  The work buffer is `work_bytes` + work_extra bytes
    prefilled with work_fill, `work_shift` bytes into an allocation, with a guard behind it.  -> (dst bits [n_tokens_max][H][P], the pool image after the
    call); the guards and paddings of dst, of the work buffer and every input are checked here"""
    H, P, N, G, aps = c["H"], c["P"], c["N"], c["G"], int(c["aps"])
    n = n_tokens_max
    sl = slice(row0, row0 + n)
    ldh, ldt = P + pad_head, H * (P + pad_head) + pad_tok
    ldh_d = P + (pad_head if pad_head_d is None else pad_head_d)
    ldt_d = H * ldh_d + (pad_tok if pad_tok_d is None else pad_tok_d)
    x = np.full((n, ldt), 3.0e38, F)
    x[:, :H * ldh].reshape(n, H, ldh)[:, :, :P] = c["x"][sl]
    ld_bc = 2 * G * N + pad_bc
    bc = np.full((n, ld_bc), 3.0e38, F)
    bc[:, :G * N] = c["B"][sl].reshape(n, G * N)
    bc[:, G * N:2 * G * N] = c["C"][sl].reshape(n, G * N)
    ld_dt = H + pad_dt
    dt = np.full((n, ld_dt), 3.0e38, F)
    dt[:, :H] = c["dt"][sl]
    a_ld = (N if aps else 1) + pad_a
    A = np.full((H, a_ld), 3.0e38, F)
    A[:, :a_ld - pad_a] = c["A"].reshape(H, -1)
    d_x, d_bc, d_dt, d_A = _up(dev, x), _up(dev, bc), _up(dev, dt), _up(dev, A)
    d_D, d_db = _up(dev, c["D"]), _up(dev, c["dt_bias"])
    d_q, d_l, d_s = _up(dev, np.asarray(q_start, np.int32)), _up(dev, np.asarray(d_len, np.int32)), _up(dev, np.asarray(slot, np.int32))
    d_pool = _up(dev, pool.image)
    dst = dev.torch.full((GUARD + max(n, 1) * ldt_d + GUARD,), SENTINEL, dtype=dev.torch.int32, device="cuda")
    args = (_p(d_x.data_ptr()), ldt, ldh, _p(d_dt.data_ptr()), ld_dt, _p(d_db.data_ptr()) if with_bias else None, _p(d_A.data_ptr()), a_ld, aps,
            _p(d_bc.data_ptr()), _p(d_bc.data_ptr() + 4 * G * N), ld_bc, _p(d_D.data_ptr()) if with_D else None, H, P, N, G, len(slot), _p(d_q.data_ptr()), n,
            _p(d_l.data_ptr()), _p(d_s.data_ptr()), _p(pool.ptr(d_pool)), pool.nb_slot, pool.n_slots, _p(dst.data_ptr() + 4 * GUARD), ldt_d, ldh_d)
    if entry == "sequential":
        rc = _lib.lib().ggml_hip_ssm_scan_ragged_dev(*args, _stream(dev))
    else:
        need = _work_size(H, P, N, G, aps, len(slot), n) + work_extra
        assert need % 4 == 0 and work_shift % 4 == 0
        work = dev.torch.full(((work_shift + need) // 4 + GUARD,), int(np.uint32(work_fill).view(np.int32)), dtype=dev.torch.int32, device="cuda")
        rc = _lib.lib().ggml_hip_ssm_scan_chunked_ragged_dev(*args, _p(work.data_ptr() + work_shift) if need else None, need, _stream(dev))
    assert rc == 0, _lib.lib().ggml_hip_last_error()
    dev.torch.cuda.synchronize()
    if entry != "sequential":
        w = _bits(work)
        assert (w[:work_shift // 4] == work_fill).all() and (w[(work_shift + need) // 4:] == work_fill).all(), "written outside the work buffer"
    out = _bits(dst)
    assert (out[:GUARD] == SENTINEL).all() and (out[GUARD + n * ldt_d:] == SENTINEL).all(), "guards of dst written"
    body = out[GUARD:GUARD + n * ldt_d].reshape(n, ldt_d)
    assert (body[:, H * ldh_d:] == SENTINEL).all(), "token padding of dst written"
    body = body[:, :H * ldh_d].reshape(n, H, ldh_d)
    assert (body[:, :, P:] == SENTINEL).all(), "head padding of dst written"
    for t, want in ((d_x, x), (d_bc, bc), (d_dt, dt), (d_A, A)):
        assert np.array_equal(_bits(t), want.view(np.uint32).reshape(-1)), "an input was written"
    return body[:, :, :P], _bits(d_pool)


def _batch_pool(c, pad):
    k = batch()
    H, P, N = c["H"], c["P"], c["N"]
    pool = Pool(k.n_slots, H * P * N, pad)
    for s in range(k.n_slots):
        pool.put(s, c["pool"][s])
    for b in range(k.n_seq):
        if k.d_len[b] == 0 and 0 <= k.slot[b] < k.n_slots:
            pool.put_nan(int(k.slot[b]))
    return pool


def _batch_call(dev, name, with_D=True, with_bias=True, c=None):
    """the batch call of a shape with strides of its own everywhere: the chunked sequences against float64 under the chunked bar, the short ones bit for bit
    the sequential entry's, then what tests/test_ssm.py _rows_and_pool_of_the_batch states.  -> (y, after, pool)"""
    k = batch()
    c = case(name) if c is None else c
    H, P, N = c["H"], c["P"], c["N"]
    elems = H * P * N
    pool = _batch_pool(c, 8)
    pads = dict(pad_head=3, pad_tok=5, pad_bc=4, pad_head_d=1, pad_tok_d=2, pad_dt=3, pad_a=(4 if c["aps"] else 2), with_D=with_D, with_bias=with_bias)
    y, after = _call(dev, c, k.q_start, k.d_len, k.slot, pool, k.n_tokens_max, **pads)
    y_seq, after_seq = _call(dev, c, k.q_start, k.d_len, k.slot, pool, k.n_tokens_max, entry="sequential", **pads)
    rc, p = _plan(H, P, N, c["G"], int(c["aps"]), k.n_seq, k.n_tokens_max)
    for b in k.served:
        lo, hi = k.rows(b)
        if p.form == 1 or b in k.short:
            assert np.array_equal(y[lo:hi], y_seq[lo:hi]), ("rows of a sequential sequence", name, b)
            assert np.array_equal(pool.slot(after, int(k.slot[b])), pool.slot(after_seq, int(k.slot[b]))), ("state of a sequential sequence", name, b)
            continue
        ref_y, ref_h, bar_y, bar_h = ref(name, b, with_D, with_bias)[:4]
        got_y = y[lo:hi].view(F).astype(np.float64)
        got_h = pool.slot(after, int(k.slot[b])).view(F).astype(np.float64).reshape(H, P, N)
        ry, rh = _ratio(got_y, ref_y, bar_y), _ratio(got_h, ref_h, bar_h)
        print(f"{name} seq {b} ({k.counts[b]} tokens): kernel / bar  y {ry:.3f}  state {rh:.3f}")
        assert np.isfinite(got_y).all() and np.isfinite(got_h).all() and ry <= 1.0 and rh <= 1.0, (name, b, ry, rh)
    ts._rows_and_pool_of_the_batch(k, y, after, pool, elems)
    return y, after, pool


def _split_points():
    k = batch()
    m1 = k.Q * (k.smt // k.Q + 1)                                    # the first multiple of Q above seq_max_tokens: Q where seq_max_tokens < Q
    return m1, m1 + k.Q


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(SHAPES))
def test_chunked_scan_over_the_ragged_batch(dev, name):
    k, c = batch(), case(name)
    H, P, N = c["H"], c["P"], c["N"]
    elems = H * P * N
    y, after, pool = _batch_call(dev, name)
    # (i) + (iii): every chunked sequence alone -- n_seq = 1, another slot number in another pool, other strides, another n_tokens_max, and a work buffer at
    # another offset, of another size, prefilled with NaN bytes
    for b in k.chunked:
        lo, hi = k.rows(b)
        one = Pool(3, elems, 0)
        one.put(2, c["pool"][k.slot[b]]) if k.d_len[b] else one.put_nan(2)
        y1, after1 = _call(dev, c, [0, hi - lo], [k.d_len[b]], [2], one, hi - lo + 1, row0=lo, work_fill=NAN_BYTES, work_shift=48, work_extra=512)
        assert np.array_equal(y1[:hi - lo], y[lo:hi]), ("rows alone", name, b)
        assert np.array_equal(one.slot(after1, 2), pool.slot(after, int(k.slot[b]))), ("state alone", name, b)
    # (ii'): a sequence split at a multiple of Q, both parts longer than seq_max_tokens, gives the bits of one call
    m1, m2 = _split_points()
    T = m2 + k.smt + 4
    assert 2 + T <= k.n_tokens_max - 3 and m1 > k.smt and T - m2 > k.smt
    whole = Pool(2, elems, 4)
    whole.put(1, c["pool"][3])
    yw, endw = _call(dev, c, [0, T], [5], [1], whole, T, row0=2)
    for cut in (m1, m2):
        two = Pool(2, elems, 4)
        two.put(1, c["pool"][3])
        ya, mid = _call(dev, c, [0, cut], [5], [1], two, cut, row0=2, pad_head=1)
        two.image = mid
        yb, end = _call(dev, c, [0, T - cut], [5 + cut], [1], two, T - cut, row0=2 + cut, work_fill=NAN_BYTES)
        assert np.array_equal(np.concatenate([ya, yb]), yw), ("rows split", name, cut)
        assert np.array_equal(two.slot(end, 1), whole.slot(endw, 1)), ("state split", name, cut)


@pytest.mark.gpu
@pytest.mark.parametrize("with_D,with_bias", ((False, True), (True, False), (False, False)))
def test_chunked_scan_without_the_optional_operands(dev, with_D, with_bias):
    _batch_call(dev, "n48", with_D=with_D, with_bias=with_bias)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ("per_state_A", "P5"))
def test_a_shape_the_chunked_form_does_not_serve_is_the_sequential_entry(dev, kind):
    """per-state A and a head_dim that is no multiple of 16 are not refused: form 1, every sequence -- the long ones too -- bit for bit the old entry"""
    k = batch()
    s = dict(H=3, P=16, N=32, G=1, seed=311, aps=True) if kind == "per_state_A" else dict(H=3, P=5, N=32, G=3, seed=312, aps=False)
    rng = np.random.default_rng(s["seed"])
    n, H, P, N, G = k.n_tokens_max, s["H"], s["P"], s["N"], s["G"]
    c = dict(s, x=rng.normal(0, 1, (n, H, P)).astype(F), dt=(2.0 * rng.normal(0, 1, (n, H)) - 1.0).astype(F),
             A=(-np.exp(rng.uniform(-3.0, 2.5, (H, N) if s["aps"] else (H,)))).astype(F), B=rng.normal(0, 1, (n, G, N)).astype(F),
             C=rng.normal(0, 1, (n, G, N)).astype(F), D=rng.normal(0, 1, H).astype(F), dt_bias=(0.5 * rng.normal(0, 1, H)).astype(F),
             pool=rng.normal(0, 1, (k.n_slots, H, P, N)).astype(F))
    rc, p = _plan(H, P, N, G, int(s["aps"]), k.n_seq, k.n_tokens_max)
    assert rc == OK and p.form == 1 and p.work_bytes == 0
    _batch_call(dev, kind, c=c)


def _t(dev, a):
    return dev.torch.from_numpy(np.ascontiguousarray(a)).cuda()


@pytest.mark.gpu
def test_a_captured_step_follows_the_batch_and_no_tokens_is_accepted(dev):
    """a captured conv + chunked-scan step replayed after d_q_start, d_len and d_slot changed on the device: sequences move between the chunked and the
    sequential form in both directions.  Then n_tokens_max = 0"""
    torch = dev.torch
    k, c, cc = batch(), case("small"), ts.conv_case(64, 4)
    H, P, N, G = c["H"], c["P"], c["N"], c["G"]
    n = k.n_tokens_max
    t = functools.partial(_t, dev)
    x, dt, A, B, Cc, D, db = (t(c[key]) for key in ("x", "dt", "A", "B", "C", "D", "dt_bias"))
    rng = np.random.default_rng(77)
    cx, cw, cb = t(rng.normal(0, 1, (n, 64)).astype(F)), t(cc["w"]), t(cc["bias"])
    pool0, cpool0 = t(c["pool"].reshape(k.n_slots, -1)), t(rng.normal(0, 1, (k.n_slots, 3 * 64)).astype(F))
    work = torch.empty(dev.ssm_scan_chunked_work_size(H, P, N, G, False, k.n_seq, n), dtype=torch.uint8, device="cuda")
    # the second batch: the same bounds, the long sequences in front and split differently, slots permuted, fresh and continued swapped
    cnt2 = [2 * k.Q + 5, 1, k.smt + 1, 0, k.smt, 3, k.Q + 9, 2, k.smt + 2, 7, 1, 4]
    assert sum(cnt2) <= n
    q2 = np.concatenate([[0], np.cumsum(cnt2)]).astype(np.int32)
    len2 = np.array([0, 3, 1, 0, 2, 0, 0, 5, 1, 0, 2, 6], np.int32)
    slot2 = np.array([3, 1, 8, 6, -1, 0, 2, 9, k.n_slots, 4, 5, 7], np.int32)
    one = (k.q_start, k.d_len, k.slot)
    moved_down = [b for b in range(1, k.n_seq) if k.counts[b] > k.smt >= cnt2[b]]
    moved_up = [b for b in range(1, k.n_seq) if cnt2[b] > k.smt >= (k.counts[b] or 0)]
    assert moved_down and moved_up

    def step(q, ln, sl, pool, cpool, y, cy):
        dev.ssm_conv_ragged(cx, cw, q, ln, sl, cpool, bias=cb, act=True, out=cy)
        dev.ssm_scan_chunked_ragged(x, dt, A, B, Cc, q, ln, sl, pool, dt_bias=db, D=D, out=y, work=work)

    def fresh():
        return pool0.clone(), cpool0.clone(), torch.zeros_like(x), torch.zeros_like(cx)

    want = {}
    for key, (q, ln, sl) in (("one", one), ("two", (q2, len2, slot2))):
        pool, cpool, y, cy = fresh()
        work.fill_(255)
        step(t(q), t(ln), t(sl), pool, cpool, y, cy)
        torch.cuda.synchronize()
        want[key] = [_bits(v) for v in (pool, cpool, y, cy)]
    assert not all(np.array_equal(a, b) for a, b in zip(want["one"], want["two"]))
    d_q, d_l, d_s = t(k.q_start), t(k.d_len), t(k.slot)
    pool, cpool, y, cy = fresh()
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            step(d_q, d_l, d_s, pool, cpool, y, cy)
    torch.cuda.current_stream().wait_stream(s)
    for key, (q, ln, sl) in (("two", (q2, len2, slot2)), ("one", one)):
        d_q.copy_(t(q)), d_l.copy_(t(ln)), d_s.copy_(t(sl))
        for dst, src in zip((pool, cpool, y, cy), fresh()):
            dst.copy_(src)
        g.replay()
        torch.cuda.synchronize()
        for got, w in zip((pool, cpool, y, cy), want[key]):
            assert np.array_equal(_bits(got), w), key
    before = [_bits(v) for v in (pool, y)]
    dev.ssm_scan_chunked_ragged(x, dt, A, B, Cc, d_q, d_l, d_s, pool, dt_bias=db, D=D, n_tokens_max=0, out=y)
    torch.cuda.synchronize()
    for got, w in zip((pool, y), before):
        assert np.array_equal(_bits(got), w)


@pytest.mark.gpu
def test_the_python_face_on_the_views_of_a_mamba2_block(dev):
    """what a Mamba-2 block hands over (tests/test_ssm.py has the sequential twin): x, B and C as views of ONE [n_tokens, d_inner + 2 G N] tensor, dt and out as
    views of wider tensors, a pool with a slot stride above the slot, the work buffer left to the wrapper.  Every stride the wrapper derives is pinned: rows
    and slots are bit for bit those of the raw entry on contiguous copies"""
    torch = dev.torch
    k, name = batch(), "mamba2"
    c = case(name)
    H, P, N, G = c["H"], c["P"], c["N"], c["G"]
    d_inner, gn, elems, n = H * P, G * N, H * P * N, k.n_tokens_max
    t = functools.partial(_t, dev)
    d_q, d_l, d_s = t(k.q_start), t(k.d_len), t(k.slot)
    fresh = [int(k.slot[b]) for b in k.served if k.d_len[b] == 0]
    wide_pool = torch.full((k.n_slots, elems + 8), float("nan"), dtype=torch.float32, device="cuda")
    pool = wide_pool[:, :elems]
    pool.copy_(t(c["pool"].reshape(k.n_slots, -1)))
    pool.view(torch.int32)[fresh] = -1
    xBC = torch.cat([t(c["x"]).reshape(n, d_inner), t(c["B"]).reshape(n, gn), t(c["C"]).reshape(n, gn)], 1).contiguous()
    x = xBC[:, :d_inner].unflatten(1, (H, P))
    B = xBC[:, d_inner:d_inner + gn].unflatten(1, (G, N))
    Cc = xBC[:, d_inner + gn:].unflatten(1, (G, N))
    dt = torch.full((n, H + 3), 3.0e38, dtype=torch.float32, device="cuda")[:, :H]
    dt.copy_(t(c["dt"]))
    wide = torch.full((n, H, P + 8), float("nan"), dtype=torch.float32, device="cuda")
    wide.view(torch.int32).fill_(SENTINEL)
    out = wide[:, :, :P]
    assert (x.stride(0), x.stride(1), out.stride(0), out.stride(1), dt.stride(0), pool.stride(0)) == (d_inner + 2 * gn, P, H * (P + 8), P + 8, H + 3, elems + 8)
    got = dev.ssm_scan_chunked_ragged(x, dt, t(c["A"]), B, Cc, d_q, d_l, d_s, pool, dt_bias=t(c["dt_bias"]), D=t(c["D"]), out=out)
    torch.cuda.synchronize()
    assert got is out
    y, state = _bits(wide)[:, :, :P], _bits(pool.contiguous())
    assert (_bits(wide)[:, :, P:] == SENTINEL).all(), "the padding of out was written"
    raw_pool = _batch_pool(c, 0)
    y_raw, after = _call(dev, c, k.q_start, k.d_len, k.slot, raw_pool, n)
    owned = ts._rows_and_pool_of_the_batch(k, y_raw, after, raw_pool, elems)
    assert np.array_equal(y[owned], y_raw[owned]) and (y[~owned] == SENTINEL).all(), "rows"
    assert np.array_equal(state.reshape(-1), after[GUARD:GUARD + k.n_slots * elems]), "slots"
    p = dev.ssm_scan_chunked_plan(H, P, N, G, False, k.n_seq, n)
    assert (p.form, p.chunk, p.seq_max_tokens) == (2, k.Q, k.smt) and p.work_bytes == dev.ssm_scan_chunked_work_size(H, P, N, G, False, k.n_seq, n)
