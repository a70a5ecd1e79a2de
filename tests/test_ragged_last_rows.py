"""The last rows of a ragged step (include/ggml_hip_ext.h: ggml_hip_ragged_last_rows_dev; csrc/get_rows.hip, attn.cpp): the rows the LM head needs.

Yardstick: numpy indexing of the packed rows by d_q_start, compared as uint32 -- a copy has no rounding.  A sequence that is empty or not present
(bounds out of order, past n_tokens_max, negative) gets a row of +0.0f.  Shapes: K of one element, no multiple of 4, one workgroup's worth and more
than one (the 16-byte path covers 1024 elements per workgroup); strides at and above K; a destination that is not 16-byte aligned."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from ggmlsharp_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_SYMBOLS = ("ggml_hip_ragged_last_rows_dev",)
SENTINEL = 0x7FC00123                                               # a NaN no kernel here produces
OK, ERR_SHAPE, ERR_ARG = 0, -3, -4
FAKE = 0x1000                                                       # a non-null pointer no refusal may touch
GUARD = 64                                                          # elements
F = np.float32


def _p(x):
    return None if x is None else C.c_void_p(int(x))


# ---------------------------------------------------------------- CPU
def test_the_new_symbol_is_exported_and_declared_everywhere():
    L = _lib.lib()
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "ggml_hip_ext.h")).read(), flags=re.S)
    cs = open(os.path.join(ROOT, "integration", "GgmlHip.cs")).read()
    for name in NEW_SYMBOLS:
        assert hasattr(L, name), name
        assert re.search(r"\b%s\s*\(" % name, hdr), name
        assert name in _lib.HIP_SYMBOLS, name
        assert re.search(r"\b%s\s*\(" % name, cs), name


def _last_rc(x=FAKE, ldx=64, q_start=FAKE, n_seq=3, n_tokens_max=16, K=64, dst=FAKE, ldd=64):
    return _lib.lib().ggml_hip_ragged_last_rows_dev(_p(x), ldx, _p(q_start), n_seq, n_tokens_max, K, _p(dst), ldd, None)


def test_refusals_need_no_device():
    """(every call below is refused, or has K = 0 and returns before anything else: its pointers are no device memory, so none may get as far as a launch)"""
    rc = _last_rc
    for n_seq in (0, -1, 4097):
        assert rc(n_seq=n_seq) == ERR_SHAPE, n_seq
    assert rc(q_start=None) == ERR_ARG
    assert rc(q_start=FAKE + 2) == ERR_SHAPE
    assert rc(n_tokens_max=-1) == ERR_ARG
    assert rc(n_tokens_max=(1 << 20) + 1) == ERR_SHAPE
    assert rc(K=-1) == ERR_SHAPE
    assert rc(K=(1 << 24) + 1, ldx=1 << 25, ldd=1 << 25) == ERR_SHAPE
    assert rc(ldx=63) == ERR_SHAPE
    assert rc(ldd=63) == ERR_SHAPE
    assert rc(K=0, x=None, dst=None) == OK
    assert rc(x=None) == ERR_ARG
    assert rc(dst=None) == ERR_ARG
    assert rc(x=FAKE + 2) == ERR_SHAPE
    assert rc(dst=FAKE + 1) == ERR_SHAPE


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


def _sentinel(dev, n):
    torch = dev.torch
    return torch.full((n,), SENTINEL, dtype=torch.int32, device="cuda")


def _keeps_sentinel(dev, a):
    return bool((a.view(dev.torch.int32) == SENTINEL).all())


# counts of 1, 8 and 9; an empty sequence; bounds out of order; a bound past n_tokens_max; a negative start
N_TOKENS_MAX = 32
Q_START = np.array([0, 1, 9, 18, 18, 25, 22, 30, 40, -2, 5, 32], np.int32)
LAST = [0, 8, 17, None, 24, None, 29, None, None, None, 31]         # the row each sequence's line of dst holds; None: +0.0f


def test_the_case_is_what_it_says():
    assert len(LAST) == Q_START.size - 1
    for s, want in enumerate(LAST):
        qs, qe = int(Q_START[s]), int(Q_START[s + 1])
        assert (qe - 1 if 0 <= qs < qe <= N_TOKENS_MAX else None) == want, s
    assert [int(Q_START[s + 1] - Q_START[s]) for s in (0, 1, 2, 3)] == [1, 8, 9, 0]


@pytest.mark.gpu
@pytest.mark.parametrize("K", (1, 5, 64, 1028))
def test_last_rows_against_numpy(dev, K):
    torch = dev.torch
    n_seq = Q_START.size - 1
    rng = np.random.default_rng(11 + K)
    d_q = torch.from_numpy(Q_START.copy()).cuda()
    up = K + (-K) % 4                                                # K rounded up to a multiple of 4
    for ldx, ldd, off in ((K, K, 0), (K + 3, K + 4, 0), (up + 4, up + 8, 0), (up, up, 1)):
        x = rng.normal(0.0, 1.0, (N_TOKENS_MAX, ldx)).astype(F)
        x[:, K:] = F(3.0e38)                                         # padding columns: never copied
        x[LAST[1], 0] = F(-0.0)                                      # a copy keeps the sign of a zero
        d_x = torch.from_numpy(x).cuda()
        buf = _sentinel(dev, GUARD + off + (n_seq + 2) * ldd + GUARD)
        dst = buf.data_ptr() + 4 * (GUARD + off)                     # (off = 1: d_dst is 4-byte but not 16-byte aligned)
        rc = _lib.lib().ggml_hip_ragged_last_rows_dev(_p(d_x.data_ptr()), ldx, _p(d_q.data_ptr()), n_seq, N_TOKENS_MAX, K, _p(dst), ldd, _stream(dev))
        assert rc == 0, _lib.lib().ggml_hip_last_error()
        torch.cuda.synchronize()
        body = buf[GUARD + off:GUARD + off + (n_seq + 2) * ldd].view(n_seq + 2, ldd)
        assert _keeps_sentinel(dev, buf[:GUARD + off]) and _keeps_sentinel(dev, buf[GUARD + off + (n_seq + 2) * ldd:]), "guards written"
        assert _keeps_sentinel(dev, body[n_seq:]) and _keeps_sentinel(dev, body[:n_seq, K:]), "rows past n_seq or padding columns written"
        got = body[:n_seq, :K].cpu().numpy().view(np.uint32)
        want = np.stack([x[i, :K] if i is not None else np.zeros(K, F) for i in LAST]).view(np.uint32)
        assert np.array_equal(got, want), (K, ldx, ldd, off)
        assert np.array_equal(d_x.cpu().numpy().view(np.uint32), x.view(np.uint32)), "d_x written"


@pytest.mark.gpu
def test_the_python_face_a_captured_call_and_no_tokens_at_all(dev):
    torch = dev.torch
    n_seq = Q_START.size - 1
    rng = np.random.default_rng(5)
    x_np = rng.normal(0.0, 1.0, (N_TOKENS_MAX, 64)).astype(F)
    x = torch.from_numpy(x_np).cuda()
    d_q = torch.from_numpy(Q_START.copy()).cuda()
    want = np.stack([x_np[i] if i is not None else np.zeros(64, F) for i in LAST])
    out = dev.ragged_last_rows(x, d_q)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy().view(np.uint32), want.view(np.uint32))
    # captured once, replayed after d_q_start changed on the device: the gather follows it
    out2 = torch.zeros((n_seq, 64), device="cuda")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        g = torch.cuda.CUDAGraph()
        with torch.cuda.graph(g, stream=s):
            dev.ragged_last_rows(x, d_q, out=out2)
    torch.cuda.current_stream().wait_stream(s)
    q2 = np.arange(0, 2 * (n_seq + 1), 2, dtype=np.int32)            # every sequence two rows: the last rows are 1, 3, 5, ...
    d_q.copy_(torch.from_numpy(q2))
    g.replay()
    torch.cuda.synchronize()
    assert np.array_equal(out2.cpu().numpy().view(np.uint32), x_np[1:2 * n_seq:2].view(np.uint32))
    # n_tokens_max = 0: no sequence can hold a row, every line is +0.0f
    buf = _sentinel(dev, n_seq * 64)
    rc = _lib.lib().ggml_hip_ragged_last_rows_dev(_p(x.data_ptr()), 64, _p(d_q.data_ptr()), n_seq, 0, 64, _p(buf.data_ptr()), 64, _stream(dev))
    torch.cuda.synchronize()
    assert rc == 0 and not buf.cpu().numpy().any()
