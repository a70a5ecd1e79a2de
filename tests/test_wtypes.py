"""The table of weight types (ggmlsharp_amd/csrc/wtypes.cpp): what the library answers about a type id without a device, and -- on the
GPU -- the upload / download converters and the dequantizer of every extension type (and of two reference types) at a shape the per-type
round trips do not reach: M = 130 rows is one full 128-thread block of rows plus a partial one, K = 512 two super-blocks (the header-slot
stride and the super-block index of the converters), a host pitch wider than the row and a device shard that starts at an odd row."""
import ctypes as C

import numpy as np
import pytest

import np_bf16 as B
import np_iq4 as I
import np_kquants as KQ
import np_q2k as Q2
import np_q3k as Q3
import np_restatement as R
import test_iq4 as TI
import test_kquants as TK
import test_q2k as T2
import test_q3k as T3
from ggmlsharp_amd import _lib
from ggmlsharp_amd._lib import (BF16, BLCK_SIZE, F16, IQ4_NL, IQ4_XS, Q2_K, Q3_K, Q4_0, Q4_2, Q4_K, Q5_1, Q5_K, Q6_K, Q8_0, TYPE_SIZE)

gpu = pytest.mark.gpu
RNG = np.random.default_rng(1811)

# the documented (block elements, block bytes) of every accepted id: the tables of _lib plus the pairs the library alone sizes
SIZES = {t: (BLCK_SIZE[t], TYPE_SIZE[t]) for t in BLCK_SIZE}
SIZES.update({Q3_K: (256, 110), Q2_K: (256, 84), BF16: (1, 2), IQ4_NL: (32, 18), IQ4_XS: (256, 136)})
# extension id -> the type whose resident form (operand images, work size) it lives in; BF16 takes F16's answers
RESIDENT = {Q5_K: Q5_1, Q4_K: Q5_1, Q6_K: Q4_2, Q3_K: Q4_2, Q2_K: Q4_2, IQ4_XS: Q4_2, IQ4_NL: Q8_0, BF16: F16}


def test_every_accepted_id_has_its_documented_sizes_and_its_neighbours_have_none():
    L = _lib.lib()
    assert len(SIZES) == 13 + 8
    for t, (blck, size) in SIZES.items():
        assert (L.ggml_hip_blck_size(t), L.ggml_hip_type_size(t)) == (blck, size), t
    for t in (-1, 13, 109, 115, 121, 122, 124, 129, 131):
        assert (L.ggml_hip_blck_size(t), L.ggml_hip_type_size(t)) == (0, 0), t


def test_an_extension_type_answers_as_its_resident_type():
    L = _lib.lib()
    for t, r in RESIDENT.items():
        for K in (256, 4096):
            for N in (1, 5, 64, 300):
                assert L.ggml_hip_mul_mat_work_size(t, K, N) == L.ggml_hip_mul_mat_work_size(r, K, N), (t, K, N)
                assert L.ggml_hip_act_image_kind(t, K, N) == L.ggml_hip_act_image_kind(r, K, N), (t, K, N)


# ---------------------------------------------------------------- GPU: the converters of every type at M = 130, K = 512
M, K = 130, 512


def _f32_scales(n):
    return (RNG.standard_normal(n) * 0.01).astype(np.float32).view(np.uint8).reshape(-1, 4)


def _q4_0_blocks(nb):
    b = RNG.integers(0, 256, size=(nb, 20), dtype=np.uint8)
    b[:, 0:4] = _f32_scales(nb)
    return b


def _q8_0_blocks(nb):
    b = RNG.integers(0, 256, size=(nb, 36), dtype=np.uint8)
    b[:, 0:4] = _f32_scales(nb)
    return b


def _bf16_blocks(n):
    return RNG.integers(0, 65536, size=(n, 1), dtype=np.uint64).astype(np.uint16).view(np.uint8)      # every bit pattern, NaN payloads included


def _seeded(mod, make):
    """a per-type block helper of another test file, drawing from THIS file's generator: the blocks do not depend on which tests ran before"""
    def call(nb):
        keep, mod.RNG = mod.RNG, RNG
        try:
            return make(nb)
        finally:
            mod.RNG = keep
    return call


# type -> (raw blocks of the type, their restated dequantizer)
CASES = {
    Q5_K: (_seeded(TK, lambda nb: TK._random_blocks(nb, Q5_K)), KQ.dequantize_q5_K),
    Q4_K: (_seeded(TK, lambda nb: TK._random_blocks(nb, Q4_K)), KQ.dequantize_q4_K),
    Q6_K: (_seeded(TK, lambda nb: TK._random_blocks(nb, Q6_K)), KQ.dequantize_q6_K),
    Q3_K: (_seeded(T3, T3._random_blocks), Q3.dequantize_q3_K),
    Q2_K: (_seeded(T2, T2._random_blocks), Q2.dequantize_q2_K),
    BF16: (_bf16_blocks, lambda b: B.bf16_bits_to_f32(b.view(np.uint16))),
    IQ4_NL: (_seeded(TI, TI._nl_blocks), I.dequantize_iq4_nl),
    IQ4_XS: (_seeded(TI, TI._xs_blocks), I.dequantize_iq4_xs),
    Q4_0: (_q4_0_blocks, R.dequantize_q4_0),
    Q8_0: (_q8_0_blocks, R.dequantize_q8_0),
}


@pytest.fixture(scope="module")
def dev():
    from ggmlsharp_amd import device
    device.init(0)
    return device


def _download(L, h, nrows, rb):
    out = np.zeros((nrows, rb), np.uint8)
    _lib.check(L.ggml_hip_weight_download(h, out.ctypes.data_as(C.c_void_p), None), "ggml_hip_weight_download")
    return out


@gpu
@pytest.mark.parametrize("t", list(CASES))
def test_converters_past_one_block_of_rows_and_one_super_block(dev, t):
    import torch
    global RNG
    RNG = np.random.default_rng(1811 + t)                  # (per case: `-k` reproduces a failure with the same blocks)
    L = _lib.lib()
    make, dequantize = CASES[t]
    blck, size = SIZES[t]
    rb = size * (K // blck)
    rows = np.ascontiguousarray(make(M * K // blck)).reshape(M, rb)
    # 1. host rows with a pitch wider than the row (the bytes between the rows are not the library's to read into the weight)
    pitched = RNG.integers(0, 256, size=(M, rb + 32), dtype=np.uint8)
    pitched[:, :rb] = rows
    h = C.c_void_p()
    _lib.check(L.ggml_hip_weight_upload(t, pitched.ctypes.data_as(C.c_void_p), K, M, rb + 32, 0, M, None, C.byref(h)), "ggml_hip_weight_upload")
    try:
        assert L.ggml_hip_weight_type(h) == t and L.ggml_hip_weight_rows(h) == M and L.ggml_hip_weight_cols(h) == K
        assert np.array_equal(_download(L, h, M, rb), rows)
    finally:
        L.ggml_hip_weight_free(h)
    # 2. a shard from device memory that starts at an odd row: the converters' row_begin offset
    d_rows = torch.from_numpy(rows).cuda()
    shard = dev.Weight.from_device(t, d_rows, K, row_begin=1, row_end=130)
    assert np.array_equal(shard.download().reshape(129, rb), rows[1:130])
    shard.free()
    # 3. the dequantizer of the same blocks, bit for bit
    got = dev.dequantize_rows(t, d_rows.reshape(-1), K).cpu().numpy()
    want = np.asarray(dequantize(rows.reshape(-1, size)), np.float32).reshape(M, K)
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
