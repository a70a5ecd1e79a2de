"""numpy restatement of the BF16 extension type (include/ggml_hip_ext.h GGML_HIP_TYPE_BF16): the one f32 -> bf16 rule, the exact
widening back, and the product sum_k bf16(w) * bf16(x) in f64.  Test infrastructure only."""
import numpy as np


def f32_to_bf16_bits(x):
    """f32 values (or uint32 bit patterns) -> uint16 bf16 bits: a NaN keeps its sign and high payload with the quiet bit set,
    anything else rounds to nearest even (subnormals kept, overflow to +-inf)"""
    u = np.asarray(x)
    u = (u.view(np.uint32) if u.dtype == np.float32 else u.astype(np.uint32)).astype(np.uint64)
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    rne = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    return np.where(nan, (u >> 16) | 0x0040, rne).astype(np.uint16)


def bf16_bits_to_f32(b):
    """uint16 bf16 bits -> f32, exactly"""
    return (np.asarray(b).astype(np.uint32) << 16).view(np.float32)


def round_bf16(x):
    """f32 -> the f32 value of its bf16 rounding"""
    return bf16_bits_to_f32(f32_to_bf16_bits(np.asarray(x, np.float32)))


def mul_mat_bf16(w_bits, x):
    """dst[N, M] = sum_k bf16(w)[m, k] * bf16(x)[n, k] in f64 (every product is exact in f64: 8-bit significands)"""
    w = bf16_bits_to_f32(w_bits).astype(np.float64)
    a = round_bf16(x).astype(np.float64)
    return a @ w.T
