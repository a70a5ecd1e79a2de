// kv_pack.h -- f32 values -> the bytes of a KV-cache row, THE statement every kernel that writes a cache shares (attn.hip kv_store_kernel,
// rope.hip rope_kv_store_kernel): Q8_0 is quantize.hip's statement of quantize_row_q8_0 (amax; d = amax / 127; id = d ? 1 / d : 0;
// q = rint(v * id); the library is built without contraction and with the correctly rounded division), bit for bit
// ggml_hip_quantize_rows_dev; F16 is IEEE round to nearest even by integer arithmetic (subnormals kept, overflow to inf, a NaN stays a NaN).
#pragma once
#include "common.h"

#ifdef __HIPCC__
__device__ __forceinline__ uint32_t f32_to_f16_bits(float f) {      // (Half)f, IEEE round to nearest even (quantize.hip's algorithm)
    const uint32_t x = __float_as_uint(f);
    const uint32_t sign = (x >> 16) & 0x8000u;
    const uint32_t exp = (x >> 23) & 0xFFu;
    uint32_t man = x & 0x7FFFFFu;
    if (exp == 0xFF) return man == 0 ? (sign | 0x7C00u) : (sign | 0x7C00u | 0x0200u | (man >> 13));
    const int e = (int)exp - 127 + 15;
    if (e >= 31) return sign | 0x7C00u;
    if (e <= 0) {
        if (e < -10) return sign;
        man |= 0x800000u;
        const int shift = 14 - e;
        uint32_t hm = man >> shift;
        const uint32_t rem = man & ((1u << shift) - 1u);
        const uint32_t halfway = 1u << (shift - 1);
        if (rem > halfway || (rem == halfway && (hm & 1u))) hm++;
        return sign | hm;
    }
    uint32_t half = ((uint32_t)e << 10) | (man >> 13);
    const uint32_t rem = man & 0x1FFFu;
    if (rem > 0x1000u || (rem == 0x1000u && (half & 1u))) half++;
    return sign | half;
}

// 32 values -> one block_q8_0 {f32 d; int8 qs[32]} at o (36 bytes, 4-byte aligned)
__device__ __forceinline__ void kv_pack_q8_0(const float (&v)[QK], uint32_t *o) {
    float amax = 0.0f;
#pragma unroll
    for (int l = 0; l < QK; ++l) amax = fmaxf(amax, fabsf(v[l]));
    const float d = amax / 127.0f;
    const float id = d != 0.0f ? 1.0f / d : 0.0f;
    uint32_t w[8] = {0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
    for (int l = 0; l < QK; ++l) {
        const int q = (int)rintf(v[l] * id);
        w[l / 4] |= ((uint32_t)q & 0xFFu) << (8 * (l & 3));
    }
    o[0] = __float_as_uint(d);
#pragma unroll
    for (int k = 0; k < 8; ++k) o[1 + k] = w[k];
}

// 4 values -> 4 halves (8 bytes)
__device__ __forceinline__ uint2 kv_pack_f16(float4 f) {
    uint2 o;
    o.x = f32_to_f16_bits(f.x) | (f32_to_f16_bits(f.y) << 16);
    o.y = f32_to_f16_bits(f.z) | (f32_to_f16_bits(f.w) << 16);
    return o;
}
#endif
