// iq4.hip -- IQ4_NL and IQ4_XS weights (upstream's two non-linear 4-bit types) as UNPINNED EXTRAS.
//
// The reference has no IQ types and no upstream source is vendored: what is built here follows the PUBLISHED upstream formats, restated in
// include/ggml_hip_ext.h (GGML_HIP_TYPE_IQ4_NL / _IQ4_XS) and in tests/np_iq4.py, which is the only checker ("parity unpinned", as for the
// k-quants in kquants.hip):
//     kv = { -127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113 }          (upstream kvalues_iq4nl)
//     block_iq4_nl = { half d; u8 qs[16] }                                   18 bytes per 32 weights
//         element j < 16: the low nibble of qs[j], element j + 16: its high nibble;  y = d * kv[idx]
//     block_iq4_xs = { half d; u16 scales_h; u8 scales_l[4]; u8 qs[128] }    136 bytes per 256 weights
//         sub-block ib < 8: ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 15) | (((scales_h >> 2 ib) & 3) << 4), its 32 elements on
//         qs[16 ib .. 16 ib + 15] in IQ4_NL's nibble order;  y = (d * (ls - 32)) * kv[idx], the product d * (ls - 32) first
// Neither needs a product kernel of its own:
//   * an IQ4_NL block after the codebook lookup IS a Q8_0 block of this project -- f32 d = the half d (exact), qs[j] = kv[idx_j] -- so the
//     upload writes Q8_0's planar form (the int8 planes and the f32 d plane) and the weight is a plain Q8_0 weight to the plan and to every
//     kernel (ggml_hip_weight::up_type alone remembers the type, for the download, ggml_hip_weight_type and the size queries);
//   * an IQ4_XS super-block is eight k-blocks of Q6_K's resident form (kquants.hip): int8 planes of kv[idx] and both per-16 scales of a
//     k-block equal to d * (ls - 32) (exact in f32: 11 + 6 significant bits), the 8 header bytes kept in a 16-byte slot for the download --
//     the Q3_K pattern: ext_type = IQ4_XS, Q6_K's plan, activations by the Q8_K rule.
// VALUE RANGE (the audit for IQ4_XS): the codebook reaches -127 and 113, where Q6_K / Q3_K / Q2_K stay in [-32, 31].  Every kernel that
// serves the two-scale int8 form takes the full int8 range as it is: gemv.hip GV_TYPE_I8X2 (v_dot4_i32_i8 into int32 sums), gemm_q.hip
// GQ_TYPE_I8X2, gemm_q8s.hip Q42 and gemm_qmp.hip TWO (v_mfma_i32_32x32x16_i8 into int32 accumulators).  None offsets, packs or narrows
// the weight bytes, and a 16-element sum is at most 16 * 127 * 128 < 2^24 in magnitude, so its conversion to f32 is exact as for Q6_K.
// No form needed a change.
#include "two_scale.h"

namespace {

constexpr int8_t IQ4_KV[16] = {-127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113};
constexpr uint32_t kv_word(int k) {
    return (uint32_t)(uint8_t)IQ4_KV[4 * k] | ((uint32_t)(uint8_t)IQ4_KV[4 * k + 1] << 8) | ((uint32_t)(uint8_t)IQ4_KV[4 * k + 2] << 16) |
           ((uint32_t)(uint8_t)IQ4_KV[4 * k + 3] << 24);
}

// kv[i] for a run-time i (0..15) from four packed words in registers: no table in memory, no scratch
__device__ __forceinline__ int iq4_kv(int i) {
    const uint32_t w = i < 8 ? (i < 4 ? kv_word(0) : kv_word(1)) : (i < 12 ? kv_word(2) : kv_word(3));
    return (int)(int8_t)(uint8_t)(w >> (8 * (i & 3)));
}

// the index of a codebook value (the planes hold only codebook values): the number of entries below it
__device__ __forceinline__ int iq4_index_of(int v) {
    int i = 0;
#pragma unroll
    for (int k = 0; k < 15; ++k) i += v > (int)IQ4_KV[k] ? 1 : 0;
    return i;
}

// upstream best_index_int8(16, kvalues_iq4nl, x): the nearest entry, a tie to the upper one (a NaN: 15)
__device__ __forceinline__ int iq4_best_index(float x) {
    if (x <= -127.0f) return 0;
    if (x >= 113.0f) return 15;
    int ml = 0, mu = 15;
    while (mu - ml > 1) {
        const int mav = (ml + mu) >> 1;
        if (x < (float)iq4_kv(mav)) mu = mav; else ml = mav;
    }
    return (x - (float)iq4_kv(mu - 1) < (float)iq4_kv(mu) - x) ? mu - 1 : mu;
}

__device__ __forceinline__ uint16_t f2h_exact(float f) {    // the inverse of h2f on its image: every half bit pattern comes back
    const uint32_t x = __float_as_uint(f);
    const uint32_t sign = (x >> 16) & 0x8000u, exp = (x >> 23) & 0xFFu, man = x & 0x7FFFFFu;
    if (exp == 0xFF) return (uint16_t)(sign | 0x7C00u | (man >> 13));
    if (exp == 0 && man == 0) return (uint16_t)sign;
    const int e = (int)exp - 127 + 15;
    if (e <= 0) return (uint16_t)(sign | (uint32_t)(fabsf(f) * 16777216.0f));   // a half subnormal: man * 2^-24
    return (uint16_t)(sign | ((uint32_t)e << 10) | (man >> 13));
}

// the 32 values of a block whose nibbles are q[0..15] (element t < 16: low nibble of q[t], t + 16: its high nibble) as the two int8
// planes of Q8_0's layout (plane h byte j = element 2 j + h)
__device__ __forceinline__ void iq4_planes(const uint8_t *q, uint32_t ev[4], uint32_t od[4]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { ev[i] = 0; od[i] = 0; }
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const int idx = t < 16 ? (q[t] & 15) : (q[t - 16] >> 4);
        const uint32_t byte = (uint32_t)(uint8_t)(int8_t)iq4_kv(idx) << (8 * ((t >> 1) & 3));
        if (t & 1) od[t >> 3] |= byte; else ev[t >> 3] |= byte;
    }
}

// the inverse: the two int8 planes of a block -> its 16 nibble bytes
__device__ __forceinline__ void iq4_nibbles(uint4 e4, uint4 o4, uint8_t *q) {
    const uint32_t ev[4] = {e4.x, e4.y, e4.z, e4.w}, od[4] = {o4.x, o4.y, o4.z, o4.w};
    uint32_t idx[32];
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const uint32_t w = (t & 1) ? od[t >> 3] : ev[t >> 3];
        idx[t] = (uint32_t)iq4_index_of((int)(int8_t)(uint8_t)(w >> (8 * ((t >> 1) & 3))));
    }
#pragma unroll
    for (int t = 0; t < 16; ++t) q[t] = (uint8_t)(idx[t] | (idx[t + 16] << 4));
}

__device__ __forceinline__ int iq4xs_code(const uint8_t *blk, int ib) {     // ls of sub-block ib (0..63)
    const uint32_t sh = (uint32_t)blk[2] | ((uint32_t)blk[3] << 8);
    return (int)(((uint32_t)(blk[4 + ib / 2] >> (4 * (ib % 2))) & 15u) | (((sh >> (2 * ib)) & 3u) << 4));
}

// ---- IQ4_NL: Q8_0's planar form -----------------------------------------------------------------------------------------------------------
// one thread per (row, k-block); rows fastest so the plane stores coalesce
__global__ void iq4nl_to_planar_kernel(const uint8_t *__restrict__ aos, uint64_t nb01, int64_t row_begin, int64_t rows, int64_t Mpad,
                                       uint8_t *__restrict__ qs, float *__restrict__ d) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = blockIdx.y;
    if (m >= rows) return;
    const uint8_t *blk = aos + (uint64_t)(row_begin + m) * nb01 + (uint64_t)b * 18;
    d[b * Mpad + m] = h2f((uint16_t)(blk[0] | ((uint16_t)blk[1] << 8)));
    uint8_t q[16];
#pragma unroll
    for (int t = 0; t < 16; ++t) q[t] = blk[2 + t];
    uint32_t ev[4], od[4];
    iq4_planes(q, ev, od);
    *(uint4 *)(qs + ((b * 2 + 0) * Mpad + m) * 16) = make_uint4(ev[0], ev[1], ev[2], ev[3]);
    *(uint4 *)(qs + ((b * 2 + 1) * Mpad + m) * 16) = make_uint4(od[0], od[1], od[2], od[3]);
}

// exact inverse: one thread per (row, k-block)
__global__ void planar_to_iq4nl_kernel(uint8_t *__restrict__ aos, uint64_t nb01, int64_t rows, int64_t Mpad, const uint8_t *__restrict__ qs,
                                       const float *__restrict__ d) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = blockIdx.y;
    if (m >= rows) return;
    uint8_t *blk = aos + (uint64_t)m * nb01 + (uint64_t)b * 18;
    const uint16_t h = f2h_exact(d[b * Mpad + m]);
    blk[0] = (uint8_t)h; blk[1] = (uint8_t)(h >> 8);
    uint8_t q[16];
    iq4_nibbles(*(const uint4 *)(qs + ((b * 2 + 0) * Mpad + m) * 16), *(const uint4 *)(qs + ((b * 2 + 1) * Mpad + m) * 16), q);
#pragma unroll
    for (int t = 0; t < 16; ++t) blk[2 + t] = q[t];
}

// ---- IQ4_XS: Q6_K's resident form (the planar Q4_2 form on int8 planes, both scales of a k-block equal); the converters are two_scale.h's ----
struct iq4xs_codec {
    static constexpr int BYTES = 136, QOFF = 8, QLEN = 128, HDR = 8, SLOT = 16;
    static constexpr bool MINS = false;
    static __device__ __forceinline__ int hdr_pos(int i) { return i; }                        // d, scales_h, scales_l[4]
    static __device__ __forceinline__ void scales(const uint8_t *blk, int ib, float &d0, float &d1) {
        d0 = d1 = h2f_at(blk) * (float)(iq4xs_code(blk, ib) - 32);                            // exact: 11 + 6 significant bits
    }
    static __device__ __forceinline__ int value(const uint8_t *blk, int ib, int t) {          // IQ4_NL's nibble order
        const uint8_t q = blk[8 + 16 * ib + (t & 15)];
        return iq4_kv(t < 16 ? (q & 15) : (q >> 4));
    }
    static __device__ __forceinline__ void put(uint32_t *q, int ib, int t, int v) {
        or_byte(q, 16 * ib + (t & 15), (uint32_t)iq4_index_of(v) << (4 * (t >> 4)));
    }
};

// ---- dequantize_row_iq4_nl of the published format: one thread per 32-element block ----------------------------------------------------------
__global__ void dequantize_iq4nl_kernel(const uint8_t *__restrict__ in, int64_t nkb, float *__restrict__ y) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nkb) return;
    const uint8_t *blk = in + k * 18, *q = blk + 2;
    const float dl = h2f_at(blk);
    float *o = y + k * 32;
#pragma unroll
    for (int t = 0; t < 16; ++t) {
        o[t] = dl * (float)iq4_kv(q[t] & 15);
        o[t + 16] = dl * (float)iq4_kv(q[t] >> 4);
    }
}

// ---- the device quantizer: upstream quantize_row_iq4_nl_impl without importance weights, ntry = 7 (restated in include/ggml_hip_ext.h;
// tests/np_iq4.py is the same steps).  Every float operation is a binary32 operation in the order written (-ffp-contract=off, correctly
// rounded division), nearest = round half to even.  One lane per 32-element block; for IQ4_XS the eight lanes of a super-block find its
// scale of largest magnitude by width-8 shuffles.
// a block's scale: the x^2-weighted least-squares fit of the codebook under the start scale max / 127, then under fifteen trial scales
__device__ __forceinline__ float iq4_block_scale(const float *v) {
    float amax = 0.0f, mx = 0.0f;
#pragma unroll
    for (int j = 0; j < 32; ++j) { const float ax = fabsf(v[j]); if (ax > amax) { amax = ax; mx = v[j]; } }   // the first of largest magnitude
    if (amax < 1e-15f) return 0.0f;
    auto sums = [&](float id, float &sumqx, float &sumq2) {
        sumqx = 0.0f; sumq2 = 0.0f;
#pragma unroll
        for (int j = 0; j < 32; ++j) {
            const float q = (float)iq4_kv(iq4_best_index(id * v[j]));
            const float w = v[j] * v[j];
            sumqx += (w * q) * v[j];
            sumq2 += (w * q) * q;
        }
    };
    float d = -mx / -127.0f;                                // -max / kv[0]
    float sumqx, sumq2;
    sums(1.0f / d, sumqx, sumq2);
    d = sumqx / sumq2;
    float best = d * sumqx;
    for (int itry = -7; itry <= 7; ++itry) {
        sums((float)(itry - 127) / mx, sumqx, sumq2);
        if (sumq2 > 0.0f && sumqx * sumqx > best * sumq2) { d = sumqx / sumq2; best = d * sumqx; }
    }
    return d;
}

template <bool XS>
__global__ __launch_bounds__(128) void quantize_iq4_kernel(const float *__restrict__ x, int64_t nkb, uint8_t *__restrict__ out) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = tid < nkb;
    const int64_t k = active ? tid : nkb - 1;               // (idle lanes of the last group shadow the last block: the shuffles want every lane)
    float v[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 t = ((const float4 *)(x + k * 32))[i];
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
    const float scale = iq4_block_scale(v);
    float id;                                               // the final codes: L[j] = best_index(id * x[j])
    uint8_t *q;
    if constexpr (XS) {
        // max_scale: the first sub-block scale of largest magnitude (upstream: `if (fabsf(d) > amax_scale)` from 0 -- a NaN never wins)
        const int ib = (int)(k & 7);
        const float a = fabsf(scale);
        float key = a > 0.0f ? a : 0.0f;
        int kidx = ib;
#pragma unroll
        for (int o = 1; o < 8; o <<= 1) {
            const float ok = __shfl_xor(key, o, 8);
            const int oi = __shfl_xor(kidx, o, 8);
            if (ok > key || (ok == key && oi < kidx)) { key = ok; kidx = oi; }
        }
        const float mxs = __shfl(scale, kidx, 8);
        const float max_scale = key > 0.0f ? mxs : 0.0f;
        const float D = -max_scale / 32.0f;
        const _Float16 dh = (_Float16)D;
        const float iD = D != 0.0f ? 1.0f / D : 0.0f;
        const float r = rintf(iD * scale);                  // (a NaN scale -- a fit that overflowed -- has nearest 0, as upstream's nearest_int gives)
        const int l = r == r ? (int)fminf(fmaxf(r, -32.0f), 31.0f) : 0;
        const float dl = D * (float)l;
        id = dl != 0.0f ? 1.0f / dl : 0.0f;
        uint8_t *blk = out + (k >> 3) * 136;
        q = blk + 8 + 16 * ib;
        int codes[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) codes[i] = __shfl(l + 32, i, 8);
        if (active && ib == 0) {
            const uint16_t hbits = __builtin_bit_cast(uint16_t, dh);
            uint32_t sh = 0;
#pragma unroll
            for (int i = 0; i < 8; ++i) sh |= (uint32_t)(codes[i] >> 4) << (2 * i);
            blk[0] = (uint8_t)hbits; blk[1] = (uint8_t)(hbits >> 8);
            blk[2] = (uint8_t)sh; blk[3] = (uint8_t)(sh >> 8);
#pragma unroll
            for (int i = 0; i < 4; ++i) blk[4 + i] = (uint8_t)((codes[2 * i] & 15) | ((codes[2 * i + 1] & 15) << 4));
        }
    } else {
        uint8_t *blk = out + k * 18;
        q = blk + 2;
        id = scale != 0.0f ? 1.0f / scale : 0.0f;
        if (active) {
            const uint16_t hbits = __builtin_bit_cast(uint16_t, (_Float16)scale);
            blk[0] = (uint8_t)hbits; blk[1] = (uint8_t)(hbits >> 8);
        }
    }
    if (active) {
#pragma unroll
        for (int t = 0; t < 16; ++t) q[t] = (uint8_t)(iq4_best_index(id * v[t]) | (iq4_best_index(id * v[t + 16]) << 4));
    }
}

}  // namespace

// ---- the four operations of the two types (wtypes.cpp's rows point here; type = GGML_HIP_TYPE_IQ4_NL or _IQ4_XS) ----
hipError_t launch_iq4_to_planar(int type, const uint8_t *aos, uint64_t nb01, int64_t row_begin, int64_t rows, ggml_hip_weight *w, hipStream_t st) {
    if (type == GGML_HIP_TYPE_IQ4_XS) return two_scale_to_planar<iq4xs_codec>(aos, nb01, row_begin, rows, w, st);
    if (rows <= 0 || w->nbk <= 0) return hipSuccess;
    dim3 grid((unsigned)((rows + 127) / 128), (unsigned)w->nbk);
    iq4nl_to_planar_kernel<<<grid, 128, 0, st>>>(aos, nb01, row_begin, rows, w->Mpad, w->qs, w->d);
    return hipGetLastError();
}

hipError_t launch_planar_to_iq4(const ggml_hip_weight *w, uint8_t *aos, hipStream_t st) {
    if (w->ext_type == GGML_HIP_TYPE_IQ4_XS) return planar_to_two_scale<iq4xs_codec>(w, aos, st);
    if (w->M <= 0 || w->nbk <= 0) return hipSuccess;
    dim3 grid((unsigned)((w->M + 127) / 128), (unsigned)w->nbk);
    planar_to_iq4nl_kernel<<<grid, 128, 0, st>>>(aos, (uint64_t)w->nbk * 18, w->M, w->Mpad, w->qs, w->d);
    return hipGetLastError();
}

hipError_t launch_dequantize_iq4(int type, const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st) {
    if (type == GGML_HIP_TYPE_IQ4_XS) return dequantize_two_scale<iq4xs_codec>(blocks, nrows, k, y, st);
    const int64_t nkb = nrows * (k / 32);
    if (nkb <= 0) return hipSuccess;
    dequantize_iq4nl_kernel<<<dim3((unsigned)((nkb + 127) / 128)), 128, 0, st>>>((const uint8_t *)blocks, nkb, y);
    return hipGetLastError();
}

hipError_t launch_quantize_iq4(int type, const float *x, int64_t nrows, int64_t k, void *blocks, hipStream_t st) {
    const int64_t nkb = nrows * (k / 32);
    if (nkb <= 0) return hipSuccess;
    const dim3 grid((unsigned)((nkb + 127) / 128));
    if (type == GGML_HIP_TYPE_IQ4_XS) quantize_iq4_kernel<true><<<grid, 128, 0, st>>>(x, nkb, (uint8_t *)blocks);
    else quantize_iq4_kernel<false><<<grid, 128, 0, st>>>(x, nkb, (uint8_t *)blocks);
    return hipGetLastError();
}
