// two_scale.h -- the converters of the two-scale resident form, written ONCE over a per-format codec (device code; kquants.hip, iq4.hip).
//
// The form (kquants.hip "Q6_K"): a super-block of 256 weights is eight 32-element k-blocks of the planar Q4_2 form on its int8 planes --
// plane h byte j of a k-block = element 2 j + h, as Q8_0's planes -- with the effective scale of the k-block's first 16 elements in the d
// plane and of its last 16 in the m plane, and the header bytes of the super-block in a slot of the khdr plane for the byte-exact
// download.  Q6_K, Q3_K, Q2_K (its block term) and IQ4_XS live in it; they differ only in where a super-block keeps its bits.
//
// A codec says that and nothing else:
//     BYTES                          a super-block in the file format
//     QOFF, QLEN                     its quant bytes [QOFF, QOFF + QLEN): everything put() writes (QLEN a multiple of 4)
//     HDR, SLOT, hdr_pos(i)          its HDR header bytes -- byte i at hdr_pos(i) -- kept in a khdr slot of SLOT bytes (16 or 32)
//     scales(blk, bq, d0, d1)        the two effective scales of k-block bq (0..7) of the super-block at blk (each exact in f32)
//     value(blk, bq, t)              element t (0..31) of that k-block as the int8 the planes hold
//     put(q, bq, t, v)               the inverse of value(): ORs v's bits into the quant bytes q (or_byte; byte i of q = byte QOFF + i of the super-block)
//     MINS, mins(blk, bq, m0, m1)    Q2_K alone: the dequantizer subtracts a min per 16 elements (no resident form carries it)
#pragma once
#include "common.h"

namespace {

__device__ __forceinline__ float h2f(uint16_t h) {          // IEEE binary16 -> binary32, exact (NaN payloads kept, nothing quieted)
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    if (exp == 0) return __uint_as_float(__float_as_uint((float)man * 5.9604644775390625e-08f) | sign);
    if (exp == 31) return __uint_as_float(sign | 0x7F800000u | (man << 13));
    return __uint_as_float(sign | ((exp + 112u) << 23) | (man << 13));
}
__device__ __forceinline__ float h2f_at(const uint8_t *p) { return h2f((uint16_t)(p[0] | ((uint16_t)p[1] << 8))); }   // (a half at any byte offset)

// byte i of a little-endian byte string held in words |= b
__device__ __forceinline__ void or_byte(uint32_t *q, int i, uint32_t b) { q[i >> 2] |= b << (8 * (i & 3)); }

// one thread per (row, k-block); rows fastest so the plane stores coalesce
template <class C>
__global__ void two_scale_to_planar_kernel(const uint8_t *__restrict__ aos, uint64_t nb01, int64_t row_begin, int64_t rows, int64_t Mpad,
                                           uint8_t *__restrict__ i8p, float *__restrict__ d, float *__restrict__ mm, uint8_t *__restrict__ khdr) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = blockIdx.y;
    if (m >= rows) return;
    const int64_t sb = b >> 3;
    const int bq = (int)(b & 7);
    const uint8_t *blk = aos + (uint64_t)(row_begin + m) * nb01 + (uint64_t)sb * C::BYTES;
    const int64_t pi = b * Mpad + m;
    float d0, d1;
    C::scales(blk, bq, d0, d1);
    d[pi] = d0;
    mm[pi] = d1;
    uint32_t ev[4] = {0, 0, 0, 0}, od[4] = {0, 0, 0, 0};
#pragma unroll
    for (int t = 0; t < 32; ++t) {
        const uint32_t byte = (uint32_t)(uint8_t)(int8_t)C::value(blk, bq, t) << (8 * ((t >> 1) & 3));
        if (t & 1) od[t >> 3] |= byte; else ev[t >> 3] |= byte;      // plane h byte j = element 2 j + h
    }
    *(uint4 *)(i8p + ((b * 2 + 0) * Mpad + m) * 16) = make_uint4(ev[0], ev[1], ev[2], ev[3]);
    *(uint4 *)(i8p + ((b * 2 + 1) * Mpad + m) * 16) = make_uint4(od[0], od[1], od[2], od[3]);
    if (bq == 0) {
        uint32_t h[C::SLOT / 4] = {};
#pragma unroll
        for (int i = 0; i < C::HDR; ++i) h[i >> 2] |= (uint32_t)blk[C::hdr_pos(i)] << (8 * (i & 3));
        uint4 *o = (uint4 *)(khdr + (sb * Mpad + m) * C::SLOT);
#pragma unroll
        for (int i = 0; i < C::SLOT / 16; ++i) o[i] = make_uint4(h[4 * i], h[4 * i + 1], h[4 * i + 2], h[4 * i + 3]);
    }
}

// exact inverse: one thread per (row, super-block); launched with 128 threads, and says so: the unrolled body keeps sixteen plane loads in flight
template <class C>
__global__ __launch_bounds__(128) void planar_to_two_scale_kernel(uint8_t *__restrict__ aos, uint64_t nb01, int64_t rows, int64_t Mpad, const uint8_t *__restrict__ i8p,
                                           const uint8_t *__restrict__ khdr) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t sb = blockIdx.y;
    if (m >= rows) return;
    uint8_t *blk = aos + (uint64_t)m * nb01 + (uint64_t)sb * C::BYTES;
    // the quant bytes are put together in registers (every loop unrolled: each index a constant) and stored once -- as ORs into global
    // memory the 96-byte Q3_K inverse took twice its time
    uint32_t q[C::QLEN / 4] = {};
#pragma unroll
    for (int bq = 0; bq < 8; ++bq) {
        const int64_t b = sb * 8 + bq;
#pragma unroll
        for (int hsel = 0; hsel < 2; ++hsel) {
            const uint4 w4 = *(const uint4 *)(i8p + ((b * 2 + hsel) * Mpad + m) * 16);
            const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
#pragma unroll
            for (int j = 0; j < 16; ++j) C::put(q, bq, 2 * j + hsel, (int)(int8_t)((w[j >> 2] >> (8 * (j & 3))) & 0xFFu));
        }
    }
#pragma unroll
    for (int i = 0; i < C::QLEN; ++i) blk[C::QOFF + i] = (uint8_t)(q[i >> 2] >> (8 * (i & 3)));   // (a super-block is only 2-byte aligned: bytes)
    const uint8_t *h = khdr + (sb * Mpad + m) * C::SLOT;
    for (int i = 0; i < C::HDR; ++i) blk[C::hdr_pos(i)] = h[i];
}

// the format's dequantize_row: one thread per (row-major) k-block of 32 outputs.  y = (its 16 elements' scale) * value, the scale's own
// product first; with mins (Q2_K) y = scale * value - min, one multiply then one subtract (no contraction: -ffp-contract=off)
template <class C>
__global__ void dequantize_two_scale_kernel(const uint8_t *__restrict__ in, int64_t nkb, float *__restrict__ y) {
    const int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (k >= nkb) return;
    const uint8_t *blk = in + (k >> 3) * C::BYTES;
    const int bq = (int)(k & 7);
    float d0, d1, m0 = 0.0f, m1 = 0.0f;
    C::scales(blk, bq, d0, d1);
    if constexpr (C::MINS) C::mins(blk, bq, m0, m1);
    float *o = y + k * 32;
    for (int t = 0; t < 32; ++t) {
        const float v = (float)C::value(blk, bq, t);
        if constexpr (C::MINS) o[t] = (t < 16 ? d0 : d1) * v - (t < 16 ? m0 : m1);
        else o[t] = (t < 16 ? d0 : d1) * v;
    }
}

template <class C>
hipError_t two_scale_to_planar(const uint8_t *aos, uint64_t nb01, int64_t row_begin, int64_t rows, ggml_hip_weight *w, hipStream_t st) {
    if (rows <= 0 || w->nbk <= 0) return hipSuccess;
    dim3 grid((unsigned)((rows + 127) / 128), (unsigned)w->nbk);
    two_scale_to_planar_kernel<C><<<grid, 128, 0, st>>>(aos, nb01, row_begin, rows, w->Mpad, w->i8p, w->d, w->m, w->khdr);
    return hipGetLastError();
}
template <class C>
hipError_t planar_to_two_scale(const ggml_hip_weight *w, uint8_t *aos, hipStream_t st) {
    if (w->M <= 0 || w->nbk <= 0) return hipSuccess;
    dim3 grid((unsigned)((w->M + 127) / 128), (unsigned)(w->nbk / 8));
    planar_to_two_scale_kernel<C><<<grid, 128, 0, st>>>(aos, (uint64_t)(w->nbk / 8) * C::BYTES, w->M, w->Mpad, w->i8p, w->khdr);
    return hipGetLastError();
}
template <class C>
hipError_t dequantize_two_scale(const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st) {
    const int64_t nkb = nrows * (k / 32);
    if (nkb <= 0) return hipSuccess;
    dequantize_two_scale_kernel<C><<<dim3((unsigned)((nkb + 127) / 128)), 128, 0, st>>>((const uint8_t *)blocks, nkb, y);
    return hipGetLastError();
}

}  // namespace
