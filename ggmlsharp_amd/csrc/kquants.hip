// kquants.hip -- Q5_K (r4: and Q4_K, Q6_K; then Q3_K and Q2_K) weights (and the Q8_K activation rule) as an UNPINNED EXTRA.
//
// The reference has no k-quants (TypeDefinitions.cs:153-169 stops at Q8_1; `grep -i q5_K` over /root/reference finds
// nothing -- SURVEY 8(a) row K), BASELINE.json's north_star and config 4 name them anyway.  What is built here follows the
// PUBLISHED upstream format (ggml k_quants, June 2023; not vendored, not referenced by any project file of the reference):
//     block_q5_K = { half d; half dmin; u8 scales[12]; u8 qh[32]; u8 qs[128] }        176 bytes per 256 weights
//     w[e] = d * sc_j * q[e] - dmin * m_j,  j = e / 32, sc_j / m_j the 6-bit entries of scales[] (get_scale_min_k4),
//     q[e] = 4 low bits from qs (element 64 g + l: low nibble of qs[32 g + l], 64 g + 32 + l: its high nibble) + bit
//     (2 g) / (2 g + 1) of qh[l] as the fifth bit
//     block_q4_K = { half d; half dmin; u8 scales[12]; u8 qs[128] }                    144 bytes: the same without the fifth bits (q in 0..15)
//     block_q8_K = { float d; i8 qs[256]; i16 bsums[16] }: iscale = -128 / (the first element of largest magnitude),
//     q = min(127, round-half-even(iscale * x)), d = 1 / iscale
//     dot per super-block: (d * dy) * sum_j sc_j * <q_j, a_j>  -  (dmin * dy) * sum_j m_j * bsum_j
// There is NO oracle in the reference for any of it: tests/np_kquants.py restates the published algorithm and is the only
// checker ("parity unpinned", stated wherever Q5_K appears).
//
// Design: a 32-element sub-block of Q5_K IS a Q5_1 block with effective scale d * sc_j (exact in f32: 11 + 6 bits) and
// effective min -(dmin * m_j) (exact) -- only the bit layout differs.  So the upload re-lays a super-block out as eight
// k-blocks of the resident planar Q5_1 form (nibble plane, fifth-bit plane, scale plane, min plane), and every Q5_1
// kernel of the path -- the mat-vec, the f16-MFMA mat-mat with its K split, the int8-MFMA mat-mat -- serves it unchanged.
// The INIT phase quantizes the activations with the Q8_K rule (one scale per 256 elements, quantize.hip K1 with K8 =
// true) into the same operand images.  The 16 header bytes of every super-block are kept beside the planes so that a
// download returns the uploaded bytes.
// Q6_K and Q3_K (sixteen sub-blocks of 16 with a signed scale each, no min) live in the planar Q4_2 form on int8 planes instead --
// two scales per 32-element k-block -- and run the int8 kernels that take two scales per k-block; Q3_K's planes are exactly those of the
// Q6_K super-block it transcodes to (see the two sections below).  Q2_K's sub-blocks of 16 each carry a min as well, which no resident
// form has (the min-term products of the Q5_1 form are built per 32 elements): its block term lives in Q6_K's form and runs Q6_K's kernels,
// and its min term is subtracted behind the product by a pass of its own (the Q2_K section at the end).
#include "two_scale.h"

namespace {

// upstream get_scale_min_k4
__device__ __forceinline__ void scale_min_k4(int j, const uint8_t *q, uint32_t &sc, uint32_t &m) {
    if (j < 4) {
        sc = q[j] & 63u;
        m = q[j + 4] & 63u;
    } else {
        sc = (q[j + 4] & 0xFu) | ((uint32_t)(q[j - 4] >> 6) << 4);
        m = (q[j + 4] >> 4) | ((uint32_t)(q[j] >> 6) << 4);
    }
}

// one thread per (row, 32-element sub-block); rows fastest so the planar stores coalesce
// (Q5 = false: Q4_K -- 144-byte super-blocks, the nibbles straight behind the 16 header bytes, no fifth bits)
template <bool Q5>
__global__ void q5k_to_planar_kernel(const uint8_t *__restrict__ aos, uint64_t nb01, int64_t row_begin, int64_t rows, int64_t Mpad,
                                     uint8_t *__restrict__ qs, uint32_t *__restrict__ qh, float *__restrict__ d, float *__restrict__ mm,
                                     uint8_t *__restrict__ khdr) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t b = blockIdx.y;                           // k-block (32 elements)
    if (m >= rows) return;
    const int64_t sb = b >> 3;
    const int j = (int)(b & 7), g = j >> 1, hi = j & 1;
    const uint8_t *blk = aos + (uint64_t)(row_begin + m) * nb01 + (uint64_t)sb * (Q5 ? 176 : 144);
    const uint8_t *scales = blk + 4, *qhs = blk + 16, *ql = blk + (Q5 ? 48 : 16) + 32 * g;
    uint32_t sc, mn;
    scale_min_k4(j, scales, sc, mn);
    const float dd = h2f(*(const uint16_t *)blk), dmin = h2f(*(const uint16_t *)(blk + 2));
    const int64_t pi = b * Mpad + m;
    d[pi] = dd * (float)sc;                                 // exact: 11 + 6 significant bits
    mm[pi] = -(dmin * (float)mn);                           // the Q5_1 form adds its min: w = d q + m
    uint32_t w[4] = {0, 0, 0, 0}, hbits = 0;
#pragma unroll
    for (int l = 0; l < 32; ++l) {
        const uint32_t nib = hi ? (uint32_t)(ql[l] >> 4) : (uint32_t)(ql[l] & 15u);
        w[l >> 3] |= nib << (4 * (l & 7));                  // byte l/2 = element l | element l+1 << 4 (the Q5_1 plane's order)
        if constexpr (Q5) hbits |= (uint32_t)((qhs[l] >> j) & 1u) << l;
    }
    *(uint4 *)(qs + pi * 16) = make_uint4(w[0], w[1], w[2], w[3]);
    qh[pi] = hbits;
    if (j == 0) *(uint4 *)(khdr + (sb * Mpad + m) * 16) = make_uint4(((const uint32_t *)blk)[0], ((const uint32_t *)blk)[1],
                                                                     ((const uint32_t *)blk)[2], ((const uint32_t *)blk)[3]);
}

// exact inverse: one thread per (row, super-block)
template <bool Q5>
__global__ void planar_to_q5k_kernel(uint8_t *__restrict__ aos, uint64_t nb01, int64_t rows, int64_t Mpad, const uint8_t *__restrict__ qs,
                                     const uint32_t *__restrict__ qh, const uint8_t *__restrict__ khdr) {
    const int64_t m = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t sb = blockIdx.y;
    if (m >= rows) return;
    uint8_t *blk = aos + (uint64_t)m * nb01 + (uint64_t)sb * (Q5 ? 176 : 144);
    const uint4 h = *(const uint4 *)(khdr + (sb * Mpad + m) * 16);
    // (176-byte blocks are only 16-byte aligned when nb01 is: write bytes)
    const uint32_t hw[4] = {h.x, h.y, h.z, h.w};
    for (int i = 0; i < 16; ++i) blk[i] = (uint8_t)(hw[i >> 2] >> (8 * (i & 3)));
    uint8_t qhb[32];
    for (int l = 0; l < 32; ++l) qhb[l] = 0;
    for (int j = 0; j < 8; ++j) {
        const int64_t pi = (sb * 8 + j) * Mpad + m;
        const uint4 w4 = *(const uint4 *)(qs + pi * 16);
        const uint32_t w[4] = {w4.x, w4.y, w4.z, w4.w};
        const uint32_t hb = qh[pi];
        uint8_t *ql = blk + (Q5 ? 48 : 16) + 32 * (j >> 1);
        for (int l = 0; l < 32; ++l) {
            const uint32_t nib = (w[l >> 3] >> (4 * (l & 7))) & 15u;
            if (j & 1) ql[l] = (uint8_t)((ql[l] & 0x0Fu) | (nib << 4));
            else ql[l] = (uint8_t)nib;                      // (the even sub-block of a pair comes first: it initialises the byte)
            qhb[l] |= (uint8_t)(((hb >> l) & 1u) << j);
        }
    }
    if constexpr (Q5) for (int l = 0; l < 32; ++l) blk[16 + l] = qhb[l];
}

// dequantize_row_q5_K (Q5 = false: dequantize_row_q4_K) of the published format: one thread per (row-major) sub-block of 32 outputs
template <bool Q5>
__global__ void dequantize_q5k_kernel(const uint8_t *__restrict__ in, int64_t nsub, float *__restrict__ y) {
    const int64_t s = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= nsub) return;
    const uint8_t *blk = in + (s >> 3) * (Q5 ? 176 : 144);
    const int j = (int)(s & 7), g = j >> 1, hi = j & 1;
    uint32_t sc, mn;
    scale_min_k4(j, blk + 4, sc, mn);
    const float d1 = h2f(*(const uint16_t *)blk) * (float)sc, m1 = h2f(*(const uint16_t *)(blk + 2)) * (float)mn;
    const uint8_t *ql = blk + (Q5 ? 48 : 16) + 32 * g, *qhs = blk + 16;
    float *o = y + s * 32;
    for (int l = 0; l < 32; ++l) {
        const int q = (int)(hi ? (ql[l] >> 4) : (ql[l] & 15)) + (Q5 && ((qhs[l] >> j) & 1) ? 16 : 0);
        o[l] = d1 * (float)q - m1;                          // upstream: d1 * q - m1, one multiply then one subtract
    }
}

// ---- r4: a device quantizer for the two extension types --------------------------------------------------------------------------------
// quantize_row_q5_K_reference / _q4_K_reference of the published format (ggml k_quants, 2023-06), restated: per 32-element sub-block
// make_qkx1_quants(32, nmax, x, L, &min, 5) -- an affine code over [min(0, min x), max x], its scale refitted up to five times by least
// squares (scale = sum (x - min) l / sum l^2, min = mean(x - scale l) capped at 0) until no code changes; then the eight scales / mins of a
// super-block as 6-bit multiples of d = max scale / 63 and dmin = max min / 63 (halves), and the codes again under the ROUNDED scales:
// l = nearest((x + dmin m) / (d sc)) in 0..nmax.  Every float operation is a binary32 operation in the order written (the library is
// built with -ffp-contract=off), nearest = round half to even.  UNPINNED like the rest of the extension: tests/np_kquants.py restates the
// same steps and the device bytes are compared with its bytes; neither was run against upstream.
// Eight lanes per super-block (one sub-block each), the super-block's maxima and the bit transpositions by width-8 shuffles.
template <bool Q5>
__global__ void quantize_kq_kernel(const float *__restrict__ x, int64_t nsb, uint8_t *__restrict__ out) {
    constexpr int NMAX = Q5 ? 31 : 15, BYTES = Q5 ? 176 : 144;
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t sb_raw = tid >> 3;
    const bool active = sb_raw < nsb;
    const int64_t sb = active ? sb_raw : nsb - 1;           // (idle lanes of the last group shadow the last super-block: the shuffles want every lane)
    const int j = (int)(tid & 7);
    const float *xs = x + sb * 256 + 32 * j;
    float v[32];
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const float4 t = ((const float4 *)xs)[i];
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
    int L[32];
    float mn = v[0], mx = v[0];
#pragma unroll
    for (int i = 1; i < 32; ++i) { if (v[i] < mn) mn = v[i]; if (v[i] > mx) mx = v[i]; }
    float scale = 0.0f, the_min = 0.0f;
#pragma unroll
    for (int i = 0; i < 32; ++i) L[i] = -1;                 // (upstream compares with an uninitialised L on the first try: every code "changes")
    if (mx == mn) {
#pragma unroll
        for (int i = 0; i < 32; ++i) L[i] = 0;
    } else {
        if (mn > 0.0f) mn = 0.0f;
        float iscale = (float)NMAX / (mx - mn);
        scale = 1.0f / iscale;
        for (int itry = 0; itry < 5; ++itry) {
            float sumlx = 0.0f;
            int suml2 = 0;
            bool changed = false;
#pragma unroll
            for (int i = 0; i < 32; ++i) {
                int l = (int)rintf(iscale * (v[i] - mn));
                l = l < 0 ? 0 : l > NMAX ? NMAX : l;
                if (l != L[i]) { L[i] = l; changed = true; }
                sumlx += (v[i] - mn) * (float)l;
                suml2 += l * l;
            }
            scale = sumlx / (float)suml2;
            float sum = 0.0f;
#pragma unroll
            for (int i = 0; i < 32; ++i) sum += v[i] - scale * (float)L[i];
            mn = sum / 32.0f;
            if (mn > 0.0f) mn = 0.0f;
            iscale = 1.0f / scale;
            if (!changed) break;
        }
        the_min = -mn;
    }
    // the super-block's largest scale and min (upstream: `if (scale > max_scale)` from 0)
    float max_scale = scale > 0.0f ? scale : 0.0f, max_min = the_min > 0.0f ? the_min : 0.0f;
#pragma unroll
    for (int o = 1; o < 8; o <<= 1) {
        const float a = __shfl_xor(max_scale, o, 8), b = __shfl_xor(max_min, o, 8);
        if (a > max_scale) max_scale = a;
        if (b > max_min) max_min = b;
    }
    const float inv_scale = max_scale > 0.0f ? 63.0f / max_scale : 0.0f, inv_min = max_min > 0.0f ? 63.0f / max_min : 0.0f;
    int ls = (int)rintf(inv_scale * scale), lm = (int)rintf(inv_min * the_min);
    ls = (ls & 255) > 63 ? 63 : (ls & 255);                 // (upstream stores nearest_int in a uint8_t, then MIN(63, .))
    lm = (lm & 255) > 63 ? 63 : (lm & 255);
    const _Float16 dh = (_Float16)(max_scale / 63.0f), dminh = (_Float16)(max_min / 63.0f);
    const float dd = (float)dh * (float)ls;
    if (dd != 0.0f) {
        const float dm = (float)dminh * (float)lm;
#pragma unroll
        for (int i = 0; i < 32; ++i) {
            int l = (int)rintf((v[i] + dm) / dd);
            L[i] = l < 0 ? 0 : l > NMAX ? NMAX : l;
        }
    }
    uint8_t *blk = out + sb * BYTES;
    // header: d, dmin, scales[12] (lane 0, with every lane's ls / lm)
    int lsa[8], lma[8];
#pragma unroll
    for (int q = 0; q < 8; ++q) { lsa[q] = __shfl(ls, q, 8); lma[q] = __shfl(lm, q, 8); }
    if (active && j == 0) {
        *(uint16_t *)blk = __builtin_bit_cast(uint16_t, dh);
        *(uint16_t *)(blk + 2) = __builtin_bit_cast(uint16_t, dminh);
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            blk[4 + q] = (uint8_t)(lsa[q] | ((lsa[q + 4] >> 4) << 6));
            blk[8 + q] = (uint8_t)(lma[q] | ((lma[q + 4] >> 4) << 6));
            blk[12 + q] = (uint8_t)((lsa[q + 4] & 15) | ((lma[q + 4] & 15) << 4));
        }
    }
    // nibbles: sub-blocks 2g / 2g + 1 share the bytes qs[32 g ..]: the even lane writes both
    uint32_t lo[8];                                         // this lane's 32 low nibbles as bytes-to-be (four per word), and its fifth bits
    uint32_t hb = 0;
#pragma unroll
    for (int i = 0; i < 8; ++i) lo[i] = 0;
#pragma unroll
    for (int i = 0; i < 32; ++i) {
        lo[i >> 2] |= (uint32_t)(L[i] & 15) << (8 * (i & 3));
        hb |= (uint32_t)((L[i] >> 4) & 1) << i;
    }
    uint8_t *ql = blk + (Q5 ? 48 : 16) + 32 * (j >> 1);
#pragma unroll
    for (int i = 0; i < 8; ++i) {
        const uint32_t other = __shfl_xor(lo[i], 1, 8);     // (the odd lane's nibbles go to the high halves)
        if (active && !(j & 1)) ((uint32_t *)ql)[i] = lo[i] | (other << 4);
    }
    if constexpr (Q5) {                                     // qh[l] bit q = the fifth bit of element l of sub-block q: lane j writes bytes 4 j .. 4 j + 3
        uint32_t word = 0;
#pragma unroll
        for (int q = 0; q < 8; ++q) {
            const uint32_t h = __shfl(hb, q, 8);
#pragma unroll
            for (int b = 0; b < 4; ++b) word |= ((h >> (4 * j + b)) & 1u) << (8 * b + q);
        }
        if (active) ((uint32_t *)(blk + 16))[j] = word;
    }
}

// ---- r4: Q6_K ------------------------------------------------------------------------------------------------------------------------------
//     block_q6_K = { u8 ql[128]; u8 qh[64]; i8 scales[16]; half d }                    210 bytes per 256 weights
//     w[e] = d * scales[e / 16] * (q[e] - 32);  per half n of 128 elements and l < 32, element 128 n + 32 c + l has its low four bits in the
//     low (c < 2) or high (c >= 2) nibble of ql[64 n + 32 (c & 1) + l] and its two high bits in bits 2 c, 2 c + 1 of qh[32 n + l]
//     dot against Q8_K per super-block: (d * dy) * sum_j scales[j] * <q_j - 32, a_j>
// Resident form: a 32-element k-block is two 16-element sub-blocks with a scale each -- the structure of the reference's Q4_2 (two blocks per
// Q8_0 block, Ggml.cs:1217-1252) -- so a super-block becomes eight k-blocks of the planar Q4_2 form: int8 operand planes of q - 32 (the
// layout of Q8_0's planes), the first sub-block's effective scale d * sc (exact in f32: 11 + 8 bits) in the d plane, the second's in the m
// plane.  The int8 kernels that take two scales per k-block serve it (gemm_q8s.hip Q42, gemm_q.hip's int8-plane two-scale form); the
// nibble plane of the Q4_2 form stays empty.  32 header bytes per super-block (scales[16], d) are kept for the byte-exact download.
// The converters are two_scale.h's, over this codec.
struct q6k_codec {
    static constexpr int BYTES = 210, QOFF = 0, QLEN = 192, HDR = 18, SLOT = 32;
    static constexpr bool MINS = false;
    static __device__ __forceinline__ int hdr_pos(int i) { return 192 + i; }                  // scales[16], d
    static __device__ __forceinline__ void scales(const uint8_t *blk, int bq, float &d0, float &d1) {
        const int8_t *sc = (const int8_t *)(blk + 192);
        const float dd = h2f_at(blk + 208);
        d0 = dd * (float)sc[2 * bq];                        // exact: 11 + 8 significant bits
        d1 = dd * (float)sc[2 * bq + 1];
    }
    static __device__ __forceinline__ int value(const uint8_t *blk, int bq, int t) {
        const int n = bq >> 2, c = bq & 3;
        const uint8_t *ql = blk + 64 * n + 32 * (c & 1), *qh = blk + 128 + 32 * n;
        const uint32_t nib = c < 2 ? (uint32_t)(ql[t] & 15u) : (uint32_t)(ql[t] >> 4);
        return (int)(nib | (((uint32_t)(qh[t] >> (2 * c)) & 3u) << 4)) - 32;
    }
    static __device__ __forceinline__ void put(uint32_t *q, int bq, int t, int v) {
        const int n = bq >> 2, c = bq & 3;
        const uint32_t u = (uint32_t)(v + 32);
        or_byte(q, 64 * n + 32 * (c & 1) + t, c < 2 ? (u & 15u) : ((u & 15u) << 4));
        or_byte(q, 128 + 32 * n + t, (u >> 4) << (2 * c));
    }
};

// quantize_row_q6_K_reference with make_qx_quants in its plain form (no least-squares refinement of the sub-block scales: a VALID encoder of
// the published structure, stated as such in include/ggml_hip_ext.h; tests/np_kquants.py quantize_q6_K is the same steps): sixteen lanes per
// super-block, one sub-block each.
__global__ void quantize_q6k_kernel(const float *__restrict__ x, int64_t nsb, uint8_t *__restrict__ out) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t sb_raw = tid >> 4;
    const bool active = sb_raw < nsb;
    const int64_t sb = active ? sb_raw : nsb - 1;
    const int j = (int)(tid & 15);
    const float *xs = x + sb * 256 + 16 * j;
    float v[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 t = ((const float4 *)xs)[i];
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
    float amax = 0.0f, mx = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { const float ax = fabsf(v[i]); if (ax > amax) { amax = ax; mx = v[i]; } }
    const float iscale = amax != 0.0f ? -32.0f / mx : 0.0f;
    const float scale = amax != 0.0f ? 1.0f / iscale : 0.0f;
    int L[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        int l = (int)rintf(iscale * v[i]);
        l = l < -32 ? -32 : l > 31 ? 31 : l;
        L[i] = amax != 0.0f ? l + 32 : 0;
    }
    // the first sub-block scale of largest magnitude
    float best = fabsf(scale);
    int bidx = j;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const float ob = __shfl_xor(best, o, 16);
        const int oi = __shfl_xor(bidx, o, 16);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    const float max_scale = __shfl(scale, bidx, 16);
    const bool zero = best == 0.0f;
    const float isc = zero ? 0.0f : -128.0f / max_scale;
    const _Float16 dh = zero ? (_Float16)0.0f : (_Float16)(1.0f / isc);
    int sc = (int)rintf(isc * scale);
    sc = zero ? 0 : sc > 127 ? 127 : sc;
    const float dd = (float)dh * (float)sc;
    if (dd != 0.0f) {
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            int l = (int)rintf(v[i] / dd);
            l = l < -32 ? -32 : l > 31 ? 31 : l;
            L[i] = l + 32;
        }
    }
    if (zero) {
#pragma unroll
        for (int i = 0; i < 16; ++i) L[i] = 0;
    }
    uint8_t *blk = out + sb * 210;
    const int n = j >> 3, c = (j >> 1) & 3, half = j & 1;   // element 16 j + i = 128 n + 32 c + (16 half + i)
    uint32_t lo[4] = {0, 0, 0, 0}, hi[4] = {0, 0, 0, 0};    // sixteen bytes-to-be: low nibbles / the two high bits
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        lo[i >> 2] |= (uint32_t)(L[i] & 15) << (8 * (i & 3));
        hi[i >> 2] |= (uint32_t)(L[i] >> 4) << (8 * (i & 3));
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t plo = __shfl_xor(lo[k], 4, 16);      // the lane with c ^ 2: the other nibble of the same ql bytes
        const uint32_t h2 = __shfl_xor(hi[k], 2, 16), h4 = __shfl_xor(hi[k], 4, 16), h6 = __shfl_xor(hi[k], 6, 16);   // c ^ 1, c ^ 2, c ^ 3
        if (active && c < 2) {
            const uint32_t word = lo[k] | (plo << 4);
            uint8_t *q = blk + 64 * n + 32 * (c & 1) + 16 * half + 4 * k;
            q[0] = (uint8_t)word; q[1] = (uint8_t)(word >> 8); q[2] = (uint8_t)(word >> 16); q[3] = (uint8_t)(word >> 24);
        }
        if (active && c == 0) {
            const uint32_t word = hi[k] | (h2 << 2) | (h4 << 4) | (h6 << 6);
            uint8_t *q = blk + 128 + 32 * n + 16 * half + 4 * k;
            q[0] = (uint8_t)word; q[1] = (uint8_t)(word >> 8); q[2] = (uint8_t)(word >> 16); q[3] = (uint8_t)(word >> 24);
        }
    }
    if (active) {
        blk[192 + j] = (uint8_t)(int8_t)sc;
        if (j == 0) { const uint16_t hb = __builtin_bit_cast(uint16_t, dh); blk[208] = (uint8_t)hb; blk[209] = (uint8_t)(hb >> 8); }
    }
}

// ---- Q3_K ----------------------------------------------------------------------------------------------------------------------------------
//     block_q3_K = { u8 hmask[32]; u8 qs[64]; u8 scales[12]; half d }                  110 bytes per 256 weights
//     element e = 128 n + 32 s + l: v = ((qs[32 n + l] >> 2 s) & 3) + 4 ((hmask[l] >> (4 n + s)) & 1) - 4, in -4..3;  w[e] = (d * sc_{e / 16}) * v,
//     sc_j = code - 32, the 6-bit code's low nibble scales[j] & 15 (j < 8) / scales[j - 8] >> 4, its high two bits (scales[8 + j % 4] >> 2 (j / 4)) & 3
//     dot against Q8_K per super-block: (d * dy) * sum_j sc_j * <v_j, a_j>
// Resident form: Q6_K's, byte for byte.  A Q3_K super-block IS the Q6_K one with q6 = v + 32, scales[j] = sc_j and the same d, so k-block
// b = 4 n + s (elements 32 b .. 32 b + 31: bit b of hmask[l], bits 2 s, 2 s + 1 of qs[32 n + l]) becomes the two int8 planes of v and the
// scales d * sc_{2 b}, d * sc_{2 b + 1} (exact in f32: 11 + 6 significant bits); every kernel that serves Q6_K serves it unchanged.  The 14
// header bytes (scales[12], d) of a super-block are kept in a 16-byte slot; hmask and qs are rebuilt from the planes by the download.
__device__ __forceinline__ int q3k_scale(const uint8_t *scales, int j) {
    const int lo = j < 8 ? (scales[j] & 15) : (scales[j - 8] >> 4);
    return (lo | (((scales[8 + (j & 3)] >> (2 * (j >> 2))) & 3) << 4)) - 32;
}

struct q3k_codec {
    static constexpr int BYTES = 110, QOFF = 0, QLEN = 96, HDR = 14, SLOT = 16;
    static constexpr bool MINS = false;
    static __device__ __forceinline__ int hdr_pos(int i) { return 96 + i; }                   // scales[12], d
    static __device__ __forceinline__ void scales(const uint8_t *blk, int bq, float &d0, float &d1) {
        const float dd = h2f_at(blk + 108);
        d0 = dd * (float)q3k_scale(blk + 96, 2 * bq);       // exact: 11 + 6 significant bits
        d1 = dd * (float)q3k_scale(blk + 96, 2 * bq + 1);
    }
    static __device__ __forceinline__ int value(const uint8_t *blk, int bq, int t) {
        const int n = bq >> 2, s = bq & 3;
        return (int)((blk[32 + 32 * n + t] >> (2 * s)) & 3u) + 4 * (int)((blk[t] >> bq) & 1u) - 4;
    }
    static __device__ __forceinline__ void put(uint32_t *q, int bq, int t, int v) {
        const int n = bq >> 2, s = bq & 3;
        const uint32_t u = (uint32_t)(v + 4);               // 0..7
        or_byte(q, 32 + 32 * n + t, (u & 3u) << (2 * s));
        or_byte(q, t, (u >> 2) << bq);
    }
};

// quantize_row_q3_K_reference of the published format, restated (tests/np_q3k.py quantize_q3_K is the same steps): per sub-block of 16
// make_q3_quants(16, 4, x, L, true) -- codes l = nearest(-4 / max * x) in -4..3, then up to five passes that move one code at a time to
// nearest(x sl2 / slx) where that raises the x^2-weighted fit (slx^2 / sl2) -- its scale sumlx / suml2; the sixteen scales as 6-bit codes
// against d = half(max scale / -32); the codes again under the ROUNDED scales, l = nearest(x / (d sc)) in -4..3.  Every float operation a
// binary32 operation in the order written (-ffp-contract=off), nearest = round half to even.  Sixteen lanes per super-block, one sub-block
// each; the super-block's largest scale and the bit transpositions by width-16 shuffles.
__global__ void quantize_q3k_kernel(const float *__restrict__ x, int64_t nsb, uint8_t *__restrict__ out) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t sb_raw = tid >> 4;
    const bool active = sb_raw < nsb;
    const int64_t sb = active ? sb_raw : nsb - 1;           // (idle lanes of the last group shadow the last super-block: the shuffles want every lane)
    const int j = (int)(tid & 15);
    const float *xs = x + sb * 256 + 16 * j;
    float v[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 t = ((const float4 *)xs)[i];
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
    // make_q3_quants(16, nmax = 4, x, L, do_rmse = true)
    float amax = 0.0f, mx = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) { const float ax = fabsf(v[i]); if (ax > amax) { amax = ax; mx = v[i]; } }
    int L[16];
    float scale = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) L[i] = 0;                  // (an all-zero sub-block: codes 0, scale 0)
    if (amax != 0.0f) {
        const float iscale = -4.0f / mx;
        float sumlx = 0.0f, suml2 = 0.0f;
#pragma unroll
        for (int i = 0; i < 16; ++i) {
            const int l = (int)fminf(fmaxf(rintf(iscale * v[i]), -4.0f), 3.0f);
            L[i] = l;
            const float w = v[i] * v[i];
            sumlx += (w * v[i]) * (float)l;
            suml2 += (w * (float)l) * (float)l;
        }
        for (int itry = 0; itry < 5; ++itry) {
            int changed = 0;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float w = v[i] * v[i];
                float slx = sumlx - (w * v[i]) * (float)L[i];
                if (slx > 0.0f) {
                    float sl2 = suml2 - (w * (float)L[i]) * (float)L[i];
                    const int nl = (int)fminf(fmaxf(rintf((v[i] * sl2) / slx), -4.0f), 3.0f);   // (clamped before the conversion: slx may be tiny)
                    if (nl != L[i]) {
                        slx += (w * v[i]) * (float)nl;
                        sl2 += (w * (float)nl) * (float)nl;
                        if (sl2 > 0.0f && (slx * slx) * suml2 > (sumlx * sumlx) * sl2) { L[i] = nl; sumlx = slx; suml2 = sl2; ++changed; }
                    }
                }
            }
            if (!changed) break;
        }
#pragma unroll
        for (int i = 0; i < 16; ++i) L[i] += 4;
        scale = sumlx / suml2;
    }
    // the first sub-block scale of largest magnitude (upstream: `if (fabsf(scale) > amax)` from 0)
    float best = fabsf(scale);
    int bidx = j;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const float ob = __shfl_xor(best, o, 16);
        const int oi = __shfl_xor(bidx, o, 16);
        if (ob > best || (ob == best && oi < bidx)) { best = ob; bidx = oi; }
    }
    const float max_scale = __shfl(scale, bidx, 16);
    const bool zero = best == 0.0f;
    const float isc = zero ? 0.0f : -32.0f / max_scale;
    const _Float16 dh = zero ? (_Float16)0.0f : (_Float16)(1.0f / isc);
    const int code = zero ? 0 : (int)fminf(fmaxf(rintf(isc * scale), -32.0f), 31.0f) + 32;
    const float dd = (float)dh * (float)(code - 32);        // the scale as the stored bytes give it
    if (dd != 0.0f) {
#pragma unroll
        for (int i = 0; i < 16; ++i) L[i] = (int)fminf(fmaxf(rintf(v[i] / dd), -4.0f), 3.0f) + 4;
    }
    uint8_t *blk = out + sb * 110;
    // element 16 j + i = 128 n + 32 s + 16 h + i (j = 8 n + 2 s + h): its high bit is bit 4 n + s = j / 2 of hmask[16 h + i], its low two
    // bits go to bits 2 s, 2 s + 1 of qs[32 n + 16 h + i]
    const int n = j >> 3, s = (j >> 1) & 3, h = j & 1;
    uint32_t lo[4] = {0, 0, 0, 0}, hb = 0;                  // sixteen bytes-to-be of low bit pairs, sixteen high bits
#pragma unroll
    for (int i = 0; i < 16; ++i) {
        lo[i >> 2] |= (uint32_t)(L[i] & 3) << (8 * (i & 3));
        hb |= (uint32_t)(L[i] >> 2) << i;
    }
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t l2 = __shfl_xor(lo[k], 2, 16), l4 = __shfl_xor(lo[k], 4, 16), l6 = __shfl_xor(lo[k], 6, 16);   // s ^ 1, s ^ 2, s ^ 3
        if (active && s == 0) {
            const uint32_t word = lo[k] | (l2 << 2) | (l4 << 4) | (l6 << 6);
            uint8_t *q = blk + 32 + 32 * n + 16 * h + 4 * k;
            q[0] = (uint8_t)word; q[1] = (uint8_t)(word >> 8); q[2] = (uint8_t)(word >> 16); q[3] = (uint8_t)(word >> 24);
        }
    }
    uint32_t hw[4] = {0, 0, 0, 0};                          // hmask[16 h + i] bit q = the high bit of element i of sub-block 2 q + h
#pragma unroll
    for (int q = 0; q < 8; ++q) {
        const uint32_t hq = __shfl(hb, 2 * q + h, 16);
#pragma unroll
        for (int i = 0; i < 16; ++i) hw[i >> 2] |= ((hq >> i) & 1u) << (8 * (i & 3) + q);
    }
    int codes[16];
#pragma unroll
    for (int q = 0; q < 16; ++q) codes[q] = __shfl(code, q, 16);
    if (active && j < 2) {
#pragma unroll
        for (int i = 0; i < 16; ++i) blk[16 * h + i] = (uint8_t)(hw[i >> 2] >> (8 * (i & 3)));
    }
    if (active && j == 0) {
        uint32_t sc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
#pragma unroll
        for (int q = 0; q < 16; ++q) {
            if (q < 8) sc[q] |= (uint32_t)(codes[q] & 15);
            else sc[q - 8] |= (uint32_t)(codes[q] & 15) << 4;
            sc[8 + (q & 3)] |= (uint32_t)(codes[q] >> 4) << (2 * (q >> 2));
        }
#pragma unroll
        for (int i = 0; i < 12; ++i) blk[96 + i] = (uint8_t)sc[i];
        const uint16_t hbits = __builtin_bit_cast(uint16_t, dh);
        blk[108] = (uint8_t)hbits; blk[109] = (uint8_t)(hbits >> 8);
    }
}


// ---- Q2_K ----------------------------------------------------------------------------------------------------------------------------------
//     block_q2_K = { u8 scales[16]; u8 qs[64]; half d; half dmin }                       84 bytes per 256 weights
//     element e = 128 n + 32 s + l: q = (qs[32 n + l] >> 2 s) & 3 in 0..3;  w[e] = (d * sc_j) * q - dmin * m_j,  j = e / 16,
//     sc_j = scales[j] & 15, m_j = scales[j] >> 4
//     dot against Q8_K per super-block: (d * dy) * sum_j sc_j * <q_j, a_j>  -  (dmin * dy) * sum_j m_j * bsum_j
// Resident form: the block term (d * sc_j) * q IS a Q6_K super-block (q6 = q + 32, scales[j] = sc_j, the same d), so k-block b = 4 n + s
// becomes the two int8 planes of q and the scales d * sc_{2 b}, d * sc_{2 b + 1} (exact in f32: 11 + 4 significant bits) -- Q6_K's planes,
// and every Q6_K kernel computes the block term B unchanged.  The 32-byte header slot of a super-block holds scales[16], d and dmin (bytes
// 0..15, 16..17, 18..19): the download's header and the min pass's weight operand.
// The dequantizer subtracts the min as upstream does: dl * q - ml, one multiply then one subtract.
struct q2k_codec {
    static constexpr int BYTES = 84, QOFF = 16, QLEN = 64, HDR = 20, SLOT = 32;
    static constexpr bool MINS = true;
    static __device__ __forceinline__ int hdr_pos(int i) { return i < 16 ? i : 64 + i; }      // scales[16], then d and dmin (bytes 80..83)
    static __device__ __forceinline__ void scales(const uint8_t *blk, int bq, float &d0, float &d1) {
        const float dd = h2f_at(blk + 80);
        d0 = dd * (float)(blk[2 * bq] & 15);                // exact: 11 + 4 significant bits
        d1 = dd * (float)(blk[2 * bq + 1] & 15);
    }
    static __device__ __forceinline__ void mins(const uint8_t *blk, int bq, float &m0, float &m1) {
        const float dmin = h2f_at(blk + 82);
        m0 = dmin * (float)(blk[2 * bq] >> 4);
        m1 = dmin * (float)(blk[2 * bq + 1] >> 4);
    }
    static __device__ __forceinline__ int value(const uint8_t *blk, int bq, int t) {
        const uint8_t *qs = blk + 16 + 32 * (bq >> 2);
        return (int)((qs[t] >> (2 * (bq & 3))) & 3u);
    }
    static __device__ __forceinline__ void put(uint32_t *q, int bq, int t, int v) {
        or_byte(q, 32 * (bq >> 2) + t, ((uint32_t)v & 3u) << (2 * (bq & 3)));
    }
};

// quantize_row_q2_K_reference of the published format, restated (tests/np_q2k.py quantize_q2_K is the same steps): per sub-block of 16
// make_qkx1_quants(16, 3, x, L, &min, 5) (the steps of quantize_kq_kernel above over 16 elements); the sixteen scales and mins as 4-bit codes
// nearest(15 / max * v) against d = half(max scale / 15) and dmin = half(max min / 15) (0 where the maximum is 0); the codes again under the
// ROUNDED scales, l = nearest((x + dmin m) / (d sc)) in 0..3, where d sc != 0.  Every float operation a binary32 operation in the order
// written (-ffp-contract=off), nearest = round half to even.  Sixteen lanes per super-block, one sub-block each.
__global__ void quantize_q2k_kernel(const float *__restrict__ x, int64_t nsb, uint8_t *__restrict__ out) {
    const int64_t tid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t sb_raw = tid >> 4;
    const bool active = sb_raw < nsb;
    const int64_t sb = active ? sb_raw : nsb - 1;           // (idle lanes of the last group shadow the last super-block: the shuffles want every lane)
    const int j = (int)(tid & 15);
    const float *xs = x + sb * 256 + 16 * j;
    float v[16];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const float4 t = ((const float4 *)xs)[i];
        v[4 * i] = t.x; v[4 * i + 1] = t.y; v[4 * i + 2] = t.z; v[4 * i + 3] = t.w;
    }
    // make_qkx1_quants(16, nmax = 3, x, L, &the_min, ntry = 5)
    int L[16];
    float mn = v[0], mx = v[0];
#pragma unroll
    for (int i = 1; i < 16; ++i) { if (v[i] < mn) mn = v[i]; if (v[i] > mx) mx = v[i]; }
    float scale = 0.0f, the_min = 0.0f;
#pragma unroll
    for (int i = 0; i < 16; ++i) L[i] = -1;                 // (upstream compares with an uninitialised L on the first try: every code "changes")
    if (mx == mn) {
#pragma unroll
        for (int i = 0; i < 16; ++i) L[i] = 0;
    } else {
        if (mn > 0.0f) mn = 0.0f;
        float iscale = 3.0f / (mx - mn);
        scale = 1.0f / iscale;
        for (int itry = 0; itry < 5; ++itry) {
            float sumlx = 0.0f;
            int suml2 = 0;
            bool changed = false;
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                int l = (int)fminf(fmaxf(rintf(iscale * (v[i] - mn)), 0.0f), 3.0f);
                if (l != L[i]) { L[i] = l; changed = true; }
                sumlx += (v[i] - mn) * (float)l;
                suml2 += l * l;
            }
            scale = sumlx / (float)suml2;
            float sum = 0.0f;
#pragma unroll
            for (int i = 0; i < 16; ++i) sum += v[i] - scale * (float)L[i];
            mn = sum / 16.0f;
            if (mn > 0.0f) mn = 0.0f;
            iscale = 1.0f / scale;
            if (!changed) break;
        }
        the_min = -mn;
    }
    // the super-block's largest scale and min (upstream: `if (scale > max_scale)` from 0)
    float max_scale = scale > 0.0f ? scale : 0.0f, max_min = the_min > 0.0f ? the_min : 0.0f;
#pragma unroll
    for (int o = 1; o < 16; o <<= 1) {
        const float a = __shfl_xor(max_scale, o, 16), b = __shfl_xor(max_min, o, 16);
        if (a > max_scale) max_scale = a;
        if (b > max_min) max_min = b;
    }
    int ls = 0, lm = 0;
    _Float16 dh = (_Float16)0.0f, dminh = (_Float16)0.0f;
    if (max_scale > 0.0f) {
        ls = (int)fminf(fmaxf(rintf((15.0f / max_scale) * scale), 0.0f), 15.0f);
        dh = (_Float16)(max_scale / 15.0f);
    }
    if (max_min > 0.0f) {
        lm = (int)fminf(fmaxf(rintf((15.0f / max_min) * the_min), 0.0f), 15.0f);
        dminh = (_Float16)(max_min / 15.0f);
    }
    const float dd = (float)dh * (float)ls;
    if (dd != 0.0f) {
        const float dm = (float)dminh * (float)lm;
#pragma unroll
        for (int i = 0; i < 16; ++i) L[i] = (int)fminf(fmaxf(rintf((v[i] + dm) / dd), 0.0f), 3.0f);
    }
    uint8_t *blk = out + sb * 84;
    // element 16 j + i = 128 n + 32 s + 16 h + i (j = 8 n + 2 s + h): its two bits go to bits 2 s, 2 s + 1 of qs[32 n + 16 h + i]
    const int n = j >> 3, s = (j >> 1) & 3, h = j & 1;
    uint32_t lo[4] = {0, 0, 0, 0};                          // sixteen bytes-to-be of bit pairs
#pragma unroll
    for (int i = 0; i < 16; ++i) lo[i >> 2] |= (uint32_t)(L[i] & 3) << (8 * (i & 3));
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        const uint32_t l2 = __shfl_xor(lo[k], 2, 16), l4 = __shfl_xor(lo[k], 4, 16), l6 = __shfl_xor(lo[k], 6, 16);   // s ^ 1, s ^ 2, s ^ 3
        if (active && s == 0) {
            const uint32_t word = lo[k] | (l2 << 2) | (l4 << 4) | (l6 << 6);
            uint8_t *q = blk + 16 + 32 * n + 16 * h + 4 * k;
            q[0] = (uint8_t)word; q[1] = (uint8_t)(word >> 8); q[2] = (uint8_t)(word >> 16); q[3] = (uint8_t)(word >> 24);
        }
    }
    if (active) {
        blk[j] = (uint8_t)(ls | (lm << 4));
        if (j == 0) {
            const uint16_t hd = __builtin_bit_cast(uint16_t, dh), hm = __builtin_bit_cast(uint16_t, dminh);
            blk[80] = (uint8_t)hd; blk[81] = (uint8_t)(hd >> 8); blk[82] = (uint8_t)hm; blk[83] = (uint8_t)(hm >> 8);
        }
    }
}

// ---- the Q2_K min pass ---------------------------------------------------------------------------------------------------------------------
// Behind the product B of the block term (any family Q6_K's plan picks), in place:  dst[n][i] = fl(B[n][i] - T[n][i]) with T the min term
// against K1's int8 image by the Q8_K rule (dy = the image's `ad` entry of the super-block's first k-block -- K1 writes the one super-block
// scale d = 1 / iscale into all eight; bsum_j = the sum of the 16 quants of sub-block j: k-block 8 sb + j / 2, bytes 8 (j % 2) .. + 7 of both
// planes).  Per output (n, i), fixed whatever the geometry, the family, M or the shard:
//
//     acc = +0.0f
//     for sb = 0 .. K / 256 - 1 (ascending):
//         S   = sum_j m_j * bsum_j             (|bsum| <= 2048, m <= 15: |S| < 2^19, every partial sum an integer below 2^24 -- exact in
//                                               f32 in any order, so one v_mfma_f32_32x32x16_f16 per 32 x 32 tile with m and bsum as f16)
//         c   = fl(dy[n, sb] * dmin[i, sb])
//         acc = fl(acc + fl(c * (float)S))
//     dst[n, i] = fl(dst[n, i] - acc)          (no fma contraction anywhere: -ffp-contract=off)
//
// The bits depend on (K, N) and the operands alone, so row shards, the K3s / K3p switch and the two-phase entries stay bitwise consistent.
// Geometry: a workgroup of four waves owns 32 activation rows (n) x 128 TPW weight rows (i); wave w its TPW 32 x 32 tiles.  The super-blocks
// go in chunks of CH: the workgroup sums the 32 rows' bsums of a chunk once into LDS (f16, the MFMA's A operand: row n, k = j), then each
// lane loads its weight rows' slots of the chunk (scales[16] >> 4 as f16, the B operand: k = j, column i; dmin) and the chunk's products
// follow in ascending order.  The next chunk's activation loads are in flight during this chunk's products; the weight-slot loads are not,
// and at 256 VGPRs (one wave per SIMD) the pass is latency-bound.  Workgroups of one XCD take consecutive tiles (n-tile
// major), so that the activation rows they share can stay in that XCD's L2.
using q2_f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using q2_f32x16 = __attribute__((ext_vector_type(16))) float;

__device__ __forceinline__ uint32_t q2_f16_bits(int v) { return (uint32_t)__builtin_bit_cast(uint16_t, (_Float16)(float)v); }   // exact: |v| <= 2048

template <int TPW, int Q2_CH>
__global__ __launch_bounds__(256) void q2k_min_pass_kernel(const uint8_t *__restrict__ khdr, int64_t Mpad, int64_t M, int64_t nsb,
                                                           const int8_t *__restrict__ a8, const float *__restrict__ ad, int64_t Npad, int64_t N,
                                                           float *__restrict__ dst, int64_t ldd, int64_t ntiles_i, int64_t ntiles, int64_t per_xcd) {
    const int64_t tile = (int64_t)(blockIdx.x & 7) * per_xcd + (blockIdx.x >> 3);   // (workgroups go to the eight XCDs in turn)
    if (tile >= ntiles) return;
    const int64_t n0 = tile / ntiles_i * 32, i0 = tile % ntiles_i * (128 * TPW);
    __shared__ __attribute__((aligned(16))) uint32_t s_bsum[Q2_CH][32][8];   // [super-block of the chunk][row][j / 2]: bsum_j, bsum_j+1 as f16
    __shared__ __attribute__((aligned(16))) float s_dy[Q2_CH][32];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, h = lane >> 5;
    // the bsum role of this thread: row arow of the tile, k-block aq (sub-blocks 2 aq, 2 aq + 1) of every super-block of a chunk
    const int arow = tid & 31, aq = tid >> 5;
    const int64_t an = n0 + arow;
    const bool alive = an < N;                              // (rows past N: K1 wrote nothing there)
    uint4 ev[Q2_CH], od[Q2_CH];
    float dyv[Q2_CH];
    auto load_act = [&](int64_t c0) {
#pragma unroll
        for (int u = 0; u < Q2_CH; ++u) {
            const int64_t sb = c0 + u;
            ev[u] = od[u] = make_uint4(0u, 0u, 0u, 0u);
            dyv[u] = 0.0f;
            if (alive && sb < nsb) {
                const int64_t b = sb * 8 + aq;
                ev[u] = *(const uint4 *)(a8 + ((b * 2 + 0) * Npad + an) * 16);
                od[u] = *(const uint4 *)(a8 + ((b * 2 + 1) * Npad + an) * 16);
                if (aq == 0) dyv[u] = ad[(sb * 8) * Npad + an];
            }
        }
    };
    q2_f32x16 acc[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t)
#pragma unroll
        for (int e = 0; e < 16; ++e) acc[t][e] = 0.0f;
    int64_t col[TPW];
#pragma unroll
    for (int t = 0; t < TPW; ++t) col[t] = i0 + (int64_t)(wave * TPW + t) * 32 + r;
    load_act(0);
    for (int64_t c0 = 0; c0 < nsb; c0 += Q2_CH) {
        const int ones = 0x01010101;
#pragma unroll
        for (int u = 0; u < Q2_CH; ++u) {
            int s0 = __builtin_amdgcn_sdot4((int)ev[u].x, ones, 0, false);
            s0 = __builtin_amdgcn_sdot4((int)ev[u].y, ones, s0, false);
            s0 = __builtin_amdgcn_sdot4((int)od[u].x, ones, s0, false);
            s0 = __builtin_amdgcn_sdot4((int)od[u].y, ones, s0, false);
            int s1 = __builtin_amdgcn_sdot4((int)ev[u].z, ones, 0, false);
            s1 = __builtin_amdgcn_sdot4((int)ev[u].w, ones, s1, false);
            s1 = __builtin_amdgcn_sdot4((int)od[u].z, ones, s1, false);
            s1 = __builtin_amdgcn_sdot4((int)od[u].w, ones, s1, false);
            s_bsum[u][arow][aq] = q2_f16_bits(s0) | (q2_f16_bits(s1) << 16);
            if (aq == 0) s_dy[u][arow] = dyv[u];
        }
        __syncthreads();
        load_act(c0 + Q2_CH);                               // (the next chunk's activations, in flight during this chunk's products)
        uint2 sc[TPW][Q2_CH];
        uint32_t dmb[TPW][Q2_CH];
#pragma unroll
        for (int t = 0; t < TPW; ++t)
#pragma unroll
            for (int u = 0; u < Q2_CH; ++u) {
                sc[t][u] = make_uint2(0u, 0u);
                dmb[t][u] = 0;
                if (col[t] < M && c0 + u < nsb) {
                    const uint8_t *slot = khdr + ((c0 + u) * Mpad + col[t]) * 32;
                    sc[t][u] = *(const uint2 *)(slot + 8 * h);              // scales[8 h .. 8 h + 7]
                    dmb[t][u] = *(const uint16_t *)(slot + 18);
                }
            }
#pragma unroll
        for (int u = 0; u < Q2_CH; ++u) {
            if (c0 + u >= nsb) break;                       // (uniform over the workgroup)
            const uint4 av = *(const uint4 *)&s_bsum[u][r][4 * h];          // A[row r][k = 8 h + jj] = bsum_{8 h + jj} of row n0 + r
            const q2_f16x8 a = __builtin_bit_cast(q2_f16x8, av);
            float dy[16];                                   // the rows of this lane's accumulators: (e & 3) + 8 (e >> 2) + 4 h
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                const float4 d4 = *(const float4 *)&s_dy[u][8 * g + 4 * h];
                dy[4 * g] = d4.x; dy[4 * g + 1] = d4.y; dy[4 * g + 2] = d4.z; dy[4 * g + 3] = d4.w;
            }
#pragma unroll
            for (int t = 0; t < TPW; ++t) {
                const float dmin = h2f((uint16_t)dmb[t][u]);
                q2_f16x8 bm;                                // B[k = 8 h + jj][column r] = m_{8 h + jj} = scales[8 h + jj] >> 4
#pragma unroll
                for (int jj = 0; jj < 8; ++jj) bm[jj] = (_Float16)(float)(((jj < 4 ? sc[t][u].x : sc[t][u].y) >> (8 * (jj & 3) + 4)) & 15u);
                q2_f32x16 zero;
#pragma unroll
                for (int e = 0; e < 16; ++e) zero[e] = 0.0f;
                const q2_f32x16 S = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, bm, zero, 0, 0, 0);
#pragma unroll
                for (int e = 0; e < 16; ++e) {
                    const float c = dy[e] * dmin;
                    acc[t][e] = acc[t][e] + c * S[e];
                }
            }
        }
        __syncthreads();                                    // (the LDS of this chunk is read before the next chunk's sums overwrite it)
    }
#pragma unroll
    for (int t = 0; t < TPW; ++t) {
        if (col[t] >= M) continue;
#pragma unroll
        for (int e = 0; e < 16; ++e) {
            const int64_t n = n0 + (e & 3) + 8 * (e >> 2) + 4 * h;
            if (n < N) {
                float *o = dst + n * ldd + col[t];
                *o = *o - acc[t][e];
            }
        }
    }
}

}  // namespace

// ---- the four operations of a k-quant type (wtypes.cpp's rows point here): Q5_K / Q4_K onto the planar Q5_1 form, the others through two_scale.h
hipError_t launch_kq_to_planar(int type, const uint8_t *aos, uint64_t nb01, int64_t row_begin, int64_t rows, ggml_hip_weight *w, hipStream_t st) {
    switch (type) {
    case GGML_HIP_TYPE_Q6_K: return two_scale_to_planar<q6k_codec>(aos, nb01, row_begin, rows, w, st);
    case GGML_HIP_TYPE_Q3_K: return two_scale_to_planar<q3k_codec>(aos, nb01, row_begin, rows, w, st);
    case GGML_HIP_TYPE_Q2_K: return two_scale_to_planar<q2k_codec>(aos, nb01, row_begin, rows, w, st);
    }
    if (rows <= 0) return hipSuccess;
    dim3 grid((unsigned)((rows + 127) / 128), (unsigned)w->nbk);
    if (type == GGML_HIP_TYPE_Q5_K) q5k_to_planar_kernel<true><<<grid, 128, 0, st>>>(aos, nb01, row_begin, rows, w->Mpad, w->qs, w->qh, w->d, w->m, w->khdr);
    else q5k_to_planar_kernel<false><<<grid, 128, 0, st>>>(aos, nb01, row_begin, rows, w->Mpad, w->qs, w->qh, w->d, w->m, w->khdr);
    return hipGetLastError();
}

hipError_t launch_planar_to_kq(const ggml_hip_weight *w, uint8_t *aos, hipStream_t st) {
    switch (w->ext_type) {
    case GGML_HIP_TYPE_Q6_K: return planar_to_two_scale<q6k_codec>(w, aos, st);
    case GGML_HIP_TYPE_Q3_K: return planar_to_two_scale<q3k_codec>(w, aos, st);
    case GGML_HIP_TYPE_Q2_K: return planar_to_two_scale<q2k_codec>(w, aos, st);
    }
    if (w->M <= 0) return hipSuccess;
    dim3 grid((unsigned)((w->M + 127) / 128), (unsigned)(w->nbk / 8));
    if (w->ext_type == GGML_HIP_TYPE_Q5_K) planar_to_q5k_kernel<true><<<grid, 128, 0, st>>>(aos, (uint64_t)(w->nbk / 8) * 176, w->M, w->Mpad, w->qs, w->qh, w->khdr);
    else planar_to_q5k_kernel<false><<<grid, 128, 0, st>>>(aos, (uint64_t)(w->nbk / 8) * 144, w->M, w->Mpad, w->qs, w->qh, w->khdr);
    return hipGetLastError();
}

hipError_t launch_dequantize_kq(int type, const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st) {
    switch (type) {
    case GGML_HIP_TYPE_Q6_K: return dequantize_two_scale<q6k_codec>(blocks, nrows, k, y, st);
    case GGML_HIP_TYPE_Q3_K: return dequantize_two_scale<q3k_codec>(blocks, nrows, k, y, st);
    case GGML_HIP_TYPE_Q2_K: return dequantize_two_scale<q2k_codec>(blocks, nrows, k, y, st);
    }
    const int64_t nsub = nrows * (k / 32);
    if (nsub <= 0) return hipSuccess;
    if (type == GGML_HIP_TYPE_Q5_K) dequantize_q5k_kernel<true><<<dim3((unsigned)((nsub + 127) / 128)), 128, 0, st>>>((const uint8_t *)blocks, nsub, y);
    else dequantize_q5k_kernel<false><<<dim3((unsigned)((nsub + 127) / 128)), 128, 0, st>>>((const uint8_t *)blocks, nsub, y);
    return hipGetLastError();
}

// x: contiguous rows, 16-byte aligned.  Q5_K / Q4_K: eight lanes per super-block, the others sixteen
hipError_t launch_quantize_kq(int type, const float *x, int64_t nrows, int64_t k, void *blocks, hipStream_t st) {
    const int64_t nsb = nrows * (k / 256);
    if (nsb <= 0) return hipSuccess;
    const dim3 g8((unsigned)((nsb * 8 + 127) / 128)), g16((unsigned)((nsb * 16 + 127) / 128));
    switch (type) {
    case GGML_HIP_TYPE_Q6_K: quantize_q6k_kernel<<<g16, 128, 0, st>>>(x, nsb, (uint8_t *)blocks); break;
    case GGML_HIP_TYPE_Q3_K: quantize_q3k_kernel<<<g16, 128, 0, st>>>(x, nsb, (uint8_t *)blocks); break;
    case GGML_HIP_TYPE_Q2_K: quantize_q2k_kernel<<<g16, 128, 0, st>>>(x, nsb, (uint8_t *)blocks); break;
    case GGML_HIP_TYPE_Q5_K: quantize_kq_kernel<true><<<g8, 128, 0, st>>>(x, nsb, (uint8_t *)blocks); break;
    default:                 quantize_kq_kernel<false><<<g8, 128, 0, st>>>(x, nsb, (uint8_t *)blocks); break;
    }
    return hipGetLastError();
}

hipError_t launch_q2k_min_pass(const ggml_hip_weight *w, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st, int form) {
    if (N <= 0 || w->M <= 0) return hipSuccess;
    if (!w->khdr || w->K % 256 != 0 || p.Npad < (N + 31) / 32 * 32 || form < 0 || form > 2) return hipErrorInvalidValue;
    const int64_t nt_n = (N + 31) / 32;
    // two 32-column tiles per wave and chunks of 8 super-blocks where that still leaves a workgroup for every CU (fewer re-reads of the
    // activation rows), else one tile per wave and chunks of 16 (half the round trips of the few workgroups there are).  The two forms
    // compute every output in the same order: the same bits (tests/test_q2k.py runs both on the same inputs through `form`, 1 / 2).
    const bool two = form == 0 ? nt_n * ((w->M + 255) / 256) >= 256 : form == 2;
    const int64_t nt_i = two ? (w->M + 255) / 256 : (w->M + 127) / 128, ntiles = nt_n * nt_i, per = (ntiles + 7) / 8;
    const dim3 grid((unsigned)(per * 8));
    if (two) q2k_min_pass_kernel<2, 8><<<grid, 256, 0, st>>>(w->khdr, w->Mpad, w->M, w->K / 256, p.a8, p.ad, p.Npad, N, dst, ldd, nt_i, ntiles, per);
    else q2k_min_pass_kernel<1, 16><<<grid, 256, 0, st>>>(w->khdr, w->Mpad, w->M, w->K / 256, p.a8, p.ad, p.Npad, N, dst, ldd, nt_i, ntiles, per);
    return hipGetLastError();
}
