// get_rows.hip -- rows of a RESIDENT weight by device ids (ggml_hip_get_rows_dev, decode_ends.cpp): upstream's ggml_get_rows over the
// token-embedding matrix, read from the planes a weight already keeps for its products.
//
// THE CONTRACT (include/ggml_hip_ext.h): a gathered row is bit for bit ggml_hip_weight_download of that row followed by the type table's
// dequantize row function.  Every resident plane holds a field of the file format itself or a value the dequantizer computes first and
// exactly (the k-quants' d * sc, the widened halves), so each form below is its dequantizer's LAST operations in the dequantizer's order --
// one multiply, or one multiply then one add / subtract (the library is built with -ffp-contract=off):
//     Q4_0, Q5_0             (float)(q - 8 | 16) * d                          quantize.hip dequant_block
//     Q4_1, Q5_1             (float)q * d + m
//       Q4_K, Q5_K           the same: d plane = d * sc (exact), m plane = -(dmin * m): x + (-y) is x - y (kquants.hip dequantize_q5k_kernel)
//     Q4_2                   (float)(q - 8) * d, the first 16 elements under the d plane, the last 16 under the m plane
//     Q8_0                   (float)q * d
//       IQ4_NL               the same: the int8 planes hold the codebook entries, (float)kv * d == d * (float)kv (iq4.hip)
//     Q6_K, Q3_K, IQ4_XS     (two-scale form) d01 * (float)v, d01 the d / m plane entry of the element's half (two_scale.h)
//     Q2_K                   d01 * (float)v - dmin * (float)(scales[j] >> 4), dmin and scales[] from the super-block's khdr slot
//     F32 / F16 / BF16       the row / the exact widening
// Only planes that ARE the weight are read: qs, d, m, qh, khdr, dense -- and, for the two-scale form, its int8 planes: that form keeps its
// quants nowhere else (common.h: the nibble plane is a stub there).  No operand image (q6a, mp3, gs, p16, p32, the i8p copy of a nibble
// type) is touched, nothing is added at upload.
//
// Geometry.  A row's k-blocks lie Mpad * 16 bytes apart: the read side is a gather of 16-byte pieces whatever is done, the write side is what
// coalesces.  One thread per (id, k-block): its 16 or 32 quant bytes and its scale words in, 32 consecutive floats out -- float4 stores
// where dst and ldd allow, one element at a time otherwise, the same bits.  Threads of a workgroup walk (id, k-block) with the k-block
// fastest, so a workgroup covers several ids where K is small and a contiguous stretch of one row where it is large.
// An id outside [0, M) writes +0.0f and forms no address from the id.
//
// The other gather of a step lives here too: ggml_hip_ragged_last_rows_dev (attn.cpp) copies the last packed f32 row of every sequence of a
// ragged batch, the rows the LM head needs (ragged_last_rows_kernel, the dense kernel's geometry).
#include "common.h"

namespace {

enum { GR_Q4_0, GR_Q4_1, GR_Q5_0, GR_Q5_1, GR_Q4_2, GR_Q8_0, GR_TWO_SCALE, GR_TWO_SCALE_MIN };

struct gr_planes {
    const uint8_t *qs;      // the quant plane of the form: the nibble plane, Q8_0's two int8 planes, or the two-scale form's int8 planes
    const uint32_t *qh;
    const float *d, *m;
    const uint8_t *khdr;
    int64_t M, Mpad, nbk;
};

__device__ __forceinline__ float gr_h2f(uint16_t h) {      // IEEE binary16 -> binary32, exact (payloads kept)
    const uint32_t sign = ((uint32_t)h & 0x8000u) << 16, exp = (h >> 10) & 0x1Fu, man = h & 0x3FFu;
    if (exp == 0) return __uint_as_float(__float_as_uint((float)man * 5.9604644775390625e-08f) | sign);
    if (exp == 31) return __uint_as_float(sign | 0x7F800000u | (man << 13));
    return __uint_as_float(sign | ((exp + 112u) << 23) | (man << 13));
}

// the 32 values of k-block b of row `row` (0 <= row < M, 0 <= b < nbk)
template <int FORM>
__device__ __forceinline__ void gr_block(const gr_planes &p, int64_t row, int64_t b, float (&v)[QK]) {
    const int64_t pi = b * p.Mpad + row;
    const float d = p.d[pi];
    if constexpr (FORM == GR_Q8_0 || FORM == GR_TWO_SCALE || FORM == GR_TWO_SCALE_MIN) {
        // plane h byte j = element 2 j + h
        const uint4 e4 = *(const uint4 *)(p.qs + ((b * 2 + 0) * p.Mpad + row) * 16), o4 = *(const uint4 *)(p.qs + ((b * 2 + 1) * p.Mpad + row) * 16);
        const uint32_t ev[4] = {e4.x, e4.y, e4.z, e4.w}, od[4] = {o4.x, o4.y, o4.z, o4.w};
        float d1 = d, m0 = 0.0f, m1 = 0.0f;
        if constexpr (FORM != GR_Q8_0) d1 = p.m[pi];
        if constexpr (FORM == GR_TWO_SCALE_MIN) {           // Q2_K: the slot holds scales[16], d, dmin (kquants.hip q2k_codec)
            const uint8_t *h = p.khdr + ((b >> 3) * p.Mpad + row) * 32;
            const int bq = (int)(b & 7);
            const float dmin = gr_h2f((uint16_t)(h[18] | ((uint16_t)h[19] << 8)));
            m0 = dmin * (float)(h[2 * bq] >> 4);
            m1 = dmin * (float)(h[2 * bq + 1] >> 4);
        }
#pragma unroll
        for (int j = 0; j < 16; ++j) {
            const float q0 = (float)(int)(int8_t)((ev[j >> 2] >> (8 * (j & 3))) & 0xFFu), q1 = (float)(int)(int8_t)((od[j >> 2] >> (8 * (j & 3))) & 0xFFu);
            if constexpr (FORM == GR_Q8_0) {
                v[2 * j] = q0 * d;
                v[2 * j + 1] = q1 * d;
            } else if constexpr (FORM == GR_TWO_SCALE) {
                v[2 * j] = (j < 8 ? d : d1) * q0;
                v[2 * j + 1] = (j < 8 ? d : d1) * q1;
            } else {
                v[2 * j] = (j < 8 ? d : d1) * q0 - (j < 8 ? m0 : m1);
                v[2 * j + 1] = (j < 8 ? d : d1) * q1 - (j < 8 ? m0 : m1);
            }
        }
    } else {
        // byte j of the 16 = element 2 j (low nibble), 2 j + 1 (high nibble); bit e of qh = the fifth bit of element e
        const uint4 q4 = *(const uint4 *)(p.qs + pi * 16);
        const uint32_t qq[4] = {q4.x, q4.y, q4.z, q4.w};
        float m = 0.0f;
        uint32_t hb = 0u;
        if constexpr (FORM == GR_Q4_1 || FORM == GR_Q5_1 || FORM == GR_Q4_2) m = p.m[pi];
        if constexpr (FORM == GR_Q5_0 || FORM == GR_Q5_1) hb = p.qh[pi];
#pragma unroll
        for (int e = 0; e < QK; ++e) {
            const int nib = (int)((qq[e >> 3] >> (4 * (e & 7))) & 0xFu);
            if constexpr (FORM == GR_Q4_0) v[e] = (float)(nib - 8) * d;
            else if constexpr (FORM == GR_Q4_1) { const float t = (float)nib * d; v[e] = t + m; }
            else if constexpr (FORM == GR_Q5_0) v[e] = (float)((nib | (int)(((hb >> e) & 1u) << 4)) - 16) * d;
            else if constexpr (FORM == GR_Q5_1) { const float t = (float)(nib | (int)(((hb >> e) & 1u) << 4)) * d; v[e] = t + m; }
            else v[e] = (float)(nib - 8) * (e < 16 ? d : m);      // Q4_2: the second 16-element block's scale lives in the m plane
        }
    }
}

template <int FORM, bool VEC>
__global__ __launch_bounds__(256) void get_rows_kernel(const gr_planes p, const int32_t *__restrict__ ids, int64_t n_ids, float *__restrict__ dst, int64_t ldd) {
    const int64_t g = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t i = g / p.nbk, b = g - i * p.nbk;
    if (i >= n_ids) return;
    const int64_t row = ids[i];
    float v[QK];
    if (row >= 0 && row < p.M) {
        gr_block<FORM>(p, row, b, v);
    } else {
#pragma unroll
        for (int e = 0; e < QK; ++e) v[e] = 0.0f;
    }
    float *o = dst + i * ldd + b * QK;
    if (VEC) {
#pragma unroll
        for (int l = 0; l < QK / 4; ++l) ((float4 *)o)[l] = make_float4(v[4 * l], v[4 * l + 1], v[4 * l + 2], v[4 * l + 3]);
    } else {
#pragma unroll
        for (int e = 0; e < QK; ++e) o[e] = v[e];
    }
}

// dense rows [Mpad][K]: ES bytes per element (4: f32; 2: F16, or BF16 when BF); a thread owns 4 consecutive elements (VEC) or one
template <int ES, bool BF, bool VEC>
__global__ __launch_bounds__(256) void get_rows_dense_kernel(const void *__restrict__ dense, int64_t M, int64_t K, const int32_t *__restrict__ ids, int64_t n_ids,
                                                             int blocks_per_row, float *__restrict__ dst, int64_t ldd) {
    const int64_t i = blockIdx.x / blocks_per_row;
    const int64_t k = ((int64_t)(blockIdx.x % blocks_per_row) * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (k >= K) return;
    const int64_t row = ids[i];
    const bool ok = row >= 0 && row < M;
    auto widen = [](uint16_t h) { return BF ? __uint_as_float((uint32_t)h << 16) : gr_h2f(h); };
    float *o = dst + i * ldd + k;
    if (VEC) {                                              // (K % 4 == 0: whole quads)
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok) {
            if (ES == 4) {
                r = *(const float4 *)((const float *)dense + row * K + k);
            } else {
                const uint2 h = *(const uint2 *)((const uint16_t *)dense + row * K + k);
                r = make_float4(widen((uint16_t)h.x), widen((uint16_t)(h.x >> 16)), widen((uint16_t)h.y), widen((uint16_t)(h.y >> 16)));
            }
        }
        *(float4 *)o = r;
    } else {
        float r = 0.0f;
        if (ok) r = ES == 4 ? ((const float *)dense)[row * K + k] : widen(((const uint16_t *)dense)[row * K + k]);
        *o = r;
    }
}

// ggml_hip_ragged_last_rows_dev: row s of dst = the LAST packed row of sequence s, q_start[s+1] - 1, or +0.0f where the sequence is empty or not
// present.  The guard comes before the address it protects; a thread owns 4 consecutive elements (VEC) or one, as get_rows_dense_kernel's.
template <bool VEC>
__global__ __launch_bounds__(256) void ragged_last_rows_kernel(const kv_ragged rg, const float *__restrict__ x, int64_t ldx, int64_t K, int blocks_per_row,
                                                               float *__restrict__ dst, int64_t ldd) {
    const int64_t s = blockIdx.x / blocks_per_row;
    const int64_t k = ((int64_t)(blockIdx.x % blocks_per_row) * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (k >= K) return;
    const int64_t qs = rg.q_start[s], qe = rg.q_start[s + 1];
    const bool ok = qs >= 0 && qs < qe && qe <= rg.n_tokens_max;
    float *o = dst + s * ldd + k;
    if (VEC) {                                              // (K % 4 == 0: whole quads)
        float4 r = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (ok) r = *(const float4 *)(x + (qe - 1) * ldx + k);
        *(float4 *)o = r;
    } else {
        float r = 0.0f;
        if (ok) r = x[(qe - 1) * ldx + k];
        *o = r;
    }
}

}  // namespace

hipError_t launch_ragged_last_rows(const kv_ragged &rg, const float *x, int64_t ldx, int64_t K, float *dst, int64_t ldd, hipStream_t st) {
    if (rg.n_seq <= 0 || K <= 0) return hipSuccess;
    const bool vec = (((uintptr_t)x | (uintptr_t)dst) & 15) == 0 && ldx % 4 == 0 && ldd % 4 == 0 && K % 4 == 0;
    const int64_t per_block = vec ? 1024 : 256, bpr = (K + per_block - 1) / per_block;
    if (bpr > 0x7FFFFFFF / rg.n_seq) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(rg.n_seq * bpr));
    if (vec) ragged_last_rows_kernel<true><<<grid, 256, 0, st>>>(rg, x, ldx, K, (int)bpr, dst, ldd);
    else ragged_last_rows_kernel<false><<<grid, 256, 0, st>>>(rg, x, ldx, K, (int)bpr, dst, ldd);
    return hipGetLastError();
}

// w: a resident weight of a served type (decode_ends.cpp checks); ids / dst on the weight's device
hipError_t launch_get_rows(const ggml_hip_weight *w, const int32_t *ids, int64_t n_ids, float *dst, int64_t ldd, hipStream_t st) {
    if (n_ids <= 0 || w->K <= 0) return hipSuccess;
    const bool vec = ((uintptr_t)dst & 15) == 0 && ldd % 4 == 0;
    if (w->dense) {
        const bool v4 = vec && w->K % 4 == 0;
        const int64_t per_block = v4 ? 1024 : 256, bpr = (w->K + per_block - 1) / per_block;
        if (bpr > 0x7FFFFFFF / n_ids) return hipErrorInvalidValue;
        const dim3 grid((unsigned)(n_ids * bpr));
#define DENSE(ES, BF)                                                                                                                         \
    do {                                                                                                                                      \
        if (v4) get_rows_dense_kernel<ES, BF, true><<<grid, 256, 0, st>>>(w->dense, w->M, w->K, ids, n_ids, (int)bpr, dst, ldd);              \
        else get_rows_dense_kernel<ES, BF, false><<<grid, 256, 0, st>>>(w->dense, w->M, w->K, ids, n_ids, (int)bpr, dst, ldd);                \
    } while (0)
        if (w->type == GGML_TYPE_F32) DENSE(4, false);
        else if (is_bf16(w->type)) DENSE(2, true);
        else if (w->type == GGML_TYPE_F16) DENSE(2, false);
        else return hipErrorInvalidValue;
#undef DENSE
        return hipGetLastError();
    }
    if (w->nbk <= 0) return hipSuccess;
    const wtype *ext = w->ext_type ? wtype_of(w->ext_type) : nullptr;
    const bool two_scale = ext && ext->own_i8;
    gr_planes p = {two_scale ? w->i8p : w->qs, w->qh, w->d, w->m, w->khdr, w->M, w->Mpad, w->nbk};
    if (!p.qs || !p.d) return hipErrorInvalidValue;
    const int64_t blocks = (n_ids * w->nbk + 255) / 256;
    if (blocks > 0x7FFFFFFF) return hipErrorInvalidValue;
    const dim3 grid((unsigned)blocks);
#define ROWS(FORM)                                                                                                                            \
    do {                                                                                                                                      \
        if (vec) get_rows_kernel<FORM, true><<<grid, 256, 0, st>>>(p, ids, n_ids, dst, ldd);                                                  \
        else get_rows_kernel<FORM, false><<<grid, 256, 0, st>>>(p, ids, n_ids, dst, ldd);                                                     \
    } while (0)
    if (two_scale) {
        if (!p.m) return hipErrorInvalidValue;
        if (ext->min_pass) { if (!p.khdr) return hipErrorInvalidValue; ROWS(GR_TWO_SCALE_MIN); }
        else ROWS(GR_TWO_SCALE);
        return hipGetLastError();
    }
    switch (w->type) {
    case GGML_TYPE_Q4_0: ROWS(GR_Q4_0); break;
    case GGML_TYPE_Q4_1: ROWS(GR_Q4_1); break;
    case GGML_TYPE_Q5_0: ROWS(GR_Q5_0); break;
    case GGML_TYPE_Q5_1: ROWS(GR_Q5_1); break;               // (and Q4_K / Q5_K, which live in this form)
    case GGML_TYPE_Q4_2: ROWS(GR_Q4_2); break;
    case GGML_TYPE_Q8_0: ROWS(GR_Q8_0); break;               // (and IQ4_NL)
    default: return hipErrorInvalidValue;
    }
#undef ROWS
    return hipGetLastError();
}
