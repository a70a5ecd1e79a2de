// decode_ends.cpp -- the C-ABI of include/ggml_hip_ext.h, THE ENDS OF A DECODE STEP: a token id becomes a hidden row (ggml_hip_get_rows_dev
// over a resident weight, get_rows.hip) and the LM-head logits become the next token id (ggml_hip_argmax_rows_dev / ggml_hip_sample_topk_dev,
// sample.hip).  No set, no handle: stream-ordered launches, no synchronize, no allocation, scratch from the caller; capturable.  Every
// argument is checked before a device is touched.
#include <cmath>

#include "ctx.h"

hipError_t launch_get_rows(const ggml_hip_weight *w, const int32_t *ids, int64_t n_ids, float *dst, int64_t ldd, hipStream_t st);
int64_t topk_chunk_len();
hipError_t launch_sample_topk(const float *logits, int64_t ld, int64_t n_rows, int64_t n_vocab, int k, float inv_temp, float top_p, const float *u,
                              int32_t *ids, float *probs, int32_t *token, void *work, hipStream_t st);

using namespace ghip;

namespace {

constexpr int64_t GET_ROWS_MAX_IDS = (int64_t)1 << 20;
constexpr int64_t TOPK_MAX_VOCAB = (int64_t)1 << 20;
constexpr int64_t TOPK_MAX_ROWS = 4096;
constexpr int TOPK_K_MAX = 64;

bool topk_shape_ok(int64_t n_rows, int64_t n_vocab, int k) {
    return n_rows >= 1 && n_rows <= TOPK_MAX_ROWS && n_vocab >= 1 && n_vocab <= TOPK_MAX_VOCAB && k >= 1 && k <= TOPK_K_MAX && k <= n_vocab;
}

// the rules both sampler entries share; 0, or an error code.  n_rows = 0 is the caller's to return on first.
int check_topk(const float *d_logits, int64_t ld, int64_t n_rows, int64_t n_vocab, int k, const int32_t *d_ids, const void *d_work, size_t work_bytes) {
    if (!topk_shape_ok(n_rows, n_vocab, k))
        return fail(GGML_HIP_ERR_SHAPE, "n_rows %lld (1 .. %lld), n_vocab %lld (1 .. 2^20), k %d (1 .. min(n_vocab, %d))", (long long)n_rows, (long long)TOPK_MAX_ROWS,
                    (long long)n_vocab, k, TOPK_K_MAX);
    if (ld < n_vocab) return fail(GGML_HIP_ERR_SHAPE, "ld %lld below n_vocab %lld", (long long)ld, (long long)n_vocab);
    if (!d_logits || !d_ids) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_logits | (uintptr_t)d_ids) & 3) != 0) return fail(GGML_HIP_ERR_ARG, "d_logits and d_ids must be 4-byte aligned");
    const size_t need = ggml_hip_topk_work_size(n_rows, n_vocab, k);
    if (!d_work || work_bytes < need || ((uintptr_t)d_work & 7) != 0) return fail(GGML_HIP_ERR_ARG, "work buffer missing, misaligned (8 bytes) or too small: need %zu", need);
    return GGML_HIP_OK;
}

}  // namespace

extern "C" {

int ggml_hip_get_rows_serves_for(int type) {
    const wtype *r = wtype_of(type);
    return r && r->to_planar ? 1 : 0;                       // every type that can be a resident weight (get_rows.hip says why)
}

int ggml_hip_get_rows_dev(const ggml_hip_weight *w, const int32_t *d_ids, int64_t n_ids, float *d_dst, int64_t ldd, void *stream) {
    if (n_ids < 0) return fail(GGML_HIP_ERR_ARG, "n_ids %lld", (long long)n_ids);
    if (n_ids > GET_ROWS_MAX_IDS) return fail(GGML_HIP_ERR_SHAPE, "n_ids %lld (<= 2^20)", (long long)n_ids);
    if (n_ids == 0) return GGML_HIP_OK;
    if (!w || !d_ids || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_ids | (uintptr_t)d_dst) & 3) != 0) return fail(GGML_HIP_ERR_ARG, "d_ids and d_dst must be 4-byte aligned");
    const int type = ggml_hip_weight_type(w);
    if (!ggml_hip_get_rows_serves_for(type)) return fail(GGML_HIP_ERR_TYPE, "get_rows does not serve type %d", type);
    if (ldd < w->K) return fail(GGML_HIP_ERR_SHAPE, "ldd %lld below K %lld", (long long)ldd, (long long)w->K);
    int cur = -1;
    if (hipGetDevice(&cur) != hipSuccess || cur != w->device) HIP_TRY(hipSetDevice(w->device));
    HIP_TRY(launch_get_rows(w, d_ids, n_ids, d_dst, ldd, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int64_t ggml_hip_topk_chunk(void) { return topk_chunk_len(); }

size_t ggml_hip_topk_work_size(int64_t n_rows, int64_t n_vocab, int k) {
    if (!topk_shape_ok(n_rows, n_vocab, k)) return 0;
    const int64_t C = topk_chunk_len();
    return (size_t)n_rows * (size_t)((n_vocab + C - 1) / C) * (size_t)k * sizeof(uint64_t);
}

int ggml_hip_argmax_rows_dev(const float *d_logits, int64_t ld, int64_t n_rows, int64_t n_vocab, int32_t *d_ids, void *d_work, size_t work_bytes, void *stream) {
    if (n_rows == 0) return GGML_HIP_OK;
    const int rc = check_topk(d_logits, ld, n_rows, n_vocab, 1, d_ids, d_work, work_bytes);
    if (rc) return rc;
    HIP_TRY(launch_sample_topk(d_logits, ld, n_rows, n_vocab, 1, 1.0f, 1.0f, nullptr, d_ids, nullptr, nullptr, d_work, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_sample_topk_dev(const float *d_logits, int64_t ld, int64_t n_rows, int64_t n_vocab, int k, float inv_temp, float top_p, const float *d_u,
                             int32_t *d_ids, float *d_probs, int32_t *d_token, void *d_work, size_t work_bytes, void *stream) {
    if (n_rows == 0) return GGML_HIP_OK;
    const int rc = check_topk(d_logits, ld, n_rows, n_vocab, k, d_ids, d_work, work_bytes);
    if (rc) return rc;
    if (!std::isfinite(inv_temp) || !(inv_temp > 0.0f)) return fail(GGML_HIP_ERR_ARG, "inv_temp %g: finite and > 0", (double)inv_temp);
    const bool pick = d_u && d_token;
    if (pick && !d_probs) return fail(GGML_HIP_ERR_ARG, "a pick needs d_probs: top_p and the pick are defined on the probabilities the entry writes");
    if ((((uintptr_t)d_u | (uintptr_t)d_probs | (uintptr_t)d_token) & 3) != 0) return fail(GGML_HIP_ERR_ARG, "d_u, d_probs and d_token must be 4-byte aligned");
    HIP_TRY(launch_sample_topk(d_logits, ld, n_rows, n_vocab, k, inv_temp, top_p, pick ? d_u : nullptr, d_ids, d_probs, pick ? d_token : nullptr, d_work,
                               (hipStream_t)stream));
    return GGML_HIP_OK;
}

}  // extern "C"
