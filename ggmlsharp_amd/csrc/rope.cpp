// rope.cpp -- the C-ABI of include/ggml_hip_ext.h, ROPE: the per-pair constants (ggml_hip_rope_table, host only), the rotation of Q / K rows
// (ggml_hip_rope_dev) and the rotation fused with the store into a KV cache (ggml_hip_rope_kv_store_dev, its paged and its ragged form).  The kernels are rope.hip's; the
// launchers get the table this file computes by value, so pow and log are the host's.  No set, no handle: stream-ordered launches on the
// current device, no synchronize, no allocation; capturable.
#include <cmath>

#include "ctx.h"

using namespace ghip;

namespace {

// the parameter rules shared by all three entries; 0 or an error code
int check_rope_params(const ggml_hip_rope_params_t *rp) {
    if (!rp) return fail(GGML_HIP_ERR_ARG, "rope params are null");
    if (rp->mode != 0 && rp->mode != 2) return fail(GGML_HIP_ERR_ARG, "rope mode %d: 0 (NORMAL) or 2 (NEOX); mrope and vision are not served", rp->mode);
    if (rp->n_dims < 2 || rp->n_dims % 2 != 0 || rp->n_dims > 2 * ROPE_MAX_PAIRS) return fail(GGML_HIP_ERR_SHAPE, "n_dims %d: even, in 2 .. %d", rp->n_dims, 2 * ROPE_MAX_PAIRS);
    const float f[6] = {rp->freq_base, rp->freq_scale, rp->ext_factor, rp->attn_factor, rp->beta_fast, rp->beta_slow};
    for (float v : f)
        if (!std::isfinite(v)) return fail(GGML_HIP_ERR_ARG, "a rope parameter is not finite");
    if (!(rp->freq_base > 1.0f) || !(rp->freq_scale > 0.0f)) return fail(GGML_HIP_ERR_ARG, "freq_base %g (> 1), freq_scale %g (> 0)", rp->freq_base, rp->freq_scale);
    if (rp->ext_factor != 0.0f && (rp->n_ctx_orig < 1 || !(rp->beta_fast > 0.0f) || !(rp->beta_slow > 0.0f)))
        return fail(GGML_HIP_ERR_ARG, "ext_factor != 0 needs n_ctx_orig %d >= 1 and beta_fast %g, beta_slow %g > 0", rp->n_ctx_orig, rp->beta_fast, rp->beta_slow);
    return GGML_HIP_OK;
}

// the header's formulas, all binary64 (upstream's rope_yarn and ggml_rope_yarn_corr_dims restated)
void rope_table_of(const ggml_hip_rope_params_t *rp, double *eff, double *mscale) {
    const int n_dims = rp->n_dims;
    const double base = rp->freq_base, scale = rp->freq_scale, ext = rp->ext_factor;
    double low = 0.0, high = 0.0;
    if (ext != 0.0) {
        const double pi = 3.14159265358979323846;
        auto corr = [&](double r) { return n_dims * std::log(rp->n_ctx_orig / (2.0 * pi * r)) / (2.0 * std::log(base)); };
        low = std::fmax(0.0, std::floor(corr(rp->beta_fast)));
        high = std::fmin(n_dims - 1.0, std::ceil(corr(rp->beta_slow)));
    }
    for (int i = 0; i < n_dims / 2; ++i) {
        const double extrap = std::pow(base, -2.0 * i / n_dims);
        double mix = 0.0;
        if (ext != 0.0) {
            const double y = (i - low) / std::fmax(0.001, high - low);
            mix = (1.0 - std::fmin(1.0, std::fmax(0.0, y))) * ext;
        }
        eff[i] = extrap * (scale * (1.0 - mix) + mix);
    }
    *mscale = ext != 0.0 ? rp->attn_factor * (1.0 + 0.1 * std::log(1.0 / scale)) : (double)rp->attn_factor;
}

// the rules of the rows both device entries read: D, n_dims against it, the heads, the strides of x
int check_rope_rows(const ggml_hip_rope_params_t *rp, int n_head, int D, int64_t n_tokens, int64_t ldx_tok, int64_t ldx_head) {
    if (D < 4 || D % 4 != 0 || D > 2 * ROPE_MAX_PAIRS) return fail(GGML_HIP_ERR_SHAPE, "head size %d: a multiple of 4, at most %d", D, 2 * ROPE_MAX_PAIRS);
    if (rp->n_dims > D) return fail(GGML_HIP_ERR_SHAPE, "n_dims %d above the head size %d", rp->n_dims, D);
    if (n_head < 1 || n_head > 65535) return fail(GGML_HIP_ERR_SHAPE, "n_head %d (1 .. 65535)", n_head);
    if (n_tokens < 0) return fail(GGML_HIP_ERR_ARG, "n_tokens %lld", (long long)n_tokens);
    if (n_tokens > ((int64_t)1 << 24)) return fail(GGML_HIP_ERR_SHAPE, "n_tokens %lld (<= 2^24)", (long long)n_tokens);
    if (ldx_tok % 4 != 0 || ldx_head % 4 != 0 || ldx_head < D || ldx_tok < 0 || (n_tokens > 1 && ldx_tok < D))
        return fail(GGML_HIP_ERR_SHAPE, "the strides of the rows are multiples of 4 elements, at least D");
    return GGML_HIP_OK;
}

}  // namespace

extern "C" {

int ggml_hip_rope_table(const ggml_hip_rope_params_t *rp, double *eff, double *mscale) {
    const int rc = check_rope_params(rp);
    if (rc) return rc;
    if (!eff || !mscale) return fail(GGML_HIP_ERR_ARG, "null argument");
    rope_table_of(rp, eff, mscale);
    return GGML_HIP_OK;
}

int ggml_hip_rope_dev(const ggml_hip_rope_params_t *rp, const float *d_x, int64_t ldx_tok, int64_t ldx_head, int n_head, int D, int64_t n_tokens,
                      const int32_t *d_pos, int64_t pos0, const int32_t *d_pos0, const float *d_freq_factors, float *d_dst, int64_t ldd_tok,
                      int64_t ldd_head, void *stream) {
    int rc = check_rope_params(rp);
    if (rc) return rc;
    rc = check_rope_rows(rp, n_head, D, n_tokens, ldx_tok, ldx_head);
    if (rc) return rc;
    if (ldd_tok % 4 != 0 || ldd_head % 4 != 0 || ldd_head < D || ldd_tok < 0 || (n_tokens > 1 && ldd_tok < D))
        return fail(GGML_HIP_ERR_SHAPE, "the strides of dst are multiples of 4 elements, at least D");
    if (n_tokens == 0) return GGML_HIP_OK;
    if (!d_x || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_x | (uintptr_t)d_dst) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_x and d_dst must be 16-byte aligned");
    if ((((uintptr_t)d_pos | (uintptr_t)d_pos0 | (uintptr_t)d_freq_factors) & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_pos, d_pos0 and d_freq_factors must be 4-byte aligned");
    rope_table tab;
    rope_table_of(rp, tab.eff, &tab.mscale);
    rope_args a;
    a.mode = rp->mode; a.n_dims = rp->n_dims; a.n_head = n_head; a.D = D;
    a.x = d_x; a.ldx_tok = ldx_tok; a.ldx_head = ldx_head; a.n_tokens = n_tokens;
    a.d_pos = d_pos; a.pos0 = pos0; a.d_pos0 = d_pos0; a.freq_factors = d_freq_factors;
    HIP_TRY(launch_rope(tab, a, d_dst, ldd_tok, ldd_head, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_rope_kv_store_dev(const ggml_hip_rope_params_t *rp, int kv_type, const float *d_x, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D,
                               int64_t n_tokens, const float *d_freq_factors, void *d_cache, int64_t nb_pos, int64_t nb_head, int64_t n_pos_max,
                               int64_t pos0, const int32_t *d_pos0, void *stream) {
    int rc = check_rope_params(rp);
    if (rc) return rc;
    if (kv_type != GGML_TYPE_F16 && kv_type != GGML_TYPE_Q8_0) return fail(GGML_HIP_ERR_TYPE, "kv_type %d: the cache is F16 or Q8_0", kv_type);
    rc = check_rope_rows(rp, n_head_kv, D, n_tokens, ldx_tok, ldx_head);
    if (rc) return rc;
    if (kv_type == GGML_TYPE_Q8_0 && D % QK != 0) return fail(GGML_HIP_ERR_SHAPE, "head size %d: a Q8_0 cache row is whole blocks of %d", D, QK);
    if (n_pos_max < 0) return fail(GGML_HIP_ERR_ARG, "n_pos_max %lld", (long long)n_pos_max);
    const int64_t row_bytes = kv_type == GGML_TYPE_Q8_0 ? D / QK * (int64_t)sizeof(block_q8_0) : D * 2;
    if (nb_pos % 16 != 0 || nb_head % 16 != 0 || nb_pos < row_bytes || nb_head < row_bytes)
        return fail(GGML_HIP_ERR_SHAPE, "nb_pos %lld, nb_head %lld: multiples of 16 bytes, at least the %lld bytes of a row", (long long)nb_pos, (long long)nb_head,
                    (long long)row_bytes);
    if (n_tokens == 0) return GGML_HIP_OK;
    if (!d_x || !d_cache) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_x | (uintptr_t)d_cache) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_x and d_cache must be 16-byte aligned");
    if ((((uintptr_t)d_pos0 | (uintptr_t)d_freq_factors) & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_pos0 and d_freq_factors must be 4-byte aligned");
    rope_table tab;
    rope_table_of(rp, tab.eff, &tab.mscale);
    rope_args a;
    a.mode = rp->mode; a.n_dims = rp->n_dims; a.n_head = n_head_kv; a.D = D;
    a.x = d_x; a.ldx_tok = ldx_tok; a.ldx_head = ldx_head; a.n_tokens = n_tokens;
    a.d_pos = nullptr; a.pos0 = pos0; a.d_pos0 = d_pos0; a.freq_factors = d_freq_factors;
    HIP_TRY(launch_rope_kv_store(tab, a, kv_type, d_cache, nb_pos, nb_head, n_pos_max, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_rope_kv_store_paged_dev(const ggml_hip_rope_params_t *rp, int kv_type, const float *d_x, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D,
                                     int64_t n_seq, int64_t n_q, const float *d_freq_factors, void *d_pool, int64_t nb_page, int64_t nb_pos, int64_t nb_head,
                                     int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max, void *stream) {
    int rc = check_rope_params(rp);
    if (rc) return rc;
    kv_pages pg;
    rc = check_kv_pages(kv_type, D, n_head_kv, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    if (n_q < 0) return fail(GGML_HIP_ERR_ARG, "n_q %lld", (long long)n_q);
    if (n_seq * n_q > ATTN_PAGED_MAX_ROWS) return fail(GGML_HIP_ERR_SHAPE, "n_seq * n_q %lld (<= %lld)", (long long)(n_seq * n_q), (long long)ATTN_PAGED_MAX_ROWS);
    rc = check_rope_rows(rp, n_head_kv, D, n_seq * n_q, ldx_tok, ldx_head);
    if (rc) return rc;
    if (n_q == 0) return GGML_HIP_OK;
    if (!d_x || !d_pool) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_x | (uintptr_t)d_pool) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_x and d_pool must be 16-byte aligned");
    if (((uintptr_t)d_freq_factors & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_freq_factors must be 4-byte aligned");
    rope_table tab;
    rope_table_of(rp, tab.eff, &tab.mscale);
    rope_args a;
    a.mode = rp->mode; a.n_dims = rp->n_dims; a.n_head = n_head_kv; a.D = D;
    a.x = d_x; a.ldx_tok = ldx_tok; a.ldx_head = ldx_head; a.n_tokens = n_seq * n_q;
    a.d_pos = nullptr; a.pos0 = 0; a.d_pos0 = nullptr; a.freq_factors = d_freq_factors;
    HIP_TRY(launch_rope_kv_store_paged(tab, a, kv_type, n_q, d_pool, nb_pos, nb_head, pg, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_rope_kv_store_paged_ragged_dev(const ggml_hip_rope_params_t *rp, int kv_type, const float *d_x, int64_t ldx_tok, int64_t ldx_head, int n_head_kv,
                                            int D, int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const float *d_freq_factors, void *d_pool,
                                            int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages,
                                            const int32_t *d_len, int64_t n_kv_max, void *stream) {
    int rc = check_rope_params(rp);
    if (rc) return rc;
    kv_pages pg;
    rc = check_kv_pages(kv_type, D, n_head_kv, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    kv_ragged rg;
    rc = check_kv_ragged(d_q_start, n_seq, n_tokens_max, &rg);
    if (rc) return rc;
    rc = check_rope_rows(rp, n_head_kv, D, n_tokens_max, ldx_tok, ldx_head);
    if (rc) return rc;
    if (n_tokens_max == 0) return GGML_HIP_OK;
    if (!d_x || !d_pool) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_x | (uintptr_t)d_pool) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_x and d_pool must be 16-byte aligned");
    if (((uintptr_t)d_freq_factors & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_freq_factors must be 4-byte aligned");
    rope_table tab;
    rope_table_of(rp, tab.eff, &tab.mscale);
    rope_args a;
    a.mode = rp->mode; a.n_dims = rp->n_dims; a.n_head = n_head_kv; a.D = D;
    a.x = d_x; a.ldx_tok = ldx_tok; a.ldx_head = ldx_head; a.n_tokens = n_tokens_max;
    a.d_pos = nullptr; a.pos0 = 0; a.d_pos0 = nullptr; a.freq_factors = d_freq_factors;
    HIP_TRY(launch_rope_kv_store_paged_ragged(tab, a, kv_type, rg, d_pool, nb_pos, nb_head, pg, (hipStream_t)stream));
    return GGML_HIP_OK;
}

}  // extern "C"
