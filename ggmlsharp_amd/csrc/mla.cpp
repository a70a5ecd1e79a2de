// mla.cpp -- the C-ABI of include/ggml_hip_ext.h, section MLA: latent attention over a latent KV cache (ggml_hip_attn_mla_dev, ggml_hip_attn_mla_paged_dev),
// their plans and work sizes, and the paged store of latent rows (ggml_hip_kv_store_latent_paged_dev).  The kernels and their arithmetic are mla.hip's, the
// form and every grid plan.cpp's (plan_attn_mla).  No set, no handle: stream-ordered launches on the current device, no synchronize, no allocation; capturable.
// Every refusal is decided before a device is touched.
#include "ctx.h"

using namespace ghip;

namespace {

constexpr size_t MLA_ALIGN = 256;

int64_t latent_row_bytes(int kv_type) { return kv_type == GGML_TYPE_Q8_0 ? MLA_DK / QK * (int64_t)sizeof(block_q8_0) : MLA_DK * 2; }

// the shape rules shared by the plans, the work sizes and the entries; 0 or an error code
int check_mla_shape(int kv_type, int D_k, int D_v, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max) {
    if (!(kv_type == GGML_TYPE_F16 || kv_type == GGML_TYPE_Q8_0)) return fail(GGML_HIP_ERR_TYPE, "kv_type %d: the cache is F16 or Q8_0", kv_type);
    if (D_k != MLA_DK || D_v != MLA_DV) return fail(GGML_HIP_ERR_SHAPE, "(D_k, D_v) = (%d, %d): only (%d, %d) is served", D_k, D_v, MLA_DK, MLA_DV);
    if (n_head < 1 || n_head > 256) return fail(GGML_HIP_ERR_SHAPE, "n_head %d (1 .. 256)", n_head);
    if (n_q < 0 || n_kv_max < 0) return fail(GGML_HIP_ERR_ARG, "n_q %lld, n_kv_max %lld", (long long)n_q, (long long)n_kv_max);
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    if (n_q > (1 << 20) || n_kv_max > (1 << 24) || n_seq * n_q > ATTN_PAGED_MAX_ROWS || n_seq * n_q * n_head > 0x7FFFFFFF)
        return fail(GGML_HIP_ERR_SHAPE, "n_seq * n_q %lld (<= 2^20, times n_head below 2^31), n_kv_max %lld (<= 2^24)", (long long)(n_seq * n_q), (long long)n_kv_max);
    return GGML_HIP_OK;
}

// the strides of q [rows][n_head][576] and dst [rows][n_head][512]
int check_mla_rows(int64_t rows, int64_t ldq_tok, int64_t ldq_head, int64_t ldd_tok, int64_t ldd_head) {
    if (ldq_tok % 4 != 0 || ldq_head % 4 != 0 || ldd_tok % 4 != 0 || ldd_head % 4 != 0 || ldq_head < MLA_DK || ldd_head < MLA_DV || ldq_tok < 0 || ldd_tok < 0 ||
        (rows > 1 && (ldq_tok < MLA_DK || ldd_tok < MLA_DV)))
        return fail(GGML_HIP_ERR_SHAPE, "the strides of q and dst are multiples of 4 elements, at least %d (q) and %d (dst)", MLA_DK, MLA_DV);
    return GGML_HIP_OK;
}

// the page table of a latent pool (check_kv_pages at one row of 576 elements per position); fills *pg
int check_latent_pages(int kv_type, int64_t nb_page, int64_t nb_pos, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_seq,
                       int64_t n_kv_max, kv_pages *pg) {
    if (!(kv_type == GGML_TYPE_F16 || kv_type == GGML_TYPE_Q8_0)) return fail(GGML_HIP_ERR_TYPE, "kv_type %d: the cache is F16 or Q8_0", kv_type);
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    if (n_kv_max < 0) return fail(GGML_HIP_ERR_ARG, "n_kv_max %lld", (long long)n_kv_max);
    if (n_kv_max > (1 << 24)) return fail(GGML_HIP_ERR_SHAPE, "n_kv_max %lld (<= 2^24)", (long long)n_kv_max);
    const int64_t row_bytes = latent_row_bytes(kv_type);
    if (nb_pos % 16 != 0 || nb_pos < row_bytes || nb_pos > ((int64_t)1 << 40))
        return fail(GGML_HIP_ERR_SHAPE, "nb_pos %lld: a multiple of 16 bytes, at least the %lld bytes of a row", (long long)nb_pos, (long long)row_bytes);
    const int64_t span = (ATTN_CHUNK - 1) * nb_pos + row_bytes;      // the bytes the rows of one page span
    if (nb_page % 16 != 0 || nb_page < span)
        return fail(GGML_HIP_ERR_SHAPE, "nb_page %lld: a multiple of 16 bytes, at least the %lld bytes a page's rows span", (long long)nb_page, (long long)span);
    if (n_pages <= 0) return fail(GGML_HIP_ERR_ARG, "n_pages %d", n_pages);
    if (ld_pages < (n_kv_max + ATTN_CHUNK - 1) / ATTN_CHUNK)
        return fail(GGML_HIP_ERR_SHAPE, "ld_pages %lld below ceil(n_kv_max %lld / %d)", (long long)ld_pages, (long long)n_kv_max, ATTN_CHUNK);
    if (!d_pages || !d_len) return fail(GGML_HIP_ERR_ARG, "d_pages and d_len must not be null");
    if ((((uintptr_t)d_pages | (uintptr_t)d_len) & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_pages and d_len must be 4-byte aligned");
    pg->pages = d_pages; pg->ld_pages = ld_pages; pg->len = d_len; pg->nb_page = nb_page; pg->n_pages = n_pages; pg->n_kv_max = (int)n_kv_max;
    return GGML_HIP_OK;
}

int put_plan(int kv_type, int D_k, int D_v, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_mla_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    const int rc = check_mla_shape(kv_type, D_k, D_v, n_head, n_seq, n_q, n_kv_max);
    if (rc) return rc;
    *out = ggml_hip_attn_mla_plan_t{};
    out->chunk = ATTN_CHUNK; out->span = MLA_SPAN; out->q_tile = MLA_TILE; out->step = MLA_STEP;
    if (n_q == 0) return GGML_HIP_OK;
    const mla_plan p = plan_attn_mla(kv_type, n_head, n_seq, n_q, n_kv_max);
    if (p.form == MLA_FORM_NONE) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    out->form = p.form; out->launches = p.launches; out->n_spans = p.n_spans; out->workgroups = p.wgs; out->merge_workgroups = p.merge_wgs;
    out->work_bytes = p.work_bytes ? (p.work_bytes + MLA_ALIGN - 1) / MLA_ALIGN * MLA_ALIGN + MLA_ALIGN : 0;
    return GGML_HIP_OK;
}

size_t work_size(int kv_type, int D_k, int D_v, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max) {
    if (D_k != MLA_DK || D_v != MLA_DV || n_q <= 0) return 0;
    const mla_plan p = plan_attn_mla(kv_type, n_head, n_seq, n_q, n_kv_max);
    if (p.form == MLA_FORM_NONE || p.work_bytes == 0) return 0;
    return (p.work_bytes + MLA_ALIGN - 1) / MLA_ALIGN * MLA_ALIGN + MLA_ALIGN;     // (the base is rounded up to a 256-byte boundary)
}

// both entries behind their shape checks: pg null for the contiguous call
int mla_run(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_cache, int64_t nb_pos, int n_head, int64_t n_seq, int64_t n_q,
            int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max, const kv_pages *pg, int len_bias, int causal, float scale, float *d_dst, int64_t ldd_tok,
            int64_t ldd_head, void *d_work, size_t work_bytes, void *stream) {
    int rc = check_mla_rows(n_seq * n_q, ldq_tok, ldq_head, ldd_tok, ldd_head);
    if (rc) return rc;
    if (n_q == 0) return GGML_HIP_OK;
    if (!d_q || !d_dst || ((pg || n_kv_max > 0) && !d_cache)) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_q | (uintptr_t)d_dst | (uintptr_t)d_cache) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "q, dst and the cache must be 16-byte aligned");
    const mla_plan p = plan_attn_mla(kv_type, n_head, n_seq, n_q, n_kv_max);
    if (p.form == MLA_FORM_NONE) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    const size_t need = work_size(kv_type, MLA_DK, MLA_DV, n_head, n_seq, n_q, n_kv_max);
    if (need && (!d_work || work_bytes < need)) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_attn_mla_work_size)", need);
    mla_args a;
    a.kv_type = kv_type; a.n_head = n_head; a.causal = causal != 0;
    a.q = d_q; a.ldq_tok = ldq_tok; a.ldq_head = ldq_head;
    a.cache = d_cache; a.nb_pos = nb_pos;
    a.n_q = n_q; a.n_kv = d_n_kv ? 0 : n_kv; a.d_n_kv = d_n_kv; a.n_kv_max = n_kv_max;
    a.scale = scale;
    a.dst = d_dst; a.ldd_tok = ldd_tok; a.ldd_head = ldd_head;
    a.work = need ? (float *)(((uintptr_t)d_work + MLA_ALIGN - 1) / MLA_ALIGN * MLA_ALIGN) : nullptr;
    a.n_spans = p.n_spans;
    HIP_TRY(launch_attn_mla(p, a, n_seq, pg, len_bias, (hipStream_t)stream));
    return GGML_HIP_OK;
}

}  // namespace

extern "C" {

int ggml_hip_attn_mla_plan(int kv_type, int D_k, int D_v, int n_head, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_mla_plan_t *out) {
    return put_plan(kv_type, D_k, D_v, n_head, 1, n_q, n_kv_max, out);
}

size_t ggml_hip_attn_mla_work_size(int kv_type, int D_k, int D_v, int n_head, int64_t n_q, int64_t n_kv_max) {
    return work_size(kv_type, D_k, D_v, n_head, 1, n_q, n_kv_max);
}

int ggml_hip_attn_mla_paged_plan(int kv_type, int D_k, int D_v, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_mla_plan_t *out) {
    return put_plan(kv_type, D_k, D_v, n_head, n_seq, n_q, n_kv_max, out);
}

size_t ggml_hip_attn_mla_paged_work_size(int kv_type, int D_k, int D_v, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max) {
    return work_size(kv_type, D_k, D_v, n_head, n_seq, n_q, n_kv_max);
}

int ggml_hip_attn_mla_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_cache, int64_t nb_pos, int n_head, int D_k, int D_v,
                          int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max, int causal, float scale, float *d_dst, int64_t ldd_tok,
                          int64_t ldd_head, void *d_work, size_t work_bytes, void *stream) {
    const int rc = check_mla_shape(kv_type, D_k, D_v, n_head, 1, n_q, n_kv_max);
    if (rc) return rc;
    if (!d_n_kv && (n_kv < 0 || n_kv > n_kv_max)) return fail(GGML_HIP_ERR_ARG, "n_kv %lld outside [0, n_kv_max %lld]", (long long)n_kv, (long long)n_kv_max);
    if (((uintptr_t)d_n_kv & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_n_kv must be 4-byte aligned");
    if (nb_pos % 16 != 0 || nb_pos < latent_row_bytes(kv_type) || nb_pos > ((int64_t)1 << 40))
        return fail(GGML_HIP_ERR_SHAPE, "nb_pos %lld: a multiple of 16 bytes, at least the %lld bytes of a row", (long long)nb_pos, (long long)latent_row_bytes(kv_type));
    return mla_run(kv_type, d_q, ldq_tok, ldq_head, d_cache, nb_pos, n_head, 1, n_q, n_kv, d_n_kv, n_kv_max, nullptr, 0, causal, scale, d_dst, ldd_tok, ldd_head, d_work,
                   work_bytes, stream);
}

int ggml_hip_attn_mla_paged_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_pool, int64_t nb_page, int64_t nb_pos, int n_pages,
                                const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq, int n_head, int D_k, int D_v,
                                int64_t n_q, int64_t n_kv_max, int causal, float scale, float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work,
                                size_t work_bytes, void *stream) {
    int rc = check_mla_shape(kv_type, D_k, D_v, n_head, n_seq, n_q, n_kv_max);
    if (rc) return rc;
    kv_pages pg;
    rc = check_latent_pages(kv_type, nb_page, nb_pos, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    return mla_run(kv_type, d_q, ldq_tok, ldq_head, d_pool, nb_pos, n_head, n_seq, n_q, 0, nullptr, n_kv_max, &pg, len_bias, causal, scale, d_dst, ldd_tok, ldd_head,
                   d_work, work_bytes, stream);
}

int ggml_hip_kv_store_latent_paged_dev(int kv_type, const float *d_src, int64_t ld, int64_t n_seq, int64_t n_q, void *d_pool, int64_t nb_page, int64_t nb_pos,
                                       int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max, void *stream) {
    kv_pages pg;
    const int rc = check_latent_pages(kv_type, nb_page, nb_pos, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    if (n_q < 0) return fail(GGML_HIP_ERR_ARG, "n_q %lld", (long long)n_q);
    if (n_seq * n_q > ATTN_PAGED_MAX_ROWS) return fail(GGML_HIP_ERR_SHAPE, "n_seq * n_q %lld (<= %lld)", (long long)(n_seq * n_q), (long long)ATTN_PAGED_MAX_ROWS);
    if (ld % 4 != 0 || ld < 0 || (n_seq * n_q > 1 && ld < MLA_DK)) return fail(GGML_HIP_ERR_SHAPE, "ld %lld: a multiple of 4 elements, at least %d", (long long)ld, MLA_DK);
    if (n_q == 0) return GGML_HIP_OK;
    if (!d_src || !d_pool) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_src | (uintptr_t)d_pool) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_src and d_pool must be 16-byte aligned");
    HIP_TRY(launch_kv_store_latent_paged(kv_type, d_src, ld, n_seq, n_q, d_pool, nb_pos, pg, (hipStream_t)stream));
    return GGML_HIP_OK;
}

}  // extern "C"
