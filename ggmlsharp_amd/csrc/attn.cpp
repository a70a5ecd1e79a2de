// attn.cpp -- the C-ABI of include/ggml_hip_ext.h, attention over a KV cache: rows into the cache (ggml_hip_kv_store_dev), the attention
// itself (ggml_hip_attn_dev), its plan and work size, the paged entries, the ragged entries (a query count per sequence on the device), and the _ex entries with a sliding window, sinks and a soft-cap
// (one checked path serves an entry and its _ex twin), the _bias entries with a mask tensor and ALiBi slopes on top of those (the same paths once more), and
// ggml_hip_alibi_slopes (host only).  The kernels and their arithmetic are attn.hip's, the form is plan.cpp's (plan_attn).
// No set, no handle: stream-ordered launches on the current device, no synchronize, no allocation; capturable.
#include "ctx.h"
#include <cfloat>
#include <cmath>

using namespace ghip;

namespace {

constexpr size_t ATTN_ALIGN = 256;

int kv_type_ok(int kv_type) { return kv_type == GGML_TYPE_F16 || kv_type == GGML_TYPE_Q8_0; }

// the shape rules of ggml_hip_attn_dev shared by the plan and the work size; 0 or an error code
int check_attn_shape(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max) {
    if (!kv_type_ok(kv_type)) return fail(GGML_HIP_ERR_TYPE, "kv_type %d: the cache is F16 or Q8_0", kv_type);
    if (D != 64 && D != 128) return fail(GGML_HIP_ERR_SHAPE, "head size %d (64 or 128)", D);
    if (n_head < 1 || n_head_kv < 1 || n_head % n_head_kv != 0 || n_head / n_head_kv > 16 || n_head > 65535)
        return fail(GGML_HIP_ERR_SHAPE, "n_head %d over n_head_kv %d: the group size must be an integer in 1 .. 16", n_head, n_head_kv);
    if (n_q < 0 || n_kv_max < 0) return fail(GGML_HIP_ERR_ARG, "n_q %lld, n_kv_max %lld", (long long)n_q, (long long)n_kv_max);
    if (n_q > (1 << 20) || n_kv_max > (1 << 24) || n_q * n_head > 0x7FFFFFFF)
        return fail(GGML_HIP_ERR_SHAPE, "n_q %lld (<= 2^20), n_kv_max %lld (<= 2^24)", (long long)n_q, (long long)n_kv_max);
    return GGML_HIP_OK;
}

// the shape rules of q / dst rows [rows][n_head][D]
int check_attn_rows(int D, int64_t rows, int64_t ldq_tok, int64_t ldq_head, int64_t ldd_tok, int64_t ldd_head) {
    if (ldq_tok % 4 != 0 || ldq_head % 4 != 0 || ldd_tok % 4 != 0 || ldd_head % 4 != 0 || ldq_head < D || ldd_head < D || ldq_tok < 0 || ldd_tok < 0 ||
        (rows > 1 && (ldq_tok < D || ldd_tok < D)))
        return fail(GGML_HIP_ERR_SHAPE, "the strides of q and dst are multiples of 4 elements, at least D");
    return GGML_HIP_OK;
}

// the rules of a ggml_hip_attn_opts_t; 0 or an error code.  *on: one of the three options is set (else the base kernels run); vo: the kernels' form
int check_attn_opts(const ggml_hip_attn_opts_t *opts, int causal, float scale, bool *on, attn_var *vo) {
    *on = false;
    *vo = attn_var{};
    if (!opts) return GGML_HIP_OK;
    if (opts->reserved != 0) return fail(GGML_HIP_ERR_ARG, "opts->reserved %d must be 0", (int)opts->reserved);
    if (opts->window < 0) return fail(GGML_HIP_ERR_ARG, "window %lld (0: none, or >= 1)", (long long)opts->window);
    if (opts->window > 0 && !causal) return fail(GGML_HIP_ERR_ARG, "a window needs causal != 0");
    if (!(opts->logit_softcap >= 0.0f) || opts->logit_softcap > FLT_MAX) return fail(GGML_HIP_ERR_ARG, "logit_softcap must be 0 or a finite positive number");
    if (((uintptr_t)opts->d_sinks & 3) != 0) return fail(GGML_HIP_ERR_ARG, "d_sinks must be 4-byte aligned");
    vo->sinks = opts->d_sinks;
    vo->window = (int)(opts->window > ((int64_t)1 << 30) ? ((int64_t)1 << 30) : opts->window);      // (n_kv_max <= 2^24: beyond it every window is "none")
    vo->cap = opts->logit_softcap;
    vo->sc = vo->cap != 0.0f ? scale / vo->cap : 0.0f;               // ONE binary32 division (the header's sc')
    *on = vo->sinks || vo->window > 0 || vo->cap != 0.0f;
    return GGML_HIP_OK;
}

// the rules of a ggml_hip_attn_bias_t; 0 or an error code.  *on: a mask is given (else the _ex / ragged entry's own kernels run); bs: the kernels' form
int check_attn_bias(const ggml_hip_attn_bias_t *bias, int64_t n_kv_max, bool *on, attn_bias *bs) {
    *on = false;
    *bs = attn_bias{};
    if (!bias || (!bias->d_mask && !bias->d_slopes)) return GGML_HIP_OK;
    if (((uintptr_t)bias->d_slopes & 3) != 0) return fail(GGML_HIP_ERR_ARG, "d_slopes must be 4-byte aligned");
    if (!bias->d_mask) return fail(GGML_HIP_ERR_ARG, "d_slopes without d_mask: there is nothing to multiply");
    if (bias->ld_mask < n_kv_max || bias->ld_mask % 8 != 0 || ((uintptr_t)bias->d_mask & 15) != 0)
        return fail(GGML_HIP_ERR_SHAPE, "ld_mask %lld (>= n_kv_max %lld, a multiple of 8 halves), d_mask 16-byte aligned", (long long)bias->ld_mask, (long long)n_kv_max);
    bs->mask = (const uint16_t *)bias->d_mask; bs->ld = bias->ld_mask; bs->slopes = bias->d_slopes;
    *on = true;
    return GGML_HIP_OK;
}

// ggml_hip_attn_dev behind its refusal of upstream's extras, and ggml_hip_attn_ex_dev behind check_attn_opts: on / vo are its answer (off from the base entry)
int attn_run(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_pos, int64_t nb_head, int n_head,
             int n_head_kv, int D, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max, int causal, float scale, bool on, const attn_var &vo,
             float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream, const attn_bias *bs = nullptr) {
    int rc = check_attn_shape(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (rc) return rc;
    if (!d_n_kv && (n_kv < 0 || n_kv > n_kv_max)) return fail(GGML_HIP_ERR_ARG, "n_kv %lld outside [0, n_kv_max %lld]", (long long)n_kv, (long long)n_kv_max);
    const int64_t row_bytes = kv_type == GGML_TYPE_Q8_0 ? D / QK * (int64_t)sizeof(block_q8_0) : D * 2;
    if (ldq_tok % 4 != 0 || ldq_head % 4 != 0 || ldd_tok % 4 != 0 || ldd_head % 4 != 0 || ldq_head < D || ldd_head < D || ldq_tok < 0 || ldd_tok < 0 ||
        (n_q > 1 && (ldq_tok < D || ldd_tok < D)))
        return fail(GGML_HIP_ERR_SHAPE, "the strides of q and dst are multiples of 4 elements, at least D");
    if (nb_pos % 16 != 0 || nb_head % 16 != 0 || nb_pos < row_bytes || nb_head < row_bytes)
        return fail(GGML_HIP_ERR_SHAPE, "nb_pos %lld, nb_head %lld: multiples of 16 bytes, at least the %lld bytes of a row", (long long)nb_pos, (long long)nb_head,
                    (long long)row_bytes);
    if (n_q == 0) return GGML_HIP_OK;
    if (!d_q || !d_dst || (n_kv_max > 0 && (!d_k || !d_v))) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_q | (uintptr_t)d_dst | (uintptr_t)d_k | (uintptr_t)d_v) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "q, dst, K and V must be 16-byte aligned");
    on = on || bs;                                                   // (a mask runs the option bodies, whatever vo holds; window 0 plans like the base entry)
    const attn_plan p = on ? plan_attn_ex(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, vo.window) : plan_attn(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    const size_t need = ggml_hip_attn_work_size(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (need && (!d_work || work_bytes < need)) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_attn_work_size)", need);
    attn_args a;
    a.kv_type = kv_type; a.D = D; a.n_head = n_head; a.n_head_kv = n_head_kv; a.causal = causal != 0;
    a.q = d_q; a.ldq_tok = ldq_tok; a.ldq_head = ldq_head;
    a.k = d_k; a.v = d_v; a.nb_pos = nb_pos; a.nb_head = nb_head;
    a.n_q = n_q; a.n_kv = d_n_kv ? 0 : n_kv; a.d_n_kv = d_n_kv; a.n_kv_max = n_kv_max;
    a.scale = scale;
    a.dst = d_dst; a.ldd_tok = ldd_tok; a.ldd_head = ldd_head;
    a.work = need ? (void *)(((uintptr_t)d_work + ATTN_ALIGN - 1) / ATTN_ALIGN * ATTN_ALIGN) : nullptr;
    if (on) HIP_TRY(launch_attn_ex(p, a, vo, (hipStream_t)stream, bs));
    else HIP_TRY(launch_attn(p, a, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int attn_paged_run(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos,
                   int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq, int n_head,
                   int n_head_kv, int D, int64_t n_q, int64_t n_kv_max, int causal, float scale, bool on, const attn_var &vo, float *d_dst, int64_t ldd_tok,
                   int64_t ldd_head, void *d_work, size_t work_bytes, void *stream, const attn_bias *bs = nullptr) {
    int rc = check_attn_shape(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (rc) return rc;
    kv_pages pg;
    rc = check_kv_pages(kv_type, D, n_head_kv, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    if (n_seq * n_q > ATTN_PAGED_MAX_ROWS || n_seq * n_q * n_head > 0x7FFFFFFF)
        return fail(GGML_HIP_ERR_SHAPE, "n_seq * n_q %lld (<= %lld, times n_head below 2^31)", (long long)(n_seq * n_q), (long long)ATTN_PAGED_MAX_ROWS);
    rc = check_attn_rows(D, n_seq * n_q, ldq_tok, ldq_head, ldd_tok, ldd_head);
    if (rc) return rc;
    if (n_q == 0) return GGML_HIP_OK;
    if (!d_q || !d_dst || !d_k || !d_v) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_q | (uintptr_t)d_dst | (uintptr_t)d_k | (uintptr_t)d_v) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "q, dst, K and V must be 16-byte aligned");
    on = on || bs;
    const attn_plan p = on ? plan_attn_paged_ex(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, vo.window)
                           : plan_attn_paged(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    const size_t need = ggml_hip_attn_paged_work_size(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max);
    if (need && (!d_work || work_bytes < need)) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_attn_paged_work_size)", need);
    attn_args a;
    a.kv_type = kv_type; a.D = D; a.n_head = n_head; a.n_head_kv = n_head_kv; a.causal = causal != 0;
    a.q = d_q; a.ldq_tok = ldq_tok; a.ldq_head = ldq_head;
    a.k = d_k; a.v = d_v; a.nb_pos = nb_pos; a.nb_head = nb_head;
    a.n_q = n_q; a.n_kv = 0; a.d_n_kv = nullptr; a.n_kv_max = n_kv_max;
    a.scale = scale;
    a.dst = d_dst; a.ldd_tok = ldd_tok; a.ldd_head = ldd_head;
    a.work = need ? (void *)(((uintptr_t)d_work + ATTN_ALIGN - 1) / ATTN_ALIGN * ATTN_ALIGN) : nullptr;
    if (on) HIP_TRY(launch_attn_paged_ex(p, a, n_seq, pg, len_bias, vo, (hipStream_t)stream, bs));
    else HIP_TRY(launch_attn_paged(p, a, n_seq, pg, len_bias, (hipStream_t)stream));
    return GGML_HIP_OK;
}

// the shape of a RAGGED call's plan and work size: plan_attn_ragged's refusals as codes
int check_attn_ragged_shape(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_tokens_max, int64_t n_dec_rows_max, int64_t n_kv_max) {
    const int rc = check_attn_shape(kv_type, D, n_head, n_head_kv, n_tokens_max < 0 ? 0 : n_tokens_max, n_kv_max);     // (n_tokens_max <= 2^20, times n_head below 2^31)
    if (rc) return rc;
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    if (n_tokens_max < 0) return fail(GGML_HIP_ERR_ARG, "n_tokens_max %lld", (long long)n_tokens_max);
    if (n_dec_rows_max < 0 || n_dec_rows_max > n_tokens_max)
        return fail(GGML_HIP_ERR_ARG, "n_dec_rows_max %lld outside [0, n_tokens_max %lld]", (long long)n_dec_rows_max, (long long)n_tokens_max);
    return GGML_HIP_OK;
}

// the plan of the public struct
void put_plan(const attn_plan &p, ggml_hip_attn_plan_t *out) {
    out->form = p.form; out->chunk = p.chunk; out->q_tile = p.q_tile; out->launches = p.launches;
    out->n_chunks = p.n_chunks; out->workgroups = p.wgs;
}

}  // namespace

namespace ghip {

int check_kv_pages(int kv_type, int D, int n_head_kv, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages,
                   const int32_t *d_len, int64_t n_seq, int64_t n_kv_max, kv_pages *pg) {
    if (!kv_type_ok(kv_type)) return fail(GGML_HIP_ERR_TYPE, "kv_type %d: the cache is F16 or Q8_0", kv_type);
    if (D < 4 || D % (kv_type == GGML_TYPE_Q8_0 ? QK : 4) != 0 || D > 256) return fail(GGML_HIP_ERR_SHAPE, "head size %d", D);
    if (n_head_kv < 1 || n_head_kv > 65535) return fail(GGML_HIP_ERR_SHAPE, "n_head_kv %d (1 .. 65535)", n_head_kv);
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    if (n_kv_max < 0) return fail(GGML_HIP_ERR_ARG, "n_kv_max %lld", (long long)n_kv_max);
    if (n_kv_max > (1 << 24)) return fail(GGML_HIP_ERR_SHAPE, "n_kv_max %lld (<= 2^24)", (long long)n_kv_max);
    const int64_t row_bytes = kv_type == GGML_TYPE_Q8_0 ? D / QK * (int64_t)sizeof(block_q8_0) : D * 2;
    if (nb_pos % 16 != 0 || nb_head % 16 != 0 || nb_pos < row_bytes || nb_head < row_bytes)
        return fail(GGML_HIP_ERR_SHAPE, "nb_pos %lld, nb_head %lld: multiples of 16 bytes, at least the %lld bytes of a row", (long long)nb_pos, (long long)nb_head,
                    (long long)row_bytes);
    if (nb_pos > ((int64_t)1 << 40) || nb_head > ((int64_t)1 << 40)) return fail(GGML_HIP_ERR_SHAPE, "nb_pos %lld, nb_head %lld", (long long)nb_pos, (long long)nb_head);
    const int64_t span = (ATTN_CHUNK - 1) * nb_pos + (n_head_kv - 1) * nb_head + row_bytes;      // the bytes the rows of one page span
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


int check_kv_ragged(const int32_t *d_q_start, int64_t n_seq, int64_t n_tokens_max, kv_ragged *rg) {
    if (!d_q_start) return fail(GGML_HIP_ERR_ARG, "d_q_start must not be null");
    if (((uintptr_t)d_q_start & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_q_start must be 4-byte aligned");
    if (n_tokens_max < 0) return fail(GGML_HIP_ERR_ARG, "n_tokens_max %lld", (long long)n_tokens_max);
    if (n_tokens_max > ATTN_PAGED_MAX_ROWS) return fail(GGML_HIP_ERR_SHAPE, "n_tokens_max %lld (<= %lld)", (long long)n_tokens_max, (long long)ATTN_PAGED_MAX_ROWS);
    rg->q_start = d_q_start; rg->n_seq = (int)n_seq; rg->n_tokens_max = (int)n_tokens_max;      // (n_seq: check_kv_pages')
    return GGML_HIP_OK;
}

}  // namespace ghip

extern "C" {

int ggml_hip_kv_store_dev(int kv_type, const float *d_src, int64_t ld, int64_t n_rows, int64_t row_elems, void *d_cache, int64_t nb_pos,
                          int64_t n_pos_max, int64_t pos0, const int32_t *d_pos0, void *stream) {
    if (!kv_type_ok(kv_type)) return fail(GGML_HIP_ERR_TYPE, "kv_type %d: the cache is F16 or Q8_0", kv_type);
    if (n_rows < 0 || n_pos_max < 0) return fail(GGML_HIP_ERR_ARG, "n_rows %lld, n_pos_max %lld", (long long)n_rows, (long long)n_pos_max);
    const int64_t unit = kv_type == GGML_TYPE_Q8_0 ? QK : 4;
    if (row_elems < 1 || row_elems % unit != 0 || row_elems > ((int64_t)1 << 24) || n_rows > ((int64_t)1 << 24))
        return fail(GGML_HIP_ERR_SHAPE, "row_elems %lld (a multiple of %lld, <= 2^24), n_rows %lld (<= 2^24)", (long long)row_elems, (long long)unit, (long long)n_rows);
    const int64_t row_bytes = kv_type == GGML_TYPE_Q8_0 ? row_elems / QK * (int64_t)sizeof(block_q8_0) : row_elems * 2;
    if (ld < row_elems || ld % 4 != 0 || nb_pos < row_bytes || nb_pos % 16 != 0)
        return fail(GGML_HIP_ERR_SHAPE, "ld %lld (>= row_elems, a multiple of 4), nb_pos %lld (>= %lld row bytes, a multiple of 16)", (long long)ld, (long long)nb_pos,
                    (long long)row_bytes);
    if (n_rows == 0) return GGML_HIP_OK;
    if (!d_src || !d_cache) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (((uintptr_t)d_src & 15) != 0 || ((uintptr_t)d_cache & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_src and d_cache must be 16-byte aligned");
    HIP_TRY(launch_kv_store(kv_type, d_src, ld, n_rows, row_elems, d_cache, nb_pos, n_pos_max, pos0, d_pos0, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_attn_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    const int rc = check_attn_shape(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (rc) return rc;
    if (n_q == 0) { *out = ggml_hip_attn_plan_t{}; out->chunk = ATTN_CHUNK; return GGML_HIP_OK; }
    const attn_plan p = plan_attn(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    out->form = p.form; out->chunk = p.chunk; out->q_tile = p.q_tile; out->launches = p.launches;
    out->n_chunks = p.n_chunks; out->workgroups = p.wgs;
    return GGML_HIP_OK;
}

size_t ggml_hip_attn_work_size(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max) {
    if (!kv_type_ok(kv_type) || n_q <= 0) return 0;
    const attn_plan p = plan_attn(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE || p.work_bytes == 0) return 0;
    return (p.work_bytes + ATTN_ALIGN - 1) / ATTN_ALIGN * ATTN_ALIGN + ATTN_ALIGN;   // (the base is rounded up to a 256-byte boundary)
}

int ggml_hip_attn_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_pos, int64_t nb_head,
                      int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max, int causal, float scale,
                      const void *d_mask, float max_bias, float logit_softcap, const float *d_sinks, float *d_dst, int64_t ldd_tok, int64_t ldd_head,
                      void *d_work, size_t work_bytes, void *stream) {
    if (d_mask || d_sinks || max_bias != 0.0f || logit_softcap != 0.0f)
        return fail(GGML_HIP_ERR_ARG, "a mask tensor, ALiBi (max_bias), a soft-cap and sinks are not served: pass NULL / 0");
    return attn_run(kv_type, d_q, ldq_tok, ldq_head, d_k, d_v, nb_pos, nb_head, n_head, n_head_kv, D, n_q, n_kv, d_n_kv, n_kv_max, causal, scale, false, attn_var{},
                    d_dst, ldd_tok, ldd_head, d_work, work_bytes, stream);
}

int ggml_hip_attn_ex_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max, const ggml_hip_attn_opts_t *opts,
                          ggml_hip_attn_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    bool on; attn_var vo;
    int rc = check_attn_opts(opts, 1, 1.0f, &on, &vo);               // (a plan has no causal flag: the entry refuses a window without it)
    if (rc) return rc;
    rc = check_attn_shape(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (rc) return rc;
    if (n_q == 0) { *out = ggml_hip_attn_plan_t{}; out->chunk = ATTN_CHUNK; return GGML_HIP_OK; }
    const attn_plan p = plan_attn_ex(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, vo.window);
    if (p.form == ATTN_FORM_NONE) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    put_plan(p, out);
    return GGML_HIP_OK;
}

int ggml_hip_attn_ex_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_pos, int64_t nb_head,
                         int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max, int causal, float scale,
                         const ggml_hip_attn_opts_t *opts, float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream) {
    bool on; attn_var vo;
    const int rc = check_attn_opts(opts, causal, scale, &on, &vo);
    if (rc) return rc;
    return attn_run(kv_type, d_q, ldq_tok, ldq_head, d_k, d_v, nb_pos, nb_head, n_head, n_head_kv, D, n_q, n_kv, d_n_kv, n_kv_max, causal, scale, on, vo, d_dst,
                    ldd_tok, ldd_head, d_work, work_bytes, stream);
}

int ggml_hip_kv_store_paged_dev(int kv_type, const float *d_src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D, int64_t n_seq, int64_t n_q,
                                void *d_pool, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages,
                                const int32_t *d_len, int64_t n_kv_max, void *stream) {
    kv_pages pg;
    const int rc = check_kv_pages(kv_type, D, n_head_kv, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    if (n_q < 0) return fail(GGML_HIP_ERR_ARG, "n_q %lld", (long long)n_q);
    if (n_seq * n_q > ATTN_PAGED_MAX_ROWS) return fail(GGML_HIP_ERR_SHAPE, "n_seq * n_q %lld (<= %lld)", (long long)(n_seq * n_q), (long long)ATTN_PAGED_MAX_ROWS);
    if (ldx_tok % 4 != 0 || ldx_head % 4 != 0 || ldx_head < D || ldx_tok < 0 || (n_seq * n_q > 1 && ldx_tok < D))
        return fail(GGML_HIP_ERR_SHAPE, "the strides of the rows are multiples of 4 elements, at least D");
    if (n_q == 0) return GGML_HIP_OK;
    if (!d_src || !d_pool) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_src | (uintptr_t)d_pool) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_src and d_pool must be 16-byte aligned");
    HIP_TRY(launch_kv_store_paged(kv_type, d_src, ldx_tok, ldx_head, n_head_kv, D, n_seq, n_q, d_pool, nb_pos, nb_head, pg, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_attn_paged_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    const int rc = check_attn_shape(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (rc) return rc;
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    if (n_q == 0) { *out = ggml_hip_attn_plan_t{}; out->chunk = ATTN_CHUNK; return GGML_HIP_OK; }
    const attn_plan p = plan_attn_paged(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE)
        return fail(GGML_HIP_ERR_SHAPE, "the shape is not served: n_seq * n_q %lld (<= %lld), times n_head below 2^31", (long long)(n_seq * n_q), (long long)ATTN_PAGED_MAX_ROWS);
    out->form = p.form; out->chunk = p.chunk; out->q_tile = p.q_tile; out->launches = p.launches;
    out->n_chunks = p.n_chunks; out->workgroups = p.wgs;
    return GGML_HIP_OK;
}

size_t ggml_hip_attn_paged_work_size(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max) {
    if (!kv_type_ok(kv_type) || n_q <= 0 || n_seq <= 0) return 0;
    const attn_plan p = plan_attn_paged(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE || p.work_bytes == 0) return 0;
    return (p.work_bytes + ATTN_ALIGN - 1) / ATTN_ALIGN * ATTN_ALIGN + ATTN_ALIGN;   // (the base is rounded up to a 256-byte boundary)
}

int ggml_hip_attn_paged_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos,
                            int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq,
                            int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv_max, int causal, float scale, const void *d_mask, float max_bias,
                            float logit_softcap, const float *d_sinks, float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes,
                            void *stream) {
    if (d_mask || d_sinks || max_bias != 0.0f || logit_softcap != 0.0f)
        return fail(GGML_HIP_ERR_ARG, "a mask tensor, ALiBi (max_bias), a soft-cap and sinks are not served: pass NULL / 0");
    return attn_paged_run(kv_type, d_q, ldq_tok, ldq_head, d_k, d_v, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, len_bias, n_seq, n_head,
                          n_head_kv, D, n_q, n_kv_max, causal, scale, false, attn_var{}, d_dst, ldd_tok, ldd_head, d_work, work_bytes, stream);
}

int ggml_hip_attn_paged_ex_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max, const ggml_hip_attn_opts_t *opts,
                                ggml_hip_attn_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    bool on; attn_var vo;
    int rc = check_attn_opts(opts, 1, 1.0f, &on, &vo);
    if (rc) return rc;
    rc = check_attn_shape(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (rc) return rc;
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    if (n_q == 0) { *out = ggml_hip_attn_plan_t{}; out->chunk = ATTN_CHUNK; return GGML_HIP_OK; }
    const attn_plan p = plan_attn_paged_ex(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max, vo.window);
    if (p.form == ATTN_FORM_NONE)
        return fail(GGML_HIP_ERR_SHAPE, "the shape is not served: n_seq * n_q %lld (<= %lld), times n_head below 2^31", (long long)(n_seq * n_q), (long long)ATTN_PAGED_MAX_ROWS);
    put_plan(p, out);
    return GGML_HIP_OK;
}

int ggml_hip_attn_paged_ex_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos,
                               int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq,
                               int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv_max, int causal, float scale, const ggml_hip_attn_opts_t *opts,
                               float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream) {
    bool on; attn_var vo;
    const int rc = check_attn_opts(opts, causal, scale, &on, &vo);
    if (rc) return rc;
    return attn_paged_run(kv_type, d_q, ldq_tok, ldq_head, d_k, d_v, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, len_bias, n_seq, n_head,
                          n_head_kv, D, n_q, n_kv_max, causal, scale, on, vo, d_dst, ldd_tok, ldd_head, d_work, work_bytes, stream);
}

int ggml_hip_alibi_slopes(int n_head, float max_bias, float *out) {
    if (n_head < 1 || n_head > 65535) return fail(GGML_HIP_ERR_ARG, "n_head %d (1 .. 65535)", n_head);
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    if (!(max_bias >= 0.0f) || max_bias > FLT_MAX) return fail(GGML_HIP_ERR_ARG, "max_bias must be 0 or a finite positive number");
    int n2 = 1;
    while (2 * n2 <= n_head) n2 *= 2;                                // 2^floor(log2 n_head)
    const float m0 = powf(2.0f, -max_bias / (float)n2), m1 = powf(2.0f, -(max_bias / 2.0f) / (float)n2);
    for (int h = 0; h < n_head; ++h)
        out[h] = max_bias == 0.0f ? 1.0f : h < n2 ? powf(m0, (float)(h + 1)) : powf(m1, (float)(2 * (h - n2) + 1));
    return GGML_HIP_OK;
}

int ggml_hip_attn_bias_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_pos, int64_t nb_head,
                           int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max, int causal, float scale,
                           const ggml_hip_attn_opts_t *opts, const ggml_hip_attn_bias_t *bias, float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work,
                           size_t work_bytes, void *stream) {
    bool on; attn_var vo;
    int rc = check_attn_opts(opts, causal, scale, &on, &vo);
    if (rc) return rc;
    bool mon; attn_bias bs;
    rc = check_attn_bias(bias, n_kv_max, &mon, &bs);
    if (rc) return rc;
    return attn_run(kv_type, d_q, ldq_tok, ldq_head, d_k, d_v, nb_pos, nb_head, n_head, n_head_kv, D, n_q, n_kv, d_n_kv, n_kv_max, causal, scale, on, vo, d_dst,
                    ldd_tok, ldd_head, d_work, work_bytes, stream, mon ? &bs : nullptr);
}

int ggml_hip_attn_paged_bias_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos,
                                 int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq,
                                 int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv_max, int causal, float scale, const ggml_hip_attn_opts_t *opts,
                                 const ggml_hip_attn_bias_t *bias, float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream) {
    bool on; attn_var vo;
    int rc = check_attn_opts(opts, causal, scale, &on, &vo);
    if (rc) return rc;
    bool mon; attn_bias bs;
    rc = check_attn_bias(bias, n_kv_max, &mon, &bs);
    if (rc) return rc;
    return attn_paged_run(kv_type, d_q, ldq_tok, ldq_head, d_k, d_v, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, len_bias, n_seq, n_head,
                          n_head_kv, D, n_q, n_kv_max, causal, scale, on, vo, d_dst, ldd_tok, ldd_head, d_work, work_bytes, stream, mon ? &bs : nullptr);
}

int ggml_hip_ragged_positions_dev(const int32_t *d_q_start, const int32_t *d_len, int64_t n_seq, int64_t n_tokens_max, int32_t *d_pos, void *stream) {
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    kv_ragged rg;
    const int rc = check_kv_ragged(d_q_start, n_seq, n_tokens_max, &rg);
    if (rc) return rc;
    if (!d_len) return fail(GGML_HIP_ERR_ARG, "d_len must not be null");
    if (((uintptr_t)d_len & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_len must be 4-byte aligned");
    if (n_tokens_max == 0) return GGML_HIP_OK;
    if (!d_pos) return fail(GGML_HIP_ERR_ARG, "d_pos must not be null");
    if (((uintptr_t)d_pos & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_pos must be 4-byte aligned");
    HIP_TRY(launch_ragged_positions(rg, d_len, d_pos, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_ragged_last_rows_dev(const float *d_x, int64_t ldx, const int32_t *d_q_start, int64_t n_seq, int64_t n_tokens_max, int64_t K, float *d_dst,
                                  int64_t ldd, void *stream) {
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    kv_ragged rg;
    const int rc = check_kv_ragged(d_q_start, n_seq, n_tokens_max, &rg);
    if (rc) return rc;
    if (K < 0 || K > ((int64_t)1 << 24)) return fail(GGML_HIP_ERR_SHAPE, "K %lld (0 .. 2^24)", (long long)K);
    if (ldx < K || ldd < K) return fail(GGML_HIP_ERR_SHAPE, "ldx %lld and ldd %lld must be at least K %lld", (long long)ldx, (long long)ldd, (long long)K);
    if (K == 0) return GGML_HIP_OK;
    if (!d_x || !d_dst) return fail(GGML_HIP_ERR_ARG, "d_x and d_dst must not be null");
    if ((((uintptr_t)d_x | (uintptr_t)d_dst) & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_x and d_dst must be 4-byte aligned");
    HIP_TRY(launch_ragged_last_rows(rg, d_x, ldx, K, d_dst, ldd, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_kv_store_paged_ragged_dev(int kv_type, const float *d_src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D, int64_t n_seq,
                                       const int32_t *d_q_start, int64_t n_tokens_max, void *d_pool, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                       const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max, void *stream) {
    kv_pages pg;
    int rc = check_kv_pages(kv_type, D, n_head_kv, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    kv_ragged rg;
    rc = check_kv_ragged(d_q_start, n_seq, n_tokens_max, &rg);
    if (rc) return rc;
    if (ldx_tok % 4 != 0 || ldx_head % 4 != 0 || ldx_head < D || ldx_tok < 0 || (n_tokens_max > 1 && ldx_tok < D))
        return fail(GGML_HIP_ERR_SHAPE, "the strides of the rows are multiples of 4 elements, at least D");
    if (n_tokens_max == 0) return GGML_HIP_OK;
    if (!d_src || !d_pool) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_src | (uintptr_t)d_pool) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_src and d_pool must be 16-byte aligned");
    HIP_TRY(launch_kv_store_paged_ragged(kv_type, d_src, ldx_tok, ldx_head, n_head_kv, D, rg, d_pool, nb_pos, nb_head, pg, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_attn_paged_ragged_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_tokens_max, int64_t n_dec_rows_max, int64_t n_kv_max,
                                    const ggml_hip_attn_opts_t *opts, ggml_hip_attn_ragged_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    bool on; attn_var vo;
    int rc = check_attn_opts(opts, 1, 1.0f, &on, &vo);               // (a plan has no causal flag: the entry refuses a window without it)
    if (rc) return rc;
    rc = check_attn_ragged_shape(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max);
    if (rc) return rc;
    const attn_ragged_plan p = plan_attn_ragged(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, vo.window);
    if (!p.ok) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    *out = ggml_hip_attn_ragged_plan_t{};
    out->chunk = p.chunk; out->launches = p.launches; out->n_chunks = p.n_chunks; out->max_tiles = p.max_tiles;
    out->decode_workgroups = p.decode_wgs; out->merge_workgroups = p.merge_wgs; out->prompt_workgroups = p.prompt_wgs;
    out->index_bytes = (int64_t)p.part_off;
    return GGML_HIP_OK;
}

size_t ggml_hip_attn_paged_ragged_work_size(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_tokens_max, int64_t n_dec_rows_max,
                                            int64_t n_kv_max) {
    const attn_ragged_plan p = plan_attn_ragged(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, 0);
    if (!p.ok || p.work_bytes == 0) return 0;
    return (p.work_bytes + ATTN_ALIGN - 1) / ATTN_ALIGN * ATTN_ALIGN + ATTN_ALIGN;   // (the base is rounded up to a 256-byte boundary)
}

int ggml_hip_attn_paged_ragged_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_page,
                                   int64_t nb_pos, int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int add_q,
                                   int len_bias, int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, int64_t n_dec_rows_max, int n_head, int n_head_kv,
                                   int D, int64_t n_kv_max, int causal, float scale, const ggml_hip_attn_opts_t *opts, float *d_dst, int64_t ldd_tok,
                                   int64_t ldd_head, void *d_work, size_t work_bytes, void *stream) {
    return ggml_hip_attn_paged_ragged_bias_dev(kv_type, d_q, ldq_tok, ldq_head, d_k, d_v, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, add_q, len_bias,
                                               n_seq, d_q_start, n_tokens_max, n_dec_rows_max, n_head, n_head_kv, D, n_kv_max, causal, scale, opts, nullptr, d_dst,
                                               ldd_tok, ldd_head, d_work, work_bytes, stream);
}

int ggml_hip_attn_paged_ragged_bias_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_k, const void *d_v, int64_t nb_page,
                                        int64_t nb_pos, int64_t nb_head, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int add_q,
                                        int len_bias, int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, int64_t n_dec_rows_max, int n_head,
                                        int n_head_kv, int D, int64_t n_kv_max, int causal, float scale, const ggml_hip_attn_opts_t *opts,
                                        const ggml_hip_attn_bias_t *bias, float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes,
                                        void *stream) {
    bool on; attn_var vo;
    int rc = check_attn_opts(opts, causal, scale, &on, &vo);
    if (rc) return rc;
    bool mon; attn_bias bs;
    rc = check_attn_bias(bias, n_kv_max, &mon, &bs);
    if (rc) return rc;
    rc = check_attn_shape(kv_type, D, n_head, n_head_kv, 0, n_kv_max);
    if (rc) return rc;
    kv_pages pg;
    rc = check_kv_pages(kv_type, D, n_head_kv, nb_page, nb_pos, nb_head, n_pages, d_pages, ld_pages, d_len, n_seq, n_kv_max, &pg);
    if (rc) return rc;
    kv_ragged rg;
    rc = check_kv_ragged(d_q_start, n_seq, n_tokens_max, &rg);
    if (rc) return rc;
    rc = check_attn_ragged_shape(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max);
    if (rc) return rc;
    rc = check_attn_rows(D, n_tokens_max, ldq_tok, ldq_head, ldd_tok, ldd_head);
    if (rc) return rc;
    if (n_tokens_max == 0) return GGML_HIP_OK;
    if (!d_q || !d_dst || !d_k || !d_v) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((((uintptr_t)d_q | (uintptr_t)d_dst | (uintptr_t)d_k | (uintptr_t)d_v) & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "q, dst, K and V must be 16-byte aligned");
    const attn_ragged_plan p = plan_attn_ragged(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, on ? vo.window : 0);
    // (a mask with every option off: vo is all zero, the option bodies' arithmetic is then the base bodies')
    if (!p.ok) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    const size_t need = ggml_hip_attn_paged_ragged_work_size(kv_type, D, n_head, n_head_kv, n_seq, n_tokens_max, n_dec_rows_max, n_kv_max);
    if (!d_work || work_bytes < need) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_attn_paged_ragged_work_size)", need);
    attn_args a;
    a.kv_type = kv_type; a.D = D; a.n_head = n_head; a.n_head_kv = n_head_kv; a.causal = causal != 0;
    a.q = d_q; a.ldq_tok = ldq_tok; a.ldq_head = ldq_head;
    a.k = d_k; a.v = d_v; a.nb_pos = nb_pos; a.nb_head = nb_head;
    a.n_q = 0; a.n_kv = 0; a.d_n_kv = nullptr; a.n_kv_max = n_kv_max;
    a.scale = scale;
    a.dst = d_dst; a.ldd_tok = ldd_tok; a.ldd_head = ldd_head;
    a.work = (void *)(((uintptr_t)d_work + ATTN_ALIGN - 1) / ATTN_ALIGN * ATTN_ALIGN);
    HIP_TRY(launch_attn_paged_ragged(p, a, rg, pg, add_q != 0, len_bias, on, vo, (hipStream_t)stream, mon ? &bs : nullptr));
    return GGML_HIP_OK;
}

}  // extern "C"
