// ssm.cpp -- the C-ABI of include/ggml_hip_ext.h, SSM: the causal conv (ggml_hip_ssm_conv_ragged_dev; ggml_hip_ssm_conv_tiled_ragged_dev with the
// token-parallel tiled form for long sequences) and the selective scan (ggml_hip_ssm_scan_ragged_dev; ggml_hip_ssm_scan_chunked_ragged_dev with the
// chunked matrix form for long sequences) of a Mamba / Mamba-2 block over a ragged batch and a pool of state slots, their slot sizes and their plans
// (host only).  The kernels are ssm.hip's, ssm_chunk.hip's and ssm_conv_tile.hip's, every grid is plan.cpp's.  No set, no handle: stream-ordered launches on the current device, no synchronize, no
// allocation; capturable.  Every refusal is decided here, before a device is touched.
#include "ctx.h"

using namespace ghip;

namespace {

constexpr size_t SSM_WORK_ALIGN = 256;                             // the chunked scan and the tiled conv round their work buffer's base up to it

// the batch and the state cache both entries share: n_seq, d_q_start, n_tokens_max (check_kv_ragged), d_len, d_slot, the pool; 0 or an error code
int check_ssm_batch(int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot, const float *d_state,
                    int64_t nb_slot, int64_t n_slots, size_t slot_bytes, kv_ragged *rg) {
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    const int rc = check_kv_ragged(d_q_start, n_seq, n_tokens_max, rg);
    if (rc) return rc;
    if (!d_len || !d_slot) return fail(GGML_HIP_ERR_ARG, "d_len and d_slot must not be null");
    if ((((uintptr_t)d_len | (uintptr_t)d_slot) & 3) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_len and d_slot must be 4-byte aligned");
    if (n_slots < 1 || n_slots > 0x7FFFFFFF) return fail(GGML_HIP_ERR_ARG, "n_slots %lld (1 .. 2^31 - 1)", (long long)n_slots);
    if (nb_slot % 16 != 0 || nb_slot < (int64_t)slot_bytes || nb_slot > ((int64_t)1 << 40))
        return fail(GGML_HIP_ERR_SHAPE, "nb_slot %lld: a multiple of 16 bytes, at least the %lld bytes of a slot", (long long)nb_slot, (long long)slot_bytes);
    if (n_slots > (((int64_t)1 << 48) / nb_slot)) return fail(GGML_HIP_ERR_SHAPE, "the pool, n_slots %lld * nb_slot %lld, is beyond 2^48 bytes", (long long)n_slots, (long long)nb_slot);
    if (!d_state) return fail(GGML_HIP_ERR_ARG, "d_state must not be null");
    if (((uintptr_t)d_state & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "d_state must be 16-byte aligned");
    return GGML_HIP_OK;
}

// every check both scan entries share, in the order the header states them; fills the plan, the batch and the kernels' arguments
int check_ssm_scan(const float *d_x, int64_t ldx_tok, int64_t ldx_head, const float *d_dt, int64_t ld_dt, const float *d_dt_bias, const float *d_A, int64_t a_ld,
                   int a_per_state, const float *d_B, const float *d_C, int64_t ld_bc, const float *d_D, int n_head, int head_dim, int d_state_n, int n_group,
                   int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot, float *d_state, int64_t nb_slot,
                   int64_t n_slots, float *d_dst, int64_t ldd_tok, int64_t ldd_head, ssm_scan_plan *plan, kv_ragged *batch, ssm_scan_args *args) {
    const int P = head_dim, N = d_state_n;
    if (n_head < 1 || n_head > SSM_MAX_HEADS) return fail(GGML_HIP_ERR_SHAPE, "n_head %d (1 .. 2^20)", n_head);
    if (P < 1 || P > 256) return fail(GGML_HIP_ERR_SHAPE, "head_dim %d (1 .. 256)", P);
    if (N < 16 || N > 256 || N % 16 != 0) return fail(GGML_HIP_ERR_SHAPE, "d_state %d: a multiple of 16, at most 256", N);
    if (n_group < 1 || n_head % n_group != 0) return fail(GGML_HIP_ERR_SHAPE, "n_group %d must divide n_head %d", n_group, n_head);
    if (a_per_state != 0 && a_per_state != 1) return fail(GGML_HIP_ERR_ARG, "a_per_state %d: 0 or 1", a_per_state);
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    const ssm_scan_plan pl = plan_ssm_scan(n_head, P, N, n_group, n_seq);
    if (!pl.ok) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    kv_ragged &rg = *batch;
    const int rc = check_ssm_batch(n_seq, d_q_start, n_tokens_max, d_len, d_slot, d_state, nb_slot, n_slots, pl.state_bytes, &rg);
    if (rc) return rc;
    const int64_t big = (int64_t)1 << 32;
    if (ldx_head < P || ldd_head < P || ldx_tok < 0 || ldd_tok < 0 || (n_tokens_max > 1 && (ldx_tok < P || ldd_tok < P)) || ldx_head > big || ldd_head > big ||
        ldx_tok > big || ldd_tok > big)
        return fail(GGML_HIP_ERR_SHAPE, "the strides of x and dst are at least head_dim %d", P);
    if (ld_dt < n_head || ld_dt > big) return fail(GGML_HIP_ERR_SHAPE, "ld_dt %lld below n_head %d", (long long)ld_dt, n_head);
    if (a_ld < (a_per_state ? N : 1) || a_ld > big || (a_per_state && a_ld % 4 != 0))
        return fail(GGML_HIP_ERR_SHAPE, "a_ld %lld: at least %d%s", (long long)a_ld, a_per_state ? N : 1, a_per_state ? ", a multiple of 4" : "");
    if (ld_bc < (int64_t)n_group * N || ld_bc % 4 != 0 || ld_bc > big)
        return fail(GGML_HIP_ERR_SHAPE, "ld_bc %lld: a multiple of 4, at least n_group * d_state = %lld", (long long)ld_bc, (long long)n_group * N);
    if (!d_x || !d_dt || !d_A || !d_B || !d_C || !d_dst) return fail(GGML_HIP_ERR_ARG, "d_x, d_dt, d_A, d_B, d_C and d_dst must not be null");
    if ((((uintptr_t)d_B | (uintptr_t)d_C) & 15) != 0 || (a_per_state && ((uintptr_t)d_A & 15) != 0))
        return fail(GGML_HIP_ERR_SHAPE, "d_B, d_C and a per-state d_A must be 16-byte aligned");
    if ((((uintptr_t)d_x | (uintptr_t)d_dt | (uintptr_t)d_dt_bias | (uintptr_t)d_A | (uintptr_t)d_D | (uintptr_t)d_dst) & 3) != 0)
        return fail(GGML_HIP_ERR_SHAPE, "d_x, d_dt, d_dt_bias, d_A, d_D and d_dst must be 4-byte aligned");
    ssm_scan_args &a = *args;
    a.x = d_x; a.ldx_tok = ldx_tok; a.ldx_head = ldx_head; a.dt = d_dt; a.ld_dt = ld_dt; a.dt_bias = d_dt_bias; a.A = d_A; a.a_ld = a_ld; a.a_per_state = a_per_state;
    a.B = d_B; a.C = d_C; a.ld_bc = ld_bc; a.D = d_D; a.n_head = n_head; a.P = P; a.N = N; a.n_group = n_group;
    a.len = d_len; a.slot = d_slot; a.n_slots = (int)n_slots; a.state = d_state; a.slot_elems = nb_slot / 4; a.dst = d_dst; a.ldd_tok = ldd_tok; a.ldd_head = ldd_head;
    a.nq_max = 0x7FFFFFFF;
    *plan = pl;
    return GGML_HIP_OK;
}

// every check both conv entries share, in the order the header states them; fills the sequential plan and the batch
int check_ssm_conv(const float *d_x, int64_t ldx, const float *d_w, const float *d_bias, int act, int64_t n_ch, int d_conv, int64_t n_seq,
                   const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot, const float *d_state, int64_t nb_slot,
                   int64_t n_slots, const float *d_dst, int64_t ldd, ssm_conv_plan *plan, kv_ragged *rg) {
    if (n_ch < 1 || n_ch > SSM_MAX_CHANNELS) return fail(GGML_HIP_ERR_SHAPE, "n_ch %lld (1 .. 2^24)", (long long)n_ch);
    if (d_conv < 2 || d_conv > 4) return fail(GGML_HIP_ERR_SHAPE, "d_conv %d (2 .. 4)", d_conv);
    if (act != 0 && act != 1) return fail(GGML_HIP_ERR_ARG, "act %d: 0 (none) or 1 (silu)", act);
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return fail(GGML_HIP_ERR_SHAPE, "n_seq %lld (1 .. %lld)", (long long)n_seq, (long long)ATTN_PAGED_MAX_SEQ);
    *plan = plan_ssm_conv(n_ch, d_conv, n_seq);
    const int rc = check_ssm_batch(n_seq, d_q_start, n_tokens_max, d_len, d_slot, d_state, nb_slot, n_slots, plan->state_bytes, rg);
    if (rc) return rc;
    if (ldx < n_ch || ldd < n_ch || ldx > ((int64_t)1 << 32) || ldd > ((int64_t)1 << 32))
        return fail(GGML_HIP_ERR_SHAPE, "ldx %lld and ldd %lld must be at least n_ch %lld", (long long)ldx, (long long)ldd, (long long)n_ch);
    if (!d_x || !d_w || !d_dst) return fail(GGML_HIP_ERR_ARG, "d_x, d_w and d_dst must not be null");
    if ((((uintptr_t)d_x | (uintptr_t)d_w | (uintptr_t)d_bias | (uintptr_t)d_dst) & 3) != 0)
        return fail(GGML_HIP_ERR_SHAPE, "d_x, d_w, d_bias and d_dst must be 4-byte aligned");
    return GGML_HIP_OK;
}

}  // namespace

extern "C" {

size_t ggml_hip_ssm_conv_state_bytes(int64_t n_ch, int d_conv) { return plan_ssm_conv(n_ch, d_conv, 1).state_bytes; }

size_t ggml_hip_ssm_state_bytes(int n_head, int head_dim, int d_state) { return plan_ssm_scan(n_head, head_dim, d_state, 1, 1).state_bytes; }

int ggml_hip_ssm_scan_plan(int n_head, int head_dim, int d_state, int n_group, int64_t n_seq, ggml_hip_ssm_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "null argument");
    const ssm_scan_plan p = plan_ssm_scan(n_head, head_dim, d_state, n_group, n_seq);
    if (!p.ok) return fail(GGML_HIP_ERR_SHAPE, "ssm scan: n_head %d, head_dim %d, d_state %d, n_group %d, n_seq %lld", n_head, head_dim, d_state, n_group, (long long)n_seq);
    out->form = p.form; out->launches = p.launches; out->slices = p.slices; out->lanes_per_row = p.lanes_per_row;
    out->rows_per_workgroup = p.rows_per_wg; out->workgroups = p.wgs;
    return GGML_HIP_OK;
}

int ggml_hip_ssm_conv_ragged_dev(const float *d_x, int64_t ldx, const float *d_w, const float *d_bias, int act, int64_t n_ch, int d_conv, int64_t n_seq,
                                 const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot, float *d_state, int64_t nb_slot,
                                 int64_t n_slots, float *d_dst, int64_t ldd, void *stream) {
    ssm_conv_plan pl; kv_ragged rg;
    const int rc = check_ssm_conv(d_x, ldx, d_w, d_bias, act, n_ch, d_conv, n_seq, d_q_start, n_tokens_max, d_len, d_slot, d_state, nb_slot, n_slots, d_dst, ldd,
                                  &pl, &rg);
    if (rc) return rc;
    if (n_tokens_max == 0) return GGML_HIP_OK;
    HIP_TRY(launch_ssm_conv(pl, rg, d_len, d_slot, (int)n_slots, d_x, ldx, d_w, d_bias, act, n_ch, d_conv, d_state, nb_slot / 4, d_dst, ldd, 0x7FFFFFFF,
                            (hipStream_t)stream));
    return GGML_HIP_OK;
}

size_t ggml_hip_ssm_conv_tiled_work_size(int64_t n_ch, int d_conv, int64_t n_seq, int64_t n_tokens_max) {
    const ssm_conv_tiled_plan p = plan_ssm_conv_tiled(n_ch, d_conv, n_seq, n_tokens_max);
    if (!p.ok || p.work_bytes == 0) return 0;
    return p.work_bytes + SSM_WORK_ALIGN;                                // (the base is rounded up to a 256-byte boundary)
}

int ggml_hip_ssm_conv_tiled_plan(int64_t n_ch, int d_conv, int64_t n_seq, int64_t n_tokens_max, ggml_hip_ssm_conv_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "null argument");
    const ssm_conv_tiled_plan p = plan_ssm_conv_tiled(n_ch, d_conv, n_seq, n_tokens_max);
    if (!p.ok)
        return fail(GGML_HIP_ERR_SHAPE, "ssm tiled conv: n_ch %lld, d_conv %d, n_seq %lld, n_tokens_max %lld", (long long)n_ch, d_conv, (long long)n_seq,
                    (long long)n_tokens_max);
    out->form = p.form; out->tile = p.tile; out->seq_max_tokens = p.seq_max_tokens; out->launches = p.launches; out->vec = p.vec; out->reserved = 0;
    out->tiles_max = p.tiles_max; out->seqs_max = p.seqs_max;
    out->work_bytes = ggml_hip_ssm_conv_tiled_work_size(n_ch, d_conv, n_seq, n_tokens_max);
    return GGML_HIP_OK;
}

int ggml_hip_ssm_conv_tiled_ragged_dev(const float *d_x, int64_t ldx, const float *d_w, const float *d_bias, int act, int64_t n_ch, int d_conv, int64_t n_seq,
                                       const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot, float *d_state,
                                       int64_t nb_slot, int64_t n_slots, float *d_dst, int64_t ldd, void *d_work, size_t work_bytes, void *stream) {
    ssm_conv_plan seq; kv_ragged rg;
    const int rc = check_ssm_conv(d_x, ldx, d_w, d_bias, act, n_ch, d_conv, n_seq, d_q_start, n_tokens_max, d_len, d_slot, d_state, nb_slot, n_slots, d_dst, ldd,
                                  &seq, &rg);
    if (rc) return rc;
    const ssm_conv_tiled_plan pl = plan_ssm_conv_tiled(n_ch, d_conv, n_seq, n_tokens_max);
    if (!pl.ok) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    const size_t need = ggml_hip_ssm_conv_tiled_work_size(n_ch, d_conv, n_seq, n_tokens_max);
    if (need && (!d_work || work_bytes < need)) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_ssm_conv_tiled_work_size)", need);
    if (n_tokens_max == 0) return GGML_HIP_OK;
    void *work = need ? (void *)(((uintptr_t)d_work + SSM_WORK_ALIGN - 1) / SSM_WORK_ALIGN * SSM_WORK_ALIGN) : nullptr;
    HIP_TRY(launch_ssm_conv_tiled(pl, rg, d_len, d_slot, (int)n_slots, d_x, ldx, d_w, d_bias, act, n_ch, d_conv, d_state, nb_slot / 4, d_dst, ldd, work,
                                  (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_ssm_scan_ragged_dev(const float *d_x, int64_t ldx_tok, int64_t ldx_head, const float *d_dt, int64_t ld_dt, const float *d_dt_bias, const float *d_A,
                                 int64_t a_ld, int a_per_state, const float *d_B, const float *d_C, int64_t ld_bc, const float *d_D, int n_head, int head_dim,
                                 int d_state_n, int n_group, int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len,
                                 const int32_t *d_slot, float *d_state, int64_t nb_slot, int64_t n_slots, float *d_dst, int64_t ldd_tok, int64_t ldd_head,
                                 void *stream) {
    ssm_scan_plan pl; kv_ragged rg; ssm_scan_args a;
    const int rc = check_ssm_scan(d_x, ldx_tok, ldx_head, d_dt, ld_dt, d_dt_bias, d_A, a_ld, a_per_state, d_B, d_C, ld_bc, d_D, n_head, head_dim, d_state_n, n_group,
                                  n_seq, d_q_start, n_tokens_max, d_len, d_slot, d_state, nb_slot, n_slots, d_dst, ldd_tok, ldd_head, &pl, &rg, &a);
    if (rc) return rc;
    if (n_tokens_max == 0) return GGML_HIP_OK;
    HIP_TRY(launch_ssm_scan(pl, rg, a, (hipStream_t)stream));
    return GGML_HIP_OK;
}

size_t ggml_hip_ssm_scan_chunked_work_size(int n_head, int head_dim, int d_state, int n_group, int a_per_state, int64_t n_seq, int64_t n_tokens_max) {
    const ssm_chunk_plan p = plan_ssm_chunk(n_head, head_dim, d_state, n_group, a_per_state, n_seq, n_tokens_max);
    if (!p.ok || p.work_bytes == 0) return 0;
    return p.work_bytes + SSM_WORK_ALIGN;                                // (the base is rounded up to a 256-byte boundary)
}

int ggml_hip_ssm_scan_chunked_plan(int n_head, int head_dim, int d_state, int n_group, int a_per_state, int64_t n_seq, int64_t n_tokens_max,
                                   ggml_hip_ssm_chunk_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "null argument");
    const ssm_chunk_plan p = plan_ssm_chunk(n_head, head_dim, d_state, n_group, a_per_state, n_seq, n_tokens_max);
    if (!p.ok)
        return fail(GGML_HIP_ERR_SHAPE, "ssm chunked scan: n_head %d, head_dim %d, d_state %d, n_group %d, a_per_state %d, n_seq %lld, n_tokens_max %lld", n_head,
                    head_dim, d_state, n_group, a_per_state, (long long)n_seq, (long long)n_tokens_max);
    out->form = p.form; out->chunk = p.chunk; out->seq_max_tokens = p.seq_max_tokens; out->launches = p.launches; out->p_tile = p.p_tile; out->p_tiles = p.p_tiles;
    out->kernel_state = p.kernel_state; out->kernel_out = p.kernel_out; out->chunks_max = p.chunks_max; out->seqs_max = p.seqs_max;
    out->work_bytes = ggml_hip_ssm_scan_chunked_work_size(n_head, head_dim, d_state, n_group, a_per_state, n_seq, n_tokens_max);
    return GGML_HIP_OK;
}

int ggml_hip_ssm_scan_chunked_ragged_dev(const float *d_x, int64_t ldx_tok, int64_t ldx_head, const float *d_dt, int64_t ld_dt, const float *d_dt_bias,
                                         const float *d_A, int64_t a_ld, int a_per_state, const float *d_B, const float *d_C, int64_t ld_bc, const float *d_D,
                                         int n_head, int head_dim, int d_state_n, int n_group, int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max,
                                         const int32_t *d_len, const int32_t *d_slot, float *d_state, int64_t nb_slot, int64_t n_slots, float *d_dst,
                                         int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream) {
    ssm_scan_plan seq; kv_ragged rg; ssm_scan_args a;
    const int rc = check_ssm_scan(d_x, ldx_tok, ldx_head, d_dt, ld_dt, d_dt_bias, d_A, a_ld, a_per_state, d_B, d_C, ld_bc, d_D, n_head, head_dim, d_state_n, n_group,
                                  n_seq, d_q_start, n_tokens_max, d_len, d_slot, d_state, nb_slot, n_slots, d_dst, ldd_tok, ldd_head, &seq, &rg, &a);
    if (rc) return rc;
    const ssm_chunk_plan pl = plan_ssm_chunk(n_head, head_dim, d_state_n, n_group, a_per_state, n_seq, n_tokens_max);
    if (!pl.ok) return fail(GGML_HIP_ERR_SHAPE, "the shape is not served");
    const size_t need = ggml_hip_ssm_scan_chunked_work_size(n_head, head_dim, d_state_n, n_group, a_per_state, n_seq, n_tokens_max);
    if (need && (!d_work || work_bytes < need)) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_ssm_scan_chunked_work_size)", need);
    if (n_tokens_max == 0) return GGML_HIP_OK;
    void *work = need ? (void *)(((uintptr_t)d_work + SSM_WORK_ALIGN - 1) / SSM_WORK_ALIGN * SSM_WORK_ALIGN) : nullptr;
    HIP_TRY(launch_ssm_scan_chunked(pl, rg, a, work, (hipStream_t)stream));
    return GGML_HIP_OK;
}

}  // extern "C"
