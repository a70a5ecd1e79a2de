// moe.cpp -- the C-ABI of include/ggml_hip_ext.h, expert-routed products (upstream's ggml_mul_mat_id): the expert set and its two routes.
//
//   route 1  n_tokens <= 4 where the plan of mul_mat(type, M, K, 1) is the fused mat-vec: ONE launch of gemv.hip's by-id kernel, which reads
//            the ids on the device and takes each pair's expert from the set's pointer table (no host synchronize, capturable, the ids
//            may change between replays);
//   route 2  everything else: counting sort of the pairs by expert on the host, gather (moe.hip), ggml_hip_mul_mat_dev per non-empty
//            expert on its contiguous batch, scatter (moe.hip).  The maps travel inside the gather / scatter launches.
// The route is a function of (type, M, K, n_tokens) alone: route_of below is the one place that decides it, for the set's entries and for
// their device-free twins alike.
#include "ctx.h"

#include <algorithm>

using namespace ghip;

struct ggml_hip_expert_set {
    std::vector<const ggml_hip_weight *> w;
    moe_expert *d_tab = nullptr;          // [n_expert] operand plane + side image of every expert (what the by-id mat-vec reads)
    int device = -1;
    int type = 0, ext_type = 0;           // the resident type and the k-quant it was uploaded as (ggml_hip_weight's fields)
    int64_t M = 0, K = 0;
};

namespace {

int device_current(int device) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == device) return GGML_HIP_OK;
    const hipError_t e = hipSetDevice(device);
    return e == hipSuccess ? GGML_HIP_OK : fail(GGML_HIP_ERR_RUNTIME, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
}

int route_of(int type, int ext_type, int64_t M, int64_t K, int64_t n_tokens) {
    return n_tokens <= 4 && plan_mul_mat(type, ext_type, M, K, 1, true).family == MMF_GEMV_FUSED ? 1 : 2;
}

// the batch route's work buffer: [gathered src1 rows P x ldg][sorted results P x ldr][the product's own work buffer], each piece on a
// 256-byte boundary behind a base rounded up to one.  The product's buffer is sized for ALL pairs on one expert (the size grows with N).
constexpr size_t MOE_ALIGN = 256;
size_t align_up(size_t n) { return (n + MOE_ALIGN - 1) / MOE_ALIGN * MOE_ALIGN; }
int64_t ld4(int64_t n) { return (n + 3) / 4 * 4; }
struct moe_work { size_t gathered, results, product, product_bytes, total; };
moe_work work_of(int type, int64_t M, int64_t K, int64_t P) {
    moe_work o;
    o.gathered = 0;
    o.results = o.gathered + align_up((size_t)P * (size_t)ld4(K) * 4);
    o.product = o.results + align_up((size_t)P * (size_t)ld4(M) * 4);
    o.product_bytes = ggml_hip_mul_mat_work_size(type, K, P);
    o.total = o.product + align_up(o.product_bytes) + MOE_ALIGN;
    return o;
}

int check_shape(int64_t n_tokens, int n_used) {
    if (n_tokens < 0 || n_used < 1) return fail(GGML_HIP_ERR_ARG, "n_tokens %lld, n_used %d", (long long)n_tokens, n_used);
    if (n_tokens > (int64_t)(1 << 28) / n_used) return fail(GGML_HIP_ERR_SHAPE, "more than 2^28 (token, slot) pairs");
    return GGML_HIP_OK;
}

// a public type id -> the resident type and ext_type a weight of it carries (what ggml_hip_mm_plan does)
int resolve_type(int type, int64_t M, int64_t K, int *t, int *ext) {
    const bool kq = is_kquant(type);
    *t = kq ? kquant_resident_type(type) : is_iq4nl(type) ? GGML_TYPE_Q8_0 : type;
    *ext = kq ? type : 0;
    if (!is_bf16(*t) && (*t < 0 || *t >= GGML_TYPE_COUNT || !weight_type_ok(*t))) return fail(GGML_HIP_ERR_TYPE, "type %d is not a supported weight type", type);
    if (M <= 0 || K <= 0 || K % ggml_hip_blck_size(*t) != 0 || (is_q(*t) && K % QK != 0) || (kq && K % 256 != 0)) return fail(GGML_HIP_ERR_SHAPE, "bad shape");
    return GGML_HIP_OK;
}

}  // namespace

extern "C" {

int ggml_hip_expert_set_create(const ggml_hip_weight *const *w, int n_expert, void *stream, ggml_hip_expert_set **out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    *out = nullptr;
    if (!w) return fail(GGML_HIP_ERR_ARG, "null weight list");
    if (n_expert < 2 || n_expert > 1024) return fail(GGML_HIP_ERR_ARG, "n_expert %d (2 .. 1024)", n_expert);
    for (int e = 0; e < n_expert; ++e) {
        if (!w[e]) return fail(GGML_HIP_ERR_ARG, "expert %d is null", e);
        if (w[e]->device != w[0]->device) return fail(GGML_HIP_ERR_ARG, "expert %d lives on device %d, expert 0 on device %d", e, w[e]->device, w[0]->device);
        if (w[e]->type != w[0]->type || w[e]->ext_type != w[0]->ext_type || w[e]->up_type != w[0]->up_type)
            return fail(GGML_HIP_ERR_ARG, "expert %d has type %d, expert 0 type %d: one type per set", e, ggml_hip_weight_type(w[e]), ggml_hip_weight_type(w[0]));
        if (w[e]->K != w[0]->K || w[e]->M != w[0]->M || w[e]->Mpad != w[0]->Mpad || w[e]->nbk != w[0]->nbk)
            return fail(GGML_HIP_ERR_SHAPE, "expert %d is %lld x %lld, expert 0 %lld x %lld: one shape per set", e, (long long)w[e]->M, (long long)w[e]->K,
                        (long long)w[0]->M, (long long)w[0]->K);
    }
    if (w[0]->M <= 0) return fail(GGML_HIP_ERR_SHAPE, "the experts have no rows");
    int rc = device_current(w[0]->device);
    if (rc) return rc;
    std::vector<moe_expert> tab((size_t)n_expert);
    const bool i8x2 = w[0]->ext_type != 0 && w[0]->type == GGML_TYPE_Q4_2;      // (the two-scale k-quants: their mat-vec reads the int8 planes)
    for (int e = 0; e < n_expert; ++e) { tab[(size_t)e].qs = i8x2 ? w[e]->i8p : w[e]->qs; tab[(size_t)e].gs = w[e]->gs; }
    ggml_hip_expert_set *s = new ggml_hip_expert_set();
    s->w.assign(w, w + n_expert);
    s->device = w[0]->device; s->type = w[0]->type; s->ext_type = w[0]->ext_type; s->M = w[0]->M; s->K = w[0]->K;
    hipError_t e = hipMalloc((void **)&s->d_tab, tab.size() * sizeof(moe_expert));
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_tab, tab.data(), tab.size() * sizeof(moe_expert), hipMemcpyHostToDevice, (hipStream_t)stream);
    if (e == hipSuccess) e = hipStreamSynchronize((hipStream_t)stream);       // (the host table goes away with this call)
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (s->d_tab) (void)hipFree(s->d_tab);
        delete s;
        return fail(GGML_HIP_ERR_RUNTIME, "expert set table: %s", hipGetErrorString(e));
    }
    *out = s;
    return GGML_HIP_OK;
}

void ggml_hip_expert_set_free(ggml_hip_expert_set *s) {
    if (!s) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != s->device) (void)hipSetDevice(s->device);
    (void)hipFree(s->d_tab);
    if (cur >= 0 && cur != s->device) (void)hipSetDevice(cur);
    delete s;
}

int ggml_hip_mul_mat_id_route_for(int type, int64_t M, int64_t K, int n_expert, int64_t n_tokens, int n_used) {
    (void)n_expert;                                             // (takes no part: the route is the set's shape and the token count)
    int t = 0, ext = 0;
    int rc = resolve_type(type, M, K, &t, &ext);
    if (rc) return rc;
    rc = check_shape(n_tokens, n_used);
    if (rc) return rc;
    return route_of(t, ext, M, K, n_tokens);
}

size_t ggml_hip_mul_mat_id_work_size_for(int type, int64_t M, int64_t K, int n_expert, int64_t n_tokens, int n_used) {
    (void)n_expert;
    int t = 0, ext = 0;
    if (resolve_type(type, M, K, &t, &ext) || check_shape(n_tokens, n_used) || n_tokens == 0) return 0;
    if (route_of(t, ext, M, K, n_tokens) == 1) return 0;
    return work_of(t, M, K, n_tokens * n_used).total;
}

int ggml_hip_mul_mat_id_route(const ggml_hip_expert_set *s, int64_t n_tokens, int n_used) {
    if (!s) return fail(GGML_HIP_ERR_ARG, "null expert set");
    const int rc = check_shape(n_tokens, n_used);
    if (rc) return rc;
    return route_of(s->type, s->ext_type, s->M, s->K, n_tokens);
}

size_t ggml_hip_mul_mat_id_work_size(const ggml_hip_expert_set *s, int64_t n_tokens, int n_used) {
    if (!s || check_shape(n_tokens, n_used) || n_tokens == 0) return 0;
    if (route_of(s->type, s->ext_type, s->M, s->K, n_tokens) == 1) return 0;
    return work_of(s->type, s->M, s->K, n_tokens * n_used).total;
}

int ggml_hip_mul_mat_id_dev(const ggml_hip_expert_set *s, const int32_t *d_ids, const int32_t *h_ids, int64_t n_tokens, int n_used,
                            const float *d_src1, int64_t ld1_token, int64_t ld1_slot, float *d_dst, int64_t ldd, void *d_work, size_t work_bytes,
                            void *stream) {
    if (!s) return fail(GGML_HIP_ERR_ARG, "null expert set");
    int rc = check_shape(n_tokens, n_used);
    if (rc) return rc;
    if (n_tokens == 0) return GGML_HIP_OK;
    if (!d_src1 || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (!d_ids && !h_ids) return fail(GGML_HIP_ERR_ARG, "no ids: d_ids and h_ids are both null");
    const int64_t M = s->M, K = s->K, P = n_tokens * n_used;
    if (ldd < M || ld1_token < 0 || ld1_slot < 0 || (n_tokens > 1 && ld1_token < K) || (ld1_slot != 0 && ld1_slot < K))
        return fail(GGML_HIP_ERR_SHAPE, "ldd < M, or a src1 stride below K (ld1_slot may be 0: one row per token)");
    const int n_expert = (int)s->w.size();
    const int route = route_of(s->type, s->ext_type, M, K, n_tokens);
    hipStream_t st = (hipStream_t)stream;
    if (route == 1) {
        if (!d_ids) return fail(GGML_HIP_ERR_ARG, "the by-id mat-vec reads the ids on the device: d_ids is null");
        if (((uintptr_t)d_src1 & 15) != 0 || ld1_token % 4 != 0 || ld1_slot % 4 != 0)
            return fail(GGML_HIP_ERR_SHAPE, "src1 must be 16-byte aligned with strides that are multiples of 4 elements");
        rc = device_current(s->device);
        if (rc) return rc;
        HIP_TRY(launch_gemv_q_fused_byid(s->w[0], s->d_tab, n_expert, d_ids, P, n_used, d_src1, ld1_token, ld1_slot, d_dst, ldd, st));
        return GGML_HIP_OK;
    }
    const moe_work wk = work_of(s->type, M, K, P);
    if (!d_work || work_bytes < wk.total) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_mul_mat_id_work_size)", wk.total);
    rc = device_current(s->device);
    if (rc) return rc;
    // the ids on the host: the caller's copy, or d_ids read back with one synchronize (never inside a capture)
    std::vector<int32_t> back;
    const int32_t *ids = h_ids;
    if (!ids) {
        hipStreamCaptureStatus cs = hipStreamCaptureStatusNone;
        const hipError_t qe = hipStreamIsCapturing(st, &cs);
        if (qe != hipSuccess) (void)hipGetLastError();
        if (qe != hipSuccess || cs != hipStreamCaptureStatusNone)
            return fail(GGML_HIP_ERR_ARG, "the batch route needs the ids on the host and the stream is capturing: pass h_ids (reading d_ids back would synchronize)");
        back.resize((size_t)P);
        HIP_TRY(hipMemcpyAsync(back.data(), d_ids, (size_t)P * 4, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        ids = back.data();
    }
    // counting sort by expert, ascending p inside an expert; pos[p] = the sorted row of pair p, -1 for an id outside the set
    std::vector<int64_t> first((size_t)n_expert + 1, 0);
    for (int64_t p = 0; p < P; ++p) {
        const int32_t id = ids[p];
        if (id < 0 || id >= n_expert) {
            if (h_ids) return fail(GGML_HIP_ERR_ARG, "ids[%lld] = %d is outside [0, %d)", (long long)p, id, n_expert);
            continue;
        }
        ++first[(size_t)id + 1];
    }
    for (int e = 0; e < n_expert; ++e) first[(size_t)e + 1] += first[(size_t)e];
    const int64_t n_valid = first[(size_t)n_expert];
    std::vector<int32_t> order((size_t)n_valid), pos((size_t)P, -1);
    {
        std::vector<int64_t> next(first.begin(), first.end() - 1);
        for (int64_t p = 0; p < P; ++p) {
            const int32_t id = ids[p];
            if (id < 0 || id >= n_expert) continue;
            const int64_t j = next[(size_t)id]++;
            order[(size_t)j] = (int32_t)p; pos[(size_t)p] = (int32_t)j;
        }
    }
    uint8_t *base = (uint8_t *)(((uintptr_t)d_work + MOE_ALIGN - 1) / MOE_ALIGN * MOE_ALIGN);
    float *g = (float *)(base + wk.gathered), *r = (float *)(base + wk.results);
    void *pw = base + wk.product;
    const int64_t ldg = ld4(K), ldr = ld4(M);
    moe_map map;
    for (int64_t j0 = 0; j0 < n_valid; j0 += MOE_MAP_CHUNK) {
        const int n = (int)std::min<int64_t>(MOE_MAP_CHUNK, n_valid - j0);
        memcpy(map.v, order.data() + j0, (size_t)n * 4);
        HIP_TRY(launch_moe_gather(map, n, j0, n_used, d_src1, ld1_token, ld1_slot, K, g, ldg, st));
    }
    for (int e = 0; e < n_expert; ++e) {
        const int64_t j0 = first[(size_t)e], cnt = first[(size_t)e + 1] - j0;
        if (cnt <= 0) continue;
        rc = ggml_hip_mul_mat_dev(s->w[(size_t)e], g + j0 * ldg, cnt, ldg, r + j0 * ldr, ldr, pw, align_up(wk.product_bytes), stream);
        if (rc) return rc;
    }
    for (int64_t p0 = 0; p0 < P; p0 += MOE_MAP_CHUNK) {
        const int n = (int)std::min<int64_t>(MOE_MAP_CHUNK, P - p0);
        memcpy(map.v, pos.data() + p0, (size_t)n * 4);
        HIP_TRY(launch_moe_scatter(map, n, p0, r, ldr, M, d_dst, ldd, st));
    }
    return GGML_HIP_OK;
}

}  // extern "C"
