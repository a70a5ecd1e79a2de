// moe.cpp -- the C-ABI of include/ggml_hip_ext.h, expert-routed products (upstream's ggml_mul_mat_id): the expert set and its two routes.
//
//   route 1  n_tokens <= 4 where the plan of mul_mat(type, M, K, 1) is the fused mat-vec: ONE launch of gemv.hip's by-id kernel, which reads
//            the ids on the device and takes each pair's expert from the set's pointer table (no host synchronize, capturable, the ids
//            may change between replays);
//   route 2  everything else: counting sort of the pairs by expert on the host, gather (moe.hip), ggml_hip_mul_mat_dev per non-empty
//            expert on its contiguous batch, scatter (moe.hip).  The maps travel inside the gather / scatter launches.
// The route is a function of (type, M, K, n_tokens) alone: route_of below is the one place that decides it, for the set's entries and for
// their device-free twins alike.
//
// Beside them, reached through its own entry only (ggml_hip_mul_mat_id_grouped_dev), the GROUPED route: the ids are read on the device alone --
// routing kernels (moe.hip) sort the pairs by expert into segments padded to 32-row column tiles, a gather and ONE INIT over the bounded row
// count write the activation image, ONE K3s launch (gemm_q8s.hip / gemm_qmx.hip) runs every tile against its expert's planes, a scatter takes
// the sorted results to their pairs.  Seven launches whatever the routing and n_expert; no synchronize, no allocation; capturable.  What it
// serves, its geometry and its bounds are plan.cpp's (plan_mul_mat_id_grouped).
#include "ctx.h"

#include <algorithm>

using namespace ghip;

struct ggml_hip_expert_set {
    std::vector<const ggml_hip_weight *> w;
    moe_expert *d_tab = nullptr;          // [n_expert] operand plane + side image of every expert (what the by-id mat-vec reads)
    moe_gexpert *d_gtab = nullptr;        // [n_expert] behind it in the same allocation: operand planes + block scales as the K3s bodies take them (the grouped route)
    bool grouped_planes = false;          // every expert has the planes the grouped route's kernel of this type reads
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
    const wtype *r = wtype_of(type);
    if (!r || !r->to_planar) return fail(GGML_HIP_ERR_TYPE, "type %d is not a supported weight type", type);
    *t = r->resident;
    *ext = wtype_ext(r);
    if (M <= 0 || K <= 0 || K % k_unit(r) != 0) return fail(GGML_HIP_ERR_SHAPE, "bad shape");
    return GGML_HIP_OK;
}

// ---- the grouped route ----
// its work buffer, each piece on a 256-byte boundary behind a base rounded up to one: the routing tables (count, first [n_expert]; n_tiles; pos [P];
// order [rows]; tiles [max_tiles]), the gathered src1 rows and the sorted results ([rows] each), the activation image of `rows` rows.
// rows = 32 * max_tiles, the bound of plan.h -- it grows with min(n_expert, P).
struct grouped_work { size_t count, first, n_tiles, pos, order, tiles, gathered, results, image, image_bytes, total; int64_t max_tiles, rows; };
grouped_work grouped_work_of(int64_t M, int64_t K, int n_expert, int64_t P) {
    grouped_work o;
    o.max_tiles = moe_grouped_tiles(n_expert, P); o.rows = 32 * o.max_tiles;
    o.count = 0;
    o.first = o.count + align_up((size_t)n_expert * 4);
    o.n_tiles = o.first + align_up((size_t)n_expert * 4);
    o.pos = o.n_tiles + MOE_ALIGN;
    o.order = o.pos + align_up((size_t)P * 4);
    o.tiles = o.order + align_up((size_t)o.rows * 4);
    o.gathered = o.tiles + align_up((size_t)o.max_tiles * sizeof(moe_tile));
    o.results = o.gathered + align_up((size_t)o.rows * (size_t)ld4(K) * 4);
    o.image = o.results + align_up((size_t)o.rows * (size_t)ld4(M) * 4);
    o.image_bytes = act_bytes(K, pad_act(o.rows));
    o.total = o.image + align_up(o.image_bytes) + MOE_ALIGN;
    return o;
}

int grouped_check_shape(int64_t n_tokens, int n_used) {
    if (n_tokens < 0 || n_used < 1) return fail(GGML_HIP_ERR_ARG, "n_tokens %lld, n_used %d", (long long)n_tokens, n_used);
    if (n_tokens > MOE_GROUPED_MAX_PAIRS / n_used) return fail(GGML_HIP_ERR_SHAPE, "more than 2^20 (token, slot) pairs");
    return GGML_HIP_OK;
}

size_t grouped_work_size(int type, int ext_type, int64_t M, int64_t K, int n_expert, int64_t n_tokens, int n_used) {
    if (n_tokens <= 0 || n_used < 1 || n_tokens > MOE_GROUPED_MAX_PAIRS / n_used || n_expert < 1 || n_expert > 1024) return 0;
    if (plan_mul_mat_id_grouped(type, ext_type, M, K, n_expert, n_tokens * n_used).family == MMF_NONE) return 0;
    return grouped_work_of(M, K, n_expert, n_tokens * n_used).total;
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
    // one table for each kernel that picks an expert on the device, in one allocation: [n_expert] moe_expert, then [n_expert] moe_gexpert
    static_assert(sizeof(moe_expert) == 16 && sizeof(moe_gexpert) == 32, "the second table starts on a 32-byte boundary");
    const size_t tab_bytes = (size_t)n_expert * sizeof(moe_expert), all_bytes = tab_bytes + (size_t)n_expert * sizeof(moe_gexpert);
    std::vector<uint8_t> host(all_bytes);
    moe_expert *tab = (moe_expert *)host.data();
    moe_gexpert *gtab = (moe_gexpert *)(host.data() + tab_bytes);
    const bool i8x2 = w[0]->ext_type != 0 && w[0]->type == GGML_TYPE_Q4_2;      // (the two-scale k-quants: their mat-vec reads the int8 planes)
    const int ty = w[0]->type;
    bool planes = true;
    for (int e = 0; e < n_expert; ++e) {
        tab[e].qs = i8x2 ? w[e]->i8p : w[e]->qs; tab[e].gs = w[e]->gs;
        gtab[e] = ty == GGML_TYPE_Q4_0 ? moe_gexpert{w[e]->q6a, w[e]->q6b, w[e]->d, nullptr}
                                       : moe_gexpert{ty == GGML_TYPE_Q5_0 ? w[e]->i8p : w[e]->qs, nullptr, w[e]->d, nullptr};
        planes = planes && gtab[e].a && gtab[e].d && (ty != GGML_TYPE_Q4_0 || gtab[e].b);
    }
    ggml_hip_expert_set *s = new ggml_hip_expert_set();
    s->w.assign(w, w + n_expert);
    s->device = w[0]->device; s->type = w[0]->type; s->ext_type = w[0]->ext_type; s->M = w[0]->M; s->K = w[0]->K;
    s->grouped_planes = planes;
    hipError_t e = hipMalloc((void **)&s->d_tab, all_bytes);
    if (e == hipSuccess) s->d_gtab = (moe_gexpert *)((uint8_t *)s->d_tab + tab_bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(s->d_tab, host.data(), all_bytes, hipMemcpyHostToDevice, (hipStream_t)stream);
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

int ggml_hip_mul_mat_id_grouped_serves_for(int type, int64_t M, int64_t K) {
    const wtype *r = wtype_of(type);                       // (IQ4_NL: a plain Q8_0 weight; a k-quant: never served)
    if (M <= 0 || K <= 0 || K % QK != 0 || (r && K % r->blck != 0)) return 0;
    return plan_mul_mat_id_grouped_serves(r ? r->resident : type, r ? wtype_ext(r) : 0, M, K) ? 1 : 0;
}

int ggml_hip_mul_mat_id_grouped_serves(const ggml_hip_expert_set *s) {
    if (!s) return fail(GGML_HIP_ERR_ARG, "null expert set");
    return plan_mul_mat_id_grouped_serves(s->type, s->ext_type, s->M, s->K) ? 1 : 0;
}

size_t ggml_hip_mul_mat_id_grouped_work_size_for(int type, int64_t M, int64_t K, int n_expert, int64_t n_tokens, int n_used) {
    const wtype *r = wtype_of(type);
    if (M <= 0 || K <= 0 || K % QK != 0 || (r && K % r->blck != 0)) return 0;
    return grouped_work_size(r ? r->resident : type, r ? wtype_ext(r) : 0, M, K, n_expert, n_tokens, n_used);
}

size_t ggml_hip_mul_mat_id_grouped_work_size(const ggml_hip_expert_set *s, int64_t n_tokens, int n_used) {
    if (!s) return 0;
    return grouped_work_size(s->type, s->ext_type, s->M, s->K, (int)s->w.size(), n_tokens, n_used);
}

int ggml_hip_mul_mat_id_grouped_dev(const ggml_hip_expert_set *s, const int32_t *d_ids, int64_t n_tokens, int n_used, const float *d_src1, int64_t ld1_token,
                                    int64_t ld1_slot, float *d_dst, int64_t ldd, void *d_work, size_t work_bytes, void *stream) {
    if (!s) return fail(GGML_HIP_ERR_ARG, "null expert set");
    int rc = grouped_check_shape(n_tokens, n_used);
    if (rc) return rc;
    if (n_tokens == 0) return GGML_HIP_OK;
    const int64_t M = s->M, K = s->K, P = n_tokens * n_used;
    const int n_expert = (int)s->w.size();
    if (s->ext_type != 0 || !(s->type == GGML_TYPE_Q8_0 || s->type == GGML_TYPE_Q5_0 || s->type == GGML_TYPE_Q4_0))
        return fail(GGML_HIP_ERR_TYPE, "the grouped route serves Q8_0, Q5_0, IQ4_NL and Q4_0 sets (ggml_hip_mul_mat_id_grouped_serves); this set's type is %d",
                    ggml_hip_weight_type(s->w[0]));
    const mm_plan g = plan_mul_mat_id_grouped(s->type, s->ext_type, M, K, n_expert, P);
    if (g.family == MMF_NONE)
        return fail(GGML_HIP_ERR_SHAPE, "the grouped route does not serve %lld x %lld with %lld pairs (K / 32 in 32 .. 1024 where the plan at 32 rows is K3s)",
                    (long long)M, (long long)K, (long long)P);
    if (!d_ids || !d_src1 || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument (the ids are read on the device: d_ids)");
    if (ldd < M || ld1_token < 0 || ld1_slot < 0 || (n_tokens > 1 && ld1_token < K) || (ld1_slot != 0 && ld1_slot < K))
        return fail(GGML_HIP_ERR_SHAPE, "ldd < M, or a src1 stride below K (ld1_slot may be 0: one row per token)");
    if (((uintptr_t)d_src1 & 15) != 0 || ld1_token % 4 != 0 || ld1_slot % 4 != 0)
        return fail(GGML_HIP_ERR_SHAPE, "src1 must be 16-byte aligned with strides that are multiples of 4 elements");
    const grouped_work wk = grouped_work_of(M, K, n_expert, P);
    if (!d_work || work_bytes < wk.total) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu (ggml_hip_mul_mat_id_grouped_work_size)", wk.total);
    if (!s->grouped_planes) return fail(GGML_HIP_ERR_RUNTIME, "an expert of the set has no operand planes for the grouped kernel");
    rc = device_current(s->device);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    uint8_t *base = (uint8_t *)(((uintptr_t)d_work + MOE_ALIGN - 1) / MOE_ALIGN * MOE_ALIGN);
    const moe_route rt = {(int32_t *)(base + wk.count), (int32_t *)(base + wk.first), (int32_t *)(base + wk.n_tiles), (int32_t *)(base + wk.pos),
                          (int32_t *)(base + wk.order), (moe_tile *)(base + wk.tiles)};
    float *gth = (float *)(base + wk.gathered), *res = (float *)(base + wk.results);
    const int64_t ldg = ld4(K), ldr = ld4(M);
    const act_planes pl = act_carve(base + wk.image, K, pad_act(wk.rows));
    HIP_TRY(launch_moe_route(d_ids, P, n_expert, rt, wk.max_tiles, st));
    HIP_TRY(launch_moe_gather_dev(rt.order, wk.rows, n_used, d_src1, ld1_token, ld1_slot, K, gth, ldg, st));
    HIP_TRY(launch_quantize_act(gth, wk.rows, K, ldg, pl, g.image, st, false));     // (the image ggml_hip_mul_mat_init_dev writes for N = rows)
    const ggml_hip_weight *w0 = s->w[0];
    if (g.family == MMF_K3S_MX) HIP_TRY(launch_gemm_qmx_small_grouped(g, s->type, s->d_gtab, rt.tiles, rt.n_tiles, wk.max_tiles, M, w0->Mpad, w0->nbk, pl, res, ldr, st));
    else HIP_TRY(launch_gemm_q8_small_grouped(g, s->type, s->d_gtab, rt.tiles, rt.n_tiles, wk.max_tiles, M, w0->Mpad, w0->nbk, pl, res, ldr, st));
    HIP_TRY(launch_moe_scatter_dev(rt.pos, P, res, ldr, M, d_dst, ldd, st));
    return GGML_HIP_OK;
}

// ---- the router and the combine around the products (moe_route.hip), and the SwiGLU pair between them on device rows ----
// no set, no work buffer, nothing but launches on `stream`: they run on the current device like ggml_hip_rms_norm_mul_rows_dev

int ggml_hip_moe_route_dev(const float *d_logits, int64_t ld_logits, int64_t n_tokens, int n_expert, int n_used, int gating, int normalize, float scale,
                           int32_t *d_ids, float *d_weights, void *stream) {
    if (n_tokens < 0) return fail(GGML_HIP_ERR_ARG, "n_tokens %lld", (long long)n_tokens);
    if (n_expert < 1 || n_expert > 1024) return fail(GGML_HIP_ERR_SHAPE, "n_expert %d (1 .. 1024)", n_expert);
    if (n_used < 1 || n_used > 64 || n_used > n_expert) return fail(GGML_HIP_ERR_SHAPE, "n_used %d (1 .. min(n_expert, 64))", n_used);
    if (n_tokens > MOE_GROUPED_MAX_PAIRS / n_used) return fail(GGML_HIP_ERR_SHAPE, "more than 2^20 (token, slot) pairs");
    if (gating != 0 && gating != 1) return fail(GGML_HIP_ERR_ARG, "gating %d (0 softmax, 1 sigmoid)", gating);
    if (ld_logits < n_expert) return fail(GGML_HIP_ERR_ARG, "ld_logits %lld < n_expert %d", (long long)ld_logits, n_expert);
    if (n_tokens == 0) return GGML_HIP_OK;
    if (!d_logits || !d_ids || !d_weights) return fail(GGML_HIP_ERR_ARG, "null argument");
    HIP_TRY(launch_moe_topk(d_logits, ld_logits, n_tokens, n_expert, n_used, gating, normalize, scale, d_ids, d_weights, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_moe_combine_dev(const float *d_y, int64_t ldy, const float *d_weights, int64_t n_tokens, int n_used, int64_t M, const float *d_addend,
                             int64_t ld_add, float *d_dst, int64_t ldd, void *stream) {
    if (n_tokens < 0) return fail(GGML_HIP_ERR_ARG, "n_tokens %lld", (long long)n_tokens);
    if (n_used < 1 || n_used > 64) return fail(GGML_HIP_ERR_SHAPE, "n_used %d (1 .. 64)", n_used);
    if (n_tokens > MOE_GROUPED_MAX_PAIRS / n_used) return fail(GGML_HIP_ERR_SHAPE, "more than 2^20 (token, slot) pairs");
    if (M < 1 || ldy < M || ldd < M || (d_addend && ld_add < M)) return fail(GGML_HIP_ERR_SHAPE, "M < 1, or a row stride below M");
    if (n_tokens == 0) return GGML_HIP_OK;
    if (!d_y || !d_weights || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (M > ((int64_t)1 << 31)) return fail(GGML_HIP_ERR_SHAPE, "M %lld", (long long)M);
    HIP_TRY(launch_moe_combine(d_y, ldy, d_weights, n_tokens, n_used, M, d_addend, ld_add, d_dst, ldd, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_silu_mul_rows_dev(const float *d_a, const float *d_b, float *d_silu, float *d_y, int64_t nrows, int64_t k, void *stream) {
    if (nrows <= 0 || k <= 0) return GGML_HIP_OK;
    if (!d_a || !d_b || !d_y) return fail(GGML_HIP_ERR_ARG, "null argument (d_silu alone may be null)");
    if (nrows > ((int64_t)1 << 39) / k) return fail(GGML_HIP_ERR_SHAPE, "more than 2^39 elements");
    HIP_TRY(launch_silu_mul_f32(d_a, d_b, d_silu, d_y, nrows * k, (hipStream_t)stream));
    return GGML_HIP_OK;
}

}  // extern "C"
