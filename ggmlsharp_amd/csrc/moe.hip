// moe.hip -- the two data movers of ggml_hip_mul_mat_id_dev's batch route (moe.cpp): src1 rows into expert-contiguous order, the
// per-expert results back to their pairs.  Both take their slice of the row map BY VALUE (moe_map, common.h): a launch carries its own
// map, so nothing in host or device memory has to outlive the call and a captured call replays the routing it was captured with.
// Below them the device side of ggml_hip_mul_mat_id_grouped_dev: the routing kernels, which build the same maps (and a tile table) in
// device memory from the ids there, and the gather / scatter that read those maps -- a captured call then follows the ids of each replay.
#include "common.h"

namespace {

// sorted row j0 + j (j < n) <- the src1 row of pair map.v[j]: token p / n_used, slot p % n_used.  One workgroup per row.
template <bool VEC>
__global__ __launch_bounds__(256) void moe_gather_kernel(const moe_map map, int n, int64_t j0, int n_used, const float *__restrict__ x,
                                                         int64_t ld1_token, int64_t ld1_slot, int64_t K, float *__restrict__ g, int64_t ldg) {
    const int j = blockIdx.x;
    if (j >= n) return;
    const int p = map.v[j];
    const float *src = x + (int64_t)(p / n_used) * ld1_token + (int64_t)(p % n_used) * ld1_slot;
    float *dst = g + (j0 + j) * ldg;
    if constexpr (VEC) {
        for (int64_t k = 4 * (int64_t)threadIdx.x; k < K; k += 4 * 256) *(float4 *)(dst + k) = *(const float4 *)(src + k);
    } else {
        for (int64_t k = threadIdx.x; k < K; k += 256) dst[k] = src[k];
    }
}

// pair p0 + i (i < n) <- sorted row map.v[i], or +0.0f where map.v[i] < 0 (a pair whose id is outside the set).  One workgroup per pair.
__global__ __launch_bounds__(256) void moe_scatter_kernel(const moe_map map, int n, int64_t p0, const float *__restrict__ r, int64_t ldr,
                                                          int64_t M, float *__restrict__ dst, int64_t ldd) {
    const int i = blockIdx.x;
    if (i >= n) return;
    const int j = map.v[i];
    float *out = dst + (p0 + i) * ldd;
    const float *src = r + (int64_t)(j < 0 ? 0 : j) * ldr;
    for (int64_t m = threadIdx.x; m < M; m += 256) out[m] = j < 0 ? 0.0f : src[m];
}

// ---- the grouped route: routing on the device.  Integer work only, and every table entry has exactly one writer: nothing depends on scheduling. ----
// (1) one wave per expert e scans the ids in order: pair p with ids[p] == e gets its rank among e's pairs (ballots: ascending p) into pos[p],
//     the wave's total is count[e].  Expert 0's wave also marks the pairs whose id is outside the set (pos[p] = -1) -- the id is only ever
//     COMPARED.  All waves together fill `order` with -1 (padding until (3) says otherwise).
__global__ __launch_bounds__(64) void moe_route_count_kernel(const int32_t *__restrict__ ids, int P, int n_expert, int32_t *__restrict__ count,
                                                             int32_t *__restrict__ pos, int32_t *__restrict__ order, int rows) {
    const int e = blockIdx.x, lane = threadIdx.x;
    for (int j = e * 64 + lane; j < rows; j += n_expert * 64) order[j] = -1;
    int run = 0;
    for (int p0 = 0; p0 < P; p0 += 64) {
        const int p = p0 + lane;
        const int id = p < P ? ids[p] : -1;
        const bool mine = p < P && id == e;
        const unsigned long long b = __ballot(mine);
        if (mine) pos[p] = run + __popcll(b & ((1ull << lane) - 1ull));
        if (e == 0 && p < P && (id < 0 || id >= n_expert)) pos[p] = -1;
        run += __popcll(b);
    }
    if (lane == 0) count[e] = run;
}

// (2) one workgroup: segments in ascending expert order, each padded to whole tiles of 32 sorted rows -- an exclusive scan of the experts'
//     tile counts (n_expert <= 1024: one thread each) -- then every expert writes its own tiles; n_tiles = the scan's total.
__global__ __launch_bounds__(1024) void moe_route_layout_kernel(const int32_t *__restrict__ count, int n_expert, int32_t *__restrict__ first,
                                                                moe_tile *__restrict__ tiles, int32_t *__restrict__ n_tiles, int max_tiles) {
    __shared__ int32_t sc[1024];
    const int e = threadIdx.x;
    const int c = e < n_expert ? count[e] : 0, own = (c + 31) / 32;
    sc[e] = own;
    __syncthreads();
    for (int d = 1; d < 1024; d <<= 1) {
        const int v = e >= d ? sc[e - d] : 0;
        __syncthreads();
        sc[e] += v;
        __syncthreads();
    }
    const int t0 = sc[e] - own;
    if (e == 1023) *n_tiles = sc[e] < max_tiles ? sc[e] : max_tiles;      // (the bound holds for every routing: plan.h; the clamp costs nothing)
    if (e < n_expert) {
        first[e] = 32 * t0;
        for (int t = 0; t < own && t0 + t < max_tiles; ++t) tiles[t0 + t] = moe_tile{e, 32 * (t0 + t), c - 32 * t < 32 ? c - 32 * t : 32, 0};
    }
}

// (3) pair p -> its sorted row: first[id] + rank; the inverse into order
__global__ __launch_bounds__(256) void moe_route_place_kernel(const int32_t *__restrict__ ids, int P, int n_expert, const int32_t *__restrict__ first,
                                                              int32_t *__restrict__ pos, int32_t *__restrict__ order, int rows) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= P) return;
    const int id = ids[p];
    if (id < 0 || id >= n_expert) return;                   // (pos[p] is -1 already)
    const int j = first[id] + pos[p];
    if (j >= rows) return;                                  // (never: the bound)
    pos[p] = j;
    order[j] = p;
}

// sorted row j <- the src1 row of pair order[j], zeros for padding.  One workgroup per row.
__global__ __launch_bounds__(256) void moe_gather_dev_kernel(const int32_t *__restrict__ order, int n_used, const float *__restrict__ x, int64_t ld1_token,
                                                             int64_t ld1_slot, int64_t K, float *__restrict__ g, int64_t ldg) {
    const int64_t j = blockIdx.x;
    const int p = order[j];
    float *dst = g + j * ldg;
    if (p < 0) {
        for (int64_t k = 4 * (int64_t)threadIdx.x; k < K; k += 4 * 256) *(float4 *)(dst + k) = float4{0.0f, 0.0f, 0.0f, 0.0f};
        return;
    }
    const float *src = x + (int64_t)(p / n_used) * ld1_token + (int64_t)(p % n_used) * ld1_slot;
    for (int64_t k = 4 * (int64_t)threadIdx.x; k < K; k += 4 * 256) *(float4 *)(dst + k) = *(const float4 *)(src + k);
}

// pair p <- sorted row pos[p], or +0.0f where pos[p] < 0.  One workgroup per pair.
__global__ __launch_bounds__(256) void moe_scatter_dev_kernel(const int32_t *__restrict__ pos, const float *__restrict__ r, int64_t ldr, int64_t M,
                                                              float *__restrict__ dst, int64_t ldd) {
    const int64_t p = blockIdx.x;
    const int j = pos[p];
    float *out = dst + p * ldd;
    const float *src = r + (int64_t)(j < 0 ? 0 : j) * ldr;
    for (int64_t m = threadIdx.x; m < M; m += 256) out[m] = j < 0 ? 0.0f : src[m];
}

}  // namespace

hipError_t launch_moe_route(const int32_t *ids, int64_t P, int n_expert, const moe_route &r, int64_t max_tiles, hipStream_t st) {
    if (P <= 0 || P > (1 << 20) || n_expert < 1 || n_expert > 1024 || max_tiles <= 0 || 32 * max_tiles > 0x7FFFFFFF) return hipErrorInvalidValue;
    const int rows = (int)(32 * max_tiles);
    moe_route_count_kernel<<<dim3((unsigned)n_expert), 64, 0, st>>>(ids, (int)P, n_expert, r.count, r.pos, r.order, rows);
    moe_route_layout_kernel<<<dim3(1), 1024, 0, st>>>(r.count, n_expert, r.first, r.tiles, r.n_tiles, (int)max_tiles);
    moe_route_place_kernel<<<dim3((unsigned)((P + 255) / 256)), 256, 0, st>>>(ids, (int)P, n_expert, r.first, r.pos, r.order, rows);
    return hipGetLastError();
}

hipError_t launch_moe_gather_dev(const int32_t *order, int64_t rows, int n_used, const float *x, int64_t ld1_token, int64_t ld1_slot, int64_t K, float *g,
                                 int64_t ldg, hipStream_t st) {
    if (rows <= 0) return hipSuccess;
    if (((uintptr_t)x & 15) != 0 || ((uintptr_t)g & 15) != 0 || ld1_token % 4 != 0 || ld1_slot % 4 != 0 || ldg % 4 != 0 || K % 4 != 0) return hipErrorInvalidValue;
    moe_gather_dev_kernel<<<dim3((unsigned)rows), 256, 0, st>>>(order, n_used, x, ld1_token, ld1_slot, K, g, ldg);
    return hipGetLastError();
}

hipError_t launch_moe_scatter_dev(const int32_t *pos, int64_t P, const float *r, int64_t ldr, int64_t M, float *dst, int64_t ldd, hipStream_t st) {
    if (P <= 0) return hipSuccess;
    moe_scatter_dev_kernel<<<dim3((unsigned)P), 256, 0, st>>>(pos, r, ldr, M, dst, ldd);
    return hipGetLastError();
}

hipError_t launch_moe_gather(const moe_map &map, int n, int64_t j0, int n_used, const float *x, int64_t ld1_token, int64_t ld1_slot,
                             int64_t K, float *g, int64_t ldg, hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > MOE_MAP_CHUNK) return hipErrorInvalidValue;
    const bool vec = ((uintptr_t)x & 15) == 0 && ((uintptr_t)g & 15) == 0 && ld1_token % 4 == 0 && ld1_slot % 4 == 0 && ldg % 4 == 0 && K % 4 == 0;
    if (vec) moe_gather_kernel<true><<<dim3((unsigned)n), 256, 0, st>>>(map, n, j0, n_used, x, ld1_token, ld1_slot, K, g, ldg);
    else moe_gather_kernel<false><<<dim3((unsigned)n), 256, 0, st>>>(map, n, j0, n_used, x, ld1_token, ld1_slot, K, g, ldg);
    return hipGetLastError();
}

hipError_t launch_moe_scatter(const moe_map &map, int n, int64_t p0, const float *r, int64_t ldr, int64_t M, float *dst, int64_t ldd,
                              hipStream_t st) {
    if (n <= 0) return hipSuccess;
    if (n > MOE_MAP_CHUNK) return hipErrorInvalidValue;
    moe_scatter_kernel<<<dim3((unsigned)n), 256, 0, st>>>(map, n, p0, r, ldr, M, dst, ldd);
    return hipGetLastError();
}
