// moe.hip -- the two data movers of ggml_hip_mul_mat_id_dev's batch route (moe.cpp): src1 rows into expert-contiguous order, the
// per-expert results back to their pairs.  Both take their slice of the row map BY VALUE (moe_map, common.h): a launch carries its own
// map, so nothing in host or device memory has to outlive the call and a captured call replays the routing it was captured with.
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

}  // namespace

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
