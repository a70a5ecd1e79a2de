// moe_route.hip -- the two ends of a mixture-of-experts block around the expert-routed products (moe.cpp): the ROUTER, router logits -> the
// n_used expert ids and gate weights of every token (ggml_hip_moe_route_dev), and the COMBINE, the weighted sum of a token's pair rows
// (ggml_hip_moe_combine_dev).  include/ggml_hip_ext.h states both; the arithmetic there is the contract.
//
// Router: one wave per token, no LDS, no barrier.  Lane l holds experts l, l + 64, ... (NPL of them, at most 16) as PAIRS
//     (key << 32) | (1024 - e),   key = an order-preserving image of the logit: NaN -> 0 (below -inf), both zeros -> one key,
// 0 for an expert that does not exist or was taken.  All pairs of a token are distinct, so the wave-wide maximum of the pair IS the rank rule
// "larger logit first, equal logits: smaller index first", and n_used rounds of it give distinct ids inside [0, n_expert) whatever the
// logits hold.  The logit is only ever compared; no address is formed from it.
#include "common.h"

namespace {

__device__ __forceinline__ uint32_t route_key(float l) {
    const uint32_t u = __float_as_uint(l);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;                 // NaN: below every number (-inf is 0x007FFFFF)
    if (u == 0x80000000u) return 0x80000000u;                       // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}

__device__ __forceinline__ float route_logit(uint32_t key) {        // the inverse, for the keys of numbers
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}

__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) {
        const uint32_t lo = (uint32_t)__shfl_xor((int)(uint32_t)v, d), hi = (uint32_t)__shfl_xor((int)(uint32_t)(v >> 32), d);
        const uint64_t o = ((uint64_t)hi << 32) | lo;
        v = o > v ? o : v;
    }
    return v;
}

__device__ __forceinline__ float wave_sum_f32(float v) {            // a fixed butterfly: x + y == y + x, so every lane ends with the same bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) v = v + __shfl_xor(v, d);
    return v;
}

template <int NPL>
__global__ __launch_bounds__(256) void moe_topk_kernel(const float *__restrict__ logits, int64_t ld, int n_tokens, int n_expert, int n_used, int gating,
                                                       int normalize, float scale, int32_t *__restrict__ ids, float *__restrict__ weights) {
    const int lane = threadIdx.x & 63;
    const int t = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (t >= n_tokens) return;                                      // (whole waves leave: no barrier below)
    const float *row = logits + (int64_t)t * ld;
    float l[NPL];
    uint64_t pair[NPL];
#pragma unroll
    for (int j = 0; j < NPL; ++j) {
        const int e = lane + 64 * j;
        l[j] = e < n_expert ? row[e] : 0.0f;
        pair[j] = e < n_expert ? ((uint64_t)route_key(l[j]) << 32) | (uint32_t)(1024 - e) : 0ull;
    }
    // a round: the wave's largest pair, taken out of its owner's registers
    auto take = [&]() -> uint64_t {
        uint64_t best = pair[0];
#pragma unroll
        for (int j = 1; j < NPL; ++j) best = pair[j] > best ? pair[j] : best;
        best = wave_max_u64(best);
        const int e = 1024 - (int)(uint32_t)best;
#pragma unroll
        for (int j = 0; j < NPL; ++j)
            if (e == lane + 64 * j) pair[j] = 0ull;
        return best;
    };
    uint64_t mine = take();                                         // slot s ends up in lane s (n_used <= 64)
    const float lmax = route_logit((uint32_t)(mine >> 32));
    float S = 1.0f;
    if (gating == 0) {                                              // softmax over ALL experts: a lane's chain in ascending e, then the butterfly
        float part = 0.0f;
#pragma unroll
        for (int j = 0; j < NPL; ++j) {
            if (lane + 64 * j < n_expert) {
                const float ex = expf(l[j] - lmax);
                part = j == 0 ? ex : part + ex;
            }
        }
        S = wave_sum_f32(part);
    }
    for (int s = 1; s < n_used; ++s) {
        const uint64_t b = take();
        if (lane == s) mine = b;
    }
    const float lsel = route_logit((uint32_t)(mine >> 32));
    float w = gating == 0 ? expf(lsel - lmax) / S : 1.0f / (1.0f + expf(-lsel));
    if (normalize) {                                                // w_0 + w_1 + ... in slot order
        float sum = __shfl(w, 0);
        for (int s = 1; s < n_used; ++s) sum = sum + __shfl(w, s);
        w = w / sum;
    }
    w = w * scale;
    if (lane < n_used) {
        ids[(int64_t)t * n_used + lane] = 1024 - (int32_t)(uint32_t)mine;
        weights[(int64_t)t * n_used + lane] = w;
    }
}

// dst[t, m] = (((w[t,0] * y[t,0,m]) + w[t,1] * y[t,1,m]) + ...) [+ addend[t, m]]: one rounding per product and per sum (the library is built
// without contraction).  A workgroup serves 256 * (VEC ? 4 : 1) columns of one token; dst may BE addend (an element is read, then written,
// by one thread), so neither is __restrict__.
template <bool VEC>
__global__ __launch_bounds__(256) void moe_combine_kernel(const float *__restrict__ y, int64_t ldy, const float *__restrict__ w, int n_used, int64_t M,
                                                          int blocks_per_token, const float *addend, int64_t ld_add, float *dst, int64_t ldd) {
    const int64_t t = blockIdx.x / blocks_per_token;
    const int64_t m = ((int64_t)(blockIdx.x % blocks_per_token) * 256 + threadIdx.x) * (VEC ? 4 : 1);
    if (m >= M) return;
    const float *yr = y + t * n_used * ldy + m;
    const float *wr = w + t * n_used;
    if (VEC && m + 4 <= M) {
        float4 v = *(const float4 *)yr;
        float ws = wr[0];
        float4 acc = {ws * v.x, ws * v.y, ws * v.z, ws * v.w};
#pragma unroll 4
        for (int s = 1; s < n_used; ++s) {
            v = *(const float4 *)(yr + s * ldy);
            ws = wr[s];
            acc.x = acc.x + ws * v.x; acc.y = acc.y + ws * v.y; acc.z = acc.z + ws * v.z; acc.w = acc.w + ws * v.w;
        }
        if (addend) {
            const float4 a = *(const float4 *)(addend + t * ld_add + m);
            acc.x = acc.x + a.x; acc.y = acc.y + a.y; acc.z = acc.z + a.z; acc.w = acc.w + a.w;
        }
        *(float4 *)(dst + t * ldd + m) = acc;
        return;
    }
    const int64_t m1 = VEC ? M : m + 1;                             // (the vector form's last thread: up to three columns one by one)
    for (int64_t c = m; c < m1; ++c) {
        float acc = wr[0] * yr[c - m];
        for (int s = 1; s < n_used; ++s) acc = acc + wr[s] * yr[s * ldy + (c - m)];
        if (addend) acc = acc + addend[t * ld_add + c];
        dst[t * ldd + c] = acc;
    }
}

}  // namespace

hipError_t launch_moe_topk(const float *logits, int64_t ld, int64_t n_tokens, int n_expert, int n_used, int gating, int normalize, float scale,
                           int32_t *ids, float *weights, hipStream_t st) {
    if (n_tokens <= 0) return hipSuccess;
    if (n_expert < 1 || n_expert > 1024 || n_used < 1 || n_used > 64 || n_used > n_expert || n_tokens > (1 << 20) || ld < n_expert) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((n_tokens + 3) / 4));
    const int npl = (n_expert + 63) / 64;
#define TOPK(N) moe_topk_kernel<N><<<grid, 256, 0, st>>>(logits, ld, (int)n_tokens, n_expert, n_used, gating, normalize, scale, ids, weights)
    if (npl <= 1) TOPK(1);
    else if (npl <= 2) TOPK(2);
    else if (npl <= 4) TOPK(4);
    else if (npl <= 8) TOPK(8);
    else TOPK(16);
#undef TOPK
    return hipGetLastError();
}

hipError_t launch_moe_combine(const float *y, int64_t ldy, const float *w, int64_t n_tokens, int n_used, int64_t M, const float *addend, int64_t ld_add,
                              float *dst, int64_t ldd, hipStream_t st) {
    if (n_tokens <= 0 || M <= 0) return hipSuccess;
    const bool vec = (((uintptr_t)y | (uintptr_t)dst | (uintptr_t)addend) & 15) == 0 && ldy % 4 == 0 && ldd % 4 == 0 && (!addend || ld_add % 4 == 0);
    const int64_t per_block = vec ? 1024 : 256, bpt = (M + per_block - 1) / per_block;
    if (n_used < 1 || bpt > 0x7FFFFFFF / n_tokens) return hipErrorInvalidValue;
    const dim3 grid((unsigned)(n_tokens * bpt));
    if (vec) moe_combine_kernel<true><<<grid, 256, 0, st>>>(y, ldy, w, n_used, M, (int)bpt, addend, ld_add, dst, ldd);
    else moe_combine_kernel<false><<<grid, 256, 0, st>>>(y, ldy, w, n_used, M, (int)bpt, addend, ld_add, dst, ldd);
    return hipGetLastError();
}
