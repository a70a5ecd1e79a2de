// sample.hip -- the sampler behind the LM head (ggml_hip_argmax_rows_dev / ggml_hip_sample_topk_dev, decode_ends.cpp): the k best of a row of
// n_vocab logits, their probabilities under a temperature, top-p and the pick.  include/ggml_hip_ext.h states all of it; the text there is
// the contract.
//
// SELECTION is moe_route.hip's rule on a vocabulary: every logit becomes a 64-bit key
//     (order-preserving image of the f32: NaN -> 0 below -inf, both zeros -> one key) << 32 | (0xFFFFFFFF - index)
// so "larger logit first, equal logits: smaller index first" IS max over uint64, all keys of a row are distinct, and a key of 0 means
// "nothing here" (the low word of a real key is at least 0xFFF00000).  Because the order is total, any correct selection gives the same bits;
// this one is k rounds of a workgroup-wide key maximum with the winner taken out of its owner's registers.
//
// Two launches whatever the shape, no atomics, nothing read back:
//   topk_chunk_kernel   one workgroup of 256 threads per (row, chunk of TOPK_CHUNK logits): sixteen keys per thread in registers, k rounds,
//                       the chunk's best k keys (zeros past the chunk's length) to the work buffer in rank order.
//   topk_merge_kernel   one workgroup per row: the n_chunks * k candidate keys (at most 256 * 64 = 64 per thread) in registers, k rounds
//                       again; then the first wave turns the k winners into ids, e, S, p, n_keep and the pick -- lane s holds rank s, and
//                       every sequential sum of the header is a uniform loop over ranks in the header's order, the same in every lane.
// k = 1 is instantiated apart (ONE): one round, no removal, no probabilities.
#include "common.h"

#define TOPK_CHUNK 4096                 /* 16 logits per thread; n_vocab <= 2^20 gives at most 256 chunks */
#define TOPK_MAX_K 64

namespace {

__device__ __forceinline__ uint32_t topk_key(float l) {               // moe_route.hip route_key
    const uint32_t u = __float_as_uint(l);
    if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;                   // NaN: below every number (-inf is 0x007FFFFF)
    if (u == 0x80000000u) return 0x80000000u;                         // -0.0 == +0.0
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float topk_logit(uint32_t key) {           // the inverse, for the keys of numbers (a zero comes back as +0.0)
    return __uint_as_float((key & 0x80000000u) ? (key & 0x7FFFFFFFu) : ~key);
}
__device__ __forceinline__ uint64_t topk_pair(float l, int64_t index) { return ((uint64_t)topk_key(l) << 32) | (uint32_t)(0xFFFFFFFFu - (uint32_t)index); }

__device__ __forceinline__ uint64_t max_u64(uint64_t a, uint64_t b) { return a > b ? a : b; }
template <int CTRL>
__device__ __forceinline__ uint64_t dpp_u64(uint64_t v) {
    return (uint64_t)(uint32_t)dpp_i<CTRL>((int)(uint32_t)v) | ((uint64_t)(uint32_t)dpp_i<CTRL>((int)(uint32_t)(v >> 32)) << 32);
}
// lane `lane` of v for a lane index that is the same in every lane (v_readlane: no LDS round trip, unlike a shuffle = ds_bpermute)
__device__ __forceinline__ uint32_t lane_u32(uint32_t v, int lane) { return (uint32_t)__builtin_amdgcn_readlane((int)v, lane); }
__device__ __forceinline__ float lane_f32(float v, int lane) { return __uint_as_float(lane_u32(__float_as_uint(v), lane)); }
__device__ __forceinline__ uint64_t lane_u64(uint64_t v, int lane) { return (uint64_t)lane_u32((uint32_t)v, lane) | ((uint64_t)lane_u32((uint32_t)(v >> 32), lane) << 32); }
// the wave's maximum, the same in every lane: inside a row of 16 by DPP (after the two xor steps a quad is uniform, so a mirror joins uniform
// groups; max is idempotent), then the four rows' values are read from lanes 0, 16, 32, 48
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
    v = max_u64(v, dpp_u64<DPP_XOR1>(v));
    v = max_u64(v, dpp_u64<DPP_XOR2>(v));
    v = max_u64(v, dpp_u64<DPP_HALF_MIRROR>(v));
    v = max_u64(v, dpp_u64<DPP_ROW_MIRROR>(v));
    return max_u64(max_u64(lane_u64(v, 0), lane_u64(v, 16)), max_u64(lane_u64(v, 32), lane_u64(v, 48)));
}

// One round over the NPT keys every thread of a 256-thread workgroup holds: the workgroup's largest key in every thread; unless KEEP, the
// winner leaves its owner's registers.  s_wave: 2 x 4 slots, alternating by round, so that one barrier per round is enough (the slots a
// round reads are next written two rounds later, behind the next round's barrier).
template <int NPT, bool KEEP>
__device__ __forceinline__ uint64_t topk_round(uint64_t (&key)[NPT], uint64_t (*s_wave)[4], int round) {
    uint64_t best = key[0];
#pragma unroll
    for (int j = 1; j < NPT; ++j) best = max_u64(best, key[j]);
    best = wave_max_u64(best);
    uint64_t *slot = s_wave[round & 1];
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = best;
    __syncthreads();
    best = max_u64(max_u64(slot[0], slot[1]), max_u64(slot[2], slot[3]));
    if (!KEEP) {
#pragma unroll
        for (int j = 0; j < NPT; ++j)
            if (key[j] == best) key[j] = 0ull;              // (keys are distinct; a 0 stays a 0)
    }
    return best;
}

// (row, chunk) -> work[(row * n_chunks + chunk) * k + s], s < k: the chunk's keys of rank s, 0 past its length
template <bool ONE, bool VEC>
__global__ __launch_bounds__(256) void topk_chunk_kernel(const float *__restrict__ logits, int64_t ld, int64_t n_vocab, int n_chunks, int k, uint64_t *__restrict__ work) {
    constexpr int NPT = TOPK_CHUNK / 256;
    __shared__ uint64_t s_wave[2][4];
    const int64_t r = blockIdx.x / n_chunks, c = blockIdx.x % n_chunks;
    const float *row = logits + r * ld;
    const int64_t e0 = c * TOPK_CHUNK;
    const int t = threadIdx.x;
    uint64_t key[NPT];
    if (VEC) {                                              // (row and e0 are 16-byte aligned)
#pragma unroll
        for (int j = 0; j < NPT / 4; ++j) {
            const int64_t e = e0 + (int64_t)(j * 256 + t) * 4;
            if (e + 4 <= n_vocab) {
                const float4 f = *(const float4 *)(row + e);
                key[4 * j] = topk_pair(f.x, e); key[4 * j + 1] = topk_pair(f.y, e + 1); key[4 * j + 2] = topk_pair(f.z, e + 2); key[4 * j + 3] = topk_pair(f.w, e + 3);
            } else {
#pragma unroll
                for (int q = 0; q < 4; ++q) key[4 * j + q] = e + q < n_vocab ? topk_pair(row[e + q], e + q) : 0ull;
            }
        }
    } else {
#pragma unroll
        for (int j = 0; j < NPT; ++j) {
            const int64_t e = e0 + j * 256 + t;
            key[j] = e < n_vocab ? topk_pair(row[e], e) : 0ull;
        }
    }
    uint64_t *out = work + (int64_t)blockIdx.x * k;
    if (ONE) {
        const uint64_t best = topk_round<NPT, true>(key, s_wave, 0);
        if (t == 0) out[0] = best;
    } else {
        for (int s = 0; s < k; ++s) {
            const uint64_t best = topk_round<NPT, false>(key, s_wave, s);
            if (t == 0) out[s] = best;
        }
    }
}

struct sample_args {
    float inv_temp, top_p;
    const float *u;          // null: no pick
    int32_t *ids;            // [n_rows * k]
    float *probs;            // [n_rows * k] or null
    int32_t *token;          // [n_rows] or null
};

// row r: the n_cand = n_chunks * k candidates of the work buffer -> the k winners; then (unless ONE) the first wave's arithmetic
template <int NPT, bool ONE>
__global__ __launch_bounds__(256) void topk_merge_kernel(const uint64_t *__restrict__ work, int n_cand, int k, const sample_args a) {
    __shared__ uint64_t s_wave[2][4];
    __shared__ uint64_t s_sel[TOPK_MAX_K];
    const int64_t r = blockIdx.x;
    const int t = threadIdx.x;
    const uint64_t *cand = work + r * n_cand;
    uint64_t key[NPT];
#pragma unroll
    for (int j = 0; j < NPT; ++j) {
        const int i = j * 256 + t;
        key[j] = i < n_cand ? cand[i] : 0ull;
    }
    if (ONE) {
        const uint64_t best = topk_round<NPT, true>(key, s_wave, 0);
        if (t == 0) a.ids[r] = (int32_t)(0xFFFFFFFFu - (uint32_t)best);
        return;
    }
    for (int s = 0; s < k; ++s) {
        const uint64_t best = topk_round<NPT, false>(key, s_wave, s);
        if (t == 0) s_sel[s] = best;
    }
    __syncthreads();
    if (t >= 64) return;
    const int lane = t;
    const uint64_t mine = lane < k ? s_sel[lane] : 0ull;
    const int32_t id = (int32_t)(0xFFFFFFFFu - (uint32_t)mine);
    if (lane < k) a.ids[r * k + lane] = id;
    if (!a.probs) return;
    // e_s = expf((l_s - l_0) * inv_temp);  S = e_0 + e_1 + ... in rank order;  p_s = e_s / S
    const float l = topk_logit((uint32_t)(mine >> 32));
    const float l0 = lane_f32(l, 0);
    const float z = (l - l0) * a.inv_temp;
    const float e = expf(z);
    float S = lane_f32(e, 0);
    for (int s = 1; s < k; ++s) S = S + lane_f32(e, s);
    const float p = e / S;
    if (lane < k) a.probs[r * k + lane] = p;
    if (!a.u || !a.token) return;
    // n_keep: the smallest n >= 1 with p_0 + .. + p_(n-1) >= top_p, k if none (top_p >= 1: k without summing); C: the sum of the kept
    int n_keep = k;
    if (!(a.top_p >= 1.0f)) {
        float acc = lane_f32(p, 0);
        for (int n = 1; n <= k; ++n) {
            if (n > 1) acc = acc + lane_f32(p, n - 1);
            if (acc >= a.top_p) { n_keep = n; break; }
        }
    }
    float C = lane_f32(p, 0);
    for (int s = 1; s < n_keep; ++s) C = C + lane_f32(p, s);
    const float target = a.u[r] * C;
    // the first s < n_keep whose running sum exceeds the target, else rank n_keep - 1
    int pick = n_keep - 1;
    float run = lane_f32(p, 0);
    for (int s = 0; s < n_keep; ++s) {
        if (s > 0) run = run + lane_f32(p, s);
        if (run > target) { pick = s; break; }
    }
    const int32_t tok = (int32_t)lane_u32((uint32_t)id, pick);
    if (lane == 0) a.token[r] = tok;
}

}  // namespace

int64_t topk_chunk_len() { return TOPK_CHUNK; }

// work: n_rows * n_chunks * k keys of 8 bytes, 8-byte aligned.  probs == nullptr: ids alone; u / token null: no pick.
hipError_t launch_sample_topk(const float *logits, int64_t ld, int64_t n_rows, int64_t n_vocab, int k, float inv_temp, float top_p, const float *u,
                              int32_t *ids, float *probs, int32_t *token, void *work, hipStream_t st) {
    if (n_rows <= 0) return hipSuccess;
    if (n_vocab < 1 || n_vocab > ((int64_t)1 << 20) || k < 1 || k > TOPK_MAX_K || k > n_vocab || n_rows > 4096 || ld < n_vocab) return hipErrorInvalidValue;
    const int n_chunks = (int)((n_vocab + TOPK_CHUNK - 1) / TOPK_CHUNK);
    const bool vec = ((uintptr_t)logits & 15) == 0 && ld % 4 == 0;
    const bool one = k == 1 && !probs;
    uint64_t *w64 = (uint64_t *)work;
    const dim3 grid1((unsigned)(n_rows * n_chunks));
    if (one) {
        if (vec) topk_chunk_kernel<true, true><<<grid1, 256, 0, st>>>(logits, ld, n_vocab, n_chunks, k, w64);
        else topk_chunk_kernel<true, false><<<grid1, 256, 0, st>>>(logits, ld, n_vocab, n_chunks, k, w64);
    } else {
        if (vec) topk_chunk_kernel<false, true><<<grid1, 256, 0, st>>>(logits, ld, n_vocab, n_chunks, k, w64);
        else topk_chunk_kernel<false, false><<<grid1, 256, 0, st>>>(logits, ld, n_vocab, n_chunks, k, w64);
    }
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const sample_args a = {inv_temp, top_p, token ? u : nullptr, ids, probs, u ? token : nullptr};
    const int n_cand = n_chunks * k;
    const dim3 grid2((unsigned)n_rows);
    const int npt = (n_cand + 255) / 256;
#define MERGE(N) topk_merge_kernel<N, false><<<grid2, 256, 0, st>>>(w64, n_cand, k, a)
    if (one) topk_merge_kernel<1, true><<<grid2, 256, 0, st>>>(w64, n_cand, k, a);      // (n_cand = n_chunks <= 256)
    else if (npt <= 1) MERGE(1);
    else if (npt <= 2) MERGE(2);
    else if (npt <= 4) MERGE(4);
    else if (npt <= 8) MERGE(8);
    else if (npt <= 16) MERGE(16);
    else if (npt <= 32) MERGE(32);
    else MERGE(64);
#undef MERGE
    return hipGetLastError();
}
