// gemv.hip -- K2: quantized mat-vec / skinny mat-mat (N <= GEMV_MAX_N), HBM-bandwidth bound.
//
// Computes the COMPUTE phase of ggml_compute_forward_mul_mat_q_f32 (Ggml.cs:6676-6698) for few src1 rows:
//   dst[n*ldd + m] = sum_b dw[m,b] * da[n,b] * sum_{k in b} w[m,k] * a[n,k]
// with the integer block sums exact (ggml_vec_dot_q4_0_q8_0 Ggml.cs:1136-1159, _q5_0_q8_0 1270-1298,
// _q8_0_q8_0 1362-1378, _q4_1_q8_1 1176-1198, _q5_1_q8_1 1318-1344, _q4_2_q8_0 1216-1252 -- the last two with IEEE-half
// scales, SURVEY D7 intent) and the f32 scale-accumulate per block as in :1158.
// Only the order of the f32 additions over blocks differs from the scalar loop.
//
// Mapping, chosen for the planar weight layout ([k-block][row][16 B]):
//   workgroup = 16 weight rows x all K; lane = (row r = lane & 15, k-lane kq = lane >> 4); the 8 waves x 4 k-lanes
//   are 32 "k-workers", worker u takes blocks u, u+32, u+64, ...  A wave-wide 16-byte load therefore touches four
//   256-byte contiguous segments, every lane keeps 4 independent loads in flight, and a row's dot product needs
//   only two xor-shuffles plus one LDS pass to combine -- no atomics, fixed summation tree (deterministic).
//   The Q8 activation vector (written by K1) is staged into LDS once per 128 k-blocks and read as broadcasts.
#include "common.h"
#include <cstring>

namespace {

// GV_ROWS (template parameter) = weight rows per workgroup; 16 everywhere (see launch_typed)
#ifndef GV_MAX_WGS
#define GV_MAX_WGS 512              // persistent grid: 2 workgroups per CU (A/B at M = 32000: 512 -> 17.3 us, 1024 -> 18.5, 2048 -> 19.2)
#endif
#ifndef GV_WAVES
#define GV_WAVES 8                     // waves per workgroup (A/B: 4 -> 8 waves: 4096^2 batch-1 5.81 -> 5.40 us, 4096 x 11008 12.1 -> 10.6,
                                       // N = 8 14.8 -> 12.0, M = 32000 17.25 -> 17.1; 16 waves: 5.23 us at 4096^2 but 19.9 us at M = 32000 with
                                       // one resident workgroup per CU, and 10 % slower on Q8_0 -- and the choice must not depend on M)
#endif
#define GV_THREADS (64 * GV_WAVES)
#define GV_NKQ (64 / GV_ROWS)          // k-lanes per wave
#define GV_WORKERS (GV_WAVES * GV_NKQ) // k-workers per workgroup
#define GV_CHUNK 128  // k-blocks of activations staged in LDS at a time (N <= 8)
// wider batches (9..16 src1 rows, two-step form only) stage fewer k-blocks at a time so that the image still fits 64 KB of LDS
// r4: a pseudo-type for weights living in the planar Q4_2 form ON INT8 PLANES (the Q6_K extension, kquants.hip): Q8_0's operand loads (two planes of
// int8 per k-block, no unpacking) with Q4_2's arithmetic (two 16-element sub-blocks per k-block, the second's scale in the m plane)
constexpr int GV_TYPE_I8X2 = 100;
template <int TYPE> constexpr bool GV_W_I8 = TYPE == GGML_TYPE_Q8_0 || TYPE == GV_TYPE_I8X2;
template <int TYPE> constexpr bool GV_TWO_SC = TYPE == GGML_TYPE_Q4_2 || TYPE == GV_TYPE_I8X2;

template <int NC> struct GvChunk { static constexpr int value = NC <= 8 ? GV_CHUNK : 64; };
#ifndef GV_NT
#define GV_NT 1       // non-temporal weight loads (A/B: -DGV_NT=0)
#endif
#ifndef GV_PF_WGS
#define GV_PF_WGS 256                  // the look-ahead form (N = 1, K <= 4096) keeps two row tiles per wave in flight: ONE workgroup per CU
                                       // (A/B 512 -> 256: M = 11008 8.0 -> 7.6 us, M = 32000 16.1 -> 15.7, M = 65536 28.9 -> 28.5; the forms
                                       // without look-ahead need the second workgroup: 32000 x 4096 x 8 37.1 -> 41.8 us with 256)
#endif
#ifndef GV_OLD_FUSED
#define GV_OLD_FUSED 0                 // A/B: the former fused kernel (block-wide staging behind a barrier)
#endif

using u32x4v = __attribute__((ext_vector_type(4))) uint32_t;
__device__ __forceinline__ uint4 ld_w(const uint8_t *p) {
#if GV_NT
    const u32x4v v = __builtin_nontemporal_load((const u32x4v *)p);
    return make_uint4(v[0], v[1], v[2], v[3]);
#else
    return *(const uint4 *)p;
#endif
}

// A result store the compiler's wait-count bookkeeping does not see.  On gfx9 loads and stores share `vmcnt` but only
// operations of one kind return in order, so with a store possibly in flight hipcc turns every later "wait for this load"
// into "wait for everything" -- which drained the look-ahead weight stream once per row tile.  Hidden in asm, the store
// still occupies a counter slot, which only makes the counted waits of the loads conservative (never short).
__device__ __forceinline__ void st_result(float *p, float v) {
    asm volatile("global_store_dword %0, %1, off" : : "v"(p), "v"(v) : "memory");
}

__device__ __forceinline__ int dot4(uint32_t a, uint32_t b, int c) {
    return __builtin_amdgcn_sdot4((int)a, (int)b, c, false);
}

// bit e of qh for e = 8i + {0,2,4,6} (sel = 0) or 8i + {1,3,5,7} (sel = 1), moved to bit 4 of bytes 0..3
__device__ __forceinline__ uint32_t q5_high_bits(uint32_t qh, int i, int sel) {
    const uint32_t t = ((qh >> (8 * i + sel)) & 0x55u);
    return (t * 0x00410410u) & 0x10101010u;
}

// FUSED = true : src1 is f32; every workgroup quantizes the activation chunk itself (the INIT phase of
//                 Ggml.cs:6641-6654 / quantize_row_q8_0 733-762, same arithmetic as K1, bit-exact) straight into LDS,
//                 so the whole mul_mat at small N is ONE launch and one dependent memory round trip.
// FUSED = false: src1 was quantized earlier (K1 planes, or reference Q8 blocks through ggml_hip_vec_dot).
// The weight loads of a chunk are issued before the activations are staged, so both latencies overlap.
template <int TYPE, int NC, bool FUSED, int GV_ROWS>
__global__ __launch_bounds__(GV_THREADS) void gemv_q_kernel(const uint8_t *__restrict__ qs, const uint32_t *__restrict__ gs,
                                                    const float *__restrict__ x, int64_t ld1,
                                                    const int8_t *__restrict__ a8, const float *__restrict__ ad,
                                                    const int32_t *__restrict__ as, float *__restrict__ dst, int64_t M,
                                                    int64_t Mpad, int64_t Npad, int64_t nbk, int64_t ldd, int N, int ntiles) {
    constexpr int CH = GvChunk<NC>::value;
    static_assert(GV_ROWS == 16, "the side image (ggml_hip_weight::gs) is laid out in 16-row tiles");
    static_assert(!FUSED || NC <= 8, "the fused form quantizes N columns per workgroup: N <= 8 only");
    __shared__ uint4 sA[CH * 2 * NC];
    __shared__ float sD[CH * NC];
    __shared__ int sS[CH * NC];
    __shared__ float sRed[GV_WAVES][NC][GV_ROWS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane % GV_ROWS, kq = lane / GV_ROWS, u = wave * GV_NKQ + kq;
    constexpr int BPL = GvChunk<NC>::value / GV_WORKERS;     // k-blocks per lane per chunk
    // Persistent over row tiles: virtual block vb = blockIdx.x, + gridDim.x, ... takes tile f(vb).  When all of K fits one
    // LDS chunk the activations are quantized / staged ONCE per workgroup instead of once per 16 rows (at M = 32000 the
    // 2000 redundant quantizations were ~8 % of the kernel).  Per-row arithmetic and summation tree are unchanged.
    // (Also loading the next tile's weights a tile ahead measured 10 % SLOWER: 19.3 vs 17.3 us at M = 32000.)
    const bool single_chunk = nbk <= GvChunk<NC>::value;
    bool staged = false;
    for (int vb = blockIdx.x; vb < ntiles; vb += gridDim.x) {
    const int tile = vb;   // launch order (see the fused kernel below)
    const int64_t row = (int64_t)tile * GV_ROWS + r;  // < Mpad by construction

    float acc[NC];
#pragma unroll
    for (int c = 0; c < NC; ++c) acc[c] = 0.0f;

    for (int64_t cb = 0; cb < nbk; cb += CH) {
        const int nbc = (int)((nbk - cb) < CH ? (nbk - cb) : CH);

        // 1. all of this lane's weight loads for the chunk go out first (4 x 16 B + scales in flight per lane, 512 lanes)
        uint4 q[BPL], q2[GV_W_I8<TYPE> ? BPL : 1];
        constexpr bool HAS_M = TYPE == GGML_TYPE_Q4_1 || TYPE == GGML_TYPE_Q5_1 || GV_TWO_SC<TYPE>;   // Q4_2: second scale
        constexpr bool HAS_H = TYPE == GGML_TYPE_Q5_0 || TYPE == GGML_TYPE_Q5_1;
        constexpr int NP = 1 + (HAS_M ? 1 : 0) + (HAS_H ? 1 : 0);
        float dw[BPL], mw[HAS_M ? BPL : 1];
        uint32_t hb[HAS_H ? BPL : 1];
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            const int bl = u + GV_WORKERS * j;
            const bool ok = bl < nbc;
            const int64_t b = cb + (ok ? bl : 0);
            // once-read weight stream: non-temporal loads (MI355X_MICROARCH.md nt-weights: issued -> landed -18 %)
            if (GV_W_I8<TYPE>) {
                q[j] = ld_w(qs + ((b * 2 + 0) * Mpad + row) * 16);
                q2[j] = ld_w(qs + ((b * 2 + 1) * Mpad + row) * 16);
            } else {
                q[j] = ld_w(qs + (b * Mpad + row) * 16);
            }
            // scales / mins / fifth bits from the tile-major side image (common.h ggml_hip_weight::gs)
            const uint32_t *g = gs + (((int64_t)tile * nbk + b) * NP) * 16 + r;
            dw[j] = ok ? __uint_as_float(g[0]) : 0.0f;   // dw = 0 kills the contribution of a block past the end
            if (HAS_M) mw[j] = ok ? __uint_as_float(g[16]) : 0.0f;
            if (HAS_H) hb[j] = g[16 * (NP - 1)];
        }

        // 2. activations of the chunk -> LDS (int8 even/odd planes + scale + block sum); once per workgroup if K fits
        if (!(single_chunk && staged)) {
        __syncthreads();  // previous chunk fully consumed
        if constexpr (FUSED) {
            const int t = tid & 7, grp = tid >> 3;             // 8 lanes per 32-element block, GV_THREADS / 8 groups
            constexpr int NGRP = GV_THREADS / 8;
            constexpr int ITEMS = GV_CHUNK * NC / NGRP;       // (column, k-block) items per group
            constexpr int UNR = ITEMS < 4 ? ITEMS : 4;          // loads in flight per lane
#pragma unroll 1
            for (int it0 = 0; it0 < ITEMS; it0 += UNR) {
                float4 v[UNR];
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    const int w0 = grp + NGRP * (it0 + k);
                    const int c = w0 / GV_CHUNK, bl = w0 % GV_CHUNK;
                    const int cc = c < N ? c : N - 1;
                    const int blc = bl < nbc ? bl : nbc - 1;
                    v[k] = *(const float4 *)(x + (int64_t)cc * ld1 + (cb + blc) * QK + 4 * t);
                }
#pragma unroll
                for (int k = 0; k < UNR; ++k) {
                    const int w0 = grp + NGRP * (it0 + k);
                    const int c = w0 / GV_CHUNK, bl = w0 % GV_CHUNK;
                    const bool live = c < N && bl < nbc;       // uniform over the 8 lanes of the group
                    float amax = fmaxf(fmaxf(fabsf(v[k].x), fabsf(v[k].y)), fmaxf(fabsf(v[k].z), fabsf(v[k].w)));
                    amax = group8_max(amax);
                    const float d = amax / 127.0f;                  // Ggml.cs:751
                    const float id = d != 0.0f ? 1.0f / d : 0.0f;   // Ggml.cs:752
                    const int q0 = (int)rintf(v[k].x * id), q1 = (int)rintf(v[k].y * id);   // Ggml.cs:758-759 (D1, D2)
                    const int q2_ = (int)rintf(v[k].z * id), q3 = (int)rintf(v[k].w * id);
                    const int sum = group8_sum(q0 + q1 + q2_ + q3);
                    const uint32_t e16 = ((uint32_t)q0 & 0xFFu) | (((uint32_t)q2_ & 0xFFu) << 8);
                    const uint32_t o16 = ((uint32_t)q1 & 0xFFu) | (((uint32_t)q3 & 0xFFu) << 8);
                    const bool even_lane = (t & 1) == 0;
                    const uint32_t recv = (uint32_t)dpp_i<DPP_XOR1>((int)(even_lane ? o16 : e16));
                    const uint32_t word = even_lane ? (e16 | (recv << 16)) : (recv | (o16 << 16));
                    if (live) {
                        uint8_t *base = (uint8_t *)sA;
                        const int h = even_lane ? 0 : 1, off = even_lane ? 2 * t : 2 * t - 2;
                        *(uint32_t *)(base + ((bl * 2 + h) * NC + c) * 16 + off) = word;
                        if (t == 0) { sD[bl * NC + c] = d; sS[bl * NC + c] = sum; }
                    }
                }
            }
        } else {
            for (int i = tid; i < nbc * 2 * NC; i += GV_THREADS) {
                const int c = i % NC, bh = i / NC;  // bh = b_local*2 + h
                const int cc = c < N ? c : N - 1;
                sA[i] = *(const uint4 *)(a8 + (((cb * 2 + bh) * Npad) + cc) * 16);
            }
            for (int i = tid; i < nbc * NC; i += GV_THREADS) {
                const int c = i % NC, bl = i / NC;
                const int cc = c < N ? c : N - 1;
                sD[i] = ad[(cb + bl) * Npad + cc];
                sS[i] = as[(cb + bl) * Npad + cc];
            }
        }
        __syncthreads();
        staged = true;
        }

        // 3. integer block dots + f32 scale-accumulate (Ggml.cs:1136-1159)
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            const int bl = (u + GV_WORKERS * j) < nbc ? (u + GV_WORKERS * j) : 0;
            const uint32_t qq[4] = {q[j].x, q[j].y, q[j].z, q[j].w};
            uint32_t lo[4], hi[4];
            if (GV_W_I8<TYPE>) {
                lo[0] = q[j].x; lo[1] = q[j].y; lo[2] = q[j].z; lo[3] = q[j].w;
                hi[0] = q2[j].x; hi[1] = q2[j].y; hi[2] = q2[j].z; hi[3] = q2[j].w;
            } else {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    lo[i] = qq[i] & 0x0F0F0F0Fu;          // elements 8i+0,2,4,6  (Ggml.cs:1149)
                    hi[i] = (qq[i] >> 4) & 0x0F0F0F0Fu;   // elements 8i+1,3,5,7  (Ggml.cs:1150)
                    if (HAS_H) {                          // Ggml.cs:1285-1289 / 1330-1334
                        lo[i] |= q5_high_bits(hb[j], i, 0);
                        hi[i] |= q5_high_bits(hb[j], i, 1);
                    }
                    if (TYPE == GGML_TYPE_Q4_2) {         // (nib - 8) bytewise: the two half-block sums need their own offsets
                        lo[i] = ((lo[i] | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
                        hi[i] = ((hi[i] | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const uint4 a0 = sA[(bl * 2 + 0) * NC + c];
                const uint4 a1 = sA[(bl * 2 + 1) * NC + c];
                const float da = sD[bl * NC + c];
                const int sa = sS[bl * NC + c];
                if (GV_TWO_SC<TYPE>) {
                    // elements 0..15 (the first 16-element block, scale dw) are words 0, 1 of both planes, 16..31 (scale
                    // mw) words 2, 3: sumf += (d0 * yd) * sumi_0; sumf += (d1 * yd) * sumi_1 (Ggml.cs:1249-1250)
                    int s0 = 0, s1 = 0;
                    s0 = dot4(lo[0], a0.x, s0); s0 = dot4(lo[1], a0.y, s0); s0 = dot4(hi[0], a1.x, s0); s0 = dot4(hi[1], a1.y, s0);
                    s1 = dot4(lo[2], a0.z, s1); s1 = dot4(lo[3], a0.w, s1); s1 = dot4(hi[2], a1.z, s1); s1 = dot4(hi[3], a1.w, s1);
                    acc[c] = fmaf(dw[j] * da, (float)s0, acc[c]);
                    acc[c] = fmaf(mw[j] * da, (float)s1, acc[c]);
                    continue;
                }
                int s = 0;
                s = dot4(lo[0], a0.x, s); s = dot4(lo[1], a0.y, s); s = dot4(lo[2], a0.z, s); s = dot4(lo[3], a0.w, s);
                s = dot4(hi[0], a1.x, s); s = dot4(hi[1], a1.y, s); s = dot4(hi[2], a1.z, s); s = dot4(hi[3], a1.w, s);
                if (TYPE == GGML_TYPE_Q4_0) s -= 8 * sa;   // (nib - 8) * a summed = nib*a summed - 8 * sum(a)
                if (TYPE == GGML_TYPE_Q5_0) s -= 16 * sa;
                acc[c] = fmaf(dw[j] * da, (float)s, acc[c]);
                if (TYPE == GGML_TYPE_Q4_1 || TYPE == GGML_TYPE_Q5_1) acc[c] = fmaf(mw[j], da * (float)sa, acc[c]);   // + m * (s0 + s1)
            }
        }
    }

#pragma unroll
    for (int c = 0; c < NC; ++c) {
        float v = acc[c];
#pragma unroll
        for (int sft = GV_ROWS; sft < 64; sft <<= 1) v += __shfl_xor(v, sft);
        if (kq == 0) sRed[wave][c][r] = v;
    }
    __syncthreads();
    for (int o = tid; o < GV_ROWS * NC; o += GV_THREADS) {
        const int c = o / GV_ROWS, rr = o % GV_ROWS;
        const int64_t m = (int64_t)tile * GV_ROWS + rr;
        float quad[GV_WAVES / 4];                                                                   // fixed tree over the waves
#pragma unroll
        for (int q = 0; q < GV_WAVES / 4; ++q)
            quad[q] = (sRed[4 * q][c][rr] + sRed[4 * q + 1][c][rr]) + (sRed[4 * q + 2][c][rr] + sRed[4 * q + 3][c][rr]);
        const float tot = GV_WAVES == 4 ? quad[0] : GV_WAVES == 8 ? quad[0] + quad[1 % (GV_WAVES / 4)]
                                        : (quad[0] + quad[1 % (GV_WAVES / 4)]) + (quad[2 % (GV_WAVES / 4)] + quad[3 % (GV_WAVES / 4)]);
        if (m < M && c < N) dst[(int64_t)c * ldd + m] = tot;
    }
    __syncthreads();   // sRed is rewritten by the next tile
    }
}

// ---------------------------------------------------------------------------------------------------------------------
// K2f: the FUSED form (src1 is f32, N <= 8), restated around the latency chain instead of the barrier.
//
// What bounded the kernel above at small M was not bandwidth but its dependent chain: weight loads, THEN the activation
// loads (vector-memory results return in issue order, so the x rows queued behind 40 KB of weights per workgroup), quantize,
// __syncthreads, dots, reduce (PMC round 1: 64-77 % of wave-cycles in s_waitcnt / s_barrier).  Here
//   * every WAVE quantizes exactly the k-blocks it consumes (its 4 k-lanes x 4 blocks of a 128-block chunk) into an LDS slice
//     of its own: no workgroup barrier between the INIT arithmetic and the dots, waves drift apart freely;
//   * the activation loads are issued FIRST, the weight stream right behind them: quantizing runs while the weights are in
//     flight (the compiler's vmcnt for the x registers leaves the younger weight loads outstanding);
//   * one barrier per row tile remains (the cross-wave reduction), on a double-buffered sRed.
// Arithmetic, block -> lane assignment and summation tree are those of the kernel above, so the bits are too.
// SC: all of K fits one chunk of 128 k-blocks (K <= 4096), a launch-time fact -- two instantiations instead of one kernel
// that carries both schedules in its registers (the combined form spilled: 24 B of scratch at 128 registers)
// PRO: the rms_norm -> mul prologue (common.h mm_prologue): the quantized row is (x * rms_scale) * g, computed here.
// MULTI: several weight matrices behind one activation matrix (common.h mv_set) -- its own kernels below: with the per-item
// selects in every kernel the single-matrix call lost 5-12 % (4096 x 4096: 4.6 -> 5.2 us)
// K8 (r4): the activations are quantized by the Q8_K rule of the k-quant extension (kquants.hip; quantize.hip K1 with K8 = true: one scale per 256
// elements, iscale = -128 / the first element of largest magnitude, q = min(127, nearest(iscale x))): a wave consumes HALF a super-block at four
// places of a chunk, so the scales of all (column, super-block) pairs are computed once per workgroup into LDS ahead of the items -- behind the
// first item's loads, like the rms_norm prologue's row scale -- and the wave-private quantization reads them.  K <= 32768 (128 super-blocks).
constexpr int GV_K8_SB = 128;
#define GVF_BODY gemv_fused_body
#define GVF_WG_PARAMS
#define GVF_WG blockIdx.x
#define GVF_NWG gridDim.x
#include "gemv_fused_body.inc"
#undef GVF_BODY
#undef GVF_WG_PARAMS
#undef GVF_WG
#undef GVF_NWG
// the same text with the workgroup index handed in: the by-id mat-vec's body (gemv_fused_byid_kernel below)
#define GVF_BODY gemv_fused_body_byid
#define GVF_WG_PARAMS , unsigned wg_in, unsigned nwg_in
#define GVF_WG wg_in
#define GVF_NWG nwg_in
#include "gemv_fused_body.inc"
#undef GVF_BODY
#undef GVF_WG_PARAMS
#undef GVF_WG
#undef GVF_NWG

// one weight matrix: the arguments as they always were (the set of one is built in registers; a kernel that takes the whole
// mv_set in its argument segment ran the single-matrix call 5 % slower: 4096 x 4096 4.60 -> 4.85 us)
template <int TYPE, int NC, int GV_ROWS, bool SC, bool PRO = false, bool K8 = false>
__global__ __launch_bounds__(GV_THREADS, (NC <= 2 && !PRO ? 4 : 2)) void gemv_fused_kernel(   // two resident workgroups per CU up to 2 columns (4 columns: 133 registers, spills under 128)
    const uint8_t *__restrict__ qs, const uint32_t *__restrict__ gs, const float *__restrict__ x, int64_t ld1, float *__restrict__ dst,
    int64_t M, int64_t Mpad, int64_t nbk, int64_t ldd, int N, int ntiles, const mm_epilogue ep, const mm_prologue pro) {
    mv_set ws;
    ws.n = 1; ws.qs[0] = qs; ws.gs[0] = gs; ws.dst[0] = dst; ws.M[0] = M; ws.Mpad[0] = Mpad; ws.ldd[0] = ldd;
    gemv_fused_body<TYPE, NC, GV_ROWS, SC, PRO, false, K8>(ws, x, ld1, nbk, N, ntiles, ep, pro);
}
// several weight matrices behind one activation matrix (common.h mv_set)
template <int TYPE, int NC, int GV_ROWS, bool SC, bool PRO>
__global__ __launch_bounds__(GV_THREADS, (NC <= 2 && !PRO ? 4 : 2)) void gemv_fused_multi_kernel(
    const mv_set ws, const float *__restrict__ x, int64_t ld1, int64_t nbk, int N, int ntiles, const mm_prologue pro) {
    const mm_epilogue ep{0, nullptr, 0, nullptr, 0, 1.0f};
    gemv_fused_body<TYPE, NC, GV_ROWS, SC, PRO, true>(ws, x, ld1, nbk, N, ntiles, ep, pro);
}

// The by-id mat-vec (ggml_hip_mul_mat_id_dev, route 1): pair p = blockIdx.x / wpp, its workgroup wg = blockIdx.x % wpp of wpp.  The workgroup reads
// ids[p] ONCE, checks it against the set FIRST -- an id outside [0, n_expert) stores the pair's rows as +0.0f and returns: no table entry is
// read and no address formed from it -- then takes the expert's operand plane and side image from the set's table and runs the fused
// mat-vec's body for ONE src1 row on the tiles wg, wg + wpp, ...: block -> lane assignment, chunking, the Q8_K scale prologue and the
// reduction are the single-matrix kernel's own, so pair p's outputs are the bits of ggml_hip_mul_mat_dev(expert ids[p], its row, N = 1).
template <int TYPE, int GV_ROWS, bool SC, bool K8>
__global__ __launch_bounds__(GV_THREADS, 4) void gemv_fused_byid_kernel(
    const moe_expert *__restrict__ tab, int n_expert, const int32_t *__restrict__ ids, int n_used, unsigned wpp, const float *__restrict__ x,
    int64_t ld1_token, int64_t ld1_slot, float *__restrict__ dst, int64_t M, int64_t Mpad, int64_t nbk, int64_t ldd, int ntiles) {
    const unsigned pair = blockIdx.x / wpp, wg = blockIdx.x - pair * wpp;
    const int id = ids[pair];
    float *const out = dst + (int64_t)pair * ldd;
    if (id < 0 || id >= n_expert) {
        for (int64_t m = (int64_t)wg * GV_THREADS + threadIdx.x; m < M; m += (int64_t)wpp * GV_THREADS) out[m] = 0.0f;
        return;
    }
    const moe_expert ex = tab[id];
    mv_set ws;
    ws.n = 1; ws.qs[0] = ex.qs; ws.gs[0] = ex.gs; ws.dst[0] = out; ws.M[0] = M; ws.Mpad[0] = Mpad; ws.ldd[0] = ldd;
    const float *xr = x + (int64_t)(pair / (unsigned)n_used) * ld1_token + (int64_t)(pair % (unsigned)n_used) * ld1_slot;
    const mm_epilogue ep{0, nullptr, 0, nullptr, 0, 1.0f};
    const mm_prologue pro{nullptr, 0, nullptr, nullptr};
    gemv_fused_body_byid<TYPE, 1, GV_ROWS, SC, false, false, K8>(ws, xr, 0, nbk, 1, ntiles, ep, pro, wg, wpp);
}

template <int TYPE, bool FUSED, int ROWS>
hipError_t launch_rows(const ggml_hip_weight *w, const float *x, int64_t ld1, act_planes p, int64_t N, float *dst,
                       int64_t ldd, hipStream_t st, const mm_epilogue *epp, const mm_prologue *pro) {
    const mm_epilogue ep = epilogue_or_none(epp);
    const int ntiles = (int)((w->M + ROWS - 1) / ROWS);
    dim3 grid((unsigned)(ntiles < GV_MAX_WGS ? ntiles : GV_MAX_WGS));
    if constexpr (FUSED && !GV_OLD_FUSED) {
        if ((N <= 1 || N >= 3) && w->nbk <= GV_CHUNK && ntiles > GV_PF_WGS) grid = dim3((unsigned)GV_PF_WGS);
        // up to 4 columns; 5..8 stay on the block-staged kernel below (118 registers = two resident workgroups per CU; the
        // wave-private form needs 146 there: 32000 x 4096 x 8 41.9 against 48.5 us)
        if (N <= 4) {
#define GVF_ARGS (TYPE == GV_TYPE_I8X2 ? w->i8p : w->qs), w->gs, x, ld1, dst, w->M, w->Mpad, w->nbk, ldd, (int)N, ntiles, ep
#define GVF_LAUNCH(NC) do { \
        if (w->ext_type != 0) {                 /* a k-quant weight (planar Q5_1 form): activations by the Q8_K rule */ \
            if constexpr (TYPE == GGML_TYPE_Q5_1 || TYPE == GV_TYPE_I8X2) { \
                if (pro || ep.mode != 0 || w->nbk % 8 != 0 || w->nbk / 8 > GV_K8_SB || (TYPE == GV_TYPE_I8X2 && !w->i8p)) return hipErrorNotSupported; \
                if (w->nbk <= GV_CHUNK) gemv_fused_kernel<TYPE, NC, ROWS, true, false, true><<<grid, GV_THREADS, 0, st>>>(GVF_ARGS, mm_prologue{nullptr, 0, nullptr, nullptr}); \
                else gemv_fused_kernel<TYPE, NC, ROWS, false, false, true><<<grid, GV_THREADS, 0, st>>>(GVF_ARGS, mm_prologue{nullptr, 0, nullptr, nullptr}); \
            } else return hipErrorNotSupported; \
        } else if constexpr (TYPE == GV_TYPE_I8X2) return hipErrorNotSupported;   /* (the form exists for the k-quant extension only) */ \
        else if (pro) { \
            if (w->nbk <= GV_CHUNK) gemv_fused_kernel<TYPE, NC, ROWS, true, true><<<grid, GV_THREADS, 0, st>>>(GVF_ARGS, *pro); \
            else gemv_fused_kernel<TYPE, NC, ROWS, false, true><<<grid, GV_THREADS, 0, st>>>(GVF_ARGS, *pro); \
        } else if (w->nbk <= GV_CHUNK) gemv_fused_kernel<TYPE, NC, ROWS, true><<<grid, GV_THREADS, 0, st>>>(GVF_ARGS, mm_prologue{nullptr, 0, nullptr, nullptr}); \
        else gemv_fused_kernel<TYPE, NC, ROWS, false><<<grid, GV_THREADS, 0, st>>>(GVF_ARGS, mm_prologue{nullptr, 0, nullptr, nullptr}); } while (0)
            if (N <= 1) GVF_LAUNCH(1);
            else if (N <= 2) GVF_LAUNCH(2);
            else GVF_LAUNCH(4);
#undef GVF_LAUNCH
#undef GVF_ARGS
            return hipGetLastError();
        }
    }
    if (ep.mode != 0 || pro) return hipErrorNotSupported;          // (callers ask gemv_fused_has_epilogue first)
    if (FUSED && w->ext_type != 0) return hipErrorNotSupported;           // (the block-staged fused form quantizes by the Q8_0 rule: plan.cpp keeps k-quants off it)
#define GV_LAUNCH(NC) gemv_q_kernel<TYPE, NC, FUSED, ROWS><<<grid, GV_THREADS, 0, st>>>((TYPE == GV_TYPE_I8X2 ? w->i8p : w->qs), w->gs, x, ld1, p.a8, p.ad, p.as, dst, w->M, w->Mpad, p.Npad, w->nbk, ldd, (int)N, ntiles)
    if (N <= 1) GV_LAUNCH(1);
    else if (N <= 2) GV_LAUNCH(2);
    else if (N <= 4) GV_LAUNCH(4);
    else if (N <= 8) GV_LAUNCH(8);
    else if constexpr (!FUSED) GV_LAUNCH(16);   // 9..16 rows: the weights are still streamed once, 16 dot products per block
#undef GV_LAUNCH
    return hipGetLastError();
}

template <int TYPE, bool FUSED>
hipError_t launch_typed(const ggml_hip_weight *w, const float *x, int64_t ld1, act_planes p, int64_t N, float *dst,
                        int64_t ldd, hipStream_t st, const mm_epilogue *ep, const mm_prologue *pro) {
    // 32 rows per workgroup measured 5 % faster at M = 32000 (4.46 vs 4.24 TB/s) and 13 % slower at M = 4096; a choice by
    // M would change the summation tree between a row shard and the unsplit matrix, and the multi-GPU path promises
    // bit-identical results for any split -- so one shape for every M.
    return launch_rows<TYPE, FUSED, 16>(w, x, ld1, p, N, dst, ldd, st, ep, pro);
}

template <bool FUSED>
hipError_t launch_any(const ggml_hip_weight *w, const float *x, int64_t ld1, act_planes p, int64_t N, float *dst,
                      int64_t ldd, hipStream_t st, const mm_epilogue *ep, const mm_prologue *pro) {
    if (N <= 0 || w->M <= 0) return hipSuccess;
    if (N > (FUSED ? GEMV_MAX_N : GEMV_WIDE_MAX_N)) return hipErrorInvalidValue;
    switch (w->type) {
    case GGML_TYPE_Q4_0: return launch_typed<GGML_TYPE_Q4_0, FUSED>(w, x, ld1, p, N, dst, ldd, st, ep, pro);
    case GGML_TYPE_Q4_1: return launch_typed<GGML_TYPE_Q4_1, FUSED>(w, x, ld1, p, N, dst, ldd, st, ep, pro);
    case GGML_TYPE_Q5_0: return launch_typed<GGML_TYPE_Q5_0, FUSED>(w, x, ld1, p, N, dst, ldd, st, ep, pro);
    case GGML_TYPE_Q4_2:
        if (w->ext_type != 0) return w->i8p ? launch_typed<GV_TYPE_I8X2, FUSED>(w, x, ld1, p, N, dst, ldd, st, ep, pro) : hipErrorInvalidValue;   // (Q6_K: int8 planes)
        return launch_typed<GGML_TYPE_Q4_2, FUSED>(w, x, ld1, p, N, dst, ldd, st, ep, pro);
    case GGML_TYPE_Q5_1: return launch_typed<GGML_TYPE_Q5_1, FUSED>(w, x, ld1, p, N, dst, ldd, st, ep, pro);
    case GGML_TYPE_Q8_0: return launch_typed<GGML_TYPE_Q8_0, FUSED>(w, x, ld1, p, N, dst, ldd, st, ep, pro);
    default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_gemv_q(const ggml_hip_weight *w, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st) {
    return launch_any<false>(w, nullptr, 0, p, N, dst, ldd, st, nullptr, nullptr);
}

hipError_t launch_gemv_q_fused(const ggml_hip_weight *w, const float *x, int64_t ld1, int64_t N, float *dst, int64_t ldd,
                               hipStream_t st, const mm_epilogue *ep) {
    act_planes none = {nullptr, nullptr, nullptr, 0};
    return launch_any<true>(w, x, ld1, none, N, dst, ldd, st, ep, nullptr);
}

namespace {
// A pair's workgroups follow the single-matrix caps -- every row tile its own workgroup up to GV_MAX_WGS, GV_PF_WGS for the look-ahead form
// (K in one chunk) -- and the whole launch is held to ONE such grid: 32 pairs of tall experts are 256 / 512 workgroups that walk their pair's
// tiles round-robin, not 32 grids on top of each other.  More pairs than that: one workgroup per pair.
template <int TYPE>
hipError_t launch_byid_typed(const ggml_hip_weight *w0, const moe_expert *tab, int n_expert, const int32_t *ids, int64_t npairs, int n_used, const float *x,
                             int64_t ld1_token, int64_t ld1_slot, float *dst, int64_t ldd, hipStream_t st) {
    const int ntiles = (int)((w0->M + 15) / 16);
    const bool sc = w0->nbk <= GV_CHUNK, k8 = w0->ext_type != 0;
    const int64_t cap = sc ? GV_PF_WGS : GV_MAX_WGS;
    int64_t wpp = cap / npairs;
    wpp = wpp < 1 ? 1 : wpp > ntiles ? ntiles : wpp;
    const dim3 grid((unsigned)(npairs * wpp));
#define GVI(SC, K8) gemv_fused_byid_kernel<TYPE, 16, SC, K8><<<grid, GV_THREADS, 0, st>>>(tab, n_expert, ids, n_used, (unsigned)wpp, x, ld1_token, ld1_slot, dst, \
                                                                                          w0->M, w0->Mpad, w0->nbk, ldd, ntiles)
    if constexpr (TYPE == GGML_TYPE_Q5_1 || TYPE == GV_TYPE_I8X2) {
        if (k8) {                                   // a k-quant weight: activations by the Q8_K rule (launch_rows has the same bounds)
            if (w0->nbk % 8 != 0 || w0->nbk / 8 > GV_K8_SB) return hipErrorNotSupported;
            if (sc) GVI(true, true); else GVI(false, true);
            return hipGetLastError();
        }
    }
    if constexpr (TYPE == GV_TYPE_I8X2) return hipErrorNotSupported;   // (the form exists for the k-quant extension only)
    else {
        if (k8) return hipErrorNotSupported;
        if (sc) GVI(true, false); else GVI(false, false);
        return hipGetLastError();
    }
#undef GVI
}
}  // namespace

hipError_t launch_gemv_q_fused_byid(const ggml_hip_weight *w0, const moe_expert *tab, int n_expert, const int32_t *ids, int64_t npairs, int n_used,
                                    const float *x, int64_t ld1_token, int64_t ld1_slot, float *dst, int64_t ldd, hipStream_t st) {
    if (npairs <= 0 || w0->M <= 0) return hipSuccess;
    if (GV_OLD_FUSED || n_used < 1 || npairs > (int64_t)1 << 28) return hipErrorNotSupported;
#define GVB(T) launch_byid_typed<T>(w0, tab, n_expert, ids, npairs, n_used, x, ld1_token, ld1_slot, dst, ldd, st)
    switch (w0->type) {
    case GGML_TYPE_Q4_0: return GVB(GGML_TYPE_Q4_0);
    case GGML_TYPE_Q4_1: return GVB(GGML_TYPE_Q4_1);
    case GGML_TYPE_Q5_0: return GVB(GGML_TYPE_Q5_0);
    case GGML_TYPE_Q4_2:
        if (w0->ext_type != 0) return w0->i8p ? GVB(GV_TYPE_I8X2) : hipErrorInvalidValue;   // (Q6_K and the types in its form: int8 planes)
        return GVB(GGML_TYPE_Q4_2);
    case GGML_TYPE_Q5_1: return GVB(GGML_TYPE_Q5_1);
    case GGML_TYPE_Q8_0: return GVB(GGML_TYPE_Q8_0);
    default: return hipErrorInvalidValue;
    }
#undef GVB
}

namespace {
template <int TYPE>
hipError_t launch_multi_typed(const mv_set &ws, const float *x, int64_t ld1, const mm_prologue *pro, int64_t nbk, int64_t N, int ntiles, hipStream_t st) {
    const mm_prologue none{nullptr, 0, nullptr, nullptr};
    const bool sc = nbk <= GV_CHUNK;
    const int cap = ((N <= 1 || N >= 3) && sc) ? GV_PF_WGS : GV_MAX_WGS;
    dim3 grid((unsigned)(ntiles < cap ? ntiles : cap));
#define GVM(NC) do { \
        if (pro) { if (sc) gemv_fused_multi_kernel<TYPE, NC, 16, true, true><<<grid, GV_THREADS, 0, st>>>(ws, x, ld1, nbk, (int)N, ntiles, *pro); \
                   else gemv_fused_multi_kernel<TYPE, NC, 16, false, true><<<grid, GV_THREADS, 0, st>>>(ws, x, ld1, nbk, (int)N, ntiles, *pro); } \
        else if (sc) gemv_fused_multi_kernel<TYPE, NC, 16, true, false><<<grid, GV_THREADS, 0, st>>>(ws, x, ld1, nbk, (int)N, ntiles, none); \
        else gemv_fused_multi_kernel<TYPE, NC, 16, false, false><<<grid, GV_THREADS, 0, st>>>(ws, x, ld1, nbk, (int)N, ntiles, none); } while (0)
    if (N <= 1) GVM(1);
    else if (N <= 2) GVM(2);
    else GVM(4);
#undef GVM
    return hipGetLastError();
}
}  // namespace

hipError_t launch_gemv_q_fused_multi(const ggml_hip_weight *const *w, int n_w, const float *x, int64_t ld1, const mm_prologue *pro, int64_t N,
                                     float *const *dst, const int64_t *ldd, hipStream_t st) {
    if (n_w < 1 || n_w > 4 || N < 1 || N > 4 || GV_OLD_FUSED) return hipErrorNotSupported;
    mv_set ws;
    memset(&ws, 0, sizeof ws);
    ws.n = n_w;
    int ntiles = 0;
    for (int i = 0; i < 4; ++i) {
        if (i < n_w) {
            if (w[i]->type != w[0]->type || w[i]->nbk != w[0]->nbk || w[i]->M <= 0) return hipErrorInvalidValue;
            ntiles += (int)((w[i]->M + 15) / 16);
            ws.qs[i] = w[i]->qs; ws.gs[i] = w[i]->gs; ws.dst[i] = dst[i]; ws.M[i] = w[i]->M; ws.Mpad[i] = w[i]->Mpad; ws.ldd[i] = ldd[i];
        }
        ws.tile_end[i] = ntiles;
    }
    switch (w[0]->type) {
    case GGML_TYPE_Q4_0: return launch_multi_typed<GGML_TYPE_Q4_0>(ws, x, ld1, pro, w[0]->nbk, N, ntiles, st);
    case GGML_TYPE_Q4_1: return launch_multi_typed<GGML_TYPE_Q4_1>(ws, x, ld1, pro, w[0]->nbk, N, ntiles, st);
    case GGML_TYPE_Q5_0: return launch_multi_typed<GGML_TYPE_Q5_0>(ws, x, ld1, pro, w[0]->nbk, N, ntiles, st);
    case GGML_TYPE_Q4_2: return launch_multi_typed<GGML_TYPE_Q4_2>(ws, x, ld1, pro, w[0]->nbk, N, ntiles, st);
    case GGML_TYPE_Q5_1: return launch_multi_typed<GGML_TYPE_Q5_1>(ws, x, ld1, pro, w[0]->nbk, N, ntiles, st);
    case GGML_TYPE_Q8_0: return launch_multi_typed<GGML_TYPE_Q8_0>(ws, x, ld1, pro, w[0]->nbk, N, ntiles, st);
    default: return hipErrorInvalidValue;
    }
}

bool gemv_fused_has_epilogue(int64_t N) { return N >= 1 && N <= 4 && !GV_OLD_FUSED; }

hipError_t launch_gemv_q_fused_pro(const ggml_hip_weight *w, const float *x, int64_t ld1, const mm_prologue &pro, int64_t N, float *dst,
                                   int64_t ldd, hipStream_t st, const mm_epilogue *ep) {
    if (!gemv_fused_has_epilogue(N)) return hipErrorNotSupported;
    act_planes none = {nullptr, nullptr, nullptr, 0};
    return launch_any<true>(w, x, ld1, none, N, dst, ldd, st, ep, &pro);
}
