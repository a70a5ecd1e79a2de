// rope.hip -- the rotary position embedding of Q / K rows on the device (include/ggml_hip_ext.h ggml_hip_rope_dev), and the same rotation
// fused with the store into an F16 or Q8_0 KV cache (ggml_hip_rope_kv_store_dev); rope.cpp has the C-ABI and the per-pair constants.
// Upstream's ggml_rope_ext in its NORMAL (pairs 2i, 2i+1) and NEOX (pairs i, i + n_dims/2) modes; an EXTENSION like attention.
//
// Pair i < n_dims / 2 of the token at position pos:
//     theta = (double)pos * eff[i]   [/ (double)freq_factors[i]]        eff and mscale: the host's table (rope_table), passed by value
//     c = (float)(cos(theta) * mscale),  s = (float)(sin(theta) * mscale)                  binary64 cos / sin, ONE rounding to f32 each
//     y0 = x0 * c - x1 * s,  y1 = x0 * s + x1 * c           every f32 operation rounds once (the library is built without contraction)
// Elements n_dims .. D-1 of a row are copied bit for bit.
//
// Both kernels: a workgroup (256 threads) serves `tpb` consecutive tokens (1, or up to 8 where n_head * D is small).  Its first threads
// compute the (c, s) of every pair of its tokens ONCE into LDS -- the binary64 work is shared by all heads of a token, which is why the
// workgroup is a token and not a flat element grid -- and after one barrier all threads walk the rows of all heads.  (c, s) depends on
// (pos, i) alone, so a row's bits depend on nothing else: not on n_head, the strides, n_tokens, tpb, or where pos came from.
//
// rope_kernel<MODE, VEC>: VEC (n_dims % 8 == 0): an item is four pairs -- NORMAL: the two float4 at 8j and 8j + 4; NEOX: the float4 at 4j
// and its partner at 4j + n_dims/2 -- read whole, rotated, written back to the same places, then one float4 per item of the tail.  A thread
// always owns whole pairs and reads both halves before it writes either: in place (dst == x) is safe in both modes.  !VEC: an item is one
// pair, then one tail element; the same bits.
//
// rope_kv_store_kernel<Q8, MODE>: as kv_store_kernel, one thread per 32 (Q8_0) or 4 (F16) elements of the ROTATED row, which never goes to
// memory: a thread computes its elements from its own x values and their partners' (NEOX: the float4 n_dims/2 away; a partner is read,
// never written, so no thread waits for another) and packs them with kv_pack.h -- bit for bit rope_kernel into a temporary, then
// kv_store_kernel.  The rope position IS the cache position p0 + t; a row whose position is outside [0, n_pos_max) leaves before any
// address is formed from it.
//
// rope_kv_store_paged_kernel<Q8, MODE>: the same into a PAGED cache (common.h kv_pages; ggml_hip_rope_kv_store_paged_dev): token (b, t) of
// n_seq * n_q rows sits at len[b] + t, its rope position and, through the sequence's table row, its page row.  rope_store_unit is the
// rotate-and-pack both store kernels share, so the bytes are rope_kernel's then kv_store_paged_kernel's.  A position outside [0, n_kv_max)
// leaves before the table is read, a page id outside [0, n_pages) before any address is formed from it.
// rope_kv_store_paged_ragged_kernel<Q8, MODE>: the same body (rope_kv_store_paged_body) over the packed rows of a RAGGED batch (common.h kv_ragged;
// ggml_hip_rope_kv_store_paged_ragged_dev): the row's sequence and its index in it come from a bisection of q_start instead of t / n_q, t % n_q; a row of
// no present sequence writes nothing.
// No scratch, no atomics; LDS: 8 tokens x 128 pairs x 8 bytes.
#include "common.h"
#include "plan.h"        // ATTN_CHUNK: a page of the paged cache
#include "kv_pack.h"

namespace {

constexpr int ROPE_TPB_MAX = 8;
constexpr int ROPE_PAGE = ATTN_CHUNK;                               // positions per page of a paged cache: attention's chunk

__device__ __forceinline__ void rope_rot(float x0, float x1, float2 cs, float &y0, float &y1) {
    y0 = x0 * cs.x - x1 * cs.y;
    y1 = x0 * cs.y + x1 * cs.x;
}

// (c, s) of every pair of the workgroup's tokens -> cs[token in the workgroup][pair]; ends in the barrier.  pos_of(t): the position of token t
template <class POS>
__device__ __forceinline__ void rope_stage_cs(float2 *cs, const rope_table &tab, int half, int tpb, int64_t t0, int64_t n_tokens, POS pos_of, const float *ff) {
    for (int idx = threadIdx.x; idx < tpb * half; idx += 256) {
        const int tt = idx / half, i = idx - tt * half;
        const int64_t t = t0 + tt;
        if (t >= n_tokens) break;
        const int64_t pos = pos_of(t);
        double theta = (double)pos * tab.eff[i];
        if (ff) theta = theta / (double)ff[i];
        cs[idx] = make_float2((float)(cos(theta) * tab.mscale), (float)(sin(theta) * tab.mscale));
    }
    __syncthreads();
}

template <int MODE, bool VEC>
__global__ __launch_bounds__(256) void rope_kernel(const rope_table tab, const float *x, int64_t ldx_tok, int64_t ldx_head, int n_head, int D, int n_dims,
                                                   int64_t n_tokens, int tpb, const int32_t *__restrict__ d_pos, int64_t pos0,
                                                   const int32_t *__restrict__ d_pos0, const float *__restrict__ ff, float *dst, int64_t ldd_tok,
                                                   int64_t ldd_head, int copy_tail) {
    __shared__ __align__(16) float2 cs[ROPE_TPB_MAX * ROPE_MAX_PAIRS];
    const int half = n_dims / 2;
    const int64_t t0 = (int64_t)blockIdx.x * tpb;
    const int64_t p0 = d_pos0 ? (int64_t)*d_pos0 : pos0;
    rope_stage_cs(cs, tab, half, tpb, t0, n_tokens, [=](int64_t t) { return d_pos ? (int64_t)d_pos[t] : p0 + t; }, ff);
    const int rot = VEC ? half / 4 : half;
    const int per_head = rot + (copy_tail ? (VEC ? (D - n_dims) / 4 : D - n_dims) : 0);
    const int per_tok = n_head * per_head;
    for (int idx = threadIdx.x; idx < tpb * per_tok; idx += 256) {
        const int tt = idx / per_tok, r = idx - tt * per_tok;
        const int h = r / per_head, j = r - h * per_head;
        const int64_t t = t0 + tt;
        if (t >= n_tokens) break;
        const float *xr = x + t * ldx_tok + (int64_t)h * ldx_head;
        float *yr = dst + t * ldd_tok + (int64_t)h * ldd_head;
        const float2 *c = cs + tt * half;
        if (j >= rot) {                                             // the tail
            if constexpr (VEC) { const int e = n_dims + 4 * (j - rot); *(float4 *)(yr + e) = *(const float4 *)(xr + e); }
            else { const int e = n_dims + (j - rot); yr[e] = xr[e]; }
            continue;
        }
        if constexpr (VEC) {
            const int ea = MODE == 0 ? 8 * j : 4 * j, eb = MODE == 0 ? 8 * j + 4 : 4 * j + half;
            const float4 a = *(const float4 *)(xr + ea), b = *(const float4 *)(xr + eb);
            const float4 c01 = *(const float4 *)(c + 4 * j), c23 = *(const float4 *)(c + 4 * j + 2);
            const float2 c0 = make_float2(c01.x, c01.y), c1 = make_float2(c01.z, c01.w), c2 = make_float2(c23.x, c23.y), c3 = make_float2(c23.z, c23.w);
            float4 ya, yb;
            if constexpr (MODE == 0) {
                rope_rot(a.x, a.y, c0, ya.x, ya.y); rope_rot(a.z, a.w, c1, ya.z, ya.w);
                rope_rot(b.x, b.y, c2, yb.x, yb.y); rope_rot(b.z, b.w, c3, yb.z, yb.w);
            } else {
                rope_rot(a.x, b.x, c0, ya.x, yb.x); rope_rot(a.y, b.y, c1, ya.y, yb.y);
                rope_rot(a.z, b.z, c2, ya.z, yb.z); rope_rot(a.w, b.w, c3, ya.w, yb.w);
            }
            *(float4 *)(yr + ea) = ya;
            *(float4 *)(yr + eb) = yb;
        } else {
            const int e0 = MODE == 0 ? 2 * j : j, e1 = MODE == 0 ? 2 * j + 1 : j + half;
            const float x0 = xr[e0], x1 = xr[e1];
            float y0, y1;
            rope_rot(x0, x1, c[j], y0, y1);
            yr[e0] = y0;
            yr[e1] = y1;
        }
    }
}

// element e of the rotated row, one element at a time
template <int MODE>
__device__ __forceinline__ float rope_rotated1(const float *__restrict__ xr, int e, int n_dims, const float2 *c) {
    if (e >= n_dims) return xr[e];
    const int half = n_dims / 2;
    float y0, y1;
    if constexpr (MODE == 0) {
        rope_rot(xr[e & ~1], xr[e | 1], c[e >> 1], y0, y1);
        return (e & 1) ? y1 : y0;
    } else {
        const int i = e < half ? e : e - half;
        rope_rot(xr[i], xr[i + half], c[i], y0, y1);
        return e < half ? y0 : y1;
    }
}

// elements e .. e + 3 (e % 4 == 0) of the rotated row; vec (n_dims % 8 == 0): by float4, the group is wholly tail, low half or high half
template <int MODE>
__device__ __forceinline__ float4 rope_rotated4(const float *__restrict__ xr, int e, int n_dims, const float2 *c, bool vec) {
    if (!vec) return make_float4(rope_rotated1<MODE>(xr, e, n_dims, c), rope_rotated1<MODE>(xr, e + 1, n_dims, c), rope_rotated1<MODE>(xr, e + 2, n_dims, c),
                                 rope_rotated1<MODE>(xr, e + 3, n_dims, c));
    const float4 own = *(const float4 *)(xr + e);
    if (e >= n_dims) return own;
    float4 y;
    float o;                                                        // (the other element of each pair: computed, not kept)
    if constexpr (MODE == 0) {
        rope_rot(own.x, own.y, c[e / 2], y.x, y.y);
        rope_rot(own.z, own.w, c[e / 2 + 1], y.z, y.w);
    } else {
        const int half = n_dims / 2;
        if (e < half) {
            const float4 p = *(const float4 *)(xr + e + half);
            rope_rot(own.x, p.x, c[e], y.x, o); rope_rot(own.y, p.y, c[e + 1], y.y, o);
            rope_rot(own.z, p.z, c[e + 2], y.z, o); rope_rot(own.w, p.w, c[e + 3], y.w, o);
        } else {
            const int i = e - half;
            const float4 p = *(const float4 *)(xr + i);
            rope_rot(p.x, own.x, c[i], o, y.x); rope_rot(p.y, own.y, c[i + 1], o, y.y);
            rope_rot(p.z, own.z, c[i + 2], o, y.z); rope_rot(p.w, own.w, c[i + 3], o, y.w);
        }
    }
    return y;
}

// unit u (32 elements of a Q8_0 row, 4 of an F16 row) of the rotated row xr -> its bytes in the cache row `row`
template <bool Q8, int MODE>
__device__ __forceinline__ void rope_store_unit(const float *__restrict__ xr, uint8_t *__restrict__ row, int u, int n_dims, const float2 *c, bool vec) {
    if constexpr (Q8) {
        float v[QK];
#pragma unroll
        for (int k = 0; k < 8; ++k) {
            const float4 f = rope_rotated4<MODE>(xr, QK * u + 4 * k, n_dims, c, vec);
            v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w;
        }
        kv_pack_q8_0(v, (uint32_t *)(row + 36 * (int64_t)u));
    } else {
        *(uint2 *)(row + 8 * (int64_t)u) = kv_pack_f16(rope_rotated4<MODE>(xr, 4 * u, n_dims, c, vec));
    }
}

template <bool Q8, int MODE>
__global__ __launch_bounds__(256) void rope_kv_store_kernel(const rope_table tab, const float *__restrict__ x, int64_t ldx_tok, int64_t ldx_head, int n_head_kv,
                                                            int D, int n_dims, int64_t n_tokens, int tpb, int64_t pos0, const int32_t *__restrict__ d_pos0,
                                                            const float *__restrict__ ff, uint8_t *__restrict__ cache, int64_t nb_pos, int64_t nb_head,
                                                            int64_t n_pos_max) {
    __shared__ __align__(16) float2 cs[ROPE_TPB_MAX * ROPE_MAX_PAIRS];
    const int half = n_dims / 2;
    const int64_t t0 = (int64_t)blockIdx.x * tpb;
    const int64_t p0 = d_pos0 ? (int64_t)*d_pos0 : pos0;
    rope_stage_cs(cs, tab, half, tpb, t0, n_tokens, [=](int64_t t) { return p0 + t; }, ff);
    const bool vec = n_dims % 8 == 0;
    const int per_head = D / (Q8 ? QK : 4);
    const int per_tok = n_head_kv * per_head;
    for (int idx = threadIdx.x; idx < tpb * per_tok; idx += 256) {
        const int tt = idx / per_tok, r = idx - tt * per_tok;
        const int h = r / per_head, u = r - h * per_head;
        const int64_t t = t0 + tt;
        if (t >= n_tokens) break;
        const int64_t pos = p0 + t;
        if (pos < 0 || pos >= n_pos_max) continue;                  // (before any address is formed from it)
        rope_store_unit<Q8, MODE>(x + t * ldx_tok + (int64_t)h * ldx_head, cache + pos * nb_pos + (int64_t)h * nb_head, u, n_dims, cs + tt * half, vec);
    }
}

// The same into a PAGED cache (common.h kv_pages): token (b, t') = (t / n_q, t % n_q) of the n_seq * n_q rows sits at position
// len[b] + t', which is its rope position and, through the sequence's table row, its page row.  Every guard stands in front of the address
// it protects: the table is read only for a position inside [0, n_kv_max), the pool addressed only with a page id inside [0, n_pages).
// where(t, &b): the position of packed row t and its sequence b (whose table row names its page); a negative position writes nothing
template <bool Q8, int MODE, class WHERE>
__device__ __forceinline__ void rope_kv_store_paged_body(float2 *cs, const rope_table &tab, const float *__restrict__ x, int64_t ldx_tok, int64_t ldx_head,
                                                         int n_head_kv, int D, int n_dims, int64_t n_tokens, int tpb, WHERE where, const float *__restrict__ ff,
                                                         uint8_t *__restrict__ pool, int64_t nb_pos, int64_t nb_head, const kv_pages &pg) {
    const int half = n_dims / 2;
    const int64_t t0 = (int64_t)blockIdx.x * tpb;
    rope_stage_cs(cs, tab, half, tpb, t0, n_tokens, [=](int64_t t) { int64_t b; return where(t, &b); }, ff);
    const bool vec = n_dims % 8 == 0;
    const int per_head = D / (Q8 ? QK : 4);
    const int per_tok = n_head_kv * per_head;
    for (int idx = threadIdx.x; idx < tpb * per_tok; idx += 256) {
        const int tt = idx / per_tok, r = idx - tt * per_tok;
        const int h = r / per_head, u = r - h * per_head;
        const int64_t t = t0 + tt;
        if (t >= n_tokens) break;
        int64_t b;
        const int64_t pos = where(t, &b);
        if (pos < 0 || pos >= pg.n_kv_max) continue;                // (before the table is read)
        const int page = pg.pages[b * pg.ld_pages + pos / ROPE_PAGE];
        if (page < 0 || page >= pg.n_pages) continue;               // (before any address is formed from it)
        uint8_t *row = pool + (int64_t)page * pg.nb_page + (pos % ROPE_PAGE) * nb_pos + (int64_t)h * nb_head;
        rope_store_unit<Q8, MODE>(x + t * ldx_tok + (int64_t)h * ldx_head, row, u, n_dims, cs + tt * half, vec);
    }
}

template <bool Q8, int MODE>
__global__ __launch_bounds__(256) void rope_kv_store_paged_kernel(const rope_table tab, const float *__restrict__ x, int64_t ldx_tok, int64_t ldx_head,
                                                                  int n_head_kv, int D, int n_dims, int64_t n_tokens, int tpb, int n_q,
                                                                  const float *__restrict__ ff, uint8_t *__restrict__ pool, int64_t nb_pos, int64_t nb_head,
                                                                  const kv_pages pg) {
    __shared__ __align__(16) float2 cs[ROPE_TPB_MAX * ROPE_MAX_PAIRS];
    const auto where = [=](int64_t t, int64_t *b) { *b = t / n_q; return (int64_t)pg.len[*b] + (t - *b * n_q); };
    rope_kv_store_paged_body<Q8, MODE>(cs, tab, x, ldx_tok, ldx_head, n_head_kv, D, n_dims, n_tokens, tpb, where, ff, pool, nb_pos, nb_head, pg);
}

// The same over the packed rows of a RAGGED batch (common.h kv_ragged; ggml_hip_rope_kv_store_paged_ragged_dev): the row's sequence by bisection of
// q_start (ragged_find); a row of no present sequence gets position -1 (its (c, s) are computed for that number and never used) and writes nothing.
template <bool Q8, int MODE>
__global__ __launch_bounds__(256) void rope_kv_store_paged_ragged_kernel(const rope_table tab, const float *__restrict__ x, int64_t ldx_tok, int64_t ldx_head,
                                                                         int n_head_kv, int D, int n_dims, int tpb, const kv_ragged rg,
                                                                         const float *__restrict__ ff, uint8_t *__restrict__ pool, int64_t nb_pos,
                                                                         int64_t nb_head, const kv_pages pg) {
    __shared__ __align__(16) float2 cs[ROPE_TPB_MAX * ROPE_MAX_PAIRS];
    const auto where = [=](int64_t t, int64_t *b) {
        int tq;
        *b = ragged_find(rg, t, &tq);
        return *b < 0 ? (int64_t)-1 : (int64_t)pg.len[*b] + tq;
    };
    rope_kv_store_paged_body<Q8, MODE>(cs, tab, x, ldx_tok, ldx_head, n_head_kv, D, n_dims, (int64_t)rg.n_tokens_max, tpb, where, ff, pool, nb_pos, nb_head, pg);
}

// tokens per workgroup: as many as keep its 256 threads busy, at most ROPE_TPB_MAX
int rope_tpb(int64_t per_tok, int64_t n_tokens) {
    int64_t tpb = per_tok > 0 ? 256 / per_tok : 1;
    tpb = tpb < 1 ? 1 : tpb > ROPE_TPB_MAX ? ROPE_TPB_MAX : tpb;
    return (int)(tpb > n_tokens ? n_tokens : tpb);
}

}  // namespace

hipError_t launch_rope(const rope_table &tab, const rope_args &a, float *dst, int64_t ldd_tok, int64_t ldd_head, hipStream_t st) {
    if (a.n_tokens <= 0) return hipSuccess;
    const bool vec = a.n_dims % 8 == 0;
    const int copy_tail = !(dst == a.x && ldd_tok == a.ldx_tok && ldd_head == a.ldx_head);     // in place: the tail is there already
    const int64_t per_head = vec ? a.n_dims / 8 + (copy_tail ? (a.D - a.n_dims) / 4 : 0) : a.n_dims / 2 + (copy_tail ? a.D - a.n_dims : 0);
    const int tpb = rope_tpb(a.n_head * per_head, a.n_tokens);
    const int64_t blocks = (a.n_tokens + tpb - 1) / tpb;
    if (blocks > 0x7FFFFFFF || a.n_dims / 2 > ROPE_MAX_PAIRS) return hipErrorInvalidValue;
#define ROPE(M, V)                                                                                                                                    \
    rope_kernel<M, V><<<dim3((unsigned)blocks), 256, 0, st>>>(tab, a.x, a.ldx_tok, a.ldx_head, a.n_head, a.D, a.n_dims, a.n_tokens, tpb, a.d_pos, a.pos0, \
                                                             a.d_pos0, a.freq_factors, dst, ldd_tok, ldd_head, copy_tail)
    if (a.mode == 0 && vec) ROPE(0, true);
    else if (a.mode == 0) ROPE(0, false);
    else if (vec) ROPE(2, true);
    else ROPE(2, false);
#undef ROPE
    return hipGetLastError();
}

hipError_t launch_rope_kv_store(const rope_table &tab, const rope_args &a, int kv_type, void *cache, int64_t nb_pos, int64_t nb_head, int64_t n_pos_max,
                                hipStream_t st) {
    if (a.n_tokens <= 0) return hipSuccess;
    const bool q8 = kv_type == GGML_TYPE_Q8_0;
    const int tpb = rope_tpb((int64_t)a.n_head * (a.D / (q8 ? QK : 4)), a.n_tokens);
    const int64_t blocks = (a.n_tokens + tpb - 1) / tpb;
    if (blocks > 0x7FFFFFFF || a.n_dims / 2 > ROPE_MAX_PAIRS) return hipErrorInvalidValue;
#define ROPE_KV(Q, M)                                                                                                                                  \
    rope_kv_store_kernel<Q, M><<<dim3((unsigned)blocks), 256, 0, st>>>(tab, a.x, a.ldx_tok, a.ldx_head, a.n_head, a.D, a.n_dims, a.n_tokens, tpb, a.pos0,  \
                                                                      a.d_pos0, a.freq_factors, (uint8_t *)cache, nb_pos, nb_head, n_pos_max)
    if (q8 && a.mode == 0) ROPE_KV(true, 0);
    else if (q8) ROPE_KV(true, 2);
    else if (a.mode == 0) ROPE_KV(false, 0);
    else ROPE_KV(false, 2);
#undef ROPE_KV
    return hipGetLastError();
}

hipError_t launch_rope_kv_store_paged(const rope_table &tab, const rope_args &a, int kv_type, int64_t n_q, void *pool, int64_t nb_pos, int64_t nb_head,
                                      const kv_pages &pg, hipStream_t st) {
    if (a.n_tokens <= 0) return hipSuccess;
    const bool q8 = kv_type == GGML_TYPE_Q8_0;
    const int tpb = rope_tpb((int64_t)a.n_head * (a.D / (q8 ? QK : 4)), a.n_tokens);
    const int64_t blocks = (a.n_tokens + tpb - 1) / tpb;
    if (blocks > 0x7FFFFFFF || a.n_dims / 2 > ROPE_MAX_PAIRS || n_q < 1 || n_q > 0x7FFFFFFF) return hipErrorInvalidValue;
#define ROPE_KV(Q, M)                                                                                                                                  \
    rope_kv_store_paged_kernel<Q, M><<<dim3((unsigned)blocks), 256, 0, st>>>(tab, a.x, a.ldx_tok, a.ldx_head, a.n_head, a.D, a.n_dims, a.n_tokens, tpb,   \
                                                                            (int)n_q, a.freq_factors, (uint8_t *)pool, nb_pos, nb_head, pg)
    if (q8 && a.mode == 0) ROPE_KV(true, 0);
    else if (q8) ROPE_KV(true, 2);
    else if (a.mode == 0) ROPE_KV(false, 0);
    else ROPE_KV(false, 2);
#undef ROPE_KV
    return hipGetLastError();
}

hipError_t launch_rope_kv_store_paged_ragged(const rope_table &tab, const rope_args &a, int kv_type, const kv_ragged &rg, void *pool, int64_t nb_pos,
                                             int64_t nb_head, const kv_pages &pg, hipStream_t st) {
    if (a.n_tokens <= 0) return hipSuccess;
    const bool q8 = kv_type == GGML_TYPE_Q8_0;
    const int tpb = rope_tpb((int64_t)a.n_head * (a.D / (q8 ? QK : 4)), a.n_tokens);
    const int64_t blocks = (a.n_tokens + tpb - 1) / tpb;
    if (blocks > 0x7FFFFFFF || a.n_dims / 2 > ROPE_MAX_PAIRS || a.n_tokens != rg.n_tokens_max) return hipErrorInvalidValue;
#define ROPE_KV(Q, M)                                                                                                                                  \
    rope_kv_store_paged_ragged_kernel<Q, M><<<dim3((unsigned)blocks), 256, 0, st>>>(tab, a.x, a.ldx_tok, a.ldx_head, a.n_head, a.D, a.n_dims, tpb, rg,     \
                                                                                   a.freq_factors, (uint8_t *)pool, nb_pos, nb_head, pg)
    if (q8 && a.mode == 0) ROPE_KV(true, 0);
    else if (q8) ROPE_KV(true, 2);
    else if (a.mode == 0) ROPE_KV(false, 0);
    else ROPE_KV(false, 2);
#undef ROPE_KV
    return hipGetLastError();
}
