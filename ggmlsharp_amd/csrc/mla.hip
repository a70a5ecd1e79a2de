// mla.hip -- multi-head LATENT attention (MLA, absorbed form) over a latent KV cache on the f16 matrix cores, and the paged store of latent rows
// (include/ggml_hip_ext.h, section MLA, is the statement; mla.cpp has the C-ABI, plan.cpp plan_attn_mla chooses form and grid from n_q alone).
//
// A cache row is ONE position: MLA_DK = 576 elements in reference block format (F16 1152 bytes, Q8_0 18 blocks = 648 bytes) at base + j * nb_pos.
// Elements 0 .. 511 are the latent AND the value, 512 .. 575 the rotated key part.  Every query head reads the same row: a ROW of the problem is a
// pair (token t, head h), r = t * n_head + h, and all rows share the cache.  vis(t) is attn.hip's.
//
// ---- the chunk body (mla_body), shared by every kernel here ----
// A workgroup (4 waves) owns MLA_TILE = 64 consecutive rows of one sequence.  Wave w serves rows 32 (w & 1) .. + 31 and the output columns
// 256 (w >> 1) .. + 255; the two waves of a row half compute the same scores (the score is 53 % of the flops; the alternative is an exchange of P
// through LDS).  A lane owns ONE row (lane & 31), so m, l and alpha are per-lane scalars.  Q is rounded to f16 once and kept as an LDS image of the
// tile's 64 rows, read as the B operand of S^T = K Q^T (144 registers per lane of Q fragments spilled).  The positions are walked in STEPS of
// MLA_STEP = 64, two per chunk of 128 (a 128-position stage would be 147 KB of LDS):
//   stage   64 rows as ONE f16 image [position][576]; a Q8_0 row is dequantized while staged, f16((float)q * d); a position at or beyond n_kv is ZEROS
//   S^T     = K Q^T over all 576 columns, v_mfma_f32_32x32x16_f16, 36 k-steps ascending
//   s       = scale * S (f32), -inf where j >= vis;  m' = max(m, max s);  alpha = expf(m - m') (0 while m = -inf);  P = f16(expf(s - m')), 0 where invisible
//   l       = l * alpha + sum of the ROUNDED P;  O^T = O^T * alpha + V^T P^T over columns 0 .. 511
// V^T is not staged: the A operand V^T[d][position] is read from the SAME image with ds_read_b64_tr_b16 (4 positions x 16 columns per 16-lane group,
// delivered column-major).  The image is the swizzle of 256-byte rows that serves row reads and transposed reads without bank conflicts: five
// column tiles [64][128 halves], chunk ch (16 bytes) of row j at 256 j + 16 (ch ^ (((j & 3) << 2) | ((j >> 2) & 3))).  The transposed read needs
// EXEC all ones and 8-byte aligned addresses: every loop here is workgroup- or wave-uniform and every lane always has an in-image address.
// A step with no visible position of a row leaves its state as it is (alpha = 1, P = 0), so a row's bits do not depend on which other rows share
// its workgroup, hence not on n_head, n_q (within a form) or the row's place in the tile.  A masked weight is a ZERO operand: the cache must hold
// finite values below n_kv.
//
// WALK (n_q > 8): the workgroup walks steps 0 .. ceil(max vis / 64) - 1 ascending, dst = O / l (+0.0f where l == 0).  One launch, no work buffer.
// SPLIT (n_q <= 8): grid y is the SPAN, MLA_SPAN chunks = 2 MLA_SPAN steps; the workgroup runs the span's steps below its largest vis and writes the
// unnormalised (m, l, O[512]) of every row with a visible position in the span to work[(row * n_spans + span) * 516].  The merge (one workgroup of 512
// threads per row) is attn_merge_row's: M = max m_s; b_s = m_s == M ? 1 : expf(m_s - M); L, A[d] fma chains over s ascending, the first term the product.
// PAGED: grid z is the sequence; step st lies in page pages[b][st / 2] at row 64 (st & 1); the ids are scanned before the first stage (WALK: zero rows;
// SPLIT: the workgroup leaves and the merge, which scans too, writes the zeros).  Nothing else knows where a chunk lies.
#include "common.h"
#include "plan.h"
#include "kv_pack.h"

namespace {

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int C = ATTN_CHUNK, DK = MLA_DK, DV = MLA_DV, STEP = MLA_STEP, TILE = MLA_TILE, PART = DV + 4;
constexpr int NKS = DK / 16, NCT = STEP / 32, NDT = DV / 2 / 32, ROW_CH = DK / 8;      // k-steps of a score, 32-position tiles of a step, 32-column tiles of a wave, 16-byte chunks of a row
constexpr int IMG_TILE = STEP * 256;                                                  // one column tile of the image: 64 rows of 256 bytes
constexpr int IMG_BYTES = (DK + 127) / 128 * IMG_TILE;                                // 5 column tiles (the last half used): 80 KB
constexpr int STAGE_B = 6;                                                            // pieces a thread keeps in flight while staging
static_assert(STEP * ROW_CH % (256 * STAGE_B) == 0 && TILE * ROW_CH % (256 * STAGE_B) == 0, "the stage loops have no tail");
constexpr int Q_STRIDE = 2 * DK + 16;                                                 // bytes of a row of the Q image
constexpr int MLA_LDS = IMG_BYTES + TILE * Q_STRIDE;                                  // 153 KB of the CU's 160
static_assert(STEP == 64 && TILE == 64 && C % STEP == 0 && DV == 512 && DK == 576, "the wave map below is written for these");

// ---- attn.hip's definitions of vis and of the counts, restated (that file's are local to it) ----
__device__ __forceinline__ int visible(int t, int n_kv, int n_q, int causal) {
    if (!causal) return n_kv;
    const int v = n_kv - n_q + t + 1;
    return v < 0 ? 0 : v > n_kv ? n_kv : v;
}
__device__ __forceinline__ int device_count(const int32_t *d_n, int host_n, int n_max) {
    int n = d_n ? *d_n : host_n;
    n = n < 0 ? 0 : n;
    return n > n_max ? n_max : n;
}
__device__ __forceinline__ int paged_count(const kv_pages &pg, int b, int len_bias) {
    const int64_t n = (int64_t)pg.len[b] + len_bias;
    return (int)(n < 0 ? 0 : n > pg.n_kv_max ? pg.n_kv_max : n);
}
// 1 where one of the first ceil(n_kv / 128) entries of a sequence's table row lies outside [0, n_pages): the same answer in all NT threads, no address formed
template <int NT>
__device__ __forceinline__ int paged_any_invalid(const int32_t *__restrict__ row, int n_kv, int n_pages) {
    const int needed = (n_kv + C - 1) / C;
    int bad = 0;
    for (int c = threadIdx.x; c < needed; c += NT) {
        const int id = row[c];
        bad |= (id < 0 || id >= n_pages) ? 1 : 0;
    }
    return __syncthreads_or(bad);
}

// elements 8 c8 .. 8 c8 + 7 of a cache row in global memory, as f16 (attn.hip stage_load8)
template <bool Q8>
__device__ __forceinline__ f16x8 stage_load8(const uint8_t *row, int c8) {
    if constexpr (Q8) {
        const uint32_t *b = (const uint32_t *)(row + 36 * (c8 >> 2));
        const float d = __uint_as_float(b[0]);
        const uint32_t w0 = b[1 + 2 * (c8 & 3)], w1 = b[2 + 2 * (c8 & 3)];
        f16x8 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = (_Float16)((float)(int)(int8_t)((w0 >> (8 * i)) & 0xFFu) * d);       // (v_cvt_f16_f32: round to nearest even)
            o[4 + i] = (_Float16)((float)(int)(int8_t)((w1 >> (8 * i)) & 0xFFu) * d);
        }
        return o;
    } else {
        return *(const f16x8 *)(row + 16 * c8);
    }
}

// byte offset of 16-byte chunk c8 (0 .. 71) of row j (0 .. 63) of the staged image
__device__ __forceinline__ int img_off(int j, int c8) {
    return (c8 >> 4) * IMG_TILE + 256 * j + 16 * ((c8 & 15) ^ (((j & 3) << 2) | ((j >> 2) & 3)));
}

// the transposed read (ds_read_b64_tr_b16): the 16-lane group of a lane reads a block of 4 rows x 16 columns; lane i of the group supplies the address of
// block row i >> 2, columns 4 (i & 3) .. + 3, and receives column i of the block, block row q in element q
__device__ __forceinline__ f16x4 tr_read(const uint8_t *p) {
    typedef __fp16 fp16x4 __attribute__((__vector_size__(4 * sizeof(__fp16))));
    typedef __attribute__((address_space(3))) fp16x4 lds_fp16x4;
    return __builtin_bit_cast(f16x4, __builtin_amdgcn_ds_read_tr16_b64_v4f16((lds_fp16x4 *)p));
}

// THE BODY: rows R0 .. R0 + 63 of sequence-local row index (t * n_head + h) over steps [st_begin, st_end) of a sequence with n_kv positions.
// base: the contiguous cache, or the pool with pages = the sequence's table row (its needed entries checked by the caller).  On return lane (r, hh) of
// wave (rh, dh) holds, for row min(R0 + 32 rh + r, rows - 1): m, l, and O^T[256 dh + 32 dt + (i & 3) + 8 (i >> 2) + 4 hh] in o[dt][i].
template <bool Q8, bool PAGED>
__device__ __forceinline__ void mla_body(uint8_t *lds, const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, int n_head, int R0, int rows,
                                         const uint8_t *__restrict__ base, int64_t nb_pos, const int32_t *__restrict__ pages, int64_t nb_page, int n_kv, int vis,
                                         int wave_vis, int st_begin, int st_end, float scale, f32x16 (&o)[NDT], float &m, float &l) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, rh = wave & 1, dh = wave >> 1;
    // the tile's Q rows, rounded to f16 once, as an LDS image [64][576 + 8 halves] behind the stage (16-byte fragment reads, rows 4 banks apart); a row
    // past the sequence's last is a copy of the last.  Read as the B operand of S^T = K Q^T: lane (row r, half hh) takes Q[16 ks + 8 hh + i].
    uint8_t *qimg = lds + IMG_BYTES;
    for (int i0 = tid; i0 < TILE * ROW_CH; i0 += 256 * STAGE_B) {
        float4 a[STAGE_B], b[STAGE_B];
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) {
            const int i = i0 + 256 * u, rr = i / ROW_CH, c8 = i - rr * ROW_CH;
            const int R = min(R0 + rr, rows - 1), t = R / n_head, h = R - t * n_head;
            const float *qrow = q + (int64_t)t * ldq_tok + (int64_t)h * ldq_head + 8 * c8;
            a[u] = *(const float4 *)qrow; b[u] = *(const float4 *)(qrow + 4);
        }
#pragma unroll
        for (int u = 0; u < STAGE_B; ++u) {
            const int i = i0 + 256 * u, rr = i / ROW_CH, c8 = i - rr * ROW_CH;
            f16x8 v;
            v[0] = (_Float16)a[u].x; v[1] = (_Float16)a[u].y; v[2] = (_Float16)a[u].z; v[3] = (_Float16)a[u].w;
            v[4] = (_Float16)b[u].x; v[5] = (_Float16)b[u].y; v[6] = (_Float16)b[u].z; v[7] = (_Float16)b[u].w;
            *(f16x8 *)(qimg + rr * Q_STRIDE + 16 * c8) = v;
        }
    }
    const uint8_t *qfrag = qimg + (32 * rh + r) * Q_STRIDE + 16 * hh;    // (the first stage's barrier stands between these stores and the reads)
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.0f;
    const float ninf = -__builtin_inff();
    m = ninf; l = 0.0f;
    // The image offsets as sixteen lane constants plus compile-time terms (img_off's XOR taken apart):
    // row read of (tile ct, k-step ks), row 32 ct + r, chunk 2 ks + hh:      rbase[ks & 7] + (ks >> 3) * IMG_TILE + 8192 ct
    // transposed read of (dt, ct, ks, g), block rows 32 ct + 16 ks + 8 g + 4 hh .. + 3, columns 256 dh + 32 dt + 16 ((lane >> 4) & 1) .. + 15:
    //                                                                          tbase[g][dt & 3] + (2 dh + (dt >> 2)) * IMG_TILE + 256 (32 ct + 16 ks)
    int rbase[8], tbase[2][4];
    {
        const int xr = ((r & 3) << 2) | ((r >> 2) & 3);
#pragma unroll
        for (int k = 0; k < 8; ++k) rbase[k] = 256 * r + 16 * ((2 * k + hh) ^ xr);
        const int i = lane & 15, q = i >> 2, p = i & 3, h16 = (lane >> 4) & 1;
#pragma unroll
        for (int g = 0; g < 2; ++g)
#pragma unroll
            for (int d4 = 0; d4 < 4; ++d4) {
                const int x = (q << 2) | ((2 * g + hh) & 3), ch = 4 * d4 + 2 * h16 + (p >> 1);
                tbase[g][d4] = 256 * (4 * hh + 8 * g + q) + 16 * (ch ^ x) + 8 * (p & 1) + 2 * dh * IMG_TILE;
            }
    }
    for (int st = st_begin; st < st_end; ++st) {
        const int j0 = st * STEP, cnt = min(STEP, n_kv - j0);        // (j0 < the workgroup's largest vis <= n_kv: cnt >= 1)
        if (st > st_begin) __syncthreads();                          // (every wave is done with the previous stage)
        {
            const uint8_t *kb = PAGED ? base + (int64_t)pages[j0 / C] * nb_page + (int64_t)(j0 % C) * nb_pos : base + (int64_t)j0 * nb_pos;
            // (18 pieces of 16 bytes per thread, STAGE_B loads in flight at a time: one piece at a time pays the memory latency 18 times per step)
            for (int i0 = tid; i0 < STEP * ROW_CH; i0 += 256 * STAGE_B) {
                f16x8 kv[STAGE_B];
#pragma unroll
                for (int u = 0; u < STAGE_B; ++u) {
                    const int i = i0 + 256 * u, j = i / ROW_CH, c8 = i - j * ROW_CH;
                    if (j < cnt) kv[u] = stage_load8<Q8>(kb + (int64_t)j * nb_pos, c8);
                    else {
#pragma unroll
                        for (int e = 0; e < 8; ++e) kv[u][e] = (_Float16)0.0f;
                    }
                }
#pragma unroll
                for (int u = 0; u < STAGE_B; ++u) {
                    const int i = i0 + 256 * u, j = i / ROW_CH, c8 = i - j * ROW_CH;
                    *(f16x8 *)(lds + img_off(j, c8)) = kv[u];
                }
            }
        }
        __syncthreads();
        if (j0 >= wave_vis) continue;                                // (wave-uniform: nothing of this step is visible to the wave's rows)
        // ---- S^T = K Q^T: tile ct holds positions j0 + 32 ct + (i & 3) + 8 (i >> 2) + 4 hh of this lane's row ----
        f32x16 s[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[ct][i] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const f16x8 a = *(const f16x8 *)(lds + rbase[ks & 7] + (ks >> 3) * IMG_TILE + 8192 * ct);
                s[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, *(const f16x8 *)(qfrag + 32 * ks), s[ct], 0, 0, 0);
            }
        }
        // ---- the online softmax of this lane's row ----
        float cm = ninf;
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = j0 + 32 * ct + (i & 3) + 8 * (i >> 2) + 4 * hh;
                const float v = j < vis ? scale * s[ct][i] : ninf;
                s[ct][i] = v;
                cm = fmaxf(cm, v);
            }
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float mn = fmaxf(m, cm);
        const bool any = mn != ninf;                                 // (false: this row has seen no visible position yet)
        const float alpha = m == ninf ? 0.0f : expf(m - mn);
        float cs = 0.0f;
        f16x8 pf[NCT][2];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const float p = (any && s[ct][i] != ninf) ? expf(s[ct][i] - mn) : 0.0f;
                const _Float16 ph = (_Float16)p;
                pf[ct][i >> 3][i & 7] = ph;
                cs = cs + (float)ph;
            }
        cs = cs + __shfl_xor(cs, 32);
        l = l * alpha + cs;
        m = mn;
        // ---- O^T = O^T alpha + V^T P^T: the P tile is the B operand as it stands -- element i of k-step ks is position 16 ks + (i & 3) + 8 (i >> 2) + 4 hh;
        //      the A operand V^T[d][.] at the same positions is two transposed reads of the image, d = 256 dh + 32 dt + r.  The step's product is summed
        //      from ZERO and added to O^T alpha in f32 (round to nearest): as the MFMA's C operand a residue of O^T alpha far below the product's last
        //      bit is not rounded away but pulls the sum one ulp toward zero (a row whose weight sits on one position of a later step: V[j] minus an ulp) ----
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
            f32x16 pv;
#pragma unroll
            for (int i = 0; i < 16; ++i) pv[i] = 0.0f;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const int off = (dt >> 2) * IMG_TILE + 256 * (32 * ct + 16 * ks);
                    const f16x4 lo = tr_read(lds + tbase[0][dt & 3] + off), hi = tr_read(lds + tbase[1][dt & 3] + off);
                    f16x8 a;
                    a[0] = lo[0]; a[1] = lo[1]; a[2] = lo[2]; a[3] = lo[3]; a[4] = hi[0]; a[5] = hi[1]; a[6] = hi[2]; a[7] = hi[3];
                    pv = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf[ct][ks], pv, 0, 0, 0);
                }
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dt][i] = o[dt][i] * alpha + pv[i];
        }
    }
}

// grid: x the row tile, y the span (SPLIT; 1 for WALK), z the sequence (PAGED; 1 otherwise)
template <bool Q8, bool PAGED, bool SPLIT>
__global__ __launch_bounds__(256) void mla_kernel(const mla_args a, const kv_pages pg, int len_bias) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5, rh = wave & 1, dh = wave >> 1;
    const int b = PAGED ? (int)blockIdx.z : 0;
    const int n_q = (int)a.n_q, rows = n_q * a.n_head;               // the sequence's rows (below 2^31: the entry's rule)
    const int n_kv = PAGED ? paged_count(pg, b, len_bias) : device_count(a.d_n_kv, (int)a.n_kv, (int)a.n_kv_max);
    const int R0 = (int)blockIdx.x * TILE, Rw = R0 + 32 * rh;        // the workgroup's and the wave's first row
    const int R = min(Rw + r, rows - 1);                             // this lane's row (a lane past the rows computes a copy and stores nothing)
    const int t = R / a.n_head, h = R - t * a.n_head;
    const int vis = visible(t, n_kv, n_q, a.causal);
    const int wg_vis = visible(min(R0 + TILE - 1, rows - 1) / a.n_head, n_kv, n_q, a.causal);      // vis is monotone in the row: the workgroup's largest
    const int wave_vis = Rw < rows ? visible(min(Rw + 31, rows - 1) / a.n_head, n_kv, n_q, a.causal) : 0;
    const int n_steps = (wg_vis + STEP - 1) / STEP;
    int st_begin = 0, st_end = n_steps;
    if constexpr (SPLIT) {
        st_begin = (int)blockIdx.y * (MLA_SPAN * (C / STEP));
        if (st_begin >= n_steps) return;                             // (workgroup-uniform: no row of the tile sees the span)
        st_end = min(st_begin + MLA_SPAN * (C / STEP), n_steps);
    }
    const int64_t tok = (int64_t)b * n_q + t;
    const int32_t *pages = nullptr;
    if constexpr (PAGED) {
        pages = pg.pages + (int64_t)b * pg.ld_pages;
        if (paged_any_invalid<256>(pages, n_kv, pg.n_pages)) {
            if constexpr (!SPLIT) {
                if (Rw + r < rows) {
                    float *out = a.dst + tok * a.ldd_tok + (int64_t)h * a.ldd_head + 256 * dh;
#pragma unroll
                    for (int i = 0; i < 256 / 8; ++i) *(float4 *)(out + 8 * i + 4 * hh) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
            }
            return;                                                  // (SPLIT: the merge scans the ids itself and writes the zeros)
        }
    }
    f32x16 o[NDT];
    float m, l;
    mla_body<Q8, PAGED>(lds, a.q + (int64_t)b * n_q * a.ldq_tok, a.ldq_tok, a.ldq_head, a.n_head, R0, rows, (const uint8_t *)a.cache, a.nb_pos, pages, pg.nb_page, n_kv, vis, wave_vis,
                        st_begin, st_end, a.scale, o, m, l);
    if (Rw + r >= rows) return;
    // register i of tile dt is column 256 dh + 32 dt + (i & 3) + 8 (i >> 2) + 4 hh
    if constexpr (SPLIT) {
        if (vis <= st_begin * STEP) return;                          // (no visible position in the span: no partial)
        float *part = a.work + (((int64_t)b * rows + R) * a.n_spans + blockIdx.y) * PART;
        if (dh == 0 && hh == 0) { part[0] = m; part[1] = l; }
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g)
                *(float4 *)(part + 4 + 256 * dh + 32 * dt + 8 * g + 4 * hh) = make_float4(o[dt][4 * g], o[dt][4 * g + 1], o[dt][4 * g + 2], o[dt][4 * g + 3]);
    } else {
        float *out = a.dst + tok * a.ldd_tok + (int64_t)h * a.ldd_head + 256 * dh;
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
            for (int g = 0; g < 4; ++g) {
                float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
                if (l != 0.0f) f = make_float4(o[dt][4 * g] / l, o[dt][4 * g + 1] / l, o[dt][4 * g + 2] / l, o[dt][4 * g + 3] / l);
                *(float4 *)(out + 32 * dt + 8 * g + 4 * hh) = f;
            }
    }
}

// the merge of the SPLIT form: one workgroup of 512 threads per row of all sequences, blockIdx.x = (b * n_q + t) * n_head + h; thread d owns column d
template <bool PAGED>
__global__ __launch_bounds__(DV) void mla_merge_kernel(const mla_args a, const kv_pages pg, int len_bias) {
    const int d = threadIdx.x, n_q = (int)a.n_q;
    const int bt = blockIdx.x / a.n_head, h = blockIdx.x - bt * a.n_head;
    const int b = bt / n_q, t = bt - b * n_q;
    const int n_kv = PAGED ? paged_count(pg, b, len_bias) : device_count(a.d_n_kv, (int)a.n_kv, (int)a.n_kv_max);
    float *out = a.dst + (int64_t)bt * a.ldd_tok + (int64_t)h * a.ldd_head + d;
    if constexpr (PAGED)
        if (paged_any_invalid<DV>(pg.pages + (int64_t)b * pg.ld_pages, n_kv, pg.n_pages)) { *out = 0.0f; return; }
    const int vis = visible(t, n_kv, n_q, a.causal);
    if (vis <= 0) { *out = 0.0f; return; }
    const int ns = (vis + C * MLA_SPAN - 1) / (C * MLA_SPAN);        // <= n_spans: vis <= n_kv_max
    const float *part = a.work + (int64_t)blockIdx.x * a.n_spans * PART;
    float M = part[0];
    for (int s = 1; s < ns; ++s) M = fmaxf(M, part[(int64_t)s * PART]);
    float L, A;
    {
        const float m = part[0], bs = m == M ? 1.0f : expf(m - M);
        L = part[1] * bs; A = part[4 + d] * bs;
    }
    for (int s = 1; s < ns; ++s) {
        const float *p = part + (int64_t)s * PART;
        const float m = p[0], bs = m == M ? 1.0f : expf(m - M);
        L = fmaf(p[1], bs, L); A = fmaf(p[4 + d], bs, A);
    }
    *out = A / L;
}

// the paged store of latent rows: row (b, t) of src [n_seq * n_q][576] -> page row of position len[b] + t; one thread per 32 (Q8_0) or 4 (F16) elements,
// packed by kv_pack.h (the bytes of ggml_hip_kv_store_dev at row_elems = 576).  Every guard stands in front of the address it protects.
template <bool Q8>
__global__ __launch_bounds__(256) void kv_store_latent_paged_kernel(const float *__restrict__ src, int64_t ld, int64_t n_tokens, int n_q, uint8_t *__restrict__ pool,
                                                                    int64_t nb_pos, const kv_pages pg) {
    constexpr int UNITS = Q8 ? DK / QK : DK / 4;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_tokens * UNITS) return;
    const int64_t tok = i / UNITS;
    const int u = (int)(i - tok * UNITS);
    const int64_t b = tok / n_q;
    const int64_t pos = (int64_t)pg.len[b] + (tok - b * n_q);
    if (pos < 0 || pos >= pg.n_kv_max) return;                      // (before the table is read)
    const int page = pg.pages[b * pg.ld_pages + pos / C];
    if (page < 0 || page >= pg.n_pages) return;                     // (before any address is formed from it)
    uint8_t *row = pool + (int64_t)page * pg.nb_page + (pos % C) * nb_pos;
    const float *x = src + tok * ld;
    if constexpr (Q8) {
        const float4 *x4 = (const float4 *)(x + 32 * u);
        float v[QK];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float4 f = x4[k]; v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w; }
        kv_pack_q8_0(v, (uint32_t *)(row + 36 * (int64_t)u));
    } else {
        const float4 f = *(const float4 *)(x + 4 * u);
        *(uint2 *)(row + 8 * (int64_t)u) = kv_pack_f16(f);
    }
}

template <bool Q8, bool PAGED>
hipError_t launch_form(const mla_plan &pl, const mla_args &a, int64_t n_seq, const kv_pages &pg, int len_bias, hipStream_t st) {
    const dim3 grid((unsigned)pl.tiles, (unsigned)(pl.form == MLA_FORM_SPLIT ? pl.n_spans : 1), (unsigned)n_seq);
    if (pl.form == MLA_FORM_WALK) return launch_lds(kfn<mla_kernel<Q8, PAGED, false>>, grid, dim3(256), MLA_LDS, MLA_LDS, st, a, pg, len_bias);
    if (pl.n_spans > 0) {                                            // (n_kv_max = 0: no span, the merge writes the zeros)
        const hipError_t e = launch_lds(kfn<mla_kernel<Q8, PAGED, true>>, grid, dim3(256), MLA_LDS, MLA_LDS, st, a, pg, len_bias);
        if (e != hipSuccess) return e;
    }
    mla_merge_kernel<PAGED><<<dim3((unsigned)pl.merge_wgs), dim3(DV), 0, st>>>(a, pg, len_bias);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_attn_mla(const mla_plan &pl, const mla_args &a, int64_t n_seq, const kv_pages *pg, int len_bias, hipStream_t st) {
    const bool q8 = a.kv_type == GGML_TYPE_Q8_0;
    if (pg) return q8 ? launch_form<true, true>(pl, a, n_seq, *pg, len_bias, st) : launch_form<false, true>(pl, a, n_seq, *pg, len_bias, st);
    return q8 ? launch_form<true, false>(pl, a, 1, kv_pages{}, 0, st) : launch_form<false, false>(pl, a, 1, kv_pages{}, 0, st);
}

hipError_t launch_kv_store_latent_paged(int kv_type, const float *src, int64_t ld, int64_t n_seq, int64_t n_q, void *pool, int64_t nb_pos, const kv_pages &pg,
                                        hipStream_t st) {
    const bool q8 = kv_type == GGML_TYPE_Q8_0;
    const int64_t n_tokens = n_seq * n_q, threads = n_tokens * (q8 ? MLA_DK / QK : MLA_DK / 4);
    const dim3 grid((unsigned)((threads + 255) / 256));
    if (q8) kv_store_latent_paged_kernel<true><<<grid, dim3(256), 0, st>>>(src, ld, n_tokens, (int)n_q, (uint8_t *)pool, nb_pos, pg);
    else kv_store_latent_paged_kernel<false><<<grid, dim3(256), 0, st>>>(src, ld, n_tokens, (int)n_q, (uint8_t *)pool, nb_pos, pg);
    return hipGetLastError();
}
