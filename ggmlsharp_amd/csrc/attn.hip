// attn.hip -- attention over an F16 or Q8_0 KV cache on the device (include/ggml_hip_ext.h ggml_hip_kv_store_dev, ggml_hip_attn_dev;
// attn.cpp has the C-ABI, plan.cpp plan_attn chooses the form from n_q alone).  Upstream's ggml_flash_attn_ext without mask tensor and ALiBi;
// a sliding window, sinks and a soft-cap are the _ex entries' (the OPTIONS block below), the mask tensor and ALiBi slopes the _bias entries' (MASK AND SLOPES); an EXTENSION like mul_mat_id (the reference has the
// op's id and no dispatch).
//
// A cache row is (position j, kv head hk): D elements in reference block format at  base + j * nb_pos + hk * nb_head  (F16: 2 D bytes of IEEE
// halves; Q8_0: D / 32 blocks {f32 d; int8 qs[32]} of 36 bytes).  deq(row)[i] is the half widened (exact), or (float)qs[i] * d in ONE binary32
// rounding -- what ggml_hip_dequantize_rows_dev returns.  Query head h reads kv head h / G, G = n_head / n_head_kv.
// VISIBLE positions of query row t:  j < vis(t),  vis(t) = causal ? clamp(n_kv - n_q + t + 1, 0, n_kv) : n_kv.
// CHUNK: the positions are cut into chunks of ATTN_CHUNK = 128, chunk c = [128 c, 128 c + 128), for every (kv_type, D), both forms.
//
// ---- kv_store ----  one thread per 32 elements (Q8_0) or 4 elements (F16) of a source row, packed by kv_pack.h.  Q8_0: quantize.hip's statement of
// quantize_row_q8_0 (amax; d = amax / 127; id = d ? 1 / d : 0; q = rint(v * id); the library is built without contraction and with the
// correctly rounded division), bit for bit ggml_hip_quantize_rows_dev.  F16: IEEE round to nearest even by integer arithmetic (subnormals
// kept, overflow to inf, a NaN stays a NaN).  A row whose position is outside [0, n_pos_max) leaves before any address is formed.
//
// ---- DECODE form (n_q <= 8), all f32 ----
// A workgroup (256 threads) serves ONE kv head and ONE chunk for all R = G * n_q query rows of that kv head: it copies the chunk's K and V
// rows into LDS as they are (raw halves / raw Q8_0 blocks, each byte of the cache read once per launch), then for the rows, eight at a time:
//     s_j   = scale * dot(q, deq(K_j))       the dot an f32 fma chain over d ascending from 0.0f; q is f32 as given
//     m     = max of s_j over the chunk's visible j                                         (exact)
//     p_j   = s_j == m ? 1 : expf(s_j - m)
//     l     = sum of p_j: lane L of a wave holds p_L + p_(L+64), the 64 lane sums meet in a butterfly (lane distance 32, 16, .., 1)
//     a[d]  = p_0 * deq(V_0)[d], then a[d] = fma(p_j, deq(V_j)[d], a[d]) for j ascending  (one thread per four columns d)
// and writes the partial (m, l, a[D]) of (row, chunk) into the work buffer.  An invisible position takes no part in any of it (it is
// never multiplied by zero: what the cache holds there does not matter).  A second launch, one workgroup per query row, MERGES:
//     M = max over the row's chunks c of m_c;  b_c = m_c == M ? 1 : expf(m_c - M)
//     L = l_0 * b_0, A[d] = a_0[d] * b_0, then L = fma(l_c, b_c, L), A[d] = fma(a_c[d], b_c, A[d]) for c ASCENDING
//     dst[d] = A[d] / L                                                                      (+0.0f for a row with no visible position)
// No atomics: nothing depends on scheduling, on n_head, on n_kv_max, on the strides or on how many rows share the workgroup.
// With one visible position p = 1, l = 1, b = 1: dst is deq(V_0) bit for bit.
//
// ---- PROMPT form (n_q > 8), matrix cores ----
// A workgroup (4 waves) owns 128 consecutive query rows of one head, a wave 32 of them, and walks the chunks that hold a visible position
// of its rows in ascending order; chunks above the causal diagonal are skipped, the diagonal chunk is masked per element.  Per chunk K is
// staged in LDS as f16 [position][D], V as f16 TRANSPOSED [d][position]; a Q8_0 row is dequantized while staged: (float)q * d rounded to
// f16 (RNE).  Rows of the chunk at or beyond n_kv are staged as zeros.  Q is rounded to f16 (RNE) once.  All on v_mfma_f32_32x32x16_f16:
//     S^T   = K Q^T             f16 products exact, f32 accumulation; a lane owns one query, its registers hold the positions
//     s_j   = scale * S_j       (f32);  invisible j: -inf
//     m'    = max(m, max_j s_j);  alpha = expf(m - m') (0 for the first chunk);  p_j = expf(s_j - m'), 0 where invisible
//     P_j   = f16(p_j)          RNE;  l = l * alpha + sum_j P_j  -- the sum is of the ROUNDED weights, so dst is a true weighted mean of V
//     O^T   = O^T * alpha + V^T P^T   (f32 accumulators: the online-softmax state m, l, O stays in f32 registers)
//     dst   = O / l             (+0.0f where l == 0: no visible position)
// With one visible position P = 1, l = 1: dst is the STAGED V row bit for bit -- deq(V_0) for an F16 cache, f16(deq(V_0)) for a Q8_0 cache.
// A masked weight is a ZERO operand of the matrix core here, so the cache must hold finite values at every position below n_kv.
//
// V CONSTANT over the positions: neither form returns the constant exactly in general -- a[d] = sum of fl(p_j * c) and l = sum of p_j round
// independently, a / l is c only up to the accumulation error -- so that case is held to the tolerance, not to bits.
//
// ---- PAGED (ggml_hip_kv_store_paged_dev, ggml_hip_attn_paged_dev; common.h kv_pages) ----
// A pool of pages of ATTN_CHUNK = 128 positions, page p at pool + p * nb_page, row (jj, hk) inside it at jj * nb_pos + hk * nb_head; sequence b's
// positions [128 c, 128 c + 128) lie in page pages[b][c], and n_kv[b] = clamp(len[b] + len_bias, 0, n_kv_max).  A page IS a chunk, and neither
// form's arithmetic knows where a chunk lies: the chunk bodies below (attn_decode_chunk, attn_merge_row, attn_prompt_tile) are shared by a
// contiguous and a paged kernel each, so a sequence's rows are bit for bit the contiguous call on the same row bytes.  The paged kernels carry
// the sequence in grid z (the merge: in its row index).  A workgroup whose chunk lies at or beyond n_kv[b] leaves at once; a page id outside
// [0, n_pages) among a sequence's first ceil(n_kv[b] / 128) entries makes ALL its rows +0.0f (DECODE: the merge scans the ids; PROMPT: the
// workgroup does before its first stage) and no address is ever formed from such an id.
//
// ---- OPTIONS (ggml_hip_attn_ex_dev, ggml_hip_attn_paged_ex_dev; common.h attn_var; the header's ATTENTION OPTIONS section is the statement) ----
// The chunk bodies carry a template <bool VAR>; VAR = false IS the kernels above (every use of attn_var sits under if constexpr (VAR)), VAR = true
// serves the six _ex kernels.  WINDOW W: row t sees lo_t <= j < hi_t, hi_t = vis(t), lo_t = max(0, hi_t - W) (window_lo); a position outside takes
// part in nothing, a (row, chunk) without a visible position has no partial.  DECODE: the a[d] chain starts at the row's first visible position of
// the chunk; workgroup x serves chunk c_lo + x, c_lo = lo_0 / 128 from the n_kv the kernel reads anyway, and writes work-buffer chunk x; the merge
// walks the row's chunks lo_t / 128 .. (hi_t - 1) / 128 ascending, the first term the product.  PROMPT: the workgroup starts at the chunk of its
// first row's lo, a wave skips the chunks wholly below its first row's lo, the element mask gains j >= lo.  SOFT-CAP: s = cap * tanhf(sc' * dot),
// sc' = scale / cap from the host.  SINKS: sink_h joins M and the denominator only (DECODE: in the merge; PROMPT: one more online-softmax step
// after the last chunk).  PAGED: no table entry below c_lo[b] is read; the id scans start there.
//
// ---- MASK AND SLOPES (ggml_hip_attn_bias_dev, ggml_hip_attn_paged_bias_dev, ggml_hip_attn_paged_ragged_bias_dev; common.h attn_bias; the header's section
// ATTENTION WITH A MASK TENSOR AND ALiBi SLOPES is the statement) ----
// The bodies carry a second template <bool MSK>; MSK = false IS the kernels above (every use of attn_bias sits under if constexpr (MSK)), MSK = true (always
// with VAR = true, vo possibly all off) serves the mask kernels: the _ex and the ragged kernels instantiated once more.  A mask value of -inf hides the position
// from the row, any other value mk turns the score into fma(slope_h, mk, s).  DECODE: the score thread fetches its four rows' mask halves before its dot
// products; the softmax pass finds the row's first and last mask-visible position of the chunk by ballots and hands them to the P V pass through LDS; a
// chunk of the row's range with none writes the partial (-inf, 0, 0), and the merge returns +0.0f where M = -inf.  PROMPT: a lane fetches the 16 8-byte
// pieces of its own mask row under the chunk before the chunk is staged; the online softmax needs nothing new (an empty chunk has alpha = 1 and every P = 0).
//
// ---- RAGGED (ggml_hip_attn_paged_ragged_dev, ggml_hip_kv_store_paged_ragged_dev, ggml_hip_ragged_positions_dev; common.h kv_ragged) ----
// The paged kernels with a query count PER SEQUENCE read on the device (q_start, prefix sums over packed rows): an index launch turns q_start into row slots
// and a tile list, and the paged DECODE, merge and PROMPT kernels take (sequence, row base, n_q) from those tables -- the same chunk bodies, so the same bits.
// The RAGGED block below has the statement.
#include "common.h"
#include "plan.h"
#include "kv_pack.h"     // f32_to_f16_bits, kv_pack_q8_0, kv_pack_f16: the bytes of a cache row (shared with rope.hip)

namespace {

using f16x8 = __attribute__((ext_vector_type(8))) _Float16;
using f16x4 = __attribute__((ext_vector_type(4))) _Float16;
using f32x16 = __attribute__((ext_vector_type(16))) float;

constexpr int C = ATTN_CHUNK;

__device__ __forceinline__ float f16_bits_to_f32(uint32_t h) { return (float)__builtin_bit_cast(_Float16, (uint16_t)h); }   // exact

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

// the first visible position of a row whose visible range ends at hi, under a window of W positions (0: none): max(0, hi - W)
__device__ __forceinline__ int window_lo(int hi, int window) { return window > 0 && hi > window ? hi - window : 0; }

// ------------------------------------------------------------------------------------------------ kv_store
template <bool Q8>
__global__ __launch_bounds__(256) void kv_store_kernel(const float *__restrict__ src, int64_t ld, int64_t n_rows, int units_per_row, uint8_t *__restrict__ cache,
                                                       int64_t nb_pos, int64_t n_pos_max, int64_t pos0, const int32_t *__restrict__ d_pos0) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n_rows * units_per_row) return;
    const int64_t r = i / units_per_row;
    const int u = (int)(i - r * units_per_row);
    const int64_t pos = (d_pos0 ? (int64_t)*d_pos0 : pos0) + r;
    if (pos < 0 || pos >= n_pos_max) return;                        // (before any address is formed from it)
    uint8_t *row = cache + pos * nb_pos;
    if constexpr (Q8) {
        const float4 *x = (const float4 *)(src + r * ld + 32 * u);
        float v[QK];
#pragma unroll
        for (int k = 0; k < 8; ++k) { const float4 f = x[k]; v[4 * k] = f.x; v[4 * k + 1] = f.y; v[4 * k + 2] = f.z; v[4 * k + 3] = f.w; }
        kv_pack_q8_0(v, (uint32_t *)(row + 36 * (int64_t)u));
    } else {
        const float4 f = *(const float4 *)(src + r * ld + 4 * u);
        *(uint2 *)(row + 8 * (int64_t)u) = kv_pack_f16(f);
    }
}

// n_kv of sequence b of a paged call: clamp(len[b] + len_bias, 0, n_kv_max)
__device__ __forceinline__ int paged_count(const kv_pages &pg, int b, int len_bias) {
    const int64_t n = (int64_t)pg.len[b] + len_bias;
    return (int)(n < 0 ? 0 : n > pg.n_kv_max ? pg.n_kv_max : n);
}

// the paged store: row (b, t, hk) of [n_seq * n_q][n_head_kv][D] -> page row (len[b] + t, hk); the kv_pack.h statement of kv_store_kernel
// behind the paged address.  Every guard stands in front of the address it protects: the table is read only for a position inside
// [0, n_kv_max) (whose chunk index is below ld_pages, the entry's rule), the pool is addressed only with a page id inside [0, n_pages).
// unit u of row (tok, hk) of the source rows -> its bytes in the page row of position pos of sequence b: the guards and the packing both paged
// stores share
template <bool Q8>
__device__ __forceinline__ void kv_store_paged_unit(const float *__restrict__ src, int64_t ldx_tok, int64_t ldx_head, int64_t tok, int hk, int u, int64_t b,
                                                    int64_t pos, uint8_t *__restrict__ pool, int64_t nb_pos, int64_t nb_head, const kv_pages &pg) {
    if (pos < 0 || pos >= pg.n_kv_max) return;                      // (before the table is read)
    const int page = pg.pages[b * pg.ld_pages + pos / C];
    if (page < 0 || page >= pg.n_pages) return;                     // (before any address is formed from it)
    uint8_t *row = pool + (int64_t)page * pg.nb_page + (pos % C) * nb_pos + (int64_t)hk * nb_head;
    const float *x = src + tok * ldx_tok + (int64_t)hk * ldx_head;
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

template <bool Q8>
__global__ __launch_bounds__(256) void kv_store_paged_kernel(const float *__restrict__ src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int units_per_head,
                                                             int64_t n_tokens, int n_q, uint8_t *__restrict__ pool, int64_t nb_pos, int64_t nb_head, const kv_pages pg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per_tok = (int64_t)n_head_kv * units_per_head;
    if (i >= n_tokens * per_tok) return;
    const int64_t tok = i / per_tok;
    const int r = (int)(i - tok * per_tok), hk = r / units_per_head, u = r - hk * units_per_head;
    const int64_t b = tok / n_q;
    kv_store_paged_unit<Q8>(src, ldx_tok, ldx_head, tok, hk, u, b, (int64_t)pg.len[b] + (tok - b * n_q), pool, nb_pos, nb_head, pg);
}

// the RAGGED paged store: packed rows [n_tokens_max][n_head_kv][D], one thread per unit as above; the thread finds its row's sequence by bisection of
// q_start (common.h ragged_find: a present sequence, the row inside it -- else nothing is read or written for the row), then the unit above
template <bool Q8>
__global__ __launch_bounds__(256) void kv_store_paged_ragged_kernel(const float *__restrict__ src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv,
                                                                    int units_per_head, const kv_ragged rg, uint8_t *__restrict__ pool, int64_t nb_pos,
                                                                    int64_t nb_head, const kv_pages pg) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t per_tok = (int64_t)n_head_kv * units_per_head;
    if (i >= rg.n_tokens_max * per_tok) return;
    const int64_t tok = i / per_tok;
    const int r = (int)(i - tok * per_tok), hk = r / units_per_head, u = r - hk * units_per_head;
    int t;
    const int b = ragged_find(rg, tok, &t);
    if (b < 0) return;
    kv_store_paged_unit<Q8>(src, ldx_tok, ldx_head, tok, hk, u, b, (int64_t)pg.len[b] + t, pool, nb_pos, nb_head, pg);
}

// d_pos of the packed rows: len[b] + t for row (b, t) of a present sequence, 0 for every other row below n_tokens_max
__global__ __launch_bounds__(256) void ragged_positions_kernel(const kv_ragged rg, const int32_t *__restrict__ len, int32_t *__restrict__ pos) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rg.n_tokens_max) return;
    int t;
    const int b = ragged_find(rg, i, &t);
    pos[i] = b < 0 ? 0 : (int32_t)((uint32_t)len[b] + (uint32_t)t);
}

// ------------------------------------------------------------------------------------------------ DECODE form
// bytes of a cache row, and its stride in the LDS stage (F16: + 8, rows of 8-byte reads spread over all banks; Q8_0: + 4, an odd word count)
template <bool Q8> __host__ __device__ constexpr int row_bytes_of(int D) { return Q8 ? D / 32 * 36 : 2 * D; }
template <bool Q8> __host__ __device__ constexpr int stage_stride(int D) { return row_bytes_of<Q8>(D) + (Q8 ? 4 : 8); }
constexpr int DEC_RT = 8;                                           // query rows per pass of a decode workgroup

template <bool Q8>
__device__ __forceinline__ void load8(const uint8_t *row, int d8, float (&k)[8]) {      // elements 8 d8 .. 8 d8 + 7 of a staged row
    if constexpr (Q8) {
        const uint32_t *b = (const uint32_t *)(row + 36 * (d8 >> 2));
        const float d = __uint_as_float(b[0]);
        const uint32_t w0 = b[1 + 2 * (d8 & 3)], w1 = b[2 + 2 * (d8 & 3)];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            k[i] = (float)(int)(int8_t)((w0 >> (8 * i)) & 0xFFu) * d;
            k[4 + i] = (float)(int)(int8_t)((w1 >> (8 * i)) & 0xFFu) * d;
        }
    } else {
        const uint2 a = *(const uint2 *)(row + 16 * d8), b = *(const uint2 *)(row + 16 * d8 + 8);
        k[0] = f16_bits_to_f32(a.x & 0xFFFFu); k[1] = f16_bits_to_f32(a.x >> 16); k[2] = f16_bits_to_f32(a.y & 0xFFFFu); k[3] = f16_bits_to_f32(a.y >> 16);
        k[4] = f16_bits_to_f32(b.x & 0xFFFFu); k[5] = f16_bits_to_f32(b.x >> 16); k[6] = f16_bits_to_f32(b.y & 0xFFFFu); k[7] = f16_bits_to_f32(b.y >> 16);
    }
}

template <bool Q8>
__device__ __forceinline__ void load4(const uint8_t *row, int d4, float (&v)[4]) {      // elements 4 d4 .. 4 d4 + 3 of a staged row
    if constexpr (Q8) {
        const uint32_t *b = (const uint32_t *)(row + 36 * (d4 >> 3));
        const float d = __uint_as_float(b[0]);
        const uint32_t w = b[1 + (d4 & 7)];
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = (float)(int)(int8_t)((w >> (8 * i)) & 0xFFu) * d;
    } else {
        const uint2 a = *(const uint2 *)(row + 8 * d4);
        v[0] = f16_bits_to_f32(a.x & 0xFFFFu); v[1] = f16_bits_to_f32(a.x >> 16); v[2] = f16_bits_to_f32(a.y & 0xFFFFu); v[3] = f16_bits_to_f32(a.y >> 16);
    }
}

// the work buffer: partial (row gr = t * n_head + h, chunk c) at ((gr * n_chunks_max) + c) * (D + 4) floats: m, l, two spare, a[D]
// THE CHUNK BODY of the DECODE form, shared by the contiguous and the paged kernel: chunk c (j0 = 128 c < n_kv) of kv head hk, its rows at
// kb / vb + j * nb_pos -- where the chunk lies in memory is the caller's, the arithmetic does not know.  q and work are the sequence's own.
// VAR (the _ex kernels): the partial goes to work-buffer chunk index wc = c - c_lo, the score may be soft-capped, and a row's visible range
// inside the chunk is [f, n) instead of [0, n): its a[d] chain starts at f, and a chunk with no visible position writes no partial.
// MSK (the mask kernels, always with VAR): mrow0 = the mask row of the sequence's query 0, ld halves between rows; the score thread adds
// slope_h * mask[t][j0 + j] in one fma, a mask value of -inf makes the position invisible to the row (its score becomes the marker -inf and
// its weight the marker -1: it is skipped, never multiplied).  The a[d] chain runs from the row's first to its last MASK-VISIBLE position of
// the chunk (wave ballots, handed to the P V pass through LDS); a (row, chunk) inside the row's structural range with none writes the partial
// (m = -inf, l = 0, a = 0), which the merge takes as nothing.
template <bool Q8, int D, bool VAR, bool MSK = false>
__device__ __forceinline__ void attn_decode_chunk(uint8_t *lds, const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kb,
                                                  const uint8_t *__restrict__ vb, int64_t nb_pos, int n_head, int G, int n_q, int n_kv, int c, int wc, int hk,
                                                  int causal, float scale, float *__restrict__ work, int n_chunks_max, const attn_var &vo,
                                                  const attn_bias &bs = attn_bias{}) {
    static_assert(!MSK || VAR, "the mask kernels run the VAR bodies");
    constexpr int RB = row_bytes_of<Q8>(D), ST = stage_stride<Q8>(D), PPR = RB / 8;
    uint8_t *kst = lds, *vst = lds + C * ST;
    float *qt = (float *)(lds + 2 * C * ST);                         // [DEC_RT][D]
    float *sc = qt + DEC_RT * D;                                     // [DEC_RT][C]
    int *fl = (int *)(sc + DEC_RT * C);                              // MSK: [DEC_RT][2] first / last mask-visible position of the pass's rows (decode_lds)
    static_assert((2 * C * ST) % 16 == 0, "the query tile is read as float4");
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int j0 = c * C;
    const int cnt = min(C, n_kv - j0);                               // rows of this chunk the cache holds: all below n_kv <= n_kv_max
    // ---- the chunk's K and V rows into LDS, as they are: 8-byte pieces, each read once ----
    {
        const int per = cnt * PPR;
        constexpr int UN = 8;                                        // loads in flight per thread: all issued before the first is stored
        for (int i0 = tid; i0 < 2 * per; i0 += 256 * UN) {
            uint2 w[UN];
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int i = i0 + 256 * u;
                if (i < 2 * per) {
                    const bool isv = i >= per;
                    const int e = isv ? i - per : i, j = e / PPR, p = e - j * PPR;
                    w[u] = *(const uint2 *)((isv ? vb : kb) + (int64_t)j * nb_pos + 8 * p);
                }
            }
#pragma unroll
            for (int u = 0; u < UN; ++u) {
                const int i = i0 + 256 * u;
                if (i < 2 * per) {
                    const bool isv = i >= per;
                    const int e = isv ? i - per : i, j = e / PPR, p = e - j * PPR;
                    uint32_t *o = (uint32_t *)((isv ? vst : kst) + j * ST + 8 * p);
                    o[0] = w[u].x; o[1] = w[u].y;
                }
            }
        }
    }
    const int R = G * n_q;                                           // row r of this kv head: query t = r / G, head h = hk * G + r % G
    for (int r0 = 0; r0 < R; r0 += DEC_RT) {
        // ---- the pass's query rows (zeros past R) ----
        for (int i = tid; i < DEC_RT * (D / 4); i += 256) {
            const int ri = i / (D / 4), d4 = i - ri * (D / 4), r = r0 + ri;
            float4 f = make_float4(0.f, 0.f, 0.f, 0.f);
            if (r < R) f = *(const float4 *)(q + (int64_t)(r / G) * ldq_tok + (int64_t)(hk * G + r % G) * ldq_head + 4 * d4);
            *(float4 *)(qt + ri * D + 4 * d4) = f;
        }
        __syncthreads();
        // ---- scores: thread (position j, half hs) takes rows 4 hs .. 4 hs + 3 of the pass ----
        {
            const int j = tid & (C - 1), hs = tid >> 7;
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            uint32_t mb[4] = {0u, 0u, 0u, 0u};                       // MSK: the mask halves of this thread's four rows, in flight under the dot products
            float slope[4] = {1.0f, 1.0f, 1.0f, 1.0f};
            if constexpr (MSK) {
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    const int r = r0 + 4 * hs + i;
                    if (r < R && j < cnt) {                          // (column j0 + j < n_kv <= ld; a row past R has no mask row)
                        mb[i] = bs.mask[(int64_t)(r / G) * bs.ld + j0 + j];
                        if (bs.slopes) slope[i] = bs.slopes[hk * G + r % G];
                    }
                }
            }
            if (j < cnt) {
                const uint8_t *krow = kst + j * ST;
#pragma unroll 2
                for (int d8 = 0; d8 < D / 8; ++d8) {
                    float k[8];
                    load8<Q8>(krow, d8, k);
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float4 qa = *(const float4 *)(qt + (4 * hs + i) * D + 8 * d8), qb = *(const float4 *)(qt + (4 * hs + i) * D + 8 * d8 + 4);
                        float a = acc[i];
                        a = fmaf(qa.x, k[0], a); a = fmaf(qa.y, k[1], a); a = fmaf(qa.z, k[2], a); a = fmaf(qa.w, k[3], a);
                        a = fmaf(qb.x, k[4], a); a = fmaf(qb.y, k[5], a); a = fmaf(qb.z, k[6], a); a = fmaf(qb.w, k[7], a);
                        acc[i] = a;
                    }
                }
            }
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                float s;
                if constexpr (VAR) s = vo.cap != 0.0f ? vo.cap * tanhf(vo.sc * acc[i]) : scale * acc[i];
                else s = scale * acc[i];
                if constexpr (MSK) s = mb[i] == 0xFC00u ? -__builtin_inff() : fmaf(slope[i], f16_bits_to_f32(mb[i]), s);       // (+0.0 where nothing was read)
                sc[(4 * hs + i) * C + j] = s;
            }
        }
        __syncthreads();
        // ---- the chunk's softmax pieces: wave w takes rows w and w + 4 of the pass ----
#pragma unroll
        for (int k = 0; k < 2; ++k) {
            const int ri = wave + 4 * k, r = r0 + ri;
            if (r >= R) continue;                                    // (wave-uniform)
            const int hi = visible(r / G, n_kv, n_q, causal), vis = hi - j0;
            if (vis <= 0) continue;
            const int n = min(vis, C);
            int f = 0;                                               // the row's first visible position of the chunk (wave-uniform)
            if constexpr (VAR) {
                f = max(window_lo(hi, vo.window) - j0, 0);
                if (f >= n) continue;
            }
            bool in0 = lane >= f && lane < n, in1 = lane + 64 >= f && lane + 64 < n;
            const float ninf = -__builtin_inff();
            const float s0 = in0 ? sc[ri * C + lane] : ninf, s1 = in1 ? sc[ri * C + lane + 64] : ninf;
            if constexpr (MSK) {
                in0 = in0 && s0 != ninf; in1 = in1 && s1 != ninf;    // (the score thread's marker: masked)
                const unsigned long long b0 = __ballot(in0), b1 = __ballot(in1);
                if (lane == 0) {
                    fl[2 * ri] = b0 ? __builtin_ctzll(b0) : b1 ? 64 + __builtin_ctzll(b1) : C;
                    fl[2 * ri + 1] = b1 ? 127 - __builtin_clzll(b1) : b0 ? 63 - __builtin_clzll(b0) : -1;
                }
            }
            float m = fmaxf(s0, s1);
#pragma unroll
            for (int dd = 32; dd >= 1; dd >>= 1) m = fmaxf(m, __shfl_xor(m, dd));
            const float p0 = in0 ? (s0 == m ? 1.0f : expf(s0 - m)) : 0.0f, p1 = in1 ? (s1 == m ? 1.0f : expf(s1 - m)) : 0.0f;
            if constexpr (MSK) { sc[ri * C + lane] = in0 ? p0 : -1.0f; sc[ri * C + lane + 64] = in1 ? p1 : -1.0f; }
            else { sc[ri * C + lane] = p0; sc[ri * C + lane + 64] = p1; }
            float l = p0 + p1;
#pragma unroll
            for (int dd = 32; dd >= 1; dd >>= 1) l = l + __shfl_xor(l, dd);
            if (lane == 0) {
                const int64_t gr = (int64_t)(r / G) * n_head + hk * G + r % G;
                float *part = work + (gr * n_chunks_max + wc) * (D + 4);
                part[0] = m; part[1] = l;
            }
        }
        __syncthreads();
        // ---- a[d] = sum of p_j deq(V_j)[d], j ascending: a group of D / 4 threads per row, a thread per four columns ----
        {
            constexpr int TPR = D / 4, NG = 256 / TPR;
            const int g = tid / TPR, d4 = tid - g * TPR;
            for (int ri = g; ri < DEC_RT; ri += NG) {
                const int r = r0 + ri;
                if (r >= R) break;
                const int hi = visible(r / G, n_kv, n_q, causal), vis = hi - j0;
                if (vis <= 0) continue;
                const int n = min(vis, C);
                int f = 0;
                if constexpr (VAR) {
                    f = max(window_lo(hi, vo.window) - j0, 0);
                    if (f >= n) continue;
                }
                float v[4], a[4];
                if constexpr (MSK) {
                    const int first = fl[2 * ri], last = fl[2 * ri + 1];
                    if (last < 0) {                                  // every position masked: the empty partial
#pragma unroll
                        for (int i = 0; i < 4; ++i) a[i] = 0.0f;
                    } else {
                        load4<Q8>(vst + first * ST, d4, v);
                        const float pf = sc[ri * C + first];
#pragma unroll
                        for (int i = 0; i < 4; ++i) a[i] = pf * v[i];
#pragma unroll 4
                        for (int j = first + 1; j <= last; ++j) {
                            load4<Q8>(vst + j * ST, d4, v);
                            const float p = sc[ri * C + j];
#pragma unroll
                            for (int i = 0; i < 4; ++i) a[i] = p < 0.0f ? a[i] : fmaf(p, v[i], a[i]);     // (the marker -1: masked -- a[] is kept, the product is never taken)
                        }
                    }
                } else {
                    load4<Q8>(vst + f * ST, d4, v);
                    const float pf = sc[ri * C + f];
#pragma unroll
                    for (int i = 0; i < 4; ++i) a[i] = pf * v[i];
#pragma unroll 4
                    for (int j = f + 1; j < n; ++j) {
                        load4<Q8>(vst + j * ST, d4, v);
                        const float p = sc[ri * C + j];
#pragma unroll
                        for (int i = 0; i < 4; ++i) a[i] = fmaf(p, v[i], a[i]);
                    }
                }
                const int64_t gr = (int64_t)(r / G) * n_head + hk * G + r % G;
                *(float4 *)(work + (gr * n_chunks_max + wc) * (D + 4) + 4 + 4 * d4) = make_float4(a[0], a[1], a[2], a[3]);
            }
        }
        __syncthreads();                                             // (the next pass rewrites the query tile and the scores)
    }
}

template <bool Q8, int D>
__global__ __launch_bounds__(256) void attn_decode_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                          const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int n_head, int G, int n_q,
                                                          int n_kv_host, const int32_t *__restrict__ d_n_kv, int n_kv_max, int causal, float scale,
                                                          float *__restrict__ work, int n_chunks_max) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int c = blockIdx.x, hk = blockIdx.y;
    const int n_kv = device_count(d_n_kv, n_kv_host, n_kv_max);
    const int j0 = c * C;
    if (j0 >= n_kv) return;                                          // (the whole workgroup: no barrier was reached)
    const int64_t off = (int64_t)j0 * nb_pos + (int64_t)hk * nb_head;
    attn_decode_chunk<Q8, D, false>(lds, q, ldq_tok, ldq_head, kc + off, vc + off, nb_pos, n_head, G, n_q, n_kv, c, c, hk, causal, scale, work, n_chunks_max,
                                    attn_var{});
}

// the _ex DECODE kernel: workgroup x serves chunk c_lo + x, c_lo the chunk of row 0's first visible position, from the same clamped n_kv
// MSK (here and in every _ex / ragged kernel below): the mask kernel of the _bias entries -- the same kernel with the mask handed to the body as q is
// (the sequence's first row); MSK = false never reads bs and is the _ex kernel as it was
template <bool Q8, int D, bool MSK>
__global__ __launch_bounds__(256) void attn_decode_ex_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                             const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int n_head, int G, int n_q,
                                                             int n_kv_host, const int32_t *__restrict__ d_n_kv, int n_kv_max, int causal, float scale,
                                                             float *__restrict__ work, int n_chunks_max, const attn_var vo, const attn_bias bs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int hk = blockIdx.y;
    const int n_kv = device_count(d_n_kv, n_kv_host, n_kv_max);
    const int c = window_lo(visible(0, n_kv, n_q, causal), vo.window) / C + (int)blockIdx.x;
    const int j0 = c * C;
    if (j0 >= n_kv) return;                                          // (the whole workgroup: no barrier was reached)
    const int64_t off = (int64_t)j0 * nb_pos + (int64_t)hk * nb_head;
    attn_decode_chunk<Q8, D, true, MSK>(lds, q, ldq_tok, ldq_head, kc + off, vc + off, nb_pos, n_head, G, n_q, n_kv, c, (int)blockIdx.x, hk, causal, scale, work,
                                        n_chunks_max, vo, bs);
}

// the paged DECODE kernel: grid (chunks of n_kv_max) x (kv heads) x (sequences).  The sequence's length and the chunk's page id are
// wave-uniform scalars; a workgroup whose chunk lies at or beyond n_kv[b], or whose page id is outside [0, n_pages), leaves before any
// address is formed (the table entry itself is read only for c < ceil(n_kv[b] / 128) <= ld_pages).  Otherwise the chunk body above on
// pool + page * nb_page, with the sequence's own rows of q and of the work buffer.
template <bool Q8, int D>
__global__ __launch_bounds__(256) void attn_decode_paged_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                                const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int n_head, int G, int n_q,
                                                                const kv_pages pg, int len_bias, int causal, float scale, float *__restrict__ work,
                                                                int n_chunks_max) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int c = blockIdx.x, hk = blockIdx.y, b = blockIdx.z;
    const int n_kv = paged_count(pg, b, len_bias);
    if (c * C >= n_kv) return;                                       // (the whole workgroup: no barrier was reached)
    const int page = pg.pages[(int64_t)b * pg.ld_pages + c];
    if (page < 0 || page >= pg.n_pages) return;                      // (the merge writes this sequence's rows as zeros)
    const int64_t off = (int64_t)page * pg.nb_page + (int64_t)hk * nb_head;
    const int64_t row0 = (int64_t)b * n_q;                           // the sequence's first row of q and of the work buffer
    attn_decode_chunk<Q8, D, false>(lds, q + row0 * ldq_tok, ldq_tok, ldq_head, kc + off, vc + off, nb_pos, n_head, G, n_q, n_kv, c, c, hk, causal, scale,
                                    work + row0 * n_head * n_chunks_max * (D + 4), n_chunks_max, attn_var{});
}

// the _ex paged DECODE kernel: chunk c_lo[b] + x of sequence b; table entries below c_lo[b] are never read
template <bool Q8, int D, bool MSK>
__global__ __launch_bounds__(256) void attn_decode_paged_ex_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                                   const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int n_head, int G, int n_q,
                                                                   const kv_pages pg, int len_bias, int causal, float scale, float *__restrict__ work,
                                                                   int n_chunks_max, const attn_var vo, const attn_bias bs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int hk = blockIdx.y, b = blockIdx.z;
    const int n_kv = paged_count(pg, b, len_bias);
    const int c = window_lo(visible(0, n_kv, n_q, causal), vo.window) / C + (int)blockIdx.x;
    if (c * C >= n_kv) return;                                       // (the whole workgroup: no barrier was reached)
    const int page = pg.pages[(int64_t)b * pg.ld_pages + c];         // (c < ceil(n_kv[b] / 128) <= ld_pages)
    if (page < 0 || page >= pg.n_pages) return;                      // (before any address is formed from it; the merge writes zeros)
    const int64_t off = (int64_t)page * pg.nb_page + (int64_t)hk * nb_head;
    const int64_t row0 = (int64_t)b * n_q;
    attn_bias bb = bs;
    if constexpr (MSK) bb.mask += row0 * bs.ld;
    attn_decode_chunk<Q8, D, true, MSK>(lds, q + row0 * ldq_tok, ldq_tok, ldq_head, kc + off, vc + off, nb_pos, n_head, G, n_q, n_kv, c, (int)blockIdx.x, hk, causal,
                                        scale, work + row0 * n_head * n_chunks_max * (D + 4), n_chunks_max, vo, bb);
}

// the merge of one query row (t, h) whose partials start at `part`; thread d owns column d, every thread the row's (M, L)
// VAR: the row's chunks are lo / 128 .. (vis - 1) / 128, at work-buffer index c - c_lo (part points at index 0); head h's sink joins M and L
// MSK: a chunk of the row's range may hold the empty partial (m = -inf, l = 0, a = 0): its b is expf(-inf) = 0 against a finite M and it adds
// nothing; with M = -inf (every chunk empty, no finite sink) the row has no visible position and is +0.0f
template <int D, bool VAR, bool MSK = false>
__device__ __forceinline__ void attn_merge_row(const float *__restrict__ part, int t, int n_q, int n_kv, int causal, float *__restrict__ out, int h,
                                               const attn_var &vo) {
    const int d = threadIdx.x;
    const int vis = visible(t, n_kv, n_q, causal);
    if (vis <= 0) { *out = 0.0f; return; }
    int nc = (vis + C - 1) / C;                                      // <= n_chunks_max: vis <= n_kv <= n_kv_max
    float sink = -__builtin_inff();
    if constexpr (VAR) {
        const int c0 = window_lo(vis, vo.window) / C, c_lo = window_lo(visible(0, n_kv, n_q, causal), vo.window) / C;
        part += (int64_t)(c0 - c_lo) * (D + 4);                      // (c_lo <= c0: the bounds are monotone in t)
        nc -= c0;
        if (vo.sinks) sink = vo.sinks[h];
    }
    float M = part[0];
    for (int c = 1; c < nc; ++c) M = fmaxf(M, part[(int64_t)c * (D + 4)]);
    if constexpr (VAR) if (vo.sinks) M = fmaxf(M, sink);
    if constexpr (MSK) if (M == -__builtin_inff()) { *out = 0.0f; return; }
    float L, A;
    {
        const float m = part[0], b = m == M ? 1.0f : expf(m - M);
        L = part[1] * b; A = part[4 + d] * b;
    }
#pragma unroll 4
    for (int c = 1; c < nc; ++c) {
        const float *p = part + (int64_t)c * (D + 4);
        const float m = p[0], b = m == M ? 1.0f : expf(m - M);
        L = fmaf(p[1], b, L); A = fmaf(p[4 + d], b, A);
    }
    if constexpr (VAR) if (vo.sinks) L = L + (sink == M ? 1.0f : expf(sink - M));
    *out = A / L;
}

// the merge: one workgroup of D threads per query row (t, h)
template <int D>
__global__ __launch_bounds__(D) void attn_merge_kernel(const float *__restrict__ work, int n_chunks_max, int n_head, int n_q, int n_kv_host,
                                                       const int32_t *__restrict__ d_n_kv, int n_kv_max, int causal, float *__restrict__ dst, int64_t ldd_tok,
                                                       int64_t ldd_head) {
    const int t = blockIdx.x / n_head, h = blockIdx.x - t * n_head;
    const int n_kv = device_count(d_n_kv, n_kv_host, n_kv_max);
    attn_merge_row<D, false>(work + (int64_t)blockIdx.x * n_chunks_max * (D + 4), t, n_q, n_kv, causal,
                             dst + (int64_t)t * ldd_tok + (int64_t)h * ldd_head + threadIdx.x, h, attn_var{});
}

template <int D, bool MSK>
__global__ __launch_bounds__(D) void attn_merge_ex_kernel(const float *__restrict__ work, int n_chunks_max, int n_head, int n_q, int n_kv_host,
                                                          const int32_t *__restrict__ d_n_kv, int n_kv_max, int causal, float *__restrict__ dst, int64_t ldd_tok,
                                                          int64_t ldd_head, const attn_var vo) {
    const int t = blockIdx.x / n_head, h = blockIdx.x - t * n_head;
    const int n_kv = device_count(d_n_kv, n_kv_host, n_kv_max);
    attn_merge_row<D, true, MSK>(work + (int64_t)blockIdx.x * n_chunks_max * (D + 4), t, n_q, n_kv, causal,
                                 dst + (int64_t)t * ldd_tok + (int64_t)h * ldd_head + threadIdx.x, h, vo);
}

// 1 where one of the entries [first, ceil(n_kv / 128)) of a sequence's table row lies outside [0, n_pages), the same answer in every thread
// of the workgroup (NT threads; one barrier); no address is formed from an entry.  first: 0, or the _ex kernels' c_lo (entries below it are not read)
template <int NT>
__device__ __forceinline__ int paged_any_invalid(const int32_t *__restrict__ row, int first, int n_kv, int n_pages) {
    const int needed = (n_kv + C - 1) / C;
    int bad = 0;
    for (int c = first + threadIdx.x; c < needed; c += NT) {
        const int id = row[c];
        bad |= (id < 0 || id >= n_pages) ? 1 : 0;
    }
    return __syncthreads_or(bad);
}

// the paged merge: one workgroup per row of all sequences, blockIdx.x = (b * n_q + t) * n_head + h.  It scans the sequence's needed page
// ids first: one invalid id and the row is +0.0f (the partials of that sequence are then not read: some were never written).
template <int D>
__global__ __launch_bounds__(D) void attn_merge_paged_kernel(const float *__restrict__ work, int n_chunks_max, int n_head, int n_q, const kv_pages pg,
                                                             int len_bias, int causal, float *__restrict__ dst, int64_t ldd_tok, int64_t ldd_head) {
    const int bt = blockIdx.x / n_head, h = blockIdx.x - bt * n_head;
    const int b = bt / n_q, t = bt - b * n_q;
    const int n_kv = paged_count(pg, b, len_bias);
    float *out = dst + (int64_t)bt * ldd_tok + (int64_t)h * ldd_head + threadIdx.x;
    if (paged_any_invalid<D>(pg.pages + (int64_t)b * pg.ld_pages, 0, n_kv, pg.n_pages)) { *out = 0.0f; return; }
    attn_merge_row<D, false>(work + (int64_t)blockIdx.x * n_chunks_max * (D + 4), t, n_q, n_kv, causal, out, h, attn_var{});
}

template <int D, bool MSK>
__global__ __launch_bounds__(D) void attn_merge_paged_ex_kernel(const float *__restrict__ work, int n_chunks_max, int n_head, int n_q, const kv_pages pg,
                                                                int len_bias, int causal, float *__restrict__ dst, int64_t ldd_tok, int64_t ldd_head,
                                                                const attn_var vo) {
    const int bt = blockIdx.x / n_head, h = blockIdx.x - bt * n_head;
    const int b = bt / n_q, t = bt - b * n_q;
    const int n_kv = paged_count(pg, b, len_bias);
    float *out = dst + (int64_t)bt * ldd_tok + (int64_t)h * ldd_head + threadIdx.x;
    const int c_lo = window_lo(visible(0, n_kv, n_q, causal), vo.window) / C;
    if (paged_any_invalid<D>(pg.pages + (int64_t)b * pg.ld_pages, c_lo, n_kv, pg.n_pages)) { *out = 0.0f; return; }
    attn_merge_row<D, true, MSK>(work + (int64_t)blockIdx.x * n_chunks_max * (D + 4), t, n_q, n_kv, causal, out, h, vo);
}

// ------------------------------------------------------------------------------------------------ PROMPT form
// LDS: K [C positions][D + 8 halves] (16-byte fragment reads, rows 4 banks apart), V^T [D][C + 4 halves] (8-byte fragment reads, rows 2 banks apart)
template <int D> constexpr int prompt_k_stride() { return 2 * D + 16; }
constexpr int PROMPT_VT_STRIDE = 2 * C + 8;
template <int D> constexpr int prompt_lds() { return C * prompt_k_stride<D>() + D * PROMPT_VT_STRIDE; }

template <bool Q8>
__device__ __forceinline__ f16x8 stage_load8(const uint8_t *row, int d8) {             // elements 8 d8 .. of a cache row in global memory, as f16
    if constexpr (Q8) {
        const uint32_t *b = (const uint32_t *)(row + 36 * (d8 >> 2));
        const float d = __uint_as_float(b[0]);
        const uint32_t w0 = b[1 + 2 * (d8 & 3)], w1 = b[2 + 2 * (d8 & 3)];
        f16x8 o;
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            o[i] = (_Float16)((float)(int)(int8_t)((w0 >> (8 * i)) & 0xFFu) * d);       // (v_cvt_f16_f32: round to nearest even)
            o[4 + i] = (_Float16)((float)(int)(int8_t)((w1 >> (8 * i)) & 0xFFu) * d);
        }
        return o;
    } else {
        return *(const f16x8 *)(row + 16 * d8);
    }
}

// THE BODY of the PROMPT form, shared by the contiguous, the paged and the ragged kernel: query rows 128 tile .. 128 tile + 127 of head h of one
// sequence (q and dst are the sequence's own; tile and h are the caller's -- its blockIdx, or the ragged kernel's tile list) over n_kv positions.
// PAGED: chunk c lies at pool + pages[c] * nb_page (pages: the sequence's table row, its first ceil(n_kv / 128) entries checked by the caller); otherwise at cache + 128 c * nb_pos.  Nothing else knows where a chunk lies.
// VAR (the _ex kernels): a lane's visible range is [lo, vis), the workgroup starts at the chunk of its first row's lo and a wave skips the
// chunks wholly below its first row's lo; the score may be soft-capped; head h's sink joins the denominator after the last chunk.
// MSK (the mask kernels, always with VAR): mrow0 / ld as in attn_decode_chunk.  The lane's positions of register group (ct, i >> 2) are four consecutive
// columns of ITS OWN mask row from column j0 + 32 ct + 8 (i >> 2) + 4 hh (a multiple of 4; ld % 8 == 0 and a 16-byte aligned base: one 8-byte load, read
// only where the first column is below the lane's vis <= n_kv <= ld; all 16 pieces of a chunk are issued before its stage).  -inf: invisible (the element mask); otherwise s = fma(slope_h, mask, s).
template <bool Q8, int D, bool PAGED, bool VAR, bool MSK = false>
__device__ __forceinline__ void attn_prompt_tile(uint8_t *lds, const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                 const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, const int32_t *__restrict__ pages,
                                                 int64_t nb_page, int G, int n_q, int n_kv, int tile, int h, int causal, float scale, float *__restrict__ dst,
                                                 int64_t ldd_tok, int64_t ldd_head, const attn_var &vo, const attn_bias &bs = attn_bias{}) {
    static_assert(!MSK || VAR, "the mask kernels run the VAR bodies");
    constexpr int KS = prompt_k_stride<D>(), VS = PROMPT_VT_STRIDE, NKS = D / 16, NDT = D / 32, NCT = C / 32;
    uint8_t *kst = lds, *vt = lds + C * KS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, r = lane & 31, hh = lane >> 5;
    const int hk = h / G;
    const int q0 = tile * 128, qw = q0 + 32 * wave;                   // the workgroup's and the wave's first query row
    const int tq = min(qw + r, n_q - 1);                             // this lane's query (a lane past n_q computes a copy and stores nothing)
    const int vis = visible(tq, n_kv, n_q, causal);
    const int wg_vis = visible(min(q0 + 127, n_q - 1), n_kv, n_q, causal);         // vis is monotone in t: the workgroup's largest
    const int wave_vis = qw < n_q ? visible(min(qw + 31, n_q - 1), n_kv, n_q, causal) : 0;
    int lo = 0, wave_lo = 0, c_first = 0;                            // lo is monotone in t as vis is: the first row's is the smallest
    if constexpr (VAR) {
        lo = window_lo(vis, vo.window);
        wave_lo = qw < n_q ? window_lo(visible(qw, n_kv, n_q, causal), vo.window) : 0;
        c_first = window_lo(visible(q0, n_kv, n_q, causal), vo.window) / C;
    }
    // Q^T as the B operand: lane (query r, half hh) holds Q[tq][16 ks + 8 hh + i], rounded to f16
    f16x8 qf[NKS];
    {
        const float *qrow = q + (int64_t)tq * ldq_tok + (int64_t)h * ldq_head;
#pragma unroll
        for (int ks = 0; ks < NKS; ++ks) {
            const float4 a = *(const float4 *)(qrow + 16 * ks + 8 * hh), b = *(const float4 *)(qrow + 16 * ks + 8 * hh + 4);
            qf[ks][0] = (_Float16)a.x; qf[ks][1] = (_Float16)a.y; qf[ks][2] = (_Float16)a.z; qf[ks][3] = (_Float16)a.w;
            qf[ks][4] = (_Float16)b.x; qf[ks][5] = (_Float16)b.y; qf[ks][6] = (_Float16)b.z; qf[ks][7] = (_Float16)b.w;
        }
    }
    f32x16 o[NDT];
#pragma unroll
    for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
        for (int i = 0; i < 16; ++i) o[dt][i] = 0.0f;
    const float ninf = -__builtin_inff();
    float m = ninf, l = 0.0f;
    const uint16_t *mrow = nullptr;
    float slope = 1.0f;
    if constexpr (MSK) {
        mrow = bs.mask + (int64_t)tq * bs.ld;
        if (bs.slopes) slope = bs.slopes[h];
    }
    const int nc = (wg_vis + C - 1) / C;
    for (int c = c_first; c < nc; ++c) {
        const int j0 = c * C, cnt = min(C, n_kv - j0);               // (j0 < wg_vis <= n_kv: cnt >= 1)
        if (c > c_first) __syncthreads();                                  // (every wave is done with the previous stage)
        f16x4 mw[NCT][4];                                            // MSK: the 16 8-byte pieces of this lane's mask row under the chunk, in flight under the stage
        if constexpr (MSK) {
            const _Float16 hninf = (_Float16)(-__builtin_inff());
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int col = j0 + 32 * ct + 8 * g + 4 * hh;
                    mw[ct][g] = col < vis ? *(const f16x4 *)(mrow + col) : f16x4{hninf, hninf, hninf, hninf};
                }
        }
        // ---- stage: K rows as they lie, V transposed; 16 bytes of f16 per item, consecutive lanes along a row ----
        {
            const int64_t off = (PAGED ? (int64_t)pages[c] * nb_page : (int64_t)j0 * nb_pos) + (int64_t)hk * nb_head;
            const uint8_t *kb = kc + off, *vb = vc + off;
            for (int i = tid; i < C * (D / 8); i += 256) {
                const int j = i / (D / 8), d8 = i - j * (D / 8);
                f16x8 kv, vv;
                if (j < cnt) {
                    kv = stage_load8<Q8>(kb + (int64_t)j * nb_pos, d8);
                    vv = stage_load8<Q8>(vb + (int64_t)j * nb_pos, d8);
                } else {
#pragma unroll
                    for (int e = 0; e < 8; ++e) { kv[e] = (_Float16)0.0f; vv[e] = (_Float16)0.0f; }
                }
                *(f16x8 *)(kst + j * KS + 16 * d8) = kv;
#pragma unroll
                for (int e = 0; e < 8; ++e) *(_Float16 *)(vt + (8 * d8 + e) * VS + 2 * j) = vv[e];
            }
        }
        __syncthreads();
        if (j0 >= wave_vis) continue;                                // (wave-uniform: nothing of this chunk is visible to the wave's rows)
        if constexpr (VAR) if (j0 + C <= wave_lo) continue;          // (the same below the window of the wave's first row)
        // ---- S^T = K Q^T: tile ct holds positions j0 + 32 ct + row(i, hh) of this lane's query ----
        f32x16 s[NCT];
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int i = 0; i < 16; ++i) s[ct][i] = 0.0f;
#pragma unroll
            for (int ks = 0; ks < NKS; ++ks) {
                const f16x8 a = *(const f16x8 *)(kst + (32 * ct + r) * KS + 2 * (16 * ks + 8 * hh));
                s[ct] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, qf[ks], s[ct], 0, 0, 0);
            }
        }
        // ---- the online softmax of this lane's query; register i of a tile is row (i & 3) + 8 (i >> 2) + 4 hh ----
        float cm = ninf;
        if constexpr (MSK) {                                         // the score first, the cap decided ONCE per chunk (a branch, not 64 selects around tanhf)
            if (vo.cap != 0.0f) {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[ct][i] = vo.cap * tanhf(vo.sc * s[ct][i]);
            } else {
#pragma unroll
                for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                    for (int i = 0; i < 16; ++i) s[ct][i] = scale * s[ct][i];
            }
        }
#pragma unroll
        for (int ct = 0; ct < NCT; ++ct) {
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                const int j = j0 + 32 * ct + (i & 3) + 8 * (i >> 2) + 4 * hh;
                float v;
                if constexpr (MSK) {
                    const float mk = (float)mw[ct][i >> 2][i & 3];       // (exact)
                    v = (j < vis && j >= lo && mk != ninf) ? fmaf(slope, mk, s[ct][i]) : ninf;
                } else if constexpr (VAR) v = (j < vis && j >= lo) ? (vo.cap != 0.0f ? vo.cap * tanhf(vo.sc * s[ct][i]) : scale * s[ct][i]) : ninf;
                else v = j < vis ? scale * s[ct][i] : ninf;
                s[ct][i] = v;
                cm = fmaxf(cm, v);
            }
        }
        cm = fmaxf(cm, __shfl_xor(cm, 32));
        const float mn = fmaxf(m, cm);
        const bool any = mn != ninf;                                 // (false: this query has seen no visible position yet)
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
        // ---- O^T = O^T alpha + V^T P^T: the P tile is the B operand as it stands -- element i of k-step ks is position 16 ks + (i & 3) + 8 (i >> 2) + 4 hh,
        //      and the A operand V^T[d][.] is read at the same positions ----
#pragma unroll
        for (int dt = 0; dt < NDT; ++dt) {
#pragma unroll
            for (int i = 0; i < 16; ++i) o[dt][i] = o[dt][i] * alpha;
#pragma unroll
            for (int ct = 0; ct < NCT; ++ct)
#pragma unroll
                for (int ks = 0; ks < 2; ++ks) {
                    const uint8_t *vrow = vt + (32 * dt + r) * VS + 2 * (32 * ct + 16 * ks + 4 * hh);
                    const f16x4 lo = *(const f16x4 *)vrow, hi = *(const f16x4 *)(vrow + 16);
                    f16x8 a;
                    a[0] = lo[0]; a[1] = lo[1]; a[2] = lo[2]; a[3] = lo[3]; a[4] = hi[0]; a[5] = hi[1]; a[6] = hi[2]; a[7] = hi[3];
                    o[dt] = __builtin_amdgcn_mfma_f32_32x32x16_f16(a, pf[ct][ks], o[dt], 0, 0, 0);
                }
        }
    }
    if constexpr (VAR) {
        if (vo.sinks && m != ninf) {                                 // (a row with no visible position keeps l = 0 and writes +0.0f)
            const float sink = vo.sinks[h], mn = fmaxf(m, sink), alpha = expf(m - mn);
            l = l * alpha + expf(sink - mn);
#pragma unroll
            for (int dt = 0; dt < NDT; ++dt)
#pragma unroll
                for (int i = 0; i < 16; ++i) o[dt][i] = o[dt][i] * alpha;
        }
    }
    // ---- dst[tq][h][d] = O^T[d][query] / l: register i of tile dt is d = 32 dt + (i & 3) + 8 (i >> 2) + 4 hh ----
    if (qw + r < n_q) {
        float *out = dst + (int64_t)tq * ldd_tok + (int64_t)h * ldd_head;
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

template <bool Q8, int D>
__global__ __launch_bounds__(256) void attn_prompt_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                          const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int G, int n_q, int n_kv_host,
                                                          const int32_t *__restrict__ d_n_kv, int n_kv_max, int causal, float scale, float *__restrict__ dst,
                                                          int64_t ldd_tok, int64_t ldd_head) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int n_kv = device_count(d_n_kv, n_kv_host, n_kv_max);
    attn_prompt_tile<Q8, D, false, false>(lds, q, ldq_tok, ldq_head, kc, vc, nb_pos, nb_head, nullptr, 0, G, n_q, n_kv, (int)blockIdx.x, (int)blockIdx.y, causal, scale, dst,
                                          ldd_tok, ldd_head, attn_var{});
}

template <bool Q8, int D, bool MSK>
__global__ __launch_bounds__(256) void attn_prompt_ex_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                             const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int G, int n_q, int n_kv_host,
                                                             const int32_t *__restrict__ d_n_kv, int n_kv_max, int causal, float scale, float *__restrict__ dst,
                                                             int64_t ldd_tok, int64_t ldd_head, const attn_var vo, const attn_bias bs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int n_kv = device_count(d_n_kv, n_kv_host, n_kv_max);
    attn_prompt_tile<Q8, D, false, true, MSK>(lds, q, ldq_tok, ldq_head, kc, vc, nb_pos, nb_head, nullptr, 0, G, n_q, n_kv, (int)blockIdx.x, (int)blockIdx.y, causal, scale, dst,
                                              ldd_tok, ldd_head, vo, bs);
}

// the paged PROMPT kernel: grid (query tiles) x (heads) x (sequences).  The workgroup scans its sequence's needed page ids before its first
// stage; one invalid id and its rows are +0.0f, with no address formed from any entry.  Otherwise the body above, the chunk bases from the table.
// VAR (the _ex kernel): the scan starts at c_lo[b], the chunk of the sequence's row 0's first visible position; the body reads no entry below it
// b, row0, n_q, n_kv: the sequence, its first row of q / dst, its rows and its clamped length; tile, h: the workgroup's query tile and head -- all the
// caller's (the paged kernels: blockIdx and b * n_q; the ragged kernel: its tile list and the index tables)
template <bool Q8, int D, bool VAR, bool MSK = false>
__device__ __forceinline__ void attn_prompt_paged_body(uint8_t *lds, const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                       const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int G, int n_q, const kv_pages &pg, int b,
                                                       int64_t row0, int n_kv, int tile, int h, int causal, float scale, float *__restrict__ dst,
                                                       int64_t ldd_tok, int64_t ldd_head, const attn_var &vo, const attn_bias &bs = attn_bias{}) {
    const int32_t *pages = pg.pages + (int64_t)b * pg.ld_pages;
    float *dst_b = dst + row0 * ldd_tok;
    int c_lo = 0;
    if constexpr (VAR) c_lo = window_lo(visible(0, n_kv, n_q, causal), vo.window) / C;
    if (paged_any_invalid<256>(pages, c_lo, n_kv, pg.n_pages)) {
        const int lane = threadIdx.x & 63, tq = tile * 128 + 32 * (threadIdx.x >> 6) + (lane & 31), hh = lane >> 5;
        if (tq < n_q) {
            float *out = dst_b + (int64_t)tq * ldd_tok + (int64_t)h * ldd_head;
#pragma unroll
            for (int i = 0; i < D / 8; ++i) *(float4 *)(out + 8 * i + 4 * hh) = make_float4(0.f, 0.f, 0.f, 0.f);
        }
        return;
    }
    attn_bias bb = bs;
    if constexpr (MSK) bb.mask += row0 * bs.ld;                      // (the sequence's first mask row, as q)
    attn_prompt_tile<Q8, D, true, VAR, MSK>(lds, q + row0 * ldq_tok, ldq_tok, ldq_head, kc, vc, nb_pos, nb_head, pages, pg.nb_page, G, n_q, n_kv, tile, h, causal, scale,
                                            dst_b, ldd_tok, ldd_head, vo, bb);
}

template <bool Q8, int D>
__global__ __launch_bounds__(256) void attn_prompt_paged_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                                const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int G, int n_q,
                                                                const kv_pages pg, int len_bias, int causal, float scale, float *__restrict__ dst,
                                                                int64_t ldd_tok, int64_t ldd_head) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.z;
    attn_prompt_paged_body<Q8, D, false>(lds, q, ldq_tok, ldq_head, kc, vc, nb_pos, nb_head, G, n_q, pg, b, (int64_t)b * n_q, paged_count(pg, b, len_bias),
                                         (int)blockIdx.x, (int)blockIdx.y, causal, scale, dst, ldd_tok, ldd_head, attn_var{});
}

template <bool Q8, int D, bool MSK>
__global__ __launch_bounds__(256) void attn_prompt_paged_ex_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                                   const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int G, int n_q,
                                                                   const kv_pages pg, int len_bias, int causal, float scale, float *__restrict__ dst,
                                                                   int64_t ldd_tok, int64_t ldd_head, const attn_var vo, const attn_bias bs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int b = blockIdx.z;
    attn_prompt_paged_body<Q8, D, true, MSK>(lds, q, ldq_tok, ldq_head, kc, vc, nb_pos, nb_head, G, n_q, pg, b, (int64_t)b * n_q, paged_count(pg, b, len_bias),
                                             (int)blockIdx.x, (int)blockIdx.y, causal, scale, dst, ldd_tok, ldd_head, vo, bs);
}

// ------------------------------------------------------------------------------------------------ RAGGED
// (ggml_hip_attn_paged_ragged_dev; plan.h plan_attn_ragged has the grids and the layout of the index tables, the header's RAGGED section the statement)
// The paged kernels with each sequence's query count read on the device: launch 1 below turns q_start into the index tables, launches 2 .. 4 are the
// paged DECODE, merge and PROMPT kernels with (sequence, row base, n_q) taken from those tables instead of (blockIdx.z, b * n_q, a host n_q) -- the
// chunk bodies above, called with the sequence's own n_q, so a sequence's rows are bit for bit the uniform paged call's.
constexpr int RAG_NT = 1024, RAG_PER = (int)(ATTN_PAGED_MAX_SEQ / RAG_NT);      // the index workgroup; consecutive sequences per thread

// n_kv of sequence b of a ragged call: clamp(len[b] + (add_q ? n_q : 0) + len_bias, 0, n_kv_max)
__device__ __forceinline__ int ragged_count(const kv_pages &pg, int b, int n_q, int add_q, int len_bias) {
    const int64_t n = (int64_t)pg.len[b] + (add_q ? n_q : 0) + len_bias;
    return (int)(n < 0 ? 0 : n > pg.n_kv_max ? pg.n_kv_max : n);
}

// LAUNCH 1, one workgroup.  Thread e owns sequences 4 e .. 4 e + 3: it reads their bounds (a sequence that is not present counts as empty and its
// bounds are dropped here: seq[b] = (-1, 0, 0, 0)), and two exclusive scans through LDS over the threads give each sequence its first DECODE row slot
// and its first PROMPT tile, both in ascending b.
//   seq[b]    = (first row slot or -1, first packed row, n_q, 0)
//   slots[s]  = (b, t) of row slot s, (-1, -1) for a slot no row has
//   tiles[i]  = (b, tile) in ascending (b, tile); *n_tiles their count (never above max_tiles: plan.h; the clamp costs nothing)
// WHERE THE DECODE ROWS DO NOT ALL FIT under n_dec_rows_max (never with n_dec_rows_max >= min(n_tokens_max, 8 n_seq)) the slots are not a prefix sum:
// thread 0 walks the sequences in ascending b and gives a slot to each one that still fits behind those served before it, so a later, shorter
// sequence is still served.  A DECODE sequence without a slot is skipped by launches 2 and 3; ITS OWNER THREAD HERE writes its rows as +0.0f.
__global__ __launch_bounds__(RAG_NT) void attn_ragged_index_kernel(const kv_ragged rg, int n_dec_rows_max, int max_tiles, int4 *__restrict__ seq,
                                                                   int32_t *__restrict__ n_tiles, int2 *__restrict__ tiles, int2 *__restrict__ slots,
                                                                   float *__restrict__ dst, int64_t ldd_tok, int64_t ldd_head, int n_head, int D) {
    __shared__ int32_t s_dec[RAG_NT], s_til[RAG_NT];
    __shared__ int32_t s_slot[RAG_NT * RAG_PER];                     // in: a sequence's DECODE rows (0: it is not DECODE); out: its first slot or -1
    __shared__ int32_t s_used;
    const int e = threadIdx.x;
    int qs[RAG_PER], nq[RAG_PER];
    int own_d = 0, own_t = 0;
#pragma unroll
    for (int k = 0; k < RAG_PER; ++k) {
        const int b = RAG_PER * e + k;
        qs[k] = 0; nq[k] = 0;
        if (b < rg.n_seq) {
            const int64_t a = rg.q_start[b], z = rg.q_start[b + 1];
            if (a >= 0 && a <= z && z <= rg.n_tokens_max) { qs[k] = (int)a; nq[k] = (int)(z - a); }
        }
        const int dec = nq[k] <= ATTN_DECODE_MAX_Q ? nq[k] : 0;
        s_slot[b] = dec;
        own_d += dec;
        own_t += nq[k] > ATTN_DECODE_MAX_Q ? (nq[k] + 127) / 128 : 0;
    }
    s_dec[e] = own_d; s_til[e] = own_t;
    __syncthreads();
    for (int d = 1; d < RAG_NT; d <<= 1) {
        const int vd = e >= d ? s_dec[e - d] : 0, vt = e >= d ? s_til[e - d] : 0;
        __syncthreads();
        s_dec[e] += vd; s_til[e] += vt;
        __syncthreads();
    }
    const int total_d = s_dec[RAG_NT - 1], total_t = s_til[RAG_NT - 1];
    if (total_d <= n_dec_rows_max) {                                 // (the same answer in every thread) every DECODE sequence fits: the prefix sum
        int d = s_dec[e] - own_d;
#pragma unroll
        for (int k = 0; k < RAG_PER; ++k) {
            const int b = RAG_PER * e + k, dec = s_slot[b];
            s_slot[b] = dec ? d : -1;
            d += dec;
        }
        if (e == 0) s_used = total_d;
    } else if (e == 0) {
        int used = 0;
        for (int b = 0; b < rg.n_seq; ++b) {
            const int dec = s_slot[b];
            const bool fits = dec > 0 && used + dec <= n_dec_rows_max;
            s_slot[b] = fits ? used : -1;
            used += fits ? dec : 0;
        }
        s_used = used;
    }
    __syncthreads();
    int tt = s_til[e] - own_t;
#pragma unroll
    for (int k = 0; k < RAG_PER; ++k) {
        const int b = RAG_PER * e + k, n = nq[k];
        if (b >= rg.n_seq) break;
        const int slot = s_slot[b];
        seq[b] = make_int4(slot, qs[k], n, 0);
        if (n > ATTN_DECODE_MAX_Q) {
            for (int j = 0; j < (n + 127) / 128; ++j, ++tt)
                if (tt < max_tiles) tiles[tt] = make_int2(b, j);
        } else if (slot >= 0) {
            for (int t = 0; t < n; ++t) slots[slot + t] = make_int2(b, t);          // (slot + n <= n_dec_rows_max: it fits)
        } else {
            for (int t = 0; t < n; ++t)                              // a DECODE sequence without a slot: its rows (inside [0, n_tokens_max): it is present) are +0.0f
                for (int h = 0; h < n_head; ++h) {
                    float *out = dst + (int64_t)(qs[k] + t) * ldd_tok + (int64_t)h * ldd_head;
                    for (int d4 = 0; d4 < D / 4; ++d4) *(float4 *)(out + 4 * d4) = make_float4(0.f, 0.f, 0.f, 0.f);
                }
        }
    }
    for (int i = s_used + e; i < n_dec_rows_max; i += RAG_NT) slots[i] = make_int2(-1, -1);
    if (e == RAG_NT - 1) *n_tiles = total_t < max_tiles ? total_t : max_tiles;
}

// LAUNCH 2, the grid of attn_decode_paged_kernel / attn_decode_paged_ex_kernel: (chunks) x (kv heads) x (sequences).  A workgroup whose sequence is
// not DECODE or has no slot leaves before its first barrier; otherwise those kernels' guards and the chunk body with the sequence's own n_q, its
// rows of q from its first packed row and its partials from its first row slot.
template <bool Q8, int D, bool VAR, bool MSK>
__global__ __launch_bounds__(256) void attn_decode_ragged_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                                 const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int n_head, int G,
                                                                 const kv_pages pg, const int4 *__restrict__ seq, int add_q, int len_bias, int causal, float scale,
                                                                 float *__restrict__ work, int n_chunks_max, const attn_var vo, const attn_bias bs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    const int hk = blockIdx.y, b = blockIdx.z;
    const int4 sq = seq[b];
    if (sq.x < 0) return;                                            // (the whole workgroup: no barrier was reached)
    const int n_q = sq.z;
    const int n_kv = ragged_count(pg, b, n_q, add_q, len_bias);
    int c = blockIdx.x;
    if constexpr (VAR) c += window_lo(visible(0, n_kv, n_q, causal), vo.window) / C;
    if (c * C >= n_kv) return;
    const int page = pg.pages[(int64_t)b * pg.ld_pages + c];         // (c < ceil(n_kv[b] / 128) <= ld_pages)
    if (page < 0 || page >= pg.n_pages) return;                      // (before any address is formed from it; the merge writes zeros)
    const int64_t off = (int64_t)page * pg.nb_page + (int64_t)hk * nb_head;
    attn_bias bb = bs;
    if constexpr (MSK) bb.mask += (int64_t)sq.y * bs.ld;             // (the sequence's first packed row, as q)
    attn_decode_chunk<Q8, D, VAR, MSK>(lds, q + (int64_t)sq.y * ldq_tok, ldq_tok, ldq_head, kc + off, vc + off, nb_pos, n_head, G, n_q, n_kv, c, (int)blockIdx.x, hk,
                                       causal, scale, work + (int64_t)sq.x * n_head * n_chunks_max * (D + 4), n_chunks_max, vo, bb);
}

// LAUNCH 3, one workgroup per row slot and head, blockIdx.x = slot * n_head + h: the paged merge (its id scan, its zero row) for the slot's (b, t)
template <int D, bool VAR, bool MSK>
__global__ __launch_bounds__(D) void attn_merge_ragged_kernel(const float *__restrict__ work, int n_chunks_max, int n_head, const kv_pages pg,
                                                              const int4 *__restrict__ seq, const int2 *__restrict__ slots, int add_q, int len_bias, int causal,
                                                              float *__restrict__ dst, int64_t ldd_tok, int64_t ldd_head, const attn_var vo) {
    const int slot = blockIdx.x / n_head, h = blockIdx.x - slot * n_head;
    const int2 bt = slots[slot];
    if (bt.x < 0) return;                                            // (the whole workgroup: the slot holds no row)
    const int4 sq = seq[bt.x];
    const int n_q = sq.z;
    const int n_kv = ragged_count(pg, bt.x, n_q, add_q, len_bias);
    float *out = dst + (int64_t)(sq.y + bt.y) * ldd_tok + (int64_t)h * ldd_head + threadIdx.x;
    int c_lo = 0;
    if constexpr (VAR) c_lo = window_lo(visible(0, n_kv, n_q, causal), vo.window) / C;
    if (paged_any_invalid<D>(pg.pages + (int64_t)bt.x * pg.ld_pages, c_lo, n_kv, pg.n_pages)) { *out = 0.0f; return; }
    attn_merge_row<D, VAR, MSK>(work + (int64_t)blockIdx.x * n_chunks_max * (D + 4), bt.y, n_q, n_kv, causal, out, h, vo);
}

// LAUNCH 4, grid (heads) x (tile bound): a workgroup past the list's length leaves at once, otherwise the paged PROMPT body for its (b, tile).  The heads
// are the grid's x so that the list is walked in dispatch order: every entry past its length comes AFTER the last tile.  With the list on x the
// empty workgroups of one head stood in front of the next head's tiles, each waiting for a whole CU's registers only to leave (measured: DESIGN.md 22).
template <bool Q8, int D, bool VAR, bool MSK>
__global__ __launch_bounds__(256) void attn_prompt_ragged_kernel(const float *__restrict__ q, int64_t ldq_tok, int64_t ldq_head, const uint8_t *__restrict__ kc,
                                                                 const uint8_t *__restrict__ vc, int64_t nb_pos, int64_t nb_head, int G, const kv_pages pg,
                                                                 const int4 *__restrict__ seq, const int2 *__restrict__ tiles, const int32_t *__restrict__ n_tiles,
                                                                 int add_q, int len_bias, int causal, float scale, float *__restrict__ dst, int64_t ldd_tok,
                                                                 int64_t ldd_head, const attn_var vo, const attn_bias bs) {
    extern __shared__ __attribute__((aligned(16))) uint8_t lds[];
    if ((int)blockIdx.y >= *n_tiles) return;
    const int2 bt = tiles[blockIdx.y];
    const int4 sq = seq[bt.x];
    attn_prompt_paged_body<Q8, D, VAR, MSK>(lds, q, ldq_tok, ldq_head, kc, vc, nb_pos, nb_head, G, sq.z, pg, bt.x, (int64_t)sq.y, ragged_count(pg, bt.x, sq.z, add_q, len_bias),
                                            bt.y, (int)blockIdx.x, causal, scale, dst, ldd_tok, ldd_head, vo, bs);
}

// (+ 64: the mask kernels' [DEC_RT][2] first / last positions behind the scores)
template <bool Q8, int D, bool MSK = false> constexpr int decode_lds() { return 2 * C * stage_stride<Q8>(D) + DEC_RT * D * 4 + DEC_RT * C * 4 + (MSK ? 64 : 0); }

}  // namespace

hipError_t launch_kv_store(int kv_type, const float *src, int64_t ld, int64_t n_rows, int64_t row_elems, void *cache, int64_t nb_pos, int64_t n_pos_max,
                           int64_t pos0, const int32_t *d_pos0, hipStream_t st) {
    if (n_rows <= 0) return hipSuccess;
    const bool q8 = kv_type == GGML_TYPE_Q8_0;
    const int64_t upr = row_elems / (q8 ? 32 : 4), total = n_rows * upr;
    if (upr <= 0 || upr > 0x7FFFFFFF || total > (int64_t)0x7FFFFFFF * 256) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (q8) kv_store_kernel<true><<<grid, 256, 0, st>>>(src, ld, n_rows, (int)upr, (uint8_t *)cache, nb_pos, n_pos_max, pos0, d_pos0);
    else kv_store_kernel<false><<<grid, 256, 0, st>>>(src, ld, n_rows, (int)upr, (uint8_t *)cache, nb_pos, n_pos_max, pos0, d_pos0);
    return hipGetLastError();
}

hipError_t launch_kv_store_paged(int kv_type, const float *src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D, int64_t n_seq, int64_t n_q, void *pool,
                                 int64_t nb_pos, int64_t nb_head, const kv_pages &pg, hipStream_t st) {
    const int64_t n_tokens = n_seq * n_q;
    if (n_tokens <= 0) return hipSuccess;
    const bool q8 = kv_type == GGML_TYPE_Q8_0;
    const int64_t uph = D / (q8 ? 32 : 4), total = n_tokens * n_head_kv * uph;
    if (uph <= 0 || n_q > 0x7FFFFFFF || total > (int64_t)0x7FFFFFFF * 256) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (q8) kv_store_paged_kernel<true><<<grid, 256, 0, st>>>(src, ldx_tok, ldx_head, n_head_kv, (int)uph, n_tokens, (int)n_q, (uint8_t *)pool, nb_pos, nb_head, pg);
    else kv_store_paged_kernel<false><<<grid, 256, 0, st>>>(src, ldx_tok, ldx_head, n_head_kv, (int)uph, n_tokens, (int)n_q, (uint8_t *)pool, nb_pos, nb_head, pg);
    return hipGetLastError();
}

hipError_t launch_ragged_positions(const kv_ragged &rg, const int32_t *len, int32_t *pos, hipStream_t st) {
    if (rg.n_tokens_max <= 0) return hipSuccess;
    ragged_positions_kernel<<<dim3((unsigned)((rg.n_tokens_max + 255) / 256)), 256, 0, st>>>(rg, len, pos);
    return hipGetLastError();
}

hipError_t launch_kv_store_paged_ragged(int kv_type, const float *src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D, const kv_ragged &rg, void *pool,
                                        int64_t nb_pos, int64_t nb_head, const kv_pages &pg, hipStream_t st) {
    if (rg.n_tokens_max <= 0) return hipSuccess;
    const bool q8 = kv_type == GGML_TYPE_Q8_0;
    const int64_t uph = D / (q8 ? 32 : 4), total = (int64_t)rg.n_tokens_max * n_head_kv * uph;
    if (uph <= 0 || total > (int64_t)0x7FFFFFFF * 256) return hipErrorInvalidValue;
    const dim3 grid((unsigned)((total + 255) / 256));
    if (q8) kv_store_paged_ragged_kernel<true><<<grid, 256, 0, st>>>(src, ldx_tok, ldx_head, n_head_kv, (int)uph, rg, (uint8_t *)pool, nb_pos, nb_head, pg);
    else kv_store_paged_ragged_kernel<false><<<grid, 256, 0, st>>>(src, ldx_tok, ldx_head, n_head_kv, (int)uph, rg, (uint8_t *)pool, nb_pos, nb_head, pg);
    return hipGetLastError();
}

// every grid and every offset into the work buffer is the plan's (plan_attn_ragged); a launch whose grid the bounds leave empty is not made
// bs: the mask kernels (always the VAR bodies; var is then not read)
hipError_t launch_attn_paged_ragged(const attn_ragged_plan &pl, const attn_args &a, const kv_ragged &rg, const kv_pages &pg, int add_q, int len_bias, bool var,
                                    const attn_var &vo, hipStream_t st, const attn_bias *bs) {
    if (pl.launches == 0) return hipSuccess;
    const bool q8 = a.kv_type == GGML_TYPE_Q8_0;
    const int G = a.n_head / a.n_head_kv;
    const uint8_t *kc = (const uint8_t *)a.k, *vc = (const uint8_t *)a.v;
    uint8_t *w = (uint8_t *)a.work;
    int4 *seq = (int4 *)(w + pl.seq_off);
    int32_t *n_tiles = (int32_t *)(w + pl.n_tiles_off);
    int2 *tiles = (int2 *)(w + pl.tiles_off), *slots = (int2 *)(w + pl.slots_off);
    float *part = (float *)(w + pl.part_off);
    attn_ragged_index_kernel<<<dim3(1), RAG_NT, 0, st>>>(rg, (int)pl.dec_rows, (int)pl.max_tiles, seq, n_tiles, tiles, slots, a.dst, a.ldd_tok, a.ldd_head, a.n_head,
                                                        a.D);
    hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    const attn_bias bv = bs ? *bs : attn_bias{};
#define RAGGED(Q, DD, V, MK)                                                                                                                           \
    do {                                                                                                                                              \
        if (pl.decode_wgs > 0) {                                                                                                                      \
            e = launch_lds(kfn<attn_decode_ragged_kernel<Q, DD, V, MK>>, dim3((unsigned)pl.n_chunks, (unsigned)a.n_head_kv, (unsigned)rg.n_seq), dim3(256), \
                           (size_t)decode_lds<Q, DD, MK>(), decode_lds<Q, DD, MK>(), st, a.q, a.ldq_tok, a.ldq_head, kc, vc, a.nb_pos, a.nb_head, a.n_head, G, pg, \
                           (const int4 *)seq, add_q, len_bias, a.causal, a.scale, part, (int)pl.n_chunks, vo, bv);                                    \
            if (e != hipSuccess) return e;                                                                                                            \
        }                                                                                                                                             \
        if (pl.merge_wgs > 0)                                                                                                                         \
            attn_merge_ragged_kernel<DD, V, MK><<<dim3((unsigned)pl.merge_wgs), DD, 0, st>>>(part, (int)pl.n_chunks, a.n_head, pg, seq, slots, add_q, len_bias, \
                                                                                            a.causal, a.dst, a.ldd_tok, a.ldd_head, vo);              \
        if (pl.prompt_wgs > 0) {                                                                                                                      \
            e = launch_lds(kfn<attn_prompt_ragged_kernel<Q, DD, V, MK>>, dim3((unsigned)a.n_head, (unsigned)pl.max_tiles), dim3(256), (size_t)prompt_lds<DD>(), \
                           prompt_lds<DD>(), st, a.q, a.ldq_tok, a.ldq_head, kc, vc, a.nb_pos, a.nb_head, G, pg, (const int4 *)seq, (const int2 *)tiles, \
                           (const int32_t *)n_tiles, add_q, len_bias, a.causal, a.scale, a.dst, a.ldd_tok, a.ldd_head, vo, bv);                       \
            if (e != hipSuccess) return e;                                                                                                            \
        }                                                                                                                                             \
    } while (0)
#define RAGGED_V(Q, DD)                                                                                                                                \
    do {                                                                                                                                              \
        if (bs) RAGGED(Q, DD, true, true);                                                                                                            \
        else if (var) RAGGED(Q, DD, true, false);                                                                                                     \
        else RAGGED(Q, DD, false, false);                                                                                                             \
    } while (0)
    if (q8 && a.D == 64) RAGGED_V(true, 64);
    else if (q8) RAGGED_V(true, 128);
    else if (a.D == 64) RAGGED_V(false, 64);
    else RAGGED_V(false, 128);
#undef RAGGED_V
#undef RAGGED
    return hipGetLastError();
}

// the grids are the plan's: DECODE pl.n_chunks x kv heads x sequences and one merge workgroup per row; PROMPT query tiles x heads x sequences
// the _ex launches: the same grids from plan_attn_ex / plan_attn_paged_ex (a windowed DECODE grid follows the window), the _ex kernels, vo by value
// bs: null the _ex kernels (MSK = false), otherwise the mask kernels; the same grids
hipError_t launch_attn_paged_ex(const attn_plan &pl, const attn_args &a, int64_t n_seq, const kv_pages &pg, int len_bias, const attn_var &vo, hipStream_t st,
                                const attn_bias *bs) {
    const attn_bias bv = bs ? *bs : attn_bias{};
    const bool q8 = a.kv_type == GGML_TYPE_Q8_0;
    const int G = a.n_head / a.n_head_kv;
    const uint8_t *kc = (const uint8_t *)a.k, *vc = (const uint8_t *)a.v;
    if (pl.form == ATTN_FORM_DECODE) {
        const dim3 grid((unsigned)pl.n_chunks, (unsigned)a.n_head_kv, (unsigned)n_seq);
        float *work = (float *)a.work;
#define DECODE_M(Q, DD, MK)                                                                                                                           \
    do {                                                                                                                                              \
        if (pl.n_chunks > 0) {                                                                                                                        \
            hipError_t e = launch_lds(kfn<attn_decode_paged_ex_kernel<Q, DD, MK>>, grid, dim3(256), (size_t)decode_lds<Q, DD, MK>(), decode_lds<Q, DD, MK>(), st, a.q, \
                                      a.ldq_tok, a.ldq_head, kc, vc, a.nb_pos, a.nb_head, a.n_head, G, (int)a.n_q, pg, len_bias, a.causal, a.scale, work, \
                                      (int)pl.n_chunks, vo, bv);                                                                                      \
            if (e != hipSuccess) return e;                                                                                                            \
        }                                                                                                                                             \
        attn_merge_paged_ex_kernel<DD, MK><<<dim3((unsigned)(n_seq * a.n_q * a.n_head)), DD, 0, st>>>(work, (int)pl.n_chunks, a.n_head, (int)a.n_q, pg, len_bias, \
                                                                                                     a.causal, a.dst, a.ldd_tok, a.ldd_head, vo);     \
    } while (0)
#define DECODE(Q, DD)                                                                                                                                 \
    do {                                                                                                                                              \
        if (bs) DECODE_M(Q, DD, true);                                                                                                                \
        else DECODE_M(Q, DD, false);                                                                                                                  \
    } while (0)
        if (q8 && a.D == 64) DECODE(true, 64);
        else if (q8) DECODE(true, 128);
        else if (a.D == 64) DECODE(false, 64);
        else DECODE(false, 128);
#undef DECODE
#undef DECODE_M
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((a.n_q + 127) / 128), (unsigned)a.n_head, (unsigned)n_seq);
#define PROMPT_M(Q, DD, MK)                                                                                                                            \
    return launch_lds(kfn<attn_prompt_paged_ex_kernel<Q, DD, MK>>, grid, dim3(256), (size_t)prompt_lds<DD>(), prompt_lds<DD>(), st, a.q, a.ldq_tok, a.ldq_head, \
                      kc, vc, a.nb_pos, a.nb_head, G, (int)a.n_q, pg, len_bias, a.causal, a.scale, a.dst, a.ldd_tok, a.ldd_head, vo, bv)
#define PROMPT(Q, DD)                                                                                                                                  \
    do {                                                                                                                                              \
        if (bs) PROMPT_M(Q, DD, true);                                                                                                                \
        else PROMPT_M(Q, DD, false);                                                                                                                  \
    } while (0)
    if (q8 && a.D == 64) PROMPT(true, 64);
    else if (q8) PROMPT(true, 128);
    else if (a.D == 64) PROMPT(false, 64);
    else PROMPT(false, 128);
#undef PROMPT
#undef PROMPT_M
}

hipError_t launch_attn_ex(const attn_plan &pl, const attn_args &a, const attn_var &vo, hipStream_t st, const attn_bias *bs) {
    const attn_bias bv = bs ? *bs : attn_bias{};
    const bool q8 = a.kv_type == GGML_TYPE_Q8_0;
    const int G = a.n_head / a.n_head_kv;
    const uint8_t *kc = (const uint8_t *)a.k, *vc = (const uint8_t *)a.v;
    if (pl.form == ATTN_FORM_DECODE) {
        const dim3 grid((unsigned)pl.n_chunks, (unsigned)a.n_head_kv);
        float *work = (float *)a.work;
#define DECODE_M(Q, DD, MK)                                                                                                                           \
    do {                                                                                                                                              \
        if (pl.n_chunks > 0) {                                                                                                                        \
            hipError_t e = launch_lds(kfn<attn_decode_ex_kernel<Q, DD, MK>>, grid, dim3(256), (size_t)decode_lds<Q, DD, MK>(), decode_lds<Q, DD, MK>(), st, a.q, \
                                      a.ldq_tok, a.ldq_head, kc, vc, a.nb_pos, a.nb_head, a.n_head, G, (int)a.n_q, (int)a.n_kv, a.d_n_kv, (int)a.n_kv_max, \
                                      a.causal, a.scale, work, (int)pl.n_chunks, vo, bv);                                                             \
            if (e != hipSuccess) return e;                                                                                                            \
        }                                                                                                                                             \
        attn_merge_ex_kernel<DD, MK><<<dim3((unsigned)(a.n_q * a.n_head)), DD, 0, st>>>(work, (int)pl.n_chunks, a.n_head, (int)a.n_q, (int)a.n_kv, a.d_n_kv, \
                                                                                       (int)a.n_kv_max, a.causal, a.dst, a.ldd_tok, a.ldd_head, vo);  \
    } while (0)
#define DECODE(Q, DD)                                                                                                                                 \
    do {                                                                                                                                              \
        if (bs) DECODE_M(Q, DD, true);                                                                                                                \
        else DECODE_M(Q, DD, false);                                                                                                                  \
    } while (0)
        if (q8 && a.D == 64) DECODE(true, 64);
        else if (q8) DECODE(true, 128);
        else if (a.D == 64) DECODE(false, 64);
        else DECODE(false, 128);
#undef DECODE
#undef DECODE_M
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((a.n_q + 127) / 128), (unsigned)a.n_head);
#define PROMPT_M(Q, DD, MK)                                                                                                                            \
    return launch_lds(kfn<attn_prompt_ex_kernel<Q, DD, MK>>, grid, dim3(256), (size_t)prompt_lds<DD>(), prompt_lds<DD>(), st, a.q, a.ldq_tok, a.ldq_head, kc, vc, \
                      a.nb_pos, a.nb_head, G, (int)a.n_q, (int)a.n_kv, a.d_n_kv, (int)a.n_kv_max, a.causal, a.scale, a.dst, a.ldd_tok, a.ldd_head, vo, bv)
#define PROMPT(Q, DD)                                                                                                                                  \
    do {                                                                                                                                              \
        if (bs) PROMPT_M(Q, DD, true);                                                                                                                \
        else PROMPT_M(Q, DD, false);                                                                                                                  \
    } while (0)
    if (q8 && a.D == 64) PROMPT(true, 64);
    else if (q8) PROMPT(true, 128);
    else if (a.D == 64) PROMPT(false, 64);
    else PROMPT(false, 128);
#undef PROMPT
#undef PROMPT_M
}

hipError_t launch_attn_paged(const attn_plan &pl, const attn_args &a, int64_t n_seq, const kv_pages &pg, int len_bias, hipStream_t st) {
    const bool q8 = a.kv_type == GGML_TYPE_Q8_0;
    const int G = a.n_head / a.n_head_kv;
    const uint8_t *kc = (const uint8_t *)a.k, *vc = (const uint8_t *)a.v;
    if (pl.form == ATTN_FORM_DECODE) {
        const dim3 grid((unsigned)pl.n_chunks, (unsigned)a.n_head_kv, (unsigned)n_seq);
        float *work = (float *)a.work;
#define DECODE(Q, DD)                                                                                                                                 \
    do {                                                                                                                                              \
        if (pl.n_chunks > 0) {                                                                                                                        \
            hipError_t e = launch_lds(kfn<attn_decode_paged_kernel<Q, DD>>, grid, dim3(256), (size_t)decode_lds<Q, DD>(), decode_lds<Q, DD>(), st, a.q,  \
                                      a.ldq_tok, a.ldq_head, kc, vc, a.nb_pos, a.nb_head, a.n_head, G, (int)a.n_q, pg, len_bias, a.causal, a.scale, work, \
                                      (int)pl.n_chunks);                                                                                              \
            if (e != hipSuccess) return e;                                                                                                            \
        }                                                                                                                                             \
        attn_merge_paged_kernel<DD><<<dim3((unsigned)(n_seq * a.n_q * a.n_head)), DD, 0, st>>>(work, (int)pl.n_chunks, a.n_head, (int)a.n_q, pg, len_bias, \
                                                                                              a.causal, a.dst, a.ldd_tok, a.ldd_head);                \
    } while (0)
        if (q8 && a.D == 64) DECODE(true, 64);
        else if (q8) DECODE(true, 128);
        else if (a.D == 64) DECODE(false, 64);
        else DECODE(false, 128);
#undef DECODE
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((a.n_q + 127) / 128), (unsigned)a.n_head, (unsigned)n_seq);
#define PROMPT(Q, DD)                                                                                                                                  \
    return launch_lds(kfn<attn_prompt_paged_kernel<Q, DD>>, grid, dim3(256), (size_t)prompt_lds<DD>(), prompt_lds<DD>(), st, a.q, a.ldq_tok, a.ldq_head, kc, \
                      vc, a.nb_pos, a.nb_head, G, (int)a.n_q, pg, len_bias, a.causal, a.scale, a.dst, a.ldd_tok, a.ldd_head)
    if (q8 && a.D == 64) PROMPT(true, 64);
    else if (q8) PROMPT(true, 128);
    else if (a.D == 64) PROMPT(false, 64);
    else PROMPT(false, 128);
#undef PROMPT
}

hipError_t launch_attn(const attn_plan &pl, const attn_args &a, hipStream_t st) {
    const bool q8 = a.kv_type == GGML_TYPE_Q8_0;
    const int G = a.n_head / a.n_head_kv;
    const uint8_t *kc = (const uint8_t *)a.k, *vc = (const uint8_t *)a.v;
    if (pl.form == ATTN_FORM_DECODE) {
        const dim3 grid((unsigned)pl.n_chunks, (unsigned)a.n_head_kv);
        float *work = (float *)a.work;
#define DECODE(Q, DD)                                                                                                                                 \
    do {                                                                                                                                              \
        hipError_t e = launch_lds(kfn<attn_decode_kernel<Q, DD>>, grid, dim3(256), (size_t)decode_lds<Q, DD>(), decode_lds<Q, DD>(), st, a.q, a.ldq_tok,  \
                                  a.ldq_head, kc, vc, a.nb_pos, a.nb_head, a.n_head, G, (int)a.n_q, (int)a.n_kv, a.d_n_kv, (int)a.n_kv_max, a.causal, \
                                  a.scale, work, (int)pl.n_chunks);                                                                                  \
        if (e != hipSuccess) return e;                                                                                                                \
        attn_merge_kernel<DD><<<dim3((unsigned)(a.n_q * a.n_head)), DD, 0, st>>>(work, (int)pl.n_chunks, a.n_head, (int)a.n_q, (int)a.n_kv, a.d_n_kv,  \
                                                                                (int)a.n_kv_max, a.causal, a.dst, a.ldd_tok, a.ldd_head);             \
    } while (0)
        if (q8 && a.D == 64) DECODE(true, 64);
        else if (q8) DECODE(true, 128);
        else if (a.D == 64) DECODE(false, 64);
        else DECODE(false, 128);
#undef DECODE
        return hipGetLastError();
    }
    const dim3 grid((unsigned)((a.n_q + 127) / 128), (unsigned)a.n_head);
#define PROMPT(Q, DD)                                                                                                                                  \
    return launch_lds(kfn<attn_prompt_kernel<Q, DD>>, grid, dim3(256), (size_t)prompt_lds<DD>(), prompt_lds<DD>(), st, a.q, a.ldq_tok, a.ldq_head, kc, vc, \
                      a.nb_pos, a.nb_head, G, (int)a.n_q, (int)a.n_kv, a.d_n_kv, (int)a.n_kv_max, a.causal, a.scale, a.dst, a.ldd_tok, a.ldd_head)
    if (q8 && a.D == 64) PROMPT(true, 64);
    else if (q8) PROMPT(true, 128);
    else if (a.D == 64) PROMPT(false, 64);
    else PROMPT(false, 128);
#undef PROMPT
}
