// plan.h -- ONE decision per product: which kernel family and form serves mul_mat(type, M, K, N), and what that fixes.
//
// Every launcher consumes an mm_plan (no second decision inside the .hip files); api.cpp's image / epilogue questions are answered
// from the same plan; ggml_hip_mm_plan (include/ggml_hip_ext.h) hands it to callers and to the CPU test that sweeps
// type x K x N x M and asserts the invariant the multi-GPU path stands on:
//
//     the ORDER OF AN ELEMENT'S ADDITIONS (tree_id) is a function of (type, K, N) -- never of M.
//
// A row shard therefore computes, bit for bit, the matching columns of the unsplit product.  Only the geometry (tile height, tiles
// per workgroup, persistent grids) follows M.  The one stated exception carries a flag: planes beyond 32-bit buffer offsets
// (> 4 GiB per plane) are served by the int8 family whatever the type (MM_FLAG_WIDE).
#pragma once
#include <stdint.h>

enum mm_family {
    MMF_NONE = 0,
    MMF_GEMV_FUSED = 1,   // gemv.hip K2f / K2: INIT + COMPUTE in one launch, N <= 8
    MMF_GEMV_ROWS = 2,    // gemv.hip two-step form on K1's planes (Q4_2 at 9..16 rows where K < 2048; the COMPUTE-only entry for N <= 8)
    MMF_K3S_MX = 3,       // gemm_qmx.hip K3s: stage-free batched decode, MX (Q4_0, Q4_1)
    MMF_K3S_I8 = 4,       // gemm_q8s.hip: the same on the int8 cores (Q8_0, Q5_0, Q5_1 / Q5_K / Q4_K, Q4_2 / Q6_K; r5: Q4_1 from 65 rows)
    // (r5: 3 | 5 for Q4_0 and 4 | 6 are ONE summation tree each -- the same tree_id -- and plan_mul_mat picks between them by M where both serve)
    MMF_K3P_MX = 5,       // gemm_qmp.hip K3p: prompt-sized batches, MX (Q4_0)
    MMF_K3P_I8 = 6,       // gemm_qmp.hip K3p on the int8 cores (Q8_0, Q5_0, Q5_1, Q4_1; r5: Q4_2 and Q6_K in its form)
    MMF_MX = 7,           // gemm_qmx.hip staged forms
    MMF_F16 = 8,          // gemm_q16.hip staged forms
    MMF_I8 = 9,           // gemm_q.hip staged forms
    MMF_DENSE = 10,       // dense.hip tile kernels (f32 fma chain in k order)
    MMF_DENSE_GEMV = 11,  // dense.hip mat-vec form
    MMF_DENSE16 = 12,     // dense16.hip F16 x F32 on the f16 cores
    MMF_DENSE32 = 13,     // dense16.hip K10d: F32 x F32 as split bf16
};

// how K is divided among the partial sums of an element
enum mm_kstyle { MMK_CHAIN = 0, MMK_STAGE_SETS = 1, MMK_RANGES = 2, MMK_WORKERS = 3 };

enum { MM_FLAG_WIDE = 1, MM_FLAG_EPILOGUE_FUSED = 2, MM_FLAG_PERSISTENT = 4, MM_FLAG_Q8K = 8, MM_FLAG_NEEDS_WORK = 16,
       MM_FLAG_MIN_PIECES = 32 /* INIT writes image 0 AND the three bf16 piece planes of d * sum (K3p-int8, min-term types) */,
       MM_FLAG_MIN_PASS = 64 /* Q2_K: the product is the block term; kquants.hip's min pass subtracts the min term behind it */ };

// forms of the staged MX family (gemm_qmx.hip launch_typed): <WMT, WNT, WGM, WGN, KB, FB, KSP, VS>
enum mx_form {
    MXF_256x128 = 0,      // <2,4,4,1,4,2>       unsplit, 8 tiles per wave (the headline form)
    MXF_N32_H64 = 2,      // <1,1,2,1,4,2,4>     up to 32 rows, four-way, 64-row tiles  (1: retired; ggml_hip_mm_plan reports these numbers, so they stay)
    MXF_N32_H32,          // <1,1,1,1,4,2,4>
    MXF_S4_H128,          // <1,2,4,1,4,FB,4>    four-way, 128-row tiles (Q4_0)
    MXF_S4_H64,           // <1,2,2,1,4,FB,4>
    MXF_S4_H32,           // <1,2,1,1,4,FB,4>
    MXF_S2V2_H64,         // <1,2,2,1,4,2,2,2>   four-way tree as two wave groups x two banked passes
    MXF_S2_H128,          // <1,2,4,1,4,2,2>     two-way
    MXF_S2_H64,           // <1,2,2,1,4,2,2>
    MXF_128x128,          // <2,2,2,2,4,2>       unsplit
    MXF_64x64,            // <1,1,2,2,4,2>       unsplit, one tile per wave (Q4_0)
    MXF_128x64,           // <1,2,4,1,4,2>       unsplit
};
// forms of the staged f16 family (gemm_q16.hip): <WMT, WNT, WGM, WGN, KB, KSP>
enum f16_form { F16F_N32_H64 = 0, F16F_N32_H32, F16F_S4_H128, F16F_S4_H64, F16F_S4_H32, F16F_S2_H128, F16F_256x128, F16F_64x64, F16F_128x64 };
// staged int8 family (gemm_q.hip): <IT, JT>
enum i8_form { I8F_64x64 = 0, I8F_128x128 };
// dense16.hip F16 forms
enum d16_form { D16F_S_256x128 = 0, D16F_S_128x128, D16F_S4_H128 = 3 /* (2: retired) */, D16F_S4_H32, D16F_V2_128x128, D16F_S2_128x128, D16F_S2_128x64, D16F_128x128 };
// dense.hip
enum dense_form { DNF_TILE = 0, DNF_BIG = 1, DNF_KSPLIT = 2 /* F32, 5..256 rows (plan.cpp plan_dense): 32 x 32 tiles, K over the workgroup's eight waves */ };

// K3p (gemm_qmp.hip): k-blocks of a wave's scale table -- 80 fit whole (8 waves x 80 x 256 B = the 160 KB of LDS: K <= 20480); beyond that the
// K loop refills slices of at most 78 rows (the int8 loop keeps one spare row behind the last wave's slice), four slices at most (K <= 79872)
constexpr int K3P_TABLE_ROWS = 80, K3P_SLICE_ROWS = 78, K3P_MAX_SLICES = 4;

struct mm_plan {
    int family;           // mm_family
    int image;            // what INIT writes: 0 int8 planes, 1 / 2 f16 images, 3 bf6 image; -1 nothing (fused mat-vec, dense f32 direct);
                          //   32 f16 panels (dense16), 33 split-bf16 panels (dense32)
    int form;             // the family's form number (one template instantiation)
    // ---- what fixes an element's bits: functions of (type, K, N) only ----
    int arith;            // block-term / min-term arithmetic of the family and type
    int ksplit;           // partial sums per element, added in a fixed order at the end
    int kstyle;           // mm_kstyle
    int kunit;            // k-blocks (dense: k-steps) per stage / per range
    // ---- geometry: may follow M ----
    int tile_m, tile_n;   // output tile of a workgroup
    int waves;            // waves per workgroup
    int tiles_per_wave;
    int64_t wgs;          // workgroups launched
    int flags;            // MM_FLAG_*
    // family-specific launch parameters (K3s / K3p / q8s): k-blocks per wave, weight tiles per workgroup
    int nloc, wmt;
};

// the plan of mul_mat(type, M, K, N); ext_type = GGML_HIP_TYPE_Q5_K / _Q4_K for a k-quant weight living in the planar Q5_1 form (type = Q5_1),
// _Q6_K / _Q3_K / _Q2_K for one living in the planar Q4_2 form on int8 planes alone (type = Q4_2; Q2_K: Q6_K's COMPUTE-only plan -- no
// fused mat-vec, so the min pass always finds K1's image -- with MM_FLAG_MIN_PASS).
// one_call = the product is computed by one entry (ggml_hip_mul_mat_dev: the fused mat-vec exists); false = the COMPUTE-only entry.
mm_plan plan_mul_mat(int type, int ext_type, int64_t M, int64_t K, int64_t N, bool one_call = true);
uint32_t plan_tree_id(const mm_plan &p);
// 2..4 matrices of one type and K behind one activation image, in ONE K3s launch (gemm_qmx.hip / gemm_q8s.hip launch_*_multi): family
// MMF_K3S_MX or MMF_K3S_I8 with nloc and wmt set (tile_m = 32 * wmt; wmt 3 only here), or MMF_NONE -- then each matrix runs its own call
mm_plan plan_mul_mat_group(int type, int ext_type, const int64_t *M, const int64_t *Mpad, int n, int64_t K, int64_t N);
// what a K3s plan (single or group) fixes for its launch: the k-block slots a wave keeps in flight (MX: pairs of blocks), whether they rotate
// through a longer range, the rows of a wave's scale table, and the dynamic LDS bytes (the table or the waves' result exchange)
struct k3s_slots { int slots; bool rot; int rows; int lds; };
k3s_slots plan_k3s_slots(const mm_plan &p, int type);
// The grouped, device-routed product of ggml_hip_mul_mat_id_grouped_dev (moe.cpp): P = n_tokens * n_used pairs sorted by expert ON THE DEVICE,
// every expert's segment padded to whole 32-row column tiles, ONE K3s launch over all of them.  The counts are unknown on the host, so
// everything is sized by bounds: at most min(n_expert, P) segments are non-empty and each pads by at most 31 rows --
//     sorted rows <= P + 31 * min(n_expert, P), and their sum is whole tiles: tiles <= floor((P + 31 * min(n_expert, P)) / 32).
// The TREE is that of plan_mul_mat(type, M, K, N = 32) -- the K3s tree, a function of (type, K) alone; the geometry (32-row weight tiles,
// wmt of them per workgroup by the tile bound) is this plan's own.  Served: Q8_0 / Q5_0 / Q4_0 (ext_type 0) where that plan is K3s.
constexpr int64_t MOE_GROUPED_MAX_PAIRS = 1 << 20;
inline int64_t moe_grouped_tiles(int n_expert, int64_t P) { return (P + 31 * (P < n_expert ? P : (int64_t)n_expert)) / 32; }
bool plan_mul_mat_id_grouped_serves(int type, int ext_type, int64_t M, int64_t K);
// family MMF_K3S_I8 / MMF_K3S_MX with nloc, wmt, tile_m = 32 * wmt, tile_n = 32 and wgs = the grid bound (tile bound x weight tile groups),
// or MMF_NONE: not served, P outside 1 .. 2^20, or an activation image of the bounded rows beyond the kernels' 32-bit offsets
mm_plan plan_mul_mat_id_grouped(int type, int ext_type, int64_t M, int64_t K, int n_expert, int64_t P);
// ---- attention over a KV cache (attn.hip; ggml_hip_attn_dev) ----
// The FORM is a function of n_q alone, the CHUNK (positions per partial / per softmax step) of (kv_type, D) alone -- today one constant.
// Neither follows the device, the grid, n_head or n_kv_max, so a query row's bits do not either.
constexpr int ATTN_CHUNK = 128;
// DECODE up to this many query rows: the G * n_q rows that share a kv head ride one pass over its cache on the f32 VALU -- per chunk
// G * n_q * 128 * D * 2 fma against 2 * 128 * row bytes streamed, which at G = 4 stays under the stream's time up to about 8 rows; beyond,
// a 32-row matrix-core tile is at least a quarter full and the PROMPT form takes over.
constexpr int ATTN_DECODE_MAX_Q = 8;
enum attn_form { ATTN_FORM_NONE = 0, ATTN_FORM_DECODE = 1, ATTN_FORM_PROMPT = 2 };
struct attn_plan {
    int form;             // attn_form; NONE: the shape is not served
    int chunk;            // positions per chunk
    int q_tile;           // query rows a workgroup owns (DECODE: all G * n_q rows of its kv head)
    int launches;         // DECODE 2 (partials, merge), PROMPT 1
    int64_t n_chunks;     // ceil(n_kv_max / chunk): DECODE's grid and partial count per row
    int64_t wgs;          // workgroups of the main launch
    size_t work_bytes;    // DECODE: the partials, n_q * n_head * n_chunks * (D + 4) floats; PROMPT 0
};
attn_plan plan_attn(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max);
// ---- the same over a paged cache, n_seq independent sequences of n_q rows each in one call (ggml_hip_attn_paged_dev) ----
// plan_attn(.., n_q, ..) with a sequence dimension on every grid: the form, the chunk, q_tile, launches and n_chunks are plan_attn's (page =
// chunk), wgs and work_bytes are n_seq times its.  NONE where plan_attn says so, for n_seq outside 1 .. ATTN_PAGED_MAX_SEQ (the grids' z),
// and for n_seq * n_q above ATTN_PAGED_MAX_ROWS or n_seq * n_q * n_head above 2^31 - 1 (the merge's grid is one workgroup per row and head).
constexpr int64_t ATTN_PAGED_MAX_SEQ = 4096;
constexpr int64_t ATTN_PAGED_MAX_ROWS = 1 << 20;
attn_plan plan_attn_paged(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max);
// ---- the _ex entries (sliding window, sinks, soft-cap; ggml_hip_attn_ex_dev / ggml_hip_attn_paged_ex_dev) ----
// plan_attn / plan_attn_paged unchanged but for ONE thing: a DECODE call with a window 0 < W < n_kv_max has
// n_chunks = min(ceil(n_kv_max / 128), ceil((W + n_q - 1) / 128) + 1), the chunks the union of its rows' visible ranges can touch (the union is
// W + n_q - 1 positions long and may start anywhere in a chunk), and wgs follows.  work_bytes stays the base plan's: the base work size serves.
attn_plan plan_attn_ex(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max, int64_t window);
attn_plan plan_attn_paged_ex(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max, int64_t window);
// ---- the RAGGED paged call: a query count per sequence, read on the device (ggml_hip_attn_paged_ragged_dev) ----
// Nothing here follows the batch: every grid and size is a function of the host bounds (n_seq, n_tokens_max, n_dec_rows_max, n_kv_max, window).
// FOUR launches: the index (one workgroup), DECODE (n_chunks x kv heads x sequences), the merge (one workgroup per row slot and head), PROMPT
// (heads x max_tiles).  n_chunks is plan_attn's ceil(n_kv_max / 128), under a window 0 < W < n_kv_max plan_attn_ex's bound taken at 8 rows,
// min(ceil(n_kv_max / 128), ceil((W + 7) / 128) + 1): a DECODE sequence has at most 8 rows, whatever the device says.
// max_tiles = attn_ragged_max_tiles: the most PROMPT tiles any batch inside the bounds can hold.  A PROMPT sequence has n >= 9 rows and
// ceil(n / 128) = 1 + (n - 1) / 128 tiles, so with P such sequences over N rows the tiles are P + sum of (n_i - 1) / 128: a sequence is worth a tile
// for 9 rows, its second tile costs 120 more rows (n - 1 from 8 to 128), every further one 128.  Hence P = min(n_seq, N / 9), L = N - 9 P rows left,
// k = min(P, L / 120) second tiles, and max_tiles = P + k + (L - 120 k) / 128.
// THE WORK BUFFER, from its 256-byte aligned base: int32 x 4 [n_seq] (first row slot or -1, first packed row, n_q, 0) at seq_off = 0; the tile
// count, one int32 in 16 bytes, at n_tiles_off; int32 x 2 [max_tiles] (b, tile) at tiles_off; int32 x 2 [n_dec_rows_max] (b, t) or (-1, -1) at
// slots_off; then at part_off (a multiple of 256) the partials, n_dec_rows_max * n_head * ceil(n_kv_max / 128) * (D + 4) floats -- the UNWINDOWED
// chunk count, as the _ex entries size theirs.  work_bytes is the whole; 0 for n_tokens_max = 0 (nothing is launched).
struct attn_ragged_plan {
    int ok;               // 0: not served (plan_attn's rules; n_seq outside 1 .. 4096; n_tokens_max outside 0 .. 2^20 or times n_head above 2^31 - 1;
                          //    n_dec_rows_max outside 0 .. n_tokens_max)
    int chunk, launches;  // 128; 4: the index and every launch below whose grid is not empty (0 for n_tokens_max = 0)
    int64_t dec_rows;     // n_dec_rows_max: the row slots
    int64_t n_chunks;     // DECODE's grid x and the partials' chunk stride
    int64_t max_tiles;    // PROMPT's grid y (<= 4096 + 4096 + 2^20 / 128: inside a grid's y)
    int64_t decode_wgs, merge_wgs, prompt_wgs;
    size_t seq_off, n_tiles_off, tiles_off, slots_off, part_off, work_bytes;
};
int64_t attn_ragged_max_tiles(int64_t n_tokens_max, int64_t n_seq);
attn_ragged_plan plan_attn_ragged(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_tokens_max, int64_t n_dec_rows_max, int64_t n_kv_max,
                                  int64_t window);
// ---- MLA: latent attention over a latent KV cache (mla.hip; ggml_hip_attn_mla_dev / ggml_hip_attn_mla_paged_dev) ----
// Only (D_k, D_v) = (576, 512).  The FORM is a function of n_q alone: SPLIT up to MLA_SPLIT_MAX_Q rows per sequence, WALK above.  Both own tiles of
// MLA_TILE consecutive rows (t * n_head + h) of one sequence and walk the positions in steps of MLA_STEP, two per chunk.  SPLIT cuts the positions into
// spans of MLA_SPAN chunks: grid tiles x n_spans x n_seq, n_spans = ceil(n_kv_max / (128 * MLA_SPAN)), a partial (m, l, O[512]) per (row, span) and a
// merge launch of one workgroup per row.  WALK: grid tiles x 1 x n_seq, no work buffer.  NONE: kv_type, n_head outside 1 .. 256, n_q outside
// 1 .. 2^20, n_kv_max outside 0 .. 2^24, n_seq outside 1 .. 4096, n_seq * n_q above 2^20 or n_seq * n_q * n_head at or above 2^31.
// MLA_SPAN (one of 1, 2, 4, 8): a small span fills the chip at one sequence, a large one keeps the partials small at many.
constexpr int MLA_DK = 576, MLA_DV = 512;
constexpr int MLA_TILE = 64, MLA_STEP = 64;
#ifndef GGML_HIP_MLA_SPAN                     // (a developer build may set 1, 2 or 8 to measure the other values: tools/attn_mla_grid.py)
#define GGML_HIP_MLA_SPAN 4
#endif
constexpr int MLA_SPAN = GGML_HIP_MLA_SPAN;
static_assert(MLA_SPAN == 1 || MLA_SPAN == 2 || MLA_SPAN == 4 || MLA_SPAN == 8, "MLA_SPAN");
constexpr int MLA_SPLIT_MAX_Q = 8;
enum mla_form { MLA_FORM_NONE = 0, MLA_FORM_SPLIT = 1, MLA_FORM_WALK = 2 };
struct mla_plan {
    int form;             // mla_form; NONE: the shape is not served
    int chunk, span;      // positions per chunk; chunks per span (MLA_SPAN, both forms report it)
    int q_tile, step;     // rows a workgroup owns; positions per online-softmax step
    int launches;         // SPLIT 2 (partials, merge), WALK 1
    int64_t n_spans;      // ceil(n_kv_max / (chunk * span)): SPLIT's grid y and partials per row (WALK: the same number, unused)
    int64_t tiles;        // ceil(n_q * n_head / q_tile): grid x
    int64_t wgs;          // workgroups of the main launch
    int64_t merge_wgs;    // SPLIT: n_seq * n_q * n_head; WALK 0
    size_t work_bytes;    // SPLIT: n_seq * n_q * n_head * n_spans * (512 + 4) floats; WALK 0
};
mla_plan plan_attn_mla(int kv_type, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max);
// ---- the SSM entries: causal conv and selective scan over a ragged batch and a pool of state slots (ssm.hip; ggml_hip_ssm_*_ragged_dev) ----
// ONE launch each, grid (x) x (n_seq): a workgroup row per sequence, so a token loop's trip count is uniform over a workgroup.  Nothing follows the
// batch or n_tokens_max.  ok = 0: the shape is not served.
//   conv: one thread per (sequence, channel), 256 channels per workgroup.  1 <= n_ch <= 2^24, d_conv 2 .. 4.  A slot is [d_conv - 1][n_ch] f32.
//   scan: ONE form, sequential over a sequence's tokens, one lane per (sequence, head, p, slice of 16 states).  A state row of N = 16 * slices
//         elements lives in an aligned group of lanes_per_row = the next power of two at or above slices (1, 2, 4, 8, 16; the lanes past `slices` idle),
//         256 / lanes_per_row rows per workgroup.  1 <= n_head <= 2^20, 1 <= P <= 256, N a multiple of 16 up to 256, n_group divides n_head.
//         A slot is [n_head][P][N] f32.
constexpr int64_t SSM_MAX_CHANNELS = 1 << 24;
constexpr int SSM_MAX_HEADS = 1 << 20;
enum ssm_form { SSM_FORM_NONE = 0, SSM_FORM_SEQUENTIAL = 1 };
struct ssm_conv_plan { int ok, launches; size_t state_bytes; int64_t wgs_x, wgs; };
struct ssm_scan_plan { int ok, form, launches, slices, lanes_per_row, rows_per_wg; size_t state_bytes; int64_t wgs_x, wgs; };
ssm_conv_plan plan_ssm_conv(int64_t n_ch, int d_conv, int64_t n_seq);
ssm_scan_plan plan_ssm_scan(int n_head, int P, int N, int n_group, int64_t n_seq);
// ---- the chunked scan (ssm_chunk.hip; ggml_hip_ssm_scan_chunked_ragged_dev): the form is picked PER SEQUENCE from its own count in the call ----
// A sequence of 1 .. seq_max_tokens tokens runs plan_ssm_scan's sequential kernel; a longer one runs in chunks of `chunk` = 64 tokens counted from its
// first row of the call, as matrix products on the f32 MFMA.  chunk and seq_max_tokens follow the SHAPE alone (DESIGN.md section 26 has the measurement),
// so a sequence's bits follow the shape and its own count.  form = SEQUENTIAL (one launch, no work buffer) where no sequence can be chunked: A per state
// (the decay mask would depend on n), P no multiple of 16, or n_tokens_max <= seq_max_tokens.  Else form = CHUNKED, FIVE launches:
//   the sequential kernel          plan_ssm_scan's grid; sequences above seq_max_tokens leave at once
//   index  (1 workgroup of 1024)   q_start -> the chunked sequences (b, first chunk, chunks) and the chunk list (b, chunk of b), clamped at seqs_max / chunks_max
//   state  (n_head * p_tiles, chunks_max)   per (chunk, head, P tile of p_tile rows): delta, cs, and the chunk's own state contribution at its end
//   pass   (ceil(n_head P N / 1024), seqs_max)   per (sequence, 4 state elements), over the sequence's chunks: H_in of each chunk, the final state into the slot
//   out    (n_head * p_tiles, chunks_max)   per (chunk, head, P tile): y from H_in and the masked intra-chunk products
// p_tile: 64 where it divides P, else 32, else 16; the state and out kernels are compiled once per p_tile (kernel_state = kernel_out = p_tile).
// seqs_max = min(n_seq, n_tokens_max / (seq_max_tokens + 1)) chunked sequences fit in n_tokens_max rows; k such sequences of n_i rows have
// sum (1 + (n_i - 1) / chunk) <= k + (n_tokens_max - k) / chunk chunks, which grows with k: chunks_max is that at k = seqs_max.
// THE WORK BUFFER from its 256-byte aligned base, every part at a multiple of 256: int32 x 4 (chunks, chunked sequences, 0, 0) at hdr_off = 0;
// int32 x 4 [seqs_max] at seqs_off; int32 x 2 [chunks_max] at list_off; f32 [chunks_max][n_head][2][chunk] (cs, delta) at csd_off;
// f32 [chunks_max][n_head][P][N] at state_off (the chunk's contribution, then in place its H_in).  Nothing in it is read before the call writes it.
constexpr int SSM_CHUNK = 64;
constexpr int SSM_CHUNK_SEQ_MAX_TOKENS = 44;
enum { SSM_FORM_CHUNKED = 2 };
struct ssm_chunk_plan {
    int ok, form, chunk, seq_max_tokens, launches, p_tile, p_tiles, kernel_state, kernel_out;
    int64_t chunks_max, seqs_max, pass_wgs_x;
    size_t hdr_off, seqs_off, list_off, csd_off, state_off, work_bytes;
    ssm_scan_plan seq;
};
ssm_chunk_plan plan_ssm_chunk(int n_head, int P, int N, int n_group, int a_per_state, int64_t n_seq, int64_t n_tokens_max);
// ---- the tiled conv (ssm_conv_tile.hip; ggml_hip_ssm_conv_tiled_ragged_dev): the form is picked PER SEQUENCE from its own count in the call ----
// A sequence of 1 .. seq_max_tokens tokens runs plan_ssm_conv's sequential kernel; a longer one runs in tiles of `tile` = T tokens counted from its first
// row of the call, one thread per (tile, `vec` adjacent channels).  The statement is a fixed fma chain per token, so the tiled form is bit for bit the
// sequential one and a sequence may be split over calls and forms at any point.  tile and seq_max_tokens follow the SHAPE alone (here: nothing at all;
// DESIGN.md section 27 has the measurement).  form = SEQUENTIAL (one launch, no work buffer) where n_tokens_max <= seq_max_tokens; else form = TILED,
// FOUR launches:
//   the sequential kernel          plan_ssm_conv's grid; sequences above seq_max_tokens leave at once
//   index  (1 workgroup of 1024)   q_start -> the tile list (b, tile of b) and the count of long sequences, clamped at tiles_max / seqs_max
//   edges  (tiles_max, ceil(n_ch / (256 vec)))   per (tile, vec channels): the d_conv - 1 rows in front of the tile into the work buffer -- from x, or for a
//                                  sequence's first tile from the slot (zeros where fresh), and then THE SAME THREAD moves the sequence's last
//                                  d_conv - 1 rows of x into the slot.  The only kernel of the form that touches slots; it only reads x
//   tile   (tiles_max, ceil(n_ch / (256 vec)))   per (tile, vec channels; vec = 4 where n_ch, the strides and the pointers allow 16-byte moves, else 1): the window starts from the work buffer, then streams the tile's rows x -> dst
// (a grid's y is capped at 32768 workgroups; the kernels step over the channel blocks by gridDim.y.)
// INVARIANTS: tile >= d_conv - 1 (the rows in front of a later tile lie inside the sequence) and seq_max_tokens >= d_conv - 1 (a long sequence's new slot
// is all x), both for the largest d_conv, 4.  seqs_max = min(n_seq, n_tokens_max / (seq_max_tokens + 1)) long sequences fit in n_tokens_max rows; k such
// sequences of n_i rows have sum (1 + (n_i - 1) / tile) <= k + (n_tokens_max - k) / tile tiles, which grows with k: tiles_max is that at k = seqs_max.
// So tiles_max and seqs_max bound every batch of non-overlapping sequences inside n_seq and n_tokens_max; the index kernel clamps the others.
// THE WORK BUFFER from its 256-byte aligned base: int32 x 4 (tiles, long sequences, 0, 0) at hdr_off = 0; int32 x 2 [tiles_max] at list_off;
// f32 [tiles_max][d_conv - 1][halo_ld] at halo_off, halo_ld = n_ch rounded up to 4.  Nothing in it is read before the call writes it.
constexpr int SSM_CONV_TILE = 16;
constexpr int SSM_CONV_SEQ_MAX_TOKENS = 135;
static_assert(SSM_CONV_TILE >= 3 && SSM_CONV_SEQ_MAX_TOKENS >= 3, "a tile and a short sequence hold at least d_conv - 1 rows");
enum { SSM_FORM_TILED = 2 };
struct ssm_conv_tiled_plan {
    int ok, form, tile, seq_max_tokens, launches, vec;
    int64_t tiles_max, seqs_max, halo_ld;
    size_t hdr_off, list_off, halo_off, work_bytes;
    ssm_conv_plan seq;
};
ssm_conv_tiled_plan plan_ssm_conv_tiled(int64_t n_ch, int d_conv, int64_t n_seq, int64_t n_tokens_max);
// the K1 image INIT writes for a plan: its image where that is one of K1's (0 .. 3; else 0), + ACT_IMAGE_MIN_PIECES under MM_FLAG_MIN_PIECES
int plan_act_image(const mm_plan &p);
// the K1 image for (type, K, N) with no weight at hand: plan_act_image of the COMPUTE-only plan at M = 1 (no M: the exception cannot apply)
int plan_image_kind(int type, int64_t K, int64_t N);
// thread-local test switch (ggml_hip_debug_force_gemm): 0 auto, 1 int8, 2 f16, 3 MX
int plan_force_gemm();
void plan_set_force_gemm(int which);
