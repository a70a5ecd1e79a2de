/*
 * ggml_hip_ext.h -- the rest of libggml_hip.so's C-ABI: what goes beyond the drop-in core of ggml_hip.h (SURVEY.md 8(f) "next"
 * rows and the multi-device forms).  A host that only wants GGML_OP_MUL_MAT on the GPU needs ggml_hip.h alone.
 *   - named / output-only graph scopes, counters                       (ggml_hip_graph_begin_keyed, _graph_outputs, _debug_*_counters)
 *   - introspection and the explicit INIT step                          (ggml_hip_act_image_kind, ggml_hip_quantize_act_dev)
 *   - neighbours of the path and their fused forms                      (ggml_hip_compute_forward_{cpy,add,mul,scale,rms_norm,silu,...})
 *   - device-level fused / grouped products                             (ggml_hip_norm_mul_mat_dev, _mul_mat_multi_dev, _mul_mat_epilogue_dev, ...)
 *   - several devices in one process, one process per device           (ggml_hip_split_weight_*, _mul_mat_split_dev, _ipc_*, _push_columns_dev, ...)
 *   - the extension weight types: k-quants, IQ4, BF16                  (GGML_HIP_TYPE_* below; one row each in csrc/wtypes.cpp says what the library does with an id)
 *   - expert-routed products of a mixture-of-experts layer             (ggml_hip_expert_set_*, ggml_hip_mul_mat_id_*)
 *   - attention over a KV cache, contiguous and paged, and its options  (ggml_hip_attn_dev, _attn_paged_dev; sliding window, sinks, soft-cap: _attn_ex_dev, _attn_paged_ex_dev;
 *     a query count per sequence on the device: _attn_paged_ragged_dev and its stores)
 *   - TEST HOOKS (ggml_hip_debug_*): inert unless called; ggml_hip_debug_force_gemm acts on the CALLING THREAD only.
 */
#ifndef GGML_HIP_EXT_H
#define GGML_HIP_EXT_H

#include "ggml_hip.h"

#ifdef __cplusplus
extern "C" {
#endif
#if defined(__GNUC__)
#pragma GCC visibility push(default)   /* the library is built with -fvisibility=hidden: the two headers ARE its export list */
#endif

/* EXTENSION, not a reference type: the reference's enum stops at Q8_1 / I32 (TypeDefs:153-169) and holds no k-quants
 * (SURVEY 8(a) row K), while BASELINE.json's north_star and config 4 name Q5_K.  Built to the PUBLISHED upstream format
 * (ggml k_quants, 2023-06: 176-byte super-blocks of 256 weights; activations by the Q8_K rule) as an unpinned extra: no oracle
 * exists in the reference, tests/np_kquants.py restates the published algorithm.  Accepted by ggml_hip_weight_upload /
 * _from_device / _download, ggml_hip_mul_mat{,_init,_compute}_dev, ggml_hip_mul_mat_work_size,
 * ggml_hip_dequantize_rows_dev and (r4) ggml_hip_quantize_rows_dev (quantize_row_q5_K_reference / _q4_K_reference of the published
 * format restated: make_qkx1_quants per sub-block, 6-bit scales / mins against the super-block's d / dmin) only -- never inside a ggml_tensor (the reference cannot express the type). */
#define GGML_HIP_TYPE_Q5_K 113
/* r4: Q4_K of the same published format -- { half d; half dmin; u8 scales[12]; u8 qs[128] }, 144 bytes per 256 weights, the super-block of
 * Q5_K without its fifth-bit bytes and with the same scale / min packing and the same dot rule against Q8_K.  It lives in the same resident
 * form (eight k-blocks of the planar Q5_1 form, fifth-bit plane zero) and runs the same kernels; the same "unpinned extra" status. */
#define GGML_HIP_TYPE_Q4_K 112
/* r4: Q6_K of the same published format -- { u8 ql[128]; u8 qh[64]; i8 scales[16]; half d }, 210 bytes per 256 weights: sixteen sub-blocks
 * of 16 six-bit weights (q - 32) with a signed 8-bit scale each, no min.  Resident as eight k-blocks of the planar Q4_2 form (two scales per
 * k-block) on int8 operand planes; served by the int8 kernels that take two scales per k-block (its own mat-vec, the batched-decode form and
 * the staged int8 form: WHICH one serves a shape is ggml_hip_mm_plan's answer, the only authority -- no range is restated here).  ggml_hip_quantize_rows_dev: quantize_row_q6_K_reference WITHOUT the least-squares refinement of the
 * sub-block scales (make_qx_quants in its plain form) -- a valid encoder of the published structure.  Unpinned like the other two. */
#define GGML_HIP_TYPE_Q6_K 114
/* Q3_K of the same published format -- { u8 hmask[32]; u8 qs[64]; u8 scales[12]; half d }, 110 bytes per 256 weights: sixteen sub-blocks
 * of 16 three-bit weights v = q2 + 4 hbit - 4 (element e: n = e / 128, s = (e % 128) / 32, l = e % 32; q2 = bits 2 s, 2 s + 1 of qs[32 n + l],
 * hbit = bit 4 n + s of hmask[l]) with a 6-bit scale each (sc_j = code - 32: low nibble of scales[j] (j < 8) / high nibble of scales[j - 8],
 * high two bits 2 (j / 4), 2 (j / 4) + 1 of scales[8 + j % 4]), no min; y = (d * sc_j) * v.  A Q3_K super-block IS a Q6_K one with q6 = v + 32
 * and scales[j] = sc_j, so it lives in Q6_K's resident form byte for byte and runs the same kernels; its 14 header bytes are kept for the
 * download.  ggml_hip_quantize_rows_dev: quantize_row_q3_K_reference of the published format (make_q3_quants with its weighted refinement,
 * 6-bit scales against d = max scale / -32).  Accepted by the same entries as the other three; unpinned like them. */
#define GGML_HIP_TYPE_Q3_K 111
/* Q2_K of the same published format -- { u8 scales[16]; u8 qs[64]; half d; half dmin }, 84 bytes per 256 weights: sixteen sub-blocks of 16
 * two-bit weights q (element e: n = e / 128, s = (e % 128) / 32, l = e % 32; q = bits 2 s, 2 s + 1 of qs[32 n + l]) with a 4-bit scale
 * sc_j = scales[j] & 15 and a 4-bit min m_j = scales[j] >> 4 each (j = e / 16); y = (d * sc_j) * q - dmin * m_j.  The block term is a Q6_K
 * super-block (q6 = q + 32, scales[j] = sc_j, the same d), so a Q2_K weight lives in Q6_K's resident form and runs Q6_K's kernels, never its
 * fused mat-vec; the min term, sum over super-blocks of (dy * dmin) * sum_j m_j * bsum_j against the Q8_K activations, is subtracted from
 * the product by one pass of its own (plan flag GGML_HIP_PLAN_MIN_PASS, its arithmetic in kquants.hip).  scales[16], d and dmin are kept per
 * super-block for the download and the pass.  ggml_hip_quantize_rows_dev: quantize_row_q2_K_reference of the published format
 * (make_qkx1_quants per sub-block, 4-bit scales / mins against d = max scale / 15 and dmin = max min / 15).  Accepted by the same entries as
 * Q3_K; unpinned like the others. */
#define GGML_HIP_TYPE_Q2_K 110
/* IQ4_NL of the published upstream format (upstream id 20 + 100) -- { half d; u8 qs[16] }, 18 bytes per 32 weights: element j < 16 is the
 * low nibble of qs[j], element j + 16 its high nibble, each a 4-bit index into the codebook
 *     kv = { -127, -104, -83, -65, -49, -35, -22, -10, 1, 13, 25, 38, 53, 69, 89, 113 }   (upstream kvalues_iq4nl)
 * and y = d * kv[idx].  After the lookup a block IS a Q8_0 block of this library (f32 d = the half d, exact; qs[j] = kv[idx_j]): the weight
 * lives in Q8_0's resident form, is a plain Q8_0 weight to the plan and to every kernel (its product is bitwise the product of the
 * transcoded Q8_0 weight, activations by Q8_0's rule, where upstream multiplies IQ4_NL against Q8_0 too) and reaches every entry a Q8_0
 * weight reaches; ggml_hip_weight_type, the download (every bit pattern of d comes back) and the size queries report IQ4_NL.  K % 32.
 * ggml_hip_quantize_rows_dev: upstream quantize_row_iq4_nl_impl without importance weights, ntry = 7, restated below.  Unpinned: the
 * reference has no IQ types and no upstream source exists here; this text and tests/np_iq4.py are the yardstick. */
#define GGML_HIP_TYPE_IQ4_NL 120
/* IQ4_XS of the same published family (upstream id 23 + 100) -- { half d; u16 scales_h; u8 scales_l[4]; u8 qs[128] }, 136 bytes per 256
 * weights, little-endian: sub-block ib < 8 has the code ls = ((scales_l[ib / 2] >> 4 (ib % 2)) & 15) | (((scales_h >> 2 ib) & 3) << 4),
 * its 32 elements on qs[16 ib .. 16 ib + 15] in IQ4_NL's nibble order, y = (d * (ls - 32)) * kv[idx] with the product d * (ls - 32) formed
 * first (exact in f32: 11 + 6 significant bits).  A super-block is eight k-blocks of Q6_K's resident form with both per-16 scales of a
 * k-block equal to d * (ls - 32): Q6_K's plan and kernels serve it, activations by the Q8_K rule as upstream's; its 8 header bytes are kept
 * for the download.  K % 256.  Accepted by the entries that accept Q3_K; unpinned like IQ4_NL.
 * ggml_hip_quantize_rows_dev for both (IQ4_NL: super block = block = 32; IQ4_XS: super block 256, block 32).  Every step is ONE binary32
 * operation in the order written, subnormals kept, nearest(x) = round half to even:
 *     best_index(x): x <= kv[0] -> 0; x >= kv[15] -> 15; else ml = 0, mu = 15, while mu - ml > 1 { mav = (ml + mu) / 2;
 *                    x < kv[mav] ? mu = mav : ml = mav }; return x - kv[mu - 1] < kv[mu] - x ? mu - 1 : mu
 *     per block b of 32 (xb): w[j] = xb[j] * xb[j]; amax, max = the largest |xb[j]| and its signed value, the FIRST (strict >, from 0);
 *         if amax < 1e-15f: scale[b] = 0, next block;  d = -max / kv[0]; id = 1 / d;
 *         sumqx = sumq2 = 0; for j: q = kv[best_index(id * xb[j])]; sumqx += (w[j] * q) * xb[j]; sumq2 += (w[j] * q) * q;
 *         d = sumqx / sumq2; best = d * sumqx;
 *         for itry = -7 .. 7: id = (float)(itry + kv[0]) / max; the sums again; if sumq2 > 0 && sumqx * sumqx > best * sumq2:
 *             d = sumqx / sumq2; best = d * sumqx
 *         scale[b] = d; max_scale = the scale[b] of largest |.| (the first, strict >, from 0)
 *     IQ4_XS: D = -max_scale / 32; d = half(D) (round to nearest even); iD = D != 0 ? 1 / D : 0; per b: l = clamp(nearest(iD * scale[b]),
 *             -32, 31); dl = D * l; idl = dl != 0 ? 1 / dl : 0; L[j] = best_index(idl * xb[j]); ls = l + 32
 *     IQ4_NL: d = half(scale[0]); i = scale[0] != 0 ? 1 / scale[0] : 0; L[j] = best_index(i * x[j])
 *     Non-finite intermediates: where |x| exceeds about 1.8e18, w * q * q overflows and a block's fit gives sumqx / sumq2 = inf / inf,
 *     a NaN scale.  It never becomes max_scale (strict >), nearest(NaN) is 0 (what upstream's nearest_int gives), so an IQ4_XS sub-block
 *     with a NaN scale gets ls = 32 and every index 8; an IQ4_NL block stores a NaN d (its sign and payload are not specified) and every
 *     index 15 (best_index(NaN)).
 *     qs[j] = L[j] | L[j + 16] << 4 per 32 elements
 * (so an all-zero IQ4_NL block is d = +0 with every qs byte 0x88, an all-zero IQ4_XS super-block d = 0x8000 -- -0 from -0.0f / 32 --,
 * scales_h = 0xAAAA, scales_l = 0 and every qs byte 0x88).  Both types are never inside a ggml_tensor. */
#define GGML_HIP_TYPE_IQ4_XS 123
/* BF16 weights (upstream GGML_TYPE_BF16 = 30; the k-quants' rule "upstream id + 100"): block 1, 2 bytes per element, the upper half of an
 * IEEE f32.  The product is upstream's BF16 rule, dst = sum_k bf16(w) * bf16(x): src1 is rounded to bf16 in every kernel form (the mat-vec
 * included), each product is exact in f32 and the sum is accumulated in f32 -- the same deviation from the reference's f64 sum as F16 has.
 * Every f32 -> bf16 conversion (src1, ggml_hip_quantize_rows_dev) is ONE rule, that of upstream's current ggml_compute_fp32_to_bf16: for f32
 * bits u, a NaN ((u & 0x7fffffff) > 0x7f800000) becomes (u >> 16) | 0x0040 (quiet, sign kept); any other value (u + 0x7fff + ((u >> 16) & 1))
 * >> 16, round to nearest even, subnormals KEPT and overflow to +-inf.  (An early upstream revision flushed subnormals to zero; this does not.)
 * bf16 -> f32 is bits << 16, exact.  Resident as a row-major bf16 copy (mat-vec, tile kernel, byte-exact download) and the k-panels of F16,
 * 4 B per weight; served by bf16 twins of the F16 kernels (the v_mfma_*_bf16 forms where F16 runs its matrix-core forms), planned as F16 is
 * with arithmetic labels (tree_ids) of its own.  Accepted by the entries that accept an F16 weight (ggml_hip_weight_upload / _from_device /
 * _download, ggml_hip_mul_mat_dev, _work_size, ggml_hip_mm_plan, ggml_hip_act_image_kind, the split weight) and by
 * ggml_hip_quantize_rows_dev / ggml_hip_dequantize_rows_dev (f32 rows -> bf16 rows by the rule above, and back); refused with F16's error
 * code wherever F16 is refused.  Never inside a ggml_tensor: the reference's enum cannot express it. */
#define GGML_HIP_TYPE_BF16 130


/* OPT-IN, and a deviation from the reference's contract (which leaves EVERY node's data in host memory, Ggml.cs:3539-3704):
 * called inside an open scope, before its nodes, it names the tensors (by data pointer) whose data the caller will read after
 * ggml_hip_graph_end; no other result of the scope is copied to the host -- its host memory keeps whatever it held.  The
 * library still copies what IT needs on the host (a buffer that is recycled, a source it has to upload again).  At prompt-sized
 * batches the copies are the whole cost of a graph: 7B decoder layer at batch 512, 4.26 ms with every node's data, see DESIGN 8
 * with the last node's only.  The key of a named scope must cover the list (the host mirror never calls this). */
int  ggml_hip_graph_outputs(const void *const *host_ptrs, int n);
/* The same scope, NAMED: `key` (non-zero) identifies the graph the caller is about to run -- a hash over what decides the
 * calls it will make: every node's op, the data pointers, types, ne / nb of the node and of its sources, and the scalar
 * operands it reads on the host (the factor of a SCALE node).  Inside a scope the seams cost the host one kernel launch per
 * node and the device -> host copies of all results go out together at the end; a named scope that needed nothing else is
 * captured into a hipGraph the second time it is seen and replayed with ONE launch from the third time on (the seams
 * return at once; leaf tensors are re-read from host memory by the captured copies, so their CONTENTS may change between
 * runs -- a decoder's token loop).  Everything the key covers must be unchanged when a key is reused; a weight that is
 * rewritten must be invalidated as always (ggml_hip_invalidate*), which also drops the captured scopes.  One device slot
 * only; with several the call is ggml_hip_graph_begin.  (7B decoder layer at batch 1 through ggml_graph_compute: 439 us per
 * graph with per-node copies, 97 us in a plain scope, see DESIGN 8 for the replayed figure.) */
int  ggml_hip_graph_begin_keyed(uint64_t key);
/* Named scopes so far by what became of them: observed clean, captured, replayed, refused (tests, tuning). */
void ggml_hip_debug_scope_counters(uint64_t *observed, uint64_t *captured, uint64_t *replayed, uint64_t *refused);
/* Bytes moved over PCIe by seam 1 so far and the number of src1 operands served from a resident dst (tests, tuning). */
void ggml_hip_debug_transfer_counters(uint64_t *h2d_bytes, uint64_t *d2h_bytes, uint64_t *resident_hits);
/* The Seam-1 weight cache (device forms of leaf src0 tensors, keyed by host pointer + shape; Ggml.cs:1545: tensor data is stable for the
 * life of its context).  It is bounded by the device's memory: when an upload cannot be allocated, least-recently-used entries are evicted
 * and the upload is tried once more.  _budget sets a smaller bound per slot in bytes (0 = none) so that a test can watch the eviction happen
 * on a small problem -- the entry the running call uses always stays; _stats reports entries, resident bytes and evictions so far. */
void ggml_hip_debug_weight_cache_budget(size_t bytes_per_slot);
void ggml_hip_debug_weight_cache_stats(uint64_t *entries, uint64_t *bytes, uint64_t *evictions);


/* Which layout step 1 writes into d_work for this weight type, K and N (introspection for tests and profiling tools):
 * 0 = int8 planes (mat-vec and int8-MFMA kernels), 1 / 2 = f16 images (gemm_q16.hip), 3 = bf6 digit image (gemm_qmx.hip).
 * A function of the type, K and N ONLY -- never of the number of weight rows -- so a row shard runs the kernel form of the
 * unsplit matrix (what makes a shard's result bit for bit the matching columns).  The one exception is stated, not hidden: a
 * weight whose planes do not fit 32-bit buffer offsets (more than 4 GiB per plane) takes kind 0 whatever this says. */
int    ggml_hip_act_image_kind(int type, int64_t K, int64_t N);
/* THE PLAN of mul_mat(type, M, K, N) as ggml_hip_mul_mat_dev will run it (csrc/plan.cpp: the one place where a product's kernel is decided;
 * every launcher consumes the same structure).  No device is needed to ask.  What the row split over several GPUs stands on
 * (Ggml.cs:6665-6672: contiguous row ranges, each computed independently) is visible here and tested without a GPU:
 *     tree_id -- the ORDER OF AN ELEMENT'S ADDITIONS (arithmetic form of a block term and of the min term, number of partial sums, how K is
 *     divided among them) -- is a function of (type, K, N) and never of M,
 * so a row shard computes, bit for bit, the matching columns of the unsplit product; family / form / tiles may follow M.  The one
 * exception carries GGML_HIP_PLAN_WIDE: planes beyond 32-bit buffer offsets (> 4 GiB per plane) are served by the int8 family. */
enum {  /* ggml_hip_mm_plan_t.family */
    GGML_HIP_MMF_GEMV_FUSED = 1, GGML_HIP_MMF_GEMV_ROWS = 2, GGML_HIP_MMF_K3S_MX = 3, GGML_HIP_MMF_K3S_I8 = 4, GGML_HIP_MMF_K3P_MX = 5,
    GGML_HIP_MMF_K3P_I8 = 6, GGML_HIP_MMF_MX = 7, GGML_HIP_MMF_F16 = 8, GGML_HIP_MMF_I8 = 9, GGML_HIP_MMF_DENSE = 10,
    GGML_HIP_MMF_DENSE_GEMV = 11, GGML_HIP_MMF_DENSE16 = 12, GGML_HIP_MMF_DENSE32 = 13
};
enum {  /* ggml_hip_mm_plan_t.flags */
    GGML_HIP_PLAN_WIDE = 1,            /* the 32-bit-offset exception applied */
    GGML_HIP_PLAN_EPILOGUE_FUSED = 2,  /* an add / scale node behind the product runs in the kernel's store phase */
    GGML_HIP_PLAN_PERSISTENT = 4, GGML_HIP_PLAN_Q8K = 8,
    GGML_HIP_PLAN_NEEDS_WORK = 16,     /* the product needs a work buffer of ggml_hip_mul_mat_work_size bytes */
    GGML_HIP_PLAN_MIN_PIECES = 32,     /* INIT writes image 0 AND the bf16 piece planes of d * sum (K3p-int8 behind Q5_1 / Q4_1 / Q5_K): image_kind 0 + 64 */
    GGML_HIP_PLAN_MIN_PASS = 64        /* Q2_K: the per-16 min term is subtracted by a pass of its own behind the product (tree_id mixes it in) */
};
typedef struct ggml_hip_mm_plan_t {
    int32_t  family, image_kind, form;       /* which kernel, what INIT writes (-1 nothing, 0..3 K1's images, 0 + 64 image 0 with the min-term piece planes, 32 / 33 dense panels), which instantiation */
    uint32_t tree_id;                        /* hash of (arith, ksplit, kstyle, kunit): what fixes an element's bits */
    int32_t  arith, ksplit, kstyle, kunit;   /* kstyle: 0 one chain over K, 1 stage sets taken in turn, 2 contiguous ranges, 3 interleaved workers */
    int32_t  tile_m, tile_n, waves, tiles_per_wave;
    int64_t  workgroups;
    int32_t  flags;
} ggml_hip_mm_plan_t;
int    ggml_hip_mm_plan(int type, int64_t M, int64_t K, int64_t N, ggml_hip_mm_plan_t *out);
/* TEST HOOK, per calling thread (a host thread that never calls it is never affected): which matrix-core kernel serves
 * N > 8 on THIS thread's calls -- 0 automatic (by type, N and K), 1 int8 MFMA
 * (gemm_q.hip), 2 f16 MFMA (gemm_q16.hip), 3 MX (gemm_qmx.hip; for Q5_0 / Q8_0 its two-digit form, which needs the
 * weight to have been uploaded while 3 was in force -- the digit planes are not built otherwise).  Same results within
 * the documented tolerance whichever runs. */
void   ggml_hip_debug_force_gemm(int which);
/* TEST HOOK: the Q2_K min pass alone -- d_dst[n][i] -= the min term (GGML_HIP_PLAN_MIN_PASS) against the image ggml_hip_mul_mat_init_dev
 * wrote into d_work for this weight and N.  form: 0 the form ggml_hip_mul_mat_compute_dev runs, 1 / 2 one / two 32-column tiles per wave
 * (the same bits whichever runs).  GGML_HIP_ERR_TYPE for any other weight type. */
int    ggml_hip_debug_q2k_min_pass_dev(const ggml_hip_weight *w, int64_t N, float *d_dst, int64_t ldd, const void *d_work, size_t work_bytes,
                                       int form, void *stream);
/* 1: ggml_hip_mul_mat_dev (that entry alone; mode 0 of ggml_hip_mul_mat_epilogue_dev is that entry) quantizes src1 INSIDE the product launch for this
 * weight and N -- Q4_0 on 256 x 128 tiles in one round of workgroups, K four equal quarters of exactly eight 4-k-block stages each (3968 < K <= 4096:
 * the headline's K; shorter K, and K = 8192, measured level with or behind the two steps and decline): a head launch writes the image of the first K quarter, the product launch writes the other three a
 * quarter ahead of its own K loop.  The work buffer ends up holding the bytes ggml_hip_mul_mat_init_dev writes (image and scale planes) and dst the
 * bits of ggml_hip_mul_mat_compute_dev; the part of the image region the bf6 image leaves free holds the launch's hand-off masks.  0: the two steps. */
int    ggml_hip_mul_mat_init_fused(const ggml_hip_weight *w, int64_t N);
/* TEST HOOK (process-wide): on the fused route, the workgroups of src1 column panel `panel` (128 rows each) do not write their shares of the image,
 * so every workgroup of that panel takes the help path (it quantizes the missing shares itself).  -1: off.  Same bytes, same bits.  ONE value for the
 * whole process, read when a product is launched -- a graph captured while it is set keeps it; not for use beside concurrent callers. */
void   ggml_hip_debug_fused_init_skip_panel(int panel);
/* Step 1 alone with an explicit layout: every src1 row -> Q8_0 (quantize_row_q8_0, Ggml.cs:733-762, the loop of
 * Ggml.cs:6641-6654) written as image `image_kind` (see above) into d_work.  image_kind + 16 (kinds 0..2, K % 256 == 0):
 * the Q8_K rule of the k-quant extension instead (one scale per 256 elements; see GGML_HIP_TYPE_Q5_K).  image_kind + 64 (kind 0 only,
 * K >= 256): beside image 0, d * (float)sum(q) of every block -- the Q8_1 s0 + s1 of Ggml.cs:820-821 -- as three bf16 pieces that sum to it
 * exactly, in the half of the image region image 0 leaves free (same work size): what ggml_hip_act_image_kind returns for Q5_1 / Q4_1
 * weights wherever the min terms run as a matrix product of their own (gemm_qmp.hip, gemm_q8s.hip; the row ranges are the plan's --
 * ask ggml_hip_act_image_kind / ggml_hip_mm_plan, they are not restated here). */
int    ggml_hip_quantize_act_dev(const float *d_src1, int64_t N, int64_t K, int64_t ld1, void *d_work, size_t work_bytes,
                                 int image_kind, void *stream);

/* ---------------- neighbours of the path (SURVEY.md 8(f) "next") ----------------
 * ggml_compute_forward_cpy -> ggml_compute_forward_dup_f32 / _dup_f16, quantizing branch (Ggml.cs:8659-8663,
 * 4339-4363, 3935-3966): src0 F32 or F16 with contiguous rows, dst a contiguous Q4_0 / Q4_1 / Q4_2 / Q5_0 / Q5_1 / Q8_0 tensor with
 * the same element count.  This is the only public way to produce a quantized tensor in the reference; on the device
 * it uses the intended quantize_row_q4_0 (== _reference), not the broken AVX packNibbles path.
 * Same offload convention as Seam 1 (acts for ith == 0, COMPUTE phase). */
int ggml_hip_compute_forward_cpy(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                 struct ggml_tensor *dst);
/* ggml_compute_forward_add for a quantized src0 = ggml_compute_forward_add_q_f32 (Ggml.cs:4797-4906):
 * dst row = quantize_row_q(dequantize_row_q(src0 row) + src1 row); src1 F32, dst the type and shape of src0;
 * for an F32 src0 = ggml_compute_forward_add_f32 (Ggml.cs:4622-4682), same-shape contiguous operands, bit-exact. */
int ggml_hip_compute_forward_add(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                 const struct ggml_tensor *src1, struct ggml_tensor *dst);
/* The f32 element-wise neighbours of mul_mat in a transformer block; contiguous F32 tensors, same
 * offload convention as Seam 1; inside a graph scope operands and results stay in HBM (see ggml_hip_graph_begin).
 *   mul      ggml_compute_forward_mul_f32      Ggml.cs:5007-5035   dst = src0 * src1, same shape           (bit-exact)
 *   scale    ggml_compute_forward_scale_f32    Ggml.cs:6746-6778   dst *= *(float *)src1->data, IN PLACE: dst is a view
 *                                                                  of src0 (ggml_scale_impl Ggml.cs:8265)     (bit-exact)
 *   rms_norm ggml_compute_forward_rms_norm_f32 Ggml.cs:5858-5920   y = x / sqrt(mean(x^2) + 1e-6), squares summed in f64
 *                                                                  (only the order of the f64 additions differs) */
int ggml_hip_compute_forward_mul(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                 const struct ggml_tensor *src1, struct ggml_tensor *dst);
int ggml_hip_compute_forward_scale(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                   const struct ggml_tensor *src1, struct ggml_tensor *dst);
int ggml_hip_compute_forward_rms_norm(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                      struct ggml_tensor *dst);
/*   silu     ggml_compute_forward_silu_f32     Ggml.cs:5705-5748   the GGML_SILU_FP16 build (GGMLSharp.csproj:9): argument
 *                                                                  rounded to half, y = half(silu(x)) widened; the table
 *                                                                  of Ggml.cs:1455-1471 indexed by bit pattern (SURVEY A2,
 *                                                                  intent).  In-place form (ggml_silu_inplace): dst is a
 *                                                                  view of src0.                              (bit-exact) */
int ggml_hip_compute_forward_silu(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                  struct ggml_tensor *dst);
/* ---------------- fused neighbours (adjacent ops as prologues / epilogues of mul_mat) ----------------
 * Two graph nodes served by one call; BOTH nodes' data are produced (the reference's contract: every node's data is in host
 * memory after ggml_graph_compute), each value by the reference's own operation sequence -- bit for bit what the separate
 * seams give.  The host's node loop (Ggml.cs:3539-3704) calls one of these for node i and skips node i + 1 when it sees the
 * pair; every pair has the unfused seams as its fallback.
 *   rms_norm_mul   norm_dst = rms_norm(x), mul_dst = norm_dst * g                 one launch (fused.hip)
 *   silu_mul       silu_dst = silu(a),     mul_dst = silu_dst * b  (SwiGLU gate)  one launch (fused.hip)
 *   norm_mul_mat   the three (or, with an add node, four) nodes rms_norm, mul, mul_mat [, add] as ONE launch for N <= 4
 *   mul_mat_add    mm_dst = mul_mat(src0, src1), add_dst = mm_dst + addend        the add is applied to the accumulators in
 *   mul_mat_scale  mm_dst = scale_dst = mul_mat(src0, src1) * scalar (in place)   the store phase of the mat-mul kernels
 * (epilogue forms exist in the fused mat-vec, the MX mat-mat forms, the batched-decode forms and K3p; whether the form that serves a
 * given (weight, N) has one is ggml_hip_mul_mat_epilogue_fused's answer -- the plan's MM_FLAG_EPILOGUE_FUSED -- and elsewhere the node's
 * own kernel runs behind the mat-mul inside the same call). */
int ggml_hip_compute_forward_rms_norm_mul(const struct ggml_compute_params *params, const struct ggml_tensor *x,
                                          const struct ggml_tensor *g, struct ggml_tensor *norm_dst, struct ggml_tensor *mul_dst);
int ggml_hip_compute_forward_silu_mul(const struct ggml_compute_params *params, const struct ggml_tensor *a,
                                      const struct ggml_tensor *b, struct ggml_tensor *silu_dst, struct ggml_tensor *mul_dst);
int ggml_hip_compute_forward_mul_mat_add(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                         const struct ggml_tensor *src1, struct ggml_tensor *mm_dst,
                                         const struct ggml_tensor *addend, struct ggml_tensor *add_dst);
int ggml_hip_compute_forward_mul_mat_scale(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                           const struct ggml_tensor *src1, struct ggml_tensor *mm_dst,
                                           const struct ggml_tensor *scalar, struct ggml_tensor *scale_dst);
/* rms_norm -> mul -> mul_mat [-> add]: the norm in front of a projection and the residual behind it, for decode-sized
 * batches ONE launch (x: the norm's operand, g: the mul's other operand; addend / add_dst NULL when no add node follows) */
int ggml_hip_compute_forward_norm_mul_mat(const struct ggml_compute_params *params, const struct ggml_tensor *x,
                                          const struct ggml_tensor *g, struct ggml_tensor *norm_dst, struct ggml_tensor *mul_dst,
                                          const struct ggml_tensor *src0, struct ggml_tensor *mm_dst,
                                          const struct ggml_tensor *addend, struct ggml_tensor *add_dst);
/* Several MUL_MAT nodes with the SAME src1 (the q / k / v or gate / up projections), optionally with the rms_norm -> mul pair
 * that produces that src1 in front (pro_x / pro_g / pro_norm as x / g / norm_dst above, src1 = the mul node; NULL: no pair):
 * ONE launch inside a graph scope for batches of up to 4 rows when every src0 is a cached quantized leaf of one type and K;
 * otherwise the nodes run through their own seams one after the other.  Every node's data is produced either way. */
int ggml_hip_compute_forward_mul_mat_multi(const struct ggml_compute_params *params, int n, const struct ggml_tensor *const *src0,
                                           const struct ggml_tensor *src1, struct ggml_tensor *const *dst,
                                           const struct ggml_tensor *pro_x, const struct ggml_tensor *pro_g,
                                           struct ggml_tensor *pro_norm);
/* Device form of the prologue + epilogue: d_norm = rms_norm(d_x), d_y = d_norm * d_g (both [N][K] contiguous), then the
 * product of w and d_y with the epilogue `mode` (0 none).  ggml_hip_norm_mul_mat_fused: 1 when it is one launch. */
int ggml_hip_norm_mul_mat_dev(const ggml_hip_weight *w, const float *d_x, int64_t ld_x, const float *d_g, int64_t ld_g, int64_t N,
                              float *d_norm, float *d_y, float *d_dst, int64_t ldd, void *d_work, size_t work_bytes, int mode,
                              const float *d_addend, int64_t ld_add, float *d_dst2, int64_t ldd2, float scale, void *stream);
int ggml_hip_norm_mul_mat_fused(const ggml_hip_weight *w, int64_t N);
/* Several weight matrices behind ONE activation matrix -- the q / k / v or the gate / up projections of a transformer block
 * (each its own MUL_MAT node with the same src1, Ggml.cs:6714) -- as one launch for N <= 4: 2..4 resident matrices of one
 * quantized type and K; dst[i] receives matrix i's product ([N][M_i], row stride ldd[i]); every row is bit for bit what
 * ggml_hip_mul_mat_dev gives.  With d_g the launch also computes the rms_norm -> mul pair in front (d_src1 is then the
 * norm's input x; d_norm / d_y receive both nodes' data, as in ggml_hip_norm_mul_mat_dev).  ggml_hip_mul_mat_multi_fused
 * says whether the form exists for these matrices and N (else: one call per matrix). */
int ggml_hip_mul_mat_multi_fused(const ggml_hip_weight *const *w, int n_w, int64_t N);
int ggml_hip_mul_mat_multi_dev(const ggml_hip_weight *const *w, int n_w, const float *d_src1, int64_t ld1, int64_t N,
                               float *const *d_dst, const int64_t *ldd, const float *d_g, int64_t ld_g, float *d_norm,
                               float *d_y, void *stream);
/* The same for a batch of any size, with the scratch a batch needs (ggml_hip_mul_mat_work_size(type, K, N) bytes): src1 is
 * quantized once -- the INIT phase (Ggml.cs:6641-6654) is the same for every matrix of one type and K -- and the 1..4 matrices
 * follow, in ONE launch where the library has the form (5 <= N <= 64, Q4_0 / Q4_1, K >= 2048: three 4096-row projections fill
 * the chip that one of them half uses), else one COMPUTE after the other behind the shared image.  Every row is bit for bit
 * what ggml_hip_mul_mat_dev gives for that matrix. */
int ggml_hip_mul_mat_multi_work_dev(const ggml_hip_weight *const *w, int n_w, const float *d_src1, int64_t ld1, int64_t N,
                                    float *const *d_dst, const int64_t *ldd, void *d_work, size_t work_bytes, void *stream);
/* The pair kernel alone on contiguous device rows: d_norm = rms_norm(d_x) (Ggml.cs:5858-5920), d_y = d_norm * d_g. */
int ggml_hip_rms_norm_mul_rows_dev(const float *d_x, const float *d_g, float *d_norm, float *d_y, int64_t nrows, int64_t k, void *stream);
/* Device form of the epilogue: mode 1 add (d_dst keeps the product, d_dst2 = product + d_addend), mode 2 scale (d_dst =
 * product * scale), mode 0 = ggml_hip_mul_mat_dev. */
int ggml_hip_mul_mat_epilogue_dev(const ggml_hip_weight *w, const float *d_src1, int64_t N, int64_t ld1, float *d_dst, int64_t ldd,
                                  void *d_work, size_t work_bytes, int mode, const float *d_addend, int64_t ld_add, float *d_dst2,
                                  int64_t ldd2, float scale, void *stream);
int ggml_hip_mul_mat_epilogue_fused(const ggml_hip_weight *w, int64_t N);   /* 1: the kernel form serving N applies it itself */

/* Device forms.  src_type F32 or F16; source rows ld elements apart; blocks of all rows contiguous. */
int ggml_hip_quantize_rows_src_dev(int type, int src_type, const void *d_x, int64_t ld, int64_t nrows, int64_t k,
                                   void *d_blocks, void *stream);
int ggml_hip_add_q_f32_rows_dev(int type, const void *d_blocks_in, const float *d_x, int64_t nrows, int64_t k,
                                void *d_blocks_out, void *stream);

/* ---------------- several devices, one process (SURVEY 8(b) "n_devices", 8(e)) ----------------
 * Row split of one weight matrix over the device slots with the reference's thread partition (Ggml.cs:6665-6672: dr =
 * ceil(M / G), slot g owns rows [dr*g, min(dr*(g+1), M))).  ggml_hip_mul_mat_split_dev: d_src1[g] / d_dst[g] are slot g's
 * device buffers (src1 [N][ld1] replicated, dst [N][ldd >= M]); every slot computes its rows on its own stream and writes
 * them as columns [r0, r1) of ITS dst (the kernels take a row stride: no [G][N][Ms] intermediate, no re-layout pass); the
 * exchange then completes every slot's dst.  Stream-ordered on the slots' streams: ggml_hip_sync_slots() waits.
 * Exchange forms (ggml_hip_set_exchange): 0 = peer DMA over xGMI, one strided 2-D copy per (slot, peer) -- the default;
 * 1 = RCCL ncclAllGather of contiguous shards + the re-layout kernel below (librccl is loaded at run time; needs distinct
 * devices); 2 (r4) = no exchange pass: every slot's GEMM stores its rows into EVERY slot's dst from its own store phase
 * (ggml_hip_mul_mat_push_dev below; needs every device to reach every other's memory, else the call runs form 0).  All three only
 * move data: identical bits.  Every element equals the single-device result bit for bit (the kernel form is a function of N, K and
 * the type, never of M). */
typedef struct ggml_hip_split_weight ggml_hip_split_weight;
int  ggml_hip_split_weight_upload(int type, const void *host_rows, int64_t ne00, int64_t ne01, uint64_t nb01,
                                  ggml_hip_split_weight **out);
void ggml_hip_split_weight_free(ggml_hip_split_weight *w);
int  ggml_hip_split_weight_rows(const ggml_hip_split_weight *w, int slot, int64_t *row_begin, int64_t *row_end);
int  ggml_hip_mul_mat_split_dev(const ggml_hip_split_weight *w, const float *const *d_src1, int64_t N, int64_t ld1,
                                float *const *d_dst, int64_t ldd);
int  ggml_hip_set_exchange(int mode);
int  ggml_hip_sync_slots(void);
int  ggml_hip_debug_rccl_selftest(void);             /* the RCCL exchange form on slot 0 alone (one rank), bytes checked */
/* Device memory of a slot for hosts without their own HIP binding (the C# host): plain hipMalloc / hipMemcpy. */
void *ggml_hip_slot_malloc(int slot, size_t bytes);
void  ggml_hip_slot_free(int slot, void *p);
int   ggml_hip_slot_upload(int slot, void *d_dst, const void *host_src, size_t bytes);
int   ggml_hip_slot_download(int slot, void *host_dst, const void *d_src, size_t bytes);
/* One process PER device, direct exchange (ggmlsharp_amd/dist.py, exchange "push"): every rank allocates its reference-
 * layout dst [N][M] with ggml_hip_ipc_alloc, ships the 64-byte handle to its peers (any transport), opens theirs, and after
 * computing its rows stores them as columns [col0, col0 + Ms) of EVERY rank's dst with one kernel (d_peers: HOST array of
 * n_peers <= 16 device pointers, NULL entries skipped; compute units store over xGMI, one hop, all links at once, final
 * layout -- SURVEY 8(e) "epilogue peer-writes").  The caller orders consumers behind a barrier of its own. */
int ggml_hip_ipc_alloc(size_t bytes, void **d_ptr, uint8_t *handle64);
int ggml_hip_ipc_open(const uint8_t *handle64, void **d_ptr);
int ggml_hip_ipc_close(void *d_ptr);
int ggml_hip_ipc_free(void *d_ptr);
int ggml_hip_push_columns_dev(const float *d_shard, int64_t lds, int64_t N, int64_t Ms, float *const *d_peers, int n_peers,
                              int64_t ldd, int64_t col0, void *stream);
/* The product AND the exchange in one call (r4; SURVEY 8(e): "epilogue peer-writes straight into each peer's final [N][M] buffer"):
 * this rank's rows of W (Ggml.cs:6665-6672) against all of src1, every element stored as column col0 + m of EVERY rank's reference-layout
 * dst [N][ld_total] (Ggml.cs:6692-6697).  d_peers: HOST array of n_peers <= 16 device pointers to the buffers' BASES, this rank's own at
 * index `own`, NULL entries skipped.  Where the kernel form that serves this weight at N rows has the store-phase exchange -- the staged MX
 * forms, K3p and (r5) the batched-decode forms, up to 8 destinations: ggml_hip_mul_mat_push_fused says so -- the GEMM's store phase writes to all of them (no shard pass, no
 * second launch); otherwise the product lands in this rank's buffer and ggml_hip_push_columns_dev's kernel follows.  Same bytes either
 * way.  The caller orders consumers behind a barrier of its own. */
int ggml_hip_mul_mat_push_dev(const ggml_hip_weight *w, const float *d_src1, int64_t N, int64_t ld1, float *const *d_peers, int n_peers,
                              int own, int64_t ld_total, int64_t col0, void *d_work, size_t work_bytes, void *stream);
int ggml_hip_mul_mat_push_fused(const ggml_hip_weight *w, int64_t N, int n_peers);
/* One process PER device (torch.distributed / RCCL ranks, ggmlsharp_amd/dist.py): after an all-gather of per-rank dst
 * shards ([G][N][Ms], rank-major) produce the reference layout [N][G*Ms -> M] (SURVEY.md 8(e) "layout catch"); rows of
 * the last rank beyond M are dropped. */
int ggml_hip_relayout_gathered_dev(const float *d_gathered, int G, int64_t N, int64_t Ms, float *d_dst,
                                   int64_t M, int64_t ldd, void *stream);

/* ---------------- expert-routed products: upstream's ggml_mul_mat_id (a mixture-of-experts layer) ----------------
 * EXTENSION: the reference has no such node, so there is no seam and no host mirror for it -- a device-resident entry like the
 * multi-weight and push entries.  Upstream's shapes: as [K, M, n_expert], b [K, n_used or 1, n_tokens], ids [n_used, n_tokens],
 * dst [M, n_used, n_tokens].  A PAIR is p = t * n_used + s (token t, slot s) and
 *     dst[p * ldd + m] = sum_k deq(W[ids[p]][m, k]) * q(X[t * ld1_token + s * ld1_slot + k])
 * with this library's arithmetic for the type (Q8_0 / Q8_1 / Q8_K activations, exact block dots, the type's f32 scale statement).
 * ld1_slot = 0 is upstream's broadcast (gate / up: one src1 row per token); a non-zero stride is the down projection's own row per slot.
 * No epilogue and no prologue on this entry.
 *
 * The EXPERT SET: 2 <= n_expert <= 1024 resident weights on ONE device with the same type, ext_type, up_type, K and M (else
 * GGML_HIP_ERR_ARG / _SHAPE).  The set owns a small device table of each expert's plane pointers and NOT the weights: every weight must
 * outlive the set (freeing a weight before the set is the caller's error).  Weights uploaded whole or as row shards alike: a set of row
 * shards [r0, r1) of every expert computes columns [r0, r1) of the whole set's result, bit for bit, on both routes.
 *
 * TWO ROUTES, a function of the set and the shape alone -- never of the routing, n_expert or n_used (ggml_hip_mul_mat_id_route; the twin
 * _route_for / _work_size_for answer for (type, M, K) with no weight and no device at hand, like ggml_hip_mm_plan, and the set's entries
 * are the same function of the set's type, M and K):
 *   1  the by-id mat-vec: n_tokens <= 4 and the plan of mul_mat(type, M, K, N = 1) is the fused mat-vec (GGML_HIP_MMF_GEMV_FUSED).  ONE
 *      launch, no host synchronize, no allocation, no work buffer (work size 0): the kernel reads d_ids[p] and takes that expert's
 *      pointers from the set's table, so the call can be captured and replayed with other ids in d_ids.  h_ids is not read.  Pair p's M
 *      outputs are bit for bit ggml_hip_mul_mat_dev(expert ids[p], the row of p, N = 1).
 *   2  the batch route, every other case and every weight type: the pairs are counting-sorted by expert (ascending p inside an expert),
 *      their src1 rows gathered into expert-contiguous order in d_work, the planned product of ggml_hip_mul_mat_dev run per non-empty
 *      expert on its contiguous batch (Q2_K's min pass and the Q8_K rule come along), and the [count_e][M] results scattered to dst[p].
 *      Pair p's outputs are bitwise what ggml_hip_mul_mat_dev(expert e, its gathered batch, N = count_e) returns for that row: the
 *      summation tree is a function of (type, K, count_e), as upstream's is of the batch.  The launch sizes need the counts on the HOST:
 *      with h_ids (the same n_tokens * n_used ids in host memory) the call is asynchronous on `stream` -- the sort is host work and the
 *      gather / scatter maps travel inside their launches, so the call may be captured (the routing is then part of the graph); with
 *      h_ids == NULL d_ids is copied back with ONE synchronize of `stream`, and on a capturing stream that is GGML_HIP_ERR_ARG (the
 *      capture is left intact).
 * IDS outside [0, n_expert) are not a fault.  With h_ids on the batch route the call is refused on the host with GGML_HIP_ERR_ARG
 * before anything is launched; wherever the ids are only known on the device (route 1; route 2 with h_ids == NULL) that pair's M
 * outputs are written as +0.0f, and no address is ever formed from the bad id.
 * d_ids may be NULL only on the batch route with h_ids given.  d_src1: 16-byte aligned, ld1_token and ld1_slot multiples of 4.
 * d_work / work_bytes: ggml_hip_mul_mat_id_work_size bytes (the gathered rows, the sorted results and the largest per-expert work
 * buffer any routing can need); missing or short is GGML_HIP_ERR_ARG.  n_tokens = 0 returns 0 and writes nothing.
 * ggml_hip_mul_mat_id_route: 1 / 2, or < 0 (an error code).  n_expert takes no part in either answer. */
typedef struct ggml_hip_expert_set ggml_hip_expert_set;
int  ggml_hip_expert_set_create(const ggml_hip_weight *const *w, int n_expert, void *stream, ggml_hip_expert_set **out);
void ggml_hip_expert_set_free(ggml_hip_expert_set *s);
int    ggml_hip_mul_mat_id_route(const ggml_hip_expert_set *s, int64_t n_tokens, int n_used);   /* host only: 1 by-id mat-vec, 2 batch route, < 0 error */
size_t ggml_hip_mul_mat_id_work_size(const ggml_hip_expert_set *s, int64_t n_tokens, int n_used);
int    ggml_hip_mul_mat_id_route_for(int type, int64_t M, int64_t K, int n_expert, int64_t n_tokens, int n_used);
size_t ggml_hip_mul_mat_id_work_size_for(int type, int64_t M, int64_t K, int n_expert, int64_t n_tokens, int n_used);
int    ggml_hip_mul_mat_id_dev(const ggml_hip_expert_set *s, const int32_t *d_ids, const int32_t *h_ids,
                               int64_t n_tokens, int n_used, const float *d_src1, int64_t ld1_token, int64_t ld1_slot,
                               float *d_dst, int64_t ldd, void *d_work, size_t work_bytes, void *stream);

/* ---------------- the GROUPED route: a device-routed grouped product for mul_mat_id batches ----------------
 * An entry of its own beside the two routes above (ggml_hip_mul_mat_id_route{,_for} and ggml_hip_mul_mat_id_dev answer exactly as before:
 * 1 or 2).  For batches whose ids come out of a top-k kernel ON THE DEVICE -- a prompt-sized mixture-of-experts layer inside a decoder's
 * graph: the ids are read only on the device (no h_ids, no host synchronize, no allocation), the number of launches is fixed for a shape
 * (seven: three of routing, a gather, one INIT, ONE product, a scatter -- never a function of the routing or of n_expert), the call is
 * legal on a capturing stream and a captured call replayed with other contents in d_ids computes the new routing.
 * The same conventions as ggml_hip_mul_mat_id_dev: pair p = t * n_used + s, ld1_slot = 0 as the broadcast, d_src1 16-byte aligned with
 * strides that are multiples of 4 (GGML_HIP_ERR_SHAPE), ldd >= M, the error codes; n_tokens = 0 returns 0 and writes nothing.
 * An id outside [0, n_expert) writes that pair's M outputs as +0.0f; no address is formed from it.
 * P = n_tokens * n_used up to 2^20; more is GGML_HIP_ERR_SHAPE.
 *
 * SERVED (ggml_hip_mul_mat_id_grouped_serves = 1; _serves_for answers for (type, M, K) with no weight and no device, 1 / 0 only):
 *   - the type is Q8_0, Q5_0, IQ4_NL (a Q8_0 weight to every kernel) or Q4_0, AND
 *   - the plan of mul_mat(type, M, K, N = 32) is GGML_HIP_MMF_K3S_I8 or GGML_HIP_MMF_K3S_MX: today K / 32 in 32 .. 1024.
 * Every other type answers 0 and the entry returns GGML_HIP_ERR_TYPE; every shape outside that range answers 0 and the entry returns
 * GGML_HIP_ERR_SHAPE.  OUT OF SCOPE: the min-term types (Q4_1, Q5_1, Q5_K, Q4_K), the two-scale types (Q4_2, and Q6_K / Q3_K / Q2_K /
 * IQ4_XS in their resident forms), the dense types (F32, F16, BF16) -- they keep the batch route.
 *
 * ARITHMETIC.  The counts are not known on the host, so the summation tree cannot follow count_e as the batch route's does: it is fixed
 * by (type, K) alone, the tree of ggml_hip_mm_plan(type, M, K, 32) -- eight contiguous k-block ranges, a range's blocks in ascending
 * order with the type's f32 statement per block, the eight partial sums added in wave order.  Pair p's M outputs are BIT FOR BIT the row
 * that ggml_hip_mul_mat_dev(expert ids[p], a batch of 32 rows that holds p's src1 row at any position, N = 32) returns for that row.
 * A set of row shards [r0, r1) computes columns [r0, r1) of the whole set's result, bit for bit.
 *
 * d_work / work_bytes: ggml_hip_mul_mat_id_grouped_work_size bytes; missing or short is GGML_HIP_ERR_ARG.  The size is a function of
 * (type, M, K, n_expert, P) -- it DEPENDS ON n_expert, unlike the batch route's: the sorted rows are padded per expert to whole column
 * tiles of 32, so everything is sized by the bound P + 31 * min(n_expert, P) rows.  It is the same for every (n_tokens, n_used) with one
 * P, 0 for n_tokens = 0 and for a set the route does not serve; the _for twin and the set's entry are the same function. */
int    ggml_hip_mul_mat_id_grouped_serves(const ggml_hip_expert_set *s);                 /* 1 / 0, < 0 error */
int    ggml_hip_mul_mat_id_grouped_serves_for(int type, int64_t M, int64_t K);           /* no device needed */
size_t ggml_hip_mul_mat_id_grouped_work_size(const ggml_hip_expert_set *s, int64_t n_tokens, int n_used);
size_t ggml_hip_mul_mat_id_grouped_work_size_for(int type, int64_t M, int64_t K, int n_expert, int64_t n_tokens, int n_used);
int    ggml_hip_mul_mat_id_grouped_dev(const ggml_hip_expert_set *s, const int32_t *d_ids, int64_t n_tokens, int n_used,
                                       const float *d_src1, int64_t ld1_token, int64_t ld1_slot,
                                       float *d_dst, int64_t ldd, void *d_work, size_t work_bytes, void *stream);

/* ---------------- the ends of a mixture-of-experts block: the ROUTER in front of the products, the COMBINE behind them ----------------
 * With ggml_hip_mul_mat_dev for the router matrix, the grouped route above and ggml_hip_silu_mul_rows_dev these make a whole MoE FFN block
 * out of device entries: router product -> route -> gate / up (ld1_slot = 0) -> silu_mul_rows -> down (a row per slot) -> combine.  All three
 * entries are stream-ordered on `stream` on the current device; they do not synchronize, do not allocate, take no work buffer and may be
 * captured.  n_tokens = 0 (nrows = 0) returns 0 and writes nothing.  EXTENSIONS like the products: the reference has no such nodes.
 *
 * ggml_hip_moe_route_dev: upstream's soft_max -> top_k -> get_rows [-> sum_rows, div] [-> scale] chain for its two gate functions.
 * d_logits: f32, [n_tokens] rows of n_expert, ld_logits >= n_expert elements apart (the dst of ggml_hip_mul_mat_dev for the router matrix: no
 * alignment beyond 4 bytes).  d_ids[t * n_used + s], d_weights[t * n_used + s]: the pair order p = t * n_used + s the products read.
 *   SELECTION is exact f32 comparison alone, so the ids are defined bit for bit:
 *     - slot s of token t holds the expert of rank s under "larger logit first; equal logits: smaller index first";
 *     - -0.0 and +0.0 compare equal;
 *     - a NaN logit ranks below every non-NaN one, -inf included; NaNs rank among themselves by index;
 *     - so a token's n_used ids are always distinct and inside [0, n_expert), whatever the logits hold;
 *     - the selection is on the LOGITS.  Both gates are monotone, so this is upstream's order wherever upstream's is defined, and where
 *       rounding makes two probabilities tie this rule still decides.
 *   WEIGHTS, every operation one binary32 rounding, expf the correctly-specified library function (no fast-math form):
 *     - gating 0, softmax over ALL experts: w = expf(l - lmax) / S, lmax the rank-0 logit, S the sum of expf(l_e - lmax) over all experts in
 *       a fixed order that no scheduling changes (no atomics): expert e belongs to lane e % 64, a lane adds its experts in ascending e, the
 *       64 partial sums meet in a butterfly (lane distance 32, 16, .., 1);
 *     - gating 1, sigmoid: w = 1 / (1 + expf(-l)) of each selected expert;
 *     - normalize != 0: w_s = w_s / (w_0 + w_1 + ...), the sum in slot order;
 *     - then w_s = w_s * scale, always (1.0f is exact).
 *     - a token whose logits hold a NaN, or whose rank-0 logit is +-inf, has UNSPECIFIED weight values; its ids still follow the rule.
 *   1 <= n_expert <= 1024, 1 <= n_used <= min(n_expert, 64), n_tokens * n_used <= 2^20: else GGML_HIP_ERR_SHAPE.  A null pointer,
 *   ld_logits < n_expert, n_tokens < 0 or gating outside {0, 1}: GGML_HIP_ERR_ARG. */
int ggml_hip_moe_route_dev(const float *d_logits, int64_t ld_logits, int64_t n_tokens, int n_expert, int n_used,
                           int gating, int normalize, float scale,
                           int32_t *d_ids, float *d_weights, void *stream);
/* ggml_hip_moe_combine_dev: the weighted sum over a token's slots -- upstream's ggml_mul then ggml_add of the slot views in ascending slot
 * order.  d_y: the pair rows, [n_tokens * n_used] rows of M, ldy >= M elements apart (the dst of either mul_mat_id entry).  Every product and
 * every sum is ONE binary32 rounding, no fused multiply-add:
 *     acc = w[t,0] * y[t,0,m];  for s = 1 .. n_used-1: acc = acc + w[t,s] * y[t,s,m];  dst[t,m] = d_addend ? acc + addend[t,m] : acc
 * d_addend (the residual, or a shared expert's output) may be NULL; d_dst may EQUAL d_addend (an element is read and then written by one
 * thread); d_dst may not overlap d_y.  Any M >= 1: 16-byte accesses where every pointer is 16-byte aligned and every stride a multiple of
 * 4, one element at a time otherwise -- the same bits.  ldy, ldd or ld_add below M: GGML_HIP_ERR_SHAPE; n_used in 1 .. 64 and
 * n_tokens * n_used <= 2^20 as above; a null d_y, d_weights or d_dst: GGML_HIP_ERR_ARG. */
int ggml_hip_moe_combine_dev(const float *d_y, int64_t ldy, const float *d_weights, int64_t n_tokens, int n_used, int64_t M,
                             const float *d_addend, int64_t ld_add, float *d_dst, int64_t ldd, void *stream);
/* The SwiGLU pair on contiguous device rows [nrows][k], the device twin of ggml_hip_rms_norm_mul_rows_dev: d_silu = silu(d_a) in the
 * reference's GGML_SILU_FP16 form (Ggml.cs:5705-5748), d_y = d_silu * d_b -- the kernel and the bits of ggml_hip_compute_forward_silu_mul.
 * d_silu may be NULL (a device caller has no node whose data must exist): only d_y is written. */
int ggml_hip_silu_mul_rows_dev(const float *d_a, const float *d_b, float *d_silu, float *d_y, int64_t nrows, int64_t k, void *stream);

/* ---------------- ATTENTION over an F16 or Q8_0 KV cache: rows into the cache, softmax(scale Q K^T + causal mask) V over it ----------------
 * Upstream's ggml_flash_attn_ext, an EXTENSION like mul_mat_id (the reference has the op's id and no dispatch): device-resident entries only.
 * With ggml_hip_rms_norm_mul_rows_dev, ggml_hip_mul_mat_multi_dev (q / k / v in one launch) and the add / scale epilogues these make a decoder
 * layer's attention half out of device entries: projections -> kv_store -> attention -> output projection.  Both entries are stream-ordered on
 * `stream` on the current device; they do not synchronize and do not allocate, and may be captured.  (The rotation of Q and K between the projections and the cache is the ROPE section's, below.)
 *
 * THE CACHE.  kv_type is GGML_TYPE_F16 or GGML_TYPE_Q8_0, the same for K and V (anything else: GGML_HIP_ERR_TYPE).  A cache ROW is
 * (position j, kv head hk): D elements in reference block format -- F16: 2 D bytes of IEEE halves, what ggml_cpy f32 -> f16 writes; Q8_0:
 * D / 32 blocks of ggml_hip_type_size(Q8_0) = 36 bytes { f32 d; int8 qs[32] }, quantize_row_q8_0 (Ggml.cs:733-762) -- at byte offset
 * j * nb_pos + hk * nb_head from d_k / d_v.  deq(row)[i] is the half widened, or (float)qs[i] * d in one binary32 rounding
 * (ggml_hip_dequantize_rows_dev).  nb_pos and nb_head are multiples of 16 and at least a row's bytes; either may be the larger one.
 *
 * ggml_hip_kv_store_dev: n_rows f32 rows of row_elems elements (row i at d_src + i * ld; d_src 16-byte aligned, ld a multiple of 4 and
 * >= row_elems) -> cache rows at d_cache + (p0 + i) * nb_pos, p0 = d_pos0 ? *d_pos0 (an int32 on the device, read by the kernel: a captured
 * call appends at a new position on every replay) : pos0.  row_elems = n_head_kv * D where the heads of a position lie back to back
 * (nb_head = a row's bytes), or D with one call per head otherwise (a Q8_0 cache of D = 64 has 72-byte rows: its heads are 80 apart, one call
 * each).  Q8_0 (row_elems a multiple of 32): bit for bit ggml_hip_quantize_rows_dev(Q8_0), i.e. the oracle.  F16 (a multiple of 4): IEEE round
 * to nearest even, subnormals kept, overflow to +-inf -- numpy's astype(float16).  A row whose position is < 0 or >= n_pos_max writes
 * nothing, and no address is formed from it.  d_cache 16-byte aligned, nb_pos a multiple of 16 (GGML_HIP_ERR_SHAPE).
 *
 * ggml_hip_attn_dev:
 *     dst[t][h][:] = sum over the VISIBLE j of p[t,h,j] * deq(V[j][h / G][:]),   p[t,h,.] = softmax_j(scale * q[t][h][:] . deq(K[j][h / G][:]))
 *   q, dst: f32 [n_q][n_head][D] with element strides (ldq_tok, ldq_head) / (ldd_tok, ldd_head), 16-byte aligned, strides multiples of 4.
 *   G = n_head / n_head_kv an integer in 1 .. 16 (upstream's broadcast), D 64 or 128: else GGML_HIP_ERR_SHAPE, as are misaligned strides.
 *   VISIBLE: causal != 0: j < n_kv - n_q + t + 1 (the batch is the LAST n_q positions of the cache); causal == 0: j < n_kv.
 *   n_kv: the host argument (0 .. n_kv_max), or, when d_n_kv != NULL, that int32 on the device clamped to [0, n_kv_max].  n_kv_max sizes
 *   the launches and the work buffer and bounds every address; dst does not depend on it.  A captured decode step can therefore be
 *   replayed while the cache grows: the same launches, a fixed number of them for a shape.
 *   A query row with no visible position writes +0.0f.
 *   REFUSED before anything is launched: a mask tensor, ALiBi (max_bias != 0), a soft-cap, sinks (GGML_HIP_ERR_ARG: pass NULL / 0).
 *   d_work / work_bytes: ggml_hip_attn_work_size bytes; missing or short is GGML_HIP_ERR_ARG.  0 for n_q = 0 (which returns 0 and writes
 *   nothing) and for the PROMPT form; monotone in n_kv_max.
 *
 * TWO FORMS, chosen from n_q alone (ggml_hip_attn_plan shows the choice; no device needed).  The positions are cut into CHUNKS of 128,
 * chunk c = [128 c, 128 c + 128), for every kv_type and D -- never a function of the device, the grid, n_head or n_kv_max.
 *   DECODE (n_q <= 8; all f32).  A workgroup serves one kv head and one chunk for ALL G * n_q query rows that share the kv head: each byte
 *   of the cache is read once per launch.  Per (row, chunk): s_j = scale * dot(q, deq(K_j)) (an f32 fma chain over d ascending);
 *   m = max s_j; p_j = expf(s_j - m); l = sum p_j (lane L of 64 holds p_L + p_(L+64), then a butterfly, lane distance 32 .. 1);
 *   a[d] = p_0 deq(V_0)[d], then fma(p_j, deq(V_j)[d], a[d]) for j ascending.  A second launch merges a row's partials: M = max m_c,
 *   b_c = expf(m_c - M), L and A[d] the fma chains of l_c b_c and a_c[d] b_c over c ASCENDING, dst = A / L.  No atomics; Q8_0 rows are read
 *   as blocks and never expanded in memory.  An invisible position takes part in nothing.  One visible position: dst = deq(V_0) bit for bit.
 *   dst[t][h] is bit for bit independent of n_head, of the strides, of n_kv_max, of where n_kv comes from and of n_q within the form.
 *   PROMPT (n_q > 8; v_mfma_f32_32x32x16_f16).  A workgroup owns 128 query rows of one head and walks the chunks below the causal diagonal
 *   (the others are skipped, the diagonal chunk is masked per element).  Q is rounded to f16; a Q8_0 row is dequantized to f16 while staged
 *   ((float)q * d, then RNE); S = Q K^T and O += P V accumulate in f32; per chunk m' = max(m, max s_j), alpha = expf(m - m'),
 *   P_j = f16(expf(s_j - m')), l = l alpha + sum of the ROUNDED P_j, O = O alpha + P V; dst = O / l.  One visible position: dst is the staged
 *   V row bit for bit -- deq(V_0) for F16, f16(deq(V_0)) for Q8_0.  A masked weight is a zero operand here: the cache must hold finite values
 *   below n_kv.
 *   NEITHER form returns a V that is constant over the positions exactly: a and l round independently; that case is inside the tolerance. */
enum { GGML_HIP_ATTN_DECODE = 1, GGML_HIP_ATTN_PROMPT = 2 };      /* ggml_hip_attn_plan_t.form */
typedef struct ggml_hip_attn_plan_t {
    int32_t form, chunk, q_tile, launches;   /* the form; positions per chunk; query rows per workgroup; launches of one call (2 / 1) */
    int64_t n_chunks, workgroups;            /* ceil(n_kv_max / chunk); workgroups of the main launch */
} ggml_hip_attn_plan_t;
int    ggml_hip_kv_store_dev(int kv_type, const float *d_src, int64_t ld, int64_t n_rows, int64_t row_elems,
                             void *d_cache, int64_t nb_pos, int64_t n_pos_max, int64_t pos0, const int32_t *d_pos0, void *stream);
int    ggml_hip_attn_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_plan_t *out);
size_t ggml_hip_attn_work_size(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max);
int    ggml_hip_attn_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                         const void *d_k, const void *d_v, int64_t nb_pos, int64_t nb_head,
                         int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max,
                         int causal, float scale, const void *d_mask, float max_bias, float logit_softcap, const float *d_sinks,
                         float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);

/* ---------------- ROPE: the rotary position embedding of Q / K rows, and the rotation fused with the store into the KV cache ----------------
 * Upstream's ggml_rope_ext, an EXTENSION like attention (the reference has the op's id and no dispatch): device-resident entries only, no
 * seam, no host mirror.  With the ATTENTION entries a decode step is device entries alone: projections -> rope(q) -> rope_kv_store(k) ->
 * kv_store(v) -> attention.  Both device entries are stream-ordered on `stream` on the current device; they do not synchronize, do not
 * allocate, take no work buffer and may be captured.  n_tokens = 0 returns 0 and writes nothing.
 *
 * MODE 0 NORMAL rotates the pairs (2i, 2i+1), mode 2 NEOX the pairs (i, i + n_dims/2), i = 0 .. n_dims/2 - 1, of every row of D elements;
 * elements n_dims .. D-1 are copied bit for bit.  mrope, vision and any other mode: GGML_HIP_ERR_ARG.
 *
 * POSITIONS.  With d_pos != NULL token t sits at d_pos[t] (an int32 array on the device, upstream's `pos` tensor; ggml_hip_rope_dev
 * rotates by whatever int32 it reads).  Otherwise it sits at p0 + t, p0 = d_pos0 ? *d_pos0 (an int32 on the device, read by the kernel) :
 * pos0 -- ggml_hip_kv_store_dev's convention, so ONE device integer drives the store and the rotation of a captured step.
 *
 * THE PER-PAIR CONSTANTS (upstream's rope_yarn and ggml_rope_yarn_corr_dims restated; this text is the definition, ggml_hip_rope_table
 * returns exactly these, all binary64, and the device entries call the same function on the host and hand the kernels the result):
 *     extrap_i = freq_base ^ (-2 i / n_dims)
 *     corr(r)  = n_dims * ln(n_ctx_orig / (2 pi r)) / (2 ln freq_base)
 *     low      = max(0, floor(corr(beta_fast))),   high = min(n_dims - 1, ceil(corr(beta_slow)))
 *     ramp_i   = 1 - clamp((i - low) / max(0.001, high - low), 0, 1)
 *     mix_i    = ramp_i * ext_factor               (ext_factor == 0: mix_i = 0, and n_ctx_orig and the betas are not read)
 *     eff_i    = extrap_i * (freq_scale * (1 - mix_i) + mix_i)
 *     mscale   = attn_factor, times (1 + 0.1 ln(1 / freq_scale)) when ext_factor != 0
 * THE ROTATION of the pair (x0, x1) of pair index i at position pos:
 *     theta = (double)pos * eff_i,  divided by (double)d_freq_factors[i] where d_freq_factors != NULL (device f32 [n_dims/2], llama-3's)
 *     c = (float)(cos(theta) * mscale),  s = (float)(sin(theta) * mscale)          binary64 cos / sin, one rounding to binary32 each
 *     y0 = x0 * c - x1 * s,  y1 = x0 * s + x1 * c                                  every f32 operation rounds once, no fused multiply-add
 *   This is MORE EXACT than upstream's f32 chain (whose angle carries about 4e-3 rad of rounding at position 32768), not bit-equal to it:
 *   the angle is good to about pos * 2^-48 rad, and an element is within 4 * 2^-24 * mscale * (|x0| + |x1|) of the exact rotation up to
 *   position 2^20.  Position 0 returns the input as VALUES (mscale = 1): a zero's sign may change (x0 * 1 - x1 * 0).
 *   A row's bits depend on (pos, the row, the parameters) alone: not on n_head, the strides, n_tokens, in place or not, or where pos came from.
 *
 * SHAPES.  D a multiple of 4, at most 256; n_dims even, in 2 .. D; n_head in 1 .. 65535; n_tokens <= 2^24; the strides (elements) multiples
 * of 4 and at least D; d_x, d_dst, d_cache 16-byte aligned: else GGML_HIP_ERR_SHAPE.  mode 0 or 2, freq_base > 1, freq_scale > 0, every
 * parameter finite (and, with ext_factor != 0, n_ctx_orig >= 1 and both betas > 0): else GGML_HIP_ERR_ARG, as is a null d_x / d_dst / d_cache.
 * d_dst may EQUAL d_x with equal strides (in place: a thread owns whole pairs); any other overlap is the caller's error.
 *
 * ggml_hip_rope_kv_store_dev: rotate K rows and store them as cache rows in one launch; the rotated row never goes to memory.  kv_type F16
 * or Q8_0 (else GGML_HIP_ERR_TYPE; Q8_0: D % 32 == 0).  Only the p0 form: the rope position IS the cache position.  Row (t, hk) goes to
 * d_cache + (p0 + t) * nb_pos + hk * nb_head; nb_pos / nb_head follow ggml_hip_attn_dev's rules (multiples of 16, at least a row's bytes,
 * either may be the larger) -- because it takes nb_head, one call serves every head of a D = 64 Q8_0 cache whose heads are 80 bytes apart,
 * where ggml_hip_kv_store_dev needs a call per head.  A row whose position is < 0 or >= n_pos_max writes nothing, and no address is formed
 * from it.  THE CONTRACT: bit for bit ggml_hip_rope_dev into a temporary followed by ggml_hip_kv_store_dev. */
typedef struct ggml_hip_rope_params_t {
    int32_t n_dims, mode, n_ctx_orig;      /* mode: 0 NORMAL (pairs 2i, 2i+1), 2 NEOX (pairs i, i + n_dims/2) */
    float   freq_base, freq_scale, ext_factor, attn_factor, beta_fast, beta_slow;
} ggml_hip_rope_params_t;
/* host only, no device: the per-pair constants every kernel uses; eff: n_dims/2 doubles */
int ggml_hip_rope_table(const ggml_hip_rope_params_t *rp, double *eff, double *mscale);
int ggml_hip_rope_dev(const ggml_hip_rope_params_t *rp, const float *d_x, int64_t ldx_tok, int64_t ldx_head,
                      int n_head, int D, int64_t n_tokens,
                      const int32_t *d_pos, int64_t pos0, const int32_t *d_pos0, const float *d_freq_factors,
                      float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *stream);
int ggml_hip_rope_kv_store_dev(const ggml_hip_rope_params_t *rp, int kv_type, const float *d_x, int64_t ldx_tok, int64_t ldx_head,
                               int n_head_kv, int D, int64_t n_tokens, const float *d_freq_factors,
                               void *d_cache, int64_t nb_pos, int64_t nb_head, int64_t n_pos_max,
                               int64_t pos0, const int32_t *d_pos0, void *stream);

/* ---------------- PAGED ATTENTION: a batch of independent sequences over one pool of KV pages, in one call per entry ----------------
 * An EXTENSION like the two sections above (upstream serves a batch of sequences through its mask tensor; here the cache itself is cut into
 * pages).  ggml_hip_attn_dev and ggml_hip_kv_store_dev know ONE cache, one n_kv and one pos0; a step that decodes 32 sequences would make 32
 * attention calls and 64 stores, each sequence on a contiguous cache reserved at its maximum length.  These entries take the whole batch:
 *     projections at n_seq * n_q rows -> rope(q, d_pos) -> rope_kv_store_paged(k) -> kv_store_paged(v) -> attn_paged
 * All are stream-ordered on `stream` on the current device; none synchronizes or allocates; all may be captured; no atomics.  Every refusal
 * below is decided before a device is touched.  The entries of the sections above keep their bits and their signatures.
 *
 * THE PAGED CACHE (shared by all entries).
 *   POOL.   d_k / d_v (d_pool for a store) hold n_pages PAGES of 128 positions each -- a page is a CHUNK of ggml_hip_attn_dev, for every
 *           kv_type and D.  kv_type is F16 or Q8_0 as above (else GGML_HIP_ERR_TYPE).
 *   ROWS.   Row (position-in-page jj, kv head hk) of page p lies at byte offset  p * nb_page + jj * nb_pos + hk * nb_head,  in the reference
 *           block format ggml_hip_kv_store_dev writes.
 *   STRIDES. nb_pos and nb_head follow ggml_hip_attn_dev's rules (multiples of 16, at least a row's bytes, either may be the larger).
 *           nb_page is a multiple of 16 and at least the bytes a page's rows span, 127 * nb_pos + (n_head_kv - 1) * nb_head + a row's bytes:
 *           else GGML_HIP_ERR_SHAPE.
 *   TABLE.  d_pages: int32 [n_seq][ld_pages] on the device, ld_pages >= ceil(n_kv_max / 128) (else GGML_HIP_ERR_SHAPE).  Entry c of
 *           sequence b is the page that holds its positions [128 c, 128 c + 128).  Two sequences may name the same page (a shared prefix).
 *           Entries at or beyond ceil(n_kv[b] / 128) are never read by attention and may hold anything.
 *   LENGTHS. d_len: int32 [n_seq] on the device, never NULL: the positions sequence b held BEFORE this step.  The stores put token t of
 *           sequence b at position d_len[b] + t.  Attention uses n_kv[b] = clamp(d_len[b] + len_bias, 0, n_kv_max), len_bias a host
 *           integer: behind a store the caller passes len_bias = n_q, so ONE device array drives the rotation (d_pos = d_len for n_q = 1),
 *           the stores and the attention of a captured step, and the host adds n_q to it between replays.
 *   NULL d_pages / d_len, n_pages <= 0: GGML_HIP_ERR_ARG.  1 <= n_seq <= 4096, n_seq * n_q <= 2^20 and (attention) n_seq * n_q * n_head
 *   < 2^31 -- the grids carry the sequences in their z dimension and the merge is one workgroup per row and head: above, GGML_HIP_ERR_SHAPE.
 *   n_kv_max (0 .. 2^24) sizes the launches and bounds every position.  SIZE IT TO THE STEP, not to the model's context: the DECODE grid has
 *   ceil(n_kv_max / 128) workgroups per kv head and sequence, and those beyond a sequence's length are launched to leave at once.
 *   THE LIBRARY HAS NO ALLOCATOR: the host owns the table; page allocation, copy-on-write and defragmentation are the caller's.
 *
 * ggml_hip_kv_store_paged_dev: f32 rows [n_seq * n_q][n_head_kv][D] with element strides (ldx_tok, ldx_head) (multiples of 4, at least D;
 *   d_src and d_pool 16-byte aligned; D a multiple of 4, for Q8_0 of 32, at most 256) -> row (b, t, hk) to its page row.
 *   THE CONTRACT: the bytes written are bit for bit what ggml_hip_kv_store_dev writes for that f32 row.  A token writes nothing, and no
 *   address is formed from it, when its position is < 0 or >= n_kv_max, or when its page id is outside [0, n_pages).
 * ggml_hip_rope_kv_store_paged_dev: the same with the rotation in front; the rope position IS the cache position d_len[b] + t.
 *   THE CONTRACT: bit for bit ggml_hip_rope_dev (d_pos[b * n_q + t] = d_len[b] + t) into a temporary, then ggml_hip_kv_store_paged_dev.
 * ggml_hip_attn_paged_dev: q, dst f32 [n_seq * n_q][n_head][D] (rows of sequence b at b * n_q ..; strides as ggml_hip_attn_dev); n_q is
 *   uniform over the sequences.  The form follows n_q alone exactly as ggml_hip_attn_plan decides it (DECODE up to 8 rows per sequence,
 *   PROMPT above; the chunk is 128); ggml_hip_attn_paged_plan shows it, with the workgroups of all sequences.
 *   THE CONTRACT: for every sequence b its n_q rows of dst are BIT FOR BIT ggml_hip_attn_dev with the same n_q, n_kv = n_kv[b], causal,
 *   scale, heads and D on a contiguous cache holding the same row bytes -- in both forms: a paged call runs the same chunk body on
 *   pool + page * nb_page, and neither form's arithmetic knows where a chunk lies.  So a sequence's bits do not depend on the page
 *   assignment, n_pages, ld_pages, nb_page, n_kv_max, n_seq or its slot.
 *   A sequence with n_kv[b] = 0 writes +0.0f rows: that is how a captured graph of fixed n_seq carries idle slots.
 *   A sequence with a page id outside [0, n_pages) among its first ceil(n_kv[b] / 128) entries writes +0.0f for ALL its rows; no address is
 *   formed from that id and the other sequences are unaffected.
 *   A mask, ALiBi, a soft-cap and sinks are refused as by ggml_hip_attn_dev.
 *   d_work / work_bytes: ggml_hip_attn_paged_work_size bytes -- DECODE: n_seq * n_q * n_head * ceil(n_kv_max / 128) * (D + 4) floats plus
 *   alignment; 0 for n_seq * n_q = 0 and for PROMPT; monotone in n_seq, n_q (within DECODE) and n_kv_max.  Missing or short: GGML_HIP_ERR_ARG.
 *   n_q = 0 returns 0 and writes nothing.
 * KERNELS.  DECODE: grid (chunks of n_kv_max) x (kv heads) x (sequences); a workgroup reads its sequence's length and its chunk's page id as
 *   scalars and leaves at once if the chunk lies at or beyond n_kv[b] or the id is invalid; the merge (one workgroup per row) scans the
 *   sequence's needed ids first and writes zeros if one is invalid.  PROMPT: grid (query tiles) x (heads) x (sequences); a workgroup scans
 *   the needed ids before its first stage, then takes each chunk's base from the table. */
int    ggml_hip_kv_store_paged_dev(int kv_type, const float *d_src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D,
                                   int64_t n_seq, int64_t n_q, void *d_pool, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                   const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max, void *stream);
int    ggml_hip_rope_kv_store_paged_dev(const ggml_hip_rope_params_t *rp, int kv_type, const float *d_x, int64_t ldx_tok, int64_t ldx_head,
                                        int n_head_kv, int D, int64_t n_seq, int64_t n_q, const float *d_freq_factors,
                                        void *d_pool, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                        const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max, void *stream);
int    ggml_hip_attn_paged_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_plan_t *out);
size_t ggml_hip_attn_paged_work_size(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max);
int    ggml_hip_attn_paged_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                               const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                               const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq,
                               int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv_max,
                               int causal, float scale, const void *d_mask, float max_bias, float logit_softcap, const float *d_sinks,
                               float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);

/* ---------------- ATTENTION OPTIONS: a sliding window, attention sinks and a logit soft-cap over either cache ----------------
 * ggml_hip_attn_dev and ggml_hip_attn_paged_dev compute softmax(scale Q K^T + causal mask) V and refuse upstream's other parameters.  The
 * four entries below serve three of them -- what Mistral / Gemma 2, 3 / Phi-3 / gpt-oss layers need -- with NO mask tensor: the window is a
 * number, the sinks a vector per head, the cap a number.  A mask tensor and ALiBi are not served here: these entries have no parameter
 * for them (the _bias entries of the section ATTENTION WITH A MASK TENSOR AND ALiBi SLOPES below take them).  The base entries keep their signatures, their refusals and their bits.
 *
 * ggml_hip_attn_opts_t:  d_sinks: device f32 [n_head], 4-byte aligned, or NULL (none).  window: 0 (none), or W >= 1: the row at position P
 * sees position j only if P - j < W (upstream's pos_q - pos_k < n_swa); needs causal != 0.  logit_softcap: 0 (none) or a finite cap > 0.
 * reserved: 0.  REFUSED with GGML_HIP_ERR_ARG before a device is touched: window < 0; window > 0 with causal == 0; a cap that is negative
 * or not finite; a misaligned d_sinks; reserved != 0.  A window of n_kv_max or more is accepted.
 * EVERY RULE of the base entry holds unchanged: shapes, strides, alignment, null pointers, n_q = 0, the clamped device n_kv, the paged cache's
 * rules, no synchronize, no allocation, capturable, no atomics.  The form follows n_q alone as ggml_hip_attn_plan decides it.  The work buffer
 * is the BASE entry's (ggml_hip_attn_work_size / ggml_hip_attn_paged_work_size): always enough, there is no new size function.
 * opts == NULL, or an opts with everything off, runs the base kernels and returns the base entry's bits.
 *
 * THE ARITHMETIC.  Everything not named here is the two forms' statement above, unchanged.
 *   WINDOW.  With hi_t = the base entry's visible count of row t, row t sees lo_t <= j < hi_t, lo_t = max(0, hi_t - W).  A position outside
 *     that range takes part in nothing.  A chunk with no visible position for a row writes no partial for it and the merge reads none.
 *     DECODE: inside a chunk the a[d] chain starts at the row's first visible position (a[d] = p_f deq(V_f)[d], then fma for j ascending); the
 *     merge runs the row's chunks lo_t / 128 .. (hi_t - 1) / 128 in ascending order with the base statement (the first chunk's term is the
 *     product, the rest are fma).  PROMPT: a workgroup starts at the chunk of its FIRST row's lo; a wave skips the chunks wholly outside its
 *     rows' ranges, as it skips those above the diagonal; the element mask gains j >= lo.
 *   SOFT-CAP.  s_j = cap * tanhf(sc' * dot_j), sc' = scale / cap in ONE binary32 division on the host, tanhf the library function; it stands
 *     where scale * acc (DECODE) / scale * S_j (PROMPT) stands in the base statement.
 *   SINKS.  sink_h is read for the row's head and joins the DENOMINATOR only; it is neither scaled nor capped.
 *     DECODE merge: M = max(max_c m_c, sink_h); the base chain over the chunks against that M; then L = L + (sink_h == M ? 1.0f :
 *     expf(sink_h - M)); dst = A / L.  PROMPT, after the last chunk: mn = max(m, sink); alpha = expf(m - mn); l = l alpha + expf(sink - mn);
 *     O = O alpha; dst = O / l.  A row with no visible position still writes +0.0f.  A sink of -inf is legal and means "none"; NaN or +inf
 *     gives unspecified values in that head's rows and nothing else.
 * CONSEQUENCES (the tests hold the kernels to them bit for bit, in both forms, contiguous and paged):
 *   1. Everything off gives the base entry's bits.
 *   2. window >= n_kv gives the bits of window = 0.
 *   3. Every sink -inf gives the bits of d_sinks = NULL.
 *   4. TRANSLATION BY WHOLE CHUNKS: for k <= lo_0 / 128 the windowed call over (cache, n_kv) equals the windowed call over (the cache advanced
 *      by 128 k positions, n_kv - 128 k).  So for n_q = 1 with n_kv - W a multiple of 128 it equals the BASE entry on the advanced cache with
 *      n_kv' = W.
 *   5. The base entries' invariances hold: n_head, the strides, n_kv_max, where n_kv comes from, n_q within DECODE, the page assignment,
 *      n_pages, ld_pages, nb_page, n_seq, the slot.
 *   With q = 0, sink_h = 0 and one visible position, DECODE returns deq(V_0) / 2 bit for bit.
 *
 * THE GRID AND THE PAGE TABLE FOLLOW THE WINDOW (DECODE).  The chunk count of a windowed DECODE call is
 *     min(ceil(n_kv_max / 128), ceil((W + n_q - 1) / 128) + 1)
 * -- the chunks the union of the rows' ranges can touch; the _ex plan entries report it and the workgroups, which past the window do not grow
 * with n_kv_max (the base entries' "size n_kv_max to the step" does not bind a windowed layer).  Workgroup x serves chunk c_lo + x,
 * c_lo = lo_0 / 128, computed ON THE DEVICE from the same clamped n_kv (contiguous) or d_len[b] + len_bias (paged) the kernel reads anyway: a
 * captured step keeps working while c_lo moves between replays.  The work buffer's chunk index is x and the merge walks it in the same
 * ascending order: the bits do not change.
 * PAGED: table entries BELOW c_lo[b] are never read and may hold anything, invalid ids included; the merge's and the PROMPT kernel's id scan
 * covers [c_lo[b], ceil(n_kv[b] / 128)) only.  THIS IS WHAT LETS A HOST RECYCLE THE PAGES THAT SLID OUT OF A WINDOWED LAYER.  An invalid id
 * inside that range still zeroes that sequence's rows alone; every id is checked before an address is formed from it. */
typedef struct ggml_hip_attn_opts_t {
    const float *d_sinks;        /* device f32 [n_head], or NULL: none */
    int64_t      window;         /* 0: none; W >= 1: row at position P sees j with P - j < W */
    float        logit_softcap;  /* 0: none; cap > 0 */
    int32_t      reserved;       /* must be 0 */
} ggml_hip_attn_opts_t;
int    ggml_hip_attn_ex_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max,
                             const ggml_hip_attn_opts_t *opts, ggml_hip_attn_plan_t *out);
int    ggml_hip_attn_ex_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                            const void *d_k, const void *d_v, int64_t nb_pos, int64_t nb_head,
                            int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max,
                            int causal, float scale, const ggml_hip_attn_opts_t *opts,
                            float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);
int    ggml_hip_attn_paged_ex_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max,
                                   const ggml_hip_attn_opts_t *opts, ggml_hip_attn_plan_t *out);
int    ggml_hip_attn_paged_ex_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                                  const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                  const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq,
                                  int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv_max,
                                  int causal, float scale, const ggml_hip_attn_opts_t *opts,
                                  float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);

/* ---------------- RAGGED PAGED ATTENTION: the paged entries with a query count PER SEQUENCE, read on the device ----------------
 * ggml_hip_attn_paged_dev takes ONE n_q for all sequences.  A continuous-batching step holds sequences that decode one token, a few that
 * verify 2 .. 8 draft tokens, one or two that prefill a chunk, and idle slots: the host would split it into one paged call per distinct n_q,
 * and a captured graph would be frozen to that grouping.  The entries below take the whole step over the SAME paged cache:
 *     ragged_positions -> rope(q, d_pos) -> rope_kv_store_paged_ragged(k) -> kv_store_paged_ragged(v) -> attn_paged_ragged
 * All are stream-ordered on `stream` on the current device; none synchronizes or allocates; all may be captured; no atomics.  Every refusal
 * below is decided before a device is touched.  The entries of the sections above keep their bits and their signatures.
 *
 * THE RAGGED BATCH (shared by all entries).
 *   ROWS.   q, dst and the stores' source rows are PACKED: f32 [n_tokens_max][heads][D], the rows of sequence b one after the other.
 *   d_q_start: int32 [n_seq + 1] on the device, never NULL (GGML_HIP_ERR_ARG), 4-byte aligned (else GGML_HIP_ERR_SHAPE): prefix sums.  The
 *           rows of sequence b are rows d_q_start[b] .. d_q_start[b+1] - 1, and n_q[b] = d_q_start[b+1] - d_q_start[b].  n_q[b] = 0 is an
 *           idle slot: nothing is written for it.
 *   n_tokens_max: a host integer, 0 .. 2^20 (negative: GGML_HIP_ERR_ARG; above: GGML_HIP_ERR_SHAPE), for attention n_tokens_max * n_head
 *           < 2^31 (else GGML_HIP_ERR_SHAPE).  It sizes the grids and bounds every row address.  n_tokens_max = 0 returns 0 and writes nothing.
 *   PRESENT. Sequence b is PRESENT when 0 <= d_q_start[b] <= d_q_start[b+1] <= n_tokens_max.  A sequence that is not present writes nothing
 *           and no address is formed from its bounds.  Rows that belong to no present sequence are not written (ragged_positions writes 0).
 *           d_q_start is MEANT to ascend.  Attention looks at every sequence by itself, so a present sequence is served whatever the others'
 *           bounds are.  The stores and ragged_positions find a row's sequence by bisection of d_q_start, which is exact for ascending
 *           bounds; where the bounds do not ascend, a row is either written exactly as stated (for a present sequence that holds it) or not
 *           written at all -- never anything else, and never from an address outside the stated bounds.  Present sequences that overlap
 *           are the caller's error.
 *   THE CACHE is the paged cache of the PAGED ATTENTION section, unchanged: pool, rows, strides, table, d_len, 1 <= n_seq <= 4096, n_kv_max,
 *           and the rule that a page id outside [0, n_pages) gives zeros (a store: writes nothing) and is never turned into an address.
 *           Every refusal of the paged entries carries over with its code.
 *   POSITIONS. Token t of sequence b sits at position d_len[b] + t.  Attention uses
 *               n_kv[b] = clamp(d_len[b] + (add_q ? n_q[b] : 0) + len_bias, 0, n_kv_max);
 *           behind a store of this step's tokens the caller passes add_q = 1, len_bias = 0.
 *
 * ggml_hip_ragged_positions_dev: d_pos[i] = d_len[b] + t for every packed row i = (b, t) of a present sequence, 0 for the other rows below
 *   n_tokens_max: the int32 position array ggml_hip_rope_dev takes for Q, so a captured step follows d_q_start.  d_pos: int32 [n_tokens_max],
 *   4-byte aligned; NULL d_len / d_pos: GGML_HIP_ERR_ARG.
 * ggml_hip_ragged_last_rows_dev: the rows the LM head needs from a ragged step, gathered on the device.  d_x, d_dst: f32 rows of K elements,
 *   ldx / ldd apart.  For every s < n_seq, d_dst[s * ldd + k] = d_x[(d_q_start[s+1] - 1) * ldx + k], k < K, where
 *   0 <= d_q_start[s] < d_q_start[s+1] <= n_tokens_max; an EMPTY sequence or one that is not present gets a row of +0.0f and no address is
 *   formed from its bounds.  Columns K .. ldd - 1 and rows past n_seq are not written.  d_dst may not overlap d_x.  16-byte copies where d_x
 *   and d_dst are 16-byte aligned and K, ldx and ldd are multiples of 4, one element at a time otherwise: the same bits.  One launch.
 *   d_q_start, n_seq and n_tokens_max: the refusals of ggml_hip_ragged_positions_dev (n_tokens_max = 0: every row is +0.0f).  0 <= K <= 2^24
 *   and ldx, ldd >= K, else GGML_HIP_ERR_SHAPE; K = 0 returns 0 and writes nothing.  NULL d_x / d_dst: GGML_HIP_ERR_ARG; not 4-byte aligned:
 *   GGML_HIP_ERR_SHAPE.
 * ggml_hip_kv_store_paged_ragged_dev, ggml_hip_rope_kv_store_paged_ragged_dev: the paged stores over packed rows, one thread per 32 (Q8_0) or 4
 *   (F16) elements as theirs.  The thread finds its row's sequence by bisection of d_q_start, and every guard comes before the address it
 *   protects: a present sequence, the row inside it, the position inside [0, n_kv_max), the page id inside [0, n_pages).
 *   THE CONTRACT: the bytes written for a row are bit for bit what ggml_hip_kv_store_paged_dev / ggml_hip_rope_kv_store_paged_dev write for
 *   that row of that sequence (n_seq = 1, n_q = n_q[b], the same table row and d_len[b]).
 * ggml_hip_attn_paged_ragged_dev: q, dst packed [n_tokens_max][n_head][D] (strides as ggml_hip_attn_dev).  opts as the _ex entries take it,
 *   with their rules: NULL, or everything off, runs the base bodies, otherwise the option bodies.
 *   THE FORM IS CHOSEN PER SEQUENCE from n_q[b] alone by ggml_hip_attn_plan's rule: DECODE for 1 .. 8 rows, PROMPT above; 0 writes nothing.
 *   THE CONTRACT: for every present sequence b that has a slot or a tile (below), its n_q[b] rows of dst are BIT FOR BIT those of
 *   ggml_hip_attn_paged_dev -- ggml_hip_attn_paged_ex_dev when an option is on -- called with n_seq = 1, n_q = n_q[b], the same table row,
 *   d_len[b], len_bias = (add_q ? n_q[b] : 0) + len_bias, the same pool and the same parameters: the ragged kernels run the same chunk
 *   bodies with the sequence's own n_q.  So a sequence's bits do not depend on the other sequences, its slot, the order of the batch,
 *   n_tokens_max, n_dec_rows_max, n_kv_max or the page assignment; n_kv[b] = 0 and an invalid needed page id give +0.0f rows as there.
 *   n_dec_rows_max: a host integer, 0 .. n_tokens_max (else GGML_HIP_ERR_ARG): the DECODE-form rows the work buffer can hold.
 *   min(n_tokens_max, 8 * n_seq) can never overflow.  Below that, the DECODE sequences get their row SLOTS in ascending b, each one that
 *   still fits behind those served before it; a DECODE sequence that does not fit gets no slot and ITS ROWS ARE WRITTEN AS +0.0f (by the
 *   index launch); later sequences that fit are still served.  PROMPT sequences need no slot.
 *   d_work / work_bytes: ggml_hip_attn_paged_ragged_work_size bytes: the index tables, then n_dec_rows_max * n_head * ceil(n_kv_max / 128) *
 *   (D + 4) floats, plus alignment -- sized by the DECODE bound and never by n_tokens_max (a 2048-token prefill pays no partials).  0 for
 *   n_tokens_max = 0; monotone in n_seq, n_tokens_max, n_dec_rows_max and n_kv_max; one size serves every opts.  Missing or short:
 *   GGML_HIP_ERR_ARG.
 * FOUR LAUNCHES whatever the batch holds (ggml_hip_attn_paged_ragged_plan shows them; host only, as is the work size):
 *   1. INDEX, one workgroup: an exclusive scan through LDS over the sequences writes, to the front of d_work, for every sequence (first row
 *      slot or -1, first packed row, n_q); for every row slot its (b, t), (-1, -1) for an unused one; the list of PROMPT tiles (b, tile) in
 *      ascending (b, tile) order and its length.
 *   2. DECODE, grid (n_chunks) x (kv heads) x (sequences), the paged DECODE grid.  n_chunks = ceil(n_kv_max / 128); under a window
 *      0 < W < n_kv_max it is min(ceil(n_kv_max / 128), ceil((W + 7) / 128) + 1), the _ex entries' bound taken at 8 rows.  A workgroup whose
 *      sequence is not DECODE or has no slot leaves before its first barrier.
 *   3. MERGE, one workgroup per row slot and head, with the paged merge's id scan and zero row.
 *   4. PROMPT, grid (heads) x (max_tiles), the list in dispatch order: a workgroup past the list's length leaves at once, after the last
 *      tile.  max_tiles is the most tiles a batch inside the bounds can hold.  A PROMPT sequence has n >= 9 rows and 1 + (n - 1) / 128 tiles: it is worth a tile for 9 rows, a second one for 120
 *      more, every further one for 128.  With P = min(n_seq, n_tokens_max / 9), L = n_tokens_max - 9 P, k = min(P, L / 120):
 *          max_tiles = P + k + (L - 120 k) / 128          (integer divisions)
 *   A launch whose grid the BOUNDS leave empty (n_dec_rows_max = 0, n_kv_max = 0, n_tokens_max < 9) is not made; `launches` counts the rest. */
typedef struct ggml_hip_attn_ragged_plan_t {
    int32_t chunk, launches;                 /* positions per chunk (128); launches of one call (4) */
    int64_t n_chunks, max_tiles;             /* DECODE's chunks per sequence; the PROMPT tile bound */
    int64_t decode_workgroups, merge_workgroups, prompt_workgroups;
    int64_t index_bytes;                     /* the index tables in front of the partials, rounded up to 256 */
} ggml_hip_attn_ragged_plan_t;
int    ggml_hip_ragged_positions_dev(const int32_t *d_q_start, const int32_t *d_len, int64_t n_seq, int64_t n_tokens_max, int32_t *d_pos, void *stream);
int    ggml_hip_ragged_last_rows_dev(const float *d_x, int64_t ldx, const int32_t *d_q_start, int64_t n_seq, int64_t n_tokens_max,
                                     int64_t K, float *d_dst, int64_t ldd, void *stream);
int    ggml_hip_kv_store_paged_ragged_dev(int kv_type, const float *d_src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D,
                                          int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max,
                                          void *d_pool, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                          const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max, void *stream);
int    ggml_hip_rope_kv_store_paged_ragged_dev(const ggml_hip_rope_params_t *rp, int kv_type, const float *d_x, int64_t ldx_tok, int64_t ldx_head,
                                               int n_head_kv, int D, int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max,
                                               const float *d_freq_factors,
                                               void *d_pool, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                               const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max, void *stream);
int    ggml_hip_attn_paged_ragged_plan(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_tokens_max, int64_t n_dec_rows_max,
                                       int64_t n_kv_max, const ggml_hip_attn_opts_t *opts, ggml_hip_attn_ragged_plan_t *out);
size_t ggml_hip_attn_paged_ragged_work_size(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_tokens_max,
                                            int64_t n_dec_rows_max, int64_t n_kv_max);
int    ggml_hip_attn_paged_ragged_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                                      const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                      const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int add_q, int len_bias, int64_t n_seq,
                                      const int32_t *d_q_start, int64_t n_tokens_max, int64_t n_dec_rows_max,
                                      int n_head, int n_head_kv, int D, int64_t n_kv_max,
                                      int causal, float scale, const ggml_hip_attn_opts_t *opts,
                                      float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);

/* ---------------- ATTENTION WITH A MASK TENSOR AND ALiBi SLOPES: the _ex and the ragged entries with upstream's mask and max_bias ----------------
 * The entries above express "the last n_q positions, causal, minus a window".  Upstream's ggml_flash_attn_ext also takes a MASK tensor, added to
 * the scores, and max_bias, which scales it per head (ALiBi).  The three entries below take both over the contiguous, the paged and the ragged
 * cache: a draft TREE in speculative decoding (a draft row sees the committed cache and its own ancestors), bidirectional spans inside a causal
 * prompt (prefix-LM, image tokens), additive position biases and ALiBi models.  The base and the _ex entries keep their signatures, their
 * refusals (a mask or max_bias != 0 on the base entries included) and their bits.
 *
 * ggml_hip_attn_bias_t:
 *   d_mask:   device f16 [rows][ld_mask], or NULL (none).  THE MASK ROW OF A QUERY ROW is the row with the same row index as in q: contiguous
 *             row t; paged the row b * n_q + t; ragged the packed row.  COLUMN j is position j of that row's own sequence.  The mask is shared
 *             by all heads (upstream's broadcast).  Only rows of queries that exist are read, in 8-byte pieces that begin below the sequence's
 *             n_kv (so never at or beyond ld_mask); a value at or beyond n_kv is never used, whatever it is.
 *   ld_mask:  halves between mask rows.  ld_mask >= n_kv_max, ld_mask % 8 == 0 and d_mask 16-byte aligned, otherwise GGML_HIP_ERR_SHAPE.
 *   d_slopes: device f32 [n_head], or NULL: every slope 1.0f.  Misaligned (4 bytes), or given without d_mask (there is nothing to multiply):
 *             GGML_HIP_ERR_ARG.  The caller uploads the vector, as it does the sinks; ggml_hip_alibi_slopes computes upstream's.
 * bias == NULL, or a bias whose d_mask and d_slopes are both NULL (ld_mask is then not looked at), runs the kernels of ggml_hip_attn_ex_dev /
 * ggml_hip_attn_paged_ex_dev / ggml_hip_attn_paged_ragged_dev and returns their bits.
 * EVERY RULE of those entries carries over: opts and its refusals, shapes, strides, alignment, null pointers, n_q = 0, every refusal decided
 * before a device is touched, no synchronize, no allocation, capturable, no atomics, the clamped device-side lengths, the page-id guards (an
 * invalid needed id gives +0.0f rows and no address is formed from it), +0.0f for a row with no visible position.
 * NO NEW PLAN OR WORK-SIZE FUNCTION: the form follows n_q alone (per sequence in the ragged entry), the grids are those of ggml_hip_attn_ex_plan /
 * ggml_hip_attn_paged_ex_plan / ggml_hip_attn_paged_ragged_plan for the same opts, and the work buffer is ggml_hip_attn_work_size /
 * ggml_hip_attn_paged_work_size / ggml_hip_attn_paged_ragged_work_size: ALWAYS ENOUGH, a mask needs no partial the base entry does not have.
 *
 * THE ARITHMETIC.  Everything not named here is the statement of the two forms and of the options above.  Let s_j be the score as the form
 * computes it: scale * dot, or cap * tanhf(sc' * dot) under the soft-cap -- upstream's order, the cap before the mask.  With a mask, for the
 * query row's mask row r:
 *     mk = (float)mask[r][j]                       the exact widening
 *     mk == -inf:  position j is INVISIBLE to the row, in addition to the causal and the window rule
 *     otherwise:   s_j = fmaf(slope_h, mk, s_j)    ONE rounding; slope_h = d_slopes ? d_slopes[h] : 1.0f
 *   DECODE: an invisible position takes part in nothing (it is never multiplied: what the cache holds there does not matter); inside a chunk the
 *     a[d] chain starts at the row's FIRST visible position of the chunk, as under a window, and runs over the visible ones in ascending order.
 *   PROMPT: an invisible position is a zero operand of the matrix core, as above the diagonal.
 *   +inf or NaN in a mask row gives unspecified values in that row and nothing else.
 *   SINKS are unchanged: the denominator only, not biased.  THE WINDOW stays structural: the windowed DECODE grid, c_lo, and the page-table
 *     entries below c_lo[b] that are never read; the mask acts inside it.
 *   FULLY MASKED.  A (row, chunk) whose positions are all invisible -- by the mask alone included -- contributes nothing, anywhere in the walk:
 *     DECODE writes the partial (m = -inf, l = 0, a = 0) for it and the merge's b_c = expf(-inf - M) = 0 adds nothing; PROMPT's online softmax
 *     keeps (m, l, O) across it (alpha = 1, every P = 0) or stays empty (m = -inf).  A row with NO visible position at all writes +0.0f, never
 *     NaN: the merge finds M = -inf (with sinks: M = sink_h, A = 0, dst = 0 / L), PROMPT finds l = 0.
 * CONSEQUENCES (the tests hold the kernels to them bit for bit, in both forms):
 *   1. bias == NULL and a bias with both pointers NULL give the _ex / ragged entry's bits.
 *   2. A mask of +0.0 everywhere without slopes gives the _ex entry's bits (fmaf(1, +0, s) = s; an s of -0 becomes +0, which no later step
 *      tells apart).  d_slopes == NULL gives the bits of slopes all 1.0f.
 *   3. causal = 0 with the causal pattern written into the mask (0 / -inf) gives the bits of causal = 1 without a mask, where no output or V
 *      element is a zero whose sign could differ.
 *   4. Paged equals contiguous per sequence; ragged equals the paged entry called for the sequence alone (n_seq = 1, n_q = n_q[b], the mask
 *      advanced to the sequence's first packed row): the same chunk bodies.  The result does not depend on the page assignment, n_kv_max,
 *      ld_mask, the strides or, without slopes, on n_head.
 *
 * ggml_hip_alibi_slopes (HOST ONLY, no device; the kernels never call powf) is upstream's rule and its definition here, as
 * ggml_hip_rope_table is for rope: with n2 = 2^floor(log2 n_head), m0 = powf(2, -max_bias / n2), m1 = powf(2, -(max_bias / 2) / n2), all binary32:
 *     out[h] = powf(m0, h + 1)               for h <  n2
 *     out[h] = powf(m1, 2 (h - n2) + 1)      for h >= n2
 * and max_bias == 0 gives every slope 1.0f exactly.  n_head outside 1 .. 65535, out == NULL, or a max_bias that is negative or not finite:
 * GGML_HIP_ERR_ARG.  An ALiBi layer passes the mask -(P - j) (or upstream's own mask tensor) and these slopes. */
typedef struct ggml_hip_attn_bias_t {
    const void  *d_mask;    /* device f16 [rows][ld_mask], or NULL: none */
    int64_t      ld_mask;   /* halves between mask rows */
    const float *d_slopes;  /* device f32 [n_head], or NULL: every slope 1.0f */
} ggml_hip_attn_bias_t;
int    ggml_hip_alibi_slopes(int n_head, float max_bias, float *out);
int    ggml_hip_attn_bias_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                              const void *d_k, const void *d_v, int64_t nb_pos, int64_t nb_head,
                              int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max,
                              int causal, float scale, const ggml_hip_attn_opts_t *opts, const ggml_hip_attn_bias_t *bias,
                              float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);
int    ggml_hip_attn_paged_bias_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                                    const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                    const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq,
                                    int n_head, int n_head_kv, int D, int64_t n_q, int64_t n_kv_max,
                                    int causal, float scale, const ggml_hip_attn_opts_t *opts, const ggml_hip_attn_bias_t *bias,
                                    float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);
int    ggml_hip_attn_paged_ragged_bias_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head,
                                           const void *d_k, const void *d_v, int64_t nb_page, int64_t nb_pos, int64_t nb_head, int n_pages,
                                           const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int add_q, int len_bias, int64_t n_seq,
                                           const int32_t *d_q_start, int64_t n_tokens_max, int64_t n_dec_rows_max,
                                           int n_head, int n_head_kv, int D, int64_t n_kv_max,
                                           int causal, float scale, const ggml_hip_attn_opts_t *opts, const ggml_hip_attn_bias_t *bias,
                                           float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);

/* ---------------- THE ENDS OF A DECODE STEP: a token id -> its embedding row; the LM head's logits -> the next token id ----------------
 * Upstream's ggml_get_rows over the token-embedding matrix and its ggml_argmax / top-k -> temperature -> softmax -> top-p -> pick sampler
 * chain, EXTENSIONS like rope (the reference lists get_rows and never dispatches it): device entries only.  With them a captured decode step
 * is a closed loop, d_token -> get_rows -> the layers -> logits -> sample -> d_token: the int32 the sampler writes is the one get_rows reads
 * on the next replay, and with tied embeddings the matrix get_rows reads is the LM head's own resident weight.  Every entry is stream-ordered
 * on `stream`; none synchronizes or allocates, scratch is the caller's, all may be captured; no atomics, results independent of scheduling.
 * Every refusal below is decided before a device is touched.
 *
 * ggml_hip_get_rows_dev:  d_dst[i * ldd + k] = dequantize(W[d_ids[i]])[k], k < K, i < n_ids; d_ids an int32 array on the device.
 *   THE CONTRACT: a gathered row is bit for bit ggml_hip_weight_download of that row followed by the type's dequantize row function
 *   (ggml_hip_dequantize_rows_dev); F32: the row itself; F16 / BF16: the exact widening.  The planes a weight is resident in hold the block
 *   fields of its file format or values its dequantizer computes first and exactly, so nothing is added to a weight for this and nothing is
 *   copied: every type that can be a resident weight is served (ggml_hip_get_rows_serves_for: 1; any other id 0, and the entry returns
 *   GGML_HIP_ERR_TYPE) -- Q4_0, Q4_1, Q4_2, Q5_0, Q5_1, Q8_0, F16, F32, BF16, IQ4_NL, IQ4_XS, Q2_K, Q3_K, Q4_K, Q5_K, Q6_K.
 *   An id outside [0, M) writes a row of +0.0f and no address is formed from it (upstream asserts; a device-side id cannot be asserted on
 *   without a synchronize).  Repeated ids are fine.  Columns K .. ldd-1 of d_dst and rows past n_ids are not written.  d_dst may not overlap
 *   the weight.  16-byte stores where d_dst is 16-byte aligned and ldd % 4 == 0, one element at a time otherwise: the same bits.
 *   n_ids = 0: returns 0 and writes nothing.  n_ids < 0, or a null w / d_ids / d_dst: GGML_HIP_ERR_ARG.  n_ids > 2^20 or ldd < K:
 *   GGML_HIP_ERR_SHAPE.  d_ids and d_dst must be 4-byte aligned (GGML_HIP_ERR_ARG).  Out of scope: rows of anything but a resident weight, a
 *   backward pass, i32 / f16 outputs. */
int ggml_hip_get_rows_serves_for(int type);                       /* host only: 1 / 0 */
int ggml_hip_get_rows_dev(const ggml_hip_weight *w, const int32_t *d_ids, int64_t n_ids, float *d_dst, int64_t ldd, void *stream);
/* THE SAMPLER.  d_logits: f32, [n_rows] rows of n_vocab, ld >= n_vocab elements apart (the dst of ggml_hip_mul_mat_dev for the LM head).
 *   SELECTION is ggml_hip_moe_route_dev's rule, so a row's ids are defined bit for bit:
 *     - d_ids[r * k + s] is the index of rank s under "larger logit first; equal logits: smaller index first";
 *     - -0.0 and +0.0 compare equal;
 *     - a NaN ranks below every non-NaN value, -inf included; NaNs rank among themselves by index;
 *     - so a row's k ids are distinct and inside [0, n_vocab) whatever the logits hold.
 *   ggml_hip_argmax_rows_dev is k = 1 with no probabilities (d_ids[r]): upstream's ggml_argmax with the tie and NaN cases defined.
 *   PROBABILITIES (d_probs[r * k + s]), every operation one binary32 rounding, expf the correctly-specified library function, l_s the rank-s
 *   logit (a zero taken as +0.0):
 *       e_s = expf((l_s - l_0) * inv_temp);   S = e_0 + e_1 + ... + e_(k-1), summed sequentially in rank order;   p_s = e_s / S
 *   -- upstream's top-k, then temperature, then softmax.
 *   TOP-P AND THE PICK are defined on the p_s the entry wrote, by sequential f32 sums, so given d_probs they are bit-defined:
 *       n_keep = the smallest n >= 1 with p_0 + .. + p_(n-1) >= top_p, or k if there is none; top_p >= 1: k, without summing
 *       C      = p_0 + .. + p_(n_keep-1);   target = d_u[r] * C
 *       d_token[r] = the id of the first s < n_keep whose running sum p_0 + .. + p_s exceeds target, or of rank n_keep - 1 if none does
 *   d_u: the caller's uniforms in [0, 1), one per row, on the device -- the host refreshes them between replays; the library has no RNG.
 *   d_u == NULL or d_token == NULL: no pick.  d_probs == NULL is allowed only when there is no pick.  A row whose rank-0 logit is NaN or
 *   +-inf has UNSPECIFIED d_probs and d_token, but d_token is still one of the row's k ids and the ids still follow the rule.
 *   A row's outputs depend on its logits and the parameters alone: not on n_rows, ld or the alignment of d_logits (16-byte loads where
 *   d_logits is 16-byte aligned and ld % 4 == 0).
 *   TWO LAUNCHES whatever the shape: every (row, chunk of ggml_hip_topk_chunk() logits) gives its best min(k, chunk length) keys to the work
 *   buffer, then one workgroup per row merges them and its first wave does the arithmetic above.  The chunk length is a constant of the
 *   library, a multiple of 256.
 *   d_work / work_bytes: ggml_hip_topk_work_size(n_rows, n_vocab, k) bytes, 8-byte aligned (argmax_rows: k = 1); monotone in all three, 0
 *   only for a refused shape.  Missing, misaligned or short: GGML_HIP_ERR_ARG.
 *   1 <= n_vocab <= 2^20, 1 <= k <= min(n_vocab, 64), 1 <= n_rows <= 4096, ld >= n_vocab: else GGML_HIP_ERR_SHAPE.  A null d_logits or
 *   d_ids, inv_temp not finite or <= 0, or a d_logits, d_ids, d_u, d_probs or d_token that is not 4-byte aligned: GGML_HIP_ERR_ARG.
 *   n_rows = 0: returns 0 and writes nothing. */
int64_t ggml_hip_topk_chunk(void);                                 /* host only: the chunk length stage 1 gives a workgroup */
size_t  ggml_hip_topk_work_size(int64_t n_rows, int64_t n_vocab, int k);
int ggml_hip_argmax_rows_dev(const float *d_logits, int64_t ld, int64_t n_rows, int64_t n_vocab,
                             int32_t *d_ids, void *d_work, size_t work_bytes, void *stream);
int ggml_hip_sample_topk_dev(const float *d_logits, int64_t ld, int64_t n_rows, int64_t n_vocab, int k,
                             float inv_temp, float top_p, const float *d_u,
                             int32_t *d_ids, float *d_probs, int32_t *d_token,
                             void *d_work, size_t work_bytes, void *stream);

/* ---------------- SSM: the causal conv and the selective scan of a Mamba / Mamba-2 block over a ragged batch and a pool of state slots ----------------
 * Upstream's ggml_ssm_conv and ggml_ssm_scan, EXTENSIONS like rope (the reference lists nothing): device entries only.  With the in / out
 * projections, ggml_hip_silu_mul_rows_dev, the norms and the sampler they serve a recurrent layer, and a hybrid model that interleaves such layers
 * with attention, inside one captured step.  Both entries are stream-ordered on `stream` on the current device; neither synchronizes or allocates;
 * both may be captured; no atomics and no hand-off between workgroups.  Every refusal below is decided before a device is touched.
 *
 * THE BATCH (shared by both entries) is the ragged batch of the RAGGED PAGED ATTENTION section: packed rows, d_q_start int32 [n_seq + 1] on the device
 *   (never NULL: GGML_HIP_ERR_ARG; 4-byte aligned, else GGML_HIP_ERR_SHAPE), n_tokens_max 0 .. 2^20 (negative: GGML_HIP_ERR_ARG; above:
 *   GGML_HIP_ERR_SHAPE), 1 <= n_seq <= 4096 (else GGML_HIP_ERR_SHAPE).  Sequence b is PRESENT when 0 <= d_q_start[b] <= d_q_start[b+1] <= n_tokens_max;
 *   n_q[b] = 0 is an idle slot.  An idle sequence and one that is not present write nothing, neither rows nor state, and no address is formed from
 *   their bounds.  Rows that belong to no present sequence are not written.  Every sequence is looked at by itself (as attention does), so a present
 *   sequence is served whatever the others' bounds are; present sequences that overlap are the caller's error.  n_tokens_max = 0 returns 0 and
 *   writes nothing (after every other check).
 * THE STATE CACHE.  d_state: a pool of n_slots >= 1 f32 slots (n_slots < 1: GGML_HIP_ERR_ARG), slot s at d_state + s * nb_slot bytes; d_state 16-byte
 *   aligned, nb_slot a multiple of 16 and at least the slot's bytes (ggml_hip_ssm_conv_state_bytes / ggml_hip_ssm_state_bytes), n_slots * nb_slot
 *   <= 2^48: else GGML_HIP_ERR_SHAPE.  d_slot: int32 [n_seq] on the device: sequence b uses slot d_slot[b].  An id outside [0, n_slots) makes the
 *   sequence's output rows +0.0f and writes no state; no address is ever formed from such an id.  Two present sequences that name one slot are the
 *   caller's error.  d_len: int32 [n_seq] on the device, the array attention takes: d_len[b] == 0 is a FRESH sequence, which starts from an all-zero
 *   state -- the slot's old contents are NOT read, so NaN bytes left there do not matter -- and d_len[b] != 0 continues from the slot.  A replayed
 *   graph therefore follows admissions and evictions with no host memset.  NULL d_len / d_slot / d_state: GGML_HIP_ERR_ARG; d_len / d_slot not
 *   4-byte aligned: GGML_HIP_ERR_SHAPE.  AFTER THE CALL the slot of a present, non-idle sequence holds the state after its last token; every other
 *   slot, and the bytes between slots, are untouched.  A state element is read at most once and written at most once per call: one token per
 *   sequence moves the state twice and nothing more.
 *
 * ggml_hip_ssm_conv_ragged_dev: upstream's ggml_ssm_conv with its rolling window.  d_x, d_dst: f32 [n_tokens_max][n_ch], ldx / ldd >= n_ch apart;
 *   d_w: f32 [n_ch][d_conv] contiguous; d_bias: f32 [n_ch] or NULL; a slot is [d_conv - 1][n_ch] f32, oldest row first.  1 <= n_ch <= 2^24 and
 *   2 <= d_conv <= 4, else GGML_HIP_ERR_SHAPE; act 0 (none) or 1 (silu), else GGML_HIP_ERR_ARG.  NULL d_x / d_w / d_dst: GGML_HIP_ERR_ARG; a pointer
 *   that is not 4-byte aligned: GGML_HIP_ERR_SHAPE.  d_dst == d_x (with ldd == ldx) is allowed; any other overlap is not.
 *   THE STATEMENT.  For token t of sequence b and channel c let win be the slot's d_conv - 1 rows (zeros for a fresh sequence) followed by the
 *   sequence's rows of this call.  Every operation is one binary32 rounding:
 *       acc = w[c][0] * win[t][c];   acc = fmaf(w[c][k], win[t + k][c], acc) for k = 1 .. d_conv - 1 ascending;   acc = acc + bias[c] if given;
 *       act = 1:  dst = acc / (1.0f + expf(-acc))     -- plain f32 with the library's expf, NOT the reference's f16-table silu
 *   and the new slot is the last d_conv - 1 rows of win (for n_q[b] < d_conv - 1 that keeps old rows).  THE CONTRACT: act = 0 is bit for bit the
 *   statement; act = 1 is within 3 * 2^-24 relative of the silu of those bits (expf within 1 ulp).  The slot is bit for bit.  Nothing depends on
 *   the other sequences, the slot number, n_tokens_max, the strides or on how a sequence's tokens are split over calls.
 *   One launch: one thread per (sequence, channel) walks the sequence's tokens.  That is right for decode; a long prefill is served by
 *   ggml_hip_ssm_conv_tiled_ragged_dev below, which gives the same bits.
 *
 * ggml_hip_ssm_scan_ragged_dev: upstream's ggml_ssm_scan in both of its forms.  n_head heads of head_dim P (1 .. 256), d_state N (a multiple of 16,
 *   at most 256), n_group G dividing n_head, 1 <= n_head <= 2^20: else GGML_HIP_ERR_SHAPE.  A slot is [n_head][P][N] f32.
 *   d_x, d_dst: f32 [n_tokens_max][n_head][P], token / head strides ldx_tok, ldx_head (ldd_tok, ldd_head) >= P elements; d_dst may not overlap an input.
 *   d_dt:  f32 [n_tokens_max][n_head], ld_dt >= n_head apart.  d_dt_bias: f32 [n_head] or NULL.
 *   d_A:   f32 [n_head][a_ld].  a_per_state = 0: A_n = A[h][0] for every n, a_ld >= 1 (Mamba-2).  a_per_state = 1: A_n = A[h][n], a_ld >= N and a
 *          multiple of 4, d_A 16-byte aligned (Mamba-1, where P = 1 and n_head = d_inner).  Another value: GGML_HIP_ERR_ARG.
 *   d_B, d_C: f32 [n_tokens_max][G][N], both ld_bc >= G * N apart, ld_bc a multiple of 4, both 16-byte aligned.  Head h reads group h / (n_head / G).
 *   d_D:   f32 [n_head] or NULL.
 *   A stride or alignment outside these: GGML_HIP_ERR_SHAPE.  NULL d_x / d_dt / d_A / d_B / d_C / d_dst: GGML_HIP_ERR_ARG.
 *   THE STATEMENT, per token of a sequence in order, for head h, row p and state n; every operation is one binary32 rounding, expf and log1pf the
 *   library's functions; h_n is the state element (zero for a fresh sequence):
 *       d     = dt[t][h] + dt_bias[h]                       (d = dt[t][h] without a bias)
 *       delta = d <= 20.0f ? log1pf(expf(d)) : d
 *       a_n   = expf(delta * A_n)
 *       h_n   = fmaf(h_n, a_n, (delta * x[t][h][p]) * B[t][g][n])
 *       s_j   = h_16j * C_16j;   s_j = fmaf(h_n, C[t][g][n], s_j) for n = 16 j + 1 .. 16 j + 15 ascending        (slice j of 16 states, j < N / 16)
 *       THE BUTTERFLY: with L = N / 16 and LP the least power of two >= L, s_j = +0.0f for L <= j < LP; then for d = 1, 2, 4, .. < LP in this order
 *                      every s_j becomes s_j + s_(j xor d), all j at once.  y = s_0 (every s_j holds the same bits).
 *       y     = fmaf(D[h], x[t][h][p], y) if D is given;    dst[t][h][p] = y
 *   THREE BIT-LEVEL CONTRACTS: (i) a sequence's rows and final state are bit for bit those of a call with n_seq = 1; (ii) splitting a sequence's
 *   tokens over several calls at any point gives the same bits as one call; (iii) nothing depends on the other sequences, the slot number,
 *   n_tokens_max or the strides.
 *   ONE FORM (ggml_hip_ssm_scan_plan, host only, shows it): sequential over a sequence's tokens, one lane per (sequence, head, p, slice); a state row
 *   rides in the registers of an aligned group of LP lanes (lanes_per_row; L of them work) and the butterfly is lane moves inside the group.  One
 *   launch of ceil(n_head * P * LP / 256) * n_seq workgroups, sized by the shape and n_seq alone.
 *   LIMITS.  That form is exactly right for decode.  A long prefill walks its tokens one after the other with n_head * P * LP lanes: the chunked
 *   matrix form (SSD) for long prefills is ggml_hip_ssm_scan_chunked_ragged_dev below, and the conv's token-parallel form for them is
 *   ggml_hip_ssm_conv_tiled_ragged_dev behind it.  N that is no
 *   power-of-two multiple of 16 idles LP - L lanes of a group.  States are f32 only.
 * ggml_hip_ssm_state_bytes / ggml_hip_ssm_conv_state_bytes (host only): the bytes of one slot, n_head * P * N * 4 and (d_conv - 1) * n_ch * 4; 0 for a
 *   shape the entries refuse.
 *
 * ggml_hip_ssm_scan_chunked_ragged_dev: the same scan with a SECOND FORM for long sequences, picked PER SEQUENCE from its own count in this call (as
 *   ragged attention picks DECODE or PROMPT), so one call takes a mixed continuous-batching step.  Every argument of ggml_hip_ssm_scan_ragged_dev with
 *   the same meaning and the same refusals, and d_work / work_bytes: at least ggml_hip_ssm_scan_chunked_work_size(..) bytes, any alignment, else
 *   GGML_HIP_ERR_ARG (a size of 0 needs no buffer; NULL is accepted then).  Nothing in the buffer is read before the call has written it.  Stream-ordered,
 *   capturable, no synchronize, no allocation, no atomics; every grid is sized by the shape, n_seq and n_tokens_max alone, so a captured graph follows
 *   d_q_start, d_len and d_slot between replays -- a sequence may move from one form to the other.
 *   SHORT: a sequence of 1 .. seq_max_tokens tokens runs the sequential kernel: its rows and state are bit for bit ggml_hip_ssm_scan_ragged_dev's.
 *   LONG: a longer sequence runs the CHUNKED form where the shape is served by it: a_per_state = 0 and head_dim a multiple of 16 (16 .. 256), every
 *   d_state.  Any other shape is NOT refused: the plan says form = 1 and every sequence runs sequential (Mamba-1's per-state A has a decay mask that
 *   depends on n: no matrix form exists).  Absent and idle sequences, slot ids outside the pool (+0.0f rows, no state written, no address formed) and
 *   fresh sequences over NaN slots behave as above.  Present sequences that overlap are still the caller's error; they write nothing outside dst,
 *   the slots and the work buffer (the chunk list is clamped at chunks_max).
 *   THE CHUNKED STATEMENT.  Chunks of Q = chunk tokens are counted from the sequence's first row OF THIS CALL; the last may be partial.  Per head h, with
 *   d, delta as above and every operation one binary32 rounding:
 *       la_t = delta_t * A[h][0];   cs_t = cs_(t-1) + la_t inside the chunk, ascending, cs_(-1) = +0.0f;   xd_s = delta_s * x[s][h][p]
 *       S[p][n]     = sum_s (xd_s[p] * expf(cs_last - cs_s)) * B[s][g][n]              (s ascending over the chunk's tokens, an fmaf chain from +0.0f)
 *       H_in        = the slot (zeros for a fresh sequence) for the first chunk, else H_out of the chunk before, as the f32 that went through memory
 *       H_out[p][n] = fmaf(H_in[p][n], expf(cs_last), S[p][n])                         (the last chunk's H_out is the new slot)
 *       G[t][s]     = sum_n C[t][g][n] * B[s][g][n];   M[t][s] = expf(cs_t - cs_s) * G[t][s] for s <= t
 *       y[t][p]     = sum_n (expf(cs_t) * C[t][g][n]) * H_in[p][n] + sum_(s <= t) M[t][s] * xd_s[p]       (ONE fmaf chain from +0.0f, the n first)
 *       y           = fmaf(D[h], x[t][h][p], y) if D is given
 *   The sums over n run in the order n = 16 kb + 4 kq + c with kb, then c, then kq ascending (the f32-input MFMA's k order over float4 loads); the sum
 *   over s <= t runs over every s below the next multiple of 16 above t, ascending, the masked terms being +0.0f * xd_s.
 *   A decay is ONE expf of a difference of running sums, which is <= 0; never a quotient or product of separately exponentiated sums.  A mask -- s > t,
 *   the rows beyond a partial chunk, the rows beyond the sequence -- is a SELECT: those rows are not loaded and may hold anything.
 *   CONTRACTS.  Rows and final state are within the bar DERIVED in tests/np_ssm_chunk.py of the float64 sequential statement; that bar is wider than
 *   the sequential form's (DESIGN.md section 26 has the ratio).  Bit level: (i) a sequence alone in a call gives the same bits; (iii) nothing depends
 *   on the other sequences, the slot number, n_tokens_max, the strides or the work buffer's address and old contents; (ii') splitting a sequence at a
 *   multiple of Q gives the bits of one call when both parts are longer than seq_max_tokens.  Contract (ii) of ggml_hip_ssm_scan_ragged_dev does NOT
 *   hold at other split points (the chunk boundaries move): a caller who needs it keeps using that entry.
 * ggml_hip_ssm_scan_chunked_plan / ggml_hip_ssm_scan_chunked_work_size (host only): what a call with these bounds does, and the bytes of its work
 *   buffer (0 for a refused shape and where no sequence can be chunked).  chunk and seq_max_tokens follow the shape alone, never the batch.
 *
 * ggml_hip_ssm_conv_tiled_ragged_dev: the same conv with a SECOND, token-parallel FORM for long sequences, picked PER SEQUENCE from its own count in this
 *   call as the chunked scan does, so one captured call serves a whole ragged step.  Every argument of ggml_hip_ssm_conv_ragged_dev with the same
 *   meaning and the same refusals, and d_work / work_bytes: at least ggml_hip_ssm_conv_tiled_work_size(..) bytes, any alignment, else GGML_HIP_ERR_ARG
 *   (a size of 0 needs no buffer; NULL is accepted then).  Nothing in the buffer is read before the call has written it.  Stream-ordered, capturable,
 *   no synchronize, no allocation, no atomics, no hand-off between workgroups of one launch; every grid is sized by the shape, n_seq and n_tokens_max
 *   alone, so a captured graph follows d_q_start, d_len and d_slot between replays -- a sequence may move from one form to the other.  n_tokens_max = 0
 *   returns 0 after every other check.
 *   SHORT: a sequence of 1 .. seq_max_tokens tokens runs the sequential kernel; where n_tokens_max <= seq_max_tokens the plan says form = 1 and the call
 *   is exactly ggml_hip_ssm_conv_ragged_dev's one launch.
 *   LONG: a longer sequence runs in TILES of `tile` tokens counted from the sequence's first row OF THIS CALL (the last may be partial), one thread per
 *   (tile, 4 adjacent channels) with 16-byte loads and stores where n_ch, ldx and ldd are multiples of 4 and d_x, d_dst, d_w and d_bias are 16-byte
 *   aligned, else one thread per (tile, channel) with the same bits.  The d_conv - 1 rows in front of every tile -- the slot's for a sequence's first
 *   tile, zeros where it is fresh -- are staged in the work buffer before any row is written, and the thread that stages a slot element is the one that
 *   then writes it from the sequence's last d_conv - 1 input rows.
 *   THE CONTRACT is ggml_hip_ssm_conv_ragged_dev's, unchanged, in both forms: the statement is a fixed fma chain per token, so rows (act = 0) and the slot
 *   are bit for bit the statement and act = 1 is the same expression on those bits.  (i) a sequence alone in a call gives the same bits; (ii) splitting a
 *   sequence's tokens over calls at ANY point gives the same bits, also where a part moves from one form to the other; (iii) nothing depends on the
 *   other sequences, the slot number, n_tokens_max, the strides or the work buffer's address and old contents.  Absent and idle sequences, slot ids
 *   outside the pool (+0.0f rows, no state written, no address formed) and fresh sequences over NaN slots behave as above.  d_dst == d_x (with
 *   ldd == ldx) is allowed and gives the bits of the out-of-place call.  Present sequences that overlap are still the caller's error; they write nothing
 *   outside dst, the slots and the work buffer (the tile list is clamped at tiles_max).
 * ggml_hip_ssm_conv_tiled_plan / ggml_hip_ssm_conv_tiled_work_size (host only): what a call with these bounds does, and the bytes of its work buffer
 *   (0 for a refused shape and where no sequence can be long).  tile and seq_max_tokens follow the shape alone, never the batch. */
typedef struct ggml_hip_ssm_conv_plan_t {
    int32_t form, tile;                      /* 1: every sequence sequential; 2: tiled above seq_max_tokens.  T, in tokens */
    int32_t seq_max_tokens, launches;        /* a sequence with at most this many tokens in the call runs sequential; launches of one call (1 or 4) */
    int32_t vec, reserved;                   /* channels per thread of the tile kernel for aligned operands: 4 where n_ch is a multiple of 4, else 1; 0 */
    int64_t tiles_max, seqs_max;             /* the tile list's and the long sequences' bounds over every batch inside n_seq and n_tokens_max.  0 for form 1 */
    uint64_t work_bytes;                     /* ggml_hip_ssm_conv_tiled_work_size */
} ggml_hip_ssm_conv_plan_t;
typedef struct ggml_hip_ssm_chunk_plan_t {
    int32_t form, chunk;                     /* 1: every sequence sequential; 2: chunked above seq_max_tokens.  Q, in tokens */
    int32_t seq_max_tokens, launches;        /* a sequence with at most this many tokens in the call runs sequential; launches of one call (1 or 5) */
    int32_t p_tile, p_tiles;                 /* rows of P a workgroup of the state / out kernels owns (16, 32, 64); head_dim / p_tile.  0 for form 1 */
    int32_t kernel_state, kernel_out;        /* the compiled forms of the two matrix kernels: their p_tile.  0 for form 1 */
    int64_t chunks_max, seqs_max;            /* the chunk list's and the chunked sequences' bounds over every batch inside n_seq and n_tokens_max */
    uint64_t work_bytes;                     /* ggml_hip_ssm_scan_chunked_work_size */
} ggml_hip_ssm_chunk_plan_t;
typedef struct ggml_hip_ssm_plan_t {
    int32_t form, launches;                  /* 1: sequential over tokens, parallel over (sequence, head, p, slice); launches of one call (1) */
    int32_t slices, lanes_per_row;           /* L = N / 16; LP, the lanes of a state row's group */
    int64_t rows_per_workgroup, workgroups;  /* 256 / LP; ceil(n_head * P / rows_per_workgroup) * n_seq */
} ggml_hip_ssm_plan_t;
size_t ggml_hip_ssm_conv_state_bytes(int64_t n_ch, int d_conv);
size_t ggml_hip_ssm_state_bytes(int n_head, int head_dim, int d_state);
int    ggml_hip_ssm_scan_plan(int n_head, int head_dim, int d_state, int n_group, int64_t n_seq, ggml_hip_ssm_plan_t *out);
int    ggml_hip_ssm_conv_ragged_dev(const float *d_x, int64_t ldx, const float *d_w, const float *d_bias, int act, int64_t n_ch, int d_conv,
                                    int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot,
                                    float *d_state, int64_t nb_slot, int64_t n_slots, float *d_dst, int64_t ldd, void *stream);
int    ggml_hip_ssm_scan_ragged_dev(const float *d_x, int64_t ldx_tok, int64_t ldx_head, const float *d_dt, int64_t ld_dt, const float *d_dt_bias,
                                    const float *d_A, int64_t a_ld, int a_per_state, const float *d_B, const float *d_C, int64_t ld_bc,
                                    const float *d_D, int n_head, int head_dim, int d_state_n, int n_group,
                                    int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot,
                                    float *d_state, int64_t nb_slot, int64_t n_slots, float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *stream);
size_t ggml_hip_ssm_scan_chunked_work_size(int n_head, int head_dim, int d_state, int n_group, int a_per_state, int64_t n_seq, int64_t n_tokens_max);
int    ggml_hip_ssm_scan_chunked_plan(int n_head, int head_dim, int d_state, int n_group, int a_per_state, int64_t n_seq, int64_t n_tokens_max,
                                      ggml_hip_ssm_chunk_plan_t *out);
int    ggml_hip_ssm_scan_chunked_ragged_dev(const float *d_x, int64_t ldx_tok, int64_t ldx_head, const float *d_dt, int64_t ld_dt, const float *d_dt_bias,
                                            const float *d_A, int64_t a_ld, int a_per_state, const float *d_B, const float *d_C, int64_t ld_bc,
                                            const float *d_D, int n_head, int head_dim, int d_state_n, int n_group,
                                            int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot,
                                            float *d_state, int64_t nb_slot, int64_t n_slots, float *d_dst, int64_t ldd_tok, int64_t ldd_head,
                                            void *d_work, size_t work_bytes, void *stream);
size_t ggml_hip_ssm_conv_tiled_work_size(int64_t n_ch, int d_conv, int64_t n_seq, int64_t n_tokens_max);
int    ggml_hip_ssm_conv_tiled_plan(int64_t n_ch, int d_conv, int64_t n_seq, int64_t n_tokens_max, ggml_hip_ssm_conv_plan_t *out);
int    ggml_hip_ssm_conv_tiled_ragged_dev(const float *d_x, int64_t ldx, const float *d_w, const float *d_bias, int act, int64_t n_ch, int d_conv,
                                          int64_t n_seq, const int32_t *d_q_start, int64_t n_tokens_max, const int32_t *d_len, const int32_t *d_slot,
                                          float *d_state, int64_t nb_slot, int64_t n_slots, float *d_dst, int64_t ldd,
                                          void *d_work, size_t work_bytes, void *stream);


/* ---------------- MLA: multi-head LATENT attention (absorbed form) over a latent KV cache, on the f16 matrix cores ----------------
 * The attention of DeepSeek-V2 / V3 / R1 and Kimi K2 in the absorbed form, an EXTENSION like attention: device-resident entries only.  Every query head
 * reads ONE shared cache row per position.
 * THE CACHE ROW: D_k = 576 elements in the reference block format ggml_hip_kv_store_dev writes (F16: 1152 bytes; Q8_0: 18 blocks, 648 bytes), the row
 *   of position j at base + j * nb_pos.  Elements 0 .. 511 are the compressed latent and ARE the value, elements 512 .. 575 are the rotated key part.
 *   q is f32 [rows][n_head][576] in the same order, dst f32 [rows][n_head][512].  Only (D_k, D_v) = (576, 512) is served; 1 <= n_head <= 256.
 *   There is ONE cache pointer: K and V are the same bytes.  No mask, window, soft-cap or sinks: they are not parameters at all.
 * THE ROTATION of the key part stays the caller's.  The recipe for rows x f32 [n_tok][576] (row stride ld): call ggml_hip_rope_dev in place on the last 64
 *   columns as a one-head view -- d_x = d_dst = x + 512, ldx_tok = ldd_tok = ld, ldx_head = ldd_head = 64, n_head = 1, D = 64 -- then store the rows:
 *   ggml_hip_kv_store_dev with row_elems = 576 into a contiguous cache, ggml_hip_kv_store_latent_paged_dev into a paged one.
 * A ROW of the problem is a pair (t, h), r = t * n_head + h; all rows share the cache.  vis(t) = causal ? clamp(n_kv - n_q + t + 1, 0, n_kv) : n_kv as
 *   in ggml_hip_attn_dev.  n_kv is the host's, or *d_n_kv (an int32 on the device) clamped to [0, n_kv_max]; n_kv_max sizes every launch.
 * THE ARITHMETIC (fixed): the operands are the PROMPT form's.  Q is rounded to f16 (RNE) once.  An F16 row is staged as it lies, a Q8_0 row is
 *   dequantized while staged: f16((float)q * d).  Positions at or beyond n_kv are staged as ZEROS: what the cache holds there, NaN bytes included, does
 *   not matter (below n_kv the cache must hold finite values: a masked weight is a zero operand).  The positions are walked in STEPS of `step` = 64, two
 *   per chunk of 128, ascending; per step, all on v_mfma_f32_32x32x16_f16 with f32 accumulation:
 *     S = Q K^T over all 576 elements;  s = scale * S in f32, an invisible j is -inf;  m' = max(m, max s);  alpha = expf(m - m') (0 while m = -inf);
 *     P = f16(expf(s - m')), 0 where invisible;  l = l * alpha + sum of the ROUNDED P;  O = O * alpha + P V over the first 512 columns.
 *   A step without a visible position of a row leaves the row's (m, l, O) as they are (alpha = 1, every P = 0).
 * TWO FORMS, chosen from n_q alone -- never from the device, the grid, n_head, n_seq or n_kv_max:
 *   WALK (n_q > 8): a workgroup owns a tile of 64 consecutive rows and walks the steps that hold a visible position of any of them; dst = O / l.  No work
 *     buffer.
 *   SPLIT (n_q <= 8): the positions are cut into SPANS of `span` chunks (one compile-time constant, reported in the plan).  A workgroup runs the same step
 *     body over one span for its row tile and writes the unnormalised partial (m, l, O[512]) to the work buffer; a (row, span) with no visible position has no
 *     partial.  A second launch merges a row's partials: M = max m_s; b_s = m_s == M ? 1 : expf(m_s - M); L and A[d] are fma chains over the spans in
 *     ASCENDING order, the first term the product; dst = A / L.
 *   A row with no visible position is +0.0f in both.  Work size: rows * ceil(n_kv_max / (128 * span)) * (512 + 4) floats, rounded up to 256 bytes plus 256
 *   (the base is aligned by the entry); 0 for WALK; monotone in every argument.
 * THE CONTRACTS, as bits:
 *   1. One visible position: dst is the staged V row bit for bit -- deq(V_0) for F16, f16(deq(V_0)) for Q8_0 -- in both forms.
 *   2. A row's bits depend on its own q row, the cache bytes below its vis, scale, the cache type and the form ONLY: not on n_head, the row's place in a
 *      tile, the strides, n_kv_max, where n_kv comes from, or n_q within the form (row t of one call equals a row with the same vis of another call of
 *      that form).
 *   3. Paged equals contiguous per sequence, bit for bit: one step body, which does not know where a chunk lies.  Nothing depends on the page assignment,
 *      n_pages, ld_pages, nb_page, n_seq or the slot.
 * ggml_hip_attn_mla_dev: q, dst and d_cache 16-byte aligned; ldq_* / ldd_* multiples of 4 elements, ldq_head >= 576, ldd_head >= 512 (and the token strides
 *   where there is more than one token); nb_pos a multiple of 16, at least a row's bytes; n_q <= 2^20, n_kv_max <= 2^24, n_q * n_head < 2^31.  d_work /
 *   work_bytes: at least ggml_hip_attn_mla_work_size(..), else GGML_HIP_ERR_ARG.  A wrong kv_type is GGML_HIP_ERR_TYPE, a refused shape, stride or
 *   alignment GGML_HIP_ERR_SHAPE, a null or short argument GGML_HIP_ERR_ARG; every refusal is decided before a device is touched.  n_q = 0 returns 0 after
 *   the shape and stride checks.  Stream-ordered, no synchronize, no allocation, no atomics; capturable, and a captured call follows *d_n_kv.
 * ggml_hip_attn_mla_paged_dev: n_seq sequences (1 .. 4096) of n_q rows EACH (uniform; a ragged twin is left out), q / dst [n_seq * n_q][n_head][..],
 *   n_seq * n_q <= 2^20 and n_seq * n_q * n_head < 2^31.  The pool, nb_page, nb_pos, n_pages, d_pages, ld_pages, d_len and len_bias are the paged section's
 *   with one row per position (nb_page >= 127 * nb_pos + a row's bytes): n_kv[b] = clamp(d_len[b] + len_bias, 0, n_kv_max); n_kv[b] = 0 gives zero rows; a
 *   page id outside [0, n_pages) among a sequence's first ceil(n_kv[b] / 128) entries zeroes ALL its rows and never becomes an address.  NULL tables are
 *   GGML_HIP_ERR_ARG.
 * ggml_hip_kv_store_latent_paged_dev: rows src f32 [n_seq * n_q][576] (row stride ld, a multiple of 4) -> row (b, t) at position d_len[b] + t of
 *   sequence b.  The bytes written are bit for bit ggml_hip_kv_store_dev(row_elems = 576) for that row (one thread per 32 (Q8_0) or 4 (F16) elements).  A
 *   token whose position is outside [0, n_kv_max), or whose page id is outside [0, n_pages), writes nothing and no address is formed from it.
 *   (ggml_hip_kv_store_paged_dev stops at D = 256, and a Q8_0 row of 648 bytes cannot be expressed as heads.)
 * LEFT OUT: a ragged (d_q_start) twin; window, sinks, soft-cap and mask; other (D_k, D_v); a rope fused into the latent store. */
enum { GGML_HIP_ATTN_MLA_SPLIT = 1, GGML_HIP_ATTN_MLA_WALK = 2 }; /* ggml_hip_attn_mla_plan_t.form */
typedef struct ggml_hip_attn_mla_plan_t {
    int32_t form, chunk;                     /* the form (0 for n_q = 0); positions per chunk (128) */
    int32_t span, q_tile;                    /* chunks per span (MLA_SPAN, in both forms); rows (t, h) a workgroup owns */
    int32_t step, launches;                  /* positions per online-softmax step; launches of one call (SPLIT 2, WALK 1) */
    int64_t n_spans, workgroups;             /* ceil(n_kv_max / (chunk * span)); workgroups of the main launch */
    int64_t merge_workgroups;                /* SPLIT: one per row; WALK 0 */
    uint64_t work_bytes;                     /* ggml_hip_attn_mla_work_size / _paged_work_size */
} ggml_hip_attn_mla_plan_t;
int    ggml_hip_attn_mla_plan(int kv_type, int D_k, int D_v, int n_head, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_mla_plan_t *out);
size_t ggml_hip_attn_mla_work_size(int kv_type, int D_k, int D_v, int n_head, int64_t n_q, int64_t n_kv_max);
int    ggml_hip_attn_mla_paged_plan(int kv_type, int D_k, int D_v, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max, ggml_hip_attn_mla_plan_t *out);
size_t ggml_hip_attn_mla_paged_work_size(int kv_type, int D_k, int D_v, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max);
int    ggml_hip_attn_mla_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_cache, int64_t nb_pos,
                             int n_head, int D_k, int D_v, int64_t n_q, int64_t n_kv, const int32_t *d_n_kv, int64_t n_kv_max, int causal, float scale,
                             float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);
int    ggml_hip_attn_mla_paged_dev(int kv_type, const float *d_q, int64_t ldq_tok, int64_t ldq_head, const void *d_pool, int64_t nb_page, int64_t nb_pos,
                                   int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int len_bias, int64_t n_seq,
                                   int n_head, int D_k, int D_v, int64_t n_q, int64_t n_kv_max, int causal, float scale,
                                   float *d_dst, int64_t ldd_tok, int64_t ldd_head, void *d_work, size_t work_bytes, void *stream);
int    ggml_hip_kv_store_latent_paged_dev(int kv_type, const float *d_src, int64_t ld, int64_t n_seq, int64_t n_q, void *d_pool, int64_t nb_page,
                                          int64_t nb_pos, int n_pages, const int32_t *d_pages, int64_t ld_pages, const int32_t *d_len, int64_t n_kv_max,
                                          void *stream);

#if defined(__GNUC__)
#pragma GCC visibility pop
#endif
#ifdef __cplusplus
}
#endif
#endif /* GGML_HIP_EXT_H */
