// GgmlHip.cs -- P/Invoke declarations for libggml_hip.so (include/ggml_hip.h), to be added to the GGMLSharp project
// (GGMLSharp/GgmlHip.cs).  The text of INTEGRATION.md section 1, as a file a maintainer can drop in; integration/README.md
// says how to build.  NOT compiled here: neither the build image nor the GPU boxes carry a .NET toolchain.
using System.Runtime.InteropServices;

namespace GGMLSharp;

internal static unsafe partial class GgmlHip
{
    const string Lib = "ggml_hip";   // libggml_hip.so on the loader path

    // include/ggml_hip.h -- status codes
    public const int OK = 0, ERR_NO_DEVICE = -1, ERR_TYPE = -2, ERR_SHAPE = -3, ERR_ARG = -4, ERR_RUNTIME = -5;
    // include/ggml_hip_ext.h -- extension weight types (upstream formats; the weight and _dev entries only, never in a ggml_tensor)
    public const int TYPE_Q2_K = 110, TYPE_Q3_K = 111, TYPE_Q4_K = 112, TYPE_Q5_K = 113, TYPE_Q6_K = 114, TYPE_IQ4_NL = 120, TYPE_IQ4_XS = 123,
                     TYPE_BF16 = 130;

    [DllImport(Lib)] public static extern int ggml_hip_device_count();
    [DllImport(Lib)] public static extern int ggml_hip_init(int device);                          // one device slot
    [DllImport(Lib)] public static extern int ggml_hip_init_devices(int nDevices, int* deviceIds);   // n slots: Seam 1 row-splits over them (ids null: 0..n-1)
    [DllImport(Lib)] public static extern int ggml_hip_bind_thread(int slot);                     // this managed thread's seams run on one slot (-1: all)
    [DllImport(Lib)] public static extern void ggml_hip_shutdown();
    [DllImport(Lib)] public static extern sbyte* ggml_hip_last_error();
    // the context pool is ONE allocation (Ggml.cs:1545): register it and Seam 1 moves src1 / dst by asynchronous DMA in chunks
    [DllImport(Lib)] public static extern int ggml_hip_register_host_pool(void* pool, nuint bytes);
    [DllImport(Lib)] public static extern int ggml_hip_unregister_host_pool(void* pool);

    // Seam 1: drop-in for Ggml.ggml_compute_forward_mul_mat (Ggml.cs:6714-6744).
    // ggml_compute_params / ggml_tensor are blittable and laid out exactly as TypeDefinitions.cs:299-308 / 65-99.
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_mul_mat(
        ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* src1, ggml_tensor* dst);
    [DllImport(Lib)] public static extern void ggml_hip_invalidate(void* hostPtr);
    [DllImport(Lib)] public static extern void ggml_hip_invalidate_range(void* hostPtr, nuint bytes);
    [DllImport(Lib)] public static extern void ggml_hip_invalidate_all();
    [DllImport(Lib)] public static extern int ggml_hip_graph_begin();   // results of offloaded nodes stay in HBM for their consumers
    [DllImport(Lib)] public static extern int ggml_hip_graph_begin_keyed(ulong key);   // the same, NAMED: captured / replayed when it recurs
    [DllImport(Lib)] public static extern int ggml_hip_graph_end();     // ... until here; all node data is on the host afterwards
    [DllImport(Lib)] public static extern int ggml_hip_host_read(void* p, nuint bytes);   // a CPU node inside a scope reads an offloaded result
    [DllImport(Lib)] public static extern int ggml_hip_graph_outputs(void** ptrs, int n);  // OPT-IN, not the reference's contract: only these results go home
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_mul_mat_multi(ggml_compute_params* p, int n, ggml_tensor** src0,
        ggml_tensor* src1, ggml_tensor** dst, ggml_tensor* pro_x, ggml_tensor* pro_g, ggml_tensor* pro_norm);   // q / k / v, gate / up: one call

    // neighbours of the path (SURVEY 8(f)): same calling convention, dispatched from ggml_compute_forward (Ggml.cs:8548-8760)
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_cpy(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* dst);           // f32/f16 -> Q
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_add(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* src1, ggml_tensor* dst);   // Q + f32, f32 + f32
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_mul(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* src1, ggml_tensor* dst);
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_scale(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* src1, ggml_tensor* dst);
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_rms_norm(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* dst);
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_silu(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* dst);
    // fused pairs (SURVEY 8(f) row 4): node i and the node i + 1 that consumes it, one call, both nodes' data produced
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_rms_norm_mul(ggml_compute_params* @params, ggml_tensor* x, ggml_tensor* g, ggml_tensor* normDst, ggml_tensor* mulDst);
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_silu_mul(ggml_compute_params* @params, ggml_tensor* a, ggml_tensor* b, ggml_tensor* siluDst, ggml_tensor* mulDst);
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_mul_mat_add(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* src1, ggml_tensor* mmDst, ggml_tensor* addend, ggml_tensor* addDst);
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_mul_mat_scale(ggml_compute_params* @params, ggml_tensor* src0, ggml_tensor* src1, ggml_tensor* mmDst, ggml_tensor* scalar, ggml_tensor* scaleDst);
    // rms_norm, mul, mul_mat [, add]: the pre-projection chain of a decoder block, ONE launch for decode-sized batches (addend / addDst null without an add node)
    [DllImport(Lib)] public static extern int ggml_hip_compute_forward_norm_mul_mat(ggml_compute_params* @params, ggml_tensor* x, ggml_tensor* g, ggml_tensor* normDst, ggml_tensor* mulDst, ggml_tensor* src0, ggml_tensor* mmDst, ggml_tensor* addend, ggml_tensor* addDst);

    // include/ggml_hip_ext.h -- expert-routed products (upstream's ggml_mul_mat_id; a device-resident extension entry: no seam, the reference has no such node).
    // Handles are opaque; the ids, src1, dst and work pointers are DEVICE memory (ggml_hip_slot_malloc / _upload), hIds the same ids in host memory or null.
    [DllImport(Lib)] public static extern int ggml_hip_weight_upload(int type, void* hostRows, long ne00, long ne01, ulong nb01, long rowBegin, long rowEnd, void* stream, void** weight);
    [DllImport(Lib)] public static extern void ggml_hip_weight_free(void* weight);
    [DllImport(Lib)] public static extern int ggml_hip_expert_set_create(void** weights, int nExpert, void* stream, void** set);   // the set does not own the weights
    [DllImport(Lib)] public static extern void ggml_hip_expert_set_free(void* set);
    [DllImport(Lib)] public static extern int ggml_hip_mul_mat_id_route(void* set, long nTokens, int nUsed);            // 1 by-id mat-vec, 2 batch route, < 0 error
    [DllImport(Lib)] public static extern nuint ggml_hip_mul_mat_id_work_size(void* set, long nTokens, int nUsed);
    [DllImport(Lib)] public static extern int ggml_hip_mul_mat_id_route_for(int type, long m, long k, int nExpert, long nTokens, int nUsed);   // no weight, no device needed
    [DllImport(Lib)] public static extern nuint ggml_hip_mul_mat_id_work_size_for(int type, long m, long k, int nExpert, long nTokens, int nUsed);
    [DllImport(Lib)] public static extern int ggml_hip_mul_mat_id_dev(void* set, int* dIds, int* hIds, long nTokens, int nUsed, float* dSrc1, long ld1Token, long ld1Slot,
        float* dDst, long ldd, void* dWork, nuint workBytes, void* stream);
    // ... the grouped route: the ids are read on the device alone (no hIds), a fixed number of launches, capturable; Q8_0 / Q5_0 / IQ4_NL / Q4_0 where it serves
    [DllImport(Lib)] public static extern int ggml_hip_mul_mat_id_grouped_serves(void* set);                             // 1 / 0, < 0 error
    [DllImport(Lib)] public static extern int ggml_hip_mul_mat_id_grouped_serves_for(int type, long m, long k);          // no weight, no device needed
    [DllImport(Lib)] public static extern nuint ggml_hip_mul_mat_id_grouped_work_size(void* set, long nTokens, int nUsed);
    [DllImport(Lib)] public static extern nuint ggml_hip_mul_mat_id_grouped_work_size_for(int type, long m, long k, int nExpert, long nTokens, int nUsed);
    [DllImport(Lib)] public static extern int ggml_hip_mul_mat_id_grouped_dev(void* set, int* dIds, long nTokens, int nUsed, float* dSrc1, long ld1Token, long ld1Slot,
        float* dDst, long ldd, void* dWork, nuint workBytes, void* stream);
    // ... the ends of the block, device entries like the products (stream-ordered, no synchronize, no work buffer, capturable): router logits -> the
    // n_used expert ids and gate weights of every token (gating 0 softmax, 1 sigmoid); the weighted sum of a token's pair rows (+ an addend, which
    // may be dDst itself); the SwiGLU pair on contiguous device rows (dSilu may be null)
    [DllImport(Lib)] public static extern int ggml_hip_moe_route_dev(float* dLogits, long ldLogits, long nTokens, int nExpert, int nUsed, int gating, int normalize, float scale,
        int* dIds, float* dWeights, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_moe_combine_dev(float* dY, long ldy, float* dWeights, long nTokens, int nUsed, long m, float* dAddend, long ldAdd,
        float* dDst, long ldd, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_silu_mul_rows_dev(float* dA, float* dB, float* dSilu, float* dY, long nrows, long k, void* stream);
    // ... attention over an F16 / Q8_0 KV cache (device entries, capturable): f32 rows into the cache at pos0 or at the int32 *dPos0 on the device;
    // softmax(scale Q K^T + causal mask) V over it, n_kv from the host or from the int32 *dNKv on the device (clamped to nKvMax); no mask tensor,
    // ALiBi, soft-cap or sinks (pass null / 0); the plan (form 1 decode, 2 prompt) and the work size need no device
    [DllImport(Lib)] public static extern int ggml_hip_kv_store_dev(int kvType, float* dSrc, long ld, long nRows, long rowElems, void* dCache, long nbPos, long nPosMax,
        long pos0, int* dPos0, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_attn_plan(int kvType, int d, int nHead, int nHeadKv, long nQ, long nKvMax, void* plan);
    [DllImport(Lib)] public static extern nuint ggml_hip_attn_work_size(int kvType, int d, int nHead, int nHeadKv, long nQ, long nKvMax);
    [DllImport(Lib)] public static extern int ggml_hip_attn_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPos, long nbHead,
        int nHead, int nHeadKv, int d, long nQ, long nKv, int* dNKv, long nKvMax, int causal, float scale, void* dMask, float maxBias, float logitSoftcap, float* dSinks,
        float* dDst, long lddTok, long lddHead, void* dWork, nuint workBytes, void* stream);
    // ... the rotary embedding of Q / K rows between the projections and the cache (device entries, capturable): token t sits at dPos[t] (int32 on the
    // device) or at p0 + t, p0 = *dPos0 (int32 on the device) or pos0 -- kv_store's convention; mode 0 NORMAL, 2 NEOX; dFreqFactors (llama-3's) may be
    // null; dDst may be dX (in place).  rope_kv_store: rotate K rows and store them as F16 / Q8_0 cache rows at (p0 + t) * nbPos + hk * nbHead in one
    // launch, bit for bit rope then kv_store.  rope_table: the per-pair constants (eff: nDims / 2 doubles), host only
    [StructLayout(LayoutKind.Sequential)]
    public struct ggml_hip_rope_params_t
    {
        public int n_dims, mode, n_ctx_orig;
        public float freq_base, freq_scale, ext_factor, attn_factor, beta_fast, beta_slow;
    }
    [DllImport(Lib)] public static extern int ggml_hip_rope_table(ggml_hip_rope_params_t* rp, double* eff, double* mscale);
    [DllImport(Lib)] public static extern int ggml_hip_rope_dev(ggml_hip_rope_params_t* rp, float* dX, long ldxTok, long ldxHead, int nHead, int d, long nTokens,
        int* dPos, long pos0, int* dPos0, float* dFreqFactors, float* dDst, long lddTok, long lddHead, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_rope_kv_store_dev(ggml_hip_rope_params_t* rp, int kvType, float* dX, long ldxTok, long ldxHead, int nHeadKv, int d,
        long nTokens, float* dFreqFactors, void* dCache, long nbPos, long nbHead, long nPosMax, long pos0, int* dPos0, void* stream);
    // ... paged attention: a batch of nSeq independent sequences over one pool of KV pages of 128 positions (page p at p * nbPage; row (jj, hk) at
    // jj * nbPos + hk * nbHead inside it), addressed by the int32 table dPages [nSeq][ldPages] and the int32 lengths dLen [nSeq] on the device: the
    // stores put token t of sequence b at dLen[b] + t, attention uses n_kv[b] = clamp(dLen[b] + lenBias, 0, nKvMax); per sequence bit for bit the
    // contiguous entries above; a position or page id out of range writes nothing, a sequence with an invalid needed id returns +0 rows
    [DllImport(Lib)] public static extern int ggml_hip_kv_store_paged_dev(int kvType, float* dSrc, long ldxTok, long ldxHead, int nHeadKv, int d, long nSeq, long nQ,
        void* dPool, long nbPage, long nbPos, long nbHead, int nPages, int* dPages, long ldPages, int* dLen, long nKvMax, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_rope_kv_store_paged_dev(ggml_hip_rope_params_t* rp, int kvType, float* dX, long ldxTok, long ldxHead, int nHeadKv,
        int d, long nSeq, long nQ, float* dFreqFactors, void* dPool, long nbPage, long nbPos, long nbHead, int nPages, int* dPages, long ldPages, int* dLen,
        long nKvMax, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_plan(int kvType, int d, int nHead, int nHeadKv, long nSeq, long nQ, long nKvMax, void* plan);
    [DllImport(Lib)] public static extern nuint ggml_hip_attn_paged_work_size(int kvType, int d, int nHead, int nHeadKv, long nSeq, long nQ, long nKvMax);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPage, long nbPos,
        long nbHead, int nPages, int* dPages, long ldPages, int* dLen, int lenBias, long nSeq, int nHead, int nHeadKv, int d, long nQ, long nKvMax, int causal,
        float scale, void* dMask, float maxBias, float logitSoftcap, float* dSinks, float* dDst, long lddTok, long lddHead, void* dWork, nuint workBytes,
        void* stream);
    // ... the attention OPTIONS of both caches: a sliding window (row at position P sees j with P - j < window; needs causal), attention sinks (f32
    // [nHead] on the device, in the softmax denominator only) and a logit soft-cap (cap * tanh(scale / cap * s)); opts null or all off: the base
    // entries' bits; the base entries' work sizes serve; a windowed decode grid follows the window, and paged table entries below it are never read
    [StructLayout(LayoutKind.Sequential)]
    public struct ggml_hip_attn_opts_t
    {
        public float* d_sinks;
        public long window;
        public float logit_softcap;
        public int reserved;
    }
    [DllImport(Lib)] public static extern int ggml_hip_attn_ex_plan(int kvType, int d, int nHead, int nHeadKv, long nQ, long nKvMax, ggml_hip_attn_opts_t* opts, void* plan);
    [DllImport(Lib)] public static extern int ggml_hip_attn_ex_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPos, long nbHead,
        int nHead, int nHeadKv, int d, long nQ, long nKv, int* dNKv, long nKvMax, int causal, float scale, ggml_hip_attn_opts_t* opts,
        float* dDst, long lddTok, long lddHead, void* dWork, nuint workBytes, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_ex_plan(int kvType, int d, int nHead, int nHeadKv, long nSeq, long nQ, long nKvMax,
        ggml_hip_attn_opts_t* opts, void* plan);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_ex_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPage, long nbPos,
        long nbHead, int nPages, int* dPages, long ldPages, int* dLen, int lenBias, long nSeq, int nHead, int nHeadKv, int d, long nQ, long nKvMax, int causal,
        float scale, ggml_hip_attn_opts_t* opts, float* dDst, long lddTok, long lddHead, void* dWork, nuint workBytes, void* stream);
    // ... ragged paged attention: the paged entries with a query count per sequence read on the device.  q / dst / the stores' rows are packed
    // [nTokensMax][heads][d]; dQStart int32 [nSeq + 1] holds prefix sums, sequence b owns rows dQStart[b] .. dQStart[b+1] - 1 and is present when
    // 0 <= dQStart[b] <= dQStart[b+1] <= nTokensMax (else it writes nothing); n_kv[b] = clamp(dLen[b] + (addQ ? n_q[b] : 0) + lenBias, 0, nKvMax); the form
    // follows n_q[b] per sequence; per sequence bit for bit the uniform paged entries; nDecRowsMax bounds the DECODE rows of the work buffer
    [StructLayout(LayoutKind.Sequential)]
    public struct ggml_hip_attn_ragged_plan_t
    {
        public int chunk, launches;
        public long n_chunks, max_tiles, decode_workgroups, merge_workgroups, prompt_workgroups, index_bytes;
    }
    [DllImport(Lib)] public static extern int ggml_hip_ragged_positions_dev(int* dQStart, int* dLen, long nSeq, long nTokensMax, int* dPos, void* stream);
    // (the rows the LM head needs: dDst[s] = row dQStart[s+1] - 1 of dX, +0 for an empty or absent sequence)
    [DllImport(Lib)] public static extern int ggml_hip_ragged_last_rows_dev(float* dX, long ldx, int* dQStart, long nSeq, long nTokensMax, long k, float* dDst, long ldd,
        void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_kv_store_paged_ragged_dev(int kvType, float* dSrc, long ldxTok, long ldxHead, int nHeadKv, int d, long nSeq,
        int* dQStart, long nTokensMax, void* dPool, long nbPage, long nbPos, long nbHead, int nPages, int* dPages, long ldPages, int* dLen, long nKvMax, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_rope_kv_store_paged_ragged_dev(ggml_hip_rope_params_t* rp, int kvType, float* dX, long ldxTok, long ldxHead,
        int nHeadKv, int d, long nSeq, int* dQStart, long nTokensMax, float* dFreqFactors, void* dPool, long nbPage, long nbPos, long nbHead, int nPages, int* dPages,
        long ldPages, int* dLen, long nKvMax, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_ragged_plan(int kvType, int d, int nHead, int nHeadKv, long nSeq, long nTokensMax, long nDecRowsMax,
        long nKvMax, ggml_hip_attn_opts_t* opts, ggml_hip_attn_ragged_plan_t* plan);
    [DllImport(Lib)] public static extern nuint ggml_hip_attn_paged_ragged_work_size(int kvType, int d, int nHead, int nHeadKv, long nSeq, long nTokensMax,
        long nDecRowsMax, long nKvMax);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_ragged_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPage,
        long nbPos, long nbHead, int nPages, int* dPages, long ldPages, int* dLen, int addQ, int lenBias, long nSeq, int* dQStart, long nTokensMax, long nDecRowsMax,
        int nHead, int nHeadKv, int d, long nKvMax, int causal, float scale, ggml_hip_attn_opts_t* opts, float* dDst, long lddTok, long lddHead, void* dWork,
        nuint workBytes, void* stream);
    // ... attention with a MASK tensor and ALiBi slopes over the three caches: the _ex / ragged entries with a bias.  d_mask f16 [rows][ld_mask] on the
    // device (row = the query's row index in q, column = the position; -inf hides the position from the row, any other value is added to the score
    // times the head's slope; shared by all heads), ld_mask >= nKvMax and a multiple of 8, d_mask 16-byte aligned; d_slopes f32 [nHead] or null (1.0f),
    // only with a mask.  bias null or empty: the _ex / ragged entry's bits.  The same plans and work sizes serve.  ggml_hip_alibi_slopes is host only
    [StructLayout(LayoutKind.Sequential)]
    public struct ggml_hip_attn_bias_t
    {
        public void* d_mask;
        public long ld_mask;
        public float* d_slopes;
    }
    [DllImport(Lib)] public static extern int ggml_hip_alibi_slopes(int nHead, float maxBias, float* slopes);
    [DllImport(Lib)] public static extern int ggml_hip_attn_bias_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPos, long nbHead,
        int nHead, int nHeadKv, int d, long nQ, long nKv, int* dNKv, long nKvMax, int causal, float scale, ggml_hip_attn_opts_t* opts, ggml_hip_attn_bias_t* bias,
        float* dDst, long lddTok, long lddHead, void* dWork, nuint workBytes, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_bias_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPage, long nbPos,
        long nbHead, int nPages, int* dPages, long ldPages, int* dLen, int lenBias, long nSeq, int nHead, int nHeadKv, int d, long nQ, long nKvMax, int causal,
        float scale, ggml_hip_attn_opts_t* opts, ggml_hip_attn_bias_t* bias, float* dDst, long lddTok, long lddHead, void* dWork, nuint workBytes, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_attn_paged_ragged_bias_dev(int kvType, float* dQ, long ldqTok, long ldqHead, void* dK, void* dV, long nbPage,
        long nbPos, long nbHead, int nPages, int* dPages, long ldPages, int* dLen, int addQ, int lenBias, long nSeq, int* dQStart, long nTokensMax, long nDecRowsMax,
        int nHead, int nHeadKv, int d, long nKvMax, int causal, float scale, ggml_hip_attn_opts_t* opts, ggml_hip_attn_bias_t* bias, float* dDst, long lddTok,
        long lddHead, void* dWork, nuint workBytes, void* stream);
    // ... the ends of a decode step (device entries, capturable, scratch from the caller): rows of a resident weight by int32 ids on the device, bit
    // for bit download + dequantize, an id outside [0, M) a row of +0; the k best logits of every row (larger first, ties to the smaller index, NaN
    // last), p = softmax((l - l0) * invTemp) over them, top-p and the pick by the caller's uniforms dU (null: no pick) -- the int32 written to dToken
    // is the one get_rows reads on the next replay.  The chunk length, the work size and serves_for need no device
    [DllImport(Lib)] public static extern int ggml_hip_get_rows_serves_for(int type);
    [DllImport(Lib)] public static extern int ggml_hip_get_rows_dev(void* weight, int* dIds, long nIds, float* dDst, long ldd, void* stream);
    [DllImport(Lib)] public static extern long ggml_hip_topk_chunk();
    [DllImport(Lib)] public static extern nuint ggml_hip_topk_work_size(long nRows, long nVocab, int k);
    [DllImport(Lib)] public static extern int ggml_hip_argmax_rows_dev(float* dLogits, long ld, long nRows, long nVocab, int* dIds, void* dWork, nuint workBytes, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_sample_topk_dev(float* dLogits, long ld, long nRows, long nVocab, int k, float invTemp, float topP, float* dU,
        int* dIds, float* dProbs, int* dToken, void* dWork, nuint workBytes, void* stream);
    // ... the recurrent ops of a Mamba / Mamba-2 block (upstream's ggml_ssm_conv / ggml_ssm_scan) over the ragged batch (dQStart, nTokensMax) and a pool of
    // f32 state slots: sequence b uses slot dSlot[b] (an id outside [0, nSlots): +0 rows, no state written), starts from zeros where dLen[b] == 0 (the
    // slot is not read) and leaves the state after its last token in the slot.  conv: a slot is [dConv - 1][nCh], act 1 = plain f32 silu; dDst may be dX.
    // scan: a slot is [nHead][headDim][dState]; aPerState 0: A is one value per head (Mamba-2), 1: [nHead][dState] (Mamba-1, headDim 1); B / C
    // [tok][nGroup][dState].  A sequence's bits do not depend on the batch or on how its tokens are split over calls.  The sizes and the plan are host only
    [StructLayout(LayoutKind.Sequential)]
    public struct ggml_hip_ssm_plan_t
    {
        public int form, launches, slices, lanes_per_row;
        public long rows_per_workgroup, workgroups;
    }
    [DllImport(Lib)] public static extern nuint ggml_hip_ssm_conv_state_bytes(long nCh, int dConv);
    [DllImport(Lib)] public static extern nuint ggml_hip_ssm_state_bytes(int nHead, int headDim, int dState);
    [DllImport(Lib)] public static extern int ggml_hip_ssm_scan_plan(int nHead, int headDim, int dState, int nGroup, long nSeq, ggml_hip_ssm_plan_t* plan);
    [DllImport(Lib)] public static extern int ggml_hip_ssm_conv_ragged_dev(float* dX, long ldx, float* dW, float* dBias, int act, long nCh, int dConv, long nSeq,
        int* dQStart, long nTokensMax, int* dLen, int* dSlot, float* dState, long nbSlot, long nSlots, float* dDst, long ldd, void* stream);
    [DllImport(Lib)] public static extern int ggml_hip_ssm_scan_ragged_dev(float* dX, long ldxTok, long ldxHead, float* dDt, long ldDt, float* dDtBias, float* dA,
        long aLd, int aPerState, float* dB, float* dC, long ldBc, float* dD, int nHead, int headDim, int dState, int nGroup, long nSeq, int* dQStart,
        long nTokensMax, int* dLen, int* dSlot, float* dStatePool, long nbSlot, long nSlots, float* dDst, long lddTok, long lddHead, void* stream);
    // ... and the same scan with the chunked matrix form (f32 MFMA) for the sequences of more than seq_max_tokens tokens in the call; the shorter ones are
    // bit for bit ggml_hip_ssm_scan_ragged_dev's.  dWork: ggml_hip_ssm_scan_chunked_work_size bytes (0: none needed).  A long sequence keeps its bits over
    // calls only when split at multiples of `chunk`; shapes the form does not serve (aPerState 1, headDim no multiple of 16) run sequential, form 1
    [StructLayout(LayoutKind.Sequential)]
    public struct ggml_hip_ssm_chunk_plan_t
    {
        public int form, chunk, seq_max_tokens, launches, p_tile, p_tiles, kernel_state, kernel_out;
        public long chunks_max, seqs_max;
        public ulong work_bytes;
    }
    [DllImport(Lib)] public static extern nuint ggml_hip_ssm_scan_chunked_work_size(int nHead, int headDim, int dState, int nGroup, int aPerState, long nSeq, long nTokensMax);
    [DllImport(Lib)] public static extern int ggml_hip_ssm_scan_chunked_plan(int nHead, int headDim, int dState, int nGroup, int aPerState, long nSeq, long nTokensMax,
        ggml_hip_ssm_chunk_plan_t* plan);
    [DllImport(Lib)] public static extern int ggml_hip_ssm_scan_chunked_ragged_dev(float* dX, long ldxTok, long ldxHead, float* dDt, long ldDt, float* dDtBias, float* dA,
        long aLd, int aPerState, float* dB, float* dC, long ldBc, float* dD, int nHead, int headDim, int dState, int nGroup, long nSeq, int* dQStart,
        long nTokensMax, int* dLen, int* dSlot, float* dStatePool, long nbSlot, long nSlots, float* dDst, long lddTok, long lddHead, void* dWork, nuint workBytes,
        void* stream);
    // ... and the same conv with the token-parallel tiled form for the sequences of more than seq_max_tokens tokens in the call: the same bits in both
    // forms, wherever a sequence is split over calls; dDst may be dX.  dWork: ggml_hip_ssm_conv_tiled_work_size bytes (0: none needed)
    [StructLayout(LayoutKind.Sequential)]
    public struct ggml_hip_ssm_conv_plan_t
    {
        public int form, tile, seq_max_tokens, launches, vec, reserved;
        public long tiles_max, seqs_max;
        public ulong work_bytes;
    }
    [DllImport(Lib)] public static extern nuint ggml_hip_ssm_conv_tiled_work_size(long nCh, int dConv, long nSeq, long nTokensMax);
    [DllImport(Lib)] public static extern int ggml_hip_ssm_conv_tiled_plan(long nCh, int dConv, long nSeq, long nTokensMax, ggml_hip_ssm_conv_plan_t* plan);
    [DllImport(Lib)] public static extern int ggml_hip_ssm_conv_tiled_ragged_dev(float* dX, long ldx, float* dW, float* dBias, int act, long nCh, int dConv, long nSeq,
        int* dQStart, long nTokensMax, int* dLen, int* dSlot, float* dState, long nbSlot, long nSlots, float* dDst, long ldd, void* dWork, nuint workBytes,
        void* stream);

    // Seam 2: the quantize_fns_t slots (TypeDefinitions.cs:334-342), type-indexed
    [DllImport(Lib)] public static extern int ggml_hip_quantize_row(int type, float* x, void* y, int k);
    [DllImport(Lib)] public static extern int ggml_hip_dequantize_row(int type, void* x, float* y, int k);
    [DllImport(Lib)] public static extern int ggml_hip_vec_dot(int type, int n, float* s, void* vx, void* vy);
}
