// common.h -- shared declarations for the gfx950 kernels and the C-ABI layer (internal).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>

#include "../../include/ggml_hip_ext.h"

#define QK 32

// ---- reference block layouts (TypeDefinitions.cs:236-290); AoS, as they sit in a ggml_tensor ----
#pragma pack(push, 1)
struct block_q4_0 { float d; uint8_t qs[16]; };
struct block_q4_1 { float d; float m; uint8_t qs[16]; };
struct block_q4_2 { uint16_t d; uint8_t qs[8]; };               // 16 elements; d is an IEEE half (intent)
struct block_q5_0 { uint16_t d; uint8_t qh[4]; uint8_t qs[16]; };
struct block_q5_1 { uint16_t d; uint16_t m; uint8_t qh[4]; uint8_t qs[16]; };   // d, m IEEE halves (D7, intent)
struct block_q8_0 { float d; int8_t qs[32]; };
struct block_q8_1 { float d; float s0; float s1; int8_t qs[32]; };
#pragma pack(pop)
static_assert(sizeof(block_q4_0) == 20, "Ggml.cs:76");
static_assert(sizeof(block_q4_1) == 24, "Ggml.cs:77");
static_assert(sizeof(block_q4_2) == 10, "Ggml.cs:78");
static_assert(sizeof(block_q5_0) == 22, "Ggml.cs:80");
static_assert(sizeof(block_q5_1) == 24, "Ggml.cs:81");
static_assert(sizeof(block_q8_0) == 36, "Ggml.cs:82");
static_assert(sizeof(block_q8_1) == 44, "Ggml.cs:83");
static_assert(sizeof(ggml_tensor) == 176, "TypeDefinitions.cs:65-99");
static_assert(offsetof(ggml_tensor, op) == 72 && offsetof(ggml_tensor, grad) == 80 &&
              offsetof(ggml_tensor, n_tasks) == 136 && offsetof(ggml_tensor, data) == 160, "layout");

// Rows of the weight planes are padded to a multiple of ROW_PAD (the widest weight tile of any kernel), rows of the
// activation planes to ACT_PAD (the widest activation tile).
#define ROW_PAD 256
#define ACT_PAD 256
// k-blocks: every plane (weights and activation scratch) is allocated for K_STAGE_PAD-aligned k-blocks, zero-filled
// past the real end (zero scale => the pad blocks add +0), plus K_LOOKAHEAD spare blocks on the weight side for the
// register prefetch of gemm_q16.hip.  Kernels that loop over the real nbk are unaffected.
#define K_STAGE_PAD 4
#define K_LOOKAHEAD 2
__host__ __device__ static inline int64_t pad_kblocks(int64_t nbk) { return (nbk + K_STAGE_PAD - 1) / K_STAGE_PAD * K_STAGE_PAD; }
static inline int64_t pad_rows(int64_t n) { return (n + ROW_PAD - 1) / ROW_PAD * ROW_PAD; }
static inline int64_t pad_act(int64_t n) { return (n + ACT_PAD - 1) / ACT_PAD * ACT_PAD; }

// ---- resident weight: planar (block-major) layout, see DESIGN.md "Data layout in HBM" ----
//   Q4_0/Q4_1/Q5_0/Q5_1: qs [nbk][Mpad][16] bytes of nibbles exactly as in the reference block
//   Q4_2          : the same plane; k-block b = the reference's 16-element blocks 2b (bytes 0..7) and 2b+1 (bytes 8..15),
//                   which is byte for byte the nibble order of a Q4_0 block (Ggml.cs:1217-1238 vs 1136-1150)
//   Q8_0          : qs [nbk][2][Mpad][16] int8, plane 0 = even elements, plane 1 = odd elements of the block
//   d   [nbk][Mpad] f32 (Q5_0 / Q5_1 / Q4_2: the half scale widened, exact; Q4_2: of its first 16-element block)
//   m   [nbk][Mpad] f32 (Q4_1, Q5_1: the min; Q4_2: the scale of its second 16-element block)
//   qh  [nbk][Mpad] u32 (Q5_0, Q5_1)
//   F32/F16: dense [Mpad][K] row-major copy
struct ggml_hip_weight {
    int      type;
    int64_t  M, K, Mpad, nbk;
    uint8_t *qs;
    uint32_t *qh;
    float   *d;
    float   *m;
    uint8_t *q6a;     // bf6 (e3m2) digit codes, [nbk][NF][Mpad][16 B] = the first 16 bytes of each 24-byte MFMA fragment
    uint8_t *q6b;     //   (element e at bits [6e, 6e+5]) and [nbk][NF][Mpad][8 B] = the last 8; NF = 1 (Q4_0, Q4_1: nib - 8)
                      //   or 2 (Q5_0, Q8_0: w = 16 * wh + wl, fragment 0 = wl, fragment 1 = wh) -- gemm_qmx.hip
    uint8_t *i8p;     // Q5_0 / Q5_1 / Q4_1 (the latter two unsigned, no - 16; r4: Q4_2 too, nib - 8): int8 operand planes of the int8 matrix cores, [nbk][2][Mpad][16 B] like Q8_0's qs -- plane h byte j =
                      //   element 2j + h, value (nib | bit << 4) - 16 (Ggml.cs:1285-1289); built once at upload (layout.hip), 1 B / weight
                      //   beside the 0.69 B / weight of the format, for prompt-sized batches (gemm_qmp.hip)
    void    *dense;
    uint8_t *p16;     // F16 only: k-panel-major copy [Kpad/8 + spare][Mpad][16 B] for dense16.hip
    uint8_t *p32;     // F32 only: the rows split exactly into three bf16 pieces, [Kpad/8 * 3 + spare][Mpad][16 B] (dense16.hip K10d): 6 B / weight
    uint32_t *gs;     // mat-vec side image (gemv.hip): the per-block words a 16-row tile needs beside its nibbles, tile-major
                      //   [Mpad/16][nbk][NP][16 rows] 4-byte words, planes in the order d, m, qh (NP = 1..3 by type).  A copy of
                      //   d / m / qh: in their [k-block][row] planes a tile's share of a k-block is one 64-byte piece per plane
                      //   (a fifth of the bytes cost a third of the mat-vec's time, tools/stream_floor.hip)
    uint8_t *mp3;     // Q5_1 / Q4_1 (and the Q5_K extension living in the Q5_1 form): the min plane split EXACTLY into three bf16 pieces,
                      //   [ceil(nbk / 8) * 3 (+ pad to whole pairs of k-groups)][Mpad][16 B]: plane 3 * (b / 8) + piece holds 8 consecutive k-blocks of a row --
                      //   the B operand of v_mfma_f32_32x32x16_bf16 for K3p's min-term product (gemm_qmp.hip); 0.19 B / weight
    uint8_t *khdr;    // types with a wtype::hdr_slot only: the header bytes of every super-block that the planes do not hold, for the byte-exact download (and
                      //   Q2_K's min pass), [K/256][Mpad][hdr_slot B]
    int      ext_type; // 0, or the id of a WT_ORIGIN_EXT row of the type table (wtypes.cpp): the weight was uploaded as that type's super-blocks and lives in the
                       //   planar form of the row's resident type (`type`); the plan sees it
    int      up_type;  // 0, or the id of a WT_ORIGIN_UP row (IQ4_NL): uploaded as that type and resident as a PLAIN weight of `type` (Q8_0, ext_type == 0; iq4.hip) --
                       //   read by the download, ggml_hip_weight_type and the size queries alone, never by the plan or a kernel
    size_t   bytes;
    int      device;
    uint64_t uid;     // never reused: identifies the weight in cached launch graphs
};

// ---- activation scratch ("wdata"), planar like the weights; K1 writes one of two images into the `a8` region ----
//   int8 image (mat-vec kernel):  [nbk][2][Npad][16] int8, plane 0 = even elements of the block, plane 1 = odd
//   f16 images (gemm_q16.hip)  :  [nbk][4][Npad][16 B] f16, panel p = 2*kk + h, k-slot orders in gemm_q16.hip
//   bf6 image  (gemm_qmx.hip)  :  per k-block [2][Npad][16 B] then [2][Npad][8 B]: half 0 = digits ah, half 1 = digits al
//                                 of a = 16*ah + al, 32 bf6 codes per 24-byte fragment
//   ad [nbk][Npad] f32 block scales, as [nbk][Npad] i32 block sums of the quants (MFMA images: the float d * sum)
//   sp3 (int8 image + ACT_IMAGE_MIN_PIECES only): d * sum split exactly into three bf16 pieces, [ceil(nbk / 8) * 3][Npad][16 B] like
//       ggml_hip_weight::mp3 -- in the upper half of the a8 region, which the int8 image leaves unused
struct act_planes {
    int8_t  *a8;
    float   *ad;
    int32_t *as;
    int64_t  Npad;
    uint8_t *sp3;
};
#define ACT_IMAGE_MIN_PIECES 64      /* flag on image kind 0: K1 also writes sp3 (K3p-int8 with a min-term weight type; needs K / 32 >= 8) */
static inline size_t act_bytes(int64_t K, int64_t Npad) {
    const int64_t nbk = pad_kblocks(K / QK);
    return (size_t)nbk * 4 * Npad * 16 + (size_t)nbk * Npad * 4 * 2;
}
static inline act_planes act_carve(void *base, int64_t K, int64_t Npad) {
    const int64_t nbk = pad_kblocks(K / QK);
    act_planes p;
    p.a8 = (int8_t *)base;
    p.ad = (float *)((uint8_t *)base + (size_t)nbk * 4 * Npad * 16);
    p.as = (int32_t *)((uint8_t *)p.ad + (size_t)nbk * Npad * 4);
    p.Npad = Npad;
    p.sp3 = (uint8_t *)base + (size_t)nbk * 2 * Npad * 16;   // ((nbk / 8 rounded up) * 3 planes <= 2 nbk planes from two k-blocks on)
    return p;
}

// ---- cross-lane moves inside a group of 8 lanes as DPP modifiers (no LDS round trip, unlike __shfl_xor = ds_bpermute) ----
#ifdef __HIPCC__
template <int CTRL>
__device__ __forceinline__ int dpp_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }
// K3s (gemm_qmx.hip / gemm_q8s.hip): workgroup -> (row tile, column tile), XCD-aware (speed only; a bijection whatever ntw and ncol are).
// Workgroups b and b + 8 share an XCD and its L2: the ncol column tiles of one row tile sit 8 apart in launch order, so the weight tile they
// all stream reaches that L2 once (with "row tile fastest" they were ntw launches apart and each fetched it again: what made the forms pay
// by M above 32 src1 rows).  Row tiles in whole groups of eight; the last ntw % 8 keep the plain order.
__device__ __forceinline__ void k3s_tile_of(int wg, int ntw, int ncol, int &rt, int &ct) {
    const int full = ntw & ~7;
    const int g = wg / (8 * ncol);
    if (g * 8 < full) { const int idx = wg - g * 8 * ncol; rt = g * 8 + (idx & 7); ct = idx >> 3; }
    else { const int w2 = wg - full * ncol, nt = ntw - full; rt = full + w2 % nt; ct = w2 / nt; }
}

template <int CTRL>
__device__ __forceinline__ float dpp_f(float v) { return __builtin_bit_cast(float, dpp_i<CTRL>(__builtin_bit_cast(int, v))); }
#define DPP_XOR1 0xB1        /* quad_perm:[1,0,3,2] */
#define DPP_XOR2 0x4E        /* quad_perm:[2,3,0,1] */
#define DPP_HALF_MIRROR 0x141 /* lane i <-> 7 - i inside each group of 8: joins the two quads once they are uniform */
#define DPP_NEXT 0x101       /* row_shl:1: lane i reads lane i + 1 (inside a row of 16) */
// max / sum over the 8 lanes t = lane & 7 of a group, result in every lane
__device__ __forceinline__ float group8_max(float v) {
    v = fmaxf(v, dpp_f<DPP_XOR1>(v));
    v = fmaxf(v, dpp_f<DPP_XOR2>(v));
    return fmaxf(v, dpp_f<DPP_HALF_MIRROR>(v));
}
__device__ __forceinline__ int group8_sum(int v) {
    v += dpp_i<DPP_XOR1>(v);
    v += dpp_i<DPP_XOR2>(v);
    return v + dpp_i<DPP_HALF_MIRROR>(v);
}
// ---- an f32 value as three bf16 pieces that sum to it exactly (truncation: 8 + 8 + 8 significand bits); dense16.hip K10d, gemm_qmp.hip ----
__device__ __forceinline__ void split3(float a, uint32_t &p0, uint32_t &p1, uint32_t &p2) {
    const uint32_t u = __float_as_uint(a);
    const uint32_t b0 = u & 0xFFFF0000u;
    const float r1 = a - __uint_as_float(b0);                       // exact
    const uint32_t b1 = __float_as_uint(r1) & 0xFFFF0000u;
    const float r2 = r1 - __uint_as_float(b1);                      // exact, at most 8 significant bits
    p0 = b0 >> 16; p1 = b1 >> 16; p2 = __float_as_uint(r2) >> 16;
    // r4: an infinity or a NaN.  As written above, inf - inf put a NaN into the remainder pieces and every output that touched an
    // infinite operand came out NaN where the reference's f32 product gives +-inf.  The value goes into the THIRD piece alone: of the six
    // kept piece products only a2 * b0 (b0 * a2) then sees it -- against the other operand's LEADING piece, which is zero only if that operand
    // is (inf * 0 is NaN in the reference too) -- while in the first piece it would meet remainder pieces that are zero for one operand in
    // 256 (inf * 0).  A NaN whose payload sits in the low 16 bits keeps a set quiet bit, so truncation cannot turn it into an infinity.
    // (Two infinities at the same k meet in no kept product: that one case gives NaN where the reference gives inf.)
    if ((u & 0x7F800000u) == 0x7F800000u) { p0 = 0; p1 = 0; p2 = (u >> 16) | ((u & 0x007FFFFFu) ? 0x0040u : 0u); }
}
#endif

// ---- once per kernel AND device: hipFuncAttributeMaxDynamicSharedMemorySize is a per-device property of a kernel, and one
// process may drive several devices (ggml_hip_init_devices).  One object per kernel instantiation (function-local static).
#ifdef __cplusplus
#include <atomic>
struct PerDeviceOnce {
    std::atomic<uint64_t> done{0};
    hipError_t max_dynamic_lds(const void *kern, int bytes) {
        int dev = 0;
        hipError_t e = hipGetDevice(&dev);
        if (e != hipSuccess) return e;
        const uint64_t bit = 1ull << (dev & 63);
        if (done.load(std::memory_order_acquire) & bit) return hipSuccess;
        e = hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, bytes);
        if (e == hipSuccess) done.fetch_or(bit, std::memory_order_release);
        return e;
    }
};
#endif
#ifdef __HIPCC__
// Launch KERN with `lds` bytes of dynamic LDS after raising its attribute to `attr_lds` (once per instantiation and device); returns
// the launch's error.  Grids, block sizes and LDS bytes are the caller's.  kfn<kernel<...>> names the instantiation.
template <auto KERN> struct kfn_t {};
template <auto KERN> constexpr kfn_t<KERN> kfn{};
template <auto KERN, typename... A>
hipError_t launch_lds(kfn_t<KERN>, dim3 grid, dim3 block, size_t lds, int attr_lds, hipStream_t st, A... args) {
    static PerDeviceOnce once;
    const hipError_t attr = once.max_dynamic_lds((const void *)KERN, attr_lds);
    if (attr != hipSuccess) return attr;
    KERN<<<grid, block, lds, st>>>(args...);
    return hipGetLastError();
}
#endif

// ---- epilogue applied to the accumulators of a mat-mul kernel as they are stored (the add / scale node
// that follows a mul_mat node, fused into its store phase).  mode 0: none.  mode 1 (add, Ggml.cs:4622-4682): dst keeps the
// product, dst2[n][m] = product + addend[n][m] -- both nodes' data are materialised, one f32 add, bit for bit the separate
// kernel.  mode 2 (scale, Ggml.cs:6746-6778, in place: the scale node is a view of the product): dst[n][m] = product * scale.
// mode 3 (r4, the exchange of a row split fused into the store phase -- SURVEY 8(e): "epilogue peer-writes straight into each peer's final
// [N][M] buffer"): dst is this rank's own [N][M] buffer at its column offset, push[0 .. npush) are the SAME position in every peer's buffer
// (IPC-mapped, or other slots' buffers of one process); every element is stored to all of them with dst's row stride (Ggml.cs:6692-6697
// is the layout every rank must end with).  Kernels that apply it: the staged MX forms, K3p (MX and int8).
#define MM_PUSH_MAX 7
struct mm_epilogue {
    int mode;
    const float *addend; int64_t ld_add;
    float *dst2; int64_t ld2;
    float scale;
    int npush;
    float *push[MM_PUSH_MAX];
};
// launchers take `const mm_epilogue *`, nullptr meaning none; the kernels take the epilogue by value
static inline mm_epilogue epilogue_or_none(const mm_epilogue *ep) { return ep ? *ep : mm_epilogue{0, nullptr, 0, nullptr, 0, 1.0f}; }

// ---- prologue of the fused mat-vec (prologue side): the activation row the kernel quantizes is not read
// but COMPUTED, y = (x * rms_scale(x)) * g -- the rms_norm -> mul pair in front of a mul_mat (Ggml.cs:5858-5920, 5007-5035) --
// with the reference's own operation sequence (f32 squares summed in f64 in the unfused kernel's order, one f32 multiply per
// node); workgroup 0 also writes both nodes' results (n_out = the norm, y_out = the product), [N][K] contiguous.
struct mm_prologue {
    const float *g; int64_t ld_g;
    float *n_out; float *y_out;
};

#ifdef __HIPCC__
// rms_norm's row scale 1 / sqrt(mean(x^2) + 1e-6) (Ggml.cs:5889-5915: f32 squares summed in f64), computed by ONE wave.  The
// reference adds the squares one after the other; any order of the f64 additions is within ~1e-16 of that, and ONE order is
// shared by every kernel that needs the scale (eltwise.hip, fused.hip, the mat-vec's prologue), so they agree bit for bit:
//   lane L holds four partial sums, partial q taking elements L + 64 (4 j + q), j = 0, 1, ... in order; lane total =
//   (p0 + p1) + (p2 + p3); lanes are joined inside rows of 16 by DPP (xor 1, xor 2, half mirror, row mirror -- after two
//   xor steps a quad is uniform, so a mirror is a swap of uniform groups), then rows by xor 16 and xor 32.
// Written for latency: a decode-sized norm is one wave working alone -- the loads of 32 iterations are in flight together (a
// plain loop cost one L2 round trip per iteration: 64 x ~100 ns at K = 4096), the f64 chain is 16 deep instead of 64, and
// only the last two lane steps go through ds_bpermute.
template <int CTRL>
__device__ __forceinline__ double dpp_d(double v) {
    const uint64_t u = __builtin_bit_cast(uint64_t, v);
    const uint32_t lo = (uint32_t)dpp_i<CTRL>((int)(uint32_t)u), hi = (uint32_t)dpp_i<CTRL>((int)(uint32_t)(u >> 32));
    return __builtin_bit_cast(double, (uint64_t)lo | ((uint64_t)hi << 32));
}
#define DPP_ROW_MIRROR 0x140  /* lane i <-> 15 - i inside each row of 16 */
__device__ __forceinline__ float rms_row_scale(const float *__restrict__ xr, int64_t nc, int lane) {
    constexpr int UN = 32;
    double p[4] = {0.0, 0.0, 0.0, 0.0};
    for (int64_t i0 = 0; i0 < nc; i0 += 64 * UN) {
        float v[UN];
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t i = i0 + lane + 64 * u;
            v[u] = i < nc ? xr[i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < UN; ++u) {
            const int64_t i = i0 + lane + 64 * u;
            if (i < nc) {
                const float sq = v[u] * v[u];           // float product, then widened (Ggml.cs:5903)
                p[u & 3] += (double)sq;
            }
        }
    }
    double sum = (p[0] + p[1]) + (p[2] + p[3]);
    sum += dpp_d<DPP_XOR1>(sum);
    sum += dpp_d<DPP_XOR2>(sum);
    sum += dpp_d<DPP_HALF_MIRROR>(sum);
    sum += dpp_d<DPP_ROW_MIRROR>(sum);
    sum += __shfl_xor(sum, 16);
    sum += __shfl_xor(sum, 32);
    const float mean = (float)(sum / (double)nc);       // Ggml.cs:5906
    return 1.0f / sqrtf(mean + 1e-6f);                  // Ggml.cs:5889, 5915
}
#endif

// ---- kernel launchers (implemented in the .hip files) ----
// layout.hip
hipError_t launch_repack_to_planar(int type, const uint8_t *aos, uint64_t nb01, int64_t row_begin, int64_t rows,
                                   ggml_hip_weight *w, hipStream_t st);
hipError_t launch_planar_to_aos(const ggml_hip_weight *w, uint8_t *aos, hipStream_t st);
hipError_t launch_nibbles_to_bf6(ggml_hip_weight *w, hipStream_t st);
hipError_t launch_q5_to_i8(ggml_hip_weight *w, hipStream_t st);     // Q5_0 / Q5_1 / Q4_1 nibble (+ fifth-bit) planes -> w->i8p
hipError_t launch_min_pieces(ggml_hip_weight *w, hipStream_t st);   // Q5_1 / Q4_1 min plane -> w->mp3 (three bf16 pieces, K3p's min-term product)
// up to 32 device buffers -> device-visible (mapped host) destinations in one launch; sizes and addresses multiples of 4
hipError_t launch_scatter_copy(const void *const *src, void *const *dst, const size_t *bytes, int n, hipStream_t st);
hipError_t launch_gemv_side_image(ggml_hip_weight *w, hipStream_t st);   // d / m / qh planes -> w->gs (after every write of the planes)
static inline int gemv_side_planes(int type) {
    return 1 + ((type == GGML_TYPE_Q4_1 || type == GGML_TYPE_Q5_1 || type == GGML_TYPE_Q4_2) ? 1 : 0) + ((type == GGML_TYPE_Q5_0 || type == GGML_TYPE_Q5_1) ? 1 : 0);
}
hipError_t launch_relayout_gathered(const float *g, int G, int64_t N, int64_t Ms, float *dst, int64_t M, int64_t ldd,
                                    hipStream_t st);
hipError_t launch_push_columns(const float *src, int64_t lds, int64_t N, int64_t Ms, float *const *peers, int G, int64_t ldd,
                               int64_t col0, hipStream_t st);
// quantize.hip
hipError_t launch_quantize_act(const float *x, int64_t N, int64_t K, int64_t ld1, act_planes p, int image, hipStream_t st, bool q8k = false);
// the bf6 image (kind 3) by the lane-per-block kernel: does it serve this src1, and its first nb_head k-blocks alone (+ nclr words zeroed)
bool quantize_act_bf6_serves(const float *x, int64_t N, int64_t K, int64_t ld1);
hipError_t launch_quantize_act_bf6_head(const float *x, int64_t N, int64_t K, int64_t ld1, act_planes p, int64_t nb_head, uint32_t *clr, int nclr,
                                        hipStream_t st);
// ---- the weight types: ONE row per type id the library accepts anywhere -- the reference's thirteen and the extension ids of
// include/ggml_hip_ext.h.  wtypes.cpp holds the table; everything that used to ask "is this a k-quant / IQ4_NL / BF16" reads a row.
// DESIGN.md "Adding a weight type" says what a new type has to supply.
typedef hipError_t (*wt_to_planar_fn)(int type, const uint8_t *aos, uint64_t nb01, int64_t row_begin, int64_t rows, ggml_hip_weight *w, hipStream_t st);
typedef hipError_t (*wt_from_planar_fn)(const ggml_hip_weight *w, uint8_t *aos, hipStream_t st);
typedef hipError_t (*wt_quantize_fn)(int type, const float *x, int64_t nrows, int64_t k, void *blocks, hipStream_t st);
typedef hipError_t (*wt_dequantize_fn)(int type, const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st);
enum { WT_ORIGIN_NONE, WT_ORIGIN_EXT, WT_ORIGIN_UP };
struct wtype {
    int    id;
    int    blck;       // the file format: elements ...
    size_t bytes;      //   ... and bytes of a block
    int    resident;   // the type whose planar form and kernels a weight of this type lives in (ggml_hip_weight::type); itself for native types
    int    origin;     // how the weight remembers `id`: not at all (type == id), in ext_type (the plan sees it), in up_type (the plan does not)
    bool   q8k;        // INIT quantizes the activations by the Q8_K rule (one scale per 256)
    bool   min_pass;   // the product runs on the block term alone; kquants.hip's min pass subtracts the min term behind it (plan flag MM_FLAG_MIN_PASS)
    int    hdr_slot;   // bytes per super-block in the weight's khdr plane (the header bytes a byte-exact download needs back); 0: no such plane
    bool   own_i8;     // the two-scale form: to_planar writes the int8 planes itself (launch_q5_to_i8 is skipped, the nibble plane is a stub)
    int    x_align;    // quantize: the alignment its source rows need (float4 loads), 0: none
    wt_to_planar_fn   to_planar;     // file-format rows (device memory, nb01 apart, from row_begin on) -> the resident planes; null: not a weight type
    wt_from_planar_fn from_planar;   // the exact inverse, rows packed
    wt_quantize_fn    quantize;      // contiguous f32 rows -> blocks; null: no quantizer
    wt_dequantize_fn  dequantize;    // blocks -> f32 rows; null: no dequantizer
};
const wtype *wtype_of(int id);                     // nullptr: not a type id
static inline int wtype_ext(const wtype *r) { return r->origin == WT_ORIGIN_EXT ? r->id : 0; }      // the ext_type a weight of the row carries
static inline bool kquant_min_pass(int ext_type) { const wtype *r = wtype_of(ext_type); return r && r->min_pass; }
// kquants.hip: Q5_K / Q4_K on the planar Q5_1 form, Q6_K / Q3_K / Q2_K in the two-scale int8 form (two_scale.h); unpinned extras -- the
// published upstream formats, no oracle in the reference.  x: contiguous rows, 16-byte aligned
hipError_t launch_kq_to_planar(int type, const uint8_t *aos, uint64_t nb01, int64_t row_begin, int64_t rows, ggml_hip_weight *w, hipStream_t st);
hipError_t launch_planar_to_kq(const ggml_hip_weight *w, uint8_t *aos, hipStream_t st);
hipError_t launch_dequantize_kq(int type, const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st);
hipError_t launch_quantize_kq(int type, const float *x, int64_t nrows, int64_t k, void *blocks, hipStream_t st);
// dst[n][i] -= the min term of a Q2_K weight against K1's int8 image by the Q8_K rule (columns i < M, rows n < N; kquants.hip);
// form 0: the launcher's choice, 1 / 2: one / two 32-column tiles per wave (the same bits; a test hook selects them)
hipError_t launch_q2k_min_pass(const ggml_hip_weight *w, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st, int form = 0);
// iq4.hip: IQ4_NL in Q8_0's planar form (its qs / d planes), IQ4_XS in the two-scale int8 form
hipError_t launch_iq4_to_planar(int type, const uint8_t *aos, uint64_t nb01, int64_t row_begin, int64_t rows, ggml_hip_weight *w, hipStream_t st);
hipError_t launch_planar_to_iq4(const ggml_hip_weight *w, uint8_t *aos, hipStream_t st);
hipError_t launch_dequantize_iq4(int type, const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st);
hipError_t launch_quantize_iq4(int type, const float *x, int64_t nrows, int64_t k, void *blocks, hipStream_t st);
hipError_t launch_q8_aos_to_planes(int q8type, const void *blocks, int64_t N, int64_t K, act_planes p, hipStream_t st);
hipError_t launch_quantize_rows(int type, int src_type, const void *x, int64_t ld, int64_t nrows, int64_t k, void *blocks,
                                hipStream_t st);
hipError_t launch_add_q_f32(int type, const void *blocks_in, const float *x, int64_t nrows, int64_t k, void *blocks_out,
                            hipStream_t st);
hipError_t launch_dequantize_rows(int type, const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st);
// dense16.hip: K padded to whole stages of 128, plus spare (zero) panels for the register look-ahead
#define DENSE16_SPARE_PANELS 8
static inline int64_t dense16_kpad(int64_t K) { return (K + 127) / 128 * 128; }
struct mm_plan;                      // plan.h: the one decision per product every launcher below consumes
hipError_t launch_f16_rows_to_panels(ggml_hip_weight *w, hipStream_t st);
hipError_t launch_dense16_init(const float *x, int64_t N, int64_t K, int64_t ld1, void *work, hipStream_t st);
hipError_t launch_dense16(const ggml_hip_weight *w, const mm_plan &pl, const void *work, int64_t N, float *dst, int64_t ldd, hipStream_t st);
// K10d (dense16.hip): F32 x F32 on the bf16 matrix cores, operands split into three bf16 pieces
#define DENSE32_SPARE_PANELS 24          // (one stage of look-ahead past the padded end: zero)
hipError_t launch_f32_rows_to_split_panels(ggml_hip_weight *w, hipStream_t st);
hipError_t launch_dense32_init(const float *x, int64_t N, int64_t K, int64_t ld1, void *work, hipStream_t st);
hipError_t launch_dense32(const ggml_hip_weight *w, const void *work, int64_t N, float *dst, int64_t ldd, hipStream_t st);
// BF16 weights (GGML_HIP_TYPE_BF16, an extension type: w->type holds 130 itself, so no F16 branch can take it): the F16 resident form with
// bf16 bits (row-major copy + k-panels, launch_f16_rows_to_panels moves 16-bit words whatever they mean) and bf16 twins of the F16 kernels
static inline bool is_bf16(int t) { return t == GGML_HIP_TYPE_BF16; }
static inline bool is_dense16(int t) { return t == GGML_TYPE_F16 || is_bf16(t); }   // 2-byte dense weights: F16 or BF16
// f32 -> bf16, THE rule of every conversion (include/ggml_hip_ext.h GGML_HIP_TYPE_BF16): a NaN stays a quiet NaN with its sign and high
// payload (the bare integer form would turn a NaN whose payload sits in the low bits into an infinity or carry it into the exponent: the
// separate select); anything else rounds to nearest even, subnormals kept, overflow to +-inf.  The select is written as a mask: as a
// conditional hipcc branched on it per element, and each branch drained the loads in flight (the BF16 mat-vec ran at a fifth of F16's rate)
__host__ __device__ static inline uint32_t f32_to_bf16_bits(uint32_t u) {
    const uint32_t nan = 0u - (uint32_t)((u & 0x7FFFFFFFu) > 0x7F800000u);      // all ones for a NaN
    return (((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16) & ~nan) | (((u >> 16) | 0x0040u) & nan);
}
hipError_t launch_dense16_init_bf16(const float *x, int64_t N, int64_t K, int64_t ld1, void *work, hipStream_t st);
hipError_t launch_f32_to_bf16_rows(const float *x, int64_t n, uint16_t *y, hipStream_t st);      // n contiguous elements
hipError_t launch_bf16_to_f32_rows(const uint16_t *x, int64_t n, float *y, hipStream_t st);
// eltwise.hip (op: 0 add, 1 mul; contiguous f32)
hipError_t launch_binary_f32(int op, const float *x, const float *y, float *z, int64_t n, hipStream_t st);
hipError_t launch_scale_f32(float *z, int64_t n, float v, hipStream_t st);
hipError_t launch_rms_norm_f32(const float *x, float *y, int64_t nr, int64_t nc, hipStream_t st);
hipError_t launch_silu_f32(const float *x, float *y, int64_t n, hipStream_t st);
// fused.hip: two nodes, one launch (both outputs written)
hipError_t launch_rms_norm_mul_f32(const float *x, const float *g, float *n_out, float *y_out, int64_t nr, int64_t nc, hipStream_t st);
hipError_t launch_silu_mul_f32(const float *a, const float *b, float *s_out, float *y_out, int64_t n, hipStream_t st);   // (s_out may be null: only y_out is written)
// gemv.hip / gemm_q.hip / dense.hip
hipError_t launch_gemv_q(const ggml_hip_weight *w, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st);
// Up to four weight matrices of one type and K behind ONE activation matrix (the q / k / v or the gate / up projections of a
// transformer block): the fused mat-vec walks the row tiles of all of them in one launch.  Row tiles [tile_end[i-1], tile_end[i])
// belong to matrix i; every row's arithmetic is what the single-matrix call does.
struct mv_set {
    int n;
    int tile_end[4];
    const uint8_t *qs[4];
    const uint32_t *gs[4];
    float *dst[4];
    int64_t M[4], Mpad[4], ldd[4];
};
hipError_t launch_gemv_q_fused_multi(const ggml_hip_weight *const *w, int n_w, const float *x, int64_t ld1, const mm_prologue *pro, int64_t N,
                                     float *const *dst, const int64_t *ldd, hipStream_t st);
hipError_t launch_gemv_q_fused(const ggml_hip_weight *w, const float *x, int64_t ld1, int64_t N, float *dst, int64_t ldd,
                               hipStream_t st, const mm_epilogue *ep = nullptr);
bool gemv_fused_has_epilogue(int64_t N);       // the kernel form that serves N applies an mm_epilogue itself
// the same launch with the rms_norm -> mul prologue (N <= 4 only: gemv_fused_has_epilogue)
hipError_t launch_gemv_q_fused_pro(const ggml_hip_weight *w, const float *x, int64_t ld1, const mm_prologue &pro, int64_t N, float *dst,
                                   int64_t ldd, hipStream_t st, const mm_epilogue *ep = nullptr);
// The by-id mat-vec of ggml_hip_mul_mat_id_dev (route 1): pair p = t * n_used + s runs the fused mat-vec at N = 1 on src1 row
// x + t * ld1_token + s * ld1_slot against expert ids[p], whose operand plane and side image come from the set's device table `tab` --
// the single-matrix call's bits.  An id outside [0, n_expert) writes the pair's M outputs as +0.0f without reading the table.
// w0: any member of the set (type, ext_type, M, Mpad, nbk: the same for all).  hipErrorNotSupported where the fused mat-vec has no form.
struct moe_expert { const uint8_t *qs; const uint32_t *gs; };
hipError_t launch_gemv_q_fused_byid(const ggml_hip_weight *w0, const moe_expert *tab, int n_expert, const int32_t *ids, int64_t npairs, int n_used,
                                    const float *x, int64_t ld1_token, int64_t ld1_slot, float *dst, int64_t ldd, hipStream_t st);
// moe.hip: the batch route's gather / scatter, a slice of the row map by value per launch
#define MOE_MAP_CHUNK 896
struct moe_map { int32_t v[MOE_MAP_CHUNK]; };
hipError_t launch_moe_gather(const moe_map &map, int n, int64_t j0, int n_used, const float *x, int64_t ld1_token, int64_t ld1_slot,
                             int64_t K, float *g, int64_t ldg, hipStream_t st);
hipError_t launch_moe_scatter(const moe_map &map, int n, int64_t p0, const float *r, int64_t ldr, int64_t M, float *dst, int64_t ldd,
                              hipStream_t st);
// ---- the grouped, device-routed product of ggml_hip_mul_mat_id_grouped_dev (moe.cpp; plan.h plan_mul_mat_id_grouped has the bounds) ----
// an expert's operand planes and block scales as the K3s bodies take them: Q8_0 a = qs, Q5_0 a = i8p (b unused), Q4_0 a = q6a, b = q6b
struct moe_gexpert { const uint8_t *a; const uint8_t *b; const float *d; const void *spare; };
// column tile t of the sorted rows: its expert, its first sorted row (32 t: every segment is padded to whole tiles) and how many of its 32 rows are pairs
struct moe_tile { int32_t expert, first, rows, spare; };
// the routing tables, all in the caller's work buffer: count / first [n_expert] (pairs of an expert, first sorted row of its segment),
// n_tiles [1], pos [P] (sorted row of pair p, -1: id outside the set), order [rows] (pair of sorted row j, -1: padding), tiles [max_tiles]
struct moe_route { int32_t *count, *first, *n_tiles, *pos, *order; moe_tile *tiles; };
// moe.hip: ids [P] -> the tables (three launches; stable: ascending p inside an expert; integer work only); rows = 32 * max_tiles
hipError_t launch_moe_route(const int32_t *ids, int64_t P, int n_expert, const moe_route &r, int64_t max_tiles, hipStream_t st);
// sorted row j < rows <- the src1 row of pair order[j], zeros where order[j] < 0 (x 16-byte aligned, strides and ldg multiples of 4)
hipError_t launch_moe_gather_dev(const int32_t *order, int64_t rows, int n_used, const float *x, int64_t ld1_token, int64_t ld1_slot, int64_t K, float *g,
                                 int64_t ldg, hipStream_t st);
// pair p < P <- sorted row pos[p] of r, +0.0f where pos[p] < 0
hipError_t launch_moe_scatter_dev(const int32_t *pos, int64_t P, const float *r, int64_t ldr, int64_t M, float *dst, int64_t ldd, hipStream_t st);
// moe_route.hip: the router and the combine of a mixture-of-experts block (ggml_hip_moe_route_dev / ggml_hip_moe_combine_dev, moe.cpp)
// logits [n_tokens] rows of n_expert (ld apart) -> ids / weights [n_tokens * n_used]: one wave per token, exact selection, no LDS
hipError_t launch_moe_topk(const float *logits, int64_t ld, int64_t n_tokens, int n_expert, int n_used, int gating, int normalize, float scale,
                           int32_t *ids, float *weights, hipStream_t st);
// dst[t] = sum over s (ascending) of w[t * n_used + s] * y[(t * n_used + s) * ldy ..] [+ addend[t]]: 16-byte accesses where every pointer and stride allows
hipError_t launch_moe_combine(const float *y, int64_t ldy, const float *w, int64_t n_tokens, int n_used, int64_t M, const float *addend, int64_t ld_add,
                              float *dst, int64_t ldd, hipStream_t st);
// attn.hip: rows into a KV cache, attention over it (ggml_hip_kv_store_dev / ggml_hip_attn_dev, attn.cpp; the form is plan.h's plan_attn)
struct attn_plan;
struct attn_args {
    int kv_type, D, n_head, n_head_kv, causal;
    const float *q; int64_t ldq_tok, ldq_head;
    const void *k, *v; int64_t nb_pos, nb_head;
    int64_t n_q, n_kv; const int32_t *d_n_kv; int64_t n_kv_max;
    float scale;
    float *dst; int64_t ldd_tok, ldd_head;
    void *work;                                                      // 16-byte aligned (DECODE: plan_attn's work_bytes)
};
hipError_t launch_kv_store(int kv_type, const float *src, int64_t ld, int64_t n_rows, int64_t row_elems, void *cache, int64_t nb_pos, int64_t n_pos_max,
                           int64_t pos0, const int32_t *d_pos0, hipStream_t st);
hipError_t launch_attn(const attn_plan &pl, const attn_args &a, hipStream_t st);
// The options of the _ex entries (ggml_hip_attn_ex_dev, ggml_hip_attn_paged_ex_dev), by value to the _ex kernels: sinks f32 [n_head] or null;
// window 0 (none) or W >= 1 (row at position P sees j with P - j < W; clamped to 2^30 by the entry); cap 0 (none) or > 0 with sc = scale / cap
struct attn_var { const float *sinks; int window; float cap, sc; };
// The mask and the ALiBi slopes of the _bias entries (ggml_hip_attn_bias_dev and its paged / ragged twins), by value to the mask kernels: mask f16
// [rows][ld] (the bits of IEEE halves; row = the query's row index in q, column = the position), never null here; slopes f32 [n_head] or null (1.0f)
struct attn_bias { const uint16_t *mask; int64_t ld; const float *slopes; };
// pl: plan_attn_ex's (a windowed DECODE grid holds the chunks the window can touch, workgroup x serves chunk c_lo + x)
// bs: null runs the _ex kernels; otherwise the mask kernels -- the VAR bodies with the mask (vo may have everything off)
hipError_t launch_attn_ex(const attn_plan &pl, const attn_args &a, const attn_var &vo, hipStream_t st, const attn_bias *bs = nullptr);
// The PAGED cache of the paged entries (ggml_hip_kv_store_paged_dev, ggml_hip_rope_kv_store_paged_dev, ggml_hip_attn_paged_dev): a pool of
// n_pages pages of ATTN_CHUNK positions, nb_page bytes apart; entry c of sequence b's table row (ld_pages int32 apart) names the page of its
// positions [128 c, 128 c + 128); len[b] is the positions it held before this step.  Goes to the kernels by value.
struct kv_pages {
    const int32_t *pages; int64_t ld_pages;
    const int32_t *len;
    int64_t nb_page; int n_pages; int n_kv_max;
};
// rows [n_seq * n_q][n_head_kv][D] -> row (b, t, hk) at page row (len[b] + t); a position outside [0, n_kv_max) or a page id outside
// [0, n_pages) writes nothing
hipError_t launch_kv_store_paged(int kv_type, const float *src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D, int64_t n_seq, int64_t n_q, void *pool,
                                 int64_t nb_pos, int64_t nb_head, const kv_pages &pg, hipStream_t st);
// a: k / v are the pools, n_q the rows PER SEQUENCE, q / dst [n_seq * n_q][n_head][D]; n_kv / d_n_kv are not read: n_kv[b] = clamp(len[b] + len_bias, 0, n_kv_max);
// pl: plan_attn_paged's
hipError_t launch_attn_paged(const attn_plan &pl, const attn_args &a, int64_t n_seq, const kv_pages &pg, int len_bias, hipStream_t st);
// pl: plan_attn_paged_ex's; table entries below a sequence's c_lo are never read
hipError_t launch_attn_paged_ex(const attn_plan &pl, const attn_args &a, int64_t n_seq, const kv_pages &pg, int len_bias, const attn_var &vo, hipStream_t st,
                                const attn_bias *bs = nullptr);
// The RAGGED batch of the ragged entries (ggml_hip_ragged_positions_dev, ggml_hip_kv_store_paged_ragged_dev, ggml_hip_rope_kv_store_paged_ragged_dev,
// ggml_hip_attn_paged_ragged_dev): q_start int32 [n_seq + 1] on the device, prefix sums; sequence b owns the packed rows q_start[b] .. q_start[b+1] - 1 and
// is PRESENT when 0 <= q_start[b] <= q_start[b+1] <= n_tokens_max.  Goes to the kernels by value.
struct kv_ragged {
    const int32_t *q_start; int n_seq; int n_tokens_max;
};
#ifdef __HIPCC__
// The sequence of packed row `row` < n_tokens_max by bisection of q_start: the largest b < n_seq with q_start[b] <= row, then every guard in
// front of what it protects -- the sequence is present and the row lies inside it.  Returns b and *t = the row's index in the sequence, or -1
// (the row belongs to no present sequence the bisection finds: nothing is formed from its bounds).  Reads q_start[0 .. n_seq] only.
__device__ __forceinline__ int ragged_find(const kv_ragged &rg, int64_t row, int *t) {
    int lo = 0, hi = rg.n_seq;                                       // (q_start[lo] <= row or lo == 0; q_start[hi] > row or hi == n_seq)
    while (hi - lo > 1) {
        const int mid = (lo + hi) >> 1;
        if ((int64_t)rg.q_start[mid] <= row) lo = mid; else hi = mid;
    }
    const int64_t qs = rg.q_start[lo], qe = rg.q_start[lo + 1];
    if (qs < 0 || qs > qe || qe > rg.n_tokens_max || row < qs || row >= qe) return -1;
    *t = (int)(row - qs);
    return lo;
}
// sequence b by itself (the SSM entries): present -> its first packed row and its count
__device__ __forceinline__ bool ssm_sequence(const kv_ragged &rg, int b, int64_t *qs, int *nq) {
    const int64_t s = rg.q_start[b], e = rg.q_start[b + 1];
    if (s < 0 || s > e || e > rg.n_tokens_max) return false;
    *qs = s; *nq = (int)(e - s);
    return true;
}
#endif
// d_pos[i] = len[b] + t for row i = (b, t) of a present sequence, 0 for the other rows below n_tokens_max
hipError_t launch_ragged_positions(const kv_ragged &rg, const int32_t *len, int32_t *pos, hipStream_t st);
// dst[s][0 .. K) = x[q_start[s+1] - 1][0 .. K) for a present sequence s that is not empty, +0.0f for every other s < n_seq (get_rows.hip)
hipError_t launch_ragged_last_rows(const kv_ragged &rg, const float *x, int64_t ldx, int64_t K, float *dst, int64_t ldd, hipStream_t st);
// launch_kv_store_paged over packed rows [n_tokens_max][n_head_kv][D]: the same bytes for a row of a present sequence, nothing for the others
hipError_t launch_kv_store_paged_ragged(int kv_type, const float *src, int64_t ldx_tok, int64_t ldx_head, int n_head_kv, int D, const kv_ragged &rg, void *pool,
                                        int64_t nb_pos, int64_t nb_head, const kv_pages &pg, hipStream_t st);
// a: k / v are the pools, q / dst the packed rows (a.n_q, a.n_kv, a.d_n_kv are not read), a.work the 256-byte aligned work buffer with pl's index tables
// in front; n_kv[b] = clamp(len[b] + (add_q ? n_q[b] : 0) + len_bias, 0, n_kv_max).  pl: plan_attn_ragged's, every grid and offset; var: the VAR bodies, vo theirs
struct attn_ragged_plan;
hipError_t launch_attn_paged_ragged(const attn_ragged_plan &pl, const attn_args &a, const kv_ragged &rg, const kv_pages &pg, int add_q, int len_bias, bool var,
                                    const attn_var &vo, hipStream_t st, const attn_bias *bs = nullptr);
// mla.hip: latent attention over a latent KV cache (ggml_hip_attn_mla_dev / ggml_hip_attn_mla_paged_dev, mla.cpp; the form is plan.h's plan_attn_mla).
// q [rows][n_head][576] f32, cache: one row of 576 elements per position (the contiguous cache, or the pool of a paged call), dst [rows][n_head][512];
// n_q the rows PER SEQUENCE; n_kv / d_n_kv as attn_args' (a paged call reads neither); work: 256-byte aligned, n_spans = the plan's (SPLIT)
struct mla_plan;
struct mla_args {
    int kv_type, n_head, causal;
    const float *q; int64_t ldq_tok, ldq_head;
    const void *cache; int64_t nb_pos;
    int64_t n_q, n_kv; const int32_t *d_n_kv; int64_t n_kv_max;
    float scale;
    float *dst; int64_t ldd_tok, ldd_head;
    float *work; int64_t n_spans;
};
// pg: null for the contiguous call (n_seq = 1)
hipError_t launch_attn_mla(const mla_plan &pl, const mla_args &a, int64_t n_seq, const kv_pages *pg, int len_bias, hipStream_t st);
// rows [n_seq * n_q][576] -> row (b, t) at the page row of position len[b] + t; a position outside [0, n_kv_max) or a page id outside [0, n_pages) writes nothing
hipError_t launch_kv_store_latent_paged(int kv_type, const float *src, int64_t ld, int64_t n_seq, int64_t n_q, void *pool, int64_t nb_pos, const kv_pages &pg,
                                        hipStream_t st);
// rope.hip: the rotation of Q / K rows (ggml_hip_rope_dev) and the rotation fused with kv_store (ggml_hip_rope_kv_store_dev; rope.cpp).
// The per-pair constants are the HOST's (ggml_hip_rope_table) and go to the kernels by value: eff[i] for pair i < n_dims / 2, and mscale
#define ROPE_MAX_PAIRS 128
struct rope_table { double eff[ROPE_MAX_PAIRS]; double mscale; };
struct rope_args {
    int mode, n_dims, n_head, D;                                     // mode: 0 NORMAL, 2 NEOX
    const float *x; int64_t ldx_tok, ldx_head; int64_t n_tokens;
    const int32_t *d_pos; int64_t pos0; const int32_t *d_pos0;       // token t sits at d_pos[t], or at (d_pos0 ? *d_pos0 : pos0) + t
    const float *freq_factors;
};
hipError_t launch_rope(const rope_table &tab, const rope_args &a, float *dst, int64_t ldd_tok, int64_t ldd_head, hipStream_t st);
// (a.d_pos is not read: the rope position is the cache position)
hipError_t launch_rope_kv_store(const rope_table &tab, const rope_args &a, int kv_type, void *cache, int64_t nb_pos, int64_t nb_head, int64_t n_pos_max,
                                hipStream_t st);
// the same into a paged cache: a.n_tokens = n_seq * n_q rows, token (b, t) at position pg.len[b] + t (a.d_pos, a.pos0 and a.d_pos0 are not read)
hipError_t launch_rope_kv_store_paged(const rope_table &tab, const rope_args &a, int kv_type, int64_t n_q, void *pool, int64_t nb_pos, int64_t nb_head,
                                      const kv_pages &pg, hipStream_t st);
// the same over packed rows: a.n_tokens = rg.n_tokens_max, the row's sequence and position from ragged_find
hipError_t launch_rope_kv_store_paged_ragged(const rope_table &tab, const rope_args &a, int kv_type, const kv_ragged &rg, void *pool, int64_t nb_pos,
                                             int64_t nb_head, const kv_pages &pg, hipStream_t st);
// ssm.hip: the causal conv and the selective scan of a Mamba block over a ragged batch and a pool of f32 state slots (ggml_hip_ssm_conv_ragged_dev /
// ggml_hip_ssm_scan_ragged_dev, ssm.cpp; the grids are plan.h's plan_ssm_conv / plan_ssm_scan).  len / slot: int32 [n_seq]; slot_elems: floats between slots
struct ssm_conv_plan;
struct ssm_scan_plan;
hipError_t launch_ssm_conv(const ssm_conv_plan &pl, const kv_ragged &rg, const int32_t *len, const int32_t *slot, int n_slots, const float *x, int64_t ldx,
                           const float *w, const float *bias, int act, int64_t n_ch, int d_conv, float *state, int64_t slot_elems, float *dst, int64_t ldd,
                           int nq_max, hipStream_t st);                  // nq_max: the kernel serves sequences of 1 .. nq_max tokens in this call (INT_MAX: all)
// ssm_conv_tile.hip: the same call with the sequences above pl.seq_max_tokens in the token-parallel tiled form (ggml_hip_ssm_conv_tiled_ragged_dev; plan.h
// plan_ssm_conv_tiled has the launches and the work buffer).  work: the 256-byte aligned base, null where pl.form is sequential
struct ssm_conv_tiled_plan;
hipError_t launch_ssm_conv_tiled(const ssm_conv_tiled_plan &pl, const kv_ragged &rg, const int32_t *len, const int32_t *slot, int n_slots, const float *x,
                                 int64_t ldx, const float *w, const float *bias, int act, int64_t n_ch, int d_conv, float *state, int64_t slot_elems, float *dst,
                                 int64_t ldd, void *work, hipStream_t st);
struct ssm_scan_args {
    const float *x; int64_t ldx_tok, ldx_head;                       // [tok][n_head][P]
    const float *dt; int64_t ld_dt; const float *dt_bias;            // [tok][n_head]; [n_head] or null
    const float *A; int64_t a_ld; int a_per_state;                   // [n_head][a_ld]: one value per head, or N per head
    const float *B, *C; int64_t ld_bc;                               // [tok][n_group][N], ld_bc floats between tokens (both)
    const float *D;                                                  // [n_head] or null
    int n_head, P, N, n_group;
    const int32_t *len, *slot; int n_slots;
    float *state; int64_t slot_elems;
    float *dst; int64_t ldd_tok, ldd_head;
    int nq_max;                                                      // the sequential kernel serves sequences of 1 .. nq_max tokens in this call (INT_MAX: all)
};
hipError_t launch_ssm_scan(const ssm_scan_plan &pl, const kv_ragged &rg, const ssm_scan_args &a, hipStream_t st);
// ssm_chunk.hip: the same call with the sequences above pl.seq_max_tokens in the chunked matrix form (ggml_hip_ssm_scan_chunked_ragged_dev; plan.h
// plan_ssm_chunk has the launches and the work buffer).  a.nq_max is set here; work: the 256-byte aligned base, null where pl.form is sequential
struct ssm_chunk_plan;
hipError_t launch_ssm_scan_chunked(const ssm_chunk_plan &pl, const kv_ragged &rg, const ssm_scan_args &a, void *work, hipStream_t st);
// gemm_q8s.hip / gemm_qmx.hip: ONE K3s launch over the tile table -- workgroup -> (weight tile group, column tile t); t >= *n_tiles leaves at once;
// the expert's planes come from tab[tiles[t].expert], the 32 sorted rows at 32 t of the image p (K1's image of `32 * max_tiles` rows); res [rows][ldr]
hipError_t launch_gemm_q8_small_grouped(const mm_plan &g, int type, const moe_gexpert *tab, const moe_tile *tiles, const int32_t *n_tiles, int64_t max_tiles,
                                        int64_t M, int64_t Mpad, int64_t nbk, act_planes p, float *res, int64_t ldr, hipStream_t st);
hipError_t launch_gemm_qmx_small_grouped(const mm_plan &g, int type, const moe_gexpert *tab, const moe_tile *tiles, const int32_t *n_tiles, int64_t max_tiles,
                                         int64_t M, int64_t Mpad, int64_t nbk, act_planes p, float *res, int64_t ldr, hipStream_t st);
hipError_t launch_gemm_q(const ggml_hip_weight *w, const mm_plan &pl, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st);
// Q8_0, 5 <= N <= 64, K >= 2048: the stage-free batched-decode form on the int8 matrix cores (gemm_q8s.hip; image 0 of K1); ep: add / scale in the store phase
hipError_t launch_gemm_q8_small(const ggml_hip_weight *w, const mm_plan &pl, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st, const mm_epilogue *ep);
hipError_t launch_gemm_q8_small_multi(const mm_plan &g, const ggml_hip_weight *const *w, int n_w, act_planes p, int64_t N, float *const *dst, const int64_t *ldd,
                                      hipStream_t st);
hipError_t launch_gemm_q16(const ggml_hip_weight *w, const mm_plan &pl, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st);
// 2..4 matrices of one type and K behind one activation image in ONE launch of the group plan g (plan.h plan_mul_mat_group: K3s,
// Q4_0 / Q4_1 here, Q8_0 in gemm_q8s.hip); hipErrorNotSupported where a plane or dst is beyond the kernel -- the caller then computes
// them one after the other
hipError_t launch_gemm_qmx_multi(const mm_plan &g, const ggml_hip_weight *const *w, int n_w, act_planes p, int64_t N, float *const *dst, const int64_t *ldd,
                                 hipStream_t st);
hipError_t launch_gemm_qmx(const ggml_hip_weight *w, const mm_plan &pl, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st,
                           const mm_epilogue *ep);
// The fused route of the Q4_0 256 x 128 form: K1's head launch for the first K quarter, then ONE launch that quantizes the other three quarters of src1
// inside the K loop, a quarter ahead of it (gemm_qmx.hip mx_fuse).  The same image bytes and the same product bits as INIT + COMPUTE.  _serves: by
// weight, plan and N alone; the launch also wants src1 as K1's lane-per-block kernel does (quantize_act_bf6_serves), else hipErrorNotSupported.
bool gemm_qmx_fused_serves(const ggml_hip_weight *w, const mm_plan &pl, int64_t N);
hipError_t launch_gemm_qmx_fused(const ggml_hip_weight *w, const mm_plan &pl, const float *x, int64_t ld1, act_planes p, int64_t N, float *dst, int64_t ldd,
                                 hipStream_t st);
void gemm_qmx_fused_skip_panel(int panel);                  // TEST HOOK: the producers of this column panel leave their shares to the help path (-1: none)
// Q4_0, prompt-sized batches, K >= 2048 (gemm_qmp.hip K3p); hipErrorNotSupported where the form does not apply
hipError_t launch_gemm_qmx_mid(const ggml_hip_weight *w, const mm_plan &pl, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st, const mm_epilogue *ep);
// the same form on the int8 matrix cores: Q8_0, image 0 (gemm_qmp.hip)
hipError_t launch_gemm_q8_mid(const ggml_hip_weight *w, const mm_plan &pl, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st, const mm_epilogue *ep);
hipError_t launch_dense(const ggml_hip_weight *w, const mm_plan &pl, const float *x, int64_t N, int64_t ld1, float *dst, int64_t ldd,
                        hipStream_t st);

// N at or below this goes to the wave-reduction mat-vec kernel, above it to the MFMA kernel.
#define GEMV_MAX_N 8
// ... and up to this many src1 rows the mat-vec kernel serves the type that has no small-batch MFMA configuration (Q4_2),
// in its two-step form (K1 planes, 16 columns per pass over the weights): 15 us at 4096 x 4096 x 16.  For the other
// types the 32-row, four-way-K-split tiles of gemm_qmx.hip / gemm_q16.hip take over at 9 rows (13 us / 16.5 us there).
#define GEMV_WIDE_MAX_N 16
