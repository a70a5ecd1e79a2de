// plan.cpp -- the ONE place where a product's kernel family, form and summation tree are decided (plan.h).  Host code only: no
// device is touched, so the whole decision surface is testable in a container without a GPU (tests/test_plan_cpu.py sweeps
// type x K x N x M through ggml_hip_mm_plan and asserts that tree_id never depends on M; tools/plan_dump.cpp hashes every decision
// over a wider sweep, for changes that must not move one).
//
// Every threshold here is a measurement on MI355X.  The code keeps the rule; the measurements behind it are in docs/PLAN_BOUNDS.md,
// one section per constant or rule, cited here by its name in quotes behind the file's name (tests/test_plan_cpu.py checks that every cited
// section exists).
#include "common.h"
#include "plan.h"

namespace {

thread_local int t_force_gemm = 0;   // 0 auto, 1 int8, 2 f16, 3 MX.  Per calling thread: a test hook never reaches another thread's calls

inline bool is_quant(int t) { return t >= GGML_TYPE_Q4_0 && t <= GGML_TYPE_Q8_1; }
inline int64_t cdiv(int64_t a, int64_t b) { return (a + b - 1) / b; }
constexpr uint64_t LIM32 = 0xFFFFFFFFull;                  // 32-bit buffer offsets
constexpr int64_t NO_TOP = INT64_MAX;

// ---- what the plan knows about a resident quantized type: one row each ----
struct plan_row {
    int type;
    bool min_term;         // a min term per k-block (INIT writes the min-term piece planes for the int8 stage-free pair)
    bool mx;               // MX-native: served from the bf6 image (3) on the MX cores
    bool two_scale;        // two scales per k-block: the mat-vec and the int8 kernels only
    bool kq_home;          // k-quants live in this planar form (ext_type != 0): the Q8_K rule, a fused mat-vec of their own (kq_fused_serves)
    int gemv_rows;         // src1 rows up to which the two-step mat-vec serves the type
    int k3s_first;         // first src1 row count of K3s-int8 (0: no int8 pair; the ext_type variations: k3s_i8_first)
    int64_t k3p_top;       // last src1 row count of K3p-int8 (0: no K3p-int8)
    bool four_tiles;       // K3s: four 32-row tiles per workgroup beyond 512 tile groups (else two: registers)
    bool tile16_i8;        // K3s-int8: 16-row tiles (the MX form has them for both of its types)
    int arith_i8;          // label of the stage-free int8 pair: 300, + 1 min term, + 2 fma(sumi, d1 * d0), + 4 two fma(d * yd, sumi) per k-block
    int arith_k3_mx;       // label of the stage-free MX pair
    int f16_image;         // the f16 image kind of the staged f16 family
};
// Q5_1 / Q4_2 from 9 rows: up to 8 their mat-vec is as fast; Q4_1 from 65 (q41_pair_min): below, its MX form.  K3p tops: beyond 3072
// rows the staged f16 forms of Q8_0 / Q5_0 win.  PLAN_BOUNDS.md "The stage-free int8 pair" has the table and its measurements.
constexpr plan_row ROWS[] = {
    //  type          min    mx     two    kq     gemv rows        first  top     four   t16    i8   k3mx f16
    {GGML_TYPE_Q4_0, false, true,  false, false, GEMV_MAX_N,      0,     0,      true,  false, 0,   310, 1},
    {GGML_TYPE_Q4_1, true,  true,  false, false, GEMV_MAX_N,      65,    1024,   false, false, 301, 211, 1},
    {GGML_TYPE_Q4_2, false, false, true,  true,  GEMV_WIDE_MAX_N, 9,     NO_TOP, false, true,  304, 0,   1},
    {GGML_TYPE_Q5_0, false, false, false, false, GEMV_MAX_N,      5,     3072,   true,  true,  300, 0,   1},
    {GGML_TYPE_Q5_1, true,  false, false, true,  GEMV_MAX_N,      9,     NO_TOP, false, true,  301, 0,   1},
    {GGML_TYPE_Q8_0, false, false, false, false, GEMV_MAX_N,      5,     3072,   true,  true,  302, 0,   2},
};
constexpr plan_row NO_ROW = {-1, false, false, false, false, GEMV_MAX_N, 0, 0, false, false, 0, 0, 1};   // (the block types that are no weight types)
const plan_row &row_of(int type) {
    for (const plan_row &r : ROWS)
        if (r.type == type) return r;
    return NO_ROW;
}
// Q4_1 joins the int8 pair at 65 src1 rows, behind a long K (its min-term pieces grow with K) at 129: PLAN_BOUNDS.md "q41_pair_min"
int64_t q41_pair_min(int64_t K) { return K >= 11008 ? 129 : 65; }
// first src1 row count K3s-int8 serves, 0: none.  Q4_1 only behind K >= 2048 (below, its MX form) and never as a k-quant's home; a k-quant in
// the two-scale form has no nibble plane, so its mat-vec ends at 4 rows and K3s starts at 5.
int64_t k3s_i8_first(const plan_row &r, int ext_type, int64_t K) {
    if (r.k3s_first == 0) return 0;
    if (r.mx) return ext_type != 0 || K / QK < 64 ? 0 : q41_pair_min(K);
    return r.two_scale && ext_type != 0 ? 5 : r.k3s_first;
}
// the k-quants' fused mat-vec (gemv.hip K8, the Q8_K rule in the kernel): up to 4 rows and K = 32768
bool kq_fused_serves(const plan_row &r, int64_t K, int64_t N) { return r.kq_home && N <= 4 && K % 256 == 0 && K / 256 <= 128; }

// ---- the stage-free pairs: K3s (batched decode; gemm_q8s.hip, gemm_qmx.hip launch_small) and K3p (prompt sizes; gemm_qmp.hip) ----
// Eight waves, each a contiguous range of k3_nloc(K) k-blocks -- an even number, so pairs of blocks (and the min term's pairs) stay inside
// one wave.  K3s and K3p of one type share that rule, the statement per block and the wave-order sum: ONE summation tree and one
// arithmetic label (tests/test_gpu_fullsize.py test_k3s_and_k3p_*_compute_the_same_bits), so where both serve the FAMILY may follow M.
constexpr int KS8 = 8;
int k3_nloc(int64_t K) { int n = (int)cdiv(pad_kblocks(K / QK), KS8); return n + (n & 1); }
// K3p's scale tables: a wave's whole range up to 80 k-blocks, beyond that in up to four refilled slices of 78 (K <= 79872; plan.h)
bool k3p_lds_ok(int nloc) { return nloc <= K3P_MAX_SLICES * K3P_SLICE_ROWS; }
// Both serve from K3_DUAL_MIN (below, half of K3p's 64-column tile is padding) to K3_DUAL_MAX src1 rows (a short matrix at prompt sizes is
// too few workgroups of K3p): PLAN_BOUNDS.md "K3_DUAL_MIN", "K3_DUAL_MAX"
constexpr int64_t K3_DUAL_MIN = 33, K3_DUAL_MAX = 512;
// K3s from this many k-blocks (K = 1024), up to 64 src1 rows behind K < 2048 where no K3p exists: PLAN_BOUNDS.md "K3S_KMIN"
constexpr int64_t K3S_KMIN = 32;
// where both serve, K3p takes over from this many workgroups of 64-row tiles: PLAN_BOUNDS.md "k3_dual_wgs"
int64_t k3_dual_wgs(int64_t K) { return K >= 11008 ? 192 : 160; }

// The 32-bit buffer offsets of the stage-free kernels, each its kernel's real bound: the weight planes (MX: 16 bytes per row and k-block,
// K3s reads K_LOOKAHEAD blocks ahead; int8: two 16-byte pieces) and the activation image (MX: 48 bytes per row and k-block).  K3p's waves
// reach two blocks past their ranges.
bool k3s_weights_fit32(bool mx, int64_t K, int64_t Mpad) {
    const uint64_t nbkp = (uint64_t)pad_kblocks(K / QK);
    return (mx ? (nbkp + K_LOOKAHEAD) * (uint64_t)Mpad * 16 : nbkp * 2 * (uint64_t)Mpad * 16) <= LIM32;
}
bool k3s_act_fits32(bool mx, int64_t K, int64_t Npad) {
    const uint64_t nbkp = (uint64_t)pad_kblocks(K / QK);
    return (mx ? nbkp * 48 * (uint64_t)Npad : nbkp * 2 * (uint64_t)Npad * 16) <= LIM32;
}
bool k3p_fits32(bool mx, int nloc, int64_t Mpad, int64_t Npad) {
    const uint64_t nb = (uint64_t)(KS8 * nloc + 2);
    return mx ? nb * (uint64_t)Mpad * 16 <= LIM32 && nb * 48 * (uint64_t)Npad <= LIM32
              : nb * 2 * (uint64_t)Mpad * 16 <= LIM32 && nb * 2 * (uint64_t)Npad * 16 <= LIM32;
}
// the MX / f16 images of the staged families: 64 bytes per row and k-block
bool act_image_fits32(int64_t K, int64_t N) { return (uint64_t)pad_kblocks(K / QK) * 64 * (uint64_t)pad_act(N) <= LIM32; }
// the generic bound of a weight plane (the stated exception of plan.h: beyond it the int8 family serves whatever the type)
bool weight_planes_fit32(int64_t K, int64_t Mpad) { return ((uint64_t)pad_kblocks(K / QK) + K_LOOKAHEAD) * (uint64_t)Mpad * 32 <= LIM32; }

// THE stage-free decision: which of K3s and K3p serve (type, ext_type, K, N), on which cores, and which is tried first.  By (type, K, N)
// alone but for the order, which follows M where both serve.  `image`: what the staged families would have INIT write (staged_image).
//   int8 pair (image 0, + the min-term piece planes), never under a forced family:
//     K3s  K from 1024 to 32768, from the type's first row count to 64 rows, behind K >= 2048 to K3_DUAL_MAX
//     K3p  K from 2048 while its tables fit, from K3_DUAL_MIN rows (Q4_1: q41_pair_min; K > 32768: 129, K3p alone) to the type's top
//   MX pair (image 3), for the MX-native types wherever the int8 pair does not serve:
//     K3s  K from 1024, up to 64 rows; behind K >= 2048 Q4_1 up to 128 and Q4_0 up to K3_DUAL_MAX
//     K3p  Q4_0 alone (Q4_1's K3p is the int8 kernel): K3_DUAL_MIN .. K3_DUAL_MAX rows behind K >= 2048, from 257 rows behind a shorter K
// PLAN_BOUNDS.md "The stage-free int8 pair", "The stage-free MX pair"
struct k3_choice { bool mx, k3s, k3p, k3p_first; };
k3_choice k3_stage_free(const plan_row &r, int ext_type, int image, int64_t M, int64_t K, int64_t N) {
    const int64_t nbk = K / QK;
    k3_choice c = {};
    if (nbk < K3S_KMIN) return c;
    const bool pair = nbk >= 64;                            // (K3p's waves want 8 k-blocks each)
    if (plan_force_gemm() == 0) {
        const int64_t first = k3s_i8_first(r, ext_type, K);
        c.k3s = first != 0 && nbk <= 1024 && N >= first && N <= (pair ? K3_DUAL_MAX : 64);
        const int64_t pmin = nbk > 1024 ? 129 : r.mx ? q41_pair_min(K) : K3_DUAL_MIN;
        c.k3p = r.k3p_top != 0 && pair && k3p_lds_ok(k3_nloc(K)) && N >= pmin && N <= r.k3p_top;
    }
    if (!c.k3s && !c.k3p && r.mx && image == 3) {
        c.mx = true;
        c.k3s = N <= (!pair ? 64 : r.min_term ? 128 : K3_DUAL_MAX);
        c.k3p = !r.min_term && N <= K3_DUAL_MAX && N >= (pair ? K3_DUAL_MIN : 257);
    }
    c.k3p_first = c.k3s && c.k3p && cdiv(M, 64) * cdiv(N, 64) >= k3_dual_wgs(K);
    return c;
}

// What INIT writes for the staged families and the mat-vec (the stage-free pairs: k3_stage_free): 0 = int8 planes, 1 / 2 = the f16 images,
// 3 = the bf6 image.  NOT a function of the number of weight rows.
int staged_image(const plan_row &r, int64_t K, int64_t N) {
    const int force = plan_force_gemm();
    if (N <= 4 || force == 1) return 0;
    // 5..8 rows: the mat-vec -- except where K3s-MX exists, which runs one image and kernel from 5 rows on: PLAN_BOUNDS.md "K3s-MX from 5 rows"
    if (N <= GEMV_MAX_N && !(force == 0 && r.mx && K / QK >= K3S_KMIN)) return 0;
    if (r.two_scale || !act_image_fits32(K, N)) return 0;
    if (force == 2) return r.f16_image;
    if (force == 3) return r.min_term && !r.mx ? 0 : 3;     // (a min-term type without an MX form: the forced choice falls back to the int8 kernel)
    if (r.mx) return 3;
    // the f16 kernel's K-split form wins on prompt-sized batches and its unsplit forms from 1024 rows up; in between the int8 kernel's
    // 64 x 64 tiles balance the chip better.  Decided from N and K only, like the K split itself.
    return ((N <= 512 || N >= 1024) && K / QK >= 8) ? r.f16_image : 0;
}

}  // namespace

int plan_force_gemm() { return t_force_gemm; }
void plan_set_force_gemm(int which) { t_force_gemm = which < 0 || which > 3 ? 0 : which; }

// The K1 image for (type, K, N) with no weight at hand: derived, not decided -- the image of the COMPUTE-only plan at M = 1, as api.cpp's
// weight_image_kind takes it for a weight.  0 + ACT_IMAGE_MIN_PIECES (64) = the int8 planes and the min-term piece planes.
int plan_act_image(const mm_plan &p) { return (p.image >= 0 && p.image <= 3 ? p.image : 0) | ((p.flags & MM_FLAG_MIN_PIECES) ? ACT_IMAGE_MIN_PIECES : 0); }
int plan_image_kind(int type, int64_t K, int64_t N) { return plan_act_image(plan_mul_mat(type, 0, 1, K, N, false)); }

namespace {

// ---- family plans ----

void plan_gemv(mm_plan &p, int64_t M, int64_t K, int64_t N, bool fused) {
    p.family = fused ? MMF_GEMV_FUSED : MMF_GEMV_ROWS;
    p.image = fused ? -1 : 0;
    // 16 rows per workgroup for every M (gemv.hip launch_typed: a choice by M would change the tree); 8 waves x 4 k-lanes = 32 k-workers,
    // worker u takes k-blocks u, u + 32, ...; two xor-shuffles + one LDS pass join them in a fixed order
    p.form = N <= 1 ? 1 : N <= 2 ? 2 : N <= 4 ? 4 : N <= 8 ? 8 : 16;                    // columns per pass (NC)
    // ONE label: the wave-private fused form (N <= 4) is its own kernel with the SAME quants and tree as INIT + the mat-vec, bitwise equal
    // (tests/test_gpu_parity.py test_small_n_fused_path_equals_two_step_path), so tree_id is what the COMPUTE-only entry runs too
    p.arith = 100;
    p.ksplit = 32; p.kstyle = MMK_WORKERS; p.kunit = 1;
    p.tile_m = 16; p.tile_n = p.form; p.waves = 8; p.tiles_per_wave = 1;
    const int64_t ntiles = cdiv(M, 16);
    p.wgs = ntiles < 512 ? ntiles : 512;
    if (fused && (N <= 1 || N >= 3) && K / QK <= 128 && ntiles > 256) p.wgs = 256;       // the look-ahead form: one workgroup per CU
    p.flags |= MM_FLAG_PERSISTENT;
    if (fused && N >= 1 && N <= 4) p.flags |= MM_FLAG_EPILOGUE_FUSED;
}

// A K3s plan on 32-row tiles, single or grouped: everything but the form, the grid and the launch flags.  So a group's labels are the
// single product's by construction.
void set_k3s(mm_plan &p, const plan_row &r, bool mx, int nloc, int wmt) {
    p.family = mx ? MMF_K3S_MX : MMF_K3S_I8; p.image = mx ? 3 : 0;
    if (!mx && r.min_term) p.flags |= MM_FLAG_MIN_PIECES;
    p.arith = mx ? r.arith_k3_mx : r.arith_i8;
    p.ksplit = KS8; p.kstyle = MMK_RANGES; p.kunit = nloc; p.nloc = nloc; p.wmt = wmt;
    p.tile_m = 32 * wmt; p.tile_n = 32; p.waves = KS8; p.tiles_per_wave = wmt;
}
// 32-row tiles per K3s workgroup by the number of tile groups: one round of the chip each; four only where the type's registers allow it
// (PLAN_BOUNDS.md "k3s_wmt")
int k3s_wmt(const plan_row &r, int64_t t32) { return t32 <= 256 ? 1 : (t32 <= 512 || !r.four_tiles) ? 2 : 4; }

// 16-row tiles where the 32-row tiles of K3s leave CUs idle (gemm_q8s.hip gemm_q8_small16_kernel, gemm_qmx.hip gemm_qmx_small16_kernel).
// GEOMETRY ONLY: the same eight K ranges, block order, statement and wave-order sum -- tree_id does not move, so this choice MAY look at M.
// A workgroup takes 16 rows x the src1 rows in 16-column slices, one slice while two workgroups per weight tile still fit one round; one
// round of the chip only.  The LDS the launch needs follows from the plan (plan_k3s_slots).  PLAN_BOUNDS.md "K3S_16_NMAX / K3S_16_WGS"
constexpr int64_t K3S_16_NMAX = 512, K3S_16_WGS = 256;
void k3s_tile16(mm_plan &p, int type, int64_t M, int64_t N) {
    if (N > K3S_16_NMAX) return;
    const int tn16 = N <= 16 || cdiv(M, 16) * cdiv(N, 16) <= K3S_16_WGS ? 16 : 32;
    mm_plan q = p;
    q.form = 5 + (tn16 == 16 ? 0 : 1);
    q.wmt = 1; q.tile_m = 16; q.tile_n = tn16; q.tiles_per_wave = tn16 / 16; q.wgs = cdiv(M, 16) * cdiv(N, tn16);
    if (plan_k3s_slots(q, type).lds > 160 * 1024 || q.wgs > K3S_16_WGS) return;   // (the LDS of a CU; one round)
    p = q;
}

// K3s of either pair: up to 128 k-blocks per wave (two rounds of table pieces: K <= 32768)
bool plan_k3s(mm_plan &p, const plan_row &r, bool mx, int64_t M, int64_t Mpad, int64_t K, int64_t N) {
    const int nloc = k3_nloc(K);
    if (nloc > 128 || !k3s_weights_fit32(mx, K, Mpad) || !k3s_act_fits32(mx, K, pad_act(N))) return false;
    const int64_t ncol = cdiv(N, 32);
    const int wmt = k3s_wmt(r, cdiv(M, 32) * ncol);
    set_k3s(p, r, mx, nloc, wmt);
    p.form = mx ? 0 : wmt == 4 ? 7 : wmt == 2 ? (nloc <= 8 ? 0 : 1) : nloc <= 8 ? 2 : nloc <= 16 ? 3 : 4;
    p.wgs = cdiv(M, 32 * wmt) * ncol;
    p.flags |= MM_FLAG_EPILOGUE_FUSED;
    if (mx || r.tile16_i8) k3s_tile16(p, r.type, M, N);
    return true;
}

// K3p of either pair (gemm_qmp.hip) on 128 x 64 tiles, or on 64-row wave tiles (two m-tiles instead of four) where the 128-row tiles leave
// the chip idle.  GEOMETRY ONLY, as above, so the choice may look at M (gemm_q8_mid_kernel<..., WM = 2>).  64-row tiles wherever their
// grid is one round; the int8 kernel (a 64-row workgroup costs 0.545 of a 128-row one) also on grids of a fractional number of rounds where
// ceil(workgroups / 256) rounds say they pay, with 7 % of margin; the MX kernel (0.63) for one round only.
// PLAN_BOUNDS.md "The K3p 64-row-tile rule"
bool plan_k3p(mm_plan &p, const plan_row &r, bool mx, int64_t M, int64_t Mpad, int64_t K, int64_t N) {
    const int nloc = k3_nloc(K);
    if (nloc < 8 || !k3p_lds_ok(nloc) || !k3p_fits32(mx, nloc, Mpad, pad_act(N))) return false;
    p.family = mx ? MMF_K3P_MX : MMF_K3P_I8; p.image = mx ? 3 : 0;
    p.arith = mx ? r.arith_k3_mx : r.arith_i8;
    if (!mx && r.min_term) p.flags |= MM_FLAG_MIN_PIECES;
    const int64_t wg128 = cdiv(M, 128) * cdiv(N, 64), wg64 = cdiv(M, 64) * cdiv(N, 64);
    const double r128 = (double)cdiv(wg128, 256), r64 = (double)cdiv(wg64, 256) * 0.545;
    const bool h64 = wg64 <= 256 || (!mx && r64 <= 0.93 * r128);
    p.form = 0; p.ksplit = KS8; p.kstyle = MMK_RANGES; p.kunit = nloc; p.nloc = nloc;
    p.wmt = h64 ? 2 : 4; p.tile_m = h64 ? 64 : 128; p.tile_n = 64; p.waves = KS8; p.tiles_per_wave = h64 ? 4 : 8;
    p.wgs = h64 ? wg64 : wg128;
    p.flags |= MM_FLAG_EPILOGUE_FUSED;
    return true;
}

struct FormGeo { int wmt, wnt, wgm, wgn, ksp, vs; };
void set_staged_geo(mm_plan &p, const FormGeo &g, int64_t M, int64_t N) {
    p.tile_m = g.wgm * g.wmt * 32; p.tile_n = g.wgn * g.wnt * 32;
    p.waves = g.wgm * g.wgn * g.ksp; p.tiles_per_wave = g.wmt * g.wnt;
    p.ksplit = g.ksp * g.vs; p.kstyle = p.ksplit > 1 ? MMK_STAGE_SETS : MMK_CHAIN; p.kunit = 4;
    p.wgs = cdiv(M, p.tile_m) * cdiv(N, p.tile_n);
}

// the staged MX family (gemm_qmx.hip launch_typed): the MX-native types (+ Q5_0 / Q8_0 with two weight digits when MX is forced), wherever
// the stage-free pair does not serve.  The choice of the SPLIT depends on N and K only; the tile height follows the tile count.
void plan_mx(mm_plan &p, const plan_row &r, int type, int64_t M, int64_t K, int64_t N) {
    const int64_t nbk = K / QK;
    const int64_t tm256 = cdiv(M, 256), tm128 = cdiv(M, 128), tn128 = cdiv(N, 128), t64 = cdiv(M, 64) * cdiv(N, 64);
    // one weight digit and one scale plane (Q4_0): the registers for 8 tiles per wave, for 128-row split tiles and for the 64 x 64 form
    const bool lean = r.mx && !r.min_term;
    static const FormGeo geo[] = {{2, 4, 4, 1, 1, 1}, {/* 1: retired */}, {1, 1, 2, 1, 4, 1}, {1, 1, 1, 1, 4, 1}, {1, 2, 4, 1, 4, 1}, {1, 2, 2, 1, 4, 1},
                                  {1, 2, 1, 1, 4, 1}, {1, 2, 2, 1, 2, 2}, {1, 2, 4, 1, 2, 1}, {1, 2, 2, 1, 2, 1}, {2, 2, 2, 2, 1, 1}, {1, 1, 2, 2, 1, 1},
                                  {1, 2, 4, 1, 1, 1}};
    auto take = [&](int f) {
        p.family = MMF_MX; p.image = 3; p.form = f;
        set_staged_geo(p, geo[f], M, N);
        // a min-term type: with ONE tile per wave the min-term MFMA lands between other scale-accumulates of its tile than in the multi-tile
        // forms (a different f32 addition order): the one-tile forms are chosen by N alone (up to 32 rows), the 64 x 64 form is Q4_0's only
        p.arith = 400 + (r.mx ? (r.min_term ? 1 + (p.tiles_per_wave == 1 ? 1 : 0) : 0) : 10 + type);
        p.flags |= MM_FLAG_EPILOGUE_FUSED;
    };
    // 256 x 128 tiles (unsplit, above 512 rows only: below, every form splits K) as soon as the 128 x 128 form would need MORE than one
    // round of the chip: PLAN_BOUNDS.md "MXF_256x128"
    if (lean && tm256 * tn128 >= 257 && N > 512) return take(MXF_256x128);
    // up to 128 rows (a min-term type: 256): 32-row weight tiles with K split four ways inside the workgroup; the same four-way tree on
    // taller tiles where those cover the chip
    if (N <= (lean ? 128 : 256) && nbk >= 16) {
        if (N <= 32) return take(t64 < 160 ? MXF_N32_H32 : MXF_N32_H64);
        if (t64 < 160) return take(MXF_S4_H32);
        return take(t64 <= 320 || !lean ? MXF_S4_H64 : MXF_S4_H128);
    }
    // 129 .. 256 rows (Q4_0): the four-way tree as well -- really split while the tiles are few, else two wave groups that each run two
    // of the four stage sets one after the other (same tree, same bits)
    if (lean && N <= 256 && nbk >= 16) return take(t64 <= 256 ? MXF_S4_H64 : MXF_S2V2_H64);
    if (N <= 512 && nbk >= 8) return take(tm128 * cdiv(N, 64) >= 1536 ? MXF_S2_H128 : MXF_S2_H64);
    // PLAN_BOUNDS.md "MXF_128x128"
    if (tm128 * tn128 >= 384) return take(MXF_128x128);
    // a short, wide product (a row shard of a multi-GPU split): 64 x 64 tiles of four 1-tile waves wherever the 128 x 64 grid leaves
    // CUs idle -- the same unsplit K loop per element, the same bits, only the geometry follows M (Q4_0 only: see `arith` above)
    if (lean && tm128 * cdiv(N, 64) <= 256) return take(MXF_64x64);
    return take(MXF_128x64);
}

// the staged f16 family (gemm_q16.hip launch_typed)
void plan_f16(mm_plan &p, const plan_row &r, int type, int64_t M, int64_t K, int64_t N) {
    const int64_t nbk = K / QK, t64 = cdiv(M, 64) * cdiv(N, 64);
    const bool mn = r.min_term;
    static const FormGeo geo[] = {{1, 1, 2, 1, 4, 1}, {1, 1, 1, 1, 4, 1}, {1, 2, 4, 1, 4, 1}, {1, 2, 2, 1, 4, 1}, {1, 2, 1, 1, 4, 1},
                                  {1, 2, 4, 1, 2, 1}, {2, 4, 4, 1, 1, 1}, {1, 1, 2, 2, 1, 1}, {1, 2, 4, 1, 1, 1}};
    auto take = [&](int f) {
        p.family = MMF_F16; p.image = r.f16_image; p.form = f;
        set_staged_geo(p, geo[f], M, N);
        // the min term: on the matrix pipe per pair of k-blocks in the forms that split K, on the VALU per block in the unsplit ones --
        // by the SPLIT (i.e. by N and K), not by the tile count (r3)
        p.arith = 500 + type * 4 + (mn ? (p.ksplit > 1 ? 1 : 2) : 0);
    };
    if (N <= 256 && nbk >= 16) {   // (the four-way split; 128 was the former bound)
        if (N <= 32) return take(t64 < 160 ? F16F_N32_H32 : F16F_N32_H64);
        if (t64 < 160) return take(F16F_S4_H32);
        return take(t64 <= 320 || mn ? F16F_S4_H64 : F16F_S4_H128);
    }
    if (N <= 512 && nbk >= 8) return take(F16F_S2_H128);
    if (cdiv(M, 256) * cdiv(N, 128) >= 384) return take(F16F_256x128);
    if (!mn && cdiv(M, 128) * cdiv(N, 64) <= 256) return take(F16F_64x64);
    return take(F16F_128x64);
}

// the staged int8 family (gemm_q.hip): 128 x 128 tiles when they already give >= 2 workgroups per CU, else 64 x 64; one chain over K either way
void plan_i8(mm_plan &p, int type, int64_t M, int64_t N) {
    const bool b = cdiv(M, 128) * cdiv(N, 128) >= 512;
    p.family = MMF_I8; p.image = 0; p.form = b ? I8F_128x128 : I8F_64x64;
    p.arith = 600 + type; p.ksplit = 1; p.kstyle = MMK_CHAIN; p.kunit = 4;
    p.tile_m = p.tile_n = b ? 128 : 64; p.waves = 4; p.tiles_per_wave = b ? 4 : 1;
    p.wgs = cdiv(M, p.tile_m) * cdiv(N, p.tile_n);
}

// the 32-bit offsets of dense16.hip's panels: `pieces` 16-byte panels per 8 k-steps (F16: one; F32 as split bf16: three), `spare` panels of
// look-ahead on the weight side
bool dense_panels_fit32(uint64_t Kpad, int pieces, int spare, int64_t Mpad, uint64_t Npad) {
    return (Kpad / 8 * pieces + spare) * (uint64_t)Mpad * 16 <= LIM32 && (Kpad / 8 * pieces) * Npad * 16 <= LIM32;
}

void plan_dense(mm_plan &p, int type, int64_t M, int64_t Mpad, int64_t K, int64_t N) {
    // BF16 (GGML_HIP_TYPE_BF16) is planned as F16 is -- the same families, forms and bounds on the bf16 twins of its kernels (the same bytes,
    // the same MFMA rate) -- under arithmetic labels of its own (F16's + 50), so no tree_id of F16 is one of BF16's.  Its bounds are F16's,
    // unchanged: DESIGN.md row B has the measurement.
    const bool bf = type == GGML_HIP_TYPE_BF16, f16 = type == GGML_TYPE_F16 || bf;
    const int bfa = bf ? 50 : 0;
    const uint64_t Kpad = (uint64_t)dense16_kpad(K), Npad = (uint64_t)pad_act(N);
    p.image = -1;
    // F16, more than 4 src1 rows: the f16 matrix cores (by N alone; K % 4: the INIT kernel reads src1 rows in 16-byte pieces, and a
    // contiguous row is K floats -- r4: the choice no longer depends on whether the CALLER brought a work buffer or an aligned src1:
    // ggml_hip_mul_mat_dev reports those as errors)
    if (f16 && N > 4 && K % 4 == 0) {
        if (!dense_panels_fit32(Kpad, 1, DENSE16_SPARE_PANELS, Mpad, Npad)) {
            p.flags |= MM_FLAG_WIDE;
        } else {
            const int64_t nst = (int64_t)Kpad / (16 * 8);
            const int64_t tm128 = cdiv(M, 128), tn128 = cdiv(N, 128);
            p.family = MMF_DENSE16; p.image = 32; p.flags |= MM_FLAG_NEEDS_WORK;
            p.kunit = 8;
            auto take = [&](int f, int tm, int tn, int waves, int ks, int shape16) {
                p.form = f; p.tile_m = tm; p.tile_n = tn; p.waves = waves; p.ksplit = ks; p.kstyle = ks > 1 ? MMK_STAGE_SETS : MMK_CHAIN;
                p.arith = 700 + bfa + shape16; p.wgs = cdiv(M, tm) * cdiv(N, tn);
                p.tiles_per_wave = tm * tn / 1024 * ks / waves > 0 ? tm * tn / 1024 * ks / waves : 1;
            };
            if (N > 512)   // (v_mfma_f32_16x16x32_f16, by N alone: the two tile sizes sum alike)
                return cdiv(M, 256) * tn128 >= 384 ? take(D16F_S_256x128, 256, 128, 4, 1, 1) : take(D16F_S_128x128, 128, 128, 4, 1, 1);
            // the four-way split up to 128 rows: PLAN_BOUNDS.md "D16F_S4"
            if (N <= 128 && nst >= 8)
                return tm128 * cdiv(N, 64) >= 80 ? take(D16F_S4_H128, 128, 64, 16, 4, 0) : take(D16F_S4_H32, 32, 64, 4, 4, 0);
            if (N <= 512 && nst >= 4) {
                // from 257 tiles on the two-pass form: the 8-wave form holds one workgroup per CU.  PLAN_BOUNDS.md "D16F_V2_128x128"
                if (tm128 * tn128 > 256) return take(D16F_V2_128x128, 128, 128, 4, 2, 0);
                if (tm128 * tn128 >= 160) return take(D16F_S2_128x128, 128, 128, 8, 2, 0);
                return take(D16F_S2_128x64, 128, 64, 8, 2, 0);
            }
            return take(D16F_128x128, 128, 128, 4, 1, 0);
        }
    }
    // F32 above 256 src1 rows: the bf16 cores, every operand split exactly into three bf16 pieces (K10d).  By N alone.
    if (!f16 && N > 256 && K % 4 == 0) {
        if (!dense_panels_fit32(Kpad, 3, DENSE32_SPARE_PANELS, Mpad, Npad)) {
            p.flags |= MM_FLAG_WIDE;
        } else {
            p.family = MMF_DENSE32; p.image = 33; p.form = 0; p.flags |= MM_FLAG_NEEDS_WORK;
            p.arith = 710; p.ksplit = 1; p.kstyle = MMK_CHAIN; p.kunit = 1;
            p.tile_m = p.tile_n = 128; p.waves = 4; p.tiles_per_wave = 16; p.wgs = cdiv(M, 128) * cdiv(N, 128);
            return;
        }
    }
    // r4: F32 weights, 5 .. 256 src1 rows, K a multiple of 256 from 1024 on: 32 x 32 tiles with K split over the workgroup's eight waves
    // (dense.hip dense_f32_ksplit_kernel: the tile kernels run a flat 120 us at 4096 x 4096 whatever N is).  By N and K alone.
    if (!f16 && N >= 5 && N <= 256 && K % 256 == 0 && K >= 1024) {
        p.family = MMF_DENSE; p.form = DNF_KSPLIT;
        p.arith = 740; p.ksplit = 8; p.kstyle = MMK_RANGES; p.kunit = (int)(K / 256);
        p.tile_m = p.tile_n = 32; p.waves = 8; p.tiles_per_wave = 1; p.wgs = cdiv(M, 32) * cdiv(N, 32);
        return;
    }
    // dense.hip.  Mat-vec form up to 16 rows (passes of 8 columns; rows of the resident copy are K elements apart: 16-byte pieces need
    // K % 8 (f16) / K % 4 (f32)); else the 64 x 64 tile kernel (F32: 128 x 128 tiles where they fill the chip -- bitwise the same result)
    if (N <= 16 && K % (f16 ? 8 : 4) == 0 && K >= 512) {
        p.family = MMF_DENSE_GEMV; p.form = 8;
        p.arith = 720 + bfa + (f16 ? 1 : 0); p.ksplit = 64; p.kstyle = MMK_WORKERS; p.kunit = 1;
        p.tile_m = 4; p.tile_n = 8; p.waves = 4; p.tiles_per_wave = 1; p.wgs = cdiv(M, 16);
        return;
    }
    const int64_t tm = cdiv(M, 128), tn = cdiv(N, 128);
    const bool bigt = !f16 && K % 32 == 0 && tm * tn >= 256 && tm * tn < (1 << 30) && Mpad % 128 == 0;
    p.family = MMF_DENSE; p.form = bigt ? DNF_BIG : DNF_TILE;
    p.arith = 730 + bfa + (f16 ? 1 : 0); p.ksplit = 1; p.kstyle = MMK_CHAIN; p.kunit = 32;
    p.tile_m = p.tile_n = bigt ? 128 : 64; p.waves = 4; p.tiles_per_wave = 1; p.wgs = cdiv(M, p.tile_m) * cdiv(N, p.tile_n);
}

mm_plan plan_product(int type, int ext_type, int64_t M, int64_t K, int64_t N, bool one_call) {
    mm_plan p = {};
    p.ksplit = 1;
    const int64_t Mpad = pad_rows(M > 0 ? M : 1);
    if (type == GGML_TYPE_F32 || type == GGML_TYPE_F16 || type == GGML_HIP_TYPE_BF16) { plan_dense(p, type, M, Mpad, K, N); return p; }
    if (!is_quant(type) || K <= 0 || K % QK != 0) return p;
    if (ext_type != 0) p.flags |= MM_FLAG_Q8K;
    const plan_row &r = row_of(type);
    // a form that reads K1's image (INIT first); the fused epilogues are for the reference's own types
    auto with_init = [&]() { p.flags |= MM_FLAG_NEEDS_WORK; if (ext_type != 0) p.flags &= ~MM_FLAG_EPILOGUE_FUSED; return p; };
    // the stated exception: planes that do not fit 32-bit buffer offsets (> 4 GiB per plane) are served by the int8 family and its image,
    // whatever the type.  INIT and COMPUTE both come through here, so they agree.
    const bool wide = !weight_planes_fit32(K, Mpad);
    const int image = wide ? 0 : staged_image(r, K, N);
    // the stage-free pair first, K3p ahead of K3s where both serve and its grid is large enough.  The int8 pair is tried behind `wide` too:
    // its bound is the forms' own (with the generic one a matrix just under the limit fell to the staged int8 kernel while its row shards
    // ran K3p).
    const k3_choice c = k3_stage_free(r, ext_type, image, M, K, N);
    if (c.k3p && c.k3p_first && plan_k3p(p, r, c.mx, M, Mpad, K, N)) return with_init();
    if (c.k3s && plan_k3s(p, r, c.mx, M, Mpad, K, N)) return with_init();
    if (c.k3p && !c.k3p_first && plan_k3p(p, r, c.mx, M, Mpad, K, N)) return with_init();
    // the two-step forms.  An int8 pair that refused (its planes are beyond the forms' offsets) leaves the int8 family, as `wide` does --
    // and no fused mat-vec where K3s would have served: INIT's image is decided at M = 1, where K3s does serve.
    const bool refused = !c.mx && (c.k3s || c.k3p);
    if (wide || refused) p.flags |= MM_FLAG_WIDE;
    if (image == 0 || refused) {
        const bool fused_ok = (ext_type == 0 || kq_fused_serves(r, K, N)) && !(refused && c.k3s);
        if (one_call && N <= GEMV_MAX_N && fused_ok) { plan_gemv(p, M, K, N, true); return p; }
        p.flags |= MM_FLAG_NEEDS_WORK;
        if (N <= (r.two_scale && ext_type != 0 ? 4 : r.gemv_rows)) { plan_gemv(p, M, K, N, false); return p; }
        plan_i8(p, type, M, N);
        return p;
    }
    if (image == 3) plan_mx(p, r, type, M, K, N);
    else plan_f16(p, r, type, M, K, N);
    return with_init();
}

}  // namespace

mm_plan plan_mul_mat(int type, int ext_type, int64_t M, int64_t K, int64_t N, bool one_call) {
    // Q2_K: the block term is a Q6_K product, planned as Q6_K's COMPUTE-only entry is (the fused mat-vec never: the min pass reads K1's image),
    // and the min pass behind it (kquants.hip; its bits follow (K, N) alone, so tree_id keeps its promise with the flag mixed in)
    if (!kquant_min_pass(ext_type)) return plan_product(type, ext_type, M, K, N, one_call);
    mm_plan p = plan_product(type, ext_type, M, K, N, false);
    if (p.family != MMF_NONE) p.flags |= MM_FLAG_MIN_PASS;
    return p;
}

uint32_t plan_tree_id(const mm_plan &p) {
    // what fixes an element's bits, and nothing of the geometry
    uint32_t h = 2166136261u;
    const int parts[] = {p.arith, p.ksplit, p.kstyle, p.kunit, p.flags & MM_FLAG_Q8K};
    for (int v : parts) { h ^= (uint32_t)v; h *= 16777619u; }
    if (p.flags & MM_FLAG_MIN_PASS) { h ^= (uint32_t)MM_FLAG_MIN_PASS; h *= 16777619u; }   // (only when set: every other tree_id keeps its value)
    return h;
}

// The slots of a K3s launch (gemm_qmx.hip launch_small, gemm_q8s.hip launch_q8_small and the grouped launches); the launchers map them to
// an instantiation.
k3s_slots plan_k3s_slots(const mm_plan &p, int type) {
    const int nloc = p.nloc, wmt = p.wmt;
    const bool q41 = row_of(type).min_term;                 // (of the MX pair's two types, the one with a min term)
    k3s_slots s;
    if (p.family == MMF_K3S_MX && p.tile_m == 16) {
        // pairs in flight per wave; beyond 16 k-blocks per wave: in turn (Q4_1 carries the min and d1 * sum(a) per slot: eight slots of two slices spill)
        const int np = nloc <= 8 ? 4 : 8;
        s.rot = nloc > 2 * np;
        s.slots = s.rot && q41 && p.tile_n == 32 ? 6 : np;
        s.rows = s.rot ? nloc : 2 * np;
    } else if (p.family == MMF_K3S_MX) {
        // pairs in flight: a wave's whole range for K <= 4096 (8 pairs) and K <= 2048 (4 pairs), longer K refills them in turn; two tiles per
        // workgroup 4 pairs, three or four tiles 2 (Q4_1 carries three more registers per pair: 3 / 4 in turn)
        s.rot = wmt >= 3 || nloc > (wmt == 2 ? 8 : 16);
        s.slots = wmt >= 3 ? 2 : wmt == 2 ? (s.rot && q41 ? 3 : 4) : nloc <= 8 ? 4 : s.rot && q41 ? 4 : 8;
        s.rows = nloc <= 8 ? 8 : nloc <= 16 ? 16 : nloc;
    } else {
        // int8: one tile per workgroup (and the 16-row tiles) a wave's range in 8 / 16 slots, longer K in rounds of 16; two tiles 8 slots, in
        // rounds beyond K = 2048; three or four tiles four slots in turn.  Table rows: whole rounds of the slots.
        s.slots = wmt >= 3 ? 4 : wmt == 2 || nloc <= 8 ? 8 : 16;
        s.rot = nloc > s.slots;
        s.rows = (int)cdiv(nloc, s.slots) * s.slots;
    }
    const int tab = KS8 * s.rows * p.tile_n * 4, xch = KS8 * p.tile_m * p.tile_n * 4;   // (the exchange: every wave's partial tile)
    s.lds = tab > xch ? tab : xch;
    return s;
}

// Grouped K3s: a workgroup picks its matrix from its index and runs the single-matrix kernel on it.  The rules of the single form, for the
// group's shape; then a group is planned only where every member's own COMPUTE plan has the group's tree, so each member gets its own call's bits.
mm_plan plan_mul_mat_group(int type, int ext_type, const int64_t *M, const int64_t *Mpad, int n, int64_t K, int64_t N) {
    const mm_plan none = {};
    const plan_row &r = row_of(type);
    const bool mx = r.mx;
    if (n < 2 || n > 4 || N < 5 || N > 64 || ext_type != 0 || !(mx || type == GGML_TYPE_Q8_0) || K <= 0 || K % QK != 0) return none;
    const int64_t Npad = pad_act(N);
    const int nloc = k3_nloc(K);                            // (the single-matrix forms' ranges)
    const int64_t ncol = cdiv(N, 32);                       // 32-column slices of src1
    if (nloc > 128 || Npad < 32 * ncol || (mx && K / QK < 64) || !k3s_act_fits32(mx, K, Npad)) return none;
    int64_t t32 = 0;
    for (int i = 0; i < n; ++i) {
        if (M[i] <= 0) return none;
        t32 += cdiv(M[i], 32) * ncol;
    }
    // THREE tiles per workgroup where that is the fewest that keeps the group inside one round of the chip: geometry on the form's tree, like
    // the other tile counts.  A 96-row tile may overhang the padded rows: it reads the neighbouring plane's bytes there (inside the buffer, or
    // zeros past it) and stores nothing.  PLAN_BOUNDS.md "Three tiles per workgroup of a group"
    auto groups = [&](int t) { int64_t g = 0; for (int i = 0; i < n; ++i) g += cdiv(M[i], 32 * t) * ncol; return g; };
    int wmt = k3s_wmt(r, t32);
    if (wmt == 4 && groups(3) <= 256) wmt = 3;
    mm_plan g = none;
    set_k3s(g, r, mx, nloc, wmt);
    const uint32_t tree = plan_tree_id(g);
    for (int i = 0; i < n; ++i) {
        if (!k3s_weights_fit32(mx, K, Mpad[i]) || Mpad[i] % (wmt == 3 ? 32 : 32 * wmt) != 0) return none;
        const mm_plan own = plan_mul_mat(type, ext_type, M[i], K, N, false);
        // (Q8_0: the group runs where the first matrix's own plan is K3s, not K3p)
        if (plan_tree_id(own) != tree || (!mx && i == 0 && own.family != MMF_K3S_I8)) return none;
        g.wgs += cdiv(M[i], 32 * wmt) * ncol;
    }
    return g;
}

// The grouped, device-routed product (plan.h has the bounds).  One decision: the family and tree of the single product at 32 src1 rows, on
// 32-row weight tiles -- two or four of them per workgroup once the BOUND of tile groups passes 256 / 512, the single forms' rule (every
// workgroup pulls its 32 activation columns through its CU's memory path once per launch, whatever the number of weight tiles behind them).
bool plan_mul_mat_id_grouped_serves(int type, int ext_type, int64_t M, int64_t K) {
    if (ext_type != 0 || !(type == GGML_TYPE_Q8_0 || type == GGML_TYPE_Q5_0 || type == GGML_TYPE_Q4_0) || M <= 0 || K <= 0 || K % QK != 0) return false;
    const int f = plan_mul_mat(type, 0, M, K, 32, true).family;
    return f == MMF_K3S_I8 || f == MMF_K3S_MX;
}

mm_plan plan_mul_mat_id_grouped(int type, int ext_type, int64_t M, int64_t K, int n_expert, int64_t P) {
    const mm_plan none = {};
    if (P < 1 || P > MOE_GROUPED_MAX_PAIRS || n_expert < 1 || !plan_mul_mat_id_grouped_serves(type, ext_type, M, K)) return none;
    const mm_plan one = plan_mul_mat(type, 0, M, K, 32, true);
    const plan_row &r = row_of(type);
    const bool mx = one.family == MMF_K3S_MX;
    const int64_t tiles = moe_grouped_tiles(n_expert, P);
    if (!k3s_act_fits32(mx, K, pad_act(32 * tiles))) return none;
    const int wmt = k3s_wmt(r, cdiv(M, 32) * tiles);
    mm_plan g = none;
    set_k3s(g, r, mx, one.nloc, wmt);                       // (the tree of the single product)
    g.form = 8; g.flags = one.flags & MM_FLAG_NEEDS_WORK;
    g.wgs = cdiv(M, 32 * wmt) * tiles;
    if (g.wgs > 0x7FFFFFFF || plan_k3s_slots(g, type).lds > 160 * 1024) return none;
    return g;
}

// Attention over a KV cache (attn.hip).  One decision: n_q <= ATTN_DECODE_MAX_Q is the split-KV DECODE form, everything above the
// matrix-core PROMPT form; the chunk is ATTN_CHUNK for every served (kv_type, D).  What is served: F16 / Q8_0, D 64 / 128, G in 1 .. 16.
attn_plan plan_attn(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max) {
    attn_plan p = {};
    if (!(kv_type == GGML_TYPE_F16 || kv_type == GGML_TYPE_Q8_0) || !(D == 64 || D == 128)) return p;
    if (n_head < 1 || n_head_kv < 1 || n_head % n_head_kv != 0 || n_head / n_head_kv > 16 || n_head > 65535) return p;
    if (n_q < 1 || n_q > (1 << 20) || n_kv_max < 0 || n_kv_max > (1 << 24) || n_q * n_head > 0x7FFFFFFF) return p;
    p.chunk = ATTN_CHUNK;
    p.n_chunks = cdiv(n_kv_max, ATTN_CHUNK);
    if (n_q <= ATTN_DECODE_MAX_Q) {
        p.form = ATTN_FORM_DECODE; p.q_tile = (int)(n_q * (n_head / n_head_kv)); p.launches = 2;
        p.wgs = p.n_chunks * n_head_kv;
        p.work_bytes = (size_t)n_q * (size_t)n_head * (size_t)p.n_chunks * (size_t)(D + 4) * 4;
    } else {
        p.form = ATTN_FORM_PROMPT; p.q_tile = 128; p.launches = 1;
        p.wgs = cdiv(n_q, 128) * n_head;
        p.work_bytes = 0;
    }
    return p;
}

// The paged call: plan_attn's decision per sequence, every grid n_seq deep (DECODE: chunks x kv heads x sequences, its merge one workgroup
// per row of all sequences; PROMPT: query tiles x heads x sequences).
attn_plan plan_attn_paged(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max) {
    attn_plan p = plan_attn(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE) return p;
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ || n_seq * n_q > ATTN_PAGED_MAX_ROWS || n_seq * n_q * n_head > 0x7FFFFFFF) return attn_plan{};
    p.wgs *= n_seq;
    p.work_bytes *= (size_t)n_seq;
    return p;
}

// The _ex calls: the base decision; a windowed DECODE grid follows the window instead of n_kv_max (plan.h has the bound).
attn_plan plan_attn_ex(int kv_type, int D, int n_head, int n_head_kv, int64_t n_q, int64_t n_kv_max, int64_t window) {
    attn_plan p = plan_attn(kv_type, D, n_head, n_head_kv, n_q, n_kv_max);
    if (p.form != ATTN_FORM_DECODE || window <= 0 || window >= n_kv_max) return p;
    const int64_t n = cdiv(window + n_q - 1, ATTN_CHUNK) + 1;
    if (n < p.n_chunks) { p.n_chunks = n; p.wgs = n * n_head_kv; }
    return p;
}

attn_plan plan_attn_paged_ex(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_q, int64_t n_kv_max, int64_t window) {
    attn_plan p = plan_attn_paged(kv_type, D, n_head, n_head_kv, n_seq, n_q, n_kv_max);
    if (p.form == ATTN_FORM_NONE) return p;
    const attn_plan one = plan_attn_ex(kv_type, D, n_head, n_head_kv, n_q, n_kv_max, window);
    p.n_chunks = one.n_chunks; p.wgs = one.wgs * n_seq;
    return p;
}

// MLA (plan.h has the statement): the form from n_q alone, the grids from the shape alone.
mla_plan plan_attn_mla(int kv_type, int n_head, int64_t n_seq, int64_t n_q, int64_t n_kv_max) {
    mla_plan p = {};
    if (!(kv_type == GGML_TYPE_F16 || kv_type == GGML_TYPE_Q8_0) || n_head < 1 || n_head > 256) return p;
    if (n_q < 1 || n_q > (1 << 20) || n_kv_max < 0 || n_kv_max > (1 << 24)) return p;
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ || n_seq * n_q > ATTN_PAGED_MAX_ROWS || n_seq * n_q * n_head > 0x7FFFFFFF) return p;
    p.chunk = ATTN_CHUNK; p.span = MLA_SPAN; p.q_tile = MLA_TILE; p.step = MLA_STEP;
    p.n_spans = cdiv(n_kv_max, (int64_t)ATTN_CHUNK * MLA_SPAN);
    p.tiles = cdiv(n_q * n_head, MLA_TILE);
    if (n_q <= MLA_SPLIT_MAX_Q) {
        p.form = MLA_FORM_SPLIT; p.launches = 2;
        p.wgs = p.tiles * p.n_spans * n_seq;
        p.merge_wgs = n_seq * n_q * n_head;
        p.work_bytes = (size_t)p.merge_wgs * (size_t)p.n_spans * (size_t)(MLA_DV + 4) * 4;
    } else {
        p.form = MLA_FORM_WALK; p.launches = 1;
        p.wgs = p.tiles * n_seq;
    }
    return p;
}

// The ragged paged call (plan.h has the statement): the bounds size everything, the batch nothing.
int64_t attn_ragged_max_tiles(int64_t n_tokens_max, int64_t n_seq) {
    if (n_tokens_max < 9 || n_seq < 1) return 0;
    const int64_t P = n_seq < n_tokens_max / 9 ? n_seq : n_tokens_max / 9, L = n_tokens_max - 9 * P;
    const int64_t k = P < L / 120 ? P : L / 120;
    return P + k + (L - 120 * k) / 128;
}

attn_ragged_plan plan_attn_ragged(int kv_type, int D, int n_head, int n_head_kv, int64_t n_seq, int64_t n_tokens_max, int64_t n_dec_rows_max, int64_t n_kv_max,
                                  int64_t window) {
    attn_ragged_plan p = {};
    if (n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ || n_tokens_max < 0 || n_tokens_max > ATTN_PAGED_MAX_ROWS || n_dec_rows_max < 0 || n_dec_rows_max > n_tokens_max) return p;
    const attn_plan one = plan_attn_ex(kv_type, D, n_head, n_head_kv, ATTN_DECODE_MAX_Q, n_kv_max, window);    // (the served types, D and heads; the chunks at 8 rows)
    if (one.form == ATTN_FORM_NONE || n_tokens_max * n_head > 0x7FFFFFFF) return p;
    p.ok = 1;
    p.chunk = ATTN_CHUNK;
    if (n_tokens_max == 0) return p;
    p.dec_rows = n_dec_rows_max;
    p.n_chunks = one.n_chunks;
    p.max_tiles = attn_ragged_max_tiles(n_tokens_max, n_seq);
    p.decode_wgs = n_dec_rows_max > 0 ? p.n_chunks * n_head_kv * n_seq : 0;      // (no row slot: every DECODE workgroup would leave)
    p.merge_wgs = n_dec_rows_max * n_head;
    p.prompt_wgs = p.max_tiles * n_head;
    p.launches = 1 + (p.decode_wgs > 0) + (p.merge_wgs > 0) + (p.prompt_wgs > 0);
    p.seq_off = 0;
    p.n_tiles_off = 16 * (size_t)n_seq;
    p.tiles_off = p.n_tiles_off + 16;
    p.slots_off = p.tiles_off + 8 * (size_t)p.max_tiles;
    p.part_off = (p.slots_off + 8 * (size_t)n_dec_rows_max + 255) / 256 * 256;
    p.work_bytes = p.part_off + (size_t)n_dec_rows_max * (size_t)n_head * (size_t)cdiv(n_kv_max, ATTN_CHUNK) * (size_t)(D + 4) * 4;
    return p;
}

// The SSM entries (plan.h has the statement): one launch each, a workgroup row per sequence, sized by the shape and n_seq alone.
ssm_conv_plan plan_ssm_conv(int64_t n_ch, int d_conv, int64_t n_seq) {
    ssm_conv_plan p = {};
    if (n_ch < 1 || n_ch > SSM_MAX_CHANNELS || d_conv < 2 || d_conv > 4 || n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return p;
    p.ok = 1;
    p.launches = 1;
    p.state_bytes = (size_t)(d_conv - 1) * (size_t)n_ch * 4;
    p.wgs_x = cdiv(n_ch, 256);
    p.wgs = p.wgs_x * n_seq;
    return p;
}

ssm_scan_plan plan_ssm_scan(int n_head, int P, int N, int n_group, int64_t n_seq) {
    ssm_scan_plan p = {};
    if (n_head < 1 || n_head > SSM_MAX_HEADS || P < 1 || P > 256 || N < 16 || N > 256 || N % 16 != 0) return p;
    if (n_group < 1 || n_head % n_group != 0 || n_seq < 1 || n_seq > ATTN_PAGED_MAX_SEQ) return p;
    p.ok = 1;
    p.form = SSM_FORM_SEQUENTIAL;
    p.launches = 1;
    p.slices = N / 16;
    p.lanes_per_row = 1;
    while (p.lanes_per_row < p.slices) p.lanes_per_row *= 2;
    p.rows_per_wg = 256 / p.lanes_per_row;
    p.state_bytes = (size_t)n_head * (size_t)P * (size_t)N * 4;
    p.wgs_x = cdiv((int64_t)n_head * P, p.rows_per_wg);
    p.wgs = p.wgs_x * n_seq;
    return p;
}

// The chunked scan (plan.h has the statement): the sequential plan for the short sequences, the bounds of the chunk list for the long ones.
ssm_chunk_plan plan_ssm_chunk(int n_head, int P, int N, int n_group, int a_per_state, int64_t n_seq, int64_t n_tokens_max) {
    ssm_chunk_plan p = {};
    p.seq = plan_ssm_scan(n_head, P, N, n_group, n_seq);
    if (!p.seq.ok || (a_per_state != 0 && a_per_state != 1) || n_tokens_max < 0 || n_tokens_max > ATTN_PAGED_MAX_ROWS) return p;
    p.ok = 1;
    p.form = SSM_FORM_SEQUENTIAL;
    p.chunk = SSM_CHUNK;
    p.seq_max_tokens = SSM_CHUNK_SEQ_MAX_TOKENS;
    p.launches = 1;
    if (a_per_state || P % 16 != 0 || n_tokens_max <= p.seq_max_tokens) return p;
    p.form = SSM_FORM_CHUNKED;
    p.launches = 5;
    p.p_tile = P % 64 == 0 ? 64 : P % 32 == 0 ? 32 : 16;
    p.p_tiles = P / p.p_tile;
    p.kernel_state = p.kernel_out = p.p_tile;
    p.seqs_max = n_tokens_max / (p.seq_max_tokens + 1) < n_seq ? n_tokens_max / (p.seq_max_tokens + 1) : n_seq;
    p.chunks_max = p.seqs_max + (n_tokens_max - p.seqs_max) / SSM_CHUNK;
    p.pass_wgs_x = cdiv((int64_t)n_head * P * N / 4, 256);
    const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    p.hdr_off = 0;
    p.seqs_off = 256;
    p.list_off = p.seqs_off + up(16 * (size_t)p.seqs_max);
    p.csd_off = p.list_off + up(8 * (size_t)p.chunks_max);
    p.state_off = p.csd_off + up((size_t)p.chunks_max * (size_t)n_head * 2 * SSM_CHUNK * 4);
    p.work_bytes = p.state_off + up((size_t)p.chunks_max * (size_t)n_head * (size_t)P * (size_t)N * 4);
    return p;
}

// The tiled conv (plan.h has the statement): the sequential plan for the short sequences, the bounds of the tile list for the long ones.
// tile and seq_max_tokens are measured constants: docs/PLAN_BOUNDS.md "SSM_CONV_TILE"
ssm_conv_tiled_plan plan_ssm_conv_tiled(int64_t n_ch, int d_conv, int64_t n_seq, int64_t n_tokens_max) {
    ssm_conv_tiled_plan p = {};
    p.seq = plan_ssm_conv(n_ch, d_conv, n_seq);
    if (!p.seq.ok || n_tokens_max < 0 || n_tokens_max > ATTN_PAGED_MAX_ROWS) return p;
    p.ok = 1;
    p.form = SSM_FORM_SEQUENTIAL;
    p.tile = SSM_CONV_TILE;
    p.seq_max_tokens = SSM_CONV_SEQ_MAX_TOKENS;
    p.launches = 1;
    p.vec = n_ch % 4 == 0 ? 4 : 1;
    if (n_tokens_max <= p.seq_max_tokens) return p;
    p.form = SSM_FORM_TILED;
    p.launches = 4;
    p.seqs_max = n_tokens_max / (p.seq_max_tokens + 1) < n_seq ? n_tokens_max / (p.seq_max_tokens + 1) : n_seq;
    p.tiles_max = p.seqs_max + (n_tokens_max - p.seqs_max) / SSM_CONV_TILE;
    p.halo_ld = (n_ch + 3) / 4 * 4;
    const auto up = [](size_t v) { return (v + 255) / 256 * 256; };
    p.hdr_off = 0;
    p.list_off = 256;
    p.halo_off = p.list_off + up(8 * (size_t)p.tiles_max);
    p.work_bytes = p.halo_off + up((size_t)p.tiles_max * (size_t)(d_conv - 1) * (size_t)p.halo_ld * 4);
    return p;
}
