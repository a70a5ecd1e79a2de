// ssm.hip -- the two recurrent ops of a Mamba / Mamba-2 block over a ragged batch and a pool of per-sequence state slots (include/ggml_hip_ext.h, SSM;
// the entries and every check are ssm.cpp's, every grid is plan.h's plan_ssm_conv / plan_ssm_scan).
//
// Both kernels give a SEQUENCE to a workgroup row (blockIdx.y = b), so the token loop's trip count is uniform over the workgroup, and every guard comes
// before the address it protects: the sequence is present (0 <= q_start[b] <= q_start[b+1] <= n_tokens_max) and not idle, the slot id lies inside
// [0, n_slots).  A state element is read at most once (not at all where len[b] == 0) and written once, by the lane that owns it; nothing is shared
// between workgroups, no atomics.
//
//   ssm_conv_kernel<KC>   one thread per (sequence, channel); the window of KC - 1 rows rides in registers over the sequence's tokens.  The loads of up
//                         to CONV_UNROLL tokens are issued together (they depend on nothing the loop computes); in place (dst == x) is safe because a
//                         thread reads x[t][c] before it writes dst[t][c] and no other thread touches channel c of this sequence.  Sequences of more
//                         than nq_max tokens belong to the tiled form (ssm_conv_tile.hip) and leave by whole workgroups; INT_MAX: none.
//   ssm_scan_kernel<LP, APS, FULL>  one lane per (sequence, head, p, slice of 16 states); a state row of N = 16 L elements rides in the registers of L lanes
//                         inside an aligned group of LP = the next power of two (lanes L .. LP - 1 of a group idle with a partial of +0.0f), and y meets
//                         in the xor butterfly the header states: DPP moves inside a row of 16 lanes, no LDS.
//                         FULL (N == 16 LP: no idle lanes, so lane i of the sequence owns the 64 bytes at 64 i of its slot): the state moves in whole
//                         lines -- the four lanes of a quad load the 256 bytes of their four slices 16 bytes each per instruction and a 4 x 4
//                         transpose over the quad (DPP) hands every lane its slice; the same on the way back.  Each lane reading its own 64 bytes
//                         (the plain path, kept for N = 48, 80, ..) touches a quarter of every line per instruction: 0.57 against 0.63 of the
//                         roof on a 256-sequence decode step (tools/ssm_grid.py).
#include "common.h"
#include "plan.h"

namespace {

constexpr int CONV_UNROLL = 8;

template <int KC>
__global__ __launch_bounds__(256) void ssm_conv_kernel(const kv_ragged rg, const int32_t *__restrict__ len, const int32_t *__restrict__ slot, int n_slots,
                                                       const float *x, int64_t ldx, const float *__restrict__ w, const float *__restrict__ bias, int act,
                                                       int64_t n_ch, float *state, int64_t slot_elems, float *dst, int64_t ldd, int nq_max) {
    const int b = blockIdx.y;
    const int64_t c = (int64_t)blockIdx.x * 256 + threadIdx.x;
    int64_t qs; int nq;
    if (!ssm_sequence(rg, b, &qs, &nq) || nq == 0 || nq > nq_max || c >= n_ch) return;   // (nq_max: uniform over the workgroup, as the scan's)
    const int sl = slot[b];
    if (sl < 0 || sl >= n_slots) {
        for (int t = 0; t < nq; ++t) dst[(qs + t) * ldd + c] = 0.0f;
        return;
    }
    float *st = state + (int64_t)sl * slot_elems + c;
    float wk[KC], win[KC];
#pragma unroll
    for (int k = 0; k < KC; ++k) wk[k] = w[c * KC + k];
    const bool fresh = len[b] == 0;
#pragma unroll
    for (int k = 0; k < KC - 1; ++k) win[k] = fresh ? 0.0f : st[k * n_ch];
    const float bv = bias ? bias[c] : 0.0f;
    for (int t0 = 0; t0 < nq; t0 += CONV_UNROLL) {
        float xv[CONV_UNROLL];
#pragma unroll
        for (int u = 0; u < CONV_UNROLL; ++u) xv[u] = t0 + u < nq ? x[(qs + t0 + u) * ldx + c] : 0.0f;
#pragma unroll
        for (int u = 0; u < CONV_UNROLL; ++u) {
            if (t0 + u < nq) {
                win[KC - 1] = xv[u];
                float acc = wk[0] * win[0];
#pragma unroll
                for (int k = 1; k < KC; ++k) acc = fmaf(wk[k], win[k], acc);
                if (bias) acc = acc + bv;
                if (act) acc = acc / (1.0f + expf(-acc));
                dst[(qs + t0 + u) * ldd + c] = acc;
#pragma unroll
                for (int k = 0; k < KC - 1; ++k) win[k] = win[k + 1];
            }
        }
    }
#pragma unroll
    for (int k = 0; k < KC - 1; ++k) st[k * n_ch] = win[k];
}

struct scan_args {
    const float *x; int64_t ldx_tok, ldx_head;
    const float *dt; int64_t ld_dt; const float *dt_bias;
    const float *A; int64_t a_ld;
    const float *B, *C; int64_t ld_bc;
    const float *D;
    int n_head, P, N, heads_per_group;
    const int32_t *len, *slot; int n_slots;
    float *state; int64_t slot_elems;
    float *dst; int64_t ldd_tok, ldd_head;
    int nq_max;                                                      // sequences above it belong to the chunked form (ssm_chunk.hip); INT_MAX: none
};

// the 4 x 4 transpose of v[0 .. 3] over the four lanes of a quad (r = lane & 3): lane r ends with what lane k held in v[r], k = 0 .. 3.  Two
// butterfly steps; every lane of the quad must be here
__device__ __forceinline__ void quad_transpose(float (&v)[4], int r) {
    const bool b0 = (r & 1) != 0, b1 = (r & 2) != 0;
    const float g0 = dpp_f<DPP_XOR1>(b0 ? v[0] : v[1]), g1 = dpp_f<DPP_XOR1>(b0 ? v[2] : v[3]);
    v[0] = b0 ? g0 : v[0]; v[1] = b0 ? v[1] : g0; v[2] = b0 ? g1 : v[2]; v[3] = b0 ? v[3] : g1;
    const float g2 = dpp_f<DPP_XOR2>(b1 ? v[0] : v[2]), g3 = dpp_f<DPP_XOR2>(b1 ? v[1] : v[3]);
    v[0] = b1 ? g2 : v[0]; v[2] = b1 ? v[2] : g2; v[1] = b1 ? g3 : v[1]; v[3] = b1 ? v[3] : g3;
}
__device__ __forceinline__ void quad_transpose16(float (&hs)[16], int r) {          // hs[4 k + c] = component c of register k
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        float v[4] = {hs[c], hs[4 + c], hs[8 + c], hs[12 + c]};
        quad_transpose(v, r);
        hs[c] = v[0]; hs[4 + c] = v[1]; hs[8 + c] = v[2]; hs[12 + c] = v[3];
    }
}

// LP: lanes of a state row's group (1, 2, 4, 8, 16); APS: A is per state ([n_head][N]) instead of per head; FULL: N == 16 LP (the state moves by quads)
template <int LP, bool APS, bool FULL>
__global__ __launch_bounds__(256) void ssm_scan_kernel(const kv_ragged rg, const scan_args a) {
    const int b = blockIdx.y;
    int64_t qs; int nq;
    if (!ssm_sequence(rg, b, &qs, &nq) || nq == 0 || nq > a.nq_max) return;   // (uniform over the workgroup)
    const int64_t lane = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int64_t row = lane / LP;                                       // (head, p)
    const int j = (int)(lane % LP);                                      // the slice: states 16 j .. 16 j + 15
    const bool live = row < (int64_t)a.n_head * a.P && 16 * j < a.N;     // (a whole group is inside or outside the rows: LP divides 256)
    const int h = live ? (int)(row / a.P) : 0, p = live ? (int)(row % a.P) : 0;
    const int sl = a.slot[b];
    if (sl < 0 || sl >= a.n_slots) {                                     // (uniform too)
        if (live && j == 0)
            for (int t = 0; t < nq; ++t) a.dst[(qs + t) * a.ldd_tok + (int64_t)h * a.ldd_head + p] = 0.0f;
        return;
    }
    float4 *st = (float4 *)(a.state + (int64_t)sl * a.slot_elems + ((int64_t)h * a.P + p) * a.N + 16 * j);
    float hs[16];
#pragma unroll
    for (int i = 0; i < 16; ++i) hs[i] = 0.0f;
    // FULL: piece k of this lane is part r of the slice of the quad's lane k -- float4 number 4 (q0 + k) + r of the slot, there if that lane is live
    const int r = (int)(lane & 3);
    const int64_t q0 = lane - r, n_lanes = (int64_t)a.n_head * a.P * LP;
    float4 *sq = (float4 *)(a.state + (int64_t)sl * a.slot_elems) + 4 * q0 + r;
    const bool fresh = a.len[b] == 0;                                    // (uniform)
    if (FULL) {
        if (!fresh) {
#pragma unroll
            for (int k = 0; k < 4; ++k)
                if (q0 + k < n_lanes) { const float4 v = sq[4 * k]; hs[4 * k] = v.x; hs[4 * k + 1] = v.y; hs[4 * k + 2] = v.z; hs[4 * k + 3] = v.w; }
            quad_transpose16(hs, r);
        }
    } else if (live && !fresh) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { const float4 v = st[i]; hs[4 * i] = v.x; hs[4 * i + 1] = v.y; hs[4 * i + 2] = v.z; hs[4 * i + 3] = v.w; }
    }
    float As[APS ? 16 : 1];
    if (APS) {
#pragma unroll
        for (int i = 0; i < 16; ++i) As[i] = live ? a.A[(int64_t)h * a.a_ld + 16 * j + i] : 0.0f;
    } else {
        As[0] = live ? a.A[(int64_t)h * a.a_ld] : 0.0f;
    }
    const float dtb = (live && a.dt_bias) ? a.dt_bias[h] : 0.0f;
    const float Dh = (live && a.D) ? a.D[h] : 0.0f;
    const int64_t bc = (int64_t)(h / a.heads_per_group) * a.N + 16 * j;
    for (int t = 0; t < nq; ++t) {
        const int64_t tok = qs + t;
        float s = 0.0f, xv = 0.0f;
        if (live) {
            xv = a.x[tok * a.ldx_tok + (int64_t)h * a.ldx_head + p];
            float d = a.dt[tok * a.ld_dt + h];
            if (a.dt_bias) d = d + dtb;
            const float delta = d <= 20.0f ? log1pf(expf(d)) : d;
            const float dx = delta * xv;
            const float4 *Bp = (const float4 *)(a.B + tok * a.ld_bc + bc), *Cp = (const float4 *)(a.C + tok * a.ld_bc + bc);
            float Bv[16], Cv[16];
#pragma unroll
            for (int i = 0; i < 4; ++i) {
                const float4 u = Bp[i], v = Cp[i];
                Bv[4 * i] = u.x; Bv[4 * i + 1] = u.y; Bv[4 * i + 2] = u.z; Bv[4 * i + 3] = u.w;
                Cv[4 * i] = v.x; Cv[4 * i + 1] = v.y; Cv[4 * i + 2] = v.z; Cv[4 * i + 3] = v.w;
            }
            float da = 0.0f;
            if (!APS) da = expf(delta * As[0]);
#pragma unroll
            for (int i = 0; i < 16; ++i) {
                if (APS) da = expf(delta * As[i]);
                hs[i] = fmaf(hs[i], da, dx * Bv[i]);
            }
            s = hs[0] * Cv[0];
#pragma unroll
            for (int i = 1; i < 16; ++i) s = fmaf(hs[i], Cv[i], s);
        }
        // the butterfly over the group's LP slices (every lane of the wave is here: the branches above are closed)
        if (LP >= 2) s = s + dpp_f<DPP_XOR1>(s);
        if (LP >= 4) s = s + dpp_f<DPP_XOR2>(s);
        if (LP >= 8) s = s + dpp_f<DPP_HALF_MIRROR>(s);              // (the quads are uniform: the mirror is the swap of xor 4)
        if (LP >= 16) s = s + dpp_f<DPP_ROW_MIRROR>(s);              // (the halves are uniform: the swap of xor 8)
        if (live && j == 0) {
            if (a.D) s = fmaf(Dh, xv, s);
            a.dst[tok * a.ldd_tok + (int64_t)h * a.ldd_head + p] = s;
        }
    }
    if (FULL) {
        quad_transpose16(hs, r);
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (q0 + k < n_lanes) sq[4 * k] = make_float4(hs[4 * k], hs[4 * k + 1], hs[4 * k + 2], hs[4 * k + 3]);
    } else if (live) {
#pragma unroll
        for (int i = 0; i < 4; ++i) st[i] = make_float4(hs[4 * i], hs[4 * i + 1], hs[4 * i + 2], hs[4 * i + 3]);
    }
}

template <int LP, bool FULL>
void scan_launch(bool aps, dim3 grid, hipStream_t st, const kv_ragged &rg, const scan_args &a) {
    if (aps) ssm_scan_kernel<LP, true, FULL><<<grid, 256, 0, st>>>(rg, a);
    else ssm_scan_kernel<LP, false, FULL><<<grid, 256, 0, st>>>(rg, a);
}
template <int LP>
void scan_launch(bool aps, dim3 grid, hipStream_t st, const kv_ragged &rg, const scan_args &a) {
    if (a.N == 16 * LP) scan_launch<LP, true>(aps, grid, st, rg, a);
    else scan_launch<LP, false>(aps, grid, st, rg, a);
}

}  // namespace

hipError_t launch_ssm_conv(const ssm_conv_plan &pl, const kv_ragged &rg, const int32_t *len, const int32_t *slot, int n_slots, const float *x, int64_t ldx,
                           const float *w, const float *bias, int act, int64_t n_ch, int d_conv, float *state, int64_t slot_elems, float *dst, int64_t ldd,
                           int nq_max, hipStream_t st) {
    const dim3 grid((unsigned)pl.wgs_x, (unsigned)rg.n_seq);
    switch (d_conv) {
    case 2: ssm_conv_kernel<2><<<grid, 256, 0, st>>>(rg, len, slot, n_slots, x, ldx, w, bias, act, n_ch, state, slot_elems, dst, ldd, nq_max); break;
    case 3: ssm_conv_kernel<3><<<grid, 256, 0, st>>>(rg, len, slot, n_slots, x, ldx, w, bias, act, n_ch, state, slot_elems, dst, ldd, nq_max); break;
    case 4: ssm_conv_kernel<4><<<grid, 256, 0, st>>>(rg, len, slot, n_slots, x, ldx, w, bias, act, n_ch, state, slot_elems, dst, ldd, nq_max); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

hipError_t launch_ssm_scan(const ssm_scan_plan &pl, const kv_ragged &rg, const ssm_scan_args &s, hipStream_t st) {
    scan_args a;
    a.x = s.x; a.ldx_tok = s.ldx_tok; a.ldx_head = s.ldx_head; a.dt = s.dt; a.ld_dt = s.ld_dt; a.dt_bias = s.dt_bias; a.A = s.A; a.a_ld = s.a_ld;
    a.B = s.B; a.C = s.C; a.ld_bc = s.ld_bc; a.D = s.D; a.n_head = s.n_head; a.P = s.P; a.N = s.N; a.heads_per_group = s.n_head / s.n_group;
    a.len = s.len; a.slot = s.slot; a.n_slots = s.n_slots; a.state = s.state; a.slot_elems = s.slot_elems; a.dst = s.dst; a.ldd_tok = s.ldd_tok;
    a.ldd_head = s.ldd_head; a.nq_max = s.nq_max;
    const dim3 grid((unsigned)pl.wgs_x, (unsigned)rg.n_seq);
    const bool aps = s.a_per_state != 0;
    switch (pl.lanes_per_row) {
    case 1: scan_launch<1>(aps, grid, st, rg, a); break;
    case 2: scan_launch<2>(aps, grid, st, rg, a); break;
    case 4: scan_launch<4>(aps, grid, st, rg, a); break;
    case 8: scan_launch<8>(aps, grid, st, rg, a); break;
    case 16: scan_launch<16>(aps, grid, st, rg, a); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}
