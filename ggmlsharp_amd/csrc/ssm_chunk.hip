// ssm_chunk.hip -- the selective scan of a LONG sequence in chunks of Q = 64 tokens, as matrix products on the f32-input MFMA (SSD; include/ggml_hip_ext.h,
// ggml_hip_ssm_scan_chunked_ragged_dev; the checks are ssm.cpp's, every grid and the work buffer are plan.h's plan_ssm_chunk).  A sequence of at most
// seq_max_tokens tokens stays with ssm.hip's sequential kernel, which the launcher starts first with that window.
//
// Per head, inside a chunk: delta_t and la_t = delta_t * A_h as the sequential statement has them, cs_t the running sum of la (ascending, one addition per
// token), xd_s = delta_s * x_s.  Every decay is ONE expf of a difference of two cs (<= 0), every mask a SELECT: rows past a partial chunk or past the
// sequence are never used -- the load goes to the chunk's first row instead and the operand is +0.0f.
//
//   ssm_chunk_index_kernel      one workgroup: a prefix sum over the sequences' chunk counts -> the chunked sequences and the chunk list (plan.h), clamped
//   ssm_chunk_state_kernel<PT>  per (chunk, head, P tile): wave 0 computes delta and cs (kept for the out kernel); then S[p][n] = sum_s ((xd[s][p] *
//                               expf(cs_last - cs_s)) * B[s][n], s ascending from +0.0f, on v_mfma_f32_16x16x4_f32: a wave owns the 16-column blocks nb, nb + 4,
//                               .. of N and PT / 16 independent accumulators each
//   ssm_chunk_pass_kernel       per (chunked sequence, 4 state elements): h = slot (or zeros); per chunk: S out, h in (the chunk's H_in, in place),
//                               h = fmaf(h, expf(cs_last), S); the slot at the end.  A state element is read at most once and written once in the slot
//   ssm_chunk_out_kernel<PT>    per (chunk, head, P tile), wave w owns rows 16 w .. 16 w + 15: G[t][s] = sum_n C[t][n] B[s][n] for the 16-column blocks at
//                               or below the diagonal, M[t][s] = s <= t ? expf(cs_t - cs_s) * G[t][s] : 0 through LDS into the A layout, then ONE chain
//                               y[t][p] = sum_n (expf(cs_t) * C[t][n]) * H_in[p][n] + sum_{s < 16 (w + 1)} M[t][s] * xd[s][p], and fmaf(D, x, y)
// THE k ORDER of the products over n: an MFMA step takes k = 0 .. 3 from the lane groups 0 .. 3, and a lane group kq loads the four states 16 kb + 4 kq + c as
// one float4, so the chain runs over n = 16 kb + 4 kq + c with kb, then c, then kq ascending.  Over s it is plain ascending.
// A/B operand of the 16x16x4 form: lane l holds A[i = l & 15][k = l >> 4] and B[k = l >> 4][j = l & 15]; C/D: column l & 15, rows 4 (l >> 4) + r.
#include <climits>
#include "common.h"
#include "plan.h"

namespace {

constexpr int Q = SSM_CHUNK;
constexpr int LDM = Q + 4;                                           // a wave's M tile [16][LDM]: the A-layout reads meet every bank once
typedef float f32x4 __attribute__((ext_vector_type(4)));

struct chunk_work {
    int32_t *hdr; int4 *seqs; int2 *list; float *csd; float *hst;
    int chunks_max, seqs_max, seq_max_tokens, p_tiles;
};

__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) { return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0); }

__global__ __launch_bounds__(1024) void ssm_chunk_index_kernel(const kv_ragged rg, const chunk_work w) {
    __shared__ int sc[1024], ss[1024];
    const int tid = threadIdx.x, per = (rg.n_seq + 1023) / 1024;
    int nc = 0, ns = 0;
    for (int i = 0; i < per; ++i) {
        const int b = tid * per + i;
        int64_t qs; int nq;
        if (b < rg.n_seq && ssm_sequence(rg, b, &qs, &nq) && nq > w.seq_max_tokens) { nc += (nq + Q - 1) / Q; ns += 1; }
    }
    sc[tid] = nc; ss[tid] = ns;
    __syncthreads();
    for (int d = 1; d < 1024; d *= 2) {
        const int a = tid >= d ? sc[tid - d] : 0, s = tid >= d ? ss[tid - d] : 0;
        __syncthreads();
        sc[tid] += a; ss[tid] += s;
        __syncthreads();
    }
    int c0 = sc[tid] - nc, s0 = ss[tid] - ns;
    for (int i = 0; i < per; ++i) {
        const int b = tid * per + i;
        int64_t qs; int nq;
        if (b < rg.n_seq && ssm_sequence(rg, b, &qs, &nq) && nq > w.seq_max_tokens) {
            const int n = (nq + Q - 1) / Q;
            const int lo = c0 < w.chunks_max ? c0 : w.chunks_max, hi = c0 + n < w.chunks_max ? c0 + n : w.chunks_max;
            if (s0 < w.seqs_max) w.seqs[s0] = make_int4(b, lo, hi - lo, 0);
            for (int c = lo; c < hi; ++c) w.list[c] = make_int2(b, c - c0);
            c0 += n; s0 += 1;
        }
    }
    if (tid == 1023) {
        w.hdr[0] = sc[1023] < w.chunks_max ? sc[1023] : w.chunks_max;
        w.hdr[1] = ss[1023] < w.seqs_max ? ss[1023] : w.seqs_max;
        w.hdr[2] = 0; w.hdr[3] = 0;
    }
}

// the chunk of workgroup row ci: its sequence, its first packed row and its tokens (1 .. Q); false past the list
__device__ __forceinline__ bool chunk_of(const kv_ragged &rg, const chunk_work &w, int ci, int *b, int64_t *tok0, int *len) {
    if (ci >= w.hdr[0]) return false;
    const int2 e = w.list[ci];
    const int64_t qs = rg.q_start[e.x];
    const int nq = (int)(rg.q_start[e.x + 1] - qs);
    *b = e.x; *tok0 = qs + (int64_t)e.y * Q;
    const int left = nq - e.y * Q;
    *len = left < Q ? left : Q;
    return true;
}

template <int PT>
__global__ __launch_bounds__(256) void ssm_chunk_state_kernel(const kv_ragged rg, const ssm_scan_args a, const chunk_work w) {
    constexpr int LDX = PT == 16 ? 16 : PT + 16;                     // (rows 16 banks apart: the four k of an MFMA step meet every bank once)
    __shared__ float s_xdw[Q * LDX], s_wgt[Q], s_delta[Q];
    const int ci = blockIdx.y;
    int b, len; int64_t tok0;
    if (!chunk_of(rg, w, ci, &b, &tok0, &len)) return;
    const int h = (int)(blockIdx.x / w.p_tiles), p0 = (int)(blockIdx.x % w.p_tiles) * PT;
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    float *csd = w.csd + ((int64_t)ci * a.n_head + h) * (2 * Q);
    if (wv == 0) {
        const bool valid = lane < len;
        float delta = 0.0f, la = 0.0f;
        if (valid) {
            float d = a.dt[(tok0 + lane) * a.ld_dt + h];
            if (a.dt_bias) d = d + a.dt_bias[h];
            delta = d <= 20.0f ? log1pf(expf(d)) : d;
            la = delta * a.A[(int64_t)h * a.a_ld];
        }
        float run = 0.0f, cs = 0.0f;
#pragma unroll
        for (int i = 0; i < Q; ++i) {                                // (the rows past len add +0.0f: run ends as cs of the last token)
            run = run + __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, la), i));
            cs = lane == i ? run : cs;
        }
        s_wgt[lane] = valid ? expf(run - cs) : 0.0f;
        s_delta[lane] = delta;
        if (p0 == 0) { csd[lane] = cs; csd[Q + lane] = delta; }
    }
    __syncthreads();
    for (int idx = tid; idx < Q * PT; idx += 256) {
        const int s = idx / PT, p = idx % PT;
        float v = 0.0f;
        if (s < len) v = (s_delta[s] * a.x[(tok0 + s) * a.ldx_tok + (int64_t)h * a.ldx_head + p0 + p]) * s_wgt[s];
        s_xdw[s * LDX + p] = v;
    }
    __syncthreads();
    const int i = lane & 15, kq = lane >> 4;
    const int64_t bcol = (int64_t)(h / (a.n_head / a.n_group)) * a.N;
    float *S = w.hst + (((int64_t)ci * a.n_head + h) * a.P + p0) * a.N;
    for (int nb = wv; nb < a.N / 16; nb += 4) {
        f32x4 acc[PT / 16];
#pragma unroll
        for (int pi = 0; pi < PT / 16; ++pi) acc[pi] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
#pragma unroll
        for (int kk = 0; kk < Q / 4; ++kk) {
            const int s = 4 * kk + kq;
            float bv = a.B[(tok0 + (s < len ? s : 0)) * a.ld_bc + bcol + 16 * nb + i];
            bv = s < len ? bv : 0.0f;
#pragma unroll
            for (int pi = 0; pi < PT / 16; ++pi) acc[pi] = mfma4(s_xdw[s * LDX + 16 * pi + i], bv, acc[pi]);
        }
#pragma unroll
        for (int pi = 0; pi < PT / 16; ++pi)
#pragma unroll
            for (int r = 0; r < 4; ++r) S[(int64_t)(16 * pi + 4 * kq + r) * a.N + 16 * nb + i] = acc[pi][r];
    }
}

__global__ __launch_bounds__(256) void ssm_chunk_pass_kernel(const ssm_scan_args a, const chunk_work w) {
    const int si = blockIdx.y;
    if (si >= w.hdr[1]) return;
    const int4 e = w.seqs[si];
    const int b = e.x, first = e.y, n = e.z;
    const int sl = a.slot[b];
    if (sl < 0 || sl >= a.n_slots) return;
    const int64_t head_elems = (int64_t)a.P * a.N, elems = head_elems * a.n_head;
    const int64_t el = ((int64_t)blockIdx.x * 256 + threadIdx.x) * 4;
    if (el >= elems) return;
    const int h = (int)(el / head_elems);
    float4 *st = (float4 *)(a.state + (int64_t)sl * a.slot_elems + el);
    float4 hv = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (a.len[b] != 0) hv = *st;
    for (int c0 = 0; c0 < n; c0 += 4) {
        float4 S[4]; float dec[4];
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c0 + u < n) {
                const int64_t ci = first + c0 + u;
                S[u] = *(const float4 *)(w.hst + ci * elems + el);
                dec[u] = expf(w.csd[(ci * a.n_head + h) * (2 * Q) + Q - 1]);
            }
#pragma unroll
        for (int u = 0; u < 4; ++u)
            if (c0 + u < n) {
                *(float4 *)(w.hst + (int64_t)(first + c0 + u) * elems + el) = hv;
                hv.x = fmaf(hv.x, dec[u], S[u].x); hv.y = fmaf(hv.y, dec[u], S[u].y); hv.z = fmaf(hv.z, dec[u], S[u].z); hv.w = fmaf(hv.w, dec[u], S[u].w);
            }
    }
    *st = hv;
}

template <int PT>
__global__ __launch_bounds__(256) void ssm_chunk_out_kernel(const kv_ragged rg, const ssm_scan_args a, const chunk_work w) {
    constexpr int LDX = PT == 16 ? 16 : PT + 16;
    __shared__ float s_xd[Q * LDX], s_M[4 * 16 * LDM], s_cs[Q];
    const int ci = blockIdx.y;
    int b, len; int64_t tok0;
    if (!chunk_of(rg, w, ci, &b, &tok0, &len)) return;
    const int h = (int)(blockIdx.x / w.p_tiles), p0 = (int)(blockIdx.x % w.p_tiles) * PT;
    const int tid = threadIdx.x, lane = tid & 63, wv = __builtin_amdgcn_readfirstlane(tid >> 6);   // (the wave, known to be uniform)
    const int i = lane & 15, kq = lane >> 4;
    float *drow = a.dst + tok0 * a.ldd_tok + (int64_t)h * a.ldd_head + p0;
    const float *xrow = a.x + tok0 * a.ldx_tok + (int64_t)h * a.ldx_head + p0;
    const int sl = a.slot[b];
    if (sl < 0 || sl >= a.n_slots) {                                 // (uniform over the workgroup)
        for (int idx = tid; idx < len * PT; idx += 256) drow[(int64_t)(idx / PT) * a.ldd_tok + idx % PT] = 0.0f;
        return;
    }
    const float *csd = w.csd + ((int64_t)ci * a.n_head + h) * (2 * Q);
    if (tid < Q) s_cs[tid] = csd[tid];
    for (int idx = tid; idx < Q * PT; idx += 256) {
        const int s = idx / PT, p = idx % PT;
        s_xd[s * LDX + p] = s < len ? csd[Q + s] * xrow[(int64_t)s * a.ldx_tok + p] : 0.0f;
    }
    __syncthreads();
    const int64_t bcol = (int64_t)(h / (a.n_head / a.n_group)) * a.N;
    const int t = 16 * wv + i;                                       // the row this lane feeds as an A operand
    const bool tvalid = t < len;
    const float *Crow = a.C + (tok0 + (tvalid ? t : 0)) * a.ld_bc + bcol + 4 * kq;   // (a row past the chunk: the chunk's first row is loaded, zeros are used)
    float *Mw = s_M + wv * 16 * LDM;
    const int nkb = a.N / 16;
    {
        f32x4 G[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) G[j] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
        // two steps of 16 states per trip, every load of the trip issued before its first MFMA; an odd last trip loads its own step twice and
        // skips the second step's MFMAs.  The chain's order stays kb ascending
        if (16 * wv < len)
            for (int kb = 0; kb < nkb; kb += 2) {
                const bool two = kb + 1 < nkb;                           // (uniform)
                const int o0 = 16 * kb, o1 = two ? o0 + 16 : o0;
                float4 c0 = *(const float4 *)(Crow + o0), c1 = *(const float4 *)(Crow + o1);
                float4 b0[4], b1[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int s = 16 * j + i;
                    const float *Brow = a.B + (tok0 + (s < len ? s : 0)) * a.ld_bc + bcol + 4 * kq;
                    b0[j] = *(const float4 *)(Brow + o0); b1[j] = *(const float4 *)(Brow + o1);
                    if (s >= len) b0[j] = b1[j] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
                }
                if (!tvalid) c0 = c1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (j <= wv) { G[j] = mfma4(c0.x, b0[j].x, G[j]); G[j] = mfma4(c0.y, b0[j].y, G[j]); G[j] = mfma4(c0.z, b0[j].z, G[j]); G[j] = mfma4(c0.w, b0[j].w, G[j]); }
                if (two) {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (j <= wv) { G[j] = mfma4(c1.x, b1[j].x, G[j]); G[j] = mfma4(c1.y, b1[j].y, G[j]); G[j] = mfma4(c1.z, b1[j].z, G[j]); G[j] = mfma4(c1.w, b1[j].w, G[j]); }
                }
            }
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (j <= wv) {
                const int ss = 16 * j + i;
                const float g[4] = {G[j][0], G[j][1], G[j][2], G[j][3]};
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const int tt = 16 * wv + 4 * kq + r;
                    float m = 0.0f;
                    if (ss <= tt && tt < len) m = expf(s_cs[tt] - s_cs[ss]) * g[r];
                    Mw[(4 * kq + r) * LDM + ss] = m;
                }
            }
    }
    __syncthreads();
    if (16 * wv >= len) return;
    f32x4 acc[PT / 16];
#pragma unroll
    for (int pi = 0; pi < PT / 16; ++pi) acc[pi] = f32x4{0.0f, 0.0f, 0.0f, 0.0f};
    const float ecs = tvalid ? expf(s_cs[tvalid ? t : 0]) : 0.0f;
    const float *Hin = w.hst + (((int64_t)ci * a.n_head + h) * a.P + p0 + i) * a.N + 4 * kq;
    for (int kb = 0; kb < nkb; kb += 2) {
        const bool two = kb + 1 < nkb;
        const int o0 = 16 * kb, o1 = two ? o0 + 16 : o0;
        float4 c0 = *(const float4 *)(Crow + o0), c1 = *(const float4 *)(Crow + o1);
        float4 h0[PT / 16], h1[PT / 16];
#pragma unroll
        for (int pi = 0; pi < PT / 16; ++pi) { h0[pi] = *(const float4 *)(Hin + (int64_t)16 * pi * a.N + o0); h1[pi] = *(const float4 *)(Hin + (int64_t)16 * pi * a.N + o1); }
        if (!tvalid) c0 = c1 = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        c0.x = ecs * c0.x; c0.y = ecs * c0.y; c0.z = ecs * c0.z; c0.w = ecs * c0.w;
        c1.x = ecs * c1.x; c1.y = ecs * c1.y; c1.z = ecs * c1.z; c1.w = ecs * c1.w;
#pragma unroll
        for (int pi = 0; pi < PT / 16; ++pi) {
            acc[pi] = mfma4(c0.x, h0[pi].x, acc[pi]); acc[pi] = mfma4(c0.y, h0[pi].y, acc[pi]); acc[pi] = mfma4(c0.z, h0[pi].z, acc[pi]); acc[pi] = mfma4(c0.w, h0[pi].w, acc[pi]);
        }
        if (two) {
#pragma unroll
            for (int pi = 0; pi < PT / 16; ++pi) {
                acc[pi] = mfma4(c1.x, h1[pi].x, acc[pi]); acc[pi] = mfma4(c1.y, h1[pi].y, acc[pi]); acc[pi] = mfma4(c1.z, h1[pi].z, acc[pi]); acc[pi] = mfma4(c1.w, h1[pi].w, acc[pi]);
            }
        }
    }
    for (int kk = 0; kk < 4 * (wv + 1); ++kk) {
        const int s = 4 * kk + kq;
        const float m = Mw[i * LDM + s];
#pragma unroll
        for (int pi = 0; pi < PT / 16; ++pi) acc[pi] = mfma4(m, s_xd[s * LDX + 16 * pi + i], acc[pi]);
    }
    const float Dh = a.D ? a.D[h] : 0.0f;
#pragma unroll
    for (int pi = 0; pi < PT / 16; ++pi) {
        const float v[4] = {acc[pi][0], acc[pi][1], acc[pi][2], acc[pi][3]};
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int tt = 16 * wv + 4 * kq + r;
            if (tt < len) {
                float y = v[r];
                if (a.D) y = fmaf(Dh, xrow[(int64_t)tt * a.ldx_tok + 16 * pi + i], y);
                drow[(int64_t)tt * a.ldd_tok + 16 * pi + i] = y;
            }
        }
    }
}

template <int PT>
void chunk_launch(const dim3 grid, hipStream_t st, const kv_ragged &rg, const ssm_scan_args &a, const chunk_work &w, bool out) {
    if (out) ssm_chunk_out_kernel<PT><<<grid, 256, 0, st>>>(rg, a, w);
    else ssm_chunk_state_kernel<PT><<<grid, 256, 0, st>>>(rg, a, w);
}

hipError_t chunk_launch(int p_tile, const dim3 grid, hipStream_t st, const kv_ragged &rg, const ssm_scan_args &a, const chunk_work &w, bool out) {
    switch (p_tile) {
    case 16: chunk_launch<16>(grid, st, rg, a, w, out); break;
    case 32: chunk_launch<32>(grid, st, rg, a, w, out); break;
    case 64: chunk_launch<64>(grid, st, rg, a, w, out); break;
    default: return hipErrorInvalidValue;
    }
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ssm_scan_chunked(const ssm_chunk_plan &pl, const kv_ragged &rg, const ssm_scan_args &s, void *work, hipStream_t st) {
    ssm_scan_args a = s;
    a.nq_max = pl.form == SSM_FORM_CHUNKED ? pl.seq_max_tokens : INT_MAX;
    hipError_t e = launch_ssm_scan(pl.seq, rg, a, st);
    if (e != hipSuccess || pl.form != SSM_FORM_CHUNKED) return e;
    char *base = (char *)work;
    chunk_work w;
    w.hdr = (int32_t *)(base + pl.hdr_off); w.seqs = (int4 *)(base + pl.seqs_off); w.list = (int2 *)(base + pl.list_off);
    w.csd = (float *)(base + pl.csd_off); w.hst = (float *)(base + pl.state_off);
    w.chunks_max = (int)pl.chunks_max; w.seqs_max = (int)pl.seqs_max; w.seq_max_tokens = pl.seq_max_tokens; w.p_tiles = pl.p_tiles;
    ssm_chunk_index_kernel<<<1, 1024, 0, st>>>(rg, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    const dim3 grid((unsigned)((int64_t)a.n_head * pl.p_tiles), (unsigned)pl.chunks_max);
    if ((e = chunk_launch(pl.p_tile, grid, st, rg, a, w, false)) != hipSuccess) return e;
    ssm_chunk_pass_kernel<<<dim3((unsigned)pl.pass_wgs_x, (unsigned)pl.seqs_max), 256, 0, st>>>(a, w);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    return chunk_launch(pl.p_tile, grid, st, rg, a, w, true);
}
