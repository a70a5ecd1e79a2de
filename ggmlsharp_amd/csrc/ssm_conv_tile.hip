// ssm_conv_tile.hip -- the causal conv of a LONG sequence in tiles of T tokens, one thread per (tile, 4 adjacent channels): the token-parallel form of
// ssm.hip's ssm_conv_kernel (include/ggml_hip_ext.h, ggml_hip_ssm_conv_tiled_ragged_dev; the checks are ssm.cpp's, every grid and the work buffer are
// plan.h's plan_ssm_conv_tiled).  A sequence of at most seq_max_tokens tokens stays with the sequential kernel, which the launcher starts first with
// that window.
//
// The statement is a fixed fma chain per token over the d_conv rows that end at the token, so a tile needs nothing of the tiles in front of it but their
// last d_conv - 1 INPUT rows: the tiled form is bit for bit the sequential one, wherever the tiles are cut and wherever a sequence is split over calls.
//
// THREE HAZARDS the parallel form has and the sequential one did not (a numpy prototype of the tile scheme, tests/np_ssm_conv_tiled.py, shows each):
//   1. HALO ROWS, IN PLACE.  Tile j > 0 needs the d_conv - 1 rows in front of it, and with dst == x another workgroup overwrites exactly those rows.
//      So no tile reads a row of x outside itself: the edges kernel, a launch of its own BEFORE any row is written, copies every tile's halo into the
//      work buffer, and the tile kernel's first d_conv - 1 window rows ALWAYS come from there -- in place and out of place are one path.
//   2. THE SLOT.  The first tile reads the old slot, and the new slot is the sequence's last d_conv - 1 input rows.  Done by different workgroups of one
//      launch that is a race; in place the last input rows may already be overwritten; and a last tile of fewer than d_conv - 1 tokens does not even
//      hold them.  So ONE thread of the edges kernel, the one of (first tile, channel), does all three in order: old slot (zeros where fresh) -> work
//      buffer, the sequence's last d_conv - 1 rows of x -> registers, registers -> slot.  A long sequence has more than d_conv - 1 tokens
//      (seq_max_tokens >= d_conv - 1), so the new slot is all x.  No other kernel of the form touches a slot.
//   3. TILES ARE COUNTED FROM THE SEQUENCE'S OWN FIRST ROW.  Cut on packed-row boundaries, a tile that starts fewer than d_conv - 1 tokens into a
//      sequence would need a window mixing slot rows and x rows -- hazard 2 in a second place -- and a sequence's tiles would follow its neighbours.
//      With T >= d_conv - 1 the halo of tile j > 0 lies inside the sequence's rows of this call.
//
//   ssm_conv_index_kernel      one workgroup: a prefix sum over the long sequences' tile counts -> the tile list (b, tile of b), clamped (plan.h); the
//                              list is filled by all 1024 threads (one thread writing a long prefill's entries alone took as long as the edges pass)
//   ssm_conv_edges_kernel<KC, V>  per (tile, V channels): the halo into the work buffer; for a first tile the slot hand-over above.  Only reads x
//   ssm_conv_tile_kernel<KC, V>  per (tile, V channels): pure streaming, no LDS, no barrier.  The window lives in registers; the loads of up to
//                              CONV_UNROLL tokens are issued together (they depend on nothing the loop computes), 16 bytes each where V = 4.  In place
//                              is safe because a thread reads x[t][c ..] before it writes dst[t][c ..] and nothing else touches those channels of the tile.
// Every guard comes before the address it protects, as in ssm.hip: the list entry is below the count the index kernel wrote, the sequence is present,
// the slot id lies inside [0, n_slots) (else +0.0f rows, no state, nothing read through it).
#include <climits>
#include "common.h"
#include "plan.h"

namespace {

constexpr int CONV_UNROLL = 8;

struct conv_work {
    int32_t *hdr; int2 *list; float *halo;
    int tiles_max, seqs_max, seq_max_tokens, tile;
    int64_t halo_ld;
};

struct conv_args {
    const int32_t *len, *slot; int n_slots;
    const float *x; int64_t ldx;
    const float *w, *bias; int act;
    int64_t n_ch;
    float *state; int64_t slot_elems;
    float *dst; int64_t ldd;
};

__global__ __launch_bounds__(1024) void ssm_conv_index_kernel(const kv_ragged rg, const conv_work w) {
    __shared__ int sc[1024], ss[1024];
    const int tid = threadIdx.x, per = (rg.n_seq + 1023) / 1024, T = w.tile;
    int nc = 0, ns = 0;
    for (int i = 0; i < per; ++i) {
        const int b = tid * per + i;
        int64_t qs; int nq;
        if (b < rg.n_seq && ssm_sequence(rg, b, &qs, &nq) && nq > w.seq_max_tokens) { nc += (nq + T - 1) / T; ns += 1; }
    }
    sc[tid] = nc; ss[tid] = ns;
    __syncthreads();
    for (int d = 1; d < 1024; d *= 2) {
        const int a = tid >= d ? sc[tid - d] : 0, s = tid >= d ? ss[tid - d] : 0;
        __syncthreads();
        sc[tid] += a; ss[tid] += s;
        __syncthreads();
    }
    // the list, every thread filling entries tid, tid + 1024, ..: entry c belongs to the thread t whose sequences hold it -- the first t with
    // sc[t] > c, by bisection of the inclusive sums -- and to the sequence of that thread's `per` that the walk from sc[t - 1] reaches
    const int total = sc[1023] < w.tiles_max ? sc[1023] : w.tiles_max;
    for (int c = tid; c < total; c += 1024) {
        int lo = 0, hi = 1023;
        while (lo < hi) {
            const int mid = (lo + hi) >> 1;
            if (sc[mid] > c) hi = mid; else lo = mid + 1;
        }
        int c0 = lo ? sc[lo - 1] : 0;
        for (int i = 0; i < per; ++i) {
            const int b = lo * per + i;
            int64_t qs; int nq;
            if (b < rg.n_seq && ssm_sequence(rg, b, &qs, &nq) && nq > w.seq_max_tokens) {
                const int n = (nq + T - 1) / T;
                if (c < c0 + n) { w.list[c] = make_int2(b, c - c0); break; }
                c0 += n;
            }
        }
    }
    if (tid == 1023) {
        w.hdr[0] = total;
        w.hdr[1] = ss[1023] < w.seqs_max ? ss[1023] : w.seqs_max;
        w.hdr[2] = 0; w.hdr[3] = 0;
    }
}

// the tile of list entry ci: its sequence, the sequence's first packed row and count, the tile's number; false past the list or for a sequence that is
// not present and long (the index kernel lists no other: the second check costs two loads and keeps every address behind its guard)
__device__ __forceinline__ bool tile_of(const kv_ragged &rg, const conv_work &w, int ci, int *b, int64_t *qs, int *nq, int *j) {
    if (ci >= w.hdr[0]) return false;
    const int2 e = w.list[ci];
    if (!ssm_sequence(rg, e.x, qs, nq) || *nq <= w.seq_max_tokens) return false;
    *b = e.x; *j = e.y;
    return (int64_t)e.y * w.tile < *nq;
}

// V channels of one row: 16 bytes where V = 4
template <int V> struct chv { float f[V]; };
template <int V> __device__ __forceinline__ chv<V> ld_ch(const float *p) {
    chv<V> r;
    if constexpr (V == 4) { const float4 t = *(const float4 *)p; r.f[0] = t.x; r.f[1] = t.y; r.f[2] = t.z; r.f[3] = t.w; }
    else r.f[0] = *p;
    return r;
}
template <int V> __device__ __forceinline__ void st_ch(float *p, const chv<V> &r) {
    if constexpr (V == 4) *(float4 *)p = make_float4(r.f[0], r.f[1], r.f[2], r.f[3]);
    else *p = r.f[0];
}

template <int KC, int V>
__global__ __launch_bounds__(256) void ssm_conv_edges_kernel(const kv_ragged rg, const conv_args a, const conv_work w) {
    const int ci = blockIdx.x;
    int b, nq, j; int64_t qs;
    if (!tile_of(rg, w, ci, &b, &qs, &nq, &j)) return;
    const int sl = a.slot[b];
    if (sl < 0 || sl >= a.n_slots) return;                               // (uniform over the workgroup; the tile kernel writes the +0.0f rows)
    float *halo = w.halo + (int64_t)ci * (KC - 1) * w.halo_ld;
    const bool fresh = a.len[b] == 0;
    for (int64_t c = (((int64_t)blockIdx.y * 256) + threadIdx.x) * V; c < a.n_ch; c += (int64_t)gridDim.y * 256 * V) {
        chv<V> v[KC - 1];
        if (j > 0) {                                                     // rows j T - (KC - 1) .. j T - 1 of the sequence: inside it, T >= KC - 1
            const float *xr = a.x + (qs + (int64_t)j * w.tile - (KC - 1)) * a.ldx + c;
#pragma unroll
            for (int k = 0; k < KC - 1; ++k) v[k] = ld_ch<V>(xr + k * a.ldx);
#pragma unroll
            for (int k = 0; k < KC - 1; ++k) st_ch<V>(halo + k * w.halo_ld + c, v[k]);
        } else {                                                         // the slot hand-over: this thread alone reads and writes slot elements (k, c ..)
            float *st = a.state + (int64_t)sl * a.slot_elems + c;
            const float *xr = a.x + (qs + nq - (KC - 1)) * a.ldx + c;   // (nq > seq_max_tokens >= KC - 1)
            chv<V> last[KC - 1];
#pragma unroll
            for (int k = 0; k < KC - 1; ++k) {
                if (fresh) {
#pragma unroll
                    for (int i = 0; i < V; ++i) v[k].f[i] = 0.0f;
                } else {
                    v[k] = ld_ch<V>(st + k * a.n_ch);
                }
            }
#pragma unroll
            for (int k = 0; k < KC - 1; ++k) last[k] = ld_ch<V>(xr + k * a.ldx);
#pragma unroll
            for (int k = 0; k < KC - 1; ++k) st_ch<V>(halo + k * w.halo_ld + c, v[k]);
#pragma unroll
            for (int k = 0; k < KC - 1; ++k) st_ch<V>(st + k * a.n_ch, last[k]);
        }
    }
}

template <int KC, int V>
__global__ __launch_bounds__(256) void ssm_conv_tile_kernel(const kv_ragged rg, const conv_args a, const conv_work w) {
    const int ci = blockIdx.x;
    int b, nq, j; int64_t qs;
    if (!tile_of(rg, w, ci, &b, &qs, &nq, &j)) return;
    const int t0 = j * w.tile;
    const int n = nq - t0 < w.tile ? nq - t0 : w.tile;                  // the tile's tokens, 1 .. T
    const int sl = a.slot[b];
    const bool zero = sl < 0 || sl >= a.n_slots;                         // (uniform over the workgroup)
    const float *halo = w.halo + (int64_t)ci * (KC - 1) * w.halo_ld;
    for (int64_t c = (((int64_t)blockIdx.y * 256) + threadIdx.x) * V; c < a.n_ch; c += (int64_t)gridDim.y * 256 * V) {
        const float *xr = a.x + (qs + t0) * a.ldx + c;
        float *dr = a.dst + (qs + t0) * a.ldd + c;
        if (zero) {
            chv<V> z;
#pragma unroll
            for (int i = 0; i < V; ++i) z.f[i] = 0.0f;
            for (int t = 0; t < n; ++t) st_ch<V>(dr + t * a.ldd, z);
            continue;
        }
        float wk[V][KC];
        chv<V> win[KC], bv;
        if constexpr (V == 4) {                                          // w[c .. c + 3][0 .. KC): KC float4 in a row
#pragma unroll
            for (int k = 0; k < KC; ++k) {
                const chv<V> t = ld_ch<V>(a.w + c * KC + 4 * k);
#pragma unroll
                for (int i = 0; i < V; ++i) wk[(4 * k + i) / KC][(4 * k + i) % KC] = t.f[i];
            }
        } else {
#pragma unroll
            for (int k = 0; k < KC; ++k) wk[0][k] = a.w[c * KC + k];
        }
#pragma unroll
        for (int i = 0; i < V; ++i) bv.f[i] = 0.0f;
        if (a.bias) bv = ld_ch<V>(a.bias + c);
#pragma unroll
        for (int k = 0; k < KC - 1; ++k) win[k] = ld_ch<V>(halo + k * w.halo_ld + c);
        for (int u0 = 0; u0 < n; u0 += CONV_UNROLL) {
            chv<V> xv[CONV_UNROLL];
#pragma unroll
            for (int u = 0; u < CONV_UNROLL; ++u)
                if (u0 + u < n) xv[u] = ld_ch<V>(xr + (u0 + u) * a.ldx);
#pragma unroll
            for (int u = 0; u < CONV_UNROLL; ++u) {
                if (u0 + u < n) {
                    win[KC - 1] = xv[u];
                    chv<V> y;
#pragma unroll
                    for (int i = 0; i < V; ++i) {
                        float acc = wk[i][0] * win[0].f[i];
#pragma unroll
                        for (int k = 1; k < KC; ++k) acc = fmaf(wk[i][k], win[k].f[i], acc);
                        if (a.bias) acc = acc + bv.f[i];
                        if (a.act) acc = acc / (1.0f + expf(-acc));
                        y.f[i] = acc;
                    }
                    st_ch<V>(dr + (u0 + u) * a.ldd, y);
#pragma unroll
                    for (int k = 0; k < KC - 1; ++k) win[k] = win[k + 1];
                }
            }
        }
    }
}

template <int KC>
hipError_t conv_tiled_launch(bool vec, const dim3 grid, hipStream_t st, const kv_ragged &rg, const conv_args &a, const conv_work &w) {
    if (vec) ssm_conv_edges_kernel<KC, 4><<<grid, 256, 0, st>>>(rg, a, w);
    else ssm_conv_edges_kernel<KC, 1><<<grid, 256, 0, st>>>(rg, a, w);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
    if (vec) ssm_conv_tile_kernel<KC, 4><<<grid, 256, 0, st>>>(rg, a, w);
    else ssm_conv_tile_kernel<KC, 1><<<grid, 256, 0, st>>>(rg, a, w);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_ssm_conv_tiled(const ssm_conv_tiled_plan &pl, const kv_ragged &rg, const int32_t *len, const int32_t *slot, int n_slots, const float *x,
                                 int64_t ldx, const float *w, const float *bias, int act, int64_t n_ch, int d_conv, float *state, int64_t slot_elems, float *dst,
                                 int64_t ldd, void *work, hipStream_t st) {
    const bool tiled = pl.form == SSM_FORM_TILED;
    hipError_t e = launch_ssm_conv(pl.seq, rg, len, slot, n_slots, x, ldx, w, bias, act, n_ch, d_conv, state, slot_elems, dst, ldd,
                                   tiled ? pl.seq_max_tokens : INT_MAX, st);
    if (e != hipSuccess || !tiled) return e;
    char *base = (char *)work;
    conv_work cw;
    cw.hdr = (int32_t *)(base + pl.hdr_off); cw.list = (int2 *)(base + pl.list_off); cw.halo = (float *)(base + pl.halo_off);
    cw.tiles_max = (int)pl.tiles_max; cw.seqs_max = (int)pl.seqs_max; cw.seq_max_tokens = pl.seq_max_tokens; cw.tile = pl.tile; cw.halo_ld = pl.halo_ld;
    conv_args a;
    a.len = len; a.slot = slot; a.n_slots = n_slots; a.x = x; a.ldx = ldx; a.w = w; a.bias = bias; a.act = act; a.n_ch = n_ch; a.state = state;
    a.slot_elems = slot_elems; a.dst = dst; a.ldd = ldd;
    ssm_conv_index_kernel<<<1, 1024, 0, st>>>(rg, cw);
    if ((e = hipGetLastError()) != hipSuccess) return e;
    // 16-byte moves where every row of x, dst, w and bias starts on a 16-byte boundary for a thread's 4 channels (the halo rows and the slots' always
    // do: the pool is 16-byte aligned, nb_slot and 4 n_ch are multiples of 16)
    const bool vec = pl.vec == 4 && ldx % 4 == 0 && ldd % 4 == 0 && (((uintptr_t)x | (uintptr_t)dst | (uintptr_t)w | (uintptr_t)bias) & 15) == 0;
    const int64_t ch_wgs = vec ? (n_ch / 4 + 255) / 256 : pl.seq.wgs_x;
    const dim3 grid((unsigned)pl.tiles_max, (unsigned)(ch_wgs < 32768 ? ch_wgs : 32768));
    switch (d_conv) {
    case 2: return conv_tiled_launch<2>(vec, grid, st, rg, a, cw);
    case 3: return conv_tiled_launch<3>(vec, grid, st, rg, a, cw);
    case 4: return conv_tiled_launch<4>(vec, grid, st, rg, a, cw);
    default: return hipErrorInvalidValue;
    }
}
