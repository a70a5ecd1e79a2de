// gemv_fused_body.inc -- the body of K2f, the fused mat-vec (gemv.hip has its description and includes this text TWICE):
//   gemv_fused_body       GVF_WG = blockIdx.x, GVF_NWG = gridDim.x: the single- and multi-matrix kernels, token for token what they always were;
//   gemv_fused_body_byid  the workgroup's index and the number of workgroups that share the row tiles handed in (wg_in of nwg_in: the workgroups
//                         of ONE pair of ggml_hip_mul_mat_id_dev) -- which workgroup takes a tile is geometry, a tile's arithmetic does not know it.
// One text, so the two cannot drift apart: block -> lane assignment, chunking and the reduction order are the same by construction.  (A template
// parameter for the choice was tried first: it moved the register allocation of 68 of the existing kernels.)
template <int TYPE, int NC, int GV_ROWS, bool SC, bool PRO, bool MULTI, bool K8 = false>
__device__ __forceinline__ void GVF_BODY(const mv_set &ws, const float *__restrict__ x, int64_t ld1, int64_t nbk, int N, int ntiles,
                                         const mm_epilogue &ep, const mm_prologue &pro GVF_WG_PARAMS) {
    static_assert(GV_ROWS == 16 && GV_NKQ == 4, "lane = (row, k-lane) with 4 k-lanes per wave");
    constexpr int CH = GV_CHUNK;                       // k-blocks per chunk, all waves together
    constexpr int BPL = CH / GV_WORKERS;               // k-blocks per lane per chunk (4)
    constexpr int WBLK = GV_NKQ * BPL;                 // k-blocks per WAVE per chunk (16): local id i = kq + 4 * j
    // wave-private slice: per local block a slot of NC x {16 B even plane, 16 B odd plane} (+16 B so that the four k-lanes of
    // a wave, NC * 32 B apart, never start on the same bank), then NC scales and NC block sums
    constexpr int QSLOT = NC * 32 + 16;
    constexpr int WSLICE = WBLK * QSLOT + WBLK * NC * 8;
    __shared__ __attribute__((aligned(16))) uint8_t sAct[GV_WAVES * WSLICE];
    __shared__ float sRed[2][GV_WAVES][NC][GV_ROWS];

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int r = lane % GV_ROWS, kq = lane / GV_ROWS, u = wave * GV_NKQ + kq;
    uint8_t *const myq = sAct + wave * WSLICE;
    float *const myd = (float *)(myq + WBLK * QSLOT);
    int *const mys = (int *)(myd + WBLK * NC);
    constexpr bool single_chunk = SC;
    bool staged = false;
    int parity = 0;
    __shared__ float sScale[NC];
    __shared__ float sK8[K8 ? NC * GV_K8_SB * 2 : 1];      // (column, super-block) -> iscale, d
    static_assert(!(K8 && (PRO || MULTI)), "the Q8_K rule: the plain single-matrix call only");
    constexpr bool HAS_M = TYPE == GGML_TYPE_Q4_1 || TYPE == GGML_TYPE_Q5_1 || GV_TWO_SC<TYPE>;   // Q4_2: second scale
    constexpr bool HAS_H = TYPE == GGML_TYPE_Q5_0 || TYPE == GGML_TYPE_Q5_1;
    constexpr int NP = 1 + (HAS_M ? 1 : 0) + (HAS_H ? 1 : 0);

    // The work of a workgroup is a sequence of ITEMS (row tile, chunk of 128 k-blocks), tiles taken round-robin over the
    // persistent grid.  The weight registers are double-buffered across items: item w+1's weights are requested BEFORE item
    // w is consumed, so the memory pipe never drains between tiles (a tile's dots, reduction and barrier used to sit between
    // two bursts of loads: ~10 % of a round at M = 32000).
    const int nchunks = (int)((nbk + CH - 1) / CH);
    const int my_tiles = GVF_WG < ntiles ? (ntiles - 1 - (int)GVF_WG) / (int)GVF_NWG + 1 : 0;
    const int nitems = my_tiles * nchunks;
    auto tile_of = [&](int w) {
        // row tiles in launch order (neighbouring workgroups stream neighbouring 256-byte pieces of every k-block row; the
        // per-XCD ranges this used to hand out existed for the [k-block][row] scale plane, whose 128-byte lines two tiles
        // shared -- with the tile-major side image they cost 3-6 % at M >= 11008)
        return (int)GVF_WG + (w / nchunks) * (int)GVF_NWG;
    };
    // the matrix a global row tile belongs to (common.h mv_set; one matrix: the selects fold to its fields) and the tile in it
    struct Sel { const uint8_t *qs; const uint32_t *gs; float *dst; int64_t M, Mpad, ldd; int tile; };
    auto select = [&](int gt) {
        Sel o;
        if constexpr (!MULTI) {
            o.qs = ws.qs[0]; o.gs = ws.gs[0]; o.dst = ws.dst[0]; o.M = ws.M[0]; o.Mpad = ws.Mpad[0]; o.ldd = ws.ldd[0]; o.tile = gt;
            return o;
        }
        const int k = (gt >= ws.tile_end[0]) + (gt >= ws.tile_end[1]) + (gt >= ws.tile_end[2]);
        o.qs = k == 0 ? ws.qs[0] : k == 1 ? ws.qs[1] : k == 2 ? ws.qs[2] : ws.qs[3];
        o.gs = k == 0 ? ws.gs[0] : k == 1 ? ws.gs[1] : k == 2 ? ws.gs[2] : ws.gs[3];
        o.dst = k == 0 ? ws.dst[0] : k == 1 ? ws.dst[1] : k == 2 ? ws.dst[2] : ws.dst[3];
        o.M = k == 0 ? ws.M[0] : k == 1 ? ws.M[1] : k == 2 ? ws.M[2] : ws.M[3];
        o.Mpad = k == 0 ? ws.Mpad[0] : k == 1 ? ws.Mpad[1] : k == 2 ? ws.Mpad[2] : ws.Mpad[3];
        o.ldd = k == 0 ? ws.ldd[0] : k == 1 ? ws.ldd[1] : k == 2 ? ws.ldd[2] : ws.ldd[3];
        o.tile = gt - (k == 0 ? 0 : k == 1 ? ws.tile_end[0] : k == 2 ? ws.tile_end[1] : ws.tile_end[2]);
        return o;
    };
    // (wider batches keep one register set: their activation registers already fill the budget, and the second set cost
    // them a resident workgroup -- 32000 x 4096 x 8: 50.5 us with it against 41.9 without)
    // (the look-ahead form: one column, and three / four -- 11008 x 4096 x 4 15.6 -> 12.6 us, 32000 x 4096 x 4 29.6 -> 23.3 with
    // one workgroup per CU; two columns measured level to worse: 11008 x 4096 x 2 8.3 -> 9.1 us)
    constexpr bool PF = SC && (NC == 1 || NC == 4);
    uint4 q[BPL], q2[GV_W_I8<TYPE> ? BPL : 1], qn[PF ? BPL : 1], q2n[PF && GV_W_I8<TYPE> ? BPL : 1];
    float dw[BPL], mw[HAS_M ? BPL : 1], dwn[PF ? BPL : 1], mwn[PF && HAS_M ? BPL : 1];
    uint32_t hb[HAS_H ? BPL : 1], hbn[PF && HAS_H ? BPL : 1];
    // the weight stream of one item (4 x 16 B + scales in flight per lane)
    auto load_item = [&](int w, uint4 *Q, uint4 *Q2, float *DW, float *MW, uint32_t *HB) {
        const Sel sel = select(tile_of(w));
        const uint8_t *const qs = sel.qs;
        const uint32_t *const gs = sel.gs;
        const int64_t Mpad = sel.Mpad;
        const int tl = sel.tile;
        const int64_t row = (int64_t)tl * GV_ROWS + r;  // < Mpad by construction
        const int64_t cb = (int64_t)(w % nchunks) * CH;
        const int nbc = (int)((nbk - cb) < CH ? (nbk - cb) : CH);
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            const int bl = u + GV_WORKERS * j;
            const bool ok = bl < nbc;
            const int64_t b = cb + (ok ? bl : 0);
            if (GV_W_I8<TYPE>) {
                Q[j] = ld_w(qs + ((b * 2 + 0) * Mpad + row) * 16);
                Q2[j] = ld_w(qs + ((b * 2 + 1) * Mpad + row) * 16);
            } else {
                Q[j] = ld_w(qs + (b * Mpad + row) * 16);
            }
            // (unconditional loads from a clamped block: no branch and no use of a result inside the load sequence -- the item's
            // consumer zeroes the scales of a block past the end of K)
            // scales / mins / fifth bits from the tile-major side image (common.h ggml_hip_weight::gs): the four k-lanes of a
            // wave read four adjacent 64-byte pieces
            const uint32_t *g = gs + (((int64_t)tl * nbk + b) * NP) * 16 + r;
            DW[j] = __uint_as_float(g[0]);
            if (HAS_M) MW[j] = __uint_as_float(g[16]);
            if (HAS_H) HB[j] = g[16 * (NP - 1)];
        }
    };

    float acc[NC];
    constexpr int ITEMS = WBLK * NC / 8;           // activation passes of the wave (8 groups of 8 lanes per pass)
    const int t = lane & 7, grp = lane >> 3;
    // prologue: the first item's activations go out FIRST, its weights right behind them
    // (at most XB passes are held in registers at a time: all of them for N <= 2; wider batches fetch the later passes
    // while they quantize the earlier ones)
    constexpr int XB = NC >= 8 ? 2 : (ITEMS < 4 ? ITEMS : 4);
    float4 v[XB], vg[PRO ? XB : 1];
    auto load_x = [&](int w, int p0) {
        const int64_t cb = (int64_t)(w % nchunks) * CH;
        const int nbc = (int)((nbk - cb) < CH ? (nbk - cb) : CH);
#pragma unroll
        for (int pp = 0; pp < XB; ++pp) {
            const int p = p0 + pp;
            const int it = grp + 8 * p, c = it / WBLK, i = it % WBLK;
            const int bl = wave * GV_NKQ + (i & 3) + GV_WORKERS * (i >> 2);        // block of the chunk
            const int cc = c < N ? c : N - 1, blc = bl < nbc ? bl : nbc - 1;
            v[pp] = *(const float4 *)(x + (int64_t)cc * ld1 + (cb + blc) * QK + 4 * t);
            if constexpr (PRO) vg[pp] = *(const float4 *)(pro.g + (int64_t)cc * pro.ld_g + (cb + blc) * QK + 4 * t);
        }
    };
    if constexpr (PRO) {
        // rms_norm's row scale (Ggml.cs:5889-5915): wave c computes row c's, in the element order and f64 tree every kernel
        // shares (common.h rms_row_scale).  The other waves put their first item's loads in flight BEFORE they wait for it,
        // the computing waves right after: the weight stream starts at launch, not behind the norm.
        if (wave < N) {
            const float sc = rms_row_scale(x + (int64_t)wave * ld1, nbk * QK, lane);
            if (lane == 0) sScale[wave] = sc;
        }
        if (nitems > 0) { load_x(0, 0); load_item(0, q, q2, dw, mw, hb); }
        __syncthreads();
    } else {
        if constexpr (!K8) {
            if (nitems > 0) { load_x(0, 0); load_item(0, q, q2, dw, mw, hb); }
        } else {
            const int nsb = (int)(nbk >> 3);                // (K % 256 == 0 for the k-quants)
            // K1's own arrangement (quantize.hip, K8 = true): EIGHT LANES per super-block, lane t holding elements 32 j + 4 t .. + 3 of its eight
            // k-blocks, joined by three DPP steps -- 64 super-blocks per trip of the workgroup (a wave per super-block and six rounds of
            // ds_bpermute shuffles measured 4096 x 4096 x 1 / x 4 6.5 / 12.9 us against the reference types' 4.0 / 6.8).  The first trip's loads
            // go out BEHIND the first item's activations and IN FRONT of its weights (vector-memory results return in issue order).
            const int g8 = tid >> 3, t8 = tid & 7;
            float4 e8[8];
            auto k8_load = [&](int base) {
                const int item = base + g8;
                const int it2 = item < N * nsb ? item : 0;
                const float *src = x + (int64_t)(it2 / nsb) * ld1 + (int64_t)(it2 % nsb) * 256 + 4 * t8;
#pragma unroll
                for (int jb = 0; jb < 8; ++jb) e8[jb] = *(const float4 *)(src + 32 * jb);
            };
            auto k8_reduce = [&](int base) {
                const int item = base + g8;
                float am = 0.0f, mx = 0.0f;
                int ix = 0;                                 // this lane's first element of largest magnitude (element order)
#pragma unroll
                for (int jb = 0; jb < 8; ++jb) {
                    const float e[4] = {e8[jb].x, e8[jb].y, e8[jb].z, e8[jb].w};
#pragma unroll
                    for (int q4 = 0; q4 < 4; ++q4)
                        if (fabsf(e[q4]) > am) { am = fabsf(e[q4]); mx = e[q4]; ix = 32 * jb + 4 * t8 + q4; }
                }
                auto join = [&](float oa, float om, int oi) {   // the larger magnitude wins, equal magnitudes the earlier element
                    const bool take = oa > am || (oa == am && oi < ix);
                    am = take ? oa : am; mx = take ? om : mx; ix = take ? oi : ix;
                };
                join(dpp_f<DPP_XOR1>(am), dpp_f<DPP_XOR1>(mx), dpp_i<DPP_XOR1>(ix));
                join(dpp_f<DPP_XOR2>(am), dpp_f<DPP_XOR2>(mx), dpp_i<DPP_XOR2>(ix));
                join(dpp_f<DPP_HALF_MIRROR>(am), dpp_f<DPP_HALF_MIRROR>(mx), dpp_i<DPP_HALF_MIRROR>(ix));
                const float isc = am != 0.0f ? -128.0f / mx : 0.0f;
                if (t8 == 0 && item < N * nsb) {
                    const int c = item / nsb, sb = item % nsb;
                    sK8[(c * GV_K8_SB + sb) * 2] = isc; sK8[(c * GV_K8_SB + sb) * 2 + 1] = am != 0.0f ? 1.0f / isc : 0.0f;
                }
            };
            if (nitems > 0) load_x(0, 0);
            k8_load(0);
            if (nitems > 0) load_item(0, q, q2, dw, mw, hb);
            k8_reduce(0);
            for (int base = GV_THREADS / 8; base < N * nsb; base += GV_THREADS / 8) { k8_load(base); k8_reduce(base); }
            __syncthreads();
        }
    }

    // one item: INIT arithmetic for this wave's blocks (first item of a single-chunk K, every item otherwise), block dots on
    // the weight registers handed in, and -- on a row tile's last chunk -- the reduction and the store
    auto do_item = [&](int w, const uint4 *Q, const uint4 *Q2, const float *DW, const float *MW, const uint32_t *HB) {
        const int cidx = w % nchunks;
        const int64_t cb = (int64_t)cidx * CH;
        const int nbc = (int)((nbk - cb) < CH ? (nbk - cb) : CH);
        const Sel sel = select(tile_of(w));
        const int tile = sel.tile;
        float *const dst = sel.dst;
        const int64_t M = sel.M, ldd = sel.ldd;
        if (cidx == 0) {
#pragma unroll
            for (int c = 0; c < NC; ++c) acc[c] = 0.0f;
        }
        const bool stage_now = !(single_chunk && staged);
        // 3. INIT phase for this wave's blocks (Ggml.cs:6641-6654 / quantize_row_q8_0 733-762, the arithmetic of K1)
        if (stage_now) {
            if (!single_chunk) __builtin_amdgcn_wave_barrier();   // (the previous chunk's reads of the slice are done: same wave, in order)
#pragma unroll
            for (int p = 0; p < ITEMS; ++p) {
                if (p > 0 && p % XB == 0) load_x(w, p);
                float4 vp = v[p % XB];
                const int it = grp + 8 * p, c = it / WBLK, i = it % WBLK;
                const int bl = wave * GV_NKQ + (i & 3) + GV_WORKERS * (i >> 2);
                const bool live = bl < nbc;                        // uniform over the 8 lanes of the group
                if constexpr (PRO) {
                    const int cc = c < N ? c : N - 1;
                    const float sc = sScale[cc];
                    const float4 gg = vg[p % XB];
                    const float4 nn = make_float4(vp.x * sc, vp.y * sc, vp.z * sc, vp.w * sc);          // the rms_norm node
                    vp = make_float4(nn.x * gg.x, nn.y * gg.y, nn.z * gg.z, nn.w * gg.w);              // the mul node
                    if (blockIdx.x == 0 && live && c < N) {       // both nodes' data, written once (every workgroup computes the same)
                        const int64_t e = (int64_t)c * (nbk * QK) + (cb + bl) * QK + 4 * t;
                        *(float4 *)(pro.n_out + e) = nn;
                        *(float4 *)(pro.y_out + e) = vp;
                    }
                }
                float d, id;
                if constexpr (K8) {                              // the super-block's scale, computed ahead of the items
                    const int cc = c < N ? c : N - 1;
                    const int sbi = (int)((cb + (live ? bl : 0)) >> 3);
                    id = sK8[(cc * GV_K8_SB + sbi) * 2]; d = sK8[(cc * GV_K8_SB + sbi) * 2 + 1];
                    vp = make_float4(fminf(127.0f, rintf(vp.x * id)), fminf(127.0f, rintf(vp.y * id)), fminf(127.0f, rintf(vp.z * id)), fminf(127.0f, rintf(vp.w * id)));
                    id = 1.0f;                                   // (vp holds the quants: x * 1 and the nearest integer of an integer are exact)
                } else {
                    float amax = fmaxf(fmaxf(fabsf(vp.x), fabsf(vp.y)), fmaxf(fabsf(vp.z), fabsf(vp.w)));
                    amax = group8_max(amax);
                    d = amax / 127.0f;                           // Ggml.cs:751
                    id = d != 0.0f ? 1.0f / d : 0.0f;            // Ggml.cs:752
                }
                const int q0 = (int)rintf(vp.x * id), q1 = (int)rintf(vp.y * id);   // Ggml.cs:758-759 (D1, D2)
                const int q2_ = (int)rintf(vp.z * id), q3 = (int)rintf(vp.w * id);
                const int sum = group8_sum(q0 + q1 + q2_ + q3);
                const uint32_t e16 = ((uint32_t)q0 & 0xFFu) | (((uint32_t)q2_ & 0xFFu) << 8);
                const uint32_t o16 = ((uint32_t)q1 & 0xFFu) | (((uint32_t)q3 & 0xFFu) << 8);
                const bool even_lane = (t & 1) == 0;
                const uint32_t recv = (uint32_t)dpp_i<DPP_XOR1>((int)(even_lane ? o16 : e16));
                const uint32_t word = even_lane ? (e16 | (recv << 16)) : (recv | (o16 << 16));
                const int h = even_lane ? 0 : 1, off = even_lane ? 2 * t : 2 * t - 2;
                // a block past the end of K is written as zeros (its weights carry dw = 0; 0 * garbage could be NaN)
                *(uint32_t *)(myq + i * QSLOT + (c * 2 + h) * 16 + off) = live ? word : 0u;
                if (t == 0) { myd[i * NC + c] = live ? d : 0.0f; mys[i * NC + c] = live ? sum : 0; }
            }
            // same wave wrote and reads: LDS operations of one wave complete in order; only the compiler needs the fence
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
            __builtin_amdgcn_wave_barrier();
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
            staged = true;
        }

        // 4. integer block dots + f32 scale-accumulate (Ggml.cs:1136-1159)
#pragma unroll
        for (int j = 0; j < BPL; ++j) {
            const int i = kq + GV_NKQ * j;
            const bool ok = u + GV_WORKERS * j < nbc;
            const float dwj = ok ? DW[j] : 0.0f;          // dw = 0 kills the contribution of a block past the end
            const float mwj = HAS_M && ok ? MW[HAS_M ? j : 0] : 0.0f;
            const uint32_t qq[4] = {Q[j].x, Q[j].y, Q[j].z, Q[j].w};
            uint32_t lo[4], hi[4];
            if (GV_W_I8<TYPE>) {
                lo[0] = Q[j].x; lo[1] = Q[j].y; lo[2] = Q[j].z; lo[3] = Q[j].w;
                hi[0] = Q2[j].x; hi[1] = Q2[j].y; hi[2] = Q2[j].z; hi[3] = Q2[j].w;
            } else {
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    lo[k] = qq[k] & 0x0F0F0F0Fu;          // elements 8k+0,2,4,6  (Ggml.cs:1149)
                    hi[k] = (qq[k] >> 4) & 0x0F0F0F0Fu;   // elements 8k+1,3,5,7  (Ggml.cs:1150)
                    if (HAS_H) {                          // Ggml.cs:1285-1289 / 1330-1334
                        lo[k] |= q5_high_bits(HB[j], k, 0);
                        hi[k] |= q5_high_bits(HB[j], k, 1);
                    }
                    if (TYPE == GGML_TYPE_Q4_2) {         // (nib - 8) bytewise: the two half-block sums need their own offsets
                        lo[k] = ((lo[k] | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
                        hi[k] = ((hi[k] | 0x80808080u) - 0x08080808u) ^ 0x80808080u;
                    }
                }
            }
#pragma unroll
            for (int c = 0; c < NC; ++c) {
                const uint4 a0 = *(const uint4 *)(myq + i * QSLOT + (c * 2 + 0) * 16);
                const uint4 a1 = *(const uint4 *)(myq + i * QSLOT + (c * 2 + 1) * 16);
                const float da = myd[i * NC + c];
                const int sa = mys[i * NC + c];
                if (GV_TWO_SC<TYPE>) {
                    int s0 = 0, s1 = 0;
                    s0 = dot4(lo[0], a0.x, s0); s0 = dot4(lo[1], a0.y, s0); s0 = dot4(hi[0], a1.x, s0); s0 = dot4(hi[1], a1.y, s0);
                    s1 = dot4(lo[2], a0.z, s1); s1 = dot4(lo[3], a0.w, s1); s1 = dot4(hi[2], a1.z, s1); s1 = dot4(hi[3], a1.w, s1);
                    acc[c] = fmaf(dwj * da, (float)s0, acc[c]);
                    acc[c] = fmaf(mwj * da, (float)s1, acc[c]);
                    continue;
                }
                int sdot = 0;
                sdot = dot4(lo[0], a0.x, sdot); sdot = dot4(lo[1], a0.y, sdot); sdot = dot4(lo[2], a0.z, sdot); sdot = dot4(lo[3], a0.w, sdot);
                sdot = dot4(hi[0], a1.x, sdot); sdot = dot4(hi[1], a1.y, sdot); sdot = dot4(hi[2], a1.z, sdot); sdot = dot4(hi[3], a1.w, sdot);
                if (TYPE == GGML_TYPE_Q4_0) sdot -= 8 * sa;   // (nib - 8) * a summed = nib*a summed - 8 * sum(a)
                if (TYPE == GGML_TYPE_Q5_0) sdot -= 16 * sa;
                acc[c] = fmaf(dwj * da, (float)sdot, acc[c]);
                if (TYPE == GGML_TYPE_Q4_1 || TYPE == GGML_TYPE_Q5_1) acc[c] = fmaf(mwj, da * (float)sa, acc[c]);   // + m * (s0 + s1)
            }
        }
        if (cidx != nchunks - 1) return;                // the row tile's last chunk: reduce and store below

        // 5. k-lanes by two xor-shuffles, waves through LDS: the fixed tree of the kernel above.  sRed alternates between two
        //    buffers, so ONE barrier per tile orders everything (tile t+2's writes come after tile t+1's barrier, which every
        //    wave reaches only after its tile-t reads)
#pragma unroll
        for (int c = 0; c < NC; ++c) {
            float vsum = acc[c];
#pragma unroll
            for (int sft = GV_ROWS; sft < 64; sft <<= 1) vsum += __shfl_xor(vsum, sft);
            if (kq == 0) sRed[parity][wave][c][r] = vsum;
        }
        __syncthreads();
        for (int o = tid; o < GV_ROWS * NC; o += GV_THREADS) {
            const int c = o / GV_ROWS, rr = o % GV_ROWS;
            const int64_t m = (int64_t)tile * GV_ROWS + rr;
            float quad[GV_WAVES / 4];                                                                   // fixed tree over the waves
#pragma unroll
            for (int qd = 0; qd < GV_WAVES / 4; ++qd)
                quad[qd] = (sRed[parity][4 * qd][c][rr] + sRed[parity][4 * qd + 1][c][rr]) + (sRed[parity][4 * qd + 2][c][rr] + sRed[parity][4 * qd + 3][c][rr]);
            const float tot = GV_WAVES == 4 ? quad[0] : GV_WAVES == 8 ? quad[0] + quad[1 % (GV_WAVES / 4)]
                                            : (quad[0] + quad[1 % (GV_WAVES / 4)]) + (quad[2 % (GV_WAVES / 4)] + quad[3 % (GV_WAVES / 4)]);
            if (m < M && c < N) {
                // the node that follows the mul_mat, applied as the product is stored (common.h mm_epilogue)
                st_result(dst + (int64_t)c * ldd + m, ep.mode == 2 ? tot * ep.scale : tot);
                if (ep.mode == 1) st_result(ep.dst2 + (int64_t)c * ep.ld2 + m, tot + ep.addend[(int64_t)c * ep.ld_add + m]);
            }
        }
        parity ^= 1;
    };

    if constexpr (PF) {
        // The look-ahead pays where a workgroup walks several row tiles of one chunk (4096 x 4096: 5.06 -> 4.66 us, M = 32000:
        // 19.3 -> 18.7).  Two register sets take turns (the loop is unrolled by two items): a copy "current = next" at the end
        // of an item would make the wave wait for the look-ahead data THERE, i.e. drain the memory pipe once per row tile.
        // The steady-state loop issues its look-ahead loads UNCONDITIONALLY (a load sequence behind a branch makes hipcc's
        // wait counts assume the worst of both paths: every wait for the current set then also waited for half of the set
        // just requested); the last one or two items run below it.
        int w = 0;
        for (; w + 2 < nitems; w += 2) {
            load_item(w + 1, qn, q2n, dwn, mwn, hbn);                          // the NEXT item's weight stream goes out first
            do_item(w, q, q2, dw, mw, hb);
            load_item(w + 2, q, q2, dw, mw, hb);
            do_item(w + 1, qn, q2n, dwn, mwn, hbn);
        }
        if (w + 1 < nitems) {
            load_item(w + 1, qn, q2n, dwn, mwn, hbn);
            do_item(w, q, q2, dw, mw, hb);
            do_item(w + 1, qn, q2n, dwn, mwn, hbn);
        } else if (w < nitems) {
            do_item(w, q, q2, dw, mw, hb);
        }
    } else {
        // with K in several chunks the activations of every item have to be fetched and quantized as well, and asking for them
        // first, weights behind, in the item's own iteration measured better -- again with the two-set look-ahead of the
        // single-chunk form extended to the activations (4096 x 11008: 8.1 against 8.7 us, 11008 x 11008: 16.5 against 18.1),
        // and against ONE chunk of 384 k-blocks (all 11 block loads of a lane at once, same bits: any chunk size that is a
        // multiple of 32 leaves a lane's block sequence alone): 4096 x 11008 9.4 us, 4096 x 8192 8.8 against 6.6
        for (int w = 0; w < nitems; ++w) {
            if (w > 0) {
                if (!(single_chunk && staged)) load_x(w, 0);
                load_item(w, q, q2, dw, mw, hb);
            }
            do_item(w, q, q2, dw, mw, hb);
        }
    }
}
