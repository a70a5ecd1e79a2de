// seams.cpp -- the C-ABI of include/ggml_hip.h, part 2: the host-pointer seams.
//   Seam 1  ggml_compute_forward_mul_mat (Ggml.cs:6714-6744): pipelined host -> device / kernels / device -> host on
//           three streams per device slot, row-split over the slots the caller is not bound away from, its operands and
//           result resident inside a graph scope (scope.cpp), its weights from the cache (wcache.cpp);
//   its neighbours: cpy -> Q, add (q + f32, f32 + f32), mul, scale, rms_norm, silu, and the fused forms.
#include "ctx.h"

namespace ghip {
namespace {

// every writer of host tensor memory: weight-cache entries built from it and other resident copies overlapping it are stale
void note_host_write(Call &call, const ggml_tensor *dst, bool keep_exact_resident) {
    const size_t bytes = tensor_host_bytes(dst);
    for (DeviceCtx *c : call.ctxs) {
        c->invalidate(dst->data, bytes);
        c->drop_overlapping(dst->data, bytes, keep_exact_resident);
    }
}

// device pointer of a contiguous f32 operand on slot c: its resident copy if an earlier node of this graph produced it,
// else an upload from host memory into `scratch` on the slot's compute stream
int operand_f32(DeviceCtx *c, bool in_graph, const ggml_tensor *t, Scratch &scratch, const float **out) {
    const size_t bytes = (size_t)nelem(t) * 4;
    if (in_graph) {
        const void *r = c->resident_lookup(t->data, bytes);
        if (r) { *out = (const float *)r; ++c->resident_hits; return 0; }
        if (c->before_host_read(t->data, bytes)) return -1;   // host memory may be owed an earlier node's result, or still receiving it
        // the upload stays resident for the rest of the scope: a leaf used by several nodes (the residual stream) moves once
        void *keep = c->resident_buffer(t->data, bytes);
        if (!keep) return -1;
        if (!host_range_pinned(t->data, bytes)) c->scope_dirty();   // a copy from pageable memory is staged by the runtime: not something a capture may hold
        c->note_leaf(t->data, bytes);
        if (hipMemcpyAsync(keep, t->data, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return -1;
        c->h2d_bytes += bytes;
        *out = (const float *)keep;
        return 0;
    }
    if (scratch.ensure(bytes)) return -1;
    if (hipMemcpyAsync(scratch.p, t->data, bytes, hipMemcpyHostToDevice, c->stream) != hipSuccess) return -1;
    c->h2d_bytes += bytes;
    *out = (const float *)scratch.p;
    return 0;
}
// device buffer for a contiguous f32 result: kept resident inside a graph scope (in place when dst shares src's data)
float *result_f32(DeviceCtx *c, bool in_graph, const ggml_tensor *t, Scratch &scratch) {
    const size_t bytes = (size_t)nelem(t) * 4;
    if (in_graph) return (float *)c->resident_buffer(t->data, bytes);
    return scratch.ensure(bytes) ? nullptr : (float *)scratch.p;
}
int finish_f32(DeviceCtx *c, bool in_graph, bool to_host, ggml_tensor *t, const float *dev) {
    const size_t bytes = (size_t)nelem(t) * 4;
    if (to_host && in_graph) {
        c->owe(t->data, dev, bytes);        // (dev is the tensor's resident buffer: result_f32)
    } else if (to_host) {
        if (hipMemcpyAsync(t->data, dev, bytes, hipMemcpyDeviceToHost, c->stream) != hipSuccess) return -1;
        c->d2h_bytes += bytes;
    }
    if (!in_graph && hipStreamSynchronize(c->stream) != hipSuccess) return -1;
    return 0;
}
// the slots an element-wise node runs on: all of them inside a graph scope (every slot then holds every resident
// tensor, so a later row-split mul_mat finds its src1 in its own HBM), the first one otherwise
int eltwise_slots(const Call &call) { return call.in_graph() ? call.G() : 1; }

// The body of every element-wise seam: up to two contiguous f32 inputs, up to two contiguous f32 outputs (checked by the caller), on every slot
// of eltwise_slots.  launch(c, in_graph, first, in, out) issues the node's kernel(s) on c->stream for the device pointers in[] / out[], `first`
// on the slot whose results go to host memory, and returns a status; the LAST output's way home is the driver's (finish_f32).
template <class Launch>
int eltwise_seam(const char *name, std::initializer_list<const ggml_tensor *> inputs, std::initializer_list<ggml_tensor *> outputs, Launch launch) {
    Call call;
    int rc = call.begin();
    if (rc) return rc;
    const bool in_graph = call.in_graph();
    const int ns = eltwise_slots(call);
    for (int g = 0; g < ns; ++g) {
        DeviceCtx *c = call.ctxs[(size_t)g];
        rc = c->make_current();
        if (rc) return rc;
        Scratch *const in_scratch[2] = {&c->src1, &c->stage}, *const out_scratch[2] = {&c->dst, &c->dst2};
        const float *in[2] = {nullptr, nullptr};
        float *out[2] = {nullptr, nullptr};
        int i = 0;
        for (const ggml_tensor *t : inputs)
            if (operand_f32(c, in_graph, t, *in_scratch[i], &in[i])) return fail(GGML_HIP_ERR_RUNTIME, "%s: operand staging failed", name);
            else ++i;
        if (g == 0)                                  // (after the operands were resolved: an output may alias one of them)
            for (ggml_tensor *t : outputs) note_host_write(call, t, true);
        bool ok = true;
        i = 0;
        for (ggml_tensor *t : outputs) { out[i] = result_f32(c, in_graph, t, *out_scratch[i]); ok = ok && out[i]; ++i; }
        if (!ok) return fail(GGML_HIP_ERR_RUNTIME, "%s: hipMalloc failed", name);
        rc = launch(c, in_graph, g == 0, in, out);
        if (rc) return rc;
        if (finish_f32(c, in_graph, g == 0, *(outputs.end() - 1), out[i - 1])) return fail(GGML_HIP_ERR_RUNTIME, "%s: copy back failed", name);
    }
    return GGML_HIP_OK;
}

// Seam-1 pipeline: src1 rows per chunk.  A function of N and K only (never of M or the slot count), so a row shard and the
// unsplit matrix run the same kernel forms on the same chunks: bit-identical results for any split.
#ifndef SEAM_MIN_CHUNK
#define SEAM_MIN_CHUNK 128            // (A/B 256 / 512 rows: 4096 x 4096 x 512 0.349 -> 0.365 / 0.373 ms, x 4096 1.71 -> 1.76 / 1.73: no gain)
#endif
int64_t seam_chunk_rows(int64_t N, int64_t K, bool pinned) {
    if (!pinned) return N;                              // pageable memory: the runtime stages synchronously, nothing overlaps
    const int64_t x_bytes = N * K * 4;
    if (N < 128 || x_bytes < (2ll << 20)) return N;
    // what the pipeline cannot hide is its fill and drain -- the first chunk's upload and the last chunk's download -- but
    // every chunk costs the host ~10 runtime calls and each DMA its launch latency: N / 8 rows per chunk, at least 128
    // (measured on MI355X / PCIe 5, 4096 x 4096 x {4096, 512}: 8 chunks 1.71 / 0.36 ms (two chunks at 512), 16 chunks 1.75 / 0.39 ms;
    // the box moves 94 GB/s with both directions busy: 1.42 ms for the 134 MB of the first shape)
    int64_t rows = ((N + 7) / 8 + 31) / 32 * 32;
    if (rows < SEAM_MIN_CHUNK) rows = SEAM_MIN_CHUNK;
    return rows;
}

// ---------------- the Seam-1 pipeline of one 2-D slice on one slot ----------------
struct PipeArgs {
    const ggml_hip_weight *w;
    const uint8_t *x_host; uint64_t nb11;          // src1 rows on the host (ignored when x is resident)
    uint8_t *d_host; uint64_t nb1;                 // dst rows on the host
    const float *xd; bool upload = false;          // src1 on the device (+ whether it has to be uploaded first)
    float *dd; int64_t ldd;                        // dst on the device: base (already at this slot's column) and row stride
    int64_t N, K, Ms, col0, chunk;
    void *work; size_t work_cap;
    // the node that follows the mul_mat, fused into its kernels (common.h mm_epilogue); mode 0 = none
    int epi_mode = 0;
    const float *addend = nullptr;                 // [N][Ms] on the device (mode 1)
    float *dst2 = nullptr; uint8_t *d2_host = nullptr; uint64_t nb1_2 = 0;   // the add node's result, device and host
    float scale = 1.0f;                            // mode 2
    bool owe_dst = false;                          // graph scope, outputs-only: dst is resident and the caller does not want it -- owed, not copied
    // the rms_norm -> mul pair in front of the mul_mat, computed by the mat-vec's prologue (common.h mm_prologue): src1 IS the
    // mul node; x / g are its inputs on the device, pro_n / pro_y receive both nodes' results ([N][K]), n_host / y_host their tensors
    const float *pro_x = nullptr, *pro_g = nullptr;
    float *pro_n = nullptr, *pro_y = nullptr;
    uint8_t *n_host = nullptr, *y_host = nullptr;
};

// the kernels of src1 rows [r, r + n) on the compute stream
int launch_rows(DeviceCtx *c, const PipeArgs &a, int64_t r, int64_t n) {
    if (a.pro_x)        // (a prologue call is a single chunk: N <= 4)
        return ggml_hip_norm_mul_mat_dev(a.w, a.pro_x, a.K, a.pro_g, a.K, n, a.pro_n, a.pro_y, a.dd, a.ldd, a.work, a.work_cap, a.epi_mode, a.addend, a.Ms,
                                         a.dst2, a.Ms, a.scale, c->stream);
    return ggml_hip_mul_mat_epilogue_dev(a.w, a.xd + (size_t)r * a.K, n, a.K, a.dd + (size_t)r * a.ldd, a.ldd, a.work, a.work_cap, a.epi_mode,
                                         a.addend ? a.addend + (size_t)r * a.Ms : nullptr, a.Ms, a.dst2 ? a.dst2 + (size_t)r * a.Ms : nullptr, a.Ms,
                                         a.scale, c->stream);
}

// H2D of chunk k on s_h2d | INIT + COMPUTE of chunk k on stream | D2H of chunk k on s_d2h, chained by events.
int issue_chunks(DeviceCtx *c, const PipeArgs &a) {
    hipError_t e = hipSuccess;
    // fork: uploads wait for everything issued so far on the compute stream (earlier kernels may still read the src1 scratch)
    e = hipEventRecord(c->ev_compute, c->stream);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->s_h2d, c->ev_compute, 0);
    int k = 0;
    for (int64_t r = 0; r < a.N && e == hipSuccess; r += a.chunk, ++k) {
        const int64_t n = a.N - r < a.chunk ? a.N - r : a.chunk;
        const int ke = k % PIPE_EVENTS;
        if (a.upload) {
            if (a.nb11 == (uint64_t)a.K * 4)      // contiguous rows: one linear DMA
                e = hipMemcpyAsync((uint8_t *)a.xd + (size_t)r * a.K * 4, a.x_host + (size_t)r * a.nb11, (size_t)n * a.K * 4, hipMemcpyHostToDevice, c->s_h2d);
            else
                e = hipMemcpy2DAsync((uint8_t *)a.xd + (size_t)r * a.K * 4, (size_t)a.K * 4, a.x_host + (size_t)r * a.nb11, a.nb11, (size_t)a.K * 4,
                                     (size_t)n, hipMemcpyHostToDevice, c->s_h2d);
            if (e == hipSuccess) e = hipEventRecord(c->ev_in[ke], c->s_h2d);
            if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_in[ke], 0);
            if (e != hipSuccess) break;
        }
        const int rc = launch_rows(c, a, r, n);
        if (rc) return rc;
        if (a.owe_dst) continue;
        e = hipEventRecord(c->ev_k[ke], c->stream);
        if (e == hipSuccess) e = hipStreamWaitEvent(c->s_d2h, c->ev_k[ke], 0);
        if (e == hipSuccess) {
            if (a.nb1 == (uint64_t)a.Ms * 4 && a.ldd == a.Ms)    // whole contiguous rows (one slot): one linear DMA
                e = hipMemcpyAsync(a.d_host + (size_t)r * a.nb1, a.dd + (size_t)r * a.ldd, (size_t)n * a.Ms * 4, hipMemcpyDeviceToHost, c->s_d2h);
            else
                e = hipMemcpy2DAsync(a.d_host + (size_t)r * a.nb1 + (size_t)a.col0 * 4, a.nb1, a.dd + (size_t)r * a.ldd, (size_t)a.ldd * 4,
                                     (size_t)a.Ms * 4, (size_t)n, hipMemcpyDeviceToHost, c->s_d2h);
            if (e == hipSuccess && a.epi_mode == 1)             // the add node's data goes to the host too (contiguous rows)
                e = hipMemcpyAsync(a.d2_host + (size_t)r * a.nb1_2, a.dst2 + (size_t)r * a.Ms, (size_t)n * a.Ms * 4, hipMemcpyDeviceToHost, c->s_d2h);
            if (e == hipSuccess && a.pro_x) {                    // ... and so do the norm and the mul node's
                e = hipMemcpyAsync(a.n_host, a.pro_n, (size_t)n * a.K * 4, hipMemcpyDeviceToHost, c->s_d2h);
                if (e == hipSuccess) e = hipMemcpyAsync(a.y_host, a.pro_y, (size_t)n * a.K * 4, hipMemcpyDeviceToHost, c->s_d2h);
            }
        }
    }
    if (e != hipSuccess) return fail(GGML_HIP_ERR_RUNTIME, "seam 1 pipeline: %s", hipGetErrorString(e));
    return GGML_HIP_OK;
}

// (Capturing a recurring pipeline into a hipGraph and replaying it with one launch was built and measured: the replay runs
// the copy and kernel branches one after the other -- 4096 x 4096 x 4096 3.10 ms against 1.75 ms for the three live
// streams, x 512 0.66 against 0.39 -- so the pipeline is always issued directly.  Results going home by kernel stores through
// the pool's device mapping instead of the DMA engine were measured as well: a copy kernel per chunk 2.08 / 0.45 ms, the
// mat-mat epilogue storing straight into the mapping 1.92 / 0.40 ms, against 1.72 / 0.35 ms -- the DMA engines stay.)
int run_pipeline(DeviceCtx *c, const PipeArgs &a) {
    // order against work issued earlier on the copy streams (they read / write the scratch buffers this call reuses)
    hipError_t e = hipEventRecord(c->ev_d2h, c->s_d2h);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_d2h, 0);
    if (e == hipSuccess) e = hipEventRecord(c->ev_xchg, c->s_h2d);
    if (e == hipSuccess) e = hipStreamWaitEvent(c->stream, c->ev_xchg, 0);
    if (e != hipSuccess) return fail(GGML_HIP_ERR_RUNTIME, "seam 1 pipeline: %s", hipGetErrorString(e));
    if (a.upload) c->h2d_bytes += (size_t)a.N * a.K * 4;
    c->d2h_busy = true;
    c->d2h_bytes += (size_t)a.N * a.Ms * 4 * (a.epi_mode == 1 ? 2 : 1) + (a.pro_x ? (size_t)a.N * a.K * 8 : 0);
    return issue_chunks(c, a);
}

}  // namespace
}  // namespace ghip

using namespace ghip;

extern "C" {

// inside a replayed graph scope the seams have nothing to do: ggml_hip_graph_end launches the captured scope
static bool scope_replaying() {
    const int b = bound_slot();
    DeviceCtx *c = slot(b >= 0 ? b : 0);
    if (!c) return false;
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    return !c->dead && c->scope_mode == 3 && c->scope_owner == std::this_thread::get_id();
}
// a node seam has nothing to do for the other threads and phases of a node -- the offload convention of the reference's own dead GPU
// blocks (Ggml.cs:6510-6521) -- nor inside a replayed scope
static bool seam_idle(const struct ggml_compute_params *params) {
    return params->ith != 0 || params->type != GGML_TASK_COMPUTE || scope_replaying();
}

struct SeamEpi {                                    // the node after the mul_mat (fused seams below); mode as in mm_epilogue
    int mode;
    const struct ggml_tensor *addend;               // mode 1: the other operand of the add node
    struct ggml_tensor *add_dst;                    //         and that node
    float scale;                                    // mode 2
    // prologue (rms_norm -> mul in front): src1 of the call is the mul node; these are the pair's operands and the norm node
    const struct ggml_tensor *pro_x = nullptr, *pro_g = nullptr;
    struct ggml_tensor *pro_norm = nullptr;
};
static const int SEAM_NOT_FUSABLE = 1;              // (internal) the caller runs the two seams one after the other

/* Seam 1.  Checks mirror the Debug.Asserts of the three drivers (Ggml.cs:6026-6046, 6222-6241, 6477-6504) and of
 * ggml_mul_mat_impl (Ggml.cs:8228-8229); the reference silently drops them in Release, here they are errors.  No device is touched. */
static int seam1_check(const struct ggml_tensor *src0, const struct ggml_tensor *src1, const struct ggml_tensor *dst) {
    const int type = src0->type;
    if (type < 0 || type >= GGML_TYPE_COUNT || !weight_type_ok(type))
        return fail(GGML_HIP_ERR_TYPE, "src0 type %d unsupported (Q4_3/Q8_1 null slots; Q4_2/Q5_1 broken storage, SURVEY D7/D8)", type);
    if (src1->type != GGML_TYPE_F32 || dst->type != GGML_TYPE_F32) return fail(GGML_HIP_ERR_TYPE, "src1 and dst must be F32");
    const int64_t ne00 = src0->ne[0], ne01 = src0->ne[1], ne02 = src0->ne[2], ne03 = src0->ne[3];
    const int64_t ne10 = src1->ne[0], ne11 = src1->ne[1], ne12 = src1->ne[2], ne13 = src1->ne[3];
    if (ne00 != ne10 || ne02 != ne12 || ne03 != ne13) return fail(GGML_HIP_ERR_SHAPE, "!ggml_can_mul_mat (Ggml.cs:8345-8353)");
    if (dst->ne[0] != ne01 || dst->ne[1] != ne11 || dst->ne[2] != ne02 || dst->ne[3] != ne03)
        return fail(GGML_HIP_ERR_SHAPE, "dst shape (Ggml.cs:6488-6491)");
    if (src0->nb[0] != TSIZE[type]) return fail(GGML_HIP_ERR_SHAPE, "permuted src0 (Ggml.cs:6477)");
    if (src0->nb[0] > src0->nb[1]) return fail(GGML_HIP_ERR_SHAPE, "transposed src0 (Ggml.cs:8229)");
    if (src1->nb[0] != 4) return fail(GGML_HIP_ERR_SHAPE, "permuted src1 (Ggml.cs:6478)");
    if (dst->nb[0] != 4 || dst->nb[0] > dst->nb[1] || dst->nb[1] > dst->nb[2] || dst->nb[2] > dst->nb[3])
        return fail(GGML_HIP_ERR_SHAPE, "dst transposed or permuted (Ggml.cs:6481-6484)");
    if (ne00 % BLCK[type] != 0) return fail(GGML_HIP_ERR_SHAPE, "ne00 %% 32 != 0 (Ggml.cs:6694)");
    if (src1->nb[1] % 4 != 0 || dst->nb[1] % 4 != 0) return fail(GGML_HIP_ERR_SHAPE, "row strides must be multiples of 4");
    if (!src0->data || !src1->data || !dst->data) return fail(GGML_HIP_ERR_ARG, "null data");
    return GGML_HIP_OK;
}

// a neighbour is fused when one slot serves one 2-D slice with contiguous f32 tensors of dst's shape; anything else: two seams
static bool epi_fusable(int G, const ggml_tensor *src0, const ggml_tensor *src1, const ggml_tensor *dst, const SeamEpi &epi) {
    const int64_t ne01 = src0->ne[1], ne10 = src1->ne[0], ne11 = src1->ne[1];
    bool ok = G == 1 && src0->ne[2] * src0->ne[3] == 1 && dst->nb[1] == (uint64_t)ne01 * 4;
    if (ok && epi.mode == 1) {
        const ggml_tensor *a = epi.addend, *d2 = epi.add_dst;
        ok = a && d2 && a->data && d2->data && contiguous_f32(a) && contiguous_f32(d2) && a->ne[0] == ne01 && a->ne[1] == ne11 &&
             a->ne[2] == 1 && a->ne[3] == 1 && d2->ne[0] == ne01 && d2->ne[1] == ne11 && d2->ne[2] == 1 && d2->ne[3] == 1 && d2->data != dst->data;
    }
    if (ok && epi.pro_x) {    // the prologue form: the fused mat-vec only (N <= 4), contiguous [K, N] operands
        const ggml_tensor *ts[3] = {epi.pro_x, epi.pro_g, epi.pro_norm};
        ok = ne11 <= 4 && is_q(src0->type) && contiguous_f32(src1);
        for (const ggml_tensor *t : ts)
            ok = ok && t && t->data && contiguous_f32(t) && t->ne[0] == ne10 && t->ne[1] == ne11 && t->ne[2] == 1 && t->ne[3] == 1;
        ok = ok && epi.pro_norm->data != src1->data && epi.pro_norm->data != dst->data;
    }
    return ok;
}

// the fused neighbours' device side (slot 0: they are fused on one slot only)
struct Staged {
    const float *addend = nullptr; float *dst2 = nullptr;          // the add node's other operand and its result buffer
    const float *pro_x = nullptr, *pro_g = nullptr;                // the norm -> mul pair's operands
    float *pro_n = nullptr, *pro_y = nullptr;                      // and both nodes' result buffers
};
static int stage_epilogue(Call &call, const SeamEpi &epi, Staged *st) {
    DeviceCtx *c = call.ctxs[0];
    const bool in_graph = call.in_graph();
    if (operand_f32(c, in_graph, epi.addend, c->stage, &st->addend)) return fail(GGML_HIP_ERR_RUNTIME, "mul_mat + add: operand staging failed");
    note_host_write(call, epi.add_dst, true);
    st->dst2 = result_f32(c, in_graph, epi.add_dst, c->dst2);
    return st->dst2 ? GGML_HIP_OK : fail(GGML_HIP_ERR_RUNTIME, "mul_mat + add: hipMalloc failed");
}
// (`mul` is the mul node: the src1 of the products behind the pair)
static int stage_prologue(Call &call, const char *name, const ggml_tensor *x, const ggml_tensor *g, const ggml_tensor *norm, const ggml_tensor *mul, Staged *st) {
    DeviceCtx *c = call.ctxs[0];
    const bool in_graph = call.in_graph();
    if (operand_f32(c, in_graph, x, c->aux[0], &st->pro_x) || operand_f32(c, in_graph, g, c->aux[1], &st->pro_g))
        return fail(GGML_HIP_ERR_RUNTIME, "%s: operand staging failed", name);
    note_host_write(call, norm, true);
    note_host_write(call, mul, true);
    st->pro_n = result_f32(c, in_graph, norm, c->aux[2]);
    st->pro_y = result_f32(c, in_graph, mul, c->aux[3]);
    return st->pro_n && st->pro_y ? GGML_HIP_OK : fail(GGML_HIP_ERR_RUNTIME, "%s: hipMalloc failed", name);
}

struct Seam1 {                                      // what the stages of one call share, filled once
    const ggml_tensor *src0, *src1;
    ggml_tensor *dst;
    const SeamEpi *epi;
    int G;
    bool in_graph;
    int64_t ne00, ne01, ne02, ne03, ne11, nslice;   // (ne10 == ne00, ne12 == ne02, ne13 == ne03: seam1_check)
    size_t x_bytes, d_full, w_bytes;                // one slice of src1 and of dst; the kernels' work buffer
    bool src1_contig, dst_contig, pinned, cacheable;
    int64_t chunk;
    Staged st;
    bool pro() const { return epi && epi->pro_x; }
    int mode() const { return epi ? epi->mode : 0; }
    float scale() const { return epi ? epi->scale : 1.0f; }
    Seam1(const Call &call, const ggml_tensor *src0_, const ggml_tensor *src1_, ggml_tensor *dst_, const SeamEpi *epi_)
        : src0(src0_), src1(src1_), dst(dst_), epi(epi_), G(call.G()), in_graph(call.in_graph()) {
        ne00 = src0->ne[0]; ne01 = src0->ne[1]; ne02 = src0->ne[2]; ne03 = src0->ne[3]; ne11 = src1->ne[1];
        nslice = ne02 * ne03;
        x_bytes = (size_t)ne11 * ne00 * 4; d_full = (size_t)ne11 * ne01 * 4;
        w_bytes = ggml_hip_mul_mat_work_size(src0->type, ne00, ne11);
        src1_contig = src1->nb[1] == (uint64_t)ne00 * 4 && src1->nb[2] == src1->nb[1] * (uint64_t)ne11 && src1->nb[3] == src1->nb[2] * (uint64_t)ne02;
        dst_contig = dst->nb[1] == (uint64_t)ne01 * 4 && dst->nb[2] == dst->nb[1] * (uint64_t)ne11 && dst->nb[3] == dst->nb[2] * (uint64_t)ne02;
        pinned = host_range_pinned(src1->data, tensor_host_bytes(src1)) && host_range_pinned(dst->data, tensor_host_bytes(dst));
        chunk = seam_chunk_rows(ne11, ne00, pinned);
        // a src0 that some node computes (or that is a leaf the host rewrites between computes without telling us) must not be
        // served from the cache: only leaves are cached, and every seam that writes host memory invalidates what overlaps it
        cacheable = src0->op == GGML_OP_NONE;
    }
};

struct Seam1Slot {                                  // one slot's share of a call
    DeviceCtx *c = nullptr;
    std::vector<ggml_hip_weight *> W;               // [slice]: rows [r0, r1) of src0
    const uint8_t *x_res = nullptr;                 // graph scope: src1 is the (contiguous) dst of an earlier offloaded node, in HBM
    uint8_t *d_res = nullptr;                       // graph scope, contiguous dst: the [N][M] copy kept for the nodes that follow
    int64_t r0 = 0, r1 = 0, Ms = 0;
};
// weights computed for this call alone (a computed src0 outside a graph scope): freed when the call is over
struct OwnedWeights {
    std::vector<ggml_hip_weight *> w;
    ~OwnedWeights() { for (ggml_hip_weight *x : w) ggml_hip_weight_free(x); }
};
static int seam1_slot(const Seam1 &s, DeviceCtx *c, int g, OwnedWeights *owned, Seam1Slot *p) {
    int rc = c->make_current();
    if (rc) return rc;
    p->c = c;
    shard_rows(s.ne01, s.G, g, &p->r0, &p->r1);
    p->Ms = p->r1 - p->r0;
    rc = c->acquire_weights(s.src0, p->r0, p->r1, s.cacheable, s.in_graph, &p->W, &owned->w);
    if (rc) return rc;
    if (s.in_graph && s.src1_contig) {
        p->x_res = (const uint8_t *)c->resident_lookup(s.src1->data, s.x_bytes * (size_t)s.nslice);
        if (p->x_res) ++c->resident_hits;
    }
    if (s.in_graph && s.dst_contig) {
        p->d_res = (uint8_t *)c->resident_buffer(s.dst->data, s.d_full * (size_t)s.nslice);
        if (!p->d_res) return fail(GGML_HIP_ERR_RUNTIME, "hipMalloc failed for a resident dst");
    }
    if ((!p->x_res && c->src1.ensure(s.x_bytes)) || (!p->d_res && c->dst.ensure((size_t)s.ne11 * (size_t)(p->Ms > 0 ? p->Ms : 1) * 4)) ||
        c->work.ensure(s.w_bytes ? s.w_bytes : 16))
        return fail(GGML_HIP_ERR_RUNTIME, "hipMalloc failed for scratch");
    return GGML_HIP_OK;
}

// one 2-D slice on one slot (slice offsets as in Ggml.cs:6566-6570): everything of PipeArgs but how src1 gets there and dst gets home
static PipeArgs slice_args(const Seam1 &s, const Seam1Slot &p, int64_t i02, int64_t i03) {
    const size_t sl = (size_t)(i03 * s.ne02 + i02);
    PipeArgs pa;
    pa.w = p.W[sl];
    pa.x_host = (const uint8_t *)s.src1->data + i02 * s.src1->nb[2] + i03 * s.src1->nb[3]; pa.nb11 = s.src1->nb[1];
    pa.d_host = (uint8_t *)s.dst->data + i02 * s.dst->nb[2] + i03 * s.dst->nb[3]; pa.nb1 = s.dst->nb[1];
    pa.xd = p.x_res ? (const float *)(p.x_res + sl * s.x_bytes) : (const float *)p.c->src1.p;
    // device dst: this slot's columns of the resident [N][M] copy, or a [N][Ms] scratch shard
    pa.dd = p.d_res ? (float *)(p.d_res + sl * s.d_full) + p.r0 : (float *)p.c->dst.p;
    pa.ldd = p.d_res ? s.ne01 : p.Ms;
    pa.N = s.ne11; pa.K = s.ne00; pa.Ms = p.Ms; pa.col0 = p.r0; pa.chunk = s.chunk;
    pa.work = p.c->work.p; pa.work_cap = p.c->work.cap;
    pa.epi_mode = s.mode(); pa.scale = s.scale();
    if (s.mode() == 1) { pa.addend = s.st.addend; pa.dst2 = s.st.dst2; pa.d2_host = (uint8_t *)s.epi->add_dst->data; pa.nb1_2 = s.epi->add_dst->nb[1]; }
    if (s.pro()) {
        pa.pro_x = s.st.pro_x; pa.pro_g = s.st.pro_g; pa.pro_n = s.st.pro_n; pa.pro_y = s.st.pro_y;
        pa.n_host = (uint8_t *)s.epi->pro_norm->data; pa.y_host = (uint8_t *)s.src1->data;
    }
    return pa;
}

// one slot keeps dst resident (d_res: a graph scope, a contiguous dst): its way home can be owed to the scope
static bool dst_kept(const Seam1 &s, const Seam1Slot &p) { return s.in_graph && s.G == 1 && p.d_res; }
// Graph scope, one slot, one chunk, dst kept resident: the node is its kernels on the compute stream and
// nothing else -- no fork / join over the copy streams, no device -> host copy of its own (DeviceCtx::owe:
// the host copies of a scope's results go out together).  17 nodes of a 7B decoder layer at batch 1:
// 439 -> see DESIGN 8 us per graph compute.
// (a batch of any size when src1 is already in HBM: there is no upload for chunks to overlap; the result's way
// home overlaps the NEXT nodes' kernels -- DeviceCtx::owe sends a large one at once on the copy stream)
static bool runs_resident(const Seam1 &s, const Seam1Slot &p) {
    return dst_kept(s, p) && (p.x_res || s.pro() || (s.ne11 <= s.chunk && s.src1->nb[1] == (uint64_t)s.ne00 * 4));
}
static int run_resident(const Seam1 &s, const Seam1Slot &p, const PipeArgs &pa) {
    DeviceCtx *c = p.c;
    if (!p.x_res && !s.pro()) {
        if (!s.pinned) c->scope_dirty();
        if (s.nslice == 1) c->note_leaf(s.src1->data, s.x_bytes);
        const hipError_t e = hipMemcpyAsync(c->src1.p, pa.x_host, s.x_bytes, hipMemcpyHostToDevice, c->stream);
        if (e != hipSuccess) return fail(GGML_HIP_ERR_RUNTIME, "seam 1: %s", hipGetErrorString(e));
        c->h2d_bytes += s.x_bytes;
    }
    const int rc = launch_rows(c, pa, 0, pa.N);
    if (rc) return rc;
    c->owe(pa.d_host, pa.dd, s.d_full);
    if (pa.epi_mode == 1) c->owe(pa.d2_host, pa.dst2, s.d_full);
    if (s.pro()) {
        c->owe(pa.n_host, pa.pro_n, s.x_bytes);
        c->owe(pa.y_host, pa.pro_y, s.x_bytes);
    }
    return GGML_HIP_OK;
}
static int run_pipelined(const Seam1 &s, const Seam1Slot &p, PipeArgs pa) {
    DeviceCtx *c = p.c;
    c->scope_dirty();                               // the three-stream pipeline is issued live
    pa.upload = !p.x_res && !s.pro();
    if (dst_kept(s, p) && !s.epi && !c->wanted(s.dst->data)) {
        pa.owe_dst = true;                          // (kept for the library's own needs, dropped at scope end)
        c->owe(pa.d_host, pa.dd, s.d_full);
    }
    return run_pipeline(c, pa);
}
// row split inside a graph scope: every slot's resident copy of dst gets the other slots' columns, so the next
// node finds its operand whole in its own HBM (peer DMA over xGMI, or an in-process RCCL all-gather: multi.cpp)
static int exchange_slice(const Seam1 &s, Call &call, const std::vector<Seam1Slot> &slots, int64_t sl) {
    std::vector<float *> bufs;
    std::vector<int64_t> r0, r1;
    for (const Seam1Slot &p : slots) { bufs.push_back((float *)(p.d_res + (size_t)sl * s.d_full)); r0.push_back(p.r0); r1.push_back(p.r1); }
    return exchange_columns(s.G, call.ctxs.data(), bufs.data(), s.ne11, s.ne01, r0.data(), r1.data());
}

static int seam1(const struct ggml_compute_params *params, const struct ggml_tensor *src0, const struct ggml_tensor *src1,
                 struct ggml_tensor *dst, const SeamEpi *epi) {
    if (!params || !src0 || !src1 || !dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    int rc = seam1_check(src0, src1, dst);
    if (rc) return rc;
    if (src0->ne[1] == 0 || src1->ne[1] == 0 || src0->ne[2] * src0->ne[3] == 0) return GGML_HIP_OK;

    Call call;
    rc = call.begin();
    if (rc) return rc;
    if (epi && !epi_fusable(call.G(), src0, src1, dst, *epi)) return SEAM_NOT_FUSABLE;
    Seam1 s(call, src0, src1, dst, epi);

    // dst is about to be written: stale weight-cache entries / resident copies of anything overlapping it go first
    note_host_write(call, dst, true);

    OwnedWeights owned;
    std::vector<Seam1Slot> slots((size_t)s.G);
    for (int g = 0; g < s.G; ++g) {
        rc = seam1_slot(s, call.ctxs[(size_t)g], g, &owned, &slots[(size_t)g]);
        if (rc) return rc;
    }
    if (s.mode() == 1) rc = stage_epilogue(call, *epi, &s.st);
    if (!rc && s.pro()) {
        rc = stage_prologue(call, "norm + mul + mul_mat", epi->pro_x, epi->pro_g, epi->pro_norm, src1, &s.st);
        slots[0].x_res = nullptr;                   // src1 is produced by this call, not looked up
    }
    if (rc) return rc;

    for (int64_t i03 = 0; i03 < s.ne03 && !rc; ++i03)
        for (int64_t i02 = 0; i02 < s.ne02 && !rc; ++i02) {
            for (const Seam1Slot &p : slots) {
                if (p.Ms <= 0) continue;
                rc = p.c->make_current();
                if (rc) break;
                const PipeArgs pa = slice_args(s, p, i02, i03);
                // src1 comes from host memory: inside a graph scope an earlier node's device -> host copy into that
                // very memory may still be in flight
                if (!p.x_res && s.in_graph && !s.pro()) rc = p.c->before_host_read(pa.x_host, (size_t)(s.ne11 - 1) * src1->nb[1] + (size_t)s.ne00 * 4);
                if (!rc) rc = runs_resident(s, p) ? run_resident(s, p, pa) : run_pipelined(s, p, pa);
                if (rc) break;
            }
            if (!rc && s.G > 1 && slots[0].d_res) rc = exchange_slice(s, call, slots, i03 * s.ne02 + i02);
        }
    // outside a graph scope the call returns with dst on the host; inside, ggml_hip_graph_end waits once.  The call's own weights
    // (`owned`, freed on return) go only after the kernels that read them: the slots are synchronised first.
    if (!s.in_graph || rc || !owned.w.empty())
        for (DeviceCtx *c : call.ctxs) {
            int r = c->make_current();
            if (!r) r = c->sync_all();
            if (r && !rc) rc = r;
        }
    return rc;
}

int ggml_hip_compute_forward_mul_mat(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                     const struct ggml_tensor *src1, struct ggml_tensor *dst) {
    return seam1(params, src0, src1, dst, nullptr);
}

/* mul_mat node + the ADD node that consumes it (epilogue side): mm_dst = mul_mat(src0, src1),
 * add_dst = mm_dst + addend, the add applied in the store phase of the mat-mul kernels where they have the form
 * (ggml_hip_mul_mat_epilogue_fused), by the add kernel behind them otherwise; both nodes' data reach host memory. */
int ggml_hip_compute_forward_mul_mat_add(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                         const struct ggml_tensor *src1, struct ggml_tensor *mm_dst,
                                         const struct ggml_tensor *addend, struct ggml_tensor *add_dst) {
    if (!params || !src0 || !src1 || !mm_dst || !addend || !add_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    const SeamEpi epi = {1, addend, add_dst, 1.0f};
    int rc = seam1(params, src0, src1, mm_dst, &epi);
    if (rc != SEAM_NOT_FUSABLE) return rc;
    rc = seam1(params, src0, src1, mm_dst, nullptr);
    if (rc) return rc;
    return ggml_hip_compute_forward_add(params, mm_dst, addend, add_dst);
}

/* mul_mat node + the SCALE node on it (in place: the scale node is a view of the product, Ggml.cs:8265): the data both
 * nodes share ends as product * scalar. */
int ggml_hip_compute_forward_mul_mat_scale(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                           const struct ggml_tensor *src1, struct ggml_tensor *mm_dst,
                                           const struct ggml_tensor *scalar, struct ggml_tensor *scale_dst) {
    if (!params || !src0 || !src1 || !mm_dst || !scalar || !scale_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    if (scalar->type != GGML_TYPE_F32 || nelem(scalar) != 1 || !scalar->data) return fail(GGML_HIP_ERR_SHAPE, "scale: src1 must be an F32 scalar (Ggml.cs:6755)");
    bool fusable = scale_dst->data == mm_dst->data && scalar->op == GGML_OP_NONE;   // a view of the product; the scalar a leaf in host memory
    for (int i = 0; i < 4; ++i) fusable = fusable && scale_dst->ne[i] == mm_dst->ne[i];
    int rc = SEAM_NOT_FUSABLE;
    if (fusable) {
        const SeamEpi epi = {2, nullptr, nullptr, *(const float *)scalar->data};
        rc = seam1(params, src0, src1, mm_dst, &epi);
    }
    if (rc != SEAM_NOT_FUSABLE) return rc;
    rc = seam1(params, src0, src1, mm_dst, nullptr);
    if (rc) return rc;
    return ggml_hip_compute_forward_scale(params, mm_dst, scalar, scale_dst);
}

/* rms_norm node, the MUL node that consumes it, the MUL_MAT node whose src1 that is [, the ADD node on the product]: the
 * whole pre-projection chain of a transformer block as ONE launch for decode-sized batches (N <= 4: the fused mat-vec computes
 * y = (x * rms_scale) * g in its prologue, quantizes it in-kernel and applies the add in its store phase); larger batches, several
 * slots or strided tensors run the pair seam and the mul_mat(+add) seam one after the other.  Every node's data is produced. */
int ggml_hip_compute_forward_norm_mul_mat(const struct ggml_compute_params *params, const struct ggml_tensor *x, const struct ggml_tensor *g,
                                          struct ggml_tensor *norm_dst, struct ggml_tensor *mul_dst, const struct ggml_tensor *src0,
                                          struct ggml_tensor *mm_dst, const struct ggml_tensor *addend, struct ggml_tensor *add_dst) {
    if (!params || !x || !g || !norm_dst || !mul_dst || !src0 || !mm_dst || ((addend == nullptr) != (add_dst == nullptr))) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    SeamEpi epi = {addend ? 1 : 0, addend, add_dst, 1.0f};
    epi.pro_x = x; epi.pro_g = g; epi.pro_norm = norm_dst;
    int rc = seam1(params, src0, mul_dst, mm_dst, &epi);
    if (rc != SEAM_NOT_FUSABLE) return rc;
    rc = ggml_hip_compute_forward_rms_norm_mul(params, x, g, norm_dst, mul_dst);
    if (rc) return rc;
    if (addend) return ggml_hip_compute_forward_mul_mat_add(params, src0, mul_dst, mm_dst, addend, add_dst);
    return seam1(params, src0, mul_dst, mm_dst, nullptr);
}

/* Several MUL_MAT nodes with the SAME src1 (q / k / v, gate / up; optionally the rms_norm -> mul pair that produces that src1
 * in front) as one call: one launch inside a graph scope on one slot for N <= 4 when every weight is a cached leaf of one
 * quantized type and K and every tensor is contiguous; anything else runs the nodes through their own seams, one after the
 * other (which also fills the weight cache, so the next compute of the graph takes the fused form).  pro_x == NULL: no pair. */
int ggml_hip_compute_forward_mul_mat_multi(const struct ggml_compute_params *params, int n, const struct ggml_tensor *const *src0,
                                           const struct ggml_tensor *src1, struct ggml_tensor *const *dst, const struct ggml_tensor *pro_x,
                                           const struct ggml_tensor *pro_g, struct ggml_tensor *pro_norm) {
    if (!params || !src0 || !src1 || !dst || n < 1 || n > 4) return fail(GGML_HIP_ERR_ARG, "bad argument (1..4 nodes)");
    for (int i = 0; i < n; ++i)
        if (!src0[i] || !dst[i]) return fail(GGML_HIP_ERR_ARG, "null argument");
    if ((pro_x == nullptr) != (pro_g == nullptr) || (pro_x == nullptr) != (pro_norm == nullptr)) return fail(GGML_HIP_ERR_ARG, "prologue: x, g and the norm node go together");
    if (seam_idle(params)) return GGML_HIP_OK;
    auto one_by_one = [&]() {
        int rc = pro_x ? ggml_hip_compute_forward_norm_mul_mat(params, pro_x, pro_g, pro_norm, const_cast<ggml_tensor *>(src1), src0[0], dst[0], nullptr, nullptr)
                       : seam1(params, src0[0], src1, dst[0], nullptr);
        for (int i = 1; i < n && !rc; ++i) rc = seam1(params, src0[i], src1, dst[i], nullptr);
        return rc;
    };
    if (n < 2) return one_by_one();
    const int type = src0[0]->type;
    const int64_t K = src1->ne[0], N = src1->ne[1];
    bool ok = type >= 0 && type < GGML_TYPE_COUNT && is_q(type) && weight_type_ok(type) && src1->type == GGML_TYPE_F32 && N >= 1 && N <= 64 &&
              src1->ne[2] == 1 && src1->ne[3] == 1 && src1->data && contiguous_f32(src1) && K % QK == 0;
    for (int i = 0; i < n && ok; ++i) {
        const ggml_tensor *w = src0[i], *d = dst[i];
        ok = w->type == type && w->op == GGML_OP_NONE && w->data && w->ne[0] == K && w->ne[2] == 1 && w->ne[3] == 1 && w->ne[1] > 0 &&
             w->nb[0] == TSIZE[type] && w->nb[0] <= w->nb[1] && d->type == GGML_TYPE_F32 && d->data && contiguous_f32(d) && d->ne[0] == w->ne[1] &&
             d->ne[1] == N && d->ne[2] == 1 && d->ne[3] == 1;
        for (int j = 0; j < i && ok; ++j) ok = dst[j]->data != d->data;
    }
    if (ok && pro_x) {
        const ggml_tensor *ts[3] = {pro_x, pro_g, pro_norm};
        for (const ggml_tensor *t : ts)
            ok = ok && t->data && t->type == GGML_TYPE_F32 && contiguous_f32(t) && t->ne[0] == K && t->ne[1] == N && t->ne[2] == 1 && t->ne[3] == 1;
        ok = ok && pro_norm->data != src1->data;
    }
    if (!ok) return one_by_one();
    Call call;
    int rc = call.begin();
    if (rc) return rc;
    if (call.G() != 1 || !call.in_graph()) return one_by_one();
    DeviceCtx *c = call.ctxs[0];
    rc = c->make_current();
    if (rc) return rc;
    const ggml_hip_weight *W[4];
    for (int i = 0; i < n; ++i) {
        const ggml_tensor *w = src0[i];
        const CacheKey key{w->data, type, w->ne[0], w->ne[1], w->ne[2], w->ne[3], w->nb[1], w->nb[2], w->nb[3], (int64_t)0, w->ne[1]};
        auto it = c->cache.find(key);
        if (it == c->cache.end() || it->second.slices.size() != 1) return one_by_one();      // (uploads and caches them: fused next time)
        W[i] = it->second.slices[0];
    }
    // up to 4 rows: the fused mat-vec takes them (and the prologue) in one launch; 5..64 rows (Q4_0 / Q4_1): one INIT for all of them and one launch
    // where gemm_qmx.hip has the form (ggml_hip_mul_mat_multi_work_dev), the norm -> mul pair in front as its own kernel
    const bool fused_rows = ggml_hip_mul_mat_multi_fused(W, n, N) != 0;
    if (!fused_rows && (N <= 4 || !ggml_hip_mul_mat_epilogue_fused(W[0], N))) return one_by_one();
    for (int i = 0; i < n; ++i) note_host_write(call, dst[i], true);
    Staged st;
    const float *xd = nullptr;
    if (pro_x) {
        rc = stage_prologue(call, "multi mul_mat", pro_x, pro_g, pro_norm, src1, &st);
        if (rc) return rc;
        xd = st.pro_x;
    } else if (operand_f32(c, true, src1, c->src1, &xd)) {
        return fail(GGML_HIP_ERR_RUNTIME, "multi mul_mat: operand staging failed");
    }
    const float *gd = st.pro_g;
    float *nd = st.pro_n, *yd = st.pro_y;
    float *dd[4];
    int64_t ldd[4];
    for (int i = 0; i < n; ++i) {
        dd[i] = result_f32(c, true, dst[i], c->dst);
        if (!dd[i]) return fail(GGML_HIP_ERR_RUNTIME, "multi mul_mat: hipMalloc failed for a resident dst");
        ldd[i] = dst[i]->ne[0];
    }
    if (fused_rows) {
        rc = ggml_hip_mul_mat_multi_dev(W, n, xd, K, N, dd, ldd, gd, K, nd, yd, c->stream);
    } else {
        const size_t w_bytes = ggml_hip_mul_mat_work_size(type, K, N);
        if (c->work.ensure(w_bytes ? w_bytes : 16)) return fail(GGML_HIP_ERR_RUNTIME, "multi mul_mat: hipMalloc failed for scratch");
        if (pro_x) rc = ggml_hip_rms_norm_mul_rows_dev(xd, gd, nd, yd, N, K, c->stream);
        if (!rc) rc = ggml_hip_mul_mat_multi_work_dev(W, n, pro_x ? yd : xd, K, N, dd, ldd, c->work.p, c->work.cap, c->stream);
    }
    if (rc) return rc;
    for (int i = 0; i < n; ++i) c->owe(dst[i]->data, dd[i], (size_t)N * dst[i]->ne[0] * 4);
    if (pro_x) {
        c->owe(pro_norm->data, nd, (size_t)N * K * 4);
        c->owe(src1->data, yd, (size_t)N * K * 4);
    }
    return GGML_HIP_OK;
}

/* ggml_compute_forward_cpy, quantizing branch of dup_f32 / dup_f16 (Ggml.cs:4339-4363, 3935-3966) */
int ggml_hip_compute_forward_cpy(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                 struct ggml_tensor *dst) {
    if (!params || !src0 || !dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    const int st = src0->type, dt = dst->type;
    if (st != GGML_TYPE_F32 && st != GGML_TYPE_F16) return fail(GGML_HIP_ERR_TYPE, "cpy: src0 must be F32 or F16 (Ggml.cs:4602-4619)");
    if (!wq_ok(dt))
        return fail(GGML_HIP_ERR_TYPE, "cpy: only the quantizing branch is on this path (dst type %d)", dt);
    const int64_t ne00 = src0->ne[0], ne01 = src0->ne[1], ne02 = src0->ne[2], ne03 = src0->ne[3];
    const int64_t n_src = ne00 * ne01 * ne02 * ne03, n_dst = dst->ne[0] * dst->ne[1] * dst->ne[2] * dst->ne[3];
    if (n_src != n_dst) return fail(GGML_HIP_ERR_SHAPE, "cpy: element counts differ (Ggml.cs:8281)");
    const size_t es = st == GGML_TYPE_F32 ? 4 : 2;
    if (src0->nb[0] != es) return fail(GGML_HIP_ERR_SHAPE, "cpy: src0 rows must be contiguous");
    if (dst->nb[0] != TSIZE[dt] || dst->nb[1] != dst->nb[0] * (uint64_t)(dst->ne[0] / BLCK[dt]) || dst->nb[2] != dst->nb[1] * (uint64_t)dst->ne[1] ||
        dst->nb[3] != dst->nb[2] * (uint64_t)dst->ne[2])
        return fail(GGML_HIP_ERR_SHAPE, "cpy: dst must be contiguous (Ggml.cs:4290)");
    if (ne00 % QK != 0) return fail(GGML_HIP_ERR_SHAPE, "cpy: ne00 %% 32 != 0");
    if (src0->nb[1] % 16 != 0 && ne01 * ne02 * ne03 > 1) return fail(GGML_HIP_ERR_SHAPE, "cpy: src0 row stride must be a multiple of 16 bytes");
    if (!src0->data || !dst->data) return fail(GGML_HIP_ERR_ARG, "null data");
    if (n_src == 0) return GGML_HIP_OK;
    Call call;
    int rc = call.begin();
    if (rc) return rc;
    DeviceCtx *c = call.ctxs[0];                      // the result goes to host memory only: one slot does it
    rc = c->make_current();
    if (rc) return rc;
    if (call.in_graph()) { rc = c->pay_and_sync(); if (rc) return rc; }   // operands may be dst of an earlier node owed to / on its way to the host
    note_host_write(call, dst, false);                // dst is usually a future src0: its cached device copy (if any) is now stale
    const size_t row_in = (size_t)ne00 * es, rs = row_bytes_of(dt, ne00);   // rs as in Ggml.cs:4345
    if (c->src1.ensure(row_in * ne01) || c->dst.ensure(rs * ne01)) return fail(GGML_HIP_ERR_RUNTIME, "hipMalloc failed for scratch");
    size_t id = 0;
    for (int64_t i03 = 0; i03 < ne03; ++i03)
        for (int64_t i02 = 0; i02 < ne02; ++i02) {
            const uint8_t *src = (const uint8_t *)src0->data + i02 * src0->nb[2] + i03 * src0->nb[3];
            HIP_TRY(hipMemcpy2DAsync(c->src1.p, row_in, src, src0->nb[1], row_in, (size_t)ne01, hipMemcpyHostToDevice, c->stream));
            rc = ggml_hip_quantize_rows_src_dev(dt, st, c->src1.p, ne00, ne01, ne00, c->dst.p, c->stream);
            if (rc) return rc;
            HIP_TRY(hipMemcpyAsync((uint8_t *)dst->data + id, c->dst.p, rs * ne01, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
            id += rs * ne01;
        }
    return GGML_HIP_OK;
}

/* ggml_compute_forward_add_f32 / _mul_f32 (Ggml.cs:4622-4682, 5007-5035): same-shape contiguous f32 operands */
static int binary_f32_seam(int op, const struct ggml_tensor *src0, const struct ggml_tensor *src1, struct ggml_tensor *dst) {
    const char *name = op == 0 ? "add_f32" : "mul_f32";
    if (src0->type != GGML_TYPE_F32 || src1->type != GGML_TYPE_F32 || dst->type != GGML_TYPE_F32) return fail(GGML_HIP_ERR_TYPE, "%s: F32 operands only (Ggml.cs:5043-5056)", name);
    for (int i = 0; i < 4; ++i)
        if (src0->ne[i] != src1->ne[i] || src0->ne[i] != dst->ne[i]) return fail(GGML_HIP_ERR_SHAPE, "%s: shapes differ (Ggml.cs:4628, 5014)", name);
    if (!contiguous_f32(src0) || !contiguous_f32(src1) || !contiguous_f32(dst)) return fail(GGML_HIP_ERR_SHAPE, "%s: contiguous operands only", name);
    if (!src0->data || !src1->data || !dst->data) return fail(GGML_HIP_ERR_ARG, "null data");
    if (nelem(src0) == 0) return GGML_HIP_OK;
    return eltwise_seam(name, {src0, src1}, {dst}, [&](DeviceCtx *c, bool, bool, const float *const *in, float *const *out) -> int {
        HIP_TRY(launch_binary_f32(op, in[0], in[1], out[0], nelem(src0), c->stream));
        return GGML_HIP_OK;
    });
}

/* ggml_compute_forward_add_q_f32 (Ggml.cs:4797-4906) */
int ggml_hip_compute_forward_add(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                 const struct ggml_tensor *src1, struct ggml_tensor *dst) {
    if (!params || !src0 || !src1 || !dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    const int t = src0->type;
    if (t == GGML_TYPE_F32) return binary_f32_seam(0, src0, src1, dst);      // ggml_compute_forward_add_f32 (Ggml.cs:4622-4682)
    if (!wq_ok(t))
        return fail(GGML_HIP_ERR_TYPE, "add: src0 must be F32 or quantized (add_q_f32), got type %d", t);
    if (dst->type != t || src1->type != GGML_TYPE_F32) return fail(GGML_HIP_ERR_TYPE, "add_q_f32: dst must have src0's type, src1 F32 (Ggml.cs:4863-4865)");
    for (int i = 0; i < 4; ++i)
        if (src0->ne[i] != src1->ne[i] || src0->ne[i] != dst->ne[i]) return fail(GGML_HIP_ERR_SHAPE, "add_q_f32: shapes differ (Ggml.cs:4803)");
    if (src0->nb[0] != TSIZE[t] || dst->nb[0] != TSIZE[t] || src1->nb[0] != 4) return fail(GGML_HIP_ERR_SHAPE, "add_q_f32: permuted operand (Ggml.cs:4853-4854)");
    const int64_t ne00 = src0->ne[0], ne01 = src0->ne[1], ne02 = src0->ne[2], ne03 = src0->ne[3];
    if (ne00 % QK != 0) return fail(GGML_HIP_ERR_SHAPE, "ne00 %% 32 != 0 (Ggml.cs:4893)");
    if (src1->nb[1] % 16 != 0 && ne01 > 1) return fail(GGML_HIP_ERR_SHAPE, "add_q_f32: src1 row stride must be a multiple of 16 bytes");
    if (!src0->data || !src1->data || !dst->data) return fail(GGML_HIP_ERR_ARG, "null data");
    if (ne00 * ne01 * ne02 * ne03 == 0) return GGML_HIP_OK;
    Call call;
    int rc = call.begin();
    if (rc) return rc;
    DeviceCtx *c = call.ctxs[0];
    rc = c->make_current();
    if (rc) return rc;
    if (call.in_graph()) { rc = c->pay_and_sync(); if (rc) return rc; }   // operands may be dst of an earlier node owed to / on its way to the host
    note_host_write(call, dst, false);
    const size_t rs = row_bytes_of(t, ne00), rx = (size_t)ne00 * 4;
    if (c->stage.ensure(rs * ne01) || c->src1.ensure(rx * ne01) || c->dst.ensure(rs * ne01)) return fail(GGML_HIP_ERR_RUNTIME, "hipMalloc failed for scratch");
    for (int64_t i03 = 0; i03 < ne03; ++i03)
        for (int64_t i02 = 0; i02 < ne02; ++i02) {
            const uint8_t *a = (const uint8_t *)src0->data + i02 * src0->nb[2] + i03 * src0->nb[3];
            const uint8_t *b = (const uint8_t *)src1->data + i02 * src1->nb[2] + i03 * src1->nb[3];
            // the reference offsets dst rows by i3*nb0 (Ggml.cs:4891), an upstream typo for nb3; intent is followed
            uint8_t *d = (uint8_t *)dst->data + i02 * dst->nb[2] + i03 * dst->nb[3];
            HIP_TRY(hipMemcpy2DAsync(c->stage.p, rs, a, src0->nb[1], rs, (size_t)ne01, hipMemcpyHostToDevice, c->stream));
            HIP_TRY(hipMemcpy2DAsync(c->src1.p, rx, b, src1->nb[1], rx, (size_t)ne01, hipMemcpyHostToDevice, c->stream));
            rc = ggml_hip_add_q_f32_rows_dev(t, c->stage.p, (const float *)c->src1.p, ne01, ne00, c->dst.p, c->stream);
            if (rc) return rc;
            HIP_TRY(hipMemcpy2DAsync(d, dst->nb[1], c->dst.p, rs, rs, (size_t)ne01, hipMemcpyDeviceToHost, c->stream));
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    return GGML_HIP_OK;
}

/* ggml_compute_forward_mul (Ggml.cs:5037-5056) */
int ggml_hip_compute_forward_mul(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                 const struct ggml_tensor *src1, struct ggml_tensor *dst) {
    if (!params || !src0 || !src1 || !dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    return binary_f32_seam(1, src0, src1, dst);
}

/* ggml_compute_forward_scale_f32 (Ggml.cs:6746-6778): dst (a view of src0) *= *(float *)src1->data */
int ggml_hip_compute_forward_scale(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                   const struct ggml_tensor *src1, struct ggml_tensor *dst) {
    if (!params || !src0 || !src1 || !dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    if (src0->type != GGML_TYPE_F32 || src1->type != GGML_TYPE_F32 || dst->type != GGML_TYPE_F32) return fail(GGML_HIP_ERR_TYPE, "scale: F32 only (Ggml.cs:6786-6799)");
    if (nelem(src1) != 1) return fail(GGML_HIP_ERR_SHAPE, "scale: src1 must be a scalar (Ggml.cs:6755)");
    for (int i = 0; i < 4; ++i)
        if (src0->ne[i] != dst->ne[i]) return fail(GGML_HIP_ERR_SHAPE, "scale: shapes differ (Ggml.cs:6754)");
    if (!contiguous_f32(src0) || !contiguous_f32(dst)) return fail(GGML_HIP_ERR_SHAPE, "scale: contiguous operands only (Ggml.cs:6752-6753)");
    if (!src0->data || !src1->data || !dst->data) return fail(GGML_HIP_ERR_ARG, "null data");
    if (nelem(src0) == 0) return GGML_HIP_OK;
    float v = 0.0f;
    // the reference scales dst's own memory: when dst is not a view of src0 that memory is whatever it held before, and
    // so it is here (the input is dst: the device form of "dst" is then an upload of dst->data, not of src0->data)
    return eltwise_seam("scale", {dst}, {dst}, [&](DeviceCtx *c, bool in_graph, bool first, const float *const *in, float *const *out) -> int {
        if (first) {
            if (in_graph) { const int rc = c->before_host_read(src1->data, 4); if (rc) return rc; }      // the scalar is read from host memory (and is part of a named scope's key)
            v = *(const float *)src1->data;
        }
        if (out[0] != in[0]) HIP_TRY(hipMemcpyAsync(out[0], in[0], (size_t)nelem(dst) * 4, hipMemcpyDeviceToDevice, c->stream));
        HIP_TRY(launch_scale_f32(out[0], nelem(dst), v, c->stream));
        return GGML_HIP_OK;
    });
}

// unary f32 seams share one body: which = 0 rms_norm (Ggml.cs:5858-5920), 1 silu (Ggml.cs:5705-5748)
static int unary_f32_seam(int which, const struct ggml_tensor *src0, struct ggml_tensor *dst) {
    const char *name = which == 0 ? "rms_norm" : "silu";
    if (src0->type != GGML_TYPE_F32 || dst->type != GGML_TYPE_F32) return fail(GGML_HIP_ERR_TYPE, "%s: F32 only (Ggml.cs:5927-5940, 5755-5768)", name);
    for (int i = 0; i < 4; ++i)
        if (src0->ne[i] != dst->ne[i]) return fail(GGML_HIP_ERR_SHAPE, "%s: shapes differ (Ggml.cs:5863, 5712)", name);
    if (!contiguous_f32(src0) || !contiguous_f32(dst)) return fail(GGML_HIP_ERR_SHAPE, "%s: contiguous operands only (Ggml.cs:5710-5711)", name);
    if (!src0->data || !dst->data) return fail(GGML_HIP_ERR_ARG, "null data");
    if (nelem(src0) == 0) return GGML_HIP_OK;
    return eltwise_seam(name, {src0}, {dst}, [&](DeviceCtx *c, bool, bool, const float *const *in, float *const *out) -> int {
        if (which == 0) HIP_TRY(launch_rms_norm_f32(in[0], out[0], nelem(src0) / src0->ne[0], src0->ne[0], c->stream));
        else HIP_TRY(launch_silu_f32(in[0], out[0], nelem(src0), c->stream));
        return GGML_HIP_OK;
    });
}

// two element-wise nodes, one launch (fused.hip): which = 0 rms_norm -> mul, 1 silu -> mul.  `first` is the operand of the
// first node, `other` the second operand of the mul node; both nodes' results are written and reach host memory.
static int fused_pair_seam(int which, const struct ggml_tensor *first, const struct ggml_tensor *other, struct ggml_tensor *mid_dst,
                           struct ggml_tensor *mul_dst) {
    const char *name = which == 0 ? "rms_norm + mul" : "silu + mul";
    const ggml_tensor *all[4] = {first, other, mid_dst, mul_dst};
    for (const ggml_tensor *t : all) {
        if (t->type != GGML_TYPE_F32) return fail(GGML_HIP_ERR_TYPE, "%s: F32 only", name);
        if (!contiguous_f32(t)) return fail(GGML_HIP_ERR_SHAPE, "%s: contiguous operands only", name);
        if (!t->data) return fail(GGML_HIP_ERR_ARG, "null data");
        for (int i = 0; i < 4; ++i)
            if (t->ne[i] != first->ne[i]) return fail(GGML_HIP_ERR_SHAPE, "%s: shapes differ", name);
    }
    if (mid_dst->data == mul_dst->data) return fail(GGML_HIP_ERR_SHAPE, "%s: the two nodes share their data", name);
    if (nelem(first) == 0) return GGML_HIP_OK;
    return eltwise_seam(name, {first, other}, {mid_dst, mul_dst}, [&](DeviceCtx *c, bool in_graph, bool to_host, const float *const *in, float *const *out) -> int {
        if (which == 0) HIP_TRY(launch_rms_norm_mul_f32(in[0], in[1], out[0], out[1], nelem(first) / first->ne[0], first->ne[0], c->stream));
        else HIP_TRY(launch_silu_mul_f32(in[0], in[1], out[0], out[1], nelem(first), c->stream));
        // the mid node's result (both copies on the compute stream; outside a graph scope the mul node's finish waits for both)
        const size_t bytes = (size_t)nelem(first) * 4;
        if (to_host && in_graph) {
            c->owe(mid_dst->data, out[0], bytes);
        } else if (to_host) {
            HIP_TRY(hipMemcpyAsync(mid_dst->data, out[0], bytes, hipMemcpyDeviceToHost, c->stream));
            c->d2h_bytes += bytes;
        }
        return GGML_HIP_OK;
    });
}

/* rms_norm node + the MUL node that consumes it (prologue side of a mul_mat): norm_dst = rms_norm(x),
 * mul_dst = norm_dst * g, one launch, the unfused kernels' bits */
int ggml_hip_compute_forward_rms_norm_mul(const struct ggml_compute_params *params, const struct ggml_tensor *x,
                                          const struct ggml_tensor *g, struct ggml_tensor *norm_dst, struct ggml_tensor *mul_dst) {
    if (!params || !x || !g || !norm_dst || !mul_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    return fused_pair_seam(0, x, g, norm_dst, mul_dst);
}

/* silu node + the MUL node that consumes it (the SwiGLU gate): silu_dst = silu(a), mul_dst = silu_dst * b */
int ggml_hip_compute_forward_silu_mul(const struct ggml_compute_params *params, const struct ggml_tensor *a,
                                      const struct ggml_tensor *b, struct ggml_tensor *silu_dst, struct ggml_tensor *mul_dst) {
    if (!params || !a || !b || !silu_dst || !mul_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    return fused_pair_seam(1, a, b, silu_dst, mul_dst);
}

/* ggml_compute_forward_rms_norm_f32 (Ggml.cs:5858-5920) */
int ggml_hip_compute_forward_rms_norm(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                      struct ggml_tensor *dst) {
    if (!params || !src0 || !dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    return unary_f32_seam(0, src0, dst);
}

/* ggml_compute_forward_silu_f32 (Ggml.cs:5705-5748) */
int ggml_hip_compute_forward_silu(const struct ggml_compute_params *params, const struct ggml_tensor *src0,
                                  struct ggml_tensor *dst) {
    if (!params || !src0 || !dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (seam_idle(params)) return GGML_HIP_OK;
    return unary_f32_seam(1, src0, dst);
}

}  // extern "C"
