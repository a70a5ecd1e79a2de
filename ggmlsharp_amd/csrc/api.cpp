// api.cpp -- the C-ABI of include/ggml_hip.h, part 1: lifecycle and device slots, resident weights, the hot path on
// device-resident data, the row functions (Seam 2).  seams.cpp holds the host-pointer seams, scope.cpp the graph scope,
// wcache.cpp the Seam-1 weight cache, multi.cpp the row split over several devices.  No CPU fallback anywhere: without a
// device every compute entry returns GGML_HIP_ERR_NO_DEVICE.
#include "ctx.h"
#include "plan.h"
#include <algorithm>
#include <vector>

namespace ghip {

thread_local std::string t_err;
thread_local int t_slot = -1;                     // ggml_hip_bind_thread
std::mutex g_table_mu;
DeviceCtx *g_slots[MAX_SLOTS] = {};
std::atomic<int> g_nslots{0};

// An error reported while the calling thread has a NAMED graph scope open: the host falls back to its own code for
// that node, so the scope must never be captured -- a replay would skip the seams, the fallback with them, and
// the node's data would never be produced.  The key is refused for good; a capture in progress is ended and issued live.
static void poison_open_scope() {
    const int b = bound_slot();
    DeviceCtx *c = slot(b >= 0 ? b : 0);
    if (!c) return;
    std::unique_lock<std::recursive_mutex> lk(c->mu, std::try_to_lock);
    if (!lk.owns_lock()) return;
    if ((c->scope_mode != 1 && c->scope_mode != 2) || c->scope_owner != std::this_thread::get_id()) return;
    const uint64_t key = c->scope_key;
    if (c->scope_mode == 2) c->scope_dirty();
    else c->scope_clean = false;
    DeviceCtx::Captured &e = c->captured[key];
    e.seen = 0;
    if (!e.refused) { e.refused = true; ++c->n_refused; }
}

int fail(int code, const char *fmt, ...) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    t_err = buf;
    if (code != GGML_HIP_OK) poison_open_scope();
    return code;
}

const int BLCK[GGML_TYPE_COUNT] = {1, 1, 32, 32, 16, 16, 32, 32, 32, 32, 1, 1, 1};          // Ggml.cs:55-70
const size_t TSIZE[GGML_TYPE_COUNT] = {4, 2, 20, 24, 10, 12, 22, 24, 36, 44, 1, 2, 4};      // Ggml.cs:72-87

// Q4_2 and Q5_1 follow SURVEY D7's intent (their half scales are IEEE bit patterns, as in the upstream scalar code the C#
// transcribes); Q4_3 / Q8_1 have null slots (D8).
bool wq_ok(int t) {
    return t == GGML_TYPE_Q4_0 || t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q4_2 || t == GGML_TYPE_Q5_0 || t == GGML_TYPE_Q5_1 ||
           t == GGML_TYPE_Q8_0;
}
bool weight_type_ok(int t) { return wq_ok(t) || t == GGML_TYPE_F32 || t == GGML_TYPE_F16; }
bool is_q(int t) { return t >= GGML_TYPE_Q4_0 && t <= GGML_TYPE_Q8_1; }
int vec_dot_type(int t) {  // Ggml.cs:219-290
    switch (t) {
    case GGML_TYPE_Q4_0: case GGML_TYPE_Q4_2: case GGML_TYPE_Q5_0: case GGML_TYPE_Q8_0: return GGML_TYPE_Q8_0;
    case GGML_TYPE_Q4_1: case GGML_TYPE_Q5_1: return GGML_TYPE_Q8_1;
    default: return -1;
    }
}
bool contiguous_f32(const ggml_tensor *t) {
    return t->type == GGML_TYPE_F32 && t->nb[0] == 4 && t->nb[1] == (uint64_t)t->ne[0] * 4 && t->nb[2] == t->nb[1] * (uint64_t)t->ne[1] &&
           t->nb[3] == t->nb[2] * (uint64_t)t->ne[2];
}

namespace {
bool has_min_plane(int t) { return t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q4_2; }   // Q4_2: its second scale
bool has_qh_plane(int t) { return t == GGML_TYPE_Q5_0 || t == GGML_TYPE_Q5_1; }
bool has_i8_planes(int t) { return t == GGML_TYPE_Q5_0 || t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q4_1 || t == GGML_TYPE_Q4_2; }   // int8 operand planes (gemm_qmp.hip)
bool has_min_pieces(int t) { return t == GGML_TYPE_Q5_1 || t == GGML_TYPE_Q4_1; }                 // the min plane as three bf16 pieces (K3p-int8's min-term product)
// a line of the reference's source belongs in a message about one of ITS types only
const char *ref_cite(const wtype *r, const char *cite) { return r->id < GGML_TYPE_COUNT ? cite : ""; }
// the row of the type a weight was uploaded as
const wtype *weight_row(const ggml_hip_weight *w) { return wtype_of(ggml_hip_weight_type(w)); }
}  // namespace

// Kernel selection lives in plan.cpp (plan.h): ONE decision per product -- family, form, summation tree -- that every launcher consumes.
// The K1 image for (type, K, N): NOT a function of the number of weight rows (a row shard runs the kernel form of the unsplit matrix).
int act_image_kind(int type, int64_t K, int64_t N) { return plan_image_kind(type, K, N); }
mm_plan weight_plan(const ggml_hip_weight *w, int64_t N, bool one_call) { return plan_mul_mat(w->type, w->ext_type, w->M, w->K, N, one_call); }
// ... for ONE weight, as the two-phase entries see it (INIT writes it, COMPUTE reads it): the stated exception included -- planes beyond
// 32-bit buffer offsets are served by the int8 family and its image
int weight_image_kind(const ggml_hip_weight *w, int64_t N) { return plan_act_image(weight_plan(w, N, false)); }

// ---------------- DeviceCtx ----------------
int DeviceCtx::make_current() const {
    hipError_t e = hipSetDevice(device);   // calls arrive on arbitrary host threads (SURVEY 8(b) "Threading")
    if (e != hipSuccess) return fail(GGML_HIP_ERR_RUNTIME, "hipSetDevice(%d): %s", device, hipGetErrorString(e));
    return GGML_HIP_OK;
}
int DeviceCtx::sync_all() {
    scope_dirty();
    d2h_busy = false;
    hipError_t e = hipStreamSynchronize(stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s_h2d);
    if (e == hipSuccess) e = hipStreamSynchronize(s_d2h);
    return e == hipSuccess ? GGML_HIP_OK : fail(GGML_HIP_ERR_RUNTIME, "stream synchronize: %s", hipGetErrorString(e));
}

int n_slots() { return g_nslots.load(std::memory_order_acquire); }
DeviceCtx *slot(int i) { return (i >= 0 && i < n_slots()) ? g_slots[i] : nullptr; }
int bound_slot() { return (t_slot >= 0 && t_slot < n_slots()) ? t_slot : -1; }

int Call::begin() {
    int rc = ensure_init();
    if (rc) return rc;
    const int b = bound_slot();
    if (b >= 0) ctxs.push_back(slot(b));
    else for (int i = 0; i < n_slots(); ++i) ctxs.push_back(slot(i));
    for (DeviceCtx *c : ctxs) {
        if (!c) return fail(GGML_HIP_ERR_RUNTIME, "library was shut down during the call");
        locks.emplace_back(c->mu);                 // slot order: no lock-order inversion between callers
        if (c->dead) return fail(GGML_HIP_ERR_RUNTIME, "library was shut down during the call");   // (ggml_hip_shutdown won the race for this slot's lock)
        // another thread is capturing a named scope on this slot's stream: this call's launches are none of that graph's
        // business -- the capture is ended and issued live (its owner carries on live), then this call runs
        if (c->scope_mode == 2 && c->scope_owner != std::this_thread::get_id()) c->scope_dirty();
    }
    return GGML_HIP_OK;
}

namespace {

int create_slot_locked(int i, int device) {
    DeviceCtx *c = new DeviceCtx();
    c->slot = i;
    c->device = device;
    hipError_t e = hipSetDevice(device);
    hipDeviceProp_t prop;
    if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
    if (e == hipSuccess) c->arch = prop.gcnArchName;
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->s_h2d, hipStreamNonBlocking);
    if (e == hipSuccess) e = hipStreamCreateWithFlags(&c->s_d2h, hipStreamNonBlocking);
    for (int k = 0; k < PIPE_EVENTS && e == hipSuccess; ++k) {
        e = hipEventCreateWithFlags(&c->ev_in[k], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_k[k], hipEventDisableTiming);
    }
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_compute, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_d2h, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_xchg, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_ready, hipEventDisableTiming);
    if (e != hipSuccess) {
        delete c;
        return fail(GGML_HIP_ERR_RUNTIME, "device %d: %s", device, hipGetErrorString(e));
    }
    g_slots[i] = c;
    return GGML_HIP_OK;
}

std::vector<DeviceCtx *> g_graveyard;              // contexts of shut-down slots: resources released, the object kept for late lockers

void release_slot_resources_locked(DeviceCtx *c) {
    (void)hipSetDevice(c->device);
    (void)c->sync_all();
    c->free_cache();
    c->src1.release(); c->dst.release(); c->dst2.release(); c->work.release(); c->stage.release();
    for (Scratch &a : c->aux) a.release();
    c->drain(true);
    for (int k = 0; k < PIPE_EVENTS; ++k) {
        if (c->ev_in[k]) (void)hipEventDestroy(c->ev_in[k]);
        if (c->ev_k[k]) (void)hipEventDestroy(c->ev_k[k]);
    }
    for (hipEvent_t ev : {c->ev_compute, c->ev_d2h, c->ev_xchg, c->ev_ready})
        if (ev) (void)hipEventDestroy(ev);
    for (hipStream_t s : {c->stream, c->s_h2d, c->s_d2h})
        if (s) (void)hipStreamDestroy(s);
    c->stream = c->s_h2d = c->s_d2h = nullptr;
}
void destroy_slot_locked(DeviceCtx *c) {            // (a slot that never became visible: failed initialisation)
    release_slot_resources_locked(c);
    delete c;
}

int init_slots(int n, const int *ids) {
    const int ndev = ggml_hip_device_count();
    if (ndev <= 0) return fail(GGML_HIP_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU path");
    if (n <= 0 || n > MAX_SLOTS) return fail(GGML_HIP_ERR_ARG, "n_devices %d out of range [1,%d]", n, MAX_SLOTS);
    for (int i = 0; i < n; ++i) {
        const int d = ids ? ids[i] : i;
        if (d < 0 || d >= ndev) return fail(GGML_HIP_ERR_ARG, "device %d out of range [0,%d)", d, ndev);
    }
    std::lock_guard<std::mutex> lk(g_table_mu);
    if (g_nslots.load() > 0) {
        bool same = g_nslots.load() == n;
        for (int i = 0; same && i < n; ++i) same = g_slots[i]->device == (ids ? ids[i] : i);
        if (same) return GGML_HIP_OK;
        // streams, scratch, caches and kernel attributes belong to the devices they were created on: no silent re-targeting
        return fail(GGML_HIP_ERR_ARG, "already initialised on a different device set; call ggml_hip_shutdown first");
    }
    for (int i = 0; i < n; ++i) {
        int rc = create_slot_locked(i, ids ? ids[i] : i);
        if (rc) {
            for (int k = 0; k < i; ++k) { destroy_slot_locked(g_slots[k]); g_slots[k] = nullptr; }
            return rc;
        }
    }
    // peer access between distinct devices (xGMI on an MI355X node): kernels and DMA engines of one slot may then address
    // another slot's buffers directly.  Failure is not fatal -- peer copies then stage through the host.
    for (int i = 0; i < n; ++i)
        for (int k = 0; k < n; ++k) {
            if (g_slots[i]->device == g_slots[k]->device) continue;
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, g_slots[i]->device, g_slots[k]->device) == hipSuccess && can) {
                (void)hipSetDevice(g_slots[i]->device);
                hipError_t e = hipDeviceEnablePeerAccess(g_slots[k]->device, 0);
                if (e != hipSuccess) (void)hipGetLastError();     // already enabled, or refused: clear the sticky error
            }
        }
    (void)hipSetDevice(g_slots[0]->device);
    g_nslots.store(n, std::memory_order_release);
    return GGML_HIP_OK;
}

}  // namespace

int ensure_init() {
    if (n_slots() > 0) return GGML_HIP_OK;
    return ggml_hip_init(0);
}

// the slot a device-level or row-function call runs on: the calling thread's bound slot, else slot 0
static DeviceCtx *call_slot() {
    const int b = bound_slot();
    return slot(b >= 0 ? b : 0);
}

// a weight of row r's resident form, its planes carved from one allocation (a plane the form does not have stays null)
static int alloc_weight(DeviceCtx *c, const wtype *r, int64_t K, int64_t M, ggml_hip_weight **out) {
    ggml_hip_weight *w = new ggml_hip_weight();
    memset(w, 0, sizeof *w);
    const int type = r->resident;
    if (r->origin == WT_ORIGIN_EXT) w->ext_type = r->id;    // (a k-quant weight: Q5_K / Q4_K in the planar Q5_1 form, the two-scale types in the planar Q4_2 form)
    if (r->origin == WT_ORIGIN_UP) w->up_type = r->id;      // (IQ4_NL: type == Q8_0, the planes of a plain Q8_0 weight)
    static std::atomic<uint64_t> next_uid{1};
    w->type = type; w->M = M; w->K = K; w->Mpad = pad_rows(M > 0 ? M : 1); w->device = c->device; w->uid = next_uid.fetch_add(1);
    const bool dense = type == GGML_TYPE_F32 || is_dense16(type);
    constexpr size_t NONE = ~(size_t)0;
    size_t total = 0;
    auto take = [&](bool have, size_t bytes) { if (!have) return NONE; const size_t off = total; total += bytes; return off; };
    size_t off_p = NONE, off_qs = NONE, off_d = NONE, off_m = NONE, off_qh = NONE, off_gs = NONE, off_i8 = NONE, off_mp = NONE, off_kh = NONE, off_6a = NONE, off_6b = NONE;
    if (dense) {
        total = ((size_t)w->Mpad * K * (type == GGML_TYPE_F32 ? 4 : 2) + 255) / 256 * 256;
        // F16 / BF16: the k-panel copy for the MFMA kernels; F32: the rows as three bf16 pieces per element (dense16.hip K10d)
        off_p = take(true, (size_t)(is_dense16(type) ? dense16_kpad(K) / 8 + DENSE16_SPARE_PANELS : dense16_kpad(K) / 8 * 3 + DENSE32_SPARE_PANELS) * w->Mpad * 16);
    } else {
        w->nbk = K / QK;
        const size_t nba = (size_t)(pad_kblocks(w->nbk) + K_LOOKAHEAD);   // allocated k-blocks (zero past the real end)
        const size_t plane = nba * w->Mpad * 4;
        // (the two-scale form lives on the int8 planes alone -- no kernel it is planned onto reads the nibble plane: a stub)
        off_qs = take(true, r->own_i8 ? 256 : nba * w->Mpad * (type == GGML_TYPE_Q8_0 ? 32 : 16));
        off_d = take(true, plane);
        off_m = take(has_min_plane(type), plane);
        off_qh = take(has_qh_plane(type), plane);
        off_gs = take(true, (size_t)w->nbk * w->Mpad * 4 * gemv_side_planes(type));       // the mat-vec's tile-major copy of d / m / qh
        off_i8 = take(has_i8_planes(type), nba * w->Mpad * 32);                           // zero past the end of K
        off_mp = take(has_min_pieces(type), (size_t)((w->nbk + 15) / 16 * 2 * 3) * w->Mpad * 16);   // whole pairs of k-groups, zero past the end of K
        off_kh = take(r->hdr_slot != 0, (size_t)(w->nbk / 8 + 1) * w->Mpad * r->hdr_slot);  // super-block headers, for the byte-exact download
        // bf6 operand planes of the MX mat-mat kernel: 0.75 B / weight and digit (Q5_0, Q8_0: two digits)
        const bool q4 = type == GGML_TYPE_Q4_0 || type == GGML_TYPE_Q4_1;
        const bool with6 = q4 || (plan_force_gemm() == 3 && (type == GGML_TYPE_Q5_0 || type == GGML_TYPE_Q8_0));
        off_6a = take(with6, nba * (q4 ? 1 : 2) * w->Mpad * 16);
        off_6b = take(with6, nba * (q4 ? 1 : 2) * w->Mpad * 8);
    }
    if (total == 0) total = 16;
    void *base = nullptr;
    hipError_t e = hipMalloc(&base, total);
    if (e != hipSuccess) { delete w; return fail(GGML_HIP_ERR_RUNTIME, "hipMalloc(%zu): %s", total, hipGetErrorString(e)); }
    w->bytes = total;
    auto at = [&](size_t off) { return off == NONE ? nullptr : (uint8_t *)base + off; };
    if (dense) {
        w->dense = base;
        (is_dense16(type) ? w->p16 : w->p32) = at(off_p);
    }
    w->qs = at(off_qs); w->d = (float *)at(off_d); w->m = (float *)at(off_m); w->qh = (uint32_t *)at(off_qh); w->gs = (uint32_t *)at(off_gs);
    w->i8p = at(off_i8); w->mp3 = at(off_mp); w->khdr = at(off_kh); w->q6a = at(off_6a); w->q6b = at(off_6b);
    *out = w;
    return GGML_HIP_OK;
}

static void *weight_base(const ggml_hip_weight *w) { return w->dense ? w->dense : (void *)w->qs; }

// One sequence for every type, driven by its row: the file-format rows (staged to the device when they are the host's) go through the row's
// converter into the resident planes, then the operand images built from those planes -- each pass a no-op on a weight without the plane it fills.
int make_weight(DeviceCtx *c, int type, const void *rows, bool rows_on_host, int64_t ne00, int64_t ne01, uint64_t nb01,
                int64_t row_begin, int64_t row_end, hipStream_t st, ggml_hip_weight **out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    *out = nullptr;
    const wtype *r = wtype_of(type);
    if (!r || !r->to_planar)
        return fail(GGML_HIP_ERR_TYPE, "type %d is not a supported weight type (Q4_3/Q8_1 have null slots, Ggml.cs:248,278-282)", type);
    if (!rows || ne00 <= 0 || ne01 < 0 || row_begin < 0 || row_end < row_begin || row_end > ne01)
        return fail(GGML_HIP_ERR_ARG, "bad weight arguments");
    if (ne00 % k_unit(r) != 0) return fail(GGML_HIP_ERR_SHAPE, "ne00 %% %d != 0%s", (int)k_unit(r), ref_cite(r, " (Ggml.cs:6694)"));
    const uint64_t row_bytes = (uint64_t)r->bytes * (uint64_t)(ne00 / r->blck);
    if (nb01 < row_bytes) return fail(GGML_HIP_ERR_SHAPE, "nb01 smaller than a row (transposed src0, Ggml.cs:8229)");
    const bool dense = r->resident == GGML_TYPE_F32 || is_dense16(r->resident);
    if (!rows_on_host && dense && (nb01 % 2 != 0 || ((uintptr_t)rows & 1)))
        return fail(GGML_HIP_ERR_SHAPE, "dense device rows must be 2-byte aligned");
    int rc = c ? GGML_HIP_OK : ensure_init();
    if (rc) return rc;
    if (!c) c = call_slot();
    rc = c->make_current();
    if (rc) return rc;
    const int64_t rows_n = row_end - row_begin;
    ggml_hip_weight *w = nullptr;
    rc = alloc_weight(c, r, ne00, rows_n, &w);
    if (rc) return rc;
    hipError_t e = hipMemsetAsync(weight_base(w), 0, w->bytes, st);
    void *staging = nullptr;
    if (e == hipSuccess && rows_on_host && rows_n > 0) {
        e = hipMalloc(&staging, (size_t)rows_n * row_bytes);
        if (e == hipSuccess)
            e = hipMemcpy2DAsync(staging, row_bytes, (const uint8_t *)rows + (uint64_t)row_begin * nb01, nb01, row_bytes,
                                 (size_t)rows_n, hipMemcpyHostToDevice, st);
        if (e == hipSuccess) e = r->to_planar(type, (const uint8_t *)staging, row_bytes, 0, rows_n, w, st);
    } else if (e == hipSuccess) {
        e = r->to_planar(type, (const uint8_t *)rows, nb01, row_begin, rows_n, w, st);
    }
    if (e == hipSuccess) e = launch_nibbles_to_bf6(w, st);
    if (e == hipSuccess && !r->own_i8) e = launch_q5_to_i8(w, st);      // (the two-scale converters write the int8 planes themselves)
    if (e == hipSuccess) e = launch_min_pieces(w, st);
    if (e == hipSuccess) e = launch_gemv_side_image(w, st);
    if (e == hipSuccess) e = launch_f16_rows_to_panels(w, st);
    if (e == hipSuccess) e = launch_f32_rows_to_split_panels(w, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (staging) (void)hipFree(staging);
    if (e != hipSuccess) {
        (void)hipFree(weight_base(w));
        delete w;
        return fail(GGML_HIP_ERR_RUNTIME, "weight upload: %s", hipGetErrorString(e));
    }
    *out = w;
    return GGML_HIP_OK;
}

// device-level entries take the caller's stream; the device the weight lives on must be current for the launch
static int weight_device_current(const ggml_hip_weight *w) {
    int cur = -1;
    if (hipGetDevice(&cur) == hipSuccess && cur == w->device) return GGML_HIP_OK;
    hipError_t e = hipSetDevice(w->device);
    return e == hipSuccess ? GGML_HIP_OK : fail(GGML_HIP_ERR_RUNTIME, "hipSetDevice(%d): %s", w->device, hipGetErrorString(e));
}

}  // namespace ghip

using namespace ghip;

extern "C" {

int ggml_hip_blck_size(int type) { const wtype *r = wtype_of(type); return r ? r->blck : 0; }
size_t ggml_hip_type_size(int type) { const wtype *r = wtype_of(type); return r ? r->bytes : 0; }

int ggml_hip_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) { (void)hipGetLastError(); return 0; }
    return n;
}

int ggml_hip_init(int device) {
    const int n = ggml_hip_device_count();
    if (n <= 0) return fail(GGML_HIP_ERR_NO_DEVICE, "no HIP device visible; this library has no CPU path");
    if (device < 0 || device >= n) return fail(GGML_HIP_ERR_ARG, "device %d out of range [0,%d)", device, n);
    if (n_slots() > 0) {
        // a process that already drives a device set keeps it; selecting one of ITS devices for the calling thread is fine
        for (int i = 0; i < n_slots(); ++i)
            if (slot(i)->device == device) { HIP_TRY(hipSetDevice(device)); return GGML_HIP_OK; }
        return fail(GGML_HIP_ERR_ARG, "already initialised on another device (%d); call ggml_hip_shutdown first", slot(0)->device);
    }
    return init_slots(1, &device);
}

int ggml_hip_init_devices(int n_devices, const int *device_ids) { return init_slots(n_devices, device_ids); }
int ggml_hip_n_slots(void) { return n_slots(); }
int ggml_hip_slot_device(int s) { DeviceCtx *c = slot(s); return c ? c->device : -1; }

int ggml_hip_bind_thread(int s) {
    if (s < -1 || s >= n_slots()) return fail(GGML_HIP_ERR_ARG, "slot %d out of range [-1,%d)", s, n_slots());
    t_slot = s;
    if (s >= 0) return slot(s)->make_current();
    return GGML_HIP_OK;
}

void ggml_hip_shutdown(void) {
    std::lock_guard<std::mutex> lk(g_table_mu);
    const int n = g_nslots.load();
    if (n == 0) return;
    g_nslots.store(0, std::memory_order_release);
    for (int i = 0; i < n; ++i) {
        DeviceCtx *c = g_slots[i];
        {
            // a seam that is still inside finishes first; one that fetched the pointer before n_slots dropped to 0 but has not
            // locked yet finds `dead` set when it does (Call::begin, scope_replaying) and returns "not initialised"
            std::lock_guard<std::recursive_mutex> l2(c->mu);
            c->dead = true;
            g_slots[i] = nullptr;
            release_slot_resources_locked(c);
        }
        g_graveyard.push_back(c);          // the object (its mutex) outlives late lockers; freed at the next shutdown / process end
    }
    for (size_t k = 0; k + 64 < g_graveyard.size(); ++k) { delete g_graveyard[k]; g_graveyard[k] = nullptr; }
    g_graveyard.erase(std::remove(g_graveyard.begin(), g_graveyard.end(), nullptr), g_graveyard.end());
    rccl_shutdown();
}

const char *ggml_hip_last_error(void) { return t_err.c_str(); }
const char *ggml_hip_arch(void) { DeviceCtx *c = slot(0); return c ? c->arch.c_str() : ""; }

int ggml_hip_weight_upload(int type, const void *host_rows, int64_t ne00, int64_t ne01, uint64_t nb01,
                           int64_t row_begin, int64_t row_end, void *stream, ggml_hip_weight **out) {
    return make_weight(nullptr, type, host_rows, true, ne00, ne01, nb01, row_begin, row_end, (hipStream_t)stream, out);
}

int ggml_hip_weight_from_device(int type, const void *dev_rows, int64_t ne00, int64_t ne01, uint64_t nb01,
                                int64_t row_begin, int64_t row_end, void *stream, ggml_hip_weight **out) {
    return make_weight(nullptr, type, dev_rows, false, ne00, ne01, nb01, row_begin, row_end, (hipStream_t)stream, out);
}

int ggml_hip_weight_download(const ggml_hip_weight *w, void *host_rows, void *stream) {
    if (!w || !host_rows) return fail(GGML_HIP_ERR_ARG, "null argument");
    int rc = ensure_init();
    if (rc) return rc;
    rc = weight_device_current(w);
    if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const wtype *r = weight_row(w);                         // (the uploaded type: IQ4_NL's rows are not its resident Q8_0's)
    const size_t total = r->bytes * (size_t)(w->K / r->blck) * (size_t)w->M;
    if (total == 0) return GGML_HIP_OK;
    void *staging = nullptr;
    HIP_TRY(hipMalloc(&staging, total));
    hipError_t e = r->from_planar(w, (uint8_t *)staging, st);
    if (e == hipSuccess) e = hipMemcpyAsync(host_rows, staging, total, hipMemcpyDeviceToHost, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    (void)hipFree(staging);
    if (e != hipSuccess) return fail(GGML_HIP_ERR_RUNTIME, "weight download: %s", hipGetErrorString(e));
    return GGML_HIP_OK;
}

void ggml_hip_weight_free(ggml_hip_weight *w) {
    if (!w) return;
    int cur = -1;
    (void)hipGetDevice(&cur);
    if (cur != w->device) (void)hipSetDevice(w->device);
    (void)hipFree(weight_base(w));
    if (cur >= 0 && cur != w->device) (void)hipSetDevice(cur);
    delete w;
}
int64_t ggml_hip_weight_rows(const ggml_hip_weight *w) { return w ? w->M : 0; }
int64_t ggml_hip_weight_cols(const ggml_hip_weight *w) { return w ? w->K : 0; }
int ggml_hip_weight_type(const ggml_hip_weight *w) { return w ? (w->up_type ? w->up_type : w->ext_type ? w->ext_type : w->type) : -1; }

size_t ggml_hip_mul_mat_work_size(int type, int64_t K, int64_t N) {
    if (K <= 0 || N <= 0) return 0;
    if (const wtype *r = wtype_of(type)) type = r->resident;    // same operand images
    if (is_dense16(type)) return (size_t)dense16_kpad(K) * (size_t)pad_act(N) * 2;   // src1 as Half (Ggml.cs:3356-3357), padded (BF16: as bf16)
    if (type == GGML_TYPE_F32) return N > 256 ? (size_t)dense16_kpad(K) * (size_t)pad_act(N) * 6 : 0;   // src1 as three bf16 pieces (dense16.hip K10d; the reference needs none)
    if (!is_q(type)) return 0;
    return act_bytes(K, pad_act(N));
}

// the INIT kernels read src1 rows in 16-byte pieces (float4 loads, LDS-DMA): base and row stride must allow that
static int check_src1_alignment(const float *d_src1, int64_t ld1) {
    if (((uintptr_t)d_src1 & 15) != 0 || ld1 % 4 != 0)
        return fail(GGML_HIP_ERR_SHAPE, "src1 must be 16-byte aligned with a row stride that is a multiple of 4 elements");
    return GGML_HIP_OK;
}

// ONE plan per call: an entry plans once and hands the plan to the INIT and COMPUTE steps below, so the two agree because they hold the
// same plan.  A one-call plan that is not the fused mat-vec IS the COMPUTE-only plan, field for field (tools/plan_dump.cpp --check).
// The INIT step of a quantized weight: K1 writes the image of `pl` (d_src1 is not null, N > 0)
static int mul_mat_init_step(const ggml_hip_weight *w, const mm_plan &pl, const float *d_src1, int64_t N, int64_t ld1, void *d_work,
                             size_t work_bytes, void *stream) {
    if (ld1 < w->K) return fail(GGML_HIP_ERR_SHAPE, "ld1 < K");
    int rc = check_src1_alignment(d_src1, ld1);
    if (rc) return rc;
    if (!d_work || work_bytes < ggml_hip_mul_mat_work_size(w->type, w->K, N))
        return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu", ggml_hip_mul_mat_work_size(w->type, w->K, N));
    rc = weight_device_current(w);
    if (rc) return rc;
    act_planes p = act_carve(d_work, w->K, pad_act(N));
    HIP_TRY(launch_quantize_act(d_src1, N, w->K, ld1, p, plan_act_image(pl), (hipStream_t)stream, weight_row(w)->q8k));
    return GGML_HIP_OK;
}

int ggml_hip_mul_mat_init_dev(const ggml_hip_weight *w, const float *d_src1, int64_t N, int64_t ld1, void *d_work,
                              size_t work_bytes, void *stream) {
    if (!w || !d_src1) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (N <= 0) return GGML_HIP_OK;
    if (!is_q(w->type)) return GGML_HIP_OK;  // dense: INIT is a no-op for f32 (Ggml.cs:6117-6120); f16 rounds in-kernel
    return mul_mat_init_step(w, weight_plan(w, N, false), d_src1, N, ld1, d_work, work_bytes, stream);
}

int ggml_hip_act_image_kind(int type, int64_t K, int64_t N) {
    const wtype *r = wtype_of(type);
    const int t = r ? r->resident : type;
    return act_image_kind(is_dense16(t) ? GGML_TYPE_F16 : t, K, N);   // (BF16: F16's answer)
}
void ggml_hip_debug_force_gemm(int which) { plan_set_force_gemm(which); }

// the plan of mul_mat(type, M, K, N) as ggml_hip_mul_mat_dev will run it; no device is needed (tests/test_plan_cpu.py)
int ggml_hip_mm_plan(int type, int64_t M, int64_t K, int64_t N, ggml_hip_mm_plan_t *out) {
    if (!out) return fail(GGML_HIP_ERR_ARG, "out is null");
    const wtype *r = wtype_of(type);
    if (!r || !r->to_planar) return fail(GGML_HIP_ERR_TYPE, "type %d is not a supported weight type", type);
    if (M <= 0 || K <= 0 || N <= 0 || K % k_unit(r) != 0) return fail(GGML_HIP_ERR_SHAPE, "bad shape");
    const mm_plan p = plan_mul_mat(r->resident, wtype_ext(r), M, K, N, true);
    out->family = p.family; out->image_kind = p.image | ((p.flags & MM_FLAG_MIN_PIECES) ? ACT_IMAGE_MIN_PIECES : 0); out->form = p.form; out->tree_id = plan_tree_id(p);
    out->ksplit = p.ksplit; out->kstyle = p.kstyle; out->kunit = p.kunit; out->arith = p.arith;
    out->tile_m = p.tile_m; out->tile_n = p.tile_n; out->waves = p.waves; out->tiles_per_wave = p.tiles_per_wave;
    out->workgroups = p.wgs; out->flags = p.flags;
    return GGML_HIP_OK;
}

int ggml_hip_quantize_act_dev(const float *d_src1, int64_t N, int64_t K, int64_t ld1, void *d_work, size_t work_bytes,
                              int image_kind, void *stream) {
    if (N <= 0) return GGML_HIP_OK;
    if (!d_src1 || !d_work) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (K <= 0 || K % QK != 0 || ld1 < K) return fail(GGML_HIP_ERR_SHAPE, "K %% 32 != 0 or ld1 < K");
    int rc = check_src1_alignment(d_src1, ld1);
    if (rc) return rc;
    const bool pieces = image_kind >= 0 && (image_kind & ACT_IMAGE_MIN_PIECES) != 0;   // + 64 (kind 0 only): the min-term piece planes as well
    if (pieces) image_kind &= ~ACT_IMAGE_MIN_PIECES;
    const bool q8k = image_kind >= 16;                         // + 16: the Q8_K rule of the k-quants (K % 256 == 0; kinds 0..2)
    if (q8k) image_kind -= 16;
    if (image_kind < 0 || image_kind > 3 || (q8k && (image_kind == 3 || K % 256 != 0)) || (pieces && (image_kind != 0 || K / QK < 8)))
        return fail(GGML_HIP_ERR_ARG, "image kind %d", image_kind);
    if (work_bytes < act_bytes(K, pad_act(N))) return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu", act_bytes(K, pad_act(N)));
    // the MFMA images are written (and read) through 32-bit buffer offsets: 64 image bytes per row and k-block
    if (image_kind != 0 && (uint64_t)pad_kblocks(K / QK) * 64 * (uint64_t)pad_act(N) > 0xFFFFFFFFull)
        return fail(GGML_HIP_ERR_SHAPE, "image kind %d needs K/32 * 64 * Npad < 4 GiB (ggml_hip_act_image_kind never selects it beyond that)", image_kind);
    HIP_TRY(launch_quantize_act(d_src1, N, K, ld1, act_carve(d_work, K, pad_act(N)), image_kind | (pieces ? ACT_IMAGE_MIN_PIECES : 0), (hipStream_t)stream, q8k));
    return GGML_HIP_OK;
}

// the COMPUTE launch of an INIT-based plan: the family's launcher, with the store-phase epilogue (nullptr: none) where the plan fuses one
static hipError_t launch_planned(const ggml_hip_weight *w, const mm_plan &pl, act_planes p, int64_t N, float *dst, int64_t ldd, hipStream_t st,
                                 const mm_epilogue *ep) {
    switch (pl.family) {
    case MMF_K3S_I8:    return launch_gemm_q8_small(w, pl, p, N, dst, ldd, st, ep);
    case MMF_K3P_I8:    return launch_gemm_q8_mid(w, pl, p, N, dst, ldd, st, ep);
    case MMF_K3S_MX: case MMF_K3P_MX: case MMF_MX:
                        return launch_gemm_qmx(w, pl, p, N, dst, ldd, st, ep);   // (its ld_add / ld2 bound covers every MX form, K3p-MX included)
    }
    if (ep) return hipErrorNotSupported;                    // (the other families have no fused epilogue: plan flags)
    switch (pl.family) {
    case MMF_GEMV_ROWS: return launch_gemv_q(w, p, N, dst, ldd, st);
    case MMF_F16:       return launch_gemm_q16(w, pl, p, N, dst, ldd, st);
    case MMF_I8:        return launch_gemm_q(w, pl, p, N, dst, ldd, st);
    default:            return hipErrorInvalidValue;
    }
}

// The COMPUTE step of a quantized weight on the image the INIT step wrote for the same plan (d_dst is not null, N > 0, M > 0)
static int mul_mat_compute_step(const ggml_hip_weight *w, const mm_plan &pl, int64_t N, float *d_dst, int64_t ldd, const void *d_work,
                                size_t work_bytes, void *stream) {
    if (ldd < w->M) return fail(GGML_HIP_ERR_SHAPE, "ldd < M");
    if (!d_work || work_bytes < ggml_hip_mul_mat_work_size(w->type, w->K, N)) return fail(GGML_HIP_ERR_ARG, "work buffer too small");
    int rc = weight_device_current(w);
    if (rc) return rc;
    const act_planes p = act_carve((void *)d_work, w->K, pad_act(N));
    HIP_TRY(launch_planned(w, pl, p, N, d_dst, ldd, (hipStream_t)stream, nullptr));
    if (pl.flags & MM_FLAG_MIN_PASS) HIP_TRY(launch_q2k_min_pass(w, p, N, d_dst, ldd, (hipStream_t)stream));   // (Q2_K: dst -= its min term)
    return GGML_HIP_OK;
}

int ggml_hip_mul_mat_compute_dev(const ggml_hip_weight *w, int64_t N, float *d_dst, int64_t ldd, const void *d_work,
                                 size_t work_bytes, void *stream) {
    if (!w || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (N <= 0 || w->M <= 0) return GGML_HIP_OK;
    if (!is_q(w->type)) return fail(GGML_HIP_ERR_TYPE, "compute_dev is the quantized COMPUTE phase; use ggml_hip_mul_mat_dev for dense");
    return mul_mat_compute_step(w, weight_plan(w, N, false), N, d_dst, ldd, d_work, work_bytes, stream);   // (INIT wrote this plan's image)
}

// the Q2_K min pass alone, on the image ggml_hip_mul_mat_init_dev wrote (TEST HOOK: the two forms side by side, and the pass's own time)
int ggml_hip_debug_q2k_min_pass_dev(const ggml_hip_weight *w, int64_t N, float *d_dst, int64_t ldd, const void *d_work, size_t work_bytes,
                                    int form, void *stream) {
    if (!w || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (!kquant_min_pass(w->ext_type)) return fail(GGML_HIP_ERR_TYPE, "the min pass is for Q2_K weights");
    if (form < 0 || form > 2) return fail(GGML_HIP_ERR_ARG, "form %d (0 auto, 1, 2)", form);
    if (N <= 0 || w->M <= 0) return GGML_HIP_OK;
    if (ldd < w->M) return fail(GGML_HIP_ERR_SHAPE, "ldd < M");
    if (!d_work || work_bytes < ggml_hip_mul_mat_work_size(w->type, w->K, N)) return fail(GGML_HIP_ERR_ARG, "work buffer too small");
    int rc = weight_device_current(w);
    if (rc) return rc;
    HIP_TRY(launch_q2k_min_pass(w, act_carve((void *)d_work, w->K, pad_act(N)), N, d_dst, ldd, (hipStream_t)stream, form));
    return GGML_HIP_OK;
}

// does ggml_hip_mul_mat_dev quantize src1 inside the product launch for this weight and N?  (By weight, plan and N; src1 itself must suit K1's
// lane-per-block kernel as well.)  ggml_hip_mul_mat_init_dev / _compute_dev never do: they are the two steps, and the fused route's reference.
static bool fused_init_route(const ggml_hip_weight *w, const mm_plan &pl, int64_t N) {
    return is_q(w->type) && !weight_row(w)->q8k && plan_act_image(pl) == 3 && !(pl.flags & MM_FLAG_MIN_PASS) && gemm_qmx_fused_serves(w, pl, N);
}

// the product under its one-call plan `pl` (w is not null, N > 0, M > 0)
static int mul_mat_planned(const ggml_hip_weight *w, const mm_plan &pl, const float *d_src1, int64_t N, int64_t ld1, float *d_dst,
                           int64_t ldd, void *d_work, size_t work_bytes, void *stream, bool may_fuse_init = false) {
    if (!d_src1 || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (ld1 < w->K || ldd < w->M) return fail(GGML_HIP_ERR_SHAPE, "ld1 < K or ldd < M");
    int rc = weight_device_current(w);
    if (rc) return rc;
    if (!is_q(w->type)) {
        if (pl.family == MMF_DENSE16 || pl.family == MMF_DENSE32) {
            // The matrix-core forms need INIT scratch (the reference's own wdata for F16, Ggml.cs:6362-6379; three bf16 pieces per element for
            // F32 above 256 rows) and read src1 rows in 16-byte pieces.  r4: a missing buffer or a misaligned src1 is an ERROR -- it
            // used to select dense.hip silently, whose arithmetic differs in the last bits, so the same product could differ between callers.
            if (!d_work || work_bytes < ggml_hip_mul_mat_work_size(w->type, w->K, N))
                return fail(GGML_HIP_ERR_ARG, "work buffer too small: this shape needs %zu bytes (ggml_hip_mul_mat_work_size)", ggml_hip_mul_mat_work_size(w->type, w->K, N));
            if (ld1 % 4 != 0 || ((uintptr_t)d_src1 & 15) != 0) return fail(GGML_HIP_ERR_SHAPE, "src1 rows must be 16-byte aligned (base and row stride) for this shape");
            if (pl.family == MMF_DENSE16) {
                if (is_bf16(w->type)) HIP_TRY(launch_dense16_init_bf16(d_src1, N, w->K, ld1, d_work, (hipStream_t)stream));   // INIT: src1 -> bf16
                else HIP_TRY(launch_dense16_init(d_src1, N, w->K, ld1, d_work, (hipStream_t)stream));  // INIT: src1 -> Half (Ggml.cs:6362-6379)
                HIP_TRY(launch_dense16(w, pl, d_work, N, d_dst, ldd, (hipStream_t)stream));
            } else {
                HIP_TRY(launch_dense32_init(d_src1, N, w->K, ld1, d_work, (hipStream_t)stream));
                HIP_TRY(launch_dense32(w, d_work, N, d_dst, ldd, (hipStream_t)stream));
            }
            return GGML_HIP_OK;
        }
        HIP_TRY(launch_dense(w, pl, d_src1, N, ld1, d_dst, ldd, (hipStream_t)stream));
        return GGML_HIP_OK;
    }
    if (pl.family == MMF_GEMV_FUSED) {                      // small N: INIT and COMPUTE fused in one launch, no scratch needed
        rc = check_src1_alignment(d_src1, ld1);     // (float4 loads of the activation rows)
        if (rc) return rc;
        HIP_TRY(launch_gemv_q_fused(w, d_src1, ld1, N, d_dst, ldd, (hipStream_t)stream));
        return GGML_HIP_OK;
    }
    // the headline form quantizes src1 inside the product launch (gemm_qmx.hip mx_fuse): the arguments INIT and COMPUTE would refuse are refused
    // the same way, and a src1 only the general INIT kernel reads goes through the two steps below
    if (may_fuse_init && fused_init_route(w, pl, N) && quantize_act_bf6_serves(d_src1, N, w->K, ld1)) {
        if (!d_work || work_bytes < ggml_hip_mul_mat_work_size(w->type, w->K, N))
            return fail(GGML_HIP_ERR_ARG, "work buffer too small: need %zu", ggml_hip_mul_mat_work_size(w->type, w->K, N));
        HIP_TRY(launch_gemm_qmx_fused(w, pl, d_src1, ld1, act_carve(d_work, w->K, pad_act(N)), N, d_dst, ldd, (hipStream_t)stream));
        return GGML_HIP_OK;
    }
    rc = mul_mat_init_step(w, pl, d_src1, N, ld1, d_work, work_bytes, stream);
    if (rc) return rc;
    return mul_mat_compute_step(w, pl, N, d_dst, ldd, d_work, work_bytes, stream);
}

int ggml_hip_mul_mat_init_fused(const ggml_hip_weight *w, int64_t N) { return w && N > 0 && w->M > 0 && fused_init_route(w, weight_plan(w, N, true), N) ? 1 : 0; }
void ggml_hip_debug_fused_init_skip_panel(int panel) { gemm_qmx_fused_skip_panel(panel); }

int ggml_hip_mul_mat_dev(const ggml_hip_weight *w, const float *d_src1, int64_t N, int64_t ld1, float *d_dst,
                         int64_t ldd, void *d_work, size_t work_bytes, void *stream) {
    if (!w) return fail(GGML_HIP_ERR_ARG, "null weight");
    if (N <= 0 || w->M <= 0) return GGML_HIP_OK;
    return mul_mat_planned(w, weight_plan(w, N, true), d_src1, N, ld1, d_dst, ldd, d_work, work_bytes, stream, true);   // (this entry alone fuses INIT)
}

// does a kernel form with a fused store-phase epilogue serve this weight under its one-call plan?  The fused mat-vec (N <= 4), the MX
// mat-mat (Q4_0 / Q4_1), K3p and Q8_0's batched-decode form; every other form runs the epilogue as its own launch behind the mat-mul.
// (The plan's flag: selection, this report and the launch agree by construction -- ADVICE r3.)
static bool epilogue_is_fused(const ggml_hip_weight *w, const mm_plan &pl) {
    return is_q(w->type) && w->ext_type == 0 && (pl.flags & MM_FLAG_EPILOGUE_FUSED) != 0;
}

int ggml_hip_mul_mat_epilogue_fused(const ggml_hip_weight *w, int64_t N) { return w && epilogue_is_fused(w, weight_plan(w, N, true)) ? 1 : 0; }

int ggml_hip_mul_mat_epilogue_dev(const ggml_hip_weight *w, const float *d_src1, int64_t N, int64_t ld1, float *d_dst, int64_t ldd,
                                  void *d_work, size_t work_bytes, int mode, const float *d_addend, int64_t ld_add, float *d_dst2,
                                  int64_t ldd2, float scale, void *stream) {
    if (mode == 0) return ggml_hip_mul_mat_dev(w, d_src1, N, ld1, d_dst, ldd, d_work, work_bytes, stream);
    if (!w) return fail(GGML_HIP_ERR_ARG, "null weight");
    if (mode != 1 && mode != 2) return fail(GGML_HIP_ERR_ARG, "epilogue mode %d (1 = add, 2 = scale)", mode);
    if (N <= 0 || w->M <= 0) return GGML_HIP_OK;
    if (mode == 1 && (!d_addend || !d_dst2 || ld_add < w->M || ldd2 < w->M)) return fail(GGML_HIP_ERR_ARG, "add epilogue: addend / dst2 missing or too narrow");
    const mm_epilogue ep = {mode, d_addend, ld_add, d_dst2, ldd2, scale};
    const mm_plan plan = weight_plan(w, N, true);
    if (epilogue_is_fused(w, plan)) {
        if (!d_src1 || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
        if (ld1 < w->K || ldd < w->M) return fail(GGML_HIP_ERR_SHAPE, "ld1 < K or ldd < M");
        int rc = weight_device_current(w);
        if (rc) return rc;
        if (plan.family == MMF_GEMV_FUSED) {
            rc = check_src1_alignment(d_src1, ld1);
            if (rc) return rc;
            HIP_TRY(launch_gemv_q_fused(w, d_src1, ld1, N, d_dst, ldd, (hipStream_t)stream, &ep));
            return GGML_HIP_OK;
        }
        rc = mul_mat_init_step(w, plan, d_src1, N, ld1, d_work, work_bytes, stream);
        if (rc) return rc;
        const hipError_t e = launch_planned(w, plan, act_carve(d_work, w->K, pad_act(N)), N, d_dst, ldd, (hipStream_t)stream, &ep);
        if (e == hipSuccess) return GGML_HIP_OK;
        // not supported = operands of the EPILOGUE beyond the 32-bit offsets of these kernels (ld_add / ld2 past 4 GiB): the product itself
        // succeeds, so it does with an epilogue -- the unfused path below
        if (e != hipErrorNotSupported) HIP_TRY(e);
        (void)hipGetLastError();
    }
    // no fused form for this kernel: the product, then the node's own kernel row by row (same values)
    int rc = mul_mat_planned(w, plan, d_src1, N, ld1, d_dst, ldd, d_work, work_bytes, stream);
    if (rc) return rc;
    if (mode == 2) {
        if (ldd == w->M) HIP_TRY(launch_scale_f32(d_dst, N * w->M, scale, (hipStream_t)stream));
        else for (int64_t n = 0; n < N; ++n) HIP_TRY(launch_scale_f32(d_dst + n * ldd, w->M, scale, (hipStream_t)stream));
        return GGML_HIP_OK;
    }
    if (ldd == w->M && ld_add == w->M && ldd2 == w->M) HIP_TRY(launch_binary_f32(0, d_dst, d_addend, d_dst2, N * w->M, (hipStream_t)stream));
    else for (int64_t n = 0; n < N; ++n) HIP_TRY(launch_binary_f32(0, d_dst + n * ldd, d_addend + n * ld_add, d_dst2 + n * ldd2, w->M, (hipStream_t)stream));
    return GGML_HIP_OK;
}

/* ---- the row split's product + exchange ---- */
// Which kernel forms store to the peers themselves: the staged MX forms and K3p (plan.h).  The others compute into this rank's own buffer
// and hand their columns to the peers with the column-push kernel (layout.hip) behind the product: the same bytes, one more launch.
static bool push_is_fused(const ggml_hip_weight *w, const mm_plan &pl, int n_peers) {
    if (!is_q(w->type) || n_peers - 1 > MM_PUSH_MAX) return false;
    if (pl.flags & MM_FLAG_MIN_PASS) return false;          // (Q2_K: the min pass must run before the columns leave)
    const int f = pl.family;
    // (r5: the batched-decode forms too -- a short shard at prompt sizes runs them)
    return f == MMF_MX || f == MMF_K3P_MX || f == MMF_K3P_I8 || f == MMF_K3S_MX || f == MMF_K3S_I8;
}
int ggml_hip_mul_mat_push_fused(const ggml_hip_weight *w, int64_t N, int n_peers) {
    return w && push_is_fused(w, weight_plan(w, N, true), n_peers) ? 1 : 0;
}

int ggml_hip_mul_mat_push_dev(const ggml_hip_weight *w, const float *d_src1, int64_t N, int64_t ld1, float *const *d_peers, int n_peers, int own,
                              int64_t ld_total, int64_t col0, void *d_work, size_t work_bytes, void *stream) {
    if (!w || !d_peers) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (n_peers < 1 || n_peers > 16 || own < 0 || own >= n_peers || !d_peers[own]) return fail(GGML_HIP_ERR_ARG, "1..16 destination buffers, this rank's own among them");
    if (N <= 0 || w->M <= 0) return GGML_HIP_OK;
    if (col0 < 0 || ld_total < col0 + w->M) return fail(GGML_HIP_ERR_SHAPE, "ld_total < col0 + M");
    float *mine = d_peers[own] + col0;
    const mm_plan plan = weight_plan(w, N, true);
    if (push_is_fused(w, plan, n_peers)) {
        if (!d_src1) return fail(GGML_HIP_ERR_ARG, "null argument");
        if (ld1 < w->K) return fail(GGML_HIP_ERR_SHAPE, "ld1 < K");
        mm_epilogue ep = {3, nullptr, 0, nullptr, 0, 1.0f, 0, {}};
        for (int g = 0; g < n_peers; ++g)
            if (g != own && d_peers[g]) ep.push[ep.npush++] = d_peers[g] + col0;
        int rc = weight_device_current(w);
        if (rc) return rc;
        rc = mul_mat_init_step(w, plan, d_src1, N, ld1, d_work, work_bytes, stream);
        if (rc) return rc;
        const hipError_t e = launch_planned(w, plan, act_carve(d_work, w->K, pad_act(N)), N, mine, ld_total, (hipStream_t)stream, &ep);
        if (e == hipSuccess) return GGML_HIP_OK;
        // not supported = ld_total beyond what the store phase addresses (a tile's rows past the 32-bit buffer offsets of the staged MX forms,
        // a row stride past K3p's int): the product itself still runs, as ggml_hip_mul_mat_epilogue_dev's unfused path does -- the plain
        // product (the one-call entry routes such a dst to a kernel that can address it) and the column-push kernel behind it
        if (e != hipErrorNotSupported) HIP_TRY(e);
        (void)hipGetLastError();
    }
    int rc = mul_mat_planned(w, plan, d_src1, N, ld1, mine, ld_total, d_work, work_bytes, stream);
    if (rc) return rc;
    std::vector<float *> others((size_t)n_peers);
    for (int g = 0; g < n_peers; ++g) others[(size_t)g] = g == own ? nullptr : d_peers[g];
    HIP_TRY(launch_push_columns(mine, ld_total, N, w->M, others.data(), n_peers, ld_total, col0, (hipStream_t)stream));
    return GGML_HIP_OK;
}

// rms_norm -> mul -> mul_mat [-> add | scale] on device-resident rows.  One launch where the fused mat-vec serves N (the
// prologue computes and quantizes y = (x * rms_scale) * g in-kernel and writes both nodes' results), else the pair kernel of
// fused.hip followed by the mat-mul with its epilogue.  d_x, d_g: [N] rows, ld_x / ld_g elements apart; d_norm, d_y: [N][K].
static bool prologue_is_fused(const ggml_hip_weight *w, int64_t N, const float *d_x, int64_t ld_x, const float *d_g, int64_t ld_g,
                              const float *d_norm, const float *d_y) {
    return is_q(w->type) && w->ext_type == 0 && gemv_fused_has_epilogue(N) && ld_x % 4 == 0 && ld_g % 4 == 0 &&
           (((uintptr_t)d_x | (uintptr_t)d_g | (uintptr_t)d_norm | (uintptr_t)d_y) & 15) == 0;
}

int ggml_hip_norm_mul_mat_fused(const ggml_hip_weight *w, int64_t N) {
    return w && is_q(w->type) && w->ext_type == 0 && gemv_fused_has_epilogue(N) ? 1 : 0;
}

int ggml_hip_norm_mul_mat_dev(const ggml_hip_weight *w, const float *d_x, int64_t ld_x, const float *d_g, int64_t ld_g, int64_t N,
                              float *d_norm, float *d_y, float *d_dst, int64_t ldd, void *d_work, size_t work_bytes, int mode,
                              const float *d_addend, int64_t ld_add, float *d_dst2, int64_t ldd2, float scale, void *stream) {
    if (!w || !d_x || !d_g || !d_norm || !d_y || !d_dst) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (N <= 0 || w->M <= 0) return GGML_HIP_OK;
    if (ld_x < w->K || ld_g < w->K || ldd < w->M) return fail(GGML_HIP_ERR_SHAPE, "row stride smaller than a row");
    if (mode < 0 || mode > 2) return fail(GGML_HIP_ERR_ARG, "epilogue mode %d", mode);
    if (mode == 1 && (!d_addend || !d_dst2 || ld_add < w->M || ldd2 < w->M)) return fail(GGML_HIP_ERR_ARG, "add epilogue: addend / dst2 missing or too narrow");
    int rc = weight_device_current(w);
    if (rc) return rc;
    if (prologue_is_fused(w, N, d_x, ld_x, d_g, ld_g, d_norm, d_y)) {
        const mm_prologue pro = {d_g, ld_g, d_norm, d_y};
        const mm_epilogue ep = {mode, d_addend, ld_add, d_dst2, ldd2, scale};
        HIP_TRY(launch_gemv_q_fused_pro(w, d_x, ld_x, pro, N, d_dst, ldd, (hipStream_t)stream, mode ? &ep : nullptr));
        return GGML_HIP_OK;
    }
    if (ld_x == w->K && ld_g == w->K) HIP_TRY(launch_rms_norm_mul_f32(d_x, d_g, d_norm, d_y, N, w->K, (hipStream_t)stream));
    else for (int64_t n = 0; n < N; ++n) HIP_TRY(launch_rms_norm_mul_f32(d_x + n * ld_x, d_g + n * ld_g, d_norm + n * w->K, d_y + n * w->K, 1, w->K, (hipStream_t)stream));
    return ggml_hip_mul_mat_epilogue_dev(w, d_y, N, w->K, d_dst, ldd, d_work, work_bytes, mode, d_addend, ld_add, d_dst2, ldd2, scale, stream);
}

/* ---- several weight matrices behind ONE activation matrix (q / k / v, gate / up): one launch for N <= 4 ---- */
static bool multi_ok(const ggml_hip_weight *const *w, int n_w, int64_t N) {
    if (!w || n_w < 2 || n_w > 4 || !gemv_fused_has_epilogue(N)) return false;
    for (int i = 0; i < n_w; ++i)
        if (!w[i] || !is_q(w[i]->type) || w[i]->ext_type != 0 || w[i]->type != w[0]->type || w[i]->K != w[0]->K || w[i]->device != w[0]->device || w[i]->M <= 0)
            return false;
    return true;
}
int ggml_hip_mul_mat_multi_fused(const ggml_hip_weight *const *w, int n_w, int64_t N) { return multi_ok(w, n_w, N) ? 1 : 0; }

int ggml_hip_mul_mat_multi_dev(const ggml_hip_weight *const *w, int n_w, const float *d_src1, int64_t ld1, int64_t N, float *const *d_dst,
                               const int64_t *ldd, const float *d_g, int64_t ld_g, float *d_norm, float *d_y, void *stream) {
    if (!w || !d_src1 || !d_dst || !ldd) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (!multi_ok(w, n_w, N)) return fail(GGML_HIP_ERR_SHAPE, "multi mul_mat: 2..4 quantized matrices of one type and K on one device, N <= 4");
    for (int i = 0; i < n_w; ++i)
        if (!d_dst[i] || ldd[i] < w[i]->M) return fail(GGML_HIP_ERR_SHAPE, "multi mul_mat: dst %d missing or its row stride smaller than a row", i);
    if (ld1 < w[0]->K) return fail(GGML_HIP_ERR_SHAPE, "row stride smaller than a row");
    int rc = weight_device_current(w[0]);
    if (rc) return rc;
    rc = check_src1_alignment(d_src1, ld1);
    if (rc) return rc;
    const bool with_pro = d_g != nullptr;
    if (with_pro) {
        if (!d_norm || !d_y || ld_g < w[0]->K) return fail(GGML_HIP_ERR_ARG, "prologue: norm / mul outputs missing or g too narrow");
        if (!prologue_is_fused(w[0], N, d_src1, ld1, d_g, ld_g, d_norm, d_y)) return fail(GGML_HIP_ERR_SHAPE, "prologue: operands must be 16-byte aligned with row strides that are multiples of 4");
    }
    const mm_prologue pro = {d_g, ld_g, d_norm, d_y};
    HIP_TRY(launch_gemv_q_fused_multi(w, n_w, d_src1, ld1, with_pro ? &pro : nullptr, N, d_dst, ldd, (hipStream_t)stream));
    return GGML_HIP_OK;
}

/* the same for any N, with the work buffer a batch needs: src1 is quantized ONCE (the INIT phase, Ggml.cs:6641-6654, is the same for
 * every matrix of one type and K) and the matrices follow -- in one launch where plan.cpp plans the group (plan_mul_mat_group: K3s,
 * 5 <= N <= 64), else one COMPUTE after the other behind the shared image.  Every row is bit for bit what ggml_hip_mul_mat_dev gives for that matrix. */
int ggml_hip_mul_mat_multi_work_dev(const ggml_hip_weight *const *w, int n_w, const float *d_src1, int64_t ld1, int64_t N, float *const *d_dst,
                                    const int64_t *ldd, void *d_work, size_t work_bytes, void *stream) {
    if (!w || !d_src1 || !d_dst || !ldd) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (n_w < 1 || n_w > 4) return fail(GGML_HIP_ERR_ARG, "multi mul_mat: 1..4 matrices");
    if (N <= 0) return GGML_HIP_OK;
    for (int i = 0; i < n_w; ++i) {
        if (!w[i] || !d_dst[i]) return fail(GGML_HIP_ERR_ARG, "multi mul_mat: matrix or dst %d missing", i);
        if (!is_q(w[i]->type) || w[i]->type != w[0]->type || w[i]->ext_type != w[0]->ext_type || w[i]->K != w[0]->K || w[i]->device != w[0]->device)
            return fail(GGML_HIP_ERR_SHAPE, "multi mul_mat: quantized matrices of one type and K on one device");
        if (ldd[i] < w[i]->M) return fail(GGML_HIP_ERR_SHAPE, "multi mul_mat: dst %d row stride smaller than a row", i);
    }
    if (n_w >= 2 && multi_ok(w, n_w, N)) return ggml_hip_mul_mat_multi_dev(w, n_w, d_src1, ld1, N, d_dst, ldd, nullptr, 0, nullptr, nullptr, stream);
    // one image for all of them?  (the image kind of a type follows N and K; M enters for shapes beyond the 32-bit offsets only)
    mm_plan pl[4];
    for (int i = 0; i < n_w; ++i) pl[i] = weight_plan(w[i], N, false);   // (the COMPUTE-only plans: one INIT, then a COMPUTE each)
    bool shared = pl[0].family != MMF_GEMV_ROWS && w[0]->ext_type == 0;
    for (int i = 1; i < n_w && shared; ++i) shared = plan_act_image(pl[i]) == plan_act_image(pl[0]);
    if (!shared) {                                          // (each matrix through the one-call entry, under its own one-call plan)
        for (int i = 0; i < n_w; ++i) {
            const int rc = ggml_hip_mul_mat_dev(w[i], d_src1, N, ld1, d_dst[i], ldd[i], d_work, work_bytes, stream);
            if (rc) return rc;
        }
        return GGML_HIP_OK;
    }
    int rc = mul_mat_init_step(w[0], pl[0], d_src1, N, ld1, d_work, work_bytes, stream);
    if (rc) return rc;
    int64_t M[4], Mpad[4];
    for (int i = 0; i < n_w; ++i) { M[i] = w[i]->M; Mpad[i] = w[i]->Mpad; }
    const mm_plan g = plan_mul_mat_group(w[0]->type, w[0]->ext_type, M, Mpad, n_w, w[0]->K, N);
    if (g.family != MMF_NONE) {
        for (int i = 1; i < n_w; ++i) { rc = weight_device_current(w[i]); if (rc) return rc; }
        const act_planes p = act_carve(d_work, w[0]->K, pad_act(N));
        const hipError_t e = g.family == MMF_K3S_MX ? launch_gemm_qmx_multi(g, w, n_w, p, N, d_dst, ldd, (hipStream_t)stream)
                                                    : launch_gemm_q8_small_multi(g, w, n_w, p, N, d_dst, ldd, (hipStream_t)stream);
        if (e == hipSuccess) return GGML_HIP_OK;
        if (e != hipErrorNotSupported) { (void)hipGetLastError(); return fail(GGML_HIP_ERR_RUNTIME, "multi mul_mat: %s", hipGetErrorString(e)); }
    }
    for (int i = 0; i < n_w; ++i) {
        if (w[i]->M <= 0) continue;
        rc = mul_mat_compute_step(w[i], pl[i], N, d_dst[i], ldd[i], d_work, work_bytes, stream);
        if (rc) return rc;
    }
    return GGML_HIP_OK;
}

int ggml_hip_rms_norm_mul_rows_dev(const float *d_x, const float *d_g, float *d_norm, float *d_y, int64_t nrows, int64_t k, void *stream) {
    if (nrows <= 0 || k <= 0) return GGML_HIP_OK;
    if (!d_x || !d_g || !d_norm || !d_y) return fail(GGML_HIP_ERR_ARG, "null argument");
    HIP_TRY(launch_rms_norm_mul_f32(d_x, d_g, d_norm, d_y, nrows, k, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_quantize_rows_dev(int type, const float *d_x, int64_t nrows, int64_t k, void *d_blocks, void *stream) {
    if (nrows <= 0) return GGML_HIP_OK;  // empty input: nothing to do (buffers may be null)
    if (!d_x || !d_blocks) return fail(GGML_HIP_ERR_ARG, "null argument");
    const wtype *r = wtype_of(type);
    if (!r || !r->quantize) return fail(GGML_HIP_ERR_TYPE, "quantize: unsupported type %d", type);
    if (r->blck == 1 && k <= 0) return fail(GGML_HIP_ERR_SHAPE, "k <= 0");
    if (k % k_unit(r) != 0) return fail(GGML_HIP_ERR_SHAPE, "k %% %d != 0%s", (int)k_unit(r), ref_cite(r, " (Ggml.cs:336)"));
    if (r->x_align && ((uintptr_t)d_x & (uintptr_t)(r->x_align - 1)) != 0) return fail(GGML_HIP_ERR_SHAPE, "the rows must be %d-byte aligned", r->x_align);
    HIP_TRY(r->quantize(type, d_x, nrows, k, d_blocks, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_dequantize_rows_dev(int type, const void *d_blocks, int64_t nrows, int64_t k, float *d_y, void *stream) {
    if (nrows <= 0) return GGML_HIP_OK;
    if (!d_y || !d_blocks) return fail(GGML_HIP_ERR_ARG, "null argument");
    const wtype *r = wtype_of(type);
    if (!r || !r->dequantize) return fail(GGML_HIP_ERR_TYPE, "dequantize: unsupported type %d (Q8_1 slot is null, Ggml.cs:278)", type);
    if (r->blck == 1 && k <= 0) return fail(GGML_HIP_ERR_SHAPE, "k <= 0");
    if (k % k_unit(r) != 0) return fail(GGML_HIP_ERR_SHAPE, "k %% %d != 0%s", (int)k_unit(r), ref_cite(r, " (Ggml.cs:839)"));
    HIP_TRY(r->dequantize(type, d_blocks, nrows, k, d_y, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_quantize_row(int type, const float *x, void *y, int k) {
    if (!x || !y || k <= 0) return fail(GGML_HIP_ERR_ARG, "bad argument");
    int rc = ensure_init();
    if (rc) return rc;
    if (type < 0 || type >= GGML_TYPE_COUNT || !is_q(type)) return fail(GGML_HIP_ERR_TYPE, "not a quantized type");
    DeviceCtx *c = call_slot();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    rc = c->make_current();
    if (rc) return rc;
    const size_t xb = (size_t)k * 4, yb = TSIZE[type] * (size_t)(k / BLCK[type]);
    if (c->src1.ensure(xb) || c->dst.ensure(yb)) return fail(GGML_HIP_ERR_RUNTIME, "hipMalloc failed");
    HIP_TRY(hipMemcpyAsync(c->src1.p, x, xb, hipMemcpyHostToDevice, c->stream));
    rc = ggml_hip_quantize_rows_dev(type, (const float *)c->src1.p, 1, k, c->dst.p, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(y, c->dst.p, yb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GGML_HIP_OK;
}

int ggml_hip_dequantize_row(int type, const void *x, float *y, int k) {
    if (!x || !y || k <= 0) return fail(GGML_HIP_ERR_ARG, "bad argument");
    int rc = ensure_init();
    if (rc) return rc;
    if (type < 0 || type >= GGML_TYPE_COUNT || !is_q(type)) return fail(GGML_HIP_ERR_TYPE, "not a quantized type");
    DeviceCtx *c = call_slot();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    rc = c->make_current();
    if (rc) return rc;
    const size_t yb = (size_t)k * 4, xb = TSIZE[type] * (size_t)(k / BLCK[type]);
    if (c->src1.ensure(xb) || c->dst.ensure(yb)) return fail(GGML_HIP_ERR_RUNTIME, "hipMalloc failed");
    HIP_TRY(hipMemcpyAsync(c->src1.p, x, xb, hipMemcpyHostToDevice, c->stream));
    rc = ggml_hip_dequantize_rows_dev(type, c->src1.p, 1, k, (float *)c->dst.p, c->stream);
    if (rc) return rc;
    HIP_TRY(hipMemcpyAsync(y, c->dst.p, yb, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return GGML_HIP_OK;
}

int ggml_hip_vec_dot(int type, int n, float *s, const void *vx, const void *vy) {
    if (!s || !vx || !vy || n <= 0) return fail(GGML_HIP_ERR_ARG, "bad argument");
    const int vt = (type >= 0 && type < GGML_TYPE_COUNT) ? vec_dot_type(type) : -1;
    if (vt < 0) return fail(GGML_HIP_ERR_TYPE, "vec_dot: type %d has no usable slot (D7/D8)", type);
    if (n % QK != 0) return fail(GGML_HIP_ERR_SHAPE, "n %% 32 != 0 (Ggml.cs:1129)");
    int rc = ensure_init();
    if (rc) return rc;
    DeviceCtx *c = call_slot();
    std::lock_guard<std::recursive_mutex> lk(c->mu);
    ggml_hip_weight *w = nullptr;
    const uint64_t xb = (uint64_t)row_bytes_of(type, n);
    rc = make_weight(c, type, vx, true, n, 1, xb, 0, 1, c->stream, &w);
    if (rc) return rc;
    const size_t yb = TSIZE[vt] * (size_t)(n / QK);
    const size_t wb = ggml_hip_mul_mat_work_size(type, n, 1);
    rc = GGML_HIP_OK;
    if (c->src1.ensure(yb) || c->work.ensure(wb) || c->dst.ensure(4)) rc = fail(GGML_HIP_ERR_RUNTIME, "hipMalloc failed");
    hipError_t e = hipSuccess;
    if (!rc) {
        e = hipMemcpyAsync(c->src1.p, vy, yb, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = launch_q8_aos_to_planes(vt, c->src1.p, 1, n, act_carve(c->work.p, n, pad_act(1)), c->stream);
        if (e == hipSuccess) rc = ggml_hip_mul_mat_compute_dev(w, 1, (float *)c->dst.p, 1, c->work.p, wb, c->stream);
        if (e == hipSuccess && !rc) e = hipMemcpyAsync(s, c->dst.p, 4, hipMemcpyDeviceToHost, c->stream);
        if (e == hipSuccess && !rc) e = hipStreamSynchronize(c->stream);
    }
    ggml_hip_weight_free(w);
    if (e != hipSuccess) return fail(GGML_HIP_ERR_RUNTIME, "vec_dot: %s", hipGetErrorString(e));
    return rc;
}

int ggml_hip_relayout_gathered_dev(const float *d_gathered, int G, int64_t N, int64_t Ms, float *d_dst, int64_t M,
                                   int64_t ldd, void *stream) {
    if (!d_gathered || !d_dst || G <= 0 || Ms <= 0) return fail(GGML_HIP_ERR_ARG, "bad argument");
    if (ldd < M) return fail(GGML_HIP_ERR_SHAPE, "ldd < M");
    HIP_TRY(launch_relayout_gathered(d_gathered, G, N, Ms, d_dst, M, ldd, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_quantize_rows_src_dev(int type, int src_type, const void *d_x, int64_t ld, int64_t nrows, int64_t k,
                                   void *d_blocks, void *stream) {
    if (nrows <= 0) return GGML_HIP_OK;
    if (!d_x || !d_blocks) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (!(wq_ok(type) || type == GGML_TYPE_Q8_1))
        return fail(GGML_HIP_ERR_TYPE, "quantize: unsupported type %d", type);
    if (src_type != GGML_TYPE_F32 && src_type != GGML_TYPE_F16) return fail(GGML_HIP_ERR_TYPE, "quantize: source must be F32 or F16");
    if (k % QK != 0 || ld < k) return fail(GGML_HIP_ERR_SHAPE, "k %% 32 != 0 or ld < k");
    if (src_type == GGML_TYPE_F16 && ld % 8 != 0) return fail(GGML_HIP_ERR_SHAPE, "f16 rows must be 16-byte aligned (ld %% 8)");
    if (src_type == GGML_TYPE_F32 && ld % 4 != 0) return fail(GGML_HIP_ERR_SHAPE, "f32 rows must be 16-byte aligned (ld %% 4)");
    HIP_TRY(launch_quantize_rows(type, src_type, d_x, ld, nrows, k, d_blocks, (hipStream_t)stream));
    return GGML_HIP_OK;
}

int ggml_hip_add_q_f32_rows_dev(int type, const void *d_blocks_in, const float *d_x, int64_t nrows, int64_t k,
                                void *d_blocks_out, void *stream) {
    if (nrows <= 0) return GGML_HIP_OK;
    if (!d_blocks_in || !d_x || !d_blocks_out) return fail(GGML_HIP_ERR_ARG, "null argument");
    if (!wq_ok(type))
        return fail(GGML_HIP_ERR_TYPE, "add_q_f32: unsupported type %d", type);
    if (k % QK != 0) return fail(GGML_HIP_ERR_SHAPE, "k %% 32 != 0 (Ggml.cs:4893)");
    HIP_TRY(launch_add_q_f32(type, d_blocks_in, d_x, nrows, k, d_blocks_out, (hipStream_t)stream));
    return GGML_HIP_OK;
}

}  // extern "C"
