// wcache.cpp -- the Seam-1 weight cache of a slot (ctx.h CachedWeight): the device form of a leaf src0, kept under a key of its host
// pointer, type, shape, strides and row shard.  Acquisition for one call (hit, or upload with one evict-and-retry, then insert under
// the budget), invalidation by every writer of host memory, least-recently-used eviction, the budget knob and the stats.
#include "ctx.h"

namespace ghip {

// a budget per slot in bytes (0 = the device's memory is the limit): ggml_hip_debug_weight_cache_budget, a test hook
static std::atomic<size_t> g_weight_cache_budget{0};

void DeviceCtx::invalidate(const void *host, size_t bytes) {
    const uint8_t *a = (const uint8_t *)host, *b = a + (bytes ? bytes : 1);
    bool synced = false;
    for (auto it = cache.begin(); it != cache.end();) {
        const uint8_t *x = (const uint8_t *)it->second.host, *y = x + (it->second.host_bytes ? it->second.host_bytes : 1);
        if (x < b && a < y) {
            if (!synced) { (void)sync_all(); drop_captured(); synced = true; }     // kernels of an open graph scope may still read the entry
            for (ggml_hip_weight *w : it->second.slices) ggml_hip_weight_free(w);
            cache_bytes -= it->second.dev_bytes < cache_bytes ? it->second.dev_bytes : cache_bytes;
            it = cache.erase(it);
        } else {
            ++it;
        }
    }
}
void DeviceCtx::free_cache() {
    drop_captured();
    for (auto &kv : cache)
        for (ggml_hip_weight *w : kv.second.slices) ggml_hip_weight_free(w);
    cache.clear();
    cache_bytes = 0;
}
size_t DeviceCtx::evict_lru(size_t need, size_t budget, const CacheKey *keep) {
    size_t freed = 0;
    bool synced = false;
    for (;;) {
        const bool over = budget ? cache_bytes + need > budget : freed < need;
        if (!over) break;
        auto victim = cache.end();
        for (auto it = cache.begin(); it != cache.end(); ++it) {
            if (keep && it->first == *keep) continue;
            if (victim == cache.end() || it->second.last_use < victim->second.last_use) victim = it;
        }
        if (victim == cache.end()) break;                   // nothing left that may go
        if (!synced) { (void)sync_all(); drop_captured(); synced = true; }     // kernels in flight (an open graph scope) may still read the entry
        for (ggml_hip_weight *w : victim->second.slices) ggml_hip_weight_free(w);
        freed += victim->second.dev_bytes;
        cache_bytes -= victim->second.dev_bytes < cache_bytes ? victim->second.dev_bytes : cache_bytes;
        cache.erase(victim);
        ++cache_evictions;
    }
    return freed;
}

// the 2-D slices of src0's rows [r0, r1) uploaded to this slot, from dev_src (a device copy of the rows) or from host memory
static int upload_slices(DeviceCtx *c, const ggml_tensor *src0, const uint8_t *dev_src, int64_t r0, int64_t r1, std::vector<ggml_hip_weight *> *slices) {
    int rc = GGML_HIP_OK;
    for (int64_t i03 = 0; i03 < src0->ne[3] && !rc; ++i03)
        for (int64_t i02 = 0; i02 < src0->ne[2] && !rc; ++i02) {
            ggml_hip_weight *w = nullptr;
            const size_t off = (size_t)(i02 * src0->nb[2] + i03 * src0->nb[3]);
            rc = make_weight(c, src0->type, (dev_src ? dev_src : (const uint8_t *)src0->data) + off, dev_src == nullptr, src0->ne[0], src0->ne[1],
                             src0->nb[1], r0, r1, c->stream, &w);
            if (!rc) slices->push_back(w);
        }
    return rc;
}

int DeviceCtx::acquire_weights(const ggml_tensor *src0, int64_t r0, int64_t r1, bool cacheable, bool in_graph, std::vector<ggml_hip_weight *> *W,
                               std::vector<ggml_hip_weight *> *owned) {
    const int type = src0->type;
    const CacheKey key{src0->data, type, src0->ne[0], src0->ne[1], src0->ne[2], src0->ne[3], src0->nb[1], src0->nb[2], src0->nb[3], r0, r1};
    auto it = cacheable ? cache.find(key) : cache.end();
    if (it != cache.end()) {
        *W = it->second.slices;
        it->second.last_use = ++cache_clock;
        return GGML_HIP_OK;
    }
    // the source rows: a device copy left by the node that computed them (graph scope), else host memory -- which an
    // earlier node's device -> host copy may still be filling, so wait for this slot's streams first
    const uint8_t *dev_src = nullptr;
    if (!cacheable && in_graph && ggml_hip_type_size(type) == src0->nb[0] && (type == GGML_TYPE_F32) && contiguous_f32(src0))
        dev_src = (const uint8_t *)resident_lookup(src0->data, (size_t)nelem(src0) * 4);
    int rc = GGML_HIP_OK;
    if (!dev_src && in_graph) { rc = pay_and_sync(); if (rc) return rc; }
    scope_dirty();                                // a weight upload (allocation, staging, a wait) is not replayable
    std::vector<ggml_hip_weight *> slices;
    // r5: the cache is bounded by the device's memory (and by the budget of ggml_hip_debug_weight_cache_budget, a test hook): when an
    // upload cannot be allocated, the least recently used leaf entries go and the upload is tried ONCE more (it used
    // to be an error return for good -- resident images are 1.5-2.6 x the file format)
    for (int attempt = 0; attempt < 2; ++attempt) {
        rc = upload_slices(this, src0, dev_src, r0, r1, &slices);
        if (rc != GGML_HIP_ERR_RUNTIME || attempt == 1 || cache.empty()) break;
        size_t have = 0;
        for (ggml_hip_weight *x : slices) { have += x->bytes; ggml_hip_weight_free(x); }
        slices.clear();
        (void)hipGetLastError();
        // (how much the failed upload wanted is not known here: at least what its slices so far took, and no less than a quarter of the cache)
        const size_t want = have > cache_bytes / 4 ? have : cache_bytes / 4;
        if (evict_lru(want ? want : 1, 0, nullptr) == 0) break;
    }
    if (rc) {
        for (ggml_hip_weight *x : slices) ggml_hip_weight_free(x);
        return rc;
    }
    *W = slices;
    if (cacheable) {
        CachedWeight cw;
        cw.host = src0->data; cw.host_bytes = tensor_host_bytes(src0); cw.slices = slices;
        cw.row_begin = r0; cw.row_end = r1;
        cw.last_use = ++cache_clock;
        for (ggml_hip_weight *x : slices) cw.dev_bytes += x->bytes;
        cache_bytes += cw.dev_bytes;
        cache.emplace(key, std::move(cw));
        const size_t budget = g_weight_cache_budget.load(std::memory_order_relaxed);
        if (budget && cache_bytes > budget) evict_lru(0, budget, &key);   // (the entry this call runs on stays, whatever its size)
    } else if (in_graph) {
        for (ggml_hip_weight *x : slices) transient.push_back(x);     // alive until graph end (kernels in flight)
    } else {
        for (ggml_hip_weight *x : slices) owned->push_back(x);        // the caller's: freed when its call is over
    }
    return GGML_HIP_OK;
}

}  // namespace ghip

using namespace ghip;

extern "C" {

void ggml_hip_debug_weight_cache_budget(size_t bytes_per_slot) { g_weight_cache_budget.store(bytes_per_slot, std::memory_order_relaxed); }
/* what the cache holds / has evicted so far */
void ggml_hip_debug_weight_cache_stats(uint64_t *entries, uint64_t *bytes, uint64_t *evictions) {
    uint64_t n = 0, b = 0, e = 0;
    for (int i = 0; i < n_slots(); ++i) {
        DeviceCtx *c = slot(i);
        std::lock_guard<std::recursive_mutex> lk(c->mu);
        n += c->cache.size(); b += c->cache_bytes; e += c->cache_evictions;
    }
    if (entries) *entries = n;
    if (bytes) *bytes = b;
    if (evictions) *evictions = e;
}

}  // extern "C"
