// plan_dump -- every decision of csrc/plan.cpp's mat-mul planners over a fixed sweep, as one hash per line.  Host code only: it includes plan.h,
// calls no HIP function and needs no GPU.  A change that must not move a decision (a refactor of plan.cpp) is checked by running this before and
// after and comparing the lines: a line that differs names the function, the type pair and the force value to look at.
//
//   make -C ggmlsharp_amd/csrc plan_dump && tools/bin/plan_dump [--check]
//
// --check asserts three invariants and exits non-zero on a breach:
//   (i)   the tree id of a product is independent of M, outside MM_FLAG_WIDE;
//   (ii)  the image of a non-WIDE plan that is neither the fused mat-vec nor MMF_NONE, plus the pieces flag, equals plan_image_kind(type, K, N);
//   (iii) a one_call plan that is not MMF_GEMV_FUSED is field for field the COMPUTE-only plan.
// A plan_image_kind line hashes the image INIT really writes -- that of the COMPUTE-only plan at M = 1, as weight_image_kind takes it for a
// weight -- and the line `image_kind_differs` lists every (type, force, K, N) where plan_image_kind answers otherwise: together they pin the
// function, and a change of it at the listed points moves that one line alone.
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "../include/ggml_hip.h"
#include "../include/ggml_hip_ext.h"
#include "../ggmlsharp_amd/csrc/plan.h"

namespace {

constexpr int IMAGE_MIN_PIECES = 64;     // (common.h ACT_IMAGE_MIN_PIECES; common.h itself needs the HIP headers)
int64_t pad256(int64_t n) { return (n + 255) / 256 * 256; }   // (common.h pad_rows)

struct Hash {
    uint64_t h = 1469598103934665603ull;
    void add(int64_t v) { for (int i = 0; i < 8; ++i) { h ^= (uint64_t)(v >> (8 * i)) & 0xFF; h *= 1099511628211ull; } }
};

bool is_k3s(const mm_plan &p) { return p.family == MMF_K3S_MX || p.family == MMF_K3S_I8; }

void add_plan(Hash &h, const mm_plan &p, int type) {
    const int64_t f[] = {p.family, p.image, p.form, p.arith, p.ksplit, p.kstyle, p.kunit, p.tile_m, p.tile_n, p.waves, p.tiles_per_wave, p.wgs, p.flags,
                         p.nloc, p.wmt, (int64_t)plan_tree_id(p)};
    for (int64_t v : f) h.add(v);
    if (is_k3s(p)) { const k3s_slots s = plan_k3s_slots(p, type); h.add(s.slots); h.add(s.rot); h.add(s.rows); h.add(s.lds); }
}

bool same_plan(const mm_plan &a, const mm_plan &b) {
    return a.family == b.family && a.image == b.image && a.form == b.form && a.arith == b.arith && a.ksplit == b.ksplit && a.kstyle == b.kstyle &&
           a.kunit == b.kunit && a.tile_m == b.tile_m && a.tile_n == b.tile_n && a.waves == b.waves && a.tiles_per_wave == b.tiles_per_wave &&
           a.wgs == b.wgs && a.flags == b.flags && a.nloc == b.nloc && a.wmt == b.wmt;
}

int plan_image(const mm_plan &p) { return (p.image >= 0 && p.image <= 3 ? p.image : 0) | ((p.flags & MM_FLAG_MIN_PIECES) ? IMAGE_MIN_PIECES : 0); }

struct Pair { int type, ext; const char *name; };
const Pair PAIRS[] = {
    {GGML_TYPE_Q4_0, 0, "Q4_0"}, {GGML_TYPE_Q4_1, 0, "Q4_1"}, {GGML_TYPE_Q4_2, 0, "Q4_2"}, {GGML_TYPE_Q5_0, 0, "Q5_0"}, {GGML_TYPE_Q5_1, 0, "Q5_1"},
    {GGML_TYPE_Q8_0, 0, "Q8_0"}, {GGML_TYPE_F32, 0, "F32"}, {GGML_TYPE_F16, 0, "F16"}, {GGML_HIP_TYPE_BF16, 0, "BF16"},
    {GGML_TYPE_Q5_1, GGML_HIP_TYPE_Q5_K, "Q5_1/Q5_K"}, {GGML_TYPE_Q5_1, GGML_HIP_TYPE_Q4_K, "Q5_1/Q4_K"}, {GGML_TYPE_Q4_2, GGML_HIP_TYPE_Q6_K, "Q4_2/Q6_K"},
    {GGML_TYPE_Q4_2, GGML_HIP_TYPE_Q3_K, "Q4_2/Q3_K"}, {GGML_TYPE_Q4_2, GGML_HIP_TYPE_Q2_K, "Q4_2/Q2_K"}, {GGML_TYPE_Q4_2, GGML_HIP_TYPE_IQ4_XS, "Q4_2/IQ4_XS"},
};
bool quantized(int t) { return t >= GGML_TYPE_Q4_0 && t <= GGML_TYPE_Q8_0; }

// tests/test_plan_cpu.py's K and M values and the ones the bounds of plan.cpp turn on
const int64_t KS[] = {32, 64, 256, 512, 768, 1024, 1536, 1792, 2048, 2112, 2304, 4096, 4352, 8192, 11008, 13824, 16384, 20480, 22016, 28672, 32768, 33024,
                      36864, 79872, 79904};
const int64_t MS[] = {1, 31, 32, 100, 256, 512, 1000, 1024, 2048, 2049, 2560, 4000, 4096, 4112, 5120, 8192, 11008, 12000, 16384, 24576, 26000, 32000, 33000,
                      65536, 262144};
std::vector<int64_t> sweep_n() {
    std::vector<int64_t> ns;
    for (int64_t n = 1; n <= 1100; ++n) ns.push_back(n);
    for (int64_t n = 1100 + 37; n < 4200; n += 37) ns.push_back(n);
    for (int64_t n : {(int64_t)4200, (int64_t)65536, (int64_t)1 << 20, ((int64_t)1 << 21) + 4099}) ns.push_back(n);
    return ns;
}

uint64_t g_total = 1469598103934665603ull;
long long g_plans = 0, g_breach[3] = {0, 0, 0};
void line(const std::string &what, uint64_t h, long long n) {
    std::printf("%s hash=%016llx plans=%lld\n", what.c_str(), (unsigned long long)h, n);
    Hash t; t.h = g_total; t.add((int64_t)h); g_total = t.h;
    g_plans += n;
}
void breach(int which, const char *name, int force, int64_t M, int64_t K, int64_t N) {
    static const char *const names[] = {"i", "ii", "iii"};
    if (g_breach[which]++ < 10)
        std::fprintf(stderr, "invariant (%s) fails: %s force %d M %lld K %lld N %lld\n", names[which], name, force, (long long)M, (long long)K, (long long)N);
}

void dump_mul_mat(const std::vector<int64_t> &ns) {
    for (const Pair &pr : PAIRS)
        for (int force = 0; force < 4; ++force) {
            plan_set_force_gemm(force);
            Hash h[2];
            long long n_plans = 0;
            for (int64_t K : KS) {
                if (pr.ext != 0 && K % 256 != 0) continue;
                for (int64_t N : ns) {
                    const int ik = quantized(pr.type) ? plan_image_kind(pr.type, K, N) : 0;
                    uint32_t tree[2] = {0, 0};
                    bool have[2] = {false, false};
                    for (int64_t M : MS) {
                        mm_plan p[2];
                        for (int oc = 0; oc < 2; ++oc) {
                            p[oc] = plan_mul_mat(pr.type, pr.ext, M, K, N, oc != 0);
                            add_plan(h[oc], p[oc], pr.type);
                            ++n_plans;
                            if (p[oc].flags & MM_FLAG_WIDE) continue;
                            const uint32_t id = plan_tree_id(p[oc]);
                            if (have[oc] && id != tree[oc]) breach(0, pr.name, force, M, K, N);
                            tree[oc] = id; have[oc] = true;
                            const bool has_image = quantized(pr.type) && p[oc].family != MMF_GEMV_FUSED && p[oc].family != MMF_NONE;
                            if (has_image && plan_image(p[oc]) != ik) breach(1, pr.name, force, M, K, N);
                        }
                        if (p[1].family != MMF_GEMV_FUSED && !same_plan(p[0], p[1])) breach(2, pr.name, force, M, K, N);
                    }
                }
            }
            for (int oc = 0; oc < 2; ++oc)
                line(std::string("plan_mul_mat ") + pr.name + " force=" + std::to_string(force) + " one_call=" + std::to_string(oc), h[oc].h, n_plans / 2);
        }
    plan_set_force_gemm(0);
}

void dump_image_kind(const std::vector<int64_t> &ns) {
    std::string differs;
    long long n_differs = 0;
    for (const Pair &pr : PAIRS) {
        if (pr.ext != 0 || !quantized(pr.type)) continue;       // (the activation image of a quantized product: the dense types have none)
        for (int force = 0; force < 4; ++force) {
            plan_set_force_gemm(force);
            Hash h;
            long long n = 0;
            for (int64_t K : KS)
                for (int64_t N : ns) {
                    const int ik = plan_image_kind(pr.type, K, N), pk = plan_image(plan_mul_mat(pr.type, 0, 1, K, N, false));
                    h.add(pk); ++n;
                    if (ik != pk) {
                        ++n_differs;
                        differs += std::string(" ") + pr.name + "/" + std::to_string(force) + "/" + std::to_string(K) + "/" + std::to_string(N);
                        differs += "=" + std::to_string(ik) + "|" + std::to_string(pk);
                    }
                }
            line(std::string("plan_image_kind ") + pr.name + " force=" + std::to_string(force), h.h, n);
        }
    }
    plan_set_force_gemm(0);
    std::printf("image_kind_differs points=%lld (type/force/K/N=plan_image_kind|plan):%s\n", n_differs, differs.c_str());
}

void dump_group() {
    const int types[] = {GGML_TYPE_Q4_0, GGML_TYPE_Q4_1, GGML_TYPE_Q8_0, GGML_TYPE_Q5_0 /* refused */};
    const char *names[] = {"Q4_0", "Q4_1", "Q8_0", "Q5_0"};
    const int64_t ms[] = {512, 1024, 4096, 11008, 32000};
    const std::vector<std::vector<int64_t>> mixed = {{4096, 1024}, {1024, 4096}, {11008, 4096}, {512, 32000}, {4096, 1024, 1024}, {4096, 4096, 11008},
                                                     {11008, 11008, 4096}, {32000, 512, 512}, {512, 1024, 4096, 32000}, {4096, 4096, 1024, 1024},
                                                     {11008, 11008, 4096, 512}};
    std::vector<std::vector<int64_t>> groups;
    for (int n = 2; n <= 4; ++n)
        for (int64_t m : ms) groups.push_back(std::vector<int64_t>((size_t)n, m));
    groups.insert(groups.end(), mixed.begin(), mixed.end());
    for (int ti = 0; ti < 4; ++ti)
        for (int force = 0; force < 4; ++force) {
            plan_set_force_gemm(force);
            Hash h;
            long long n = 0;
            for (const auto &g : groups)
                for (int64_t N : {4, 5, 8, 9, 16, 17, 32, 33, 64, 65})
                    for (int64_t K : {1024, 2048, 4096, 11008, 32768, 33024}) {
                        int64_t M[4], Mpad[4];
                        for (size_t i = 0; i < g.size(); ++i) { M[i] = g[i]; Mpad[i] = pad256(g[i]); }
                        add_plan(h, plan_mul_mat_group(types[ti], 0, M, Mpad, (int)g.size(), K, N), types[ti]);
                        ++n;
                    }
            line(std::string("plan_mul_mat_group ") + names[ti] + " force=" + std::to_string(force), h.h, n);
        }
    plan_set_force_gemm(0);
}

void dump_id_grouped() {
    const int types[] = {GGML_TYPE_Q8_0, GGML_TYPE_Q5_0, GGML_TYPE_Q4_0, GGML_TYPE_Q5_1 /* refused */};
    const char *names[] = {"Q8_0", "Q5_0", "Q4_0", "Q5_1"};
    for (int ti = 0; ti < 4; ++ti)
        for (int force = 0; force < 4; ++force) {
            plan_set_force_gemm(force);
            Hash h;
            long long n = 0;
            for (int64_t M : {512, 4096, 14336})
                for (int64_t K : {1024, 4096, 11008}) {
                    h.add(plan_mul_mat_id_grouped_serves(types[ti], 0, M, K));
                    for (int n_expert : {1, 8, 64, 256})
                        for (int64_t P : {(int64_t)1, (int64_t)7, (int64_t)64, (int64_t)1000, (int64_t)1 << 20, ((int64_t)1 << 20) + 1}) {
                            add_plan(h, plan_mul_mat_id_grouped(types[ti], 0, M, K, n_expert, P), types[ti]);
                            ++n;
                        }
                }
            line(std::string("plan_mul_mat_id_grouped ") + names[ti] + " force=" + std::to_string(force), h.h, n);
        }
    plan_set_force_gemm(0);
}

}  // namespace

int main(int argc, char **argv) {
    const bool check = argc > 1 && std::strcmp(argv[1], "--check") == 0;
    const std::vector<int64_t> ns = sweep_n();
    dump_mul_mat(ns);
    dump_image_kind(ns);
    dump_group();
    dump_id_grouped();
    std::printf("overall hash=%016llx plans=%lld\n", (unsigned long long)g_total, g_plans);
    if (check) {
        std::printf("check: (i) %lld (ii) %lld (iii) %lld breaches\n", g_breach[0], g_breach[1], g_breach[2]);
        return g_breach[0] || g_breach[1] || g_breach[2] ? 1 : 0;
    }
    return 0;
}
