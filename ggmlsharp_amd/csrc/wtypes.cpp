// wtypes.cpp -- the table of weight types (common.h `wtype`): what a type id IS, said once.  The reference's types come from BLCK / TSIZE
// and the predicates of ctx.h; an extension type is one row of EXT.  DESIGN.md "Adding a weight type".
#include "ctx.h"
#include <array>

using namespace ghip;

namespace {

// the row functions that do not have the table's signature already
hipError_t quantize_ref(int type, const float *x, int64_t nrows, int64_t k, void *blocks, hipStream_t st) {
    return launch_quantize_rows(type, GGML_TYPE_F32, x, k, nrows, k, blocks, st);
}
hipError_t quantize_bf16(int, const float *x, int64_t nrows, int64_t k, void *blocks, hipStream_t st) {   // f32 -> bf16 by the one rule (dense16.hip)
    return launch_f32_to_bf16_rows(x, nrows * k, (uint16_t *)blocks, st);
}
hipError_t dequantize_bf16(int, const void *blocks, int64_t nrows, int64_t k, float *y, hipStream_t st) {  // bf16 -> f32, exact
    return launch_bf16_to_f32_rows((const uint16_t *)blocks, nrows * k, y, st);
}

#define KQ_OPS  launch_kq_to_planar, launch_planar_to_kq, launch_quantize_kq, launch_dequantize_kq
#define IQ4_OPS launch_iq4_to_planar, launch_planar_to_iq4, launch_quantize_iq4, launch_dequantize_iq4
// Q5_K / Q4_K: eight k-blocks of the planar Q5_1 form per super-block.  Q6_K / Q3_K / Q2_K / IQ4_XS: the two-scale int8 form (the planar Q4_2
// form on its int8 planes alone, two_scale.h); Q2_K's min term by the min pass.  IQ4_NL: after the codebook lookup a PLAIN Q8_0 weight.
// BF16: F16's resident form with bf16 bits -- a native type (the weight's type is the id itself), its own kernels' twins.
const wtype EXT[] = {
    // id                 blck bytes resident            origin          q8k    min    slot own_i8 x_align  operations
    {GGML_HIP_TYPE_Q2_K,   256,  84, GGML_TYPE_Q4_2,     WT_ORIGIN_EXT,  true,  true,  32,  true,  16, KQ_OPS},
    {GGML_HIP_TYPE_Q3_K,   256, 110, GGML_TYPE_Q4_2,     WT_ORIGIN_EXT,  true,  false, 16,  true,  16, KQ_OPS},
    {GGML_HIP_TYPE_Q4_K,   256, 144, GGML_TYPE_Q5_1,     WT_ORIGIN_EXT,  true,  false, 16,  false, 16, KQ_OPS},
    {GGML_HIP_TYPE_Q5_K,   256, 176, GGML_TYPE_Q5_1,     WT_ORIGIN_EXT,  true,  false, 16,  false, 16, KQ_OPS},
    {GGML_HIP_TYPE_Q6_K,   256, 210, GGML_TYPE_Q4_2,     WT_ORIGIN_EXT,  true,  false, 32,  true,  16, KQ_OPS},
    {GGML_HIP_TYPE_IQ4_NL,  32,  18, GGML_TYPE_Q8_0,     WT_ORIGIN_UP,   false, false, 0,   false, 16, IQ4_OPS},
    {GGML_HIP_TYPE_IQ4_XS, 256, 136, GGML_TYPE_Q4_2,     WT_ORIGIN_EXT,  true,  false, 16,  true,  16, IQ4_OPS},
    {GGML_HIP_TYPE_BF16,     1,   2, GGML_HIP_TYPE_BF16, WT_ORIGIN_NONE, false, false, 0,   false, 0,
     launch_repack_to_planar, launch_planar_to_aos, quantize_bf16, dequantize_bf16},
};
#undef KQ_OPS
#undef IQ4_OPS

// a reference type: sized by BLCK / TSIZE, a weight where weight_type_ok says so, row functions where the reference has working slots
wtype ref_row(int t) {
    wtype r = {t, BLCK[t], TSIZE[t], t, WT_ORIGIN_NONE, false, false, 0, false, 0, nullptr, nullptr, nullptr, nullptr};
    if (weight_type_ok(t)) { r.to_planar = launch_repack_to_planar; r.from_planar = launch_planar_to_aos; }
    if (wq_ok(t) || t == GGML_TYPE_Q8_1) r.quantize = quantize_ref;
    if (wq_ok(t)) r.dequantize = launch_dequantize_rows;               // (Q8_1's slot is null, Ggml.cs:278)
    return r;
}

}  // namespace

const wtype *wtype_of(int id) {
    static const std::array<wtype, GGML_TYPE_COUNT> ref = [] {
        std::array<wtype, GGML_TYPE_COUNT> a;
        for (int t = 0; t < GGML_TYPE_COUNT; ++t) a[(size_t)t] = ref_row(t);
        return a;
    }();
    if (id >= 0 && id < GGML_TYPE_COUNT) return &ref[(size_t)id];
    for (const wtype &r : EXT)
        if (r.id == id) return &r;
    return nullptr;
}
