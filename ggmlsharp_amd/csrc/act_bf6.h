// act_bf6.h -- the arithmetic of the bf6 activation image (kind 3), stated once: quantize.hip's lane-per-block INIT kernel (K1b) and the quantizer
// inside the fused K3m launch (gemm_qmx.hip) take scale, quants and digits from the statements below; K1b packs its two fragments with
// bf6_pack32_pair, the fused quantizer one at a time with bf6_pack32 (same instruction, same operands).
//   d = amax / 127, id = 1 / d                         Ggml.cs:751-752
//   q = round-half-even(v * id)                        Ggml.cs:758-759 (D1, D2)
//   q = 16 ah + al, ah = floor((q + 8) / 16) in [-8, 8], al in [-8, 7]: both exact in bf6 (e3m2)
//   32 digits -> one 192-bit MX operand fragment: v_cvt_scalef32_2xpk16_bf6_f32 packs a[i] at position 2i, b[i] at 2i + 1
#pragma once
#include "common.h"

using bf6_f32x16 = __attribute__((ext_vector_type(16))) float;
using bf6_u32x6 = __attribute__((ext_vector_type(6))) uint32_t;

__device__ __forceinline__ void bf6_block_scale(float amax, float &d, float &id) {
    d = amax / 127.0f;                                      // Ggml.cs:751
    id = d != 0.0f ? 1.0f / d : 0.0f;                       // Ggml.cs:752
}
__device__ __forceinline__ float bf6_quant(float v, float id) { return rintf(v * id); }                       // Ggml.cs:758-759 (D1, D2)
__device__ __forceinline__ float bf6_digit_hi(float q) { return floorf(fmaf(q, 0.0625f, 0.5f)); }              // ah = floor((q + 8) / 16) in [-8, 8]
__device__ __forceinline__ float bf6_digit_lo(float q, float ah) { return fmaf(ah, -16.0f, q); }               // al = q - 16 ah in [-8, 7]

// The two fragments of a block from the digits of its even / odd elements (he, ho: high digits; le, lo: low digits), as K1b packs them.  Through asm
// with early-clobber results: hipcc's builtin lets the 6-register result overlap the 32 source registers, and the instruction writes its result before it
// has read all of them.  Both converts in ONE statement, so that no result shares a register with ANY of the 64 sources: as two statements hipcc gave the
// second result the first convert's source registers and, in 22 of 100 launches, some rows came out with wrong quants 0..4 (tools/dbg_k1b.py; 8 wait
// states between the two did not help, distinct registers did: 0 of 250).  The instruction evidently reads its sources for many cycles after issue with
// no interlock; the trailing nops keep whatever the compiler puts into the source registers next at a distance as well.
__device__ __forceinline__ void bf6_pack32_pair(const bf6_f32x16 &he, const bf6_f32x16 &ho, const bf6_f32x16 &le, const bf6_f32x16 &lo, bf6_u32x6 &fh,
                                                bf6_u32x6 &fl) {
    asm volatile("v_cvt_scalef32_2xpk16_bf6_f32 %0, %2, %3, 1.0\n\ts_nop 7\n\tv_cvt_scalef32_2xpk16_bf6_f32 %1, %4, %5, 1.0\n\t"
                 "s_nop 15\n\ts_nop 15"
                 : "=&v"(fh), "=&v"(fl) : "v"(he), "v"(ho), "v"(le), "v"(lo));
}
// ONE fragment, for the quantizer inside K3m, which has no registers for 64 digits at once and packs the high digits, then reuses their registers for
// the low ones.  This form relies on DISTANCE, not on distinct registers: in the emitted kernel the second result does land in the first convert's source
// registers, and what keeps it right is that the first convert is long done -- its own 32 trailing wait states, then the ~60 vector instructions that
// compute the low digits stand between the two (K1b's failing form had 8 wait states and nothing else).  Evidence: tests/test_fused_init_gpu.py compares
// every image byte with K1b's over some 200 launches of 0.5 M blocks each, bit for bit.  Do not shorten the nops or hoist the second pack.
__device__ __forceinline__ bf6_u32x6 bf6_pack32(const bf6_f32x16 &a, const bf6_f32x16 &b) {
    bf6_u32x6 f;
    asm volatile("v_cvt_scalef32_2xpk16_bf6_f32 %0, %1, %2, 1.0\n\ts_nop 15\n\ts_nop 15" : "=&v"(f) : "v"(a), "v"(b));
    return f;
}
