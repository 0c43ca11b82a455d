// Building blocks of the split-fp16 ("f16x3") matrix kernels -- igemm_f16x3.hip, igemm_pp.hip, wgrad_f16x3.hip and
// bwd_joint.hip -- that must agree bit for bit across them: ONE definition each.
#pragma once
#include "common.h"

typedef _Float16 f16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));
typedef unsigned int u32x4 __attribute__((ext_vector_type(4)));
typedef __attribute__((__vector_size__(4 * sizeof(short)))) short tr_v4i16;

// hi = fp16(x*s), lo = fp16(x*s - hi) for 4 elements in EIGHT vector instructions: v_fma_mix{lo,hi}_f16 multiplies in
// fp32, adds an fp16 (or zero) and rounds once to fp16 into one half of the destination.  (s is a power of two and
// x*s - hi is exactly representable, so the bits equal the two-step form (half)(x*s - (float)hi).)  hipcc's own lowering
// of the C expression spent 13 instructions per 4 elements, part of them packed-fp32 ops that issue at half rate next to
// MFMAs -- and this split runs in the matrix waves' own instruction stream, once per staged element.
__device__ __forceinline__ void dc_split_f16(const f32x4 v, float s, u32x2& hi, u32x2& lo) {
  unsigned h01, h23, l01, l23;
  asm("v_fma_mixlo_f16 %0, %4, %8, 0\n\t"
      "v_fma_mixlo_f16 %1, %6, %8, 0\n\t"
      "v_fma_mixhi_f16 %0, %5, %8, 0\n\t"
      "v_fma_mixhi_f16 %1, %7, %8, 0\n\t"
      "v_fma_mixlo_f16 %2, %4, %8, -%0 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixlo_f16 %3, %6, %8, -%1 op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %2, %5, %8, -%0 op_sel:[0,0,1] op_sel_hi:[0,0,1]\n\t"
      "v_fma_mixhi_f16 %3, %7, %8, -%1 op_sel:[0,0,1] op_sel_hi:[0,0,1]"
      : "=&v"(h01), "=&v"(h23), "=&v"(l01), "=&v"(l23)
      : "v"(v[0]), "v"(v[1]), "v"(v[2]), "v"(v[3]), "v"(s));
  hi = u32x2{h01, h23};
  lo = u32x2{l01, l23};
}

// One MFMA operand (8 consecutive k per lane) of a tile whose contraction index is its ROW index: two hardware-transposing
// ds_read_b64_tr_b16 -- each 16-lane group reads a 4-row x 16-channel block and every lane receives its channel's 4 rows.
__device__ __forceinline__ f16x8 dc_tr_frag(const char* base, int off1, int off2) {
  typedef __attribute__((address_space(3))) tr_v4i16* lds_p;
  const tr_v4i16 r0 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(base + off1));
  const tr_v4i16 r1 = __builtin_amdgcn_ds_read_tr16_b64_v4i16((lds_p)(base + off2));
  typedef short s16x8 __attribute__((ext_vector_type(8)));
  s16x8 v = {r0[0], r0[1], r0[2], r0[3], r1[0], r1[1], r1[2], r1[3]};
  return __builtin_bit_cast(f16x8, v);
}

// acc += a * b for split operands: a_lo*b_hi, then a_hi*b_lo, then a_hi*b_hi (the lo*lo term is dropped).  The order is part
// of the numerics: every f16x3 kernel adds the two small products first.
__device__ __forceinline__ void dc_mfma3(const f16x8 ah, const f16x8 al, const f16x8 bh, const f16x8 bl, f32x16& acc) {
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(al, bh, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bl, acc, 0, 0, 0);
  acc = __builtin_amdgcn_mfma_f32_32x32x16_f16(ah, bh, acc, 0, 0, 0);
}

// A data-gradient epilogue whose output v IS `da` of the BatchNorm layer in front: one element of that layer's pass-1 sums
// (sum dy, sum dy*xhat, max |dy|), dy = da * [fmaf(z, gsc, gsh) > 0] with (gsc, gsh) = dc_bn_affine(mu, is, gamma, beta) --
// the forward's own expression: identical ReLU gate.  live = the element exists (inside the image, column < Ncols).
__device__ __forceinline__ void dc_bnred_accum(float v, float z, float gsc, float gsh, float mu, float is, bool live,
                                               float& s1, float& s2, float& amax) {
  const float y = __builtin_fmaf(z, gsc, gsh);
  const float dy = (live && y > 0.f) ? v : 0.f;
  s1 += dy;
  s2 = __builtin_fmaf(dy, (z - mu) * is, s2);
  amax = fmaxf(amax, fabsf(dy));
}
