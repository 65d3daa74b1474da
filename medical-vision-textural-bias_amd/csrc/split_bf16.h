// Split precision on the bf16 matrix cores: an f32 operand as three bf16 parts and the six-product step.
//
//   x = x0 + x1 + x2 exactly:  x0 = bf16(x), x1 = bf16(x - x0), x2 = bf16(x - x0 - x1), each rounded to
//   nearest even (v_cvt_pk_bf16_f32).  bf16 has f32's exponent range, so no scaling is needed.  x0 keeps 8
//   significand bits, x - x0 (an exact f32, at most 2^-8 |x|) the 16 below them; x1 takes the upper 8 of
//   those and what is left fits 8 bits, so x2 is exact.  (Parts below the smallest normal 2^-126 follow
//   the device's denormal mode: they are at most 2^-17 of x and only arise for |x| < 2^-109.)
//
//   a . b over a 32-k MFMA step = the six part products that reach 2^-24 of the leading one,
//   a1 b1, a0 b2, a2 b0, a0 b1, a1 b0, a0 b0, accumulated in f32 on v_mfma_f32_16x16x32_bf16: 6 x 16
//   cycles per 32 k where v_mfma_f32_16x16x4_f32 takes 8 x 32.  The five small products (at most 2^-8 of
//   the leading one) go, smallest first, into an accumulator of their own, `lo`, whose roundings are 2^-8
//   of the result's; the leading a0 b0 goes into `hi`, which is rounded once per 32 k (14 times for the 432
//   terms of a 3x3x3 x 16 stencil where a single chain rounds 84 times and the f32 MFMA chain 108 times);
//   the result is hi + lo, added once at the end.  Two independent chains also keep the matrix core from
//   waiting on its own result.  The
//   dropped a1 b2, a2 b1, a2 b2 are below 2^-25 |a b| each (2^-8 . 2^-17), of either sign, against the
//   2^-24 of the running sum that every f32 accumulation rounds by; tests/test_split_bf16_cpu.py holds the
//   dot-product error to that of an f32 chain.  (A truncated leading part would be one instruction less,
//   but doubles x1 and x2 and so quadruples the dropped terms: in that test it loses to the f32 chain.)
//
// Non-finite and huge inputs: the value is clamped to +-0x7f7f7fff, the largest f32 that rounds to a
// finite bf16, before the leading part is taken (the residual is of the unclamped value), so a finite f32
// (FLT_MAX included) never becomes an infinite bf16; above the clamp x0 is the truncated value and the
// residuals are at most 2^-7 of it.  Sums that overflow f32 give +-inf as an f32 chain would, up to the
// order of the additions.  An infinite input has a finite x0, x1 = +-inf and x2 = NaN: every output it
// reaches is NaN (an f32 chain may keep +-inf).  NaN stays NaN (through x1).
#pragma once
#include <hip/hip_runtime.h>

namespace tb {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef float f32x2s __attribute__((ext_vector_type(2)));
typedef float f32x4s __attribute__((ext_vector_type(4)));

// Two floats -> their three parts, each a packed bf16 pair (a in the low half): one v_cvt_pk_bf16_f32
// per level.
__device__ __forceinline__ void split3_pk(float a, float b, unsigned& p0, unsigned& p1, unsigned& p2) {
  const float top = __uint_as_float(0x7f7f7fffu);
  const bf16x2 h = __builtin_convertvector(
      f32x2s{__builtin_amdgcn_fmed3f(a, -top, top), __builtin_amdgcn_fmed3f(b, -top, top)}, bf16x2);
  p0 = __builtin_bit_cast(unsigned, h);
  const float ra = a - __uint_as_float(p0 << 16), rb = b - __uint_as_float(p0 & 0xffff0000u);
  const bf16x2 m = __builtin_convertvector(f32x2s{ra, rb}, bf16x2);
  p1 = __builtin_bit_cast(unsigned, m);
  const float sa = ra - __uint_as_float(p1 << 16), sb = rb - __uint_as_float(p1 & 0xffff0000u);
  const bf16x2 l = __builtin_convertvector(f32x2s{sa, sb}, bf16x2);
  p2 = __builtin_bit_cast(unsigned, l);
}

// Eight floats (k order) -> the three 8 x bf16 MFMA fragments.
__device__ __forceinline__ void split3(const float (&v)[8], bf16x8& p0, bf16x8& p1, bf16x8& p2) {
  unsigned q[3][4];
#pragma unroll
  for (int j = 0; j < 4; ++j) split3_pk(v[2 * j], v[2 * j + 1], q[0][j], q[1][j], q[2][j]);
  typedef unsigned u32x4 __attribute__((ext_vector_type(4)));
  p0 = __builtin_bit_cast(bf16x8, u32x4{q[0][0], q[0][1], q[0][2], q[0][3]});
  p1 = __builtin_bit_cast(bf16x8, u32x4{q[1][0], q[1][1], q[1][2], q[1][3]});
  p2 = __builtin_bit_cast(bf16x8, u32x4{q[2][0], q[2][1], q[2][2], q[2][3]});
}

// hi + lo += a . b over one 32-k step: the five small products into lo, smallest first, a0 b0 into hi.
__device__ __forceinline__ void mfma_split6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4s& hi, f32x4s& lo) {
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[1], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[2], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[2], b[0], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[1], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[1], b[0], lo, 0, 0, 0);
  hi = __builtin_amdgcn_mfma_f32_16x16x32_bf16(a[0], b[0], hi, 0, 0, 0);
}

// The same step on v_mfma_f32_32x32x16_bf16 (16 k, a 32 x 32 result: 6 x 32 cycles where the sixteen
// mfma_f32_32x32x2f32 of 32 k take 1024, and half the LDS bytes per FLOP of the 16 x 16 form), same order.
typedef float f32x16s __attribute__((ext_vector_type(16)));

__device__ __forceinline__ void mfma_split6_32(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x16s& hi, f32x16s& lo) {
  lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[1], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[2], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[2], b[0], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[1], lo, 0, 0, 0);
  lo = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[1], b[0], lo, 0, 0, 0);
  hi = __builtin_amdgcn_mfma_f32_32x32x16_bf16(a[0], b[0], hi, 0, 0, 0);
}

}  // namespace tb
