// The operand split of every split-bf16 kernel of the library, host and device: x = hi + lo with hi = RNE_bf16(x),
// lo = RNE_bf16(x - hi).
#pragma once
#include <hip/hip_runtime.h>

namespace v3d {

typedef unsigned int u32x2 __attribute__((ext_vector_type(2)));

// fp32 -> bf16 bits, round to nearest even (finite values), and the fp32 value of bf16 bits
__host__ __device__ __forceinline__ unsigned bf16_rne(float x) {
  const unsigned u = __builtin_bit_cast(unsigned, x);
  return (u + 0x7fffu + ((u >> 16) & 1u)) >> 16;
}
__host__ __device__ __forceinline__ float bf16_value(unsigned h) { return __builtin_bit_cast(float, h << 16); }

// two fp32 -> two bf16 packed in one dword, a in the low half: one v_cvt_pk_bf16_f32 (round to nearest even in hardware, the
// bits of bf16_rne for finite values)
__device__ __forceinline__ unsigned pack_bf16x2(float a, float b) {
  typedef float f32x2_ __attribute__((ext_vector_type(2)));
  typedef __bf16 bf16x2_ __attribute__((ext_vector_type(2)));
  return __builtin_bit_cast(unsigned, __builtin_convertvector((f32x2_){a, b}, bf16x2_));
}
// The split of four values on packed pairs: 12 instead of ~50 vector instructions in the epilogues
__device__ __forceinline__ void split4(float a, float b, float c, float d, u32x2& hp, u32x2& lp) {
  hp = (u32x2){pack_bf16x2(a, b), pack_bf16x2(c, d)};
  lp = (u32x2){pack_bf16x2(a - __uint_as_float(hp.x << 16), b - __uint_as_float(hp.x & 0xffff0000u)),
               pack_bf16x2(c - __uint_as_float(hp.y << 16), d - __uint_as_float(hp.y & 0xffff0000u))};
}

}  // namespace v3d
