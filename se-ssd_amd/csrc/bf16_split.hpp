// Three-way bf16 split of f32 operands for the bf16 matrix cores (dense_wino_sk.hip shape 3, dense_deconv_split.hip):
// a = a0 + a1 + a2, each term rounded to nearest from the exact f32 residual of the previous one.
#pragma once
#include <hip/hip_runtime.h>

namespace sessd {

typedef __bf16 split_bf16x2 __attribute__((ext_vector_type(2)));
typedef float split_f32x2 __attribute__((ext_vector_type(2)));

// (x0, x1) -> three packed bf16 pairs with x = t0 + t1 + t2 (round to nearest at every step; the residuals are exact in f32)
__device__ __forceinline__ unsigned pk_bf16(float x0, float x1) {
  return __builtin_bit_cast(unsigned, __builtin_convertvector((split_f32x2){x0, x1}, split_bf16x2));
}
__device__ __forceinline__ void split3_pk(float x0, float x1, unsigned& t0, unsigned& t1, unsigned& t2) {
  t0 = pk_bf16(x0, x1);
  x0 -= __builtin_bit_cast(float, t0 << 16); x1 -= __builtin_bit_cast(float, t0 & 0xFFFF0000u);
  t1 = pk_bf16(x0, x1);
  x0 -= __builtin_bit_cast(float, t1 << 16); x1 -= __builtin_bit_cast(float, t1 & 0xFFFF0000u);
  t2 = pk_bf16(x0, x1);
}

}  // namespace sessd
