// glint_axpy.h -- the arithmetic of an axpy contribution (the contracts in include/glint_gpu.h, "Row axpy
// push" and "Row-pair axpy push"), shared by the row axpy push (glint_rowaxpy.hip) and the row-pair axpy
// push (glint_pairs.hip): a product and a sum each rounded on its own, and a value handed round a wave.
// One statement of the rounding, so the two calls cannot drift apart in a bit.
#pragma once
#include "glint_device.h"

namespace glint {

// a * b and a + b each rounded on its own: hipcc contracts a * b + c into v_fma_* by default, and a
// fused product is not the contract's (dot_step's rule, glint_dot.h). Int/Long wrap.
__device__ __forceinline__ double axpy_mul(double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return p;
}
__device__ __forceinline__ float axpy_mul(float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return p;
}
__device__ __forceinline__ long long axpy_mul(long long a, long long b) { return (long long)((u64)a * (u64)b); }
__device__ __forceinline__ int axpy_mul(int a, int b) { return (int)((u32)a * (u32)b); }
__device__ __forceinline__ double axpy_add(double a, double b) {
#pragma clang fp contract(off)
  const double r = a + b;
  return r;
}
__device__ __forceinline__ float axpy_add(float a, float b) {
#pragma clang fp contract(off)
  const float r = a + b;
  return r;
}
__device__ __forceinline__ long long axpy_add(long long a, long long b) { return vadd(a, b); }
__device__ __forceinline__ int axpy_add(int a, int b) { return vadd(a, b); }

// lane l's value of v in every lane (l wave-uniform): v_readlane_b32 per dword
template <typename V>
__device__ __forceinline__ V lane_get(V v, u32 l) {
  int w[sizeof(V) / 4];
  __builtin_memcpy(w, &v, sizeof(V));
#pragma unroll
  for (int k = 0; k < (int)(sizeof(V) / 4); ++k) w[k] = __builtin_amdgcn_readlane(w[k], (int)l);
  V r;
  __builtin_memcpy(&r, w, sizeof(V));
  return r;
}

}  // namespace glint
