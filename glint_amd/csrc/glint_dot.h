// glint_dot.h -- the arithmetic of a row dot product (the contract in include/glint_gpu.h, "Row dot
// pull"), shared by the row dot pull (glint_rowdot.hip) and the scores of the top-k pull
// (glint_topk.hip): what a lane adds, in which order, and how a query vector is loaded. One statement of
// the order, so the two calls cannot drift apart in a bit.
#pragma once
#include "glint_device.h"

namespace glint {

constexpr int kDotTile = GLINT_DOT_QUERY_TILE;  // queries per wave when q > 1 (one when q == 1)
// row-strip loads in flight per wave (kRowSumDepth's pattern): 8 for one query per wave; 2 for a tile of
// queries, whose vector strips take the registers (8 there is ~195 VGPRs, 2 waves/SIMD)
template <int QT> constexpr int kDotDepth = QT == 1 ? 8 : 2;

// acc + (a * b) with the product rounded before the add: hipcc contracts a * b + c into v_fma_* by
// default, and a fused product is not the contract's. Int/Long wrap.
__device__ __forceinline__ double dot_step(double acc, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return acc + p;
}
__device__ __forceinline__ float dot_step(float acc, float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return acc + p;
}
__device__ __forceinline__ long long dot_step(long long acc, long long a, long long b) {
  return (long long)((u64)acc + (u64)a * (u64)b);
}
__device__ __forceinline__ int dot_step(int acc, int a, int b) { return (int)((u32)acc + (u32)a * (u32)b); }

// A lane's E columns [c, c + E) of one query vector: one 16-B load when XW (E * sizeof(V) == 16, the
// vector 16-B aligned), else element by element. Columns at or past cols are zeros.
template <typename V, int E, bool XW>
__device__ __forceinline__ void x_load(V (&t)[E], const V* __restrict__ xr, i64 c, i64 cols) {
  if (XW) {
    slice_load<V, E, true>(t, xr, c, cols);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) t[e] = c + e < cols ? xr[c + e] : V(0);
  }
}

// D = kDotDepth<QT> strips of the row from strip s on (FULL: all of them exist), then their products added to
// the QT lane sums in ascending strip -- hence column -- order. The strip loads are independent; the
// adds are the only chain. A lane whose columns lie past cols multiplies zeros: acc + (+0) leaves acc
// as it is, since a sum that started from +0 is never -0.
template <typename V, int E, bool VEC16, bool SELF, bool XW, int QT, bool FULL>
__device__ __forceinline__ void dot_batch(V (&acc)[QT], const V* __restrict__ row, const V* const (&xq)[QT], u32 s,
                                          u32 nstrips, int lane, i64 cols) {
  constexpr int D = kDotDepth<QT>;
  V r[D][E];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (FULL || s + d < nstrips) slice_load<V, E, VEC16>(r[d], row, ((i64)(s + d) * 64 + lane) * E, cols);
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (FULL || s + d < nstrips) {
      const i64 c = ((i64)(s + d) * 64 + lane) * E;
#pragma unroll
      for (int j = 0; j < QT; ++j) {
        V t[E];
        if (SELF) {
#pragma unroll
          for (int e = 0; e < E; ++e) t[e] = r[d][e];
        } else {
          x_load<V, E, XW>(t, xq[j], c, cols);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) acc[j] = dot_step(acc[j], r[d][e], t[e]);
      }
    }
  }
}

}  // namespace glint
