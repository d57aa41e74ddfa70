// glint_rowadam.hip -- Adam row push (glint_mat_push_rows_adam*, DESIGN.md "Adam row push"): lazy Adam
// next to the rows. The caller sends n gradient rows; per distinct row the shard sums them and steps the
// row of the weights shard and the row of the packed moments shard (m in columns [0, cols), v in
// [cols, 2 * cols)) with one read-modify-write each:
//   rows_front      the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                   rows_prepare, rs_sort, rows_runs<false> -- one item per distinct row;
//   rows_step_fold  one wave per (item, column slice): G = the run's gradient slices added to +0 in list
//                   order, then m' = b1 * m + a1 * G, v' = b2 * v + a2 * (G * G) and
//                   w' = w - (alpha * m') / (sqrt(v') / rc2 + eps).
// The step needs a row's whole sum, so no run is ever split and there is no atomic. Every operation is
// rounded on its own in the shard's type (include/glint_gpu.h has the contract); nothing of it depends
// on the alignment of grads, the slice path or the grid.
#include <cmath>

#include "glint_rowstep.h"

namespace glint {

// The step policy of the sliced fold (glint_rowstep.h): two state parts, m and v, and the seven scalars of
// the contract, settled on the host in double and rounded once to V.
// The fourteen operations of the contract, each rounded on its own: hipcc would contract b1 * m + a1 * G
// and b2 * v + a2 * q into v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). r / rc2 and u / d
// stay divisions -- a multiplication by a reciprocal rounds differently. sqrt and / are the compiler's
// IEEE ones (step_sqrt's note).
template <typename V>
struct AdamScalars {
  static constexpr int kParts = 2;
  V b1, b2, a1, a2, alpha, rc2, eps;
  __device__ __forceinline__ void step(V& w, V (&mv)[2], V G) const {
#pragma clang fp contract(off)
    const V m = mv[0], v = mv[1];
    const V t1 = b1 * m;
    const V t2 = a1 * G;
    const V m2 = t1 + t2;
    const V q = G * G;
    const V t3 = b2 * v;
    const V t4 = a2 * q;
    const V v2 = t3 + t4;
    const V r = step_sqrt(v2);
    const V s = r / rc2;
    const V d = s + eps;
    const V u = alpha * m2;
    const V p = u / d;
    const V w2 = w - p;
    mv[0] = m2;
    mv[1] = v2;
    w = w2;
  }
};

// `s` has w's type and partition and 2 * cols columns. The scalars are settled here, once, in double.
template <typename V>
int push_rows_adam(glint_shard* w, glint_shard* s, const i64* rows, const void* grads, i64 n, double lr, double beta1,
                   double beta2, double eps, i64 step, hipStream_t st) {
  if (n > 0 && step < 1) return GLINT_EINVAL;
  const double c1 = 1.0 - std::pow(beta1, (double)step), c2 = 1.0 - std::pow(beta2, (double)step);
  const AdamScalars<V> k = {(V)beta1,     (V)beta2,          (V)(1.0 - beta1), (V)(1.0 - beta2),
                            (V)(lr / c1), (V)std::sqrt(c2), (V)eps};  // each rounded once to V here
  return push_rows_step<V>(w, s, rows, grads, n, k, st);
}

template int push_rows_adam<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                   double, i64, hipStream_t);
template int push_rows_adam<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                    double, i64, hipStream_t);

}  // namespace glint
