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
// on the alignment of grads, the slice path or the grid. The step policy, AdamScalars, and the settling of
// its scalars are in glint_steps.h.
#include "glint_steps.h"

namespace glint {

// `s` has w's type and partition and 2 * cols columns.
template <typename V>
int push_rows_adam(glint_shard* w, glint_shard* s, const i64* rows, const void* grads, i64 n, double lr, double beta1,
                   double beta2, double eps, i64 step, hipStream_t st) {
  if (n > 0 && step < 1) return GLINT_EINVAL;
  return push_rows_step<V>(w, s, rows, grads, n, adam_scalars<V>(lr, beta1, beta2, eps, step), st);
}

template int push_rows_adam<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                   double, i64, hipStream_t);
template int push_rows_adam<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                    double, i64, hipStream_t);

}  // namespace glint
