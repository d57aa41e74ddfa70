// glint_rowftrl.hip -- FTRL-proximal row push (glint_mat_push_rows_ftrl*, DESIGN.md "FTRL row push"):
// per-coordinate FTRL-proximal (McMahan et al., "Ad Click Prediction", 2013) next to the rows. The caller
// sends n gradient rows; per distinct row the shard sums them and steps the row of the weights shard and
// the row of the packed state shard (z in columns [0, cols), n in [cols, 2 * cols)) with one
// read-modify-write each:
//   rows_front      the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                   rows_prepare, rs_sort, rows_runs<false> -- one item per distinct row;
//   rows_step_fold  one wave per (item, column slice): G = the run's gradient slices added to +0 in list
//                   order, then n' = n + G * G, z' = z + (G - ((sqrt(n') - sqrt(n)) / alpha) * w) and
//                   w' = +0 where |z'| <= l1, else -(z' - copysign(l1, z')) / ((beta + sqrt(n')) / alpha + l2).
// The step needs a row's whole sum, so no run is ever split and there is no atomic. Every operation is
// rounded on its own in the shard's type (include/glint_gpu.h has the contract); nothing of it depends
// on the alignment of grads, the slice path or the grid. The step policy, FtrlScalars, is in glint_steps.h.
#include "glint_steps.h"

namespace glint {

// `s` has w's type and partition and 2 * cols columns. The scalars are rounded here, once, to V.
template <typename V>
int push_rows_ftrl(glint_shard* w, glint_shard* s, const i64* rows, const void* grads, i64 n, double alpha,
                   double beta, double l1, double l2, hipStream_t st) {
  return push_rows_step<V>(w, s, rows, grads, n, FtrlScalars<V>{(V)alpha, (V)beta, (V)l1, (V)l2}, st);
}

template int push_rows_ftrl<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                   double, hipStream_t);
template int push_rows_ftrl<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                    double, hipStream_t);

}  // namespace glint
