// glint_rowadagrad.hip -- Adagrad row push (glint_mat_push_rows_adagrad*, DESIGN.md "Adagrad row push"):
// a stateful optimizer step next to the rows. The caller sends n gradient rows; per distinct row the
// shard sums them and steps the row of the weights shard and the row of the accumulator shard with one
// read-modify-write each:
//   rows_front         the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                      rows_prepare, rs_sort, rows_runs<false> -- one item per distinct row;
//   rows_step_fold     one wave per (item, column slice): G = the run's gradient slices added to +0 in
//                      list order, then h' = h + G * G and w' = w - (lr * G) / (sqrt(h') + eps).
// The step needs a row's whole sum, so no run is ever split and there is no atomic. Every operation is
// rounded on its own in the shard's type (include/glint_gpu.h has the contract); nothing of it depends
// on the alignment of grads, the slice path or the grid.
#include "glint_rowstep.h"

namespace glint {

// The step policy of the sliced fold (glint_rowstep.h): one state part, h. lr and eps are rounded once to
// V on the host.
// The seven operations of the contract, each rounded on its own: hipcc would contract h + G * G into
// v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). u / d stays a division of the rounded lr * G
// -- G * (lr / d) rounds differently. sqrt and / are the compiler's IEEE ones (step_sqrt's note).
template <typename V>
struct AdagradScalars {
  static constexpr int kParts = 1;
  V lr, eps;
  __device__ __forceinline__ void step(V& w, V (&h)[1], V G) const {
#pragma clang fp contract(off)
    const V s = G * G;
    const V h2 = h[0] + s;
    const V r = step_sqrt(h2);
    const V d = r + eps;
    const V u = lr * G;
    const V p = u / d;
    const V w2 = w - p;
    h[0] = h2;
    w = w2;
  }
};

// `h` has w's type, partition, cols and pitch.
template <typename V>
int push_rows_adagrad(glint_shard* w, glint_shard* h, const i64* rows, const void* grads, i64 n, double lr, double eps,
                      hipStream_t st) {
  return push_rows_step<V>(w, h, rows, grads, n, AdagradScalars<V>{(V)lr, (V)eps}, st);
}

template int push_rows_adagrad<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double,
                                      hipStream_t);
template int push_rows_adagrad<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double,
                                       hipStream_t);

}  // namespace glint
