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
// on the alignment of grads, the slice path or the grid.
#include "glint_rowstep.h"

namespace glint {

__device__ __forceinline__ double ftrl_abs(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float ftrl_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double ftrl_copysign(double m, double s) { return __builtin_copysign(m, s); }
__device__ __forceinline__ float ftrl_copysign(float m, float s) { return __builtin_copysignf(m, s); }

// The step policy of the sliced fold (glint_rowstep.h): two state parts, z and n, and the four scalars of
// the contract, each rounded once to V on the host.
// The operations of the contract, each rounded on its own: hipcc would contract G - sg * w and n + G * G
// into v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). ds / alpha, b / alpha and y / d stay
// divisions -- a multiplication by a reciprocal rounds differently -- and r1 - r0 is the difference of two
// square roots, not q / (r1 + r0). sqrt and / are the compiler's IEEE ones (step_sqrt's note).
// The threshold is a select: both sides are computed and `a <= l1`, false for a NaN z', picks +0 or -e, so a
// NaN reaches w' through y. The quotient of the side not taken (d may be 0 there) is dropped unseen.
template <typename V>
struct FtrlScalars {
  static constexpr int kParts = 2;
  V alpha, beta, l1, l2;
  __device__ __forceinline__ void step(V& w, V (&zn)[2], V G) const {
#pragma clang fp contract(off)
    const V z = zn[0], n = zn[1];
    const V q = G * G;
    const V n2 = n + q;
    const V r0 = step_sqrt(n);
    const V r1 = step_sqrt(n2);
    const V ds = r1 - r0;
    const V sg = ds / alpha;
    const V t = sg * w;
    const V u = G - t;
    const V z2 = z + u;
    const V a = ftrl_abs(z2);
    const V s = ftrl_copysign(l1, z2);
    const V y = z2 - s;
    const V b = beta + r1;
    const V c = b / alpha;
    const V d = c + l2;
    const V e = y / d;
    const V w2 = a <= l1 ? V(0) : -e;
    zn[0] = z2;
    zn[1] = n2;
    w = w2;
  }
};

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
