// glint_rowadam.hip -- Adam row push (glint_mat_push_rows_adam*, DESIGN.md "Adam row push"): lazy Adam
// next to the rows. The caller sends n gradient rows; per distinct row the shard sums them and steps the
// row of the weights shard and the row of the packed moments shard (m in columns [0, cols), v in
// [cols, 2 * cols)) with one read-modify-write each:
//   rows_front      the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                   rows_prepare, rs_sort, rows_runs<false> -- one item per distinct row;
//   rows_adam_fold  one wave per (item, column slice): G = the run's gradient slices added to +0 in list
//                   order, then m' = b1 * m + a1 * G, v' = b2 * v + a2 * (G * G) and
//                   w' = w - (alpha * m') / (sqrt(v') / rc2 + eps).
// The step needs a row's whole sum, so no run is ever split and there is no atomic. Every operation is
// rounded on its own in the shard's type (include/glint_gpu.h has the contract); nothing of it depends
// on the alignment of grads, the slice path or the grid.
#include <cmath>

#include "glint_device.h"
#include "glint_host.h"

namespace glint {

constexpr int kAdamDepth = 16;  // gradient loads in flight per wave (the Adagrad fold's depth)

// the seven scalars of the contract, settled on the host in double and rounded once to V
template <typename V>
struct AdamScalars {
  V b1, b2, a1, a2, alpha, rc2, eps;
};

// The fourteen operations of the contract, each rounded on its own: hipcc would contract b1 * m + a1 * G
// and b2 * v + a2 * q into v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). r / rc2 and u / d
// stay divisions -- a multiplication by a reciprocal rounds differently. sqrt and / are the compiler's
// IEEE ones (no fast-math flag in the build; for float hipcc's default correctly rounded divide and sqrt,
// f32 subnormals kept).
__device__ __forceinline__ double adam_sqrt(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float adam_sqrt(float x) { return __builtin_sqrtf(x); }

template <typename V>
__device__ __forceinline__ void adam_step(V& w, V& m, V& v, V G, const AdamScalars<V>& k) {
#pragma clang fp contract(off)
  const V t1 = k.b1 * m;
  const V t2 = k.a1 * G;
  const V m2 = t1 + t2;
  const V q = G * G;
  const V t3 = k.b2 * v;
  const V t4 = k.a2 * q;
  const V v2 = t3 + t4;
  const V r = adam_sqrt(v2);
  const V s = r / k.rc2;
  const V d = s + k.eps;
  const V u = k.alpha * m2;
  const V p = u / d;
  const V w2 = w - p;
  m = m2;
  v = v2;
  w = w2;
}

// Records [start, start + len) of the sorted list: one slice of the weights row and of both halves of
// the moments row stepped by the run's summed gradient slice. The three row loads are issued first and
// consumed last, behind the run; the sum is rows_adagrad_item's loop: 64 record ids per wave, kAdamDepth
// loads in flight, adds strictly in list order. `vrow` is the moments row's second half, mrow + cols.
template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void rows_adam_item(const u32* __restrict__ idx, u32 start, u32 len,
                                               const V* __restrict__ grads, V* wrow, V* mrow, V* vrow,
                                               const AdamScalars<V>& k, i64 c, i64 cols, int lane) {
  V w[VPL], m[VPL], v[VPL], G[VPL];
  slice_load<V, VPL, WIDE>(w, wrow, c, cols);
  slice_load<V, VPL, WIDE>(m, mrow, c, cols);
  slice_load<V, VPL, WIDE>(v, vrow, c, cols);
#pragma unroll
  for (int e = 0; e < VPL; ++e) G[e] = V(0);
  for (u32 b = 0; b < len; b += 64) {
    const u32 nb = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < nb ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    for (u32 j = 0; j < nb; j += kAdamDepth) {
      V t[kAdamDepth][VPL];
      if (nb - j >= (u32)kAdamDepth) {
#pragma unroll
        for (int d = 0; d < kAdamDepth; ++d) {
          const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
          slice_load<V, VPL, WIDE>(t[d], grads + (i64)id * cols, c, cols);
        }
#pragma unroll
        for (int d = 0; d < kAdamDepth; ++d)
#pragma unroll
          for (int e = 0; e < VPL; ++e) G[e] = vadd(G[e], t[d][e]);
      } else {  // the run's last few records (wave-uniform tests)
#pragma unroll
        for (int d = 0; d < kAdamDepth; ++d) {
          if (j + d < nb) {
            const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
            slice_load<V, VPL, WIDE>(t[d], grads + (i64)id * cols, c, cols);
          }
        }
#pragma unroll
        for (int d = 0; d < kAdamDepth; ++d) {
          if (j + d < nb) {
#pragma unroll
            for (int e = 0; e < VPL; ++e) G[e] = vadd(G[e], t[d][e]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < VPL; ++e) adam_step<V>(w[e], m[e], v[e], G[e], k);
  slice_store<V, VPL, WIDE>(m, mrow, c, cols);
  slice_store<V, VPL, WIDE>(v, vrow, c, cols);
  slice_store<V, VPL, WIDE>(w, wrow, c, cols);
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves
// (rows_adagrad_fold_kernel's frame). A slice is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple
// of 16 and grads 16-B aligned; both shards' pitch always is, so the v half at column `cols` of the
// moments row is 16-B aligned too), else one element per lane. The moments row is found with the moments
// shard's pitch `spitch`, the weights row with part.pitch. Every item is a whole run: its row of either
// shard is read and written by this wave alone.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void rows_adam_fold_kernel(const u32* __restrict__ key, const u32* __restrict__ idx,
                                                              const uint2* __restrict__ items,
                                                              const u32* __restrict__ nitems,
                                                              const V* __restrict__ grads, V* wdata, V* sdata,
                                                              PartDesc part, i64 spitch, AdamScalars<V> k) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the item, its run and the record indices are then wave-uniform to
  // the compiler too (rows_fold_kernel's pattern)
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const u32 nslices = (u32)((cols + 64 * VPL - 1) / (64 * VPL));
  const u64 total = (u64)*nitems * nslices;
  for (u64 w = w0; w < total; w += nw) {
    const u32 it = (u32)(w / nslices), slice = (u32)(w % nslices);
    const uint2 e = items[it];
    const i64 row = (i64)key[e.x];
    const i64 c0 = (i64)slice * 64 * VPL;
    V* mrow = sdata + row * spitch;
    rows_adam_item<V, VPL, VEC16>(idx, e.x, e.y, grads, wdata + row * part.pitch, mrow, mrow + cols, k,
                                  VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues an Adam row push of n records on st (no host synchronisation): the front end's launches
// (scratch, error state and profile of `w`) and the one fold launch. Under both shards' locks; `s` has
// w's type and partition and 2 * cols columns. The scalars are settled here, once, in double.
template <typename V>
int push_rows_adam(glint_shard* w, glint_shard* s, const i64* rows, const void* grads, i64 n, double lr, double beta1,
                   double beta2, double eps, i64 step, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !grads) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  if (s->part.cols != 2 * w->part.cols || step < 1) return GLINT_EINVAL;
  RowsFront f;
  int rc = rows_front(w, rows, n, GLINT_PUSH_DETERMINISTIC, st, &f);
  if (rc) return rc;
  const double c1 = 1.0 - std::pow(beta1, (double)step), c2 = 1.0 - std::pow(beta2, (double)step);
  const AdamScalars<V> k = {(V)beta1,     (V)beta2,          (V)(1.0 - beta1), (V)(1.0 - beta2),
                            (V)(lr / c1), (V)std::sqrt(c2), (V)eps};  // each rounded once to V here
  const bool v16 = ((i64)w->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(grads, 16);
  const i64 slices = ((i64)w->part.cols * (i64)sizeof(V) + (v16 ? 1023 : 64 * (i64)sizeof(V) - 1)) /
                     (v16 ? 1024 : 64 * (i64)sizeof(V));
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)w->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const V*, V*, V*, PartDesc, i64, AdamScalars<V>) =
      v16 ? rows_adam_fold_kernel<V, true> : rows_adam_fold_kernel<V, false>;
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const V*)grads,
                  (V*)w->data, (V*)s->data, w->part, (i64)s->part.pitch, k));
  return GLINT_OK;
}

template int push_rows_adam<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                   double, i64, hipStream_t);
template int push_rows_adam<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                    double, i64, hipStream_t);

}  // namespace glint
