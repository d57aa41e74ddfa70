// glint_rowadagrad.hip -- Adagrad row push (glint_mat_push_rows_adagrad*, DESIGN.md "Adagrad row push"):
// a stateful optimizer step next to the rows. The caller sends n gradient rows; per distinct row the
// shard sums them and steps the row of the weights shard and the row of the accumulator shard with one
// read-modify-write each:
//   rows_front         the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                      rows_prepare, rs_sort, rows_runs<false> -- one item per distinct row;
//   rows_adagrad_fold  one wave per (item, column slice): G = the run's gradient slices added to +0 in
//                      list order, then h' = h + G * G and w' = w - (lr * G) / (sqrt(h') + eps).
// The step needs a row's whole sum, so no run is ever split and there is no atomic. Every operation is
// rounded on its own in the shard's type (include/glint_gpu.h has the contract); nothing of it depends
// on the alignment of grads, the slice path or the grid.
#include "glint_device.h"
#include "glint_host.h"

namespace glint {

constexpr int kAdagradDepth = 16;  // gradient loads in flight per wave (twice rows_fold_item's kRowsDepth)

// The seven operations of the contract, each rounded on its own: hipcc would contract h + G * G into
// v_fma_* by default (axpy_mul's rule, glint_rowaxpy.hip). u / d stays a division of the rounded lr * G
// -- G * (lr / d) rounds differently. sqrt and / are the compiler's IEEE ones (no fast-math flag in the
// build; for float hipcc's default correctly rounded divide and sqrt, f32 subnormals kept).
__device__ __forceinline__ double adagrad_sqrt(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float adagrad_sqrt(float x) { return __builtin_sqrtf(x); }

template <typename V>
__device__ __forceinline__ void adagrad_step(V& w, V& h, V G, V lr, V eps) {
#pragma clang fp contract(off)
  const V s = G * G;
  const V h2 = h + s;
  const V r = adagrad_sqrt(h2);
  const V d = r + eps;
  const V u = lr * G;
  const V p = u / d;
  const V w2 = w - p;
  h = h2;
  w = w2;
}

// Records [start, start + len) of the sorted list: one slice of the weights row and of the accumulator
// row stepped by the run's summed gradient slice. The two row loads are issued first and consumed last,
// behind the run; the sum is rows_fold_item's loop from a zero row: 64 record ids per wave, kAdagradDepth
// loads in flight, adds strictly in list order.
template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void rows_adagrad_item(const u32* __restrict__ idx, u32 start, u32 len,
                                                  const V* __restrict__ grads, V* wrow, V* hrow, V lr, V eps, i64 c,
                                                  i64 cols, int lane) {
  V w[VPL], h[VPL], G[VPL];
  slice_load<V, VPL, WIDE>(w, wrow, c, cols);
  slice_load<V, VPL, WIDE>(h, hrow, c, cols);
#pragma unroll
  for (int k = 0; k < VPL; ++k) G[k] = V(0);
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < m ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    for (u32 j = 0; j < m; j += kAdagradDepth) {
      V t[kAdagradDepth][VPL];
      if (m - j >= (u32)kAdagradDepth) {
#pragma unroll
        for (int d = 0; d < kAdagradDepth; ++d) {
          const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
          slice_load<V, VPL, WIDE>(t[d], grads + (i64)id * cols, c, cols);
        }
#pragma unroll
        for (int d = 0; d < kAdagradDepth; ++d)
#pragma unroll
          for (int k = 0; k < VPL; ++k) G[k] = vadd(G[k], t[d][k]);
      } else {  // the run's last few records (wave-uniform tests)
#pragma unroll
        for (int d = 0; d < kAdagradDepth; ++d) {
          if (j + d < m) {
            const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
            slice_load<V, VPL, WIDE>(t[d], grads + (i64)id * cols, c, cols);
          }
        }
#pragma unroll
        for (int d = 0; d < kAdagradDepth; ++d) {
          if (j + d < m) {
#pragma unroll
            for (int k = 0; k < VPL; ++k) G[k] = vadd(G[k], t[d][k]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int k = 0; k < VPL; ++k) adagrad_step<V>(w[k], h[k], G[k], lr, eps);
  slice_store<V, VPL, WIDE>(h, hrow, c, cols);
  slice_store<V, VPL, WIDE>(w, wrow, c, cols);
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves
// (rows_fold_kernel's frame). A slice is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple of 16
// and grads 16-B aligned; both shards' pitch always is), else one element per lane. Every item is a whole
// run: its row of either shard is read and written by this wave alone.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void rows_adagrad_fold_kernel(const u32* __restrict__ key,
                                                                 const u32* __restrict__ idx,
                                                                 const uint2* __restrict__ items,
                                                                 const u32* __restrict__ nitems,
                                                                 const V* __restrict__ grads, V* wdata, V* hdata,
                                                                 PartDesc part, V lr, V eps) {
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
    const i64 off = (i64)key[e.x] * part.pitch;
    const i64 c0 = (i64)slice * 64 * VPL;
    rows_adagrad_item<V, VPL, VEC16>(idx, e.x, e.y, grads, wdata + off, hdata + off, lr, eps,
                                     VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues an Adagrad row push of n records on st (no host synchronisation): the front end's launches
// (scratch, error state and profile of `w`) and the one fold launch. Under both shards' locks; `h` has
// w's type, partition, cols and pitch.
template <typename V>
int push_rows_adagrad(glint_shard* w, glint_shard* h, const i64* rows, const void* grads, i64 n, double lr, double eps,
                      hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !grads) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  RowsFront f;
  int rc = rows_front(w, rows, n, GLINT_PUSH_DETERMINISTIC, st, &f);
  if (rc) return rc;
  const bool v16 = ((i64)w->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(grads, 16);
  const i64 slices = ((i64)w->part.cols * (i64)sizeof(V) + (v16 ? 1023 : 64 * (i64)sizeof(V) - 1)) /
                     (v16 ? 1024 : 64 * (i64)sizeof(V));
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)w->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const V*, V*, V*, PartDesc, V, V) =
      v16 ? rows_adagrad_fold_kernel<V, true> : rows_adagrad_fold_kernel<V, false>;
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const V*)grads,
                  (V*)w->data, (V*)h->data, w->part, (V)lr, (V)eps));  // lr and eps rounded once to V here
  return GLINT_OK;
}

template int push_rows_adagrad<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double,
                                      hipStream_t);
template int push_rows_adagrad<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double,
                                       hipStream_t);

}  // namespace glint
