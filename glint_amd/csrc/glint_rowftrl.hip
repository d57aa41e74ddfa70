// glint_rowftrl.hip -- FTRL-proximal row push (glint_mat_push_rows_ftrl*, DESIGN.md "FTRL row push"):
// per-coordinate FTRL-proximal (McMahan et al., "Ad Click Prediction", 2013) next to the rows. The caller
// sends n gradient rows; per distinct row the shard sums them and steps the row of the weights shard and
// the row of the packed state shard (z in columns [0, cols), n in [cols, 2 * cols)) with one
// read-modify-write each:
//   rows_front      the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                   rows_prepare, rs_sort, rows_runs<false> -- one item per distinct row;
//   rows_ftrl_fold  one wave per (item, column slice): G = the run's gradient slices added to +0 in list
//                   order, then n' = n + G * G, z' = z + (G - ((sqrt(n') - sqrt(n)) / alpha) * w) and
//                   w' = +0 where |z'| <= l1, else -(z' - copysign(l1, z')) / ((beta + sqrt(n')) / alpha + l2).
// The step needs a row's whole sum, so no run is ever split and there is no atomic. Every operation is
// rounded on its own in the shard's type (include/glint_gpu.h has the contract); nothing of it depends
// on the alignment of grads, the slice path or the grid.
#include <cmath>

#include "glint_device.h"
#include "glint_host.h"

namespace glint {

constexpr int kFtrlDepth = 16;  // gradient loads in flight per wave (the Adam fold's depth)

// the four scalars of the contract, each rounded once to V on the host
template <typename V>
struct FtrlScalars {
  V alpha, beta, l1, l2;
};

__device__ __forceinline__ double ftrl_sqrt(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float ftrl_sqrt(float x) { return __builtin_sqrtf(x); }
__device__ __forceinline__ double ftrl_abs(double x) { return __builtin_fabs(x); }
__device__ __forceinline__ float ftrl_abs(float x) { return __builtin_fabsf(x); }
__device__ __forceinline__ double ftrl_copysign(double m, double s) { return __builtin_copysign(m, s); }
__device__ __forceinline__ float ftrl_copysign(float m, float s) { return __builtin_copysignf(m, s); }

// The operations of the contract, each rounded on its own: hipcc would contract G - sg * w and n + G * G
// into v_fma_* by default (adam_step's rule, glint_rowadam.hip). ds / alpha, b / alpha and y / d stay
// divisions -- a multiplication by a reciprocal rounds differently -- and r1 - r0 is the difference of two
// square roots, not q / (r1 + r0). sqrt and / are the compiler's IEEE ones (no fast-math flag in the build).
// The threshold is a select: both sides are computed and `a <= l1`, false for a NaN z', picks +0 or -e, so a
// NaN reaches w' through y. The quotient of the side not taken (d may be 0 there) is dropped unseen.
template <typename V>
__device__ __forceinline__ void ftrl_step(V& w, V& z, V& n, V G, const FtrlScalars<V>& k) {
#pragma clang fp contract(off)
  const V q = G * G;
  const V n2 = n + q;
  const V r0 = ftrl_sqrt(n);
  const V r1 = ftrl_sqrt(n2);
  const V ds = r1 - r0;
  const V sg = ds / k.alpha;
  const V t = sg * w;
  const V u = G - t;
  const V z2 = z + u;
  const V a = ftrl_abs(z2);
  const V s = ftrl_copysign(k.l1, z2);
  const V y = z2 - s;
  const V b = k.beta + r1;
  const V c = b / k.alpha;
  const V d = c + k.l2;
  const V e = y / d;
  const V w2 = a <= k.l1 ? V(0) : -e;
  z = z2;
  n = n2;
  w = w2;
}

// Records [start, start + len) of the sorted list: one slice of the weights row and of both halves of
// the state row stepped by the run's summed gradient slice. The three row loads are issued first and
// consumed last, behind the run; the sum is rows_adam_item's loop: 64 record ids per wave, kFtrlDepth
// loads in flight, adds strictly in list order. `nrow` is the state row's second half, zrow + cols.
template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void rows_ftrl_item(const u32* __restrict__ idx, u32 start, u32 len,
                                               const V* __restrict__ grads, V* wrow, V* zrow, V* nrow,
                                               const FtrlScalars<V>& k, i64 c, i64 cols, int lane) {
  V w[VPL], z[VPL], n[VPL], G[VPL];
  slice_load<V, VPL, WIDE>(w, wrow, c, cols);
  slice_load<V, VPL, WIDE>(z, zrow, c, cols);
  slice_load<V, VPL, WIDE>(n, nrow, c, cols);
#pragma unroll
  for (int e = 0; e < VPL; ++e) G[e] = V(0);
  for (u32 b = 0; b < len; b += 64) {
    const u32 nb = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < nb ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    for (u32 j = 0; j < nb; j += kFtrlDepth) {
      V t[kFtrlDepth][VPL];
      if (nb - j >= (u32)kFtrlDepth) {
#pragma unroll
        for (int d = 0; d < kFtrlDepth; ++d) {
          const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
          slice_load<V, VPL, WIDE>(t[d], grads + (i64)id * cols, c, cols);
        }
#pragma unroll
        for (int d = 0; d < kFtrlDepth; ++d)
#pragma unroll
          for (int e = 0; e < VPL; ++e) G[e] = vadd(G[e], t[d][e]);
      } else {  // the run's last few records (wave-uniform tests)
#pragma unroll
        for (int d = 0; d < kFtrlDepth; ++d) {
          if (j + d < nb) {
            const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
            slice_load<V, VPL, WIDE>(t[d], grads + (i64)id * cols, c, cols);
          }
        }
#pragma unroll
        for (int d = 0; d < kFtrlDepth; ++d) {
          if (j + d < nb) {
#pragma unroll
            for (int e = 0; e < VPL; ++e) G[e] = vadd(G[e], t[d][e]);
          }
        }
      }
    }
  }
#pragma unroll
  for (int e = 0; e < VPL; ++e) ftrl_step<V>(w[e], z[e], n[e], G[e], k);
  slice_store<V, VPL, WIDE>(z, zrow, c, cols);
  slice_store<V, VPL, WIDE>(n, nrow, c, cols);
  slice_store<V, VPL, WIDE>(w, wrow, c, cols);
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves
// (rows_adam_fold_kernel's frame). A slice is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple
// of 16 and grads 16-B aligned; both shards' pitch always is, so the n half at column `cols` of the
// state row is 16-B aligned too), else one element per lane. The state row is found with the state
// shard's pitch `spitch`, the weights row with part.pitch. Every item is a whole run: its row of either
// shard is read and written by this wave alone.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void rows_ftrl_fold_kernel(const u32* __restrict__ key, const u32* __restrict__ idx,
                                                              const uint2* __restrict__ items,
                                                              const u32* __restrict__ nitems,
                                                              const V* __restrict__ grads, V* wdata, V* sdata,
                                                              PartDesc part, i64 spitch, FtrlScalars<V> k) {
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
    V* zrow = sdata + row * spitch;
    rows_ftrl_item<V, VPL, VEC16>(idx, e.x, e.y, grads, wdata + row * part.pitch, zrow, zrow + cols, k,
                                  VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues an FTRL row push of n records on st (no host synchronisation): the front end's launches
// (scratch, error state and profile of `w`) and the one fold launch. Under both shards' locks; `s` has
// w's type and partition and 2 * cols columns. The scalars are rounded here, once, to V.
template <typename V>
int push_rows_ftrl(glint_shard* w, glint_shard* s, const i64* rows, const void* grads, i64 n, double alpha,
                   double beta, double l1, double l2, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !grads) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  if (s->part.cols != 2 * w->part.cols) return GLINT_EINVAL;
  RowsFront f;
  int rc = rows_front(w, rows, n, GLINT_PUSH_DETERMINISTIC, st, &f);
  if (rc) return rc;
  const FtrlScalars<V> k = {(V)alpha, (V)beta, (V)l1, (V)l2};
  const bool v16 = ((i64)w->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(grads, 16);
  const i64 slices = ((i64)w->part.cols * (i64)sizeof(V) + (v16 ? 1023 : 64 * (i64)sizeof(V) - 1)) /
                     (v16 ? 1024 : 64 * (i64)sizeof(V));
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)w->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const V*, V*, V*, PartDesc, i64, FtrlScalars<V>) =
      v16 ? rows_ftrl_fold_kernel<V, true> : rows_ftrl_fold_kernel<V, false>;
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const V*)grads,
                  (V*)w->data, (V*)s->data, w->part, (i64)s->part.pitch, k));
  return GLINT_OK;
}

template int push_rows_ftrl<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                   double, hipStream_t);
template int push_rows_ftrl<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double, double,
                                    double, hipStream_t);

}  // namespace glint
