// glint_rowstep.h -- what the optimizer row pushes share (DESIGN.md "The optimizer pushes' shared run-sum
// and fold frame"): Adagrad (glint_rowadagrad.hip), Adam (glint_rowadam.hip), FTRL-proximal
// (glint_rowftrl.hip) and row-wise Adagrad (glint_rowadagrad_rowwise.hip). Each sums a row's gradients
// to +0 in list order -- always strict, never a split run, never an atomic -- and then takes its step:
//   run_sum          the sum of one run into a lane's values, over any loader;
//   rows_step_fold   one wave per (item, column slice) over a step policy: the three sliced pushes;
//   push_rows_step   their host half.
// The additive folds (rows, wire, axpy, group, pairs) split runs and use atomics; they keep their own loops.
#pragma once
#include "glint_device.h"
#include "glint_host.h"

namespace glint {

// gradient loads in flight per wave, twice rows_fold_item's kRowsDepth: profiles/adagrad/README.md has
// the measurement that chose it
constexpr int kRowStepDepth = 16;

// the compiler's IEEE square root (no fast-math flag in the build; for float hipcc's default correctly
// rounded one, f32 subnormals kept)
__device__ __forceinline__ double step_sqrt(double x) { return __builtin_sqrt(x); }
__device__ __forceinline__ float step_sqrt(float x) { return __builtin_sqrtf(x); }

// G += a lane's VPL values at column c of records [start, start + len) of the sorted list, one after the
// other in list order: 64 record ids per wave handed round by readlane, kRowStepDepth loads in flight,
// the adds the only chain. Load(t, row, c, cols) fetches one record's values: slice_load for row slices,
// x_load for the row dot pull's strips. The caller zeroes G:
// with the zeroing in here the 16-B float folds take ~160 VGPRs instead of ~105, a wave per SIMD less.
template <typename V, int VPL, void (*Load)(V (&)[VPL], const V*, i64, i64)>
__device__ __forceinline__ void run_sum(V (&G)[VPL], const u32* __restrict__ idx, u32 start, u32 len,
                                        const V* __restrict__ grads, i64 c, i64 cols, int lane) {
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < m ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    for (u32 j = 0; j < m; j += kRowStepDepth) {
      V t[kRowStepDepth][VPL];
      if (m - j >= (u32)kRowStepDepth) {
#pragma unroll
        for (int d = 0; d < kRowStepDepth; ++d) {
          const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
          Load(t[d], grads + (i64)id * cols, c, cols);
        }
#pragma unroll
        for (int d = 0; d < kRowStepDepth; ++d)
#pragma unroll
          for (int k = 0; k < VPL; ++k) G[k] = vadd(G[k], t[d][k]);
      } else {  // the run's last few records (wave-uniform tests)
#pragma unroll
        for (int d = 0; d < kRowStepDepth; ++d) {
          if (j + d < m) {
            const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
            Load(t[d], grads + (i64)id * cols, c, cols);
          }
        }
#pragma unroll
        for (int d = 0; d < kRowStepDepth; ++d) {
          if (j + d < m) {
#pragma unroll
            for (int k = 0; k < VPL; ++k) G[k] = vadd(G[k], t[d][k]);
          }
        }
      }
    }
  }
}

// A step policy `Step` of the sliced fold is a struct of the step's scalars, each rounded once to V on the
// host, carried by value in the kernel arguments, with
//   Step::kParts                       a row's state parts: part p is columns [p * cols, +cols) of the state row;
//   k.step(V& w, V (&s)[kParts], V G)  one element's step, every operation rounded on its own.
//
// Records [start, start + len) of the sorted list: one slice of the weights row and of every part of the
// state row stepped by the run's summed gradient slice. The row loads are issued first and consumed last,
// behind the run; the parts are stored in ascending order, then the weights.
template <typename V, int VPL, bool WIDE, typename Step>
__device__ __forceinline__ void rows_step_item(const u32* __restrict__ idx, u32 start, u32 len,
                                               const V* __restrict__ grads, V* wrow, V* srow, const Step& k, i64 c,
                                               i64 cols, int lane) {
  constexpr int P = Step::kParts;
  V w[VPL], s[P][VPL], G[VPL];
  slice_load<V, VPL, WIDE>(w, wrow, c, cols);
#pragma unroll
  for (int p = 0; p < P; ++p) slice_load<V, VPL, WIDE>(s[p], srow + p * cols, c, cols);
#pragma unroll
  for (int e = 0; e < VPL; ++e) G[e] = V(0);
  run_sum<V, VPL, slice_load<V, VPL, WIDE>>(G, idx, start, len, grads, c, cols, lane);
#pragma unroll
  for (int e = 0; e < VPL; ++e) {
    V se[P];
#pragma unroll
    for (int p = 0; p < P; ++p) se[p] = s[p][e];
    k.step(w[e], se, G[e]);
#pragma unroll
    for (int p = 0; p < P; ++p) s[p][e] = se[p];
  }
#pragma unroll
  for (int p = 0; p < P; ++p) slice_store<V, VPL, WIDE>(s[p], srow + p * cols, c, cols);
  slice_store<V, VPL, WIDE>(w, wrow, c, cols);
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves
// (rows_fold_kernel's frame). A slice is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple of 16
// and grads 16-B aligned; both shards' pitch always is, so a state part at column p * cols is 16-B
// aligned too), else one element per lane. The state row is found with the state shard's pitch `spitch`,
// the weights row with part.pitch. Every item is a whole run: its row of either shard is read and written
// by this wave alone.
template <typename V, bool VEC16, typename Step>
__global__ __launch_bounds__(kTPB) void rows_step_fold_kernel(
    const u32* __restrict__ key, const u32* __restrict__ idx, const uint2* __restrict__ items,
    const u32* __restrict__ nitems, const V* __restrict__ grads, V* wdata, V* sdata, PartDesc part, i64 spitch,
    Step k) {
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
    rows_step_item<V, VPL, VEC16, Step>(idx, e.x, e.y, grads, wdata + row * part.pitch, sdata + row * spitch, k,
                                        VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues a sliced optimizer row push of n records on st (no host synchronisation): the row push's front
// end unchanged, always strict (GLINT_PUSH_DETERMINISTIC; scratch, error state and profile of `w`) -- one
// item per distinct row -- and the one fold launch. Under both shards' locks; `s` has w's type and
// partition and Step::kParts * cols columns.
template <typename V, typename Step>
int push_rows_step(glint_shard* w, glint_shard* s, const i64* rows, const void* grads, i64 n, const Step& k,
                   hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !grads) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  if (s->part.cols != Step::kParts * w->part.cols) return GLINT_EINVAL;
  RowsFront f;
  int rc = rows_front(w, rows, n, GLINT_PUSH_DETERMINISTIC, st, &f);
  if (rc) return rc;
  const bool v16 = ((i64)w->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(grads, 16);
  const unsigned gf = grid_for(n * row_slices<V>(w->part.cols, v16), kTPB / 64, (i64)w->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const V*, V*, V*, PartDesc, i64, Step) =
      v16 ? rows_step_fold_kernel<V, true, Step> : rows_step_fold_kernel<V, false, Step>;
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const V*)grads,
                  (V*)w->data, (V*)s->data, w->part, (i64)s->part.pitch, k));
  return GLINT_OK;
}

}  // namespace glint
