// glint_rowstep_group.h -- the device half of the grouped optimizer row pushes (glint_rowstep_group.hip,
// DESIGN.md "Grouped optimizer row pushes"): the bag backward fused with the optimizer's step. A record
// names a row and, through its group, one of g value rows; its contribution is that value row, optionally
// times the record's own coefficient. Per distinct row the contributions are summed to +0 in list order and
// the optimizer takes its one step -- the optimizer push of the n expanded rows, bit for bit, without
// anything of size n x cols:
//   run_sum_group                  run_sum (glint_rowstep.h) over (group id, coefficient) pairs: the sum of
//                                  one run into a lane's values, over any loader, and whether any record
//                                  contributed;
//   rows_step_group_fold           rows_step_fold_kernel's frame over it: Adagrad, Adam, FTRL;
//   rows_rowwise_group_fold        rows_adagrad_rowwise_fold_kernel's frame over it.
// The group ids are rows_group_ids_kernel's (glint_rowgroup.hip), one u32 per record. A row none of whose
// records contributed (a malformed device grp_ptr only) is not stepped: a zero-gradient step is not a no-op
// for any of the four optimizers. No atomics, no LDS.
#pragma once
#include "glint_axpy.h"  // axpy_mul, axpy_add, lane_get: the grouped row push's contribution, word for word
#include "glint_dot.h"   // dot_step, x_load: the row dot pull's arithmetic
#include "glint_steps.h"

namespace glint {

// record i -> its group, 0xFFFFFFFF (-1 as the folds read it) when no group covers it (glint_rowgroup.hip)
__global__ __launch_bounds__(kTPB) void rows_group_ids_kernel(const i64* __restrict__ grp_ptr, i64 g, i64 n,
                                                              u32* __restrict__ gids);

// Records [j, j + kRowStepDepth) of a batch of m <= 64 whose groups (-1: none) and coefficients the lanes
// hold (FULL: all of them exist; else the batch's last few, behind wave-uniform tests): the value-row loads
// are issued, v_readlane handing the group ids round, then consumed in list order -- with COEF the product
// rounded before the add, without it the stored bits and no multiply. CHECK: some record of the batch has
// no group; it is skipped by a wave-uniform branch, no load and no add.
template <typename V, int VPL, bool COEF, bool CHECK, bool FULL, void (*Load)(V (&)[VPL], const V*, i64, i64)>
__device__ __forceinline__ void group_sum_span(V (&G)[VPL], bool& any, int32_t gid, V cf, u32 j, u32 m,
                                               const V* __restrict__ vals, i64 c, i64 cols) {
  constexpr int D = kRowStepDepth;
  V t[D][VPL];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (FULL || j + d < m) {
      const int32_t k = __builtin_amdgcn_readlane(gid, (int)(j + d));
      if (!CHECK || k >= 0) Load(t[d], vals + (i64)k * cols, c, cols);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if ((FULL || j + d < m) && (!CHECK || __builtin_amdgcn_readlane(gid, (int)(j + d)) >= 0)) {
      if (COEF) {
        const V cd = lane_get(cf, j + d);
#pragma unroll
        for (int q = 0; q < VPL; ++q) G[q] = axpy_add(G[q], axpy_mul(cd, t[d][q]));
      } else {
#pragma unroll
        for (int q = 0; q < VPL; ++q) G[q] = vadd(G[q], t[d][q]);
      }
      any = true;
    }
  }
}

template <typename V, int VPL, bool COEF, bool CHECK, void (*Load)(V (&)[VPL], const V*, i64, i64)>
__device__ __forceinline__ void group_sum_batch(V (&G)[VPL], bool& any, int32_t gid, V cf, u32 m,
                                                const V* __restrict__ vals, i64 c, i64 cols) {
  for (u32 j = 0; j < m; j += kRowStepDepth) {
    if (m - j >= (u32)kRowStepDepth)
      group_sum_span<V, VPL, COEF, CHECK, true, Load>(G, any, gid, cf, j, m, vals, c, cols);
    else
      group_sum_span<V, VPL, COEF, CHECK, false, Load>(G, any, gid, cf, j, m, vals, c, cols);
  }
}

// G += a lane's VPL values at column c of the contributions of records [start, start + len) of the sorted
// list, one after the other in list order (run_sum's frame, glint_rowstep.h): the wave takes 64 records at
// a time, every lane loading its own record's index, its group id and, with COEF, its coefficient;
// kRowStepDepth loads of vals + gid * cols stay in flight, the adds the only chain. Load(t, row, c, cols)
// fetches one value row's values: slice_load for row slices, x_load for the row dot pull's strips. A batch
// that holds a record no group covers takes the checked loop behind one wave-uniform ballot
// (rows_group_item's routes, glint_rowgroup.hip). The caller zeroes G. Returns, wave-uniformly, whether any
// record contributed.
template <typename V, int VPL, bool COEF, void (*Load)(V (&)[VPL], const V*, i64, i64)>
__device__ __forceinline__ bool run_sum_group(V (&G)[VPL], const u32* __restrict__ idx, u32 start, u32 len,
                                              const u32* __restrict__ gids, const V* __restrict__ vals,
                                              const V* __restrict__ coef, i64 c, i64 cols, int lane) {
  bool any = false;
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    int32_t gid = -1;  // this lane's record: its group, or -1 when it has none
    V cf = V(0);
    bool none = false;
    if ((u32)lane < m) {
      const u32 mine = idx[(i64)start + b + lane];  // 64 record indices, one per lane
      gid = (int32_t)gids[mine];
      if (COEF) cf = coef[mine];
      none = gid < 0;
    }
    if (__ballot(none) == 0) group_sum_batch<V, VPL, COEF, false, Load>(G, any, gid, cf, m, vals, c, cols);
    else group_sum_batch<V, VPL, COEF, true, Load>(G, any, gid, cf, m, vals, c, cols);
  }
  return any;
}

// rows_step_fold_kernel's frame (glint_rowstep.h) over the grouped run-sum: persistent grid; one wave per
// (item, column slice), the slices of an item on adjacent waves. A slice is 64 lanes x 16 B when VEC16
// (cols * sizeof(V) a multiple of 16 and vals 16-B aligned, so every value row is; both shards' pitch
// always is), else one element per lane. The slices of the weights row and of every part of the state row
// are loaded before the run and consumed after it; the parts are stored in ascending order, then the
// weights. Every item is a whole run: its row of either shard is read and written by this wave alone. A row
// none of whose records contributed is not stepped and not stored.
template <typename V, bool VEC16, bool COEF, typename Step>
__global__ __launch_bounds__(kTPB) void rows_step_group_fold_kernel(
    const u32* __restrict__ key, const u32* __restrict__ idx, const uint2* __restrict__ items,
    const u32* __restrict__ nitems, const u32* __restrict__ gids, const V* __restrict__ vals,
    const V* __restrict__ coef, V* wdata, V* sdata, PartDesc part, i64 spitch, Step k) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  constexpr int P = Step::kParts;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the item, its run and the group ids handed round are then wave-uniform
  // to the compiler too (rows_fold_kernel's pattern)
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const u32 nslices = (u32)((cols + 64 * VPL - 1) / (64 * VPL));
  const u64 total = (u64)*nitems * nslices;
  for (u64 wv = w0; wv < total; wv += nw) {
    const u32 it = (u32)(wv / nslices), slice = (u32)(wv % nslices);
    const uint2 e = items[it];
    const i64 row = (i64)key[e.x];
    const i64 c0 = (i64)slice * 64 * VPL;
    const i64 c = VEC16 ? c0 + (i64)lane * VPL : c0 + lane;
    V* wrow = wdata + row * part.pitch;
    V* srow = sdata + row * spitch;
    V w[VPL], s[P][VPL], G[VPL];
    slice_load<V, VPL, VEC16>(w, wrow, c, cols);
#pragma unroll
    for (int p = 0; p < P; ++p) slice_load<V, VPL, VEC16>(s[p], srow + p * cols, c, cols);
#pragma unroll
    for (int q = 0; q < VPL; ++q) G[q] = V(0);
    if (!run_sum_group<V, VPL, COEF, slice_load<V, VPL, VEC16>>(G, idx, e.x, e.y, gids, vals, coef, c, cols, lane))
      continue;
#pragma unroll
    for (int q = 0; q < VPL; ++q) {
      V se[P];
#pragma unroll
      for (int p = 0; p < P; ++p) se[p] = s[p][q];
      k.step(w[q], se, G[q]);
#pragma unroll
      for (int p = 0; p < P; ++p) s[p][q] = se[p];
    }
#pragma unroll
    for (int p = 0; p < P; ++p) slice_store<V, VPL, VEC16>(s[p], srow + p * cols, c, cols);
    slice_store<V, VPL, VEC16>(w, wrow, c, cols);
  }
}

// rows_adagrad_rowwise_fold_kernel's frame (glint_rowadagrad_rowwise.hip) over the grouped run-sum:
// persistent grid; one wave per item. A strip is 64 lanes x E columns, lane L owning columns
// [(s * 64 + L) * E, +E) of strip s: E = 16 / sizeof(V) when VEC16 (cols * sizeof(V) a multiple of 16), else
// 1 -- the contract's layout whether or not vals is 16-B aligned (GW). Pass 1 sums the run's strips and the
// lane sums of G * G in ascending column order, the xor butterfly gives ss, rowwise_scalars h' and k; pass 2
// updates from the strips kept in registers (KEEP > 0: rows of at most KEEP strips, the strip loops
// unrolled) or from a second, identical run-sum (KEEP == 0: wider rows; the value rows come from cache).
// Whether a record contributes does not depend on the strip, so every strip's run-sum reports the same; a
// row none of whose records contributed is not stepped: neither its accumulator nor its weights are stored.
template <typename V, bool VEC16, bool GW, int KEEP, bool COEF>
__global__ __launch_bounds__(kTPB) void rows_rowwise_group_fold_kernel(
    const u32* __restrict__ key, const u32* __restrict__ idx, const uint2* __restrict__ items,
    const u32* __restrict__ nitems, const u32* __restrict__ gids, const V* __restrict__ vals,
    const V* __restrict__ coef, V* wdata, V* hdata, PartDesc part, V lr, V eps, V C) {
  constexpr int E = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const u32 nstrips = (u32)((cols + 64 * E - 1) / (64 * E));
  const u64 total = *nitems;
  for (u64 it = w0; it < total; it += nw) {
    const uint2 e = items[it];
    const i64 l = (i64)key[e.x];
    V* wrow = wdata + l * part.pitch;
    V G[KEEP > 0 ? KEEP : 1][E];
    // pass 1: the lane sums of G * G in ascending strip -- hence column -- order, from +0
    V acc = V(0);
    bool any = false;
    if (KEEP > 0) {
#pragma unroll
      for (int s = 0; s < KEEP; ++s) {
        if ((u32)s < nstrips) {
#pragma unroll
          for (int q = 0; q < E; ++q) G[s][q] = V(0);
          any = run_sum_group<V, E, COEF, x_load<V, E, GW>>(G[s], idx, e.x, e.y, gids, vals, coef,
                                                            ((i64)s * 64 + lane) * E, cols, lane);
#pragma unroll
          for (int q = 0; q < E; ++q) acc = dot_step(acc, G[s][q], G[s][q]);
        }
      }
    } else {
      for (u32 s = 0; s < nstrips; ++s) {
#pragma unroll
        for (int q = 0; q < E; ++q) G[0][q] = V(0);
        any = run_sum_group<V, E, COEF, x_load<V, E, GW>>(G[0], idx, e.x, e.y, gids, vals, coef,
                                                          ((i64)s * 64 + lane) * E, cols, lane);
#pragma unroll
        for (int q = 0; q < E; ++q) acc = dot_step(acc, G[0][q], G[0][q]);
      }
    }
    if (!any) continue;
    // the xor butterfly: IEEE addition commutes, so every lane ends with the same bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc = vadd(acc, __shfl_xor(acc, d, 64));
    V h = hdata[l];  // every lane reads it; lane 0 stores h'
    const V k = rowwise_scalars<V>(h, acc, C, lr, eps);
    if (lane == 0) hdata[l] = h;
    // pass 2
    if (KEEP > 0) {
#pragma unroll
      for (int s = 0; s < KEEP; ++s) {
        if ((u32)s < nstrips) {
          const i64 c = ((i64)s * 64 + lane) * E;
          V w[E];
          slice_load<V, E, VEC16>(w, wrow, c, cols);
#pragma unroll
          for (int q = 0; q < E; ++q) w[q] = rowwise_update<V>(w[q], k, G[s][q]);
          slice_store<V, E, VEC16>(w, wrow, c, cols);
        }
      }
    } else {
      for (u32 s = 0; s < nstrips; ++s) {
        const i64 c = ((i64)s * 64 + lane) * E;
        V w[E];
        slice_load<V, E, VEC16>(w, wrow, c, cols);
#pragma unroll
        for (int q = 0; q < E; ++q) G[0][q] = V(0);
        (void)run_sum_group<V, E, COEF, x_load<V, E, GW>>(G[0], idx, e.x, e.y, gids, vals, coef, c, cols, lane);
#pragma unroll
        for (int q = 0; q < E; ++q) w[q] = rowwise_update<V>(w[q], k, G[0][q]);
        slice_store<V, E, VEC16>(w, wrow, c, cols);
      }
    }
  }
}

}  // namespace glint
