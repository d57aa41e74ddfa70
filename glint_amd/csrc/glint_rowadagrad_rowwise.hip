// glint_rowadagrad_rowwise.hip -- row-wise Adagrad row push (glint_mat_push_rows_adagrad_rowwise*,
// DESIGN.md "Row-wise Adagrad row push"): the Adagrad row push with one accumulator per row, held in a
// vector shard, so that the optimizer state is 1 / cols of the table. Per distinct row the step needs the
// mean of the summed gradient's squares -- a reduction over the whole row between the sum and the update:
//   rows_front                 the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                              one item per distinct row;
//   rows_adagrad_rowwise_fold  one wave per item, two passes over the row in strips of 64 lanes x E
//                              columns, in the row dot pull's lane layout:
//                                pass 1  G = the run's gradient strips added to +0 in list order, each
//                                        lane adds G * G of its own columns in ascending order, the xor
//                                        butterfly gives ss; then the row scalars h' and k;
//                                pass 2  w' = w - k * G, with G kept in registers for rows of at most
//                                        GLINT_ROWWISE_KEEP_STRIPS strips and summed again (the same
//                                        loop, hence the same bits) for wider ones.
// One wave per row, not per (row, column slice): the slices of a row would need ss from each other. Every
// operation is rounded on its own in the shard's type (include/glint_gpu.h has the contract); nothing of it
// depends on the alignment of grads or the grid. No atomics, no LDS.
#include "glint_dot.h"  // dot_step, x_load: the row dot pull's arithmetic, word for word
#include "glint_rowstep.h"

namespace glint {

#ifndef GLINT_ROWWISE_KEEP_BUILD  // (a variant build for measurement sets 0: every row sums its run twice)
#define GLINT_ROWWISE_KEEP_BUILD GLINT_ROWWISE_KEEP_STRIPS
#endif
constexpr int kRowwiseKeep = GLINT_ROWWISE_KEEP_BUILD;  // strips kept in registers between the two passes

// The five row scalars of the contract, each rounded on its own; returns k and leaves h' in h. ss / C is
// a division, not a product with a reciprocal, and k = lr / d is one division per row. sqrt and / are the
// compiler's IEEE ones (step_sqrt's note, glint_rowstep.h).
template <typename V>
__device__ __forceinline__ V rowwise_scalars(V& h, V ss, V C, V lr, V eps) {
#pragma clang fp contract(off)
  const V s = ss / C;
  const V h2 = h + s;
  const V r = step_sqrt(h2);
  const V d = r + eps;
  const V k = lr / d;
  h = h2;
  return k;
}

// w' = w - (k * G), the product rounded before the subtraction: fma(-k, G, w) is not the contract's.
template <typename V>
__device__ __forceinline__ V rowwise_update(V w, V k, V G) {
#pragma clang fp contract(off)
  const V p = k * G;
  return w - p;
}

// Persistent grid; one wave per item. A strip is 64 lanes x E columns, lane L owning columns
// [(s * 64 + L) * E, +E) of strip s: E = 16 / sizeof(V) when VEC16 (cols * sizeof(V) a multiple of 16; the
// shard's pitch always is), else 1 -- the contract's layout whether or not grads is 16-B aligned (GW). Every
// item is a whole run: its row of weights and its element of state are read and written by this wave alone.
// KEEP > 0 (rows of at most KEEP strips): the summed strips stay in registers between the passes -- the
// strip loops are unrolled, so the array is indexed at compile time. KEEP == 0 (wider rows): pass 2 sums
// the run again with the same loop, hence the same bits; the second read of a short run comes from cache.
template <typename V, bool VEC16, bool GW, int KEEP>
__global__ __launch_bounds__(kTPB) void rows_adagrad_rowwise_fold_kernel(
    const u32* __restrict__ key, const u32* __restrict__ idx, const uint2* __restrict__ items,
    const u32* __restrict__ nitems, const V* __restrict__ grads, V* wdata, V* hdata, PartDesc part, V lr, V eps,
    V C) {
  constexpr int E = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the item, its run and the record indices are then wave-uniform to
  // the compiler too (rows_fold_kernel's pattern)
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
    if (KEEP > 0) {
#pragma unroll
      for (int s = 0; s < KEEP; ++s) {
        if ((u32)s < nstrips) {
#pragma unroll
          for (int k = 0; k < E; ++k) G[s][k] = V(0);
          run_sum<V, E, x_load<V, E, GW>>(G[s], idx, e.x, e.y, grads, ((i64)s * 64 + lane) * E, cols, lane);
#pragma unroll
          for (int k = 0; k < E; ++k) acc = dot_step(acc, G[s][k], G[s][k]);
        }
      }
    } else {
      for (u32 s = 0; s < nstrips; ++s) {
#pragma unroll
        for (int k = 0; k < E; ++k) G[0][k] = V(0);
        run_sum<V, E, x_load<V, E, GW>>(G[0], idx, e.x, e.y, grads, ((i64)s * 64 + lane) * E, cols, lane);
#pragma unroll
        for (int k = 0; k < E; ++k) acc = dot_step(acc, G[0][k], G[0][k]);
      }
    }
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
          for (int j = 0; j < E; ++j) w[j] = rowwise_update<V>(w[j], k, G[s][j]);
          slice_store<V, E, VEC16>(w, wrow, c, cols);
        }
      }
    } else {
      for (u32 s = 0; s < nstrips; ++s) {
        const i64 c = ((i64)s * 64 + lane) * E;
        V w[E];
        slice_load<V, E, VEC16>(w, wrow, c, cols);
#pragma unroll
        for (int j = 0; j < E; ++j) G[0][j] = V(0);
        run_sum<V, E, x_load<V, E, GW>>(G[0], idx, e.x, e.y, grads, c, cols, lane);
#pragma unroll
        for (int j = 0; j < E; ++j) w[j] = rowwise_update<V>(w[j], k, G[0][j]);
        slice_store<V, E, VEC16>(w, wrow, c, cols);
      }
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues a row-wise Adagrad row push of n records on st (no host synchronisation): the front end's
// launches (scratch, error state and profile of `w`) and the one fold launch. Under both shards' locks;
// `h` is a vector shard of w's type, size and partition.
template <typename V>
int push_rows_adagrad_rowwise(glint_shard* w, glint_shard* h, const i64* rows, const void* grads, i64 n, double lr,
                              double eps, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !grads) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  RowsFront f;
  int rc = rows_front(w, rows, n, GLINT_PUSH_DETERMINISTIC, st, &f);
  if (rc) return rc;
  const bool v16 = ((i64)w->part.cols * (i64)sizeof(V)) % 16 == 0;
  const bool gw = v16 && aligned(grads, 16);
  const i64 strip = 64 * (v16 ? (i64)(16 / sizeof(V)) : 1);
  const bool keep = ((i64)w->part.cols + strip - 1) / strip <= kRowwiseKeep;
  const unsigned gf = grid_for(n, kTPB / 64, (i64)w->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const V*, V*, V*, PartDesc, V, V, V);
  if (keep) {
    fold = !v16 ? rows_adagrad_rowwise_fold_kernel<V, false, false, kRowwiseKeep>
                : (gw ? rows_adagrad_rowwise_fold_kernel<V, true, true, kRowwiseKeep>
                      : rows_adagrad_rowwise_fold_kernel<V, true, false, kRowwiseKeep>);
  } else {
    fold = !v16 ? rows_adagrad_rowwise_fold_kernel<V, false, false, 0>
                : (gw ? rows_adagrad_rowwise_fold_kernel<V, true, true, 0>
                      : rows_adagrad_rowwise_fold_kernel<V, true, false, 0>);
  }
  // lr, eps and cols are rounded once to V here
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const V*)grads,
                  (V*)w->data, (V*)h->data, w->part, (V)lr, (V)eps, (V)w->part.cols));
  return GLINT_OK;
}

template int push_rows_adagrad_rowwise<float>(glint_shard*, glint_shard*, const i64*, const void*, i64, double, double,
                                              hipStream_t);
template int push_rows_adagrad_rowwise<double>(glint_shard*, glint_shard*, const i64*, const void*, i64, double,
                                               double, hipStream_t);

}  // namespace glint
