// glint_rowaxpy.hip -- row axpy push (glint_mat_push_rows_axpy*, DESIGN.md "Row axpy push"): the write
// half of a scoring step, row rows[i] += sum over j of coef[i][j] * x[j]. It is the row push
// (glint_rows.hip) with the contribution rows rebuilt by the wave that folds them, from q slices of x
// and the record's q coefficients, instead of read from an n x cols array:
//   rows_front      the row push's front end unchanged: rows_prepare, rs_sort, rows_runs;
//   rows_axpy_fold  one wave per (item, column slice): shard slice + the run's contributions t_i,
//                   strictly in list order, t_i = ((coef[i][0] * x[0]) + (coef[i][1] * x[1])) + ...
// The floating-point order is the contract (include/glint_gpu.h): every product is rounded before it is
// added, j ascends, the records of a row keep the list order; nothing of it depends on the alignment of
// x or coef, on q's tiling over registers or on the grid. Only the chunks of a split run (device default
// / GLINT_PUSH_UNORDERED) add with atomics, as in rows_fold.
#include "glint_axpy.h"  // axpy_mul, axpy_add, lane_get: shared with the row-pair axpy push
#include "glint_host.h"

namespace glint {

constexpr int kAxpyTile = 4;   // vectors whose slices a wave holds in registers at a time
constexpr int kAxpyDepth = 8;  // records blocked against one pass over x when q > kAxpyTile

// The contribution of the record whose coefficients lane r holds, from the q resident slices, added to acc.
template <typename V, int VPL, int QT>
__device__ __forceinline__ void axpy_record(V (&acc)[VPL], const V (&cf)[QT], const V (&xs)[QT][VPL], int q, u32 r) {
  V t[VPL];
  const V c0 = lane_get(cf[0], r);
#pragma unroll
  for (int k = 0; k < VPL; ++k) t[k] = axpy_mul(c0, xs[0][k]);
#pragma unroll
  for (int j = 1; j < QT; ++j) {
    if (j < q) {
      const V cj = lane_get(cf[j], r);
#pragma unroll
      for (int k = 0; k < VPL; ++k) t[k] = axpy_add(t[k], axpy_mul(cj, xs[j][k]));
    }
  }
#pragma unroll
  for (int k = 0; k < VPL; ++k) acc[k] = axpy_add(acc[k], t[k]);
}

// q <= QT vectors (QT 1 or kAxpyTile): their slices are loaded once per item and stay in registers, and
// every lane loads its own record's q coefficients with its record id; a contribution is then q
// multiplies and q adds on values handed round by v_readlane, and reads no memory.
template <typename V, int VPL, bool WIDE, int QT>
__device__ __forceinline__ void axpy_fold_resident(V (&acc)[VPL], const u32* __restrict__ idx, u32 start, u32 len,
                                                   const V* __restrict__ coef, const V* __restrict__ x, int q, i64 c,
                                                   i64 cols, int lane) {
  const int qq = QT == 1 ? 1 : q;
  V xs[QT][VPL];
#pragma unroll
  for (int j = 0; j < QT; ++j) {
    if (j < qq) {
      slice_load<V, VPL, WIDE>(xs[j], x + (i64)j * cols, c, cols);
    } else {
#pragma unroll
      for (int k = 0; k < VPL; ++k) xs[j][k] = V(0);
    }
  }
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < m ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    V cf[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) cf[j] = ((u32)lane < m && j < qq) ? coef[(i64)mine * qq + j] : V(0);
    // four records per trip, unrolled by hand (a loop around v_readlane is not unrolled with a remainder)
    u32 r = 0;
    for (; r + 4 <= m; r += 4) {
#pragma unroll
      for (u32 u = 0; u < 4; ++u) axpy_record<V, VPL, QT>(acc, cf, xs, qq, r + u);
    }
    for (; r < m; ++r) axpy_record<V, VPL, QT>(acc, cf, xs, qq, r);
  }
}

// The slices of kAxpyTile vectors from j0 on. A vector past q - 1 is loaded as a copy of the last one and
// never used: the loads carry no branch, so that they stay in flight over the arithmetic in front of them.
template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void axpy_tile_load(V (&xs)[kAxpyTile][VPL], const V* __restrict__ x, int j0, int q, i64 c,
                                               i64 cols) {
#pragma unroll
  for (int jj = 0; jj < kAxpyTile; ++jj) {
    const int j = j0 + jj < q ? j0 + jj : q - 1;
    slice_load<V, VPL, WIDE>(xs[jj], x + (i64)j * cols, c, cols);
  }
}

// Those vectors (FULL: all kAxpyTile exist) advance the partial t of every record of the block (ND: all
// kAxpyDepth exist), in ascending j; lane j of cf[d] holds coefficient j of record d.
template <typename V, int VPL, bool FULL, bool ND>
__device__ __forceinline__ void axpy_tile_use(V (&t)[kAxpyDepth][VPL], const V (&cf)[kAxpyDepth], u32 nd,
                                              const V (&xs)[kAxpyTile][VPL], int j0, int q) {
#pragma unroll
  for (int jj = 0; jj < kAxpyTile; ++jj) {
    if (FULL || j0 + jj < q) {
#pragma unroll
      for (int d = 0; d < kAxpyDepth; ++d) {
        if (ND || (u32)d < nd) {
          const V cj = lane_get(cf[d], (u32)(j0 + jj));
#pragma unroll
          for (int k = 0; k < VPL; ++k) t[d][k] = axpy_add(t[d][k], axpy_mul(cj, xs[jj][k]));
        }
      }
    }
  }
}

// Lane j's coefficient j of the kAxpyDepth records from position r0 of the wave's m record ids: one
// coalesced load of q elements per record. A record past m - 1 repeats the last one and a lane past q - 1
// the last coefficient; neither is used (no branch around the loads).
template <typename V>
__device__ __forceinline__ void axpy_coef_load(V (&cf)[kAxpyDepth], u32 mine, u32 r0, u32 m,
                                               const V* __restrict__ coef, int q, int lane) {
  const int jl = lane < q ? lane : q - 1;
#pragma unroll
  for (int d = 0; d < kAxpyDepth; ++d) {
    const u32 r = r0 + d < m ? r0 + d : m - 1;
    const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)r);
    cf[d] = coef[(i64)id * q + jl];
  }
}

// One block of nd <= kAxpyDepth records (ND: exactly kAxpyDepth): the first vector starts every t, vectors
// 1 .. kAxpyTile advance them from the slices the wave keeps (x0, x1), the later tiles from two buffers
// loaded one tile ahead of their use, and the finished t are added in list order.
template <typename V, int VPL, bool WIDE, bool ND>
__device__ __forceinline__ void axpy_block(V (&acc)[VPL], const V (&cf)[kAxpyDepth], u32 nd, const V (&x0)[VPL],
                                           const V (&x1)[kAxpyTile][VPL], const V* __restrict__ x, int q, i64 c,
                                           i64 cols) {
  V xa[kAxpyTile][VPL], xb[kAxpyTile][VPL];
  int j0 = 1 + kAxpyTile;
  if (j0 < q) axpy_tile_load<V, VPL, WIDE>(xa, x, j0, q, c, cols);
  V t[kAxpyDepth][VPL];
#pragma unroll
  for (int d = 0; d < kAxpyDepth; ++d) {
    const V c0 = lane_get(cf[d], 0u);
#pragma unroll
    for (int k = 0; k < VPL; ++k) t[d][k] = axpy_mul(c0, x0[k]);
  }
  axpy_tile_use<V, VPL, true, ND>(t, cf, nd, x1, 1, q);  // q > kAxpyTile: vectors 1 .. kAxpyTile exist
  while (j0 < q) {
    if (j0 + kAxpyTile < q) axpy_tile_load<V, VPL, WIDE>(xb, x, j0 + kAxpyTile, q, c, cols);
    axpy_tile_use<V, VPL, false, ND>(t, cf, nd, xa, j0, q);
    j0 += kAxpyTile;
    if (j0 >= q) break;
    if (j0 + kAxpyTile < q) axpy_tile_load<V, VPL, WIDE>(xa, x, j0 + kAxpyTile, q, c, cols);
    axpy_tile_use<V, VPL, false, ND>(t, cf, nd, xb, j0, q);
    j0 += kAxpyTile;
  }
#pragma unroll
  for (int d = 0; d < kAxpyDepth; ++d) {
    if (ND || (u32)d < nd) {
#pragma unroll
      for (int k = 0; k < VPL; ++k) acc[k] = axpy_add(acc[k], t[d][k]);
    }
  }
}

// q > kAxpyTile: kAxpyDepth records are blocked against each pass over x, so x is read once per block of
// records instead of once per record; the order of the sums is the resident path's. The slices of
// vectors 0 .. kAxpyTile are loaded once per item and kept, and the next block's coefficients are loaded
// while this block is computed.
template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void axpy_fold_blocked(V (&acc)[VPL], const u32* __restrict__ idx, u32 start, u32 len,
                                                  const V* __restrict__ coef, const V* __restrict__ x, int q, i64 c,
                                                  i64 cols, int lane) {
  V x0[VPL], x1[kAxpyTile][VPL];
  slice_load<V, VPL, WIDE>(x0, x, c, cols);
  axpy_tile_load<V, VPL, WIDE>(x1, x, 1, q, c, cols);
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < m ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    V cf[kAxpyDepth];
    axpy_coef_load<V>(cf, mine, 0u, m, coef, q, lane);
    for (u32 r0 = 0; r0 < m; r0 += kAxpyDepth) {
      V cfn[kAxpyDepth];
      axpy_coef_load<V>(cfn, mine, r0 + kAxpyDepth < m ? r0 + kAxpyDepth : r0, m, coef, q, lane);
      if (m - r0 >= (u32)kAxpyDepth) axpy_block<V, VPL, WIDE, true>(acc, cf, (u32)kAxpyDepth, x0, x1, x, q, c, cols);
      else axpy_block<V, VPL, WIDE, false>(acc, cf, m - r0, x0, x1, x, q, c, cols);
#pragma unroll
      for (int d = 0; d < kAxpyDepth; ++d) cf[d] = cfn[d];
    }
  }
}

// Records [start, start + len) of the sorted list, their contributions folded in list order into one slice
// of row `drow` (rows_fold_item's frame). ATOMIC (a chunk of a split run): the chunk's partial sum starts
// from zero and is added with device-scope atomics, each wave instruction over 64 consecutive elements.
// Otherwise the shard's slice is the first term and the sum is stored once.
template <typename V, int VPL, bool WIDE, bool ATOMIC, int QT>
__device__ __forceinline__ void rows_axpy_item(const u32* __restrict__ idx, u32 start, u32 len,
                                               const V* __restrict__ coef, const V* __restrict__ x, int q, V* drow,
                                               i64 c, i64 cols, int lane) {
  V acc[VPL];
  if (ATOMIC) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) acc[k] = V(0);
  } else {
    slice_load<V, VPL, WIDE>(acc, drow, c, cols);
  }
  if constexpr (QT > 0) axpy_fold_resident<V, VPL, WIDE, QT>(acc, idx, start, len, coef, x, q, c, cols, lane);
  else axpy_fold_blocked<V, VPL, WIDE>(acc, idx, start, len, coef, x, q, c, cols, lane);
  if (ATOMIC) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const i64 cc = c + (i64)k * 64;
      if (cc < cols) gadd(drow + cc, acc[k]);
    }
  } else {
    slice_store<V, VPL, WIDE>(acc, drow, c, cols);
  }
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves. A slice
// is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple of 16 and x 16-B aligned; the shard's pitch
// always is), else one element per lane. QT: 1 for q == 1, kAxpyTile for 2 <= q <= kAxpyTile (both keep x
// in registers), 0 for larger q (blocked).
template <typename V, bool VEC16, bool SPLIT, int QT>
__global__ __launch_bounds__(kTPB) void rows_axpy_fold_kernel(const u32* __restrict__ key, const u32* __restrict__ idx,
                                                              const uint2* __restrict__ items,
                                                              const u32* __restrict__ nitems,
                                                              const V* __restrict__ coef, const V* __restrict__ x,
                                                              int q, V* data, PartDesc part) {
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
    const bool chunk = SPLIT && (e.y & kRowsSplitBit) != 0;
    const u32 len = SPLIT ? e.y & ~kRowsSplitBit : e.y;
    V* drow = data + (i64)key[e.x] * part.pitch;
    const i64 c0 = (i64)slice * 64 * VPL;
    if (chunk) rows_axpy_item<V, VPL, false, true, QT>(idx, e.x, len, coef, x, q, drow, c0 + lane, cols, lane);
    else
      rows_axpy_item<V, VPL, VEC16, false, QT>(idx, e.x, len, coef, x, q, drow,
                                               VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------
template <typename V, bool VEC16, bool SPLIT>
static auto axpy_kernel_for(i64 q) {
  return q == 1           ? rows_axpy_fold_kernel<V, VEC16, SPLIT, 1>
         : q <= kAxpyTile ? rows_axpy_fold_kernel<V, VEC16, SPLIT, kAxpyTile>
                          : rows_axpy_fold_kernel<V, VEC16, SPLIT, 0>;
}

// Enqueues a row axpy push of n records on st (no host synchronisation): the front end's launches and
// the one fold launch. Under the shard's lock.
template <typename V>
int push_rows_axpy(glint_shard* s, const i64* rows, i64 n, const void* coef, const void* x, i64 q, int flags,
                   hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !coef || !x || q < 1 || q > GLINT_AXPY_MAX_VECTORS) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  RowsFront f;
  int rc = rows_front(s, rows, n, flags, st, &f);
  if (rc) return rc;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(x, 16);
  const i64 slices = row_slices<V>(s->part.cols, v16);
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)s->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const V*, const V*, int, V*, PartDesc) =
      v16 ? (f.strict ? axpy_kernel_for<V, true, false>(q) : axpy_kernel_for<V, true, true>(q))
          : (f.strict ? axpy_kernel_for<V, false, false>(q) : axpy_kernel_for<V, false, true>(q));
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS_AXPY, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const V*)coef,
                  (const V*)x, (int)q, (V*)s->data, s->part));
  return GLINT_OK;
}

template int push_rows_axpy<int>(glint_shard*, const i64*, i64, const void*, const void*, i64, int, hipStream_t);
template int push_rows_axpy<long long>(glint_shard*, const i64*, i64, const void*, const void*, i64, int, hipStream_t);
template int push_rows_axpy<float>(glint_shard*, const i64*, i64, const void*, const void*, i64, int, hipStream_t);
template int push_rows_axpy<double>(glint_shard*, const i64*, i64, const void*, const void*, i64, int, hipStream_t);

}  // namespace glint
