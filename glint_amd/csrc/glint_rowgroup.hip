// glint_rowgroup.hip -- grouped row push (glint_mat_push_rows_grouped*, DESIGN.md "Grouped row push"): the
// write side of the grouped row-sum pull. The caller names n rows in g groups and sends one value row per
// group; every record adds its group's row, optionally times its own coefficient, so that g x cols values
// cross the link instead of the n x cols expanded rows glint_mat_push_rows would need.
//   rows_front        the row push's front end unchanged;
//   rows_group_ids    record i -> its group, a u32 per record in the shard's group-id scratch: one thread
//                     per record searches the clamped grp_ptr, so the searches run side by side and not on
//                     the fold's chain of dependent loads (DESIGN.md has both measured);
//   rows_group_fold   one wave per (item, column slice): shard slice + the run's contributions
//                     vals[group of record i] (COEF: coef[i] * that), strictly in list order -- the row
//                     push of those rows, rounding for rounding (glint_axpy.h).
// Only `cols` elements of a shard row are read or written, never the pitch padding; `vals` has no pitch.
#include "glint_axpy.h"   // axpy_mul, axpy_add, lane_get: shared with the axpy pushes
#include "glint_group.h"  // group_cut, group_find: shared with the grouped row-dot pull
#include "glint_host.h"

namespace glint {

constexpr int kRowsDepth = 8;  // value-row slice loads in flight per wave (glint_rows.hip's kRowsDepth)

constexpr u32 kNoGroup = 0xFFFFFFFFu;  // rows_group_ids: no group covers the record (-1 as the fold reads it)

// One thread per record; neighbouring records take nearly the same path through grp_ptr.
__global__ __launch_bounds__(kTPB) void rows_group_ids_kernel(const i64* __restrict__ grp_ptr, i64 g, i64 n,
                                                              u32* __restrict__ gids) {
  for (i64 i = (i64)blockIdx.x * kTPB + threadIdx.x; i < n; i += (i64)gridDim.x * kTPB) {
    const int32_t k = group_find(grp_ptr, g, n, i);
    gids[i] = k < 0 ? kNoGroup : (u32)k;
  }
}

// The m <= 64 records whose groups (-1: none) and coefficients the lanes hold, folded in list order into
// acc: kRowsDepth value-row slice loads are issued, v_readlane handing the group ids round, then their
// contributions are added -- with COEF the product rounded before the add, without it the stored bits and
// no multiply. CHECK: some record of the batch has no group; it is skipped by a wave-uniform branch -- no
// load, no add. Without CHECK (every well-formed call) the loop carries no such branch:
// pairs_axpy_batch's routes.
template <typename V, int VPL, bool WIDE, bool COEF, bool CHECK>
__device__ __forceinline__ void rows_group_batch(V (&acc)[VPL], bool& any, int32_t gid, V cf, u32 m,
                                                 const V* __restrict__ vals, i64 c, i64 cols) {
  constexpr int D = kRowsDepth;
  for (u32 j = 0; j < m; j += D) {
    V t[D][VPL];
    const bool full = m - j >= (u32)D;  // else the batch's last few records (wave-uniform tests)
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if (full || j + d < m) {
        const int32_t k = __builtin_amdgcn_readlane(gid, (int)(j + d));
        if (!CHECK || k >= 0) slice_load<V, VPL, WIDE>(t[d], vals + (i64)k * cols, c, cols);
      }
    }
#pragma unroll
    for (int d = 0; d < D; ++d) {
      if ((full || j + d < m) && (!CHECK || __builtin_amdgcn_readlane(gid, (int)(j + d)) >= 0)) {
        if (COEF) {
          const V cd = lane_get(cf, j + d);
#pragma unroll
          for (int q = 0; q < VPL; ++q) acc[q] = axpy_add(acc[q], axpy_mul(cd, t[d][q]));
        } else {
#pragma unroll
          for (int q = 0; q < VPL; ++q) acc[q] = axpy_add(acc[q], t[d][q]);
        }
        any = true;
      }
    }
  }
}

// Records [start, start + len) of the sorted list, their contributions folded in list order into one
// slice of row `drow` (rows_fold_item's frame). The wave reads 64 record ids at a time; every lane loads
// its own record's group id and, with COEF, its coefficient. A record that no group covers (a
// malformed device grp_ptr only) is skipped -- the row's bits are as if it were absent -- and not
// reported.
// ATOMIC (a chunk of a split run): the chunk's partial sum starts from zero and is added with
// device-scope atomics, each wave instruction over 64 consecutive elements -- unless every record of
// the chunk was skipped. Otherwise the shard's slice is the first term and the sum is stored once.
template <typename V, int VPL, bool WIDE, bool ATOMIC, bool COEF>
__device__ __forceinline__ void rows_group_item(const u32* __restrict__ idx, u32 start, u32 len,
                                                const u32* __restrict__ gids, const V* __restrict__ vals,
                                                const V* __restrict__ coef, V* drow, i64 c, i64 cols, int lane) {
  V acc[VPL];
  if (ATOMIC) {
#pragma unroll
    for (int q = 0; q < VPL; ++q) acc[q] = V(0);
  } else {
    slice_load<V, VPL, WIDE>(acc, drow, c, cols);
  }
  bool any = false;  // wave-uniform: some record of the item contributed
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
    if (__ballot(none) == 0) rows_group_batch<V, VPL, WIDE, COEF, false>(acc, any, gid, cf, m, vals, c, cols);
    else rows_group_batch<V, VPL, WIDE, COEF, true>(acc, any, gid, cf, m, vals, c, cols);
  }
  if (ATOMIC) {
    if (any) {
#pragma unroll
      for (int q = 0; q < VPL; ++q) {
        const i64 cc = c + (i64)q * 64;
        if (cc < cols) gadd(drow + cc, acc[q]);
      }
    }
  } else {
    slice_store<V, VPL, WIDE>(acc, drow, c, cols);
  }
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves
// (pairs_axpy_fold_kernel's frame). A slice is 64 lanes x 16 B when VEC16 (`vals` 16-B aligned and
// cols * sizeof(V) a multiple of 16, so every value row is; the shard's pitch always is), else one
// element per lane.
template <typename V, bool VEC16, bool SPLIT, bool COEF>
__global__ __launch_bounds__(kTPB) void rows_group_fold_kernel(const u32* __restrict__ key, const u32* __restrict__ idx,
                                                               const uint2* __restrict__ items,
                                                               const u32* __restrict__ nitems,
                                                               const u32* __restrict__ gids,
                                                               const V* __restrict__ vals,
                                                               const V* __restrict__ coef, V* data, PartDesc part) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the item, its run and the group ids handed round are then
  // wave-uniform to the compiler too (rows_fold_kernel's pattern)
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
    if (chunk)
      rows_group_item<V, VPL, false, true, COEF>(idx, e.x, len, gids, vals, coef, drow, c0 + lane, cols, lane);
    else
      rows_group_item<V, VPL, VEC16, false, COEF>(idx, e.x, len, gids, vals, coef, drow,
                                                  VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------
template <typename V, bool VEC16, bool SPLIT>
int launch_group_fold(glint_shard* s, const RowsFront& f, const u32* gids, const void* vals, const void* coef,
                      unsigned grid, hipStream_t st) {
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const u32*, const V*, const V*, V*, PartDesc) =
      coef ? rows_group_fold_kernel<V, VEC16, SPLIT, true> : rows_group_fold_kernel<V, VEC16, SPLIT, false>;
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS, fold, grid, kTPB, st, f.key, f.idx, f.items, f.nitems, gids, (const V*)vals, (const V*)coef, (V*)s->data, s->part));
  return GLINT_OK;
}

// Enqueues a grouped row push of n records in g groups on st (no host synchronisation): the front end's
// launches, the group-id launch (uncounted, as the front end's) and the one fold launch. Under the shard's
// lock.
template <typename V>
int push_rows_grouped(glint_shard* s, const i64* rows, i64 n, const i64* grp_ptr, i64 g, const void* vals,
                      const void* coef, int flags, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !grp_ptr || (g > 0 && !vals)) return GLINT_EINVAL;
  if (g < 0 || g >= ((i64)1 << 31)) return GLINT_EINVAL;     // 31-bit group ids
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  int rc = grow(&s->d_grp, &s->grp_bytes, (size_t)n * 4);
  if (rc) return rc;
  u32* gids = (u32*)s->d_grp;
  RowsFront f;
  rc = rows_front(s, rows, n, flags, st, &f);
  if (rc) return rc;
  rows_group_ids_kernel<<<grid_for(n, kTPB, (i64)s->cus * 8), kTPB, 0, st>>>(grp_ptr, g, n, gids);
  HIPCHK(hipGetLastError());
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(vals, 16);
  const i64 slices = row_slices<V>(s->part.cols, v16);
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)s->cus * 8);
  if (v16)
    return f.strict ? launch_group_fold<V, true, false>(s, f, gids, vals, coef, gf, st)
                    : launch_group_fold<V, true, true>(s, f, gids, vals, coef, gf, st);
  return f.strict ? launch_group_fold<V, false, false>(s, f, gids, vals, coef, gf, st)
                  : launch_group_fold<V, false, true>(s, f, gids, vals, coef, gf, st);
}

template int push_rows_grouped<int>(glint_shard*, const i64*, i64, const i64*, i64, const void*, const void*, int,
                                    hipStream_t);
template int push_rows_grouped<long long>(glint_shard*, const i64*, i64, const i64*, i64, const void*, const void*,
                                          int, hipStream_t);
template int push_rows_grouped<float>(glint_shard*, const i64*, i64, const i64*, i64, const void*, const void*, int,
                                      hipStream_t);
template int push_rows_grouped<double>(glint_shard*, const i64*, i64, const i64*, i64, const void*, const void*,
                                       int, hipStream_t);

}  // namespace glint
