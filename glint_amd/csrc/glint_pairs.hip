// glint_pairs.hip -- row-pair dot pull and row-pair axpy push (glint_mat_pull_pairs_dot*,
// glint_mat_push_pairs_axpy*, DESIGN.md "Row-pair dot pull and axpy push"): the two halves of a scoring
// step whose other operand is not the caller's but a row of a second shard on the same device, so that
// nothing of size `cols` crosses the link.
//   pairs_dot        one wave per pair: the strips of both rows are loaded first, several in flight, then
//                    every lane adds the products of its own columns in ascending column order and the 64
//                    lane sums are combined by the xor butterfly -- the row dot pull's arithmetic
//                    (glint_dot.h), bit for bit;
//   rows_front       the row push's front end unchanged, on the destination shard;
//   pairs_axpy_fold  one wave per (item, column slice): shard slice + the run's contributions
//                    coef[i] * (source slice), strictly in list order -- the row push of those rows,
//                    rounding for rounding (glint_axpy.h).
// Each row array is translated with its own shard's PartDesc; only `cols` elements of a row of either
// shard are read or written, never the pitch padding.
#include "glint_axpy.h"  // axpy_mul, axpy_add, lane_get: shared with the row axpy push
#include "glint_dot.h"   // dot_step: shared with the row dot pull and the top-k pull's scores
#include "glint_host.h"

namespace glint {

constexpr int kPairDotDepth = 8;   // strips of each of the two rows in flight per wave (kDotDepth<1>)
constexpr int kPairAxpyDepth = 8;  // source-slice loads in flight per wave (kRowsDepth)

// D = kPairDotDepth strips of both rows from strip s on (FULL: all of them exist): the 2 D loads are
// issued first -- both rows come from HBM -- and then their products are added to the lane sum in
// ascending strip, hence column, order: dot_batch's order with one query. A lane whose columns lie past
// cols multiplies zeros: acc + (+0) leaves acc as it is, since a sum that started from +0 is never -0.
template <typename V, int E, bool VEC16, bool FULL>
__device__ __forceinline__ void pairs_dot_batch(V& acc, const V* ra, const V* rb, u32 s, u32 nstrips, int lane,
                                                i64 cols) {
  constexpr int D = kPairDotDepth;
  V a[D][E], b[D][E];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (FULL || s + d < nstrips) {
      const i64 c = ((i64)(s + d) * 64 + lane) * E;
      slice_load<V, E, VEC16>(a[d], ra, c, cols);
      slice_load<V, E, VEC16>(b[d], rb, c, cols);
    }
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (FULL || s + d < nstrips) {
#pragma unroll
      for (int e = 0; e < E; ++e) acc = dot_step(acc, a[d][e], b[d][e]);
    }
  }
}

// Persistent grid; one wave per pair (rows_dot_kernel's frame with one query). A strip is 64 lanes x E
// columns: E = 16 / sizeof(V) when VEC16 (cols * sizeof(V) a multiple of 16; both shards' pitch always
// is), else 1. A pair with either row outside its partition answers zero without a load and is recorded
// once. The two shards may be one, or views that overlap: nothing is written to either.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void pairs_dot_kernel(const i64* __restrict__ rows_a,
                                                         const i64* __restrict__ rows_b, i64 n, const V* adata,
                                                         PartDesc pa, const V* bdata, PartDesc pb,
                                                         V* __restrict__ out, ErrState* err) {
  constexpr int E = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the row ids, their local indices and the bounds tests are then
  // wave-uniform to the compiler too (rows_dot_kernel's pattern)
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = pa.cols;
  const u32 nstrips = (u32)((cols + 64 * E - 1) / (64 * E));
  for (u64 w = w0; w < (u64)n; w += nw) {
    const int32_t la = g2l(pa, rows_a[w]);
    const int32_t lb = g2l(pb, rows_b[w]);
    V acc = V(0);
    if (la >= 0 && la < pa.size && lb >= 0 && lb < pb.size) {
      const V* ra = adata + (i64)la * pa.pitch;
      const V* rb = bdata + (i64)lb * pb.pitch;
      u32 s = 0;
      for (; s + kPairDotDepth <= nstrips; s += kPairDotDepth)
        pairs_dot_batch<V, E, VEC16, true>(acc, ra, rb, s, nstrips, lane, cols);
      if (s < nstrips) pairs_dot_batch<V, E, VEC16, false>(acc, ra, rb, s, nstrips, lane, cols);
    } else if (lane == 0) {
      record_error(err, (i64)w);
    }
    // the xor butterfly: IEEE addition commutes, so every lane ends with the same bits
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) acc = vadd(acc, __shfl_xor(acc, d, 64));
    if (lane == 0) out[w] = acc;
  }
}

// The m <= 64 records whose local source rows (-1: none) and coefficients the lanes hold, folded in list
// order into acc: kPairAxpyDepth source-slice loads are issued, v_readlane handing the rows round, then
// their contributions coef * slice are added -- the product rounded before the add. CHECK: some record
// of the batch has no source row; it is skipped by a wave-uniform branch -- no load, no add. Without
// CHECK (the common case) the loop carries no such branch: rows_fold_item's loop.
template <typename V, int VPL, bool WIDE, bool CHECK>
__device__ __forceinline__ void pairs_axpy_batch(V (&acc)[VPL], bool& any, int32_t ls, V cf, u32 m,
                                                 const V* __restrict__ sdata, i64 spitch, i64 c, i64 cols) {
  constexpr int D = kPairAxpyDepth;
  for (u32 j = 0; j < m; j += D) {
    V t[D][VPL];
    if (m - j >= (u32)D) {
#pragma unroll
      for (int d = 0; d < D; ++d) {
        const int32_t l = __builtin_amdgcn_readlane(ls, (int)(j + d));
        if (!CHECK || l >= 0) slice_load<V, VPL, WIDE>(t[d], sdata + (i64)l * spitch, c, cols);
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        if (!CHECK || __builtin_amdgcn_readlane(ls, (int)(j + d)) >= 0) {
          const V cd = lane_get(cf, j + d);
#pragma unroll
          for (int k = 0; k < VPL; ++k) acc[k] = axpy_add(acc[k], axpy_mul(cd, t[d][k]));
          any = true;
        }
      }
    } else {  // the batch's last few records (wave-uniform tests)
#pragma unroll
      for (int d = 0; d < D; ++d) {
        if (j + d < m) {
          const int32_t l = __builtin_amdgcn_readlane(ls, (int)(j + d));
          if (!CHECK || l >= 0) slice_load<V, VPL, WIDE>(t[d], sdata + (i64)l * spitch, c, cols);
        }
      }
#pragma unroll
      for (int d = 0; d < D; ++d) {
        if (j + d < m && (!CHECK || __builtin_amdgcn_readlane(ls, (int)(j + d)) >= 0)) {
          const V cd = lane_get(cf, j + d);
#pragma unroll
          for (int k = 0; k < VPL; ++k) acc[k] = axpy_add(acc[k], axpy_mul(cd, t[d][k]));
          any = true;
        }
      }
    }
  }
}

// Records [start, start + len) of the sorted list, their contributions coef[i] * (slice of source row
// rows_src[i]) folded in list order into one slice of row `drow` (rows_fold_item's frame). The wave reads
// 64 record ids at a time; every lane loads its own record's source row and coefficient and translates
// the row with the source shard's partition. A record whose source row lies outside that partition is
// skipped -- the destination's bits are as if the record were absent -- and recorded once, by the wave
// of the item's first slice (`report`).
// ATOMIC (a chunk of a split run): the chunk's partial sum starts from zero and is added with
// device-scope atomics, each wave instruction over 64 consecutive elements -- unless every record of
// the chunk was skipped. Otherwise the shard's slice is the first term and the sum is stored once.
template <typename V, int VPL, bool WIDE, bool ATOMIC>
__device__ __forceinline__ void pairs_axpy_item(const u32* __restrict__ idx, u32 start, u32 len,
                                                const i64* __restrict__ rows_src, const V* __restrict__ coef,
                                                const V* __restrict__ sdata, const PartDesc& ps, V* drow, i64 c,
                                                i64 cols, int lane, bool report, ErrState* err) {
  V acc[VPL];
  if (ATOMIC) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) acc[k] = V(0);
  } else {
    slice_load<V, VPL, WIDE>(acc, drow, c, cols);
  }
  bool any = false;  // wave-uniform: some record of the item contributed
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    int32_t ls = -1;  // this lane's record: its local source row, or -1 when it has none
    V cf = V(0);
    bool bad = false;
    if ((u32)lane < m) {
      const u32 mine = idx[(i64)start + b + lane];  // 64 record indices, one per lane
      const int32_t l = g2l(ps, rows_src[mine]);
      cf = coef[mine];
      bad = !(l >= 0 && l < ps.size);
      if (!bad) ls = l;
      else if (report) record_error(err, (i64)mine);
    }
    if (__ballot(bad) == 0) pairs_axpy_batch<V, VPL, WIDE, false>(acc, any, ls, cf, m, sdata, ps.pitch, c, cols);
    else pairs_axpy_batch<V, VPL, WIDE, true>(acc, any, ls, cf, m, sdata, ps.pitch, c, cols);
  }
  if (ATOMIC) {
    if (any) {
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        const i64 cc = c + (i64)k * 64;
        if (cc < cols) gadd(drow + cc, acc[k]);
      }
    }
  } else {
    slice_store<V, VPL, WIDE>(acc, drow, c, cols);
  }
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves
// (rows_axpy_fold_kernel's frame). A slice is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple of
// 16; both shards' pitch always is), else one element per lane. The source shard shares no memory with
// the destination (checked by the caller), so it is read as it was before the call.
template <typename V, bool VEC16, bool SPLIT>
__global__ __launch_bounds__(kTPB) void pairs_axpy_fold_kernel(const u32* __restrict__ key, const u32* __restrict__ idx,
                                                               const uint2* __restrict__ items,
                                                               const u32* __restrict__ nitems,
                                                               const i64* __restrict__ rows_src,
                                                               const V* __restrict__ coef,
                                                               const V* __restrict__ sdata, PartDesc ps, V* data,
                                                               PartDesc part, ErrState* err) {
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
    if (chunk)
      pairs_axpy_item<V, VPL, false, true>(idx, e.x, len, rows_src, coef, sdata, ps, drow, c0 + lane, cols, lane,
                                           slice == 0, err);
    else
      pairs_axpy_item<V, VPL, VEC16, false>(idx, e.x, len, rows_src, coef, sdata, ps, drow,
                                            VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane, slice == 0, err);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the row-pair dot pull on st (no host synchronisation): one launch, recorded on `a`. Under
// both shards' locks; `b` has a's type, device and cols.
template <typename V>
int pull_pairs_dot(glint_shard* a, glint_shard* b, const i64* rows_a, const i64* rows_b, i64 n, void* out,
                   hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows_a || !rows_b || !out) return GLINT_EINVAL;
  const bool v16 = ((i64)a->part.cols * (i64)sizeof(V)) % 16 == 0;
  const unsigned grid = grid_for(n, kTPB / 64, (i64)a->cus * 8);
  void (*k)(const i64*, const i64*, i64, const V*, PartDesc, const V*, PartDesc, V*, ErrState*) =
      v16 ? pairs_dot_kernel<V, true> : pairs_dot_kernel<V, false>;
  HIPCHK(launch_k(a, GLINT_K_PULL_ROWS_DOT, k, grid, kTPB, st, rows_a, rows_b, n, (const V*)a->data, a->part,
                  (const V*)b->data, b->part, (V*)out, err_of(a)));
  return GLINT_OK;
}

template int pull_pairs_dot<int>(glint_shard*, glint_shard*, const i64*, const i64*, i64, void*, hipStream_t);
template int pull_pairs_dot<long long>(glint_shard*, glint_shard*, const i64*, const i64*, i64, void*, hipStream_t);
template int pull_pairs_dot<float>(glint_shard*, glint_shard*, const i64*, const i64*, i64, void*, hipStream_t);
template int pull_pairs_dot<double>(glint_shard*, glint_shard*, const i64*, const i64*, i64, void*, hipStream_t);

// Enqueues a row-pair axpy push of n records on st (no host synchronisation): the front end's launches
// (scratch, error state and profile of `dst`) and the one fold launch. Under both shards' locks; `src`
// has dst's type, device and cols and shares no memory with it.
template <typename V>
int push_pairs_axpy(glint_shard* dst, glint_shard* src, const i64* rows_dst, const i64* rows_src, const void* coef,
                    i64 n, int flags, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows_dst || !rows_src || !coef) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  RowsFront f;
  int rc = rows_front(dst, rows_dst, n, flags, st, &f);
  if (rc) return rc;
  const bool v16 = ((i64)dst->part.cols * (i64)sizeof(V)) % 16 == 0;
  const i64 slices = row_slices<V>(dst->part.cols, v16);
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)dst->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const i64*, const V*, const V*, PartDesc, V*,
               PartDesc, ErrState*) =
      v16 ? (f.strict ? pairs_axpy_fold_kernel<V, true, false> : pairs_axpy_fold_kernel<V, true, true>)
          : (f.strict ? pairs_axpy_fold_kernel<V, false, false> : pairs_axpy_fold_kernel<V, false, true>);
  HIPCHK(launch_k(dst, GLINT_K_PUSH_ROWS_AXPY, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, rows_src,
                  (const V*)coef, (const V*)src->data, src->part, (V*)dst->data, dst->part, err_of(dst)));
  return GLINT_OK;
}

template int push_pairs_axpy<int>(glint_shard*, glint_shard*, const i64*, const i64*, const void*, i64, int,
                                  hipStream_t);
template int push_pairs_axpy<long long>(glint_shard*, glint_shard*, const i64*, const i64*, const void*, i64, int,
                                        hipStream_t);
template int push_pairs_axpy<float>(glint_shard*, glint_shard*, const i64*, const i64*, const void*, i64, int,
                                    hipStream_t);
template int push_pairs_axpy<double>(glint_shard*, glint_shard*, const i64*, const i64*, const void*, i64, int,
                                     hipStream_t);

}  // namespace glint
