// glint_rows.hip -- whole-row matrix push (glint_mat_push_rows*, DESIGN.md "Row push"): the write
// counterpart of getRows. The caller's values already are the list of contribution rows, so the push
// is an inverted index -- per destination row, the records that hit it, in push order -- and one
// coalesced pass that sums each destination's rows into the shard with one plain read-modify-write:
//   rows_prepare   record i -> (local row, i), both u32; a row outside the partition gets the
//                  sentinel part.size (sorts last, skipped) and is recorded as an error;
//   rs_sort        the stable LSD radix sort of glint_sort.hip by local row: equal rows keep push order;
//   rows_runs      one work item per distinct destination row (start and length of its run in the
//                  sorted list), or per chunk of a long run when the sum's order is free;
//   rows_fold      one wave per (item, column slice): shard slice + the run's contribution slices,
//                  strictly in list order -- PartialMatrix.update's `+=` sequence
//                  (PartialMatrix.scala:74-83) over the expanded triplets, rounding for rounding.
// No float atomics on the strict path: column slices of one row are disjoint and every row has one
// item. Only the chunks of a split run (device default / GLINT_PUSH_UNORDERED) add with atomics.
#include "glint_device.h"
#include "glint_host.h"


namespace glint {

constexpr int kRowsDepth = 8;     // contribution loads in flight per wave (the adds are the only chain)
// (kRowsChunk and kRowsSplitBit: glint_host.h, with rows_front)

__global__ __launch_bounds__(kTPB) void rows_prepare_kernel(const i64* __restrict__ rows, i64 n, PartDesc part,
                                                            u32* __restrict__ key, u32* __restrict__ idx,
                                                            u32* __restrict__ nitems, ErrState* err) {
  if (blockIdx.x == 0 && threadIdx.x == 0) *nitems = 0;  // rows_runs appends from here (no memset per push)
  for (i64 i = (i64)blockIdx.x * kTPB + threadIdx.x; i < n; i += (i64)gridDim.x * kTPB) {
    const int32_t l = g2l(part, rows[i]);
    const bool ok = l >= 0 && l < part.size;
    if (!ok) record_error(err, i);
    key[i] = ok ? (u32)l : (u32)part.size;
    idx[i] = (u32)i;
  }
}

// One item per run of equal keys in the sorted list: {start, length}. The head of a run finds its end
// by a gallop and a bisection over the sorted keys (a run of one record: one probe). With SPLIT a run
// longer than kRowsChunk becomes ceil(len / kRowsChunk) items marked kRowsSplitBit. The sum over runs of
// their item counts is at most n, the capacity of `items`; their order in the list does not matter.
template <bool SPLIT>
__global__ __launch_bounds__(kTPB) void rows_runs_kernel(const u32* __restrict__ key, i64 n, u32 sentinel,
                                                         u32* __restrict__ nitems, uint2* __restrict__ items) {
  for (i64 i = (i64)blockIdx.x * kTPB + threadIdx.x; i < n; i += (i64)gridDim.x * kTPB) {
    const u32 k = key[i];
    if (k == sentinel) continue;
    if (i > 0 && key[i - 1] == k) continue;  // not the head of its run
    i64 lo = i, hi = n;                      // key[lo] == k; the end lies in (lo, hi]
    for (i64 step = 1;; step <<= 1) {
      const i64 p = lo + step;
      if (p >= n) break;
      if (key[p] != k) { hi = p; break; }
      lo = p;
    }
    while (hi - lo > 1) {
      const i64 mid = lo + (hi - lo) / 2;
      if (key[mid] == k) lo = mid;
      else hi = mid;
    }
    const i64 len = hi - i;
    if (SPLIT && len > (i64)kRowsChunk) {
      const u32 nch = (u32)((len + kRowsChunk - 1) / kRowsChunk);
      const u32 slot = atomicAdd(nitems, nch);
      for (u32 q = 0; q < nch; ++q) {
        const i64 o = (i64)q * kRowsChunk;
        const u32 l = (u32)(len - o < (i64)kRowsChunk ? len - o : (i64)kRowsChunk);
        items[slot + q] = make_uint2((u32)(i + o), l | kRowsSplitBit);
      }
    } else {
      items[atomicAdd(nitems, 1u)] = make_uint2((u32)i, (u32)len);
    }
  }
}

// Records [start, start + len) of the sorted list, folded in list order into one slice of row `drow`.
// ATOMIC (a chunk of a split run): the chunk's partial sum is added with device-scope atomics, each
// wave instruction over 64 consecutive elements; every chunk of that run does the same, so no plain
// store ever meets them. Otherwise: the shard's slice is the first term and the sum is stored once.
template <typename V, int VPL, bool WIDE, bool ATOMIC>
__device__ __forceinline__ void rows_fold_item(const u32* __restrict__ idx, u32 start, u32 len,
                                               const V* __restrict__ vals, V* drow, i64 c, i64 cols, int lane) {
  V acc[VPL];
  if (ATOMIC) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) acc[k] = V(0);
  } else {
    slice_load<V, VPL, WIDE>(acc, drow, c, cols);
  }
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < m ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    for (u32 j = 0; j < m; j += kRowsDepth) {
      V t[kRowsDepth][VPL];
      if (m - j >= (u32)kRowsDepth) {
#pragma unroll
        for (int d = 0; d < kRowsDepth; ++d) {
          const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
          slice_load<V, VPL, WIDE>(t[d], vals + (i64)id * cols, c, cols);
        }
#pragma unroll
        for (int d = 0; d < kRowsDepth; ++d)
#pragma unroll
          for (int k = 0; k < VPL; ++k) acc[k] = vadd(acc[k], t[d][k]);
      } else {  // the run's last few records (wave-uniform tests)
#pragma unroll
        for (int d = 0; d < kRowsDepth; ++d) {
          if (j + d < m) {
            const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
            slice_load<V, VPL, WIDE>(t[d], vals + (i64)id * cols, c, cols);
          }
        }
#pragma unroll
        for (int d = 0; d < kRowsDepth; ++d) {
          if (j + d < m) {
#pragma unroll
            for (int k = 0; k < VPL; ++k) acc[k] = vadd(acc[k], t[d][k]);
          }
        }
      }
    }
  }
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
// is 64 lanes x 16 B when VEC16 (the input row stride and `vals` are 16-B aligned; the shard's pitch
// always is), else one element per lane.
template <typename V, bool VEC16, bool SPLIT>
__global__ __launch_bounds__(kTPB) void rows_fold_kernel(const u32* __restrict__ key, const u32* __restrict__ idx,
                                                         const uint2* __restrict__ items,
                                                         const u32* __restrict__ nitems, const V* __restrict__ vals,
                                                         V* data, PartDesc part) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the item, its run and the record indices are then wave-uniform to
  // the compiler too (scalar loads and addresses, no per-lane copies)
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
    if (chunk) rows_fold_item<V, VPL, false, true>(idx, e.x, len, vals, drow, c0 + lane, cols, lane);
    else rows_fold_item<V, VPL, VEC16, false>(idx, e.x, len, vals, drow, VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// The row pushes' shared front end (glint_host.h): scratch layout in s->d_det, then rows_prepare,
// rs_sort and rows_runs on st. n > 0 and n < 2^32 - kSortTile (32-bit record indices and sort offsets).
int rows_front(glint_shard* s, const i64* rows, i64 n, int flags, hipStream_t st, RowsFront* out) {
  const u32 sentinel = (u32)s->part.size;
  int end_bit = 1;
  while (end_bit < 32 && ((u64)1 << end_bit) <= (u64)sentinel) ++end_bit;
  // Message order by default on the host-pointer path (kPushHostSequential's rule) and whenever the
  // caller asks for it; otherwise long runs are split (exact for Int/Long either way).
  const bool strict = (flags & GLINT_PUSH_DETERMINISTIC) ||
                      ((flags & kPushHostSequential) && !(flags & GLINT_PUSH_UNORDERED));
  const u32 ntiles = (u32)((n + kSortTile - 1) / kSortTile);
  const size_t b_key = pad256((size_t)n * 4), b_items = pad256((size_t)n * sizeof(uint2));
  const size_t b_hist = pad256((size_t)ntiles * 256 * 4);
  const size_t need = 4 * b_key + b_items + 2 * b_hist + 1024 + 256;
  int rc = grow(&s->d_det, &s->det_bytes, need);
  if (rc) return rc;
  char* base = (char*)s->d_det;
  u32* key0 = (u32*)base;
  u32* key1 = (u32*)(base + b_key);
  u32* idx0 = (u32*)(base + 2 * b_key);
  u32* idx1 = (u32*)(base + 3 * b_key);
  uint2* items = (uint2*)(base + 4 * b_key);
  u32* hist = (u32*)(base + 4 * b_key + b_items);
  u32* offs = (u32*)((char*)hist + b_hist);
  u32* tot = (u32*)((char*)offs + b_hist);
  u32* nitems = (u32*)((char*)tot + 1024);
  const unsigned g = grid_for(n, kTPB, (i64)s->cus * 8);
  rows_prepare_kernel<<<g, kTPB, 0, st>>>(rows, n, s->part, key0, idx0, nitems, err_of(s));
  HIPCHK(hipGetLastError());
  int where = 0;
  rc = rs_sort<u32, u32>(key0, idx0, key1, idx1, n, end_bit, hist, offs, tot, st, &where);
  if (rc) return rc;
  const u32* key = where ? key1 : key0;
  if (strict) rows_runs_kernel<false><<<g, kTPB, 0, st>>>(key, n, sentinel, nitems, items);
  else rows_runs_kernel<true><<<g, kTPB, 0, st>>>(key, n, sentinel, nitems, items);
  HIPCHK(hipGetLastError());
  *out = RowsFront{key, where ? idx1 : idx0, items, nitems, strict};
  return GLINT_OK;
}

// Enqueues a row push of n records on st (no host synchronisation). Under the shard's lock.
template <typename V>
int push_rows(glint_shard* s, const i64* rows, const void* vals, i64 n, int flags, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !vals) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  RowsFront f;
  int rc = rows_front(s, rows, n, flags, st, &f);
  if (rc) return rc;
  const bool strict = f.strict;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(vals, 16);
  const i64 slices = row_slices<V>(s->part.cols, v16);
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)s->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const V*, V*, PartDesc) =
      v16 ? (strict ? rows_fold_kernel<V, true, false> : rows_fold_kernel<V, true, true>)
          : (strict ? rows_fold_kernel<V, false, false> : rows_fold_kernel<V, false, true>);
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const V*)vals,
                  (V*)s->data, s->part));
  return GLINT_OK;
}

template int push_rows<int>(glint_shard*, const i64*, const void*, i64, int, hipStream_t);
template int push_rows<long long>(glint_shard*, const i64*, const void*, i64, int, hipStream_t);
template int push_rows<float>(glint_shard*, const i64*, const void*, i64, int, hipStream_t);
template int push_rows<double>(glint_shard*, const i64*, const void*, i64, int, hipStream_t);

}  // namespace glint
