// glint_rowdot.hip -- row dot-product pull (glint_mat_pull_rows_dot*, DESIGN.md "Row dot pull"): the
// requested rows times vectors the caller sends, reduced over the columns next to the data, so a
// request of n rows and q vectors is answered with n x q values instead of n x cols.
//   rows_dot   one wave per (request, tile of queries): the wave walks the row in strips of 64 lanes x E
//              columns, every lane adds the products of its own columns in ascending column order, and
//              the 64 lane sums are combined by the xor butterfly.
// The floating-point order is the contract (include/glint_gpu.h): it depends on (type, cols) only, so the
// tile width, the grid and the alignment of x never show in the bits. No atomics, no split of a row.
#include "glint_dot.h"    // dot_step, x_load, dot_batch: shared with the top-k pull's scores
#include "glint_group.h"  // group_find: shared with the grouped row push
#include "glint_host.h"

namespace glint {

// Persistent grid; one wave per (request, tile of QT queries), the tiles of a request on adjacent
// waves so that the row comes from HBM once and from cache for the other tiles. A strip is 64 lanes x
// E columns: E = 16 / sizeof(V) when VEC16 (cols * sizeof(V) a multiple of 16; the shard's pitch always
// is), else 1. Only `cols` elements of a row are read, never the pitch padding. The last tile of a
// request computes its missing queries as copies of the last one and stores only the real ones. A row
// outside the partition answers zeros without a load, recorded once (by the wave of tile 0).
template <typename V, bool VEC16, bool SELF, bool XW, int QT>
__device__ __forceinline__ void rows_dot_body(const i64* __restrict__ rows, i64 n, const V* __restrict__ x, int q,
                                              const V* __restrict__ data, const PartDesc& part, V* __restrict__ out,
                                              ErrState* err) {
  constexpr int E = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the row id, its local index and the bounds test are then
  // wave-uniform to the compiler too (rows_sum_kernel's pattern)
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const u32 nstrips = (u32)((cols + 64 * E - 1) / (64 * E));
  const u32 ntiles = (u32)((q + QT - 1) / QT);
  const u64 total = (u64)n * ntiles;
  for (u64 w = w0; w < total; w += nw) {
    const i64 i = (i64)(w / ntiles);
    const int j0 = (int)(w % ntiles) * QT;
    const int32_t l = g2l(part, rows[i]);
    V acc[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) acc[j] = V(0);
    if (l >= 0 && l < part.size) {
      const V* row = data + (i64)l * part.pitch;
      const V* xq[QT];
#pragma unroll
      for (int j = 0; j < QT; ++j) xq[j] = SELF ? row : x + (i64)(j0 + j < q ? j0 + j : q - 1) * cols;
      u32 s = 0;
      for (; s + kDotDepth<QT> <= nstrips; s += kDotDepth<QT>)
        dot_batch<V, E, VEC16, SELF, XW, QT, true>(acc, row, xq, s, nstrips, lane, cols);
      if (s < nstrips) dot_batch<V, E, VEC16, SELF, XW, QT, false>(acc, row, xq, s, nstrips, lane, cols);
    } else if (j0 == 0 && lane == 0) {
      record_error(err, i);
    }
    // the xor butterfly: IEEE addition commutes, so every lane ends with the same bits
    V mine = acc[0];
#pragma unroll
    for (int j = 0; j < QT; ++j) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) acc[j] = vadd(acc[j], __shfl_xor(acc[j], d, 64));
      if (lane == j) mine = acc[j];
    }
    if (lane < QT && j0 + lane < q) out[i * q + j0 + lane] = mine;  // lane j stores query j0 + j
  }
}

template <typename V, bool VEC16, bool SELF, int QT>
__global__ __launch_bounds__(kTPB) void rows_dot_kernel(const i64* __restrict__ rows, i64 n, const V* __restrict__ x,
                                                        int q, int xwide, const V* __restrict__ data, PartDesc part,
                                                        V* __restrict__ out, ErrState* err) {
  // x by 16 B or by element: the same loop either way, chosen once per launch
  if (VEC16 && !SELF && xwide) rows_dot_body<V, VEC16, SELF, true, QT>(rows, n, x, q, data, part, out, err);
  else rows_dot_body<V, VEC16, SELF, false, QT>(rows, n, x, q, data, part, out, err);
}

// ---- grouped row-dot pull (glint_mat_pull_rows_gdot*, DESIGN.md "Weighted row-sum pull and grouped row
// dot"): out[i] = dot(row rows[i], x[group of record i]), one vector per group and one answer per record --
// the gradient of a weighted bag with respect to its weights, n values instead of the n x g of rows_dot.
//
// Persistent grid; one wave per batch of kGdotBatch consecutive records. Every lane maps its own record's
// row id and searches the clamped grp_ptr for its group (group_find: the searches of a batch run side by
// side, not on the chain of dependent loads), then the wave walks the batch: v_readlane hands the local
// row and the group round and one rows_dot walk with q == 1 is made per record -- the same dot_batch calls
// and the same butterfly, so the bits are rows_dot's and depend on (type, cols) only, never on the batch
// width. Lane j keeps record j's answer and the batch is stored at once. A record whose row lies outside the
// partition (recorded under its index) or that no group covers (a malformed device grp_ptr only; not an
// error, as the grouped push skips it) answers +0 / 0 without a load; an empty group's vector is never read.
#ifndef GLINT_GDOT_BATCH
#define GLINT_GDOT_BATCH 4  // DESIGN.md has the sweep; any value in [1, 64] gives the same bits
#endif
constexpr int kGdotBatch = GLINT_GDOT_BATCH;
static_assert(kGdotBatch >= 1 && kGdotBatch <= 64, "a batch is handed round one wave");

template <typename V, bool VEC16, bool XW>
__device__ __forceinline__ void rows_gdot_body(const i64* __restrict__ rows, i64 n, const i64* __restrict__ grp_ptr,
                                               i64 g, const V* __restrict__ x, const V* __restrict__ data,
                                               const PartDesc& part, V* __restrict__ out, ErrState* err) {
  constexpr int E = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const u32 nstrips = (u32)((cols + 64 * E - 1) / (64 * E));
  const u64 total = ((u64)n + kGdotBatch - 1) / kGdotBatch;
  for (u64 w = w0; w < total; w += nw) {
    const i64 b = (i64)w * kGdotBatch;
    const u32 m = n - b < kGdotBatch ? (u32)(n - b) : (u32)kGdotBatch;
    // one record per lane: its local row (-1 = outside the partition) and its group (-1 = none)
    int32_t mine = -1, grp = -1;
    if ((u32)lane < m) {
      const int32_t l = g2l(part, rows[b + lane]);
      if (l >= 0 && l < part.size) mine = l;
      else record_error(err, b + lane);
      grp = group_find(grp_ptr, g, n, b + lane);
    }
    V res = V(0);
    for (u32 j = 0; j < m; ++j) {
      const int32_t l = __builtin_amdgcn_readlane(mine, (int)j);
      const int32_t k = __builtin_amdgcn_readlane(grp, (int)j);
      if (l < 0 || k < 0) continue;  // (wave-uniform)
      const V* row = data + (i64)l * part.pitch;
      const V* xq[1] = {x + (i64)k * cols};
      V acc[1] = {V(0)};
      u32 s = 0;
      for (; s + kDotDepth<1> <= nstrips; s += kDotDepth<1>)
        dot_batch<V, E, VEC16, false, XW, 1, true>(acc, row, xq, s, nstrips, lane, cols);
      if (s < nstrips) dot_batch<V, E, VEC16, false, XW, 1, false>(acc, row, xq, s, nstrips, lane, cols);
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) acc[0] = vadd(acc[0], __shfl_xor(acc[0], d, 64));  // rows_dot's butterfly
      if ((u32)lane == j) res = acc[0];
    }
    if ((u32)lane < m) out[b + lane] = res;  // lane j stores record b + j
  }
}

template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void rows_gdot_kernel(const i64* __restrict__ rows, i64 n,
                                                         const i64* __restrict__ grp_ptr, i64 g,
                                                         const V* __restrict__ x, int xwide,
                                                         const V* __restrict__ data, PartDesc part,
                                                         V* __restrict__ out, ErrState* err) {
  // x by 16 B or by element: the same loop either way, chosen once per launch (rows_dot_kernel's rule)
  if (VEC16 && xwide) rows_gdot_body<V, VEC16, true>(rows, n, grp_ptr, g, x, data, part, out, err);
  else rows_gdot_body<V, VEC16, false>(rows, n, grp_ptr, g, x, data, part, out, err);
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the grouped row-dot pull on st (no host synchronisation): one launch, no scratch. Every vector of
// x is 16-B aligned when x is and cols * sizeof(V) is a multiple of 16. Under the shard's lock.
template <typename V>
int pull_rows_gdot(glint_shard* s, const i64* rows, i64 n, const i64* grp_ptr, i64 g, const void* x, void* out,
                   hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0;
  const int xw = v16 && aligned(x, 16);
  const unsigned grid = grid_for((n + kGdotBatch - 1) / kGdotBatch, kTPB / 64, (i64)s->cus * 8);
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_DOT, v16 ? rows_gdot_kernel<V, true> : rows_gdot_kernel<V, false>, grid, kTPB,
                  st, rows, n, grp_ptr, g, (const V*)x, xw, (const V*)s->data, s->part, (V*)out, err_of(s)));
  return GLINT_OK;
}

template int pull_rows_gdot<int>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);
template int pull_rows_gdot<long long>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);
template int pull_rows_gdot<float>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);
template int pull_rows_gdot<double>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);

// Enqueues the row dot pull on st (no host synchronisation): one launch. x == nullptr is the self-dot
// (q == 1). Under the shard's lock.
template <typename V>
int pull_rows_dot(glint_shard* s, const i64* rows, i64 n, const void* x, i64 q, void* out, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0;
  const int xw = v16 && x && aligned(x, 16);
  const i64 tiles = q == 1 ? 1 : (q + kDotTile - 1) / kDotTile;
  const unsigned grid = grid_for(n * tiles, kTPB / 64, (i64)s->cus * 8);
  void (*k)(const i64*, i64, const V*, int, int, const V*, PartDesc, V*, ErrState*);
  if (!x) k = v16 ? rows_dot_kernel<V, true, true, 1> : rows_dot_kernel<V, false, true, 1>;
  else if (q == 1) k = v16 ? rows_dot_kernel<V, true, false, 1> : rows_dot_kernel<V, false, false, 1>;
  else k = v16 ? rows_dot_kernel<V, true, false, kDotTile> : rows_dot_kernel<V, false, false, kDotTile>;
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_DOT, k, grid, kTPB, st, rows, n, (const V*)x, (int)q, xw, (const V*)s->data,
                  s->part, (V*)out, err_of(s)));
  return GLINT_OK;
}

template int pull_rows_dot<int>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);
template int pull_rows_dot<long long>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);
template int pull_rows_dot<float>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);
template int pull_rows_dot<double>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);

}  // namespace glint
