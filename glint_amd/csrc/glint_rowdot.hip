// glint_rowdot.hip -- row dot-product pull (glint_mat_pull_rows_dot*, DESIGN.md "Row dot pull"): the
// requested rows times vectors the caller sends, reduced over the columns next to the data, so a
// request of n rows and q vectors is answered with n x q values instead of n x cols.
//   rows_dot   one wave per (request, tile of queries): the wave walks the row in strips of 64 lanes x E
//              columns, every lane adds the products of its own columns in ascending column order, and
//              the 64 lane sums are combined by the xor butterfly.
// The floating-point order is the contract (include/glint_gpu.h): it depends on (type, cols) only, so the
// tile width, the grid and the alignment of x never show in the bits. No atomics, no split of a row.
#include "glint_device.h"
#include "glint_host.h"

namespace glint {

constexpr int kDotTile = GLINT_DOT_QUERY_TILE;  // queries per wave when q > 1 (one when q == 1)
// row-strip loads in flight per wave (kRowSumDepth's pattern): 8 for one query per wave; 2 for a tile of
// queries, whose vector strips take the registers (8 there is ~195 VGPRs, 2 waves/SIMD)
template <int QT> constexpr int kDotDepth = QT == 1 ? 8 : 2;

// acc + (a * b) with the product rounded before the add: hipcc contracts a * b + c into v_fma_* by
// default, and a fused product is not the contract's. Int/Long wrap.
__device__ __forceinline__ double dot_step(double acc, double a, double b) {
#pragma clang fp contract(off)
  const double p = a * b;
  return acc + p;
}
__device__ __forceinline__ float dot_step(float acc, float a, float b) {
#pragma clang fp contract(off)
  const float p = a * b;
  return acc + p;
}
__device__ __forceinline__ long long dot_step(long long acc, long long a, long long b) {
  return (long long)((u64)acc + (u64)a * (u64)b);
}
__device__ __forceinline__ int dot_step(int acc, int a, int b) { return (int)((u32)acc + (u32)a * (u32)b); }

// A lane's E columns [c, c + E) of one query vector: one 16-B load when XW (E * sizeof(V) == 16, the
// vector 16-B aligned), else element by element. Columns at or past cols are zeros.
template <typename V, int E, bool XW>
__device__ __forceinline__ void x_load(V (&t)[E], const V* __restrict__ xr, i64 c, i64 cols) {
  if (XW) {
    slice_load<V, E, true>(t, xr, c, cols);
  } else {
#pragma unroll
    for (int e = 0; e < E; ++e) t[e] = c + e < cols ? xr[c + e] : V(0);
  }
}

// D = kDotDepth<QT> strips of the row from strip s on (FULL: all of them exist), then their products added to
// the QT lane sums in ascending strip -- hence column -- order. The strip loads are independent; the
// adds are the only chain. A lane whose columns lie past cols multiplies zeros: acc + (+0) leaves acc
// as it is, since a sum that started from +0 is never -0.
template <typename V, int E, bool VEC16, bool SELF, bool XW, int QT, bool FULL>
__device__ __forceinline__ void dot_batch(V (&acc)[QT], const V* __restrict__ row, const V* const (&xq)[QT], u32 s,
                                          u32 nstrips, int lane, i64 cols) {
  constexpr int D = kDotDepth<QT>;
  V r[D][E];
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (FULL || s + d < nstrips) slice_load<V, E, VEC16>(r[d], row, ((i64)(s + d) * 64 + lane) * E, cols);
  }
#pragma unroll
  for (int d = 0; d < D; ++d) {
    if (FULL || s + d < nstrips) {
      const i64 c = ((i64)(s + d) * 64 + lane) * E;
#pragma unroll
      for (int j = 0; j < QT; ++j) {
        V t[E];
        if (SELF) {
#pragma unroll
          for (int e = 0; e < E; ++e) t[e] = r[d][e];
        } else {
          x_load<V, E, XW>(t, xq[j], c, cols);
        }
#pragma unroll
        for (int e = 0; e < E; ++e) acc[j] = dot_step(acc[j], r[d][e], t[e]);
      }
    }
  }
}

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

// ---- host side ----------------------------------------------------------------------------------
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
