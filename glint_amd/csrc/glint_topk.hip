// glint_topk.hip -- top-k row pull (glint_mat_pull_topk*, DESIGN.md "Top-k pull"): for each of q query
// vectors, the k rows of the shard whose dot with it ranks highest, as (global row, score) pairs.
//   topk_scores   one wave per (local row, tile of queries): the row dot pull's dot (glint_dot.h: the
//                 same lanes, order and butterfly, so the same bits) of every row of the shard, written
//                 query-major, score[j][local], into the shard's scratch.
//   topk_select   one workgroup per (query, tile of GLINT_TOPK_TILE candidates): (rank key, inverted
//                 local row) pairs in LDS, a bitonic network that sorts them descending, the best
//                 min(k, count) written out. Level 0 takes its candidates from the scores, a later
//                 level from the level before; the level with one tile per query writes the answer.
// The levels and every buffer's place come from glint_topk_plan.h. Kernel boundaries are the only order
// between workgroups: no flags, no look-back, no waiting inside a launch, no atomics. Pairs are distinct
// (rows are), so the sorted order -- and the answer -- is a function of the shard, x and k only.
#include "glint_dot.h"
#include "glint_host.h"
#include "glint_topk_plan.h"

namespace glint {

constexpr int kSelTPB = 1024;  // a tile is 4 pairs per thread; a network step 2 compare-exchanges per thread
constexpr u32 kSelTile = (u32)kTopkTile;
// compare-exchanges of a network step one wave takes: the tile's T / 2 over the workgroup's waves
constexpr u32 kSelWavePairs = kSelTile / 2 / (kSelTPB / 64);
static_assert(kSelWavePairs % 64 == 0 && (kSelWavePairs & (kSelWavePairs - 1)) == 0, "whole lanes, a power of two");

// ---- rank keys ------------------------------------------------------------------------------------
// An unsigned key whose order is the contract's rank. Float/Double: the sign-flip key (negative values
// complemented, the others with the sign bit set), after -0 -> +0 and NaN -> 0: the least key of a
// number is -inf's, 0x007FFFFF / 0x000F..F, so every NaN ranks below every number and all NaNs tie.
// Int/Long: the value with its sign bit flipped.
template <typename V> struct Rank;
template <> struct Rank<float> { typedef u32 K; };
template <> struct Rank<int> { typedef u32 K; };
template <> struct Rank<double> { typedef u64 K; };
template <> struct Rank<long long> { typedef u64 K; };

__device__ __forceinline__ u32 rank_key(float v) {
  u32 u = __float_as_uint(v);
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return 0u;
  if (u == 0x80000000u) u = 0u;
  return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ u64 rank_key(double v) {
  u64 u = (u64)__double_as_longlong(v);
  if ((u & 0x7FFFFFFFFFFFFFFFull) > 0x7FF0000000000000ull) return 0ull;
  if (u == 0x8000000000000000ull) u = 0ull;
  return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}
__device__ __forceinline__ u32 rank_key(int v) { return (u32)v ^ 0x80000000u; }
__device__ __forceinline__ u64 rank_key(long long v) { return (u64)v ^ 0x8000000000000000ull; }

// ---- scores ---------------------------------------------------------------------------------------
// rows_dot_kernel's frame (glint_rowdot.hip) with the row taken from the wave's index: persistent grid,
// one wave per (local row, tile of QT queries), the tiles of a row on adjacent waves. The last tile
// computes its missing queries as copies of the last one and stores only the real ones. Only `cols`
// elements of a row are read, never the pitch padding.
template <typename V, bool VEC16, bool XW, int QT>
__device__ __forceinline__ void topk_scores_body(const V* __restrict__ x, int q, const V* __restrict__ data,
                                                 const PartDesc& part, V* __restrict__ scores) {
  constexpr int E = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const i64 size = part.size;
  const u32 nstrips = (u32)((cols + 64 * E - 1) / (64 * E));
  const u32 ntiles = (u32)((q + QT - 1) / QT);
  const u64 total = (u64)size * ntiles;
  for (u64 w = w0; w < total; w += nw) {
    const i64 l = (i64)(w / ntiles);
    const int j0 = (int)(w % ntiles) * QT;
    V acc[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) acc[j] = V(0);
    const V* row = data + l * part.pitch;
    const V* xq[QT];
#pragma unroll
    for (int j = 0; j < QT; ++j) xq[j] = x + (i64)(j0 + j < q ? j0 + j : q - 1) * cols;
    u32 s = 0;
    for (; s + kDotDepth<QT> <= nstrips; s += kDotDepth<QT>)
      dot_batch<V, E, VEC16, false, XW, QT, true>(acc, row, xq, s, nstrips, lane, cols);
    if (s < nstrips) dot_batch<V, E, VEC16, false, XW, QT, false>(acc, row, xq, s, nstrips, lane, cols);
    // the xor butterfly: IEEE addition commutes, so every lane ends with the same bits
    V mine = acc[0];
#pragma unroll
    for (int j = 0; j < QT; ++j) {
#pragma unroll
      for (int d = 32; d >= 1; d >>= 1) acc[j] = vadd(acc[j], __shfl_xor(acc[j], d, 64));
      if (lane == j) mine = acc[j];
    }
    if (lane < QT && j0 + lane < q) scores[(i64)(j0 + lane) * size + l] = mine;  // lane j stores query j0 + j
  }
}

template <typename V, bool VEC16, int QT>
__global__ __launch_bounds__(kTPB) void topk_scores_kernel(const V* __restrict__ x, int q, int xwide,
                                                           const V* __restrict__ data, PartDesc part,
                                                           V* __restrict__ scores) {
  if (VEC16 && xwide) topk_scores_body<V, VEC16, true, QT>(x, q, data, part, scores);
  else topk_scores_body<V, VEC16, false, QT>(x, q, data, part, scores);
}

// ---- selection ------------------------------------------------------------------------------------
template <typename V>
struct TopkSel {
  typedef typename Rank<V>::K K;
  const V* scores;   // [q][size]
  i64 size;          // the shard's rows
  const K* in_key;   // [q][n_in], unused at level 0
  const u32* in_row;
  i64 n_in;          // candidates per query
  u32 tiles;         // workgroups per query
  K* out_key;        // [q][n_out], unused at the last level
  u32* out_row;
  i64 n_out;
  u32 k;
  int first, last;   // level 0 reads the scores; the last level writes the caller's arrays
  i64* out_rows;     // [q][k], the last level's
  V* out_vals;
  PartDesc part;
};

// Workgroup (tile, query): the pairs of its candidates, sorted descending by (key, ~row) -- rank
// descending, then row ascending, in one compare per word -- and the first min(k, count) emitted. A pad
// pair is (0, 0): below every real pair, whose inverted row is at least 2^31 (rows are below 2^31).
// Every count and every row read from memory is clamped before it indexes anything.
template <typename V>
__global__ __launch_bounds__(kSelTPB) void topk_select_kernel(TopkSel<V> a) {
  typedef typename Rank<V>::K K;
  __shared__ K skey[kSelTile];
  __shared__ u32 sirow[kSelTile];
  const u32 tid = threadIdx.x;
  const u32 tile = blockIdx.x % a.tiles;
  const i64 j = (i64)(blockIdx.x / a.tiles);
  const i64 base = (i64)tile * kSelTile;
  i64 left = a.n_in - base;
  if (left < 0) left = 0;
  const u32 cnt = left < (i64)kSelTile ? (u32)left : kSelTile;
  const i64 last_row = a.size > 0 ? a.size - 1 : 0;
  u32 P = 64;
  while (P < cnt) P <<= 1;  // <= kSelTile
  for (u32 i = tid; i < P; i += kSelTPB) {
    K key = 0;
    u32 irow = 0;
    if (i < cnt) {
      if (a.first) {  // candidate base + i is local row base + i
        key = rank_key(a.scores[j * a.size + base + i]);
        irow = ~(u32)(base + i);
      } else {
        key = a.in_key[j * a.n_in + base + i];
        u32 r = a.in_row[j * a.n_in + base + i];
        if ((i64)r > last_row) r = (u32)last_row;
        irow = ~r;
      }
    }
    skey[i] = key;
    sirow[i] = irow;
  }
  __syncthreads();
  // The bitonic network of glint_ordered.hip, descending. Wave w takes the compare-exchanges
  // [w * kSelWavePairs, (w + 1) * kSelWavePairs) of every step, two per lane. With a compare distance
  // jj <= kSelWavePairs those read and write only pairs [2 w kSelWavePairs, 2 (w + 1) kSelWavePairs):
  // the wave's own, which no other wave touches in such a step. A wave's LDS instructions execute in
  // order, so between two such steps a wave-scope fence (the compiler keeps the order) stands in for the
  // workgroup barrier; the barrier is needed only behind a step with a longer distance and in front of
  // one -- 15 of the 78 steps of a full tile -- and at the end.
  const u32 wave_first = (tid >> 6) * kSelWavePairs + (tid & 63);
  for (u32 kk = 2; kk <= P; kk <<= 1) {
    for (u32 jj = kk >> 1; jj > 0; jj >>= 1) {
#pragma unroll
      for (u32 r = 0; r < kSelWavePairs / 64; ++r) {
        const u32 t = wave_first + r * 64;
        if (t < P / 2) {
          const u32 i = ((t & ~(jj - 1)) << 1) | (t & (jj - 1));
          const u32 l = i + jj;
          const K xk = skey[i], yk = skey[l];
          const u32 xr = sirow[i], yr = sirow[l];
          const bool less = xk < yk || (xk == yk && xr < yr);
          if (less == ((i & kk) == 0)) {
            skey[i] = yk;
            skey[l] = xk;
            sirow[i] = yr;
            sirow[l] = xr;
          }
        }
      }
      const u32 next = jj > 1 ? jj >> 1 : kk;  // the next step's distance (past the last step: P)
      if (jj > kSelWavePairs || next > kSelWavePairs) {
        __syncthreads();
      } else {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
        __builtin_amdgcn_wave_barrier();
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
      }
    }
  }
  __syncthreads();  // the emit below reads other waves' pairs
  const u32 m = cnt < a.k ? cnt : a.k;
  if (!a.last) {
    // every tile in front of this one is full and emitted k: this one's pairs start at tile * k
    const i64 o = j * a.n_out + (i64)tile * a.k;
    for (u32 t = tid; t < m; t += kSelTPB) {
      if ((i64)tile * a.k + t < a.n_out) {
        a.out_key[o + t] = skey[t];
        a.out_row[o + t] = ~sirow[t];
      }
    }
  } else {
    for (u32 t = tid; t < a.k; t += kSelTPB) {
      i64 g = -1;
      V v = V(0);
      if (t < m) {
        i64 r = (i64)(~sirow[t]);
        if (r > last_row) r = last_row;
        g = a.part.kind == 0 ? a.part.start + r : (i64)a.part.cidx + r * (i64)a.part.cparts;
        v = a.scores[j * a.size + r];  // the score's own bits, not the key's
      }
      a.out_rows[j * (i64)a.k + t] = g;
      a.out_vals[j * (i64)a.k + t] = v;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the top-k pull on st (no host synchronisation): the scores launch and one launch per level,
// all counted under GLINT_K_PULL_ROWS_DOT. x, out_rows and out_vals are device pointers. Under the
// shard's lock; the scratch is s->d_det.
template <typename V>
int pull_topk(glint_shard* s, const void* x, i64 q, i64 k, i64* out_rows, void* out_vals, hipStream_t st) {
  typedef typename Rank<V>::K K;
  const TopkPlan p = topk_plan(s->part.size, q, k, (i64)sizeof(V));
  if (p.levels < 1) return GLINT_EINVAL;
  int rc = grow(&s->d_det, &s->det_bytes, (size_t)p.total_bytes);
  if (rc) return rc;
  char* base = (char*)s->d_det;
  V* scores = (V*)base;
  const i64 size = s->part.size;
  if (size > 0) {
    const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0;
    const int xw = v16 && aligned(x, 16);
    const i64 qtiles = q == 1 ? 1 : (q + kDotTile - 1) / kDotTile;
    const unsigned grid = grid_for(size * qtiles, kTPB / 64, (i64)s->cus * 8);
    void (*sk)(const V*, int, int, const V*, PartDesc, V*);
    if (q == 1) sk = v16 ? topk_scores_kernel<V, true, 1> : topk_scores_kernel<V, false, 1>;
    else sk = v16 ? topk_scores_kernel<V, true, kDotTile> : topk_scores_kernel<V, false, kDotTile>;
    HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_DOT, sk, grid, kTPB, st, (const V*)x, (int)q, xw, (const V*)s->data, s->part,
                    scores));
  }
  for (int l = 0; l < p.levels; ++l) {
    const TopkLevel& lv = p.level[l];
    TopkSel<V> a{};
    a.scores = scores;
    a.size = size;
    a.in_key = (const K*)(base + lv.in_key);
    a.in_row = (const u32*)(base + lv.in_row);
    a.n_in = lv.n_in;
    a.tiles = (u32)lv.tiles;
    a.out_key = (K*)(base + lv.out_key);
    a.out_row = (u32*)(base + lv.out_row);
    a.n_out = lv.n_out;
    a.k = (u32)k;
    a.first = l == 0;
    a.last = l == p.levels - 1;
    a.out_rows = out_rows;
    a.out_vals = (V*)out_vals;
    a.part = s->part;
    HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_DOT, topk_select_kernel<V>, (unsigned)(lv.tiles * q), kSelTPB, st, a));
  }
  return GLINT_OK;
}

template int pull_topk<int>(glint_shard*, const void*, i64, i64, i64*, void*, hipStream_t);
template int pull_topk<long long>(glint_shard*, const void*, i64, i64, i64*, void*, hipStream_t);
template int pull_topk<float>(glint_shard*, const void*, i64, i64, i64*, void*, hipStream_t);
template int pull_topk<double>(glint_shard*, const void*, i64, i64, i64*, void*, hipStream_t);

}  // namespace glint
