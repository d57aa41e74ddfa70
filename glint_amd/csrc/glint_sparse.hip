// glint_sparse.hip -- sparse row pull (glint_mat_pull_rows_sparse*, DESIGN.md "Sparse row pull"): the
// non-zero elements of the requested rows as a CSR triple (row_ptr, cols, values), compacted next to
// the data so that a host pull moves the non-zeros over the link, not n x cols values.
//   sparse_count   one wave per requested row: the number of elements with v != 0 (-0.0 is not, NaN
//                  is), written as int64 into row_ptr[i]; a row outside the partition counts 0 and is
//                  recorded as an error; row_ptr[n] = 0;
//   scan           exclusive prefix over the n + 1 counts, in place, by reduce-then-scan over separate
//                  launches: tile totals, the scan of the totals (the same procedure, one level up),
//                  then the scan of each tile from its total's prefix. No workgroup ever waits for
//                  another inside a launch -- kernel boundaries are the only cross-workgroup order;
//   sparse_emit    one wave per requested row walks it in column order in strips; a lane's position is
//                  row_ptr[i] + the entries of the strips before + the entries of the lanes before it
//                  in the strip (64-bit ballots) + the entries before in the lane itself. Stores are
//                  guarded by pos < cap. No atomic decides a position: the answer is deterministic.
#include "glint_device.h"
#include "glint_host.h"

namespace glint {

constexpr int kScanTile = GLINT_SPARSE_SCAN_TILE;  // counts one scan workgroup covers
constexpr int kScanItems = kScanTile / kTPB;       // counts per thread
static_assert(kScanItems * kTPB == kScanTile, "a scan tile is a whole number of counts per thread");

typedef __attribute__((ext_vector_type(4))) unsigned int SparseU4;

// A lane's part of a strip of a row. WIDE: VPL consecutive columns from c (one 16-B load; VPL *
// sizeof(V) == 16, cols a multiple of VPL, every row 16-B aligned); else (VPL == 1) the column c.
// Columns from `cols` on -- the pitch padding among them -- are never read and count as zero.
template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void strip_load(V (&x)[VPL], const V* __restrict__ row, i64 c, i64 cols) {
  if (WIDE) {
    SparseU4 q = {0u, 0u, 0u, 0u};
    if (c < cols) q = *reinterpret_cast<const SparseU4*>(row + c);
    __builtin_memcpy(x, &q, 16);
  } else {
    x[0] = c < cols ? row[c] : V(0);
  }
}

// number of set bits of m below this lane's
__device__ __forceinline__ u32 lanes_before(u64 m) {
  return __builtin_amdgcn_mbcnt_hi((u32)(m >> 32), __builtin_amdgcn_mbcnt_lo((u32)m, 0u));
}

// Persistent grid, one wave per requested row (the layout of mat_pull_rows_kernel).
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void sparse_count_kernel(const i64* __restrict__ rows, i64 n,
                                                            const V* __restrict__ data, PartDesc part,
                                                            i64* __restrict__ row_ptr, ErrState* err) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  const i64 w0 = (i64)blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6);
  const i64 nw = (i64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  if (blockIdx.x == 0 && threadIdx.x == 0) row_ptr[n] = 0;  // the scan turns it into the total
  for (i64 i = w0; i < n; i += nw) {
    const int32_t l = g2l(part, rows[i]);
    const bool ok = l >= 0 && l < part.size;
    if (!ok && lane == 0) record_error(err, i);
    u32 cnt = 0;
    if (ok) {
      const V* row = data + (i64)l * part.pitch;
#pragma unroll 4
      for (i64 c0 = 0; c0 < cols; c0 += 64 * VPL) {
        V x[VPL];
        strip_load<V, VPL, VEC16>(x, row, c0 + (i64)lane * VPL, cols);
#pragma unroll
        for (int k = 0; k < VPL; ++k) cnt += x[k] != V(0) ? 1u : 0u;
      }
    }
#pragma unroll
    for (int d = 32; d > 0; d >>= 1) cnt += (u32)__shfl_xor((int)cnt, d, 64);
    if (lane == 0) row_ptr[i] = (i64)cnt;
  }
}

// block-wide sum of one value per thread; every thread gets it
__device__ __forceinline__ i64 block_sum(i64 v, i64* lds) {
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  i64 t = 0;
#pragma unroll
  for (int w = 0; w < kTPB / 64; ++w) t += lds[w];
  __syncthreads();
  return t;
}

// tot[b] = sum of tile b of x[0..m)
__global__ __launch_bounds__(kTPB) void scan_totals_kernel(const i64* __restrict__ x, i64 m, i64* __restrict__ tot) {
  __shared__ i64 lds[kTPB / 64];
  const i64 base = (i64)blockIdx.x * kScanTile + (i64)threadIdx.x * kScanItems;
  i64 v = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) v += base + k < m ? x[base + k] : 0;
  v = block_sum(v, lds);
  if (threadIdx.x == 0) tot[blockIdx.x] = v;
}

// x[i] = tile_base + (sum of the tile's elements before i), in place; tile_base = base[b] -- the
// exclusive prefix of the tile totals, already scanned -- or 0 for a single tile (base == nullptr).
__global__ __launch_bounds__(kTPB) void scan_tiles_kernel(i64* x, i64 m, const i64* __restrict__ base) {
  __shared__ i64 lds[kTPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 at = (i64)blockIdx.x * kScanTile + (i64)threadIdx.x * kScanItems;
  i64 v[kScanItems];
  i64 mine = 0;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    v[k] = at + k < m ? x[at + k] : 0;
    mine += v[k];
  }
  i64 inc = mine;  // inclusive prefix over the wave's lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const i64 o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  i64 run = base ? base[blockIdx.x] : 0;
  for (int w = 0; w < wave; ++w) run += lds[w];
  run += inc - mine;
#pragma unroll
  for (int k = 0; k < kScanItems; ++k) {
    if (at + k < m) x[at + k] = run;
    run += v[k];
  }
}

// Persistent grid, one wave per requested row. Entry j of request i goes to row_ptr[i] + j, columns
// ascending: strips in column order; inside a strip lane-major, then (16-B path) within the lane.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void sparse_emit_kernel(const i64* __restrict__ rows, i64 n,
                                                           const V* __restrict__ data, PartDesc part,
                                                           const i64* __restrict__ row_ptr,
                                                           int32_t* __restrict__ out_cols, V* __restrict__ out_vals,
                                                           i64 cap) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  const i64 w0 = (i64)blockIdx.x * (kTPB / 64) + (threadIdx.x >> 6);
  const i64 nw = (i64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  for (i64 i = w0; i < n; i += nw) {
    i64 pos0 = row_ptr[i];  // wave-uniform running base
    const i64 end = row_ptr[i + 1];
    // nothing to store: an empty row (a row outside the partition counted 0) or one wholly past cap
    if (end == pos0 || pos0 >= cap) continue;
    const int32_t l = g2l(part, rows[i]);
    if (l < 0 || l >= part.size) continue;
    const V* row = data + (i64)l * part.pitch;
    for (i64 c0 = 0; c0 < cols && pos0 < cap && pos0 < end; c0 += 64 * VPL) {
      const i64 c = c0 + (i64)lane * VPL;
      V x[VPL];
      strip_load<V, VPL, VEC16>(x, row, c, cols);
      u32 before = 0, total = 0;  // entries of the lanes before this one; of the whole strip
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        const u64 m = __ballot(x[k] != V(0));
        before += lanes_before(m);
        total += (u32)__popcll(m);
      }
      i64 pos = pos0 + (i64)before;
#pragma unroll
      for (int k = 0; k < VPL; ++k) {
        if (x[k] != V(0)) {
          if (pos < cap) {
            out_cols[pos] = (int32_t)(c + k);
            out_vals[pos] = x[k];
          }
          ++pos;
        }
      }
      pos0 += (i64)total;
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
namespace {

// exclusive prefix of x[0..m) in place; scratch holds the tile totals of this level and of the levels
// above it (sparse_scan_scratch words in all)
int scan_exclusive(glint_shard* s, i64* x, i64 m, i64* scratch, hipStream_t st) {
  const i64 tiles = (m + kScanTile - 1) / kScanTile;
  if (tiles <= 1) {
    HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SPARSE, scan_tiles_kernel, 1u, kTPB, st, x, m, (const i64*)nullptr));
    return GLINT_OK;
  }
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SPARSE, scan_totals_kernel, (unsigned)tiles, kTPB, st, (const i64*)x, m,
                  scratch));
  if (int rc = scan_exclusive(s, scratch, tiles, scratch + tiles, st)) return rc;
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SPARSE, scan_tiles_kernel, (unsigned)tiles, kTPB, st, x, m,
                  (const i64*)scratch));
  return GLINT_OK;
}

inline size_t sparse_scan_scratch(i64 m) {
  size_t words = 0;
  for (i64 t = (m + kScanTile - 1) / kScanTile; t > 1; t = (t + kScanTile - 1) / kScanTile) words += (size_t)t;
  return words;
}

}  // namespace

template <typename V>
int sparse_count_scan(glint_shard* s, const i64* rows, i64 n, i64* row_ptr, hipStream_t st) {
  const size_t words = sparse_scan_scratch(n + 1);
  if (int rc = grow(&s->d_det, &s->det_bytes, words * sizeof(i64))) return rc;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0;
  const unsigned g = grid_for(n, kTPB / 64, (i64)s->cus * 8);
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SPARSE, v16 ? sparse_count_kernel<V, true> : sparse_count_kernel<V, false>, g,
                  kTPB, st, rows, n, (const V*)s->data, s->part, row_ptr, err_of(s)));
  return scan_exclusive(s, row_ptr, n + 1, (i64*)s->d_det, st);
}

template <typename V>
int sparse_emit(glint_shard* s, const i64* rows, i64 n, const i64* row_ptr, int32_t* out_cols, void* out_vals,
                i64 cap, hipStream_t st) {
  if (n <= 0 || cap <= 0) return GLINT_OK;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0;
  const unsigned g = grid_for(n, kTPB / 64, (i64)s->cus * 8);
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SPARSE, v16 ? sparse_emit_kernel<V, true> : sparse_emit_kernel<V, false>, g,
                  kTPB, st, rows, n, (const V*)s->data, s->part, row_ptr, out_cols, (V*)out_vals, cap));
  return GLINT_OK;
}

#define GLINT_SPARSE_INST(V)                                                                   \
  template int sparse_count_scan<V>(glint_shard*, const i64*, i64, i64*, hipStream_t);         \
  template int sparse_emit<V>(glint_shard*, const i64*, i64, const i64*, int32_t*, void*, i64, hipStream_t);
GLINT_SPARSE_INST(int)
GLINT_SPARSE_INST(long long)
GLINT_SPARSE_INST(float)
GLINT_SPARSE_INST(double)
#undef GLINT_SPARSE_INST

}  // namespace glint
