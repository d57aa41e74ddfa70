// glint_rowmix_batch.hip -- batched row mix pull (glint_mat_pull_rows_mix_batch*, DESIGN.md "Batched row mix
// pull"): out[q x cols] = coef^T * table[rows], out[j][c] = sum over i of coef[i][j] * row_i[c], the gradient
// of the batched row dot pull's scores with respect to the caller's vectors. The product's K is the request
// list: both operands are K-major in memory, the rows are gathered along K, and K is split across
// workgroups. Two stages on the caller's stream:
//   rows_mix_batch   one workgroup per (tile of 64 vectors x 128 columns, chunk of L consecutive requests),
//                    the tile the fast grid index, so that the workgroups that gather the same chunk of rows
//                    run together and all but the first find them in L2. L is mix_chunk_len(n)
//                    (glint_mix_plan.h), a function of n only. A workgroup accumulates its chunk from zero
//                    accumulators, slabs ascending, and stores a 64 x 128 partial into P[chunk][q][cols];
//   mix_reduce       out = ((P0 + P1) + P2) + ..., chunks ascending, from P0 and not from zero.
// With one chunk the product stores straight to out and the reduce is not launched. No float atomics and no
// tickets: the kernel boundary is the only order between workgroups.
//
// Operands. The vectors j are the instruction's M (operand A is coef, element (j, i) at coef[i][j]), the
// columns its N (operand B is the gathered row i, element (i, c)). A slab is KS = 32 (Float) / 16 (Double)
// requests: KS lines of the tile's 64 coefficients and KS lines of its 128 columns, each loaded coalesced
// along the line (16 B per thread when the operand allows, else by element; zero past q or cols: tb_chunk)
// and stored K-major as it was loaded. A lane reads the element of its own (index, k) with one ds_read_b32 /
// ds_read_b64: there is no transpose pass. Both pitches are the line plus 8 elements, so that the lines one
// matrix instruction's lanes read together fall on disjoint banks (DESIGN.md has the arithmetic). Wave w owns
// columns [32 w, 32 w + 32) against all 64 vectors: Float two 32 x 32 accumulators of v_mfma_f32_32x32x2_f32,
// Double 4 x 2 of 16 x 16 of v_mfma_f64_16x16x4_f64. A lane of the result holds one column and several
// vectors, so a store instruction writes 128-byte runs of one answer row.
//
// Pipeline. Two slabs resident; the next slab's global loads are issued into registers ahead of the current
// slab's matrix instructions and stored to LDS behind them, one barrier per slab. The gather's ids run one
// slab further ahead: while slab s + 1 is fetched, threads < KS map the requests of slab s + 2 to local rows
// (rows_dot's mapping) and leave them in LDS behind the instructions, so no row load waits on an id load. A
// request past the chunk or whose row lies outside the partition is dead (-1): its row line and its
// coefficient line are zero-filled by predicate and never loaded, and it contributes 0 * 0 whatever coef
// holds for it. The workgroups of tile 0 record the rows outside the partition.
#include "glint_device.h"  // record_error, vadd
#include "glint_host.h"
#include "glint_mix_plan.h"
#include "glint_slab.h"  // tb_chunk and the vector types

namespace glint {

static_assert(GLINT_MIX_BATCH_MAX_VECTORS == GLINT_DOT_MAX_QUERIES, "the third product takes the pull's batch");

constexpr int kMixVecs = 64;   // vectors of a tile: the instruction's M
constexpr int kMixCols = 128;  // columns of a tile: its N, 32 per wave
static_assert(kMixCols == 32 * (kTPB / 64), "a wave owns 32 columns of the tile");
static_assert(GLINT_MIX_BATCH_MAX_VECTORS % kMixVecs == 0, "the largest call is a whole number of tiles");

// The geometry of a slab in LDS: KS coefficient lines, then KS row lines.
template <typename V> struct Mx {
  static constexpr int KS = kTbLineBytes / (int)sizeof(V);                // requests of a slab
  static constexpr int kCoefPitch = (kMixVecs + 8) * (int)sizeof(V);      // 288 B Float, 576 B Double
  static constexpr int kRowPitch = (kMixCols + 8) * (int)sizeof(V);       // 544 B Float, 1088 B Double
  static constexpr int kRowBase = KS * kCoefPitch;                        // behind the coefficient lines
  static constexpr int kSlabBytes = KS * (kCoefPitch + kRowPitch);        // 26 624 B either type
  static constexpr int kCoefChunks = kMixVecs * (int)sizeof(V) / 16;      // 16-B chunks of a line
  static constexpr int kRowChunks = kMixCols * (int)sizeof(V) / 16;
  static constexpr int kCoefTrip = kTPB / kCoefChunks;                    // lines the workgroup stages at once
  static constexpr int kRowTrip = kTPB / kRowChunks;
  static constexpr int kCoefStage = KS / kCoefTrip;                       // chunks a thread stages per slab
  static constexpr int kRowStage = KS / kRowTrip;
  static_assert(kCoefStage == 2 && kRowStage == 4, "six 16-B chunks per thread per slab");
  static_assert(kCoefPitch % 16 == 0 && kRowPitch % 16 == 0 && KS % 8 == 0, "aligned chunks, whole groups of 8");
};

// The wave's accumulators, the matrix instructions of one slab and the store of the finished tile.
// dst is q x cols; j0 / c0 the tile's first vector and column.
template <typename V> struct MxMma;

template <> struct MxMma<float> {
  TbF16 acc[2];  // vectors [32 m, 32 m + 32) x the wave's 32 columns
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[m][v] = 0.f;
  }
  // step (g, t): requests 8 g + t (lanes 0-31) and 8 g + 4 + t (lanes 32-63) of the slab
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    typedef Mx<float> G;
    const int l = lane & 31, h = lane >> 5;
    const unsigned char* pa = buf + 4 * h * G::kCoefPitch + l * 4;
    const unsigned char* pb = buf + G::kRowBase + 4 * h * G::kRowPitch + (32 * wave + l) * 4;
#pragma unroll
    for (int g = 0; g < G::KS / 8; ++g)
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const int k = 8 * g + t;
        const float a0 = *reinterpret_cast<const float*>(pa + k * G::kCoefPitch);
        const float a1 = *reinterpret_cast<const float*>(pa + k * G::kCoefPitch + 128);
        const float b = *reinterpret_cast<const float*>(pb + k * G::kRowPitch);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0, b, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1, b, acc[1], 0, 0, 0);
      }
  }
  // register v of a lane: vector 8 (v / 4) + 4 (lane / 32) + v % 4 of the block of 32, column lane % 32
  __device__ __forceinline__ void store(float* __restrict__ dst, int q, int j0, i64 cols, i64 c0, int wave,
                                        int lane) const {
    const i64 c = c0 + 32 * wave + (lane & 31);
    if (c >= cols) return;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int j = j0 + 32 * m + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (j < q) dst[(i64)j * cols + c] = acc[m][v];
      }
  }
};

template <> struct MxMma<double> {
  TbD4 acc[4][2];  // vectors [16 m, 16 m + 16) x columns [16 b, 16 b + 16) of the wave's 32
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[m][b][v] = 0.0;
  }
  // step (g, t): request 8 g + 2 (lane / 16) + t of the slab
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    typedef Mx<double> G;
    const int l = lane & 15, kq = lane >> 4;
    const unsigned char* pa = buf + 2 * kq * G::kCoefPitch + l * 8;
    const unsigned char* pb = buf + G::kRowBase + 2 * kq * G::kRowPitch + (32 * wave + l) * 8;
#pragma unroll
    for (int g = 0; g < G::KS / 8; ++g)
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        const int k = 8 * g + t;
        double a[4], b[2];
#pragma unroll
        for (int m = 0; m < 4; ++m) a[m] = *reinterpret_cast<const double*>(pa + k * G::kCoefPitch + 128 * m);
#pragma unroll
        for (int n = 0; n < 2; ++n) b[n] = *reinterpret_cast<const double*>(pb + k * G::kRowPitch + 128 * n);
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m], b[n], acc[m][n], 0, 0, 0);
      }
  }
  // register v of a lane: vector 4 v + lane / 16 of the block of 16, column lane % 16
  __device__ __forceinline__ void store(double* __restrict__ dst, int q, int j0, i64 cols, i64 c0, int wave,
                                        int lane) const {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int j = j0 + 16 * m + 4 * v + (lane >> 4);
        if (j >= q) continue;
#pragma unroll
        for (int b = 0; b < 2; ++b) {
          const i64 c = c0 + 32 * wave + 16 * b + (lane & 15);
          if (c < cols) dst[(i64)j * cols + c] = acc[m][b][v];
        }
      }
  }
};

// Workgroup b: tile b % ntiles -- vectors [64 (tile % nq), + 64) x columns [128 (tile / nq), + 128) -- over
// chunk b / ntiles, requests [chunk * len, min(n, (chunk + 1) * len)). It writes its partial at
// dst + chunk * q * cols (dst is `out` itself when the call has one chunk).
template <typename V>
__global__ __launch_bounds__(kTPB) void rows_mix_batch_kernel(const i64* __restrict__ rows, i64 n, i64 len,
                                                              const V* __restrict__ coef, int q, int nq, int ntiles,
                                                              int cwide, const V* __restrict__ data, PartDesc part,
                                                              int rwide, V* __restrict__ dst, ErrState* err) {
  constexpr int E = (int)(16 / sizeof(V));
  typedef Mx<V> G;
  constexpr int KS = G::KS;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][G::kSlabBytes];
  __shared__ int ids[2][KS];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const i64 cols = part.cols;
  const int tile = (int)(blockIdx.x % (unsigned)ntiles);
  const i64 chunk = (i64)(blockIdx.x / (unsigned)ntiles);
  const int j0 = (tile % nq) * kMixVecs;
  const i64 c0 = (i64)(tile / nq) * kMixCols;
  const i64 i0 = chunk * len;
  const i64 i1 = i0 + len < n ? i0 + len : n;
  const int nslab = (int)((i1 - i0 + KS - 1) / KS);
  // request tid of slab s as a local row; -1 past the chunk or outside the partition (tile 0 records it)
  auto resolve = [&](int s) -> int {
    const i64 i = i0 + (i64)s * KS + tid;
    if (i >= i1) return -1;
    const int32_t l = g2l(part, rows[i]);
    if (l >= 0 && l < part.size) return l;
    if (tile == 0) record_error(err, i);
    return -1;
  };
  // staging: chunk `cch` of coefficient lines cln + kCoefTrip p, chunk `rch` of row lines rln + kRowTrip p
  const int cch = tid % G::kCoefChunks, cln = tid / G::kCoefChunks;
  const int rch = tid % G::kRowChunks, rln = tid / G::kRowChunks;
  TbU4 sc[G::kCoefStage], sr[G::kRowStage];
  auto fetch = [&](int s) {
    const i64 k0 = i0 + (i64)s * KS;
    const int* id = ids[s & 1];
#pragma unroll
    for (int p = 0; p < G::kCoefStage; ++p) {
      const int line = cln + G::kCoefTrip * p;
      const bool live = id[line] >= 0;
      sc[p] = tb_chunk<V>(coef + (live ? k0 + line : 0) * q, j0 + cch * E, q, live, cwide != 0);
    }
#pragma unroll
    for (int p = 0; p < G::kRowStage; ++p) {
      const int l = id[rln + G::kRowTrip * p];
      sr[p] = tb_chunk<V>(data + (i64)(l >= 0 ? l : 0) * part.pitch, c0 + rch * E, cols, l >= 0, rwide != 0);
    }
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int p = 0; p < G::kCoefStage; ++p)
      *reinterpret_cast<TbU4*>(&lds[b][(cln + G::kCoefTrip * p) * G::kCoefPitch + cch * 16]) = sc[p];
#pragma unroll
    for (int p = 0; p < G::kRowStage; ++p)
      *reinterpret_cast<TbU4*>(&lds[b][G::kRowBase + (rln + G::kRowTrip * p) * G::kRowPitch + rch * 16]) = sr[p];
  };
  if (tid < KS) {
    ids[0][tid] = resolve(0);
    ids[1][tid] = resolve(1);
  }
  __syncthreads();
  MxMma<V> mma;
  mma.clear();
  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const bool more = s + 1 < nslab;
    if (more) fetch(s + 1);
    int next = -1;
    if (tid < KS) next = resolve(s + 2);
    mma.slab(lds[s & 1], wave, lane);
    // slab s + 1's buffer and slab s's ids were last read in iteration s - 1, in front of its barrier
    if (more) stash((s + 1) & 1);
    if (tid < KS) ids[s & 1][tid] = next;
    __syncthreads();
  }
  mma.store(dst + chunk * (i64)q * cols, q, j0, cols, c0, wave, lane);
}

// out[e] = ((P0[e] + P1[e]) + P2[e]) + ... over the nchunks partials of `total` elements each; nchunks == 0
// writes +0 (the answer of an empty call). A unit is 16 B when VEC16 (every partial and out 16-B aligned),
// else one element.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void mix_reduce_kernel(const V* __restrict__ part, i64 total, int nchunks,
                                                          V* __restrict__ out) {
  constexpr int E = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const i64 units = total / E;
  for (i64 u = (i64)blockIdx.x * kTPB + threadIdx.x; u < units; u += (i64)gridDim.x * kTPB) {
    V acc[E];
#pragma unroll
    for (int k = 0; k < E; ++k) acc[k] = V(0);
    for (int p = 0; p < nchunks; ++p) {
      V t[E];
      if (VEC16) {
        const TbU4 w = *reinterpret_cast<const TbU4*>(part + (i64)p * total + u * E);
        __builtin_memcpy(t, &w, 16);
      } else {
        t[0] = part[(i64)p * total + u];
      }
#pragma unroll
      for (int k = 0; k < E; ++k) acc[k] = p == 0 ? t[k] : vadd(acc[k], t[k]);
    }
    if (VEC16) {
      TbU4 w;
      __builtin_memcpy(&w, acc, 16);
      *reinterpret_cast<TbU4*>(out + u * E) = w;
    } else {
      out[u] = acc[0];
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the batched row mix pull on st (no host synchronisation): the product and, with more than one
// chunk, the reduce, both counted under GLINT_K_PULL_ROWS_SUM (the call is a dense weighted row sum). rows,
// coef and out are device pointers. The partials lie at the front of s->d_det, [chunk][q][cols]; the scratch
// is grown before anything is launched. n == 0 launches the reduce over no partials: q x cols zeros. Under
// the shard's lock.
template <typename V>
int pull_rows_mix_batch(glint_shard* s, const i64* rows, i64 n, const void* coef, i64 q, void* out, hipStream_t st) {
  const i64 cols = s->part.cols;
  const i64 total = q * cols;  // q <= 1024, cols < 2^31
  const i64 nchunks = mix_chunk_count(n);
  V* part = (V*)out;
  if (nchunks > 1) {
    if (int rc = grow(&s->d_det, &s->det_bytes, (size_t)nchunks * (size_t)total * sizeof(V))) return rc;
    part = (V*)s->d_det;
  }
  if (nchunks > 0) {
    const i64 nq = (q + kMixVecs - 1) / kMixVecs;
    const i64 ntiles = nq * ((cols + kMixCols - 1) / kMixCols);
    if (ntiles * nchunks >= ((i64)1 << 31)) return GLINT_EINVAL;
    const int cw = (q * (i64)sizeof(V)) % 16 == 0 && aligned(coef, 16);
    const int rw = (s->part.pitch * (i64)sizeof(V)) % 16 == 0 && aligned(s->data, 16);
    HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SUM, rows_mix_batch_kernel<V>, (unsigned)(ntiles * nchunks), kTPB, st, rows,
                    n, mix_chunk_len(n), (const V*)coef, (int)q, (int)nq, (int)ntiles, cw, (const V*)s->data, s->part,
                    rw, part, err_of(s)));
    if (nchunks == 1) return GLINT_OK;
  }
  const bool v16 = (total * (i64)sizeof(V)) % 16 == 0 && aligned(out, 16) && aligned(part, 16);
  const unsigned gs = grid_for(v16 ? total / (i64)(16 / sizeof(V)) : total, kTPB, (i64)s->cus * 16);
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SUM, v16 ? mix_reduce_kernel<V, true> : mix_reduce_kernel<V, false>, gs, kTPB,
                  st, (const V*)part, total, (int)nchunks, (V*)out));
  return GLINT_OK;
}

template int pull_rows_mix_batch<float>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);
template int pull_rows_mix_batch<double>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);

}  // namespace glint
