// glint_rowdot_batch.hip -- batched row dot pull (glint_mat_pull_rows_dot_batch*, DESIGN.md "Batched row dot
// pull"): out[n x q] = table[rows] * x^T for rows the caller names -- a gather, with repeats, in the caller's
// order -- computed as the matrix product it is by gfx950's matrix instructions. One launch:
//   rows_dot_batch   one workgroup per (tile of 128 requests, pass of 64 vectors), the pass the fast grid
//                    index, so that the workgroups that gather the same 128 rows run together and all but
//                    the first find them in L2. K is not split; no atomics but the error record.
// A score is one element of the batched top-k pull's chain of matrix instructions (glint_topk_batch.hip):
// the same slabs of 128 B of K ascending, the same groups of 8 columns ascending within a slab, the same
// steps t ascending within a group, the column tail 0 * 0. Its bits depend on (type, cols, the row's values,
// the vector's values) only, and they are the bits that pull reports for the same (row, vector).
//
// The gather. Thread i < 128 of the workgroup maps request i of the tile to its local row (rows_dot's
// mapping) and leaves it in LDS: -1 for a request past n or a row outside the partition. A staging thread
// then reads the local rows of its four request lines once, before the slab loop. A line of -1 is dead:
// zero-filled by predicate, never loaded. The slab scheme is glint_slab.h's and the pipeline is the top-k
// kernel's: two slabs resident, the next slab's global loads issued into registers ahead of the current
// slab's matrix instructions and stored to LDS behind them, one barrier per slab.
//
// Operands. The answer is request-major, so the requests are the instruction's M (operand A) and the
// vectors its N (operand B) -- the transpose of the top-k kernel's assignment. Each accumulator element
// still takes the same products in the same K order (a product commutes), and a lane of the result holds
// one vector and several requests, so a store instruction writes runs of consecutive vectors of a request:
//   Float   v_mfma_f32_32x32x2_f32, two 32 x 32 accumulators (the wave's 32 requests x vectors
//           [32 b, 32 b + 32)): a half-wave stores 32 consecutive values of one request, 128 B of out.
//   Double  v_mfma_f64_16x16x4_f64, 2 x 4 accumulators of 16 x 16: 16 lanes store 16 consecutive values
//           of one request, 128 B of out.
// A request whose row lies outside the partition is stored as +0 and not as what the instructions made of
// its zero line (0 * inf is NaN). Stores are by element, predicated on the request and the vector.
#include "glint_device.h"  // record_error
#include "glint_host.h"
#include "glint_slab.h"  // the slab geometry and tb_chunk: shared with the batched top-k pull

namespace glint {

static_assert(kTbRows == GLINT_DOT_BATCH_ROWS, "the tile of the header is the slab's");
static_assert(GLINT_DOT_MAX_QUERIES % kTbPass == 0, "the largest call is a whole number of passes");

// The wave's accumulators, the matrix instructions of one slab and the store of the finished scores.
// `local` is the tile's 128 local rows (-1: answer +0), `i0` / `j0` the tile's first request and the
// pass's first vector.
template <typename V> struct DbMma;

template <> struct DbMma<float> {
  TbF16 acc[2];  // the wave's 32 requests x vectors [32 b, 32 b + 32)
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[b][v] = 0.f;
  }
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    const int l = lane & 31, kofs = (lane >> 5) * 16;
    const unsigned char* pa = buf + (32 * wave + l) * kTbLinePitch + kofs;
    const unsigned char* pb = buf + (kTbRows + l) * kTbLinePitch + kofs;
#pragma unroll
    for (int g = 0; g < kTbLineBytes / 32; ++g) {
      const TbF4 a = *reinterpret_cast<const TbF4*>(pa + g * 32);
      const TbF4 b0 = *reinterpret_cast<const TbF4*>(pb + g * 32);
      const TbF4 b1 = *reinterpret_cast<const TbF4*>(pb + 32 * kTbLinePitch + g * 32);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b0[t], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b1[t], acc[1], 0, 0, 0);
      }
    }
  }
  // register v of a lane: request 8 (v / 4) + 4 (lane / 32) + v % 4 of the wave's 32, vector lane % 32
  __device__ __forceinline__ void store(float* __restrict__ out, const int* local, i64 n, i64 i0, int q, int j0,
                                        int wave, int lane) const {
#pragma unroll
    for (int b = 0; b < 2; ++b) {
      const int j = j0 + 32 * b + (lane & 31);
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int r = 32 * wave + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (i0 + r < n && j < q) out[(i0 + r) * q + j] = local[r] < 0 ? 0.f : acc[b][v];
      }
    }
  }
};

template <> struct DbMma<double> {
  TbD4 acc[2][4];  // requests [16 m, 16 m + 16) of the wave's 32 x vectors [16 b, 16 b + 16)
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[m][b][v] = 0.0;
  }
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    const int l = lane & 15, kofs = (lane >> 4) * 16;
    const unsigned char* pa = buf + (32 * wave + l) * kTbLinePitch + kofs;
    const unsigned char* pb = buf + (kTbRows + l) * kTbLinePitch + kofs;
#pragma unroll
    for (int g = 0; g < kTbLineBytes / 64; ++g) {
      TbD2 a[2], b[4];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const TbD2*>(pa + 16 * m * kTbLinePitch + g * 64);
#pragma unroll
      for (int n = 0; n < 4; ++n) b[n] = *reinterpret_cast<const TbD2*>(pb + 16 * n * kTbLinePitch + g * 64);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][t], b[n][t], acc[m][n], 0, 0, 0);
    }
  }
  // register v of a lane: request 4 v + lane / 16 of the block of 16, vector lane % 16
  __device__ __forceinline__ void store(double* __restrict__ out, const int* local, i64 n, i64 i0, int q, int j0,
                                        int wave, int lane) const {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int r = 32 * wave + 16 * m + 4 * v + (lane >> 4);
        if (i0 + r >= n) continue;
        const bool zero = local[r] < 0;
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const int j = j0 + 16 * b + (lane & 15);
          if (j < q) out[(i0 + r) * q + j] = zero ? 0.0 : acc[m][b][v];
        }
      }
  }
};

// Workgroup b: requests [128 (b / npass), + 128) against vectors [64 (b % npass), + 64) of x.
// out[i * q + j] for every request i < n of the tile and every vector j < q of the pass.
template <typename V>
__global__ __launch_bounds__(kTPB) void rows_dot_batch_kernel(const i64* __restrict__ rows, i64 n,
                                                              const V* __restrict__ x, int q, int npass, int xwide,
                                                              const V* __restrict__ data, PartDesc part, int rwide,
                                                              V* __restrict__ out, ErrState* err) {
  constexpr int E = (int)(16 / sizeof(V));
  constexpr int KS = kTbLineBytes / (int)sizeof(V);  // columns of a slab
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][kTbSlabBytes];
  __shared__ int local[kTbRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const i64 cols = part.cols;
  const int pass = (int)(blockIdx.x % (unsigned)npass);
  const i64 i0 = (i64)(blockIdx.x / (unsigned)npass) * kTbRows;
  const int j0 = pass * kTbPass;
  // the gather's row ids, once per tile; the workgroup of pass 0 records a row outside the partition
  if (tid < kTbRows) {
    int32_t l = -1;
    if (i0 + tid < n) {
      l = g2l(part, rows[i0 + tid]);
      if (l < 0 || l >= part.size) {
        l = -1;
        if (pass == 0) record_error(err, i0 + tid);
      }
    }
    local[tid] = l;
  }
  __syncthreads();
  // staging: chunk `ch` of lines ln + 32 p; a dead line keeps a valid pointer and is never read
  const int ch = tid & 7, ln = tid >> 3;
  const V* src[kTbStage];
  bool live[kTbStage];
#pragma unroll
  for (int p = 0; p < kTbStage; ++p) {
    const int line = ln + 32 * p;
    if (line < kTbRows) {
      const int l = local[line];
      live[p] = l >= 0;
      src[p] = data + (i64)(live[p] ? l : 0) * part.pitch;
    } else {
      live[p] = j0 + line - kTbRows < q;
      src[p] = x + (i64)(live[p] ? j0 + line - kTbRows : 0) * cols;
    }
  }
  TbU4 stage[kTbStage];
  auto fetch = [&](i64 k0) {
#pragma unroll
    for (int p = 0; p < kTbStage; ++p)
      stage[p] = tb_chunk<V>(src[p], k0 + ch * E, cols, live[p], (32 * p < kTbRows ? rwide : xwide) != 0);
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int p = 0; p < kTbStage; ++p)
      *reinterpret_cast<TbU4*>(&lds[b][(ln + 32 * p) * kTbLinePitch + ch * 16]) = stage[p];
  };
  const int nslab = (int)((cols + KS - 1) / KS);
  DbMma<V> mma;
  mma.clear();
  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s < nslab; ++s) {
    const bool more = s + 1 < nslab;
    if (more) fetch((i64)(s + 1) * KS);
    mma.slab(lds[s & 1], wave, lane);
    // slab s + 1's buffer was last read in iteration s - 1, in front of that iteration's barrier
    if (more) stash((s + 1) & 1);
    __syncthreads();
  }
  mma.store(out, local, n, i0, q, j0, wave, lane);
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the batched row dot pull on st (no host synchronisation): one launch, no scratch, counted under
// GLINT_K_PULL_ROWS_DOT. rows, x and out are device pointers. Under the shard's lock.
template <typename V>
int pull_rows_dot_batch(glint_shard* s, const i64* rows, i64 n, const void* x, i64 q, void* out, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  const i64 cols = s->part.cols;
  const int xw = (cols * (i64)sizeof(V)) % 16 == 0 && aligned(x, 16);
  const int rw = (s->part.pitch * (i64)sizeof(V)) % 16 == 0 && aligned(s->data, 16);
  const i64 npass = (q + kTbPass - 1) / kTbPass;
  const unsigned grid = (unsigned)((n + kTbRows - 1) / kTbRows * npass);  // n < 2^31, npass <= 16
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_DOT, rows_dot_batch_kernel<V>, grid, kTPB, st, rows, n, (const V*)x, (int)q,
                  (int)npass, xw, (const V*)s->data, s->part, rw, (V*)out, err_of(s)));
  return GLINT_OK;
}

template int pull_rows_dot_batch<float>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);
template int pull_rows_dot_batch<double>(glint_shard*, const i64*, i64, const void*, i64, void*, hipStream_t);

}  // namespace glint
