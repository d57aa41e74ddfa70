// glint_topk_batch.hip -- batched top-k row pull (glint_mat_pull_topk_batch*, DESIGN.md "Batched top-k
// pull"): glint_mat_pull_topk's answer for up to GLINT_TOPK_BATCH_MAX_QUERIES query vectors, with the
// scores computed as the matrix product they are, scores[q x size] = x * table^T, by gfx950's matrix
// instructions. The queries are taken in passes of 64; a pass is
//   topk_batch_scores   one workgroup per tile of 128 rows, against the pass's 64 queries (the missing
//                       queries of the last pass are zeros and are not stored): the score of every
//                       (query, row), written query-major, score[j][local], into the shard's scratch;
//   topk_select         the selection levels of glint_topk.hip, unchanged, over those scores.
// Kernel boundaries are the only order between workgroups; no atomics. A score is one element of a chain
// of matrix instructions over ascending columns, so its bits depend on (type, cols, the row's values,
// the query's values) only: not on the tile, the wave, the lane, the pass, q or k.
//
// The product. Both operands are contiguous along cols, the product's K, while a lane of a matrix
// operand wants one element at (line lane % L, column k0 + lane / L), so both go through LDS. A slab is
// 128 bytes of K (32 Float / 16 Double columns) of the tile's 128 rows and of the 64 queries: 192 lines
// of 128 B, each at a pitch of 144 B. Thread t stages 16-B chunk t % 8 of lines t / 8 + 32 p, p = 0..5:
// eight lanes read one line's 128 B from global memory, and one 16-B LDS store lands them. A 16-lane
// group of a 16-B LDS read takes lines l .. l + 15 at one column: 36 l words apart, 16 distinct groups
// of four banks -- no conflict. Two slabs are resident: the next slab's global loads are issued into
// registers before the current slab's matrix instructions and stored to LDS behind them, with one
// barrier per slab. The column tail, the rows past `size` and the queries past the pass are zero-filled
// by predicate in the staging and never read; a partial 16-B chunk is read element by element, so only
// `cols` elements of a row are read.
//
// Wave w owns rows [32 w, 32 w + 32) of the tile against all 64 queries. The queries are the
// instruction's M (operand A), the rows its N (operand B): a lane of the result holds one row and
// several queries, so a store instruction writes runs of consecutive rows of one query.
//   Float   v_mfma_f32_32x32x2_f32, two 32 x 32 accumulators (32 registers). A lane reads four
//           consecutive columns, k0 + 8 g + 4 (lane / 32) + t, of its line by one 16-B LDS read, and
//           instruction t = 0..3 of group g takes element t: it adds the products of columns
//           k0 + 8 g + t and k0 + 8 g + 4 + t to the accumulator.
//   Double  v_mfma_f64_16x16x4_f64, 4 x 2 accumulators of 16 x 16 (64 registers). A lane reads two
//           consecutive columns, k0 + 8 g + 2 (lane / 16) + t, and instruction t = 0..1 of group g adds
//           the products of columns k0 + 8 g + {0, 2, 4, 6} + t.
// Groups ascend within a slab and slabs ascend over cols; the columns from cols up to the next multiple
// of the slab contribute 0 * 0. That chain is the accumulation order of the contract.
#include "glint_host.h"
#include "glint_slab.h"  // the slab geometry and tb_chunk: shared with the batched row dot pull
#include "glint_topk_plan.h"

namespace glint {

static_assert(kTbRows == GLINT_TOPK_BATCH_ROWS, "the tile of the header is the slab's");
static_assert(kTbPass == GLINT_TOPK_MAX_QUERIES, "a pass is selected by a topk_plan of at most its queries");

// The wave's accumulators, the matrix instructions of one slab and the store of the finished scores.
template <typename V> struct TbMma;

template <> struct TbMma<float> {
  TbF16 acc[2];  // queries [32 m, 32 m + 32) x the wave's 32 rows
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[m][v] = 0.f;
  }
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    const int l = lane & 31, kofs = (lane >> 5) * 16;
    const unsigned char* pb = buf + (32 * wave + l) * kTbLinePitch + kofs;
    const unsigned char* pa = buf + (kTbRows + l) * kTbLinePitch + kofs;
#pragma unroll
    for (int g = 0; g < kTbLineBytes / 32; ++g) {
      const TbF4 b = *reinterpret_cast<const TbF4*>(pb + g * 32);
      const TbF4 a0 = *reinterpret_cast<const TbF4*>(pa + g * 32);
      const TbF4 a1 = *reinterpret_cast<const TbF4*>(pa + 32 * kTbLinePitch + g * 32);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a0[t], b[t], acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a1[t], b[t], acc[1], 0, 0, 0);
      }
    }
  }
  // register v of a lane: query 8 (v / 4) + 4 (lane / 32) + v % 4 of the block, row lane % 32
  __device__ __forceinline__ void store(float* __restrict__ scores, i64 size, i64 row0, int qp, int wave, int lane) const {
    const i64 row = row0 + 32 * wave + (lane & 31);
    if (row >= size) return;
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int v = 0; v < 16; ++v) {
        const int j = 32 * m + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
        if (j < qp) scores[(i64)j * size + row] = acc[m][v];
      }
  }
};

template <> struct TbMma<double> {
  TbD4 acc[4][2];  // queries [16 m, 16 m + 16) x rows [16 n, 16 n + 16) of the wave's 32
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < 4; ++m)
#pragma unroll
      for (int n = 0; n < 2; ++n)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[m][n][v] = 0.0;
  }
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    const int l = lane & 15, kofs = (lane >> 4) * 16;
    const unsigned char* pb = buf + (32 * wave + l) * kTbLinePitch + kofs;
    const unsigned char* pa = buf + (kTbRows + l) * kTbLinePitch + kofs;
#pragma unroll
    for (int g = 0; g < kTbLineBytes / 64; ++g) {
      TbD2 a[4], b[2];
#pragma unroll
      for (int n = 0; n < 2; ++n) b[n] = *reinterpret_cast<const TbD2*>(pb + 16 * n * kTbLinePitch + g * 64);
#pragma unroll
      for (int m = 0; m < 4; ++m) a[m] = *reinterpret_cast<const TbD2*>(pa + 16 * m * kTbLinePitch + g * 64);
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int m = 0; m < 4; ++m)
#pragma unroll
          for (int n = 0; n < 2; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][t], b[n][t], acc[m][n], 0, 0, 0);
    }
  }
  // register v of a lane: query 4 v + lane / 16 of the block, row lane % 16
  __device__ __forceinline__ void store(double* __restrict__ scores, i64 size, i64 row0, int qp, int wave, int lane) const {
#pragma unroll
    for (int n = 0; n < 2; ++n) {
      const i64 row = row0 + 32 * wave + 16 * n + (lane & 15);
      if (row >= size) continue;
#pragma unroll
      for (int m = 0; m < 4; ++m)
#pragma unroll
        for (int v = 0; v < 4; ++v) {
          const int j = 16 * m + 4 * v + (lane >> 4);
          if (j < qp) scores[(i64)j * size + row] = acc[m][n][v];
        }
    }
  }
};

// Workgroup b: rows [128 b, 128 b + 128) of the shard against queries x[0 .. qp), qp <= 64.
// scores[j * size + local] for every j < qp and every local row of the tile below size.
template <typename V>
__global__ __launch_bounds__(kTPB) void topk_batch_scores_kernel(const V* __restrict__ x, int qp, int xwide,
                                                                 const V* __restrict__ data, PartDesc part, int rwide,
                                                                 V* __restrict__ scores) {
  constexpr int E = (int)(16 / sizeof(V));
  constexpr int KS = kTbLineBytes / (int)sizeof(V);  // columns of a slab
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][kTbSlabBytes];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const i64 size = part.size, cols = part.cols;
  const i64 row0 = (i64)blockIdx.x * kTbRows;
  // staging: chunk `ch` of lines ln + 32 p; a pad line keeps a valid pointer and is never read
  const int ch = tid & 7, ln = tid >> 3;
  const V* src[kTbStage];
  bool live[kTbStage];
#pragma unroll
  for (int p = 0; p < kTbStage; ++p) {
    const int line = ln + 32 * p;
    if (line < kTbRows) {
      live[p] = row0 + line < size;
      src[p] = data + (live[p] ? row0 + line : 0) * part.pitch;
    } else {
      live[p] = line - kTbRows < qp;
      src[p] = x + (i64)(live[p] ? line - kTbRows : 0) * cols;
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
  TbMma<V> mma;
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
  mma.store(scores, size, row0, qp, wave, lane);
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the batched top-k pull on st (no host synchronisation): per pass of 64 queries the scores
// launch and the selection levels, all counted under GLINT_K_PULL_ROWS_DOT. x, out_rows and out_vals are
// device pointers. Under the shard's lock; the scratch is s->d_det, sized by the first (largest) pass.
template <typename V>
int pull_topk_batch(glint_shard* s, const void* x, i64 q, i64 k, i64* out_rows, void* out_vals, hipStream_t st) {
  const i64 size = s->part.size, cols = s->part.cols;
  const int xw = (cols * (i64)sizeof(V)) % 16 == 0 && aligned(x, 16);
  const int rw = (s->part.pitch * (i64)sizeof(V)) % 16 == 0 && aligned(s->data, 16);
  for (i64 q0 = 0; q0 < q; q0 += kTbPass) {
    const i64 qp = q - q0 < kTbPass ? q - q0 : kTbPass;
    const TopkPlan p = topk_plan(size, qp, k, (i64)sizeof(V));
    if (p.levels < 1) return GLINT_EINVAL;
    int rc = grow(&s->d_det, &s->det_bytes, (size_t)p.total_bytes);
    if (rc) return rc;
    if (size > 0) {
      const unsigned grid = (unsigned)((size + kTbRows - 1) / kTbRows);
      HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_DOT, topk_batch_scores_kernel<V>, grid, kTPB, st,
                      (const V*)x + q0 * cols, (int)qp, xw, (const V*)s->data, s->part, rw, (V*)s->d_det));
    }
    rc = topk_select_levels<V>(s, p, qp, k, out_rows + q0 * k, (V*)out_vals + q0 * k, st);
    if (rc) return rc;
  }
  return GLINT_OK;
}

template int pull_topk_batch<float>(glint_shard*, const void*, i64, i64, i64*, void*, hipStream_t);
template int pull_topk_batch<double>(glint_shard*, const void*, i64, i64, i64*, void*, hipStream_t);

}  // namespace glint
