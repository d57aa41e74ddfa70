// glint_rowaxpy_batch.hip -- batched row axpy push (glint_mat_push_rows_axpy_batch*, DESIGN.md "Batched row
// axpy push"): rows[i] += sum over j of coef[i][j] * x[j] for up to GLINT_AXPY_BATCH_MAX_VECTORS vectors,
// the write half of the batched row dot pull. The call is linear in coef, so the records of one row are
// first summed into one coefficient line and the push becomes one matrix product per distinct row,
// computed by gfx950's matrix instructions. Three stages on the caller's stream:
//   rows_front       the row push's front end unchanged, always strict: one item {start, len} per distinct
//                    row, idx sorted by row with equal rows in push order;
//   axpy_coef_sum    one wave per (item, slice of q): C[j] = ((+0 + coef[i0][j]) + coef[i1][j]) + ... by
//                    run_sum (glint_rowstep.h), written as line `item` of Cs[nitems][qp], qp = q rounded up
//                    to a whole slab of K, the tail [q, qp) zeros;
//   rows_axpy_batch  one workgroup per (tile of 128 items, pass of 64 columns), the pass the fast grid
//                    index: t = Cs[tile] * x[:, pass] by matrix instructions, then row += t, one add.
// No run is split and nothing is atomic but the error record of the front end.
//
// The product. K is q, walked in slabs of 128 B (32 Float / 16 Double vectors) and never split across
// workgroups; the pipeline is the batched pulls': two slabs resident, the next slab's global loads issued
// into registers ahead of the current slab's matrix instructions and stored to LDS behind them, one barrier
// per slab. Operand A (M = items) is the tile's 128 lines of Cs -- K-contiguous, 16-B aligned and whole --
// staged exactly as glint_slab.h stages table rows. Operand B (N = columns) is x transposed: a slab holds
// one line per vector j with the pass's 64 columns of x[j], loaded coalesced along the columns (16 B per
// thread when x allows, else by element), zero where j >= q or the column >= cols, and stored K-major as
// it was loaded. A lane then reads the element of its own (column, k) straight out of LDS: there is no
// transpose pass. The line pitch is 72 elements (kXbPitch), so that the k-lines one matrix instruction's
// lanes read together start 32 banks apart (DESIGN.md has the arithmetic).
//
// The accumulators are the batched row dot pull's (DbMma): Float v_mfma_f32_32x32x2_f32, two 32 x 32 per
// wave; Double v_mfma_f64_16x16x4_f64, 2 x 4 of 16 x 16. A lane of the result holds one column and several
// items, so a load or store instruction of the epilogue covers 32 (Float) / 16 (Double) consecutive columns
// of one row, 128 B. The rows' elements are loaded in front of the last slab's matrix instructions, so the
// adds do not wait on HBM behind them.
#include "glint_device.h"
#include "glint_host.h"
#include "glint_rowstep.h"  // run_sum
#include "glint_slab.h"     // the slab geometry of operand A and tb_chunk

namespace glint {

static_assert(GLINT_AXPY_BATCH_MAX_VECTORS == GLINT_DOT_MAX_QUERIES, "the write half takes the pull's batch");

// ---- stage 2: the coefficient run-sum -----------------------------------------------------------
// Persistent grid; one wave per (item, slice of the qp coefficients of its line), rows_step_fold's frame
// with q in the role of cols. A slice is 64 lanes x 16 B when VEC16 (q * sizeof(V) a multiple of 16 and
// coef 16-B aligned), else one element per lane; a line of Cs is 16-B aligned and a whole number of
// 16-B chunks either way. Elements [q, qp) are loaded as zeros by slice_load and stored as such.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void axpy_coef_sum_kernel(const u32* __restrict__ idx,
                                                             const uint2* __restrict__ items,
                                                             const u32* __restrict__ nitems,
                                                             const V* __restrict__ coef, int q, int qp,
                                                             V* __restrict__ cs) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const u32 nslices = (u32)((qp + 64 * VPL - 1) / (64 * VPL));
  const u64 total = (u64)*nitems * nslices;
  for (u64 w = w0; w < total; w += nw) {
    const u32 it = (u32)(w / nslices), slice = (u32)(w % nslices);
    const uint2 e = items[it];
    const i64 c = (i64)slice * 64 * VPL + (i64)lane * VPL;
    V G[VPL];
#pragma unroll
    for (int k = 0; k < VPL; ++k) G[k] = V(0);
    run_sum<V, VPL, slice_load<V, VPL, VEC16>>(G, idx, e.x, e.y, coef, c, (i64)q, lane);
    slice_store<V, VPL, VEC16>(G, cs + (i64)it * qp, c, (i64)qp);
  }
}

// ---- stage 3: the product and the add -----------------------------------------------------------
// Operand B's part of a slab: KS lines (one per vector) of kTbPass columns at a pitch of 72 elements,
// behind operand A's 128 lines. Both types fill the 64 lines' worth of LDS the batched pulls' vectors take.
template <typename V> struct Xb {
  static constexpr int kLineBytes = kTbPass * (int)sizeof(V);          // 256 B Float, 512 B Double
  static constexpr int kPitch = kLineBytes + kLineBytes / 8;           // 288 B Float, 576 B Double
  static constexpr int KS = kTbLineBytes / (int)sizeof(V);             // lines: vectors of a slab
  static constexpr int kChunks = kLineBytes / 16;                      // 16-B chunks of a line
  static constexpr int kLinesPerTrip = kTPB / kChunks;                 // lines the workgroup stages at once
  static constexpr int kStage = KS / kLinesPerTrip;                    // chunks a thread stages per slab
  static constexpr int kBase = kTbRows * kTbLinePitch;                 // behind operand A
  static_assert(kBase + KS * kPitch <= kTbSlabBytes, "operand B fits where the pulls keep their vectors");
  static_assert(kStage * kLinesPerTrip == KS && kPitch % 16 == 0, "whole trips of 16-B aligned chunks");
};
constexpr int kAbStageA = kTbRows / 32;  // chunks of operand A a thread stages per slab

// The wave's accumulators, the matrix instructions of one slab, the early loads of the rows' elements and
// the add and store. `local` is the tile's 128 local rows (-1: no such item); c0 the pass's first column.
template <typename V> struct AbMma;

template <> struct AbMma<float> {
  TbF16 acc[2];   // the wave's 32 items x columns [32 b, 32 b + 32)
  float row[2][16];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int v = 0; v < 16; ++v) acc[b][v] = 0.f;
  }
  // step (g, t): k = 8 g + 4 (lane / 32) + t of the slab, for A by its 16-B reads, for B by the line
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    const int l = lane & 31, h = lane >> 5;
    const unsigned char* pa = buf + (32 * wave + l) * kTbLinePitch + h * 16;
    const unsigned char* pb = buf + Xb<float>::kBase + 4 * h * Xb<float>::kPitch + l * 4;
#pragma unroll
    for (int g = 0; g < kTbLineBytes / 32; ++g) {
      const TbF4 a = *reinterpret_cast<const TbF4*>(pa + g * 32);
#pragma unroll
      for (int t = 0; t < 4; ++t) {
        const float b0 = *reinterpret_cast<const float*>(pb + (8 * g + t) * Xb<float>::kPitch);
        const float b1 = *reinterpret_cast<const float*>(pb + (8 * g + t) * Xb<float>::kPitch + 128);
        acc[0] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b0, acc[0], 0, 0, 0);
        acc[1] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[t], b1, acc[1], 0, 0, 0);
      }
    }
  }
  // register v of a lane: item 8 (v / 4) + 4 (lane / 32) + v % 4 of the wave's 32, column lane % 32
  __device__ __forceinline__ void load(const float* data, i64 pitch, const int* local, i64 cols, i64 c0, int wave,
                                       int lane) {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int l = local[32 * wave + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3)];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const i64 c = c0 + 32 * b + (lane & 31);
        row[b][v] = (l >= 0 && c < cols) ? data[(i64)l * pitch + c] : 0.f;
      }
    }
  }
  __device__ __forceinline__ void store(float* data, i64 pitch, const int* local, i64 cols, i64 c0, int wave,
                                        int lane) const {
#pragma unroll
    for (int v = 0; v < 16; ++v) {
      const int l = local[32 * wave + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3)];
#pragma unroll
      for (int b = 0; b < 2; ++b) {
        const i64 c = c0 + 32 * b + (lane & 31);
        if (l >= 0 && c < cols) data[(i64)l * pitch + c] = vadd(row[b][v], acc[b][v]);
      }
    }
  }
};

template <> struct AbMma<double> {
  TbD4 acc[2][4];  // items [16 m, 16 m + 16) of the wave's 32 x columns [16 b, 16 b + 16)
  double row[2][4][4];
  __device__ __forceinline__ void clear() {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int b = 0; b < 4; ++b)
#pragma unroll
        for (int v = 0; v < 4; ++v) acc[m][b][v] = 0.0;
  }
  // step (g, t): k = 8 g + 2 (lane / 16) + t of the slab
  __device__ __forceinline__ void slab(const unsigned char* buf, int wave, int lane) {
    const int l = lane & 15, kq = lane >> 4;
    const unsigned char* pa = buf + (32 * wave + l) * kTbLinePitch + kq * 16;
    const unsigned char* pb = buf + Xb<double>::kBase + 2 * kq * Xb<double>::kPitch + l * 8;
#pragma unroll
    for (int g = 0; g < kTbLineBytes / 64; ++g) {
      TbD2 a[2];
#pragma unroll
      for (int m = 0; m < 2; ++m) a[m] = *reinterpret_cast<const TbD2*>(pa + 16 * m * kTbLinePitch + g * 64);
#pragma unroll
      for (int t = 0; t < 2; ++t) {
        double b[4];
#pragma unroll
        for (int n = 0; n < 4; ++n)
          b[n] = *reinterpret_cast<const double*>(pb + (8 * g + t) * Xb<double>::kPitch + 128 * n);
#pragma unroll
        for (int m = 0; m < 2; ++m)
#pragma unroll
          for (int n = 0; n < 4; ++n)
            acc[m][n] = __builtin_amdgcn_mfma_f64_16x16x4f64(a[m][t], b[n], acc[m][n], 0, 0, 0);
      }
    }
  }
  // register v of a lane: item 4 v + lane / 16 of the block of 16, column lane % 16
  __device__ __forceinline__ void load(const double* data, i64 pitch, const int* local, i64 cols, i64 c0, int wave,
                                       int lane) {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int l = local[32 * wave + 16 * m + 4 * v + (lane >> 4)];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const i64 c = c0 + 16 * b + (lane & 15);
          row[m][b][v] = (l >= 0 && c < cols) ? data[(i64)l * pitch + c] : 0.0;
        }
      }
  }
  __device__ __forceinline__ void store(double* data, i64 pitch, const int* local, i64 cols, i64 c0, int wave,
                                        int lane) const {
#pragma unroll
    for (int m = 0; m < 2; ++m)
#pragma unroll
      for (int v = 0; v < 4; ++v) {
        const int l = local[32 * wave + 16 * m + 4 * v + (lane >> 4)];
#pragma unroll
        for (int b = 0; b < 4; ++b) {
          const i64 c = c0 + 16 * b + (lane & 15);
          if (l >= 0 && c < cols) data[(i64)l * pitch + c] = vadd(row[m][b][v], acc[m][b][v]);
        }
      }
  }
};

// Workgroup b: items [128 (b / npass), + 128) against columns [64 (b % npass), + 64). The grid is sized
// from n; a tile at or past *nitems returns at once. An item's row is this workgroup's alone for the
// pass's columns: items are distinct rows.
template <typename V>
__global__ __launch_bounds__(kTPB) void rows_axpy_batch_kernel(const u32* __restrict__ key,
                                                               const uint2* __restrict__ items,
                                                               const u32* __restrict__ nitems,
                                                               const V* __restrict__ cs, int qp,
                                                               const V* __restrict__ x, int q, int npass, int xwide,
                                                               V* data, PartDesc part) {
  constexpr int E = (int)(16 / sizeof(V));
  typedef Xb<V> B;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][kTbSlabBytes];
  __shared__ int local[kTbRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const i64 cols = part.cols;
  const u32 nit = *nitems;
  const u32 i0 = (blockIdx.x / (unsigned)npass) * kTbRows;
  if (i0 >= nit) return;
  const i64 c0 = (i64)(blockIdx.x % (unsigned)npass) * kTbPass;
  if (tid < kTbRows) local[tid] = i0 + tid < nit ? (int)key[items[i0 + tid].x] : -1;
  // staging. A: chunk `ch` of lines ln + 32 p of Cs, a line past nitems zero-filled and never loaded.
  // B: chunk `bch` (columns c0 + E bch ..) of the vectors bln + kLinesPerTrip p of the slab.
  const int ch = tid & 7, ln = tid >> 3;
  const int bch = tid % B::kChunks, bln = tid / B::kChunks;
  const V* srca[kAbStageA];
  bool live[kAbStageA];
#pragma unroll
  for (int p = 0; p < kAbStageA; ++p) {
    live[p] = i0 + ln + 32 * p < nit;
    srca[p] = cs + (i64)(live[p] ? i0 + ln + 32 * p : i0) * qp;
  }
  TbU4 sa[kAbStageA], sb[B::kStage];
  auto fetch = [&](int k0) {
#pragma unroll
    for (int p = 0; p < kAbStageA; ++p) sa[p] = tb_chunk<V>(srca[p], k0 + ch * E, qp, live[p], true);
#pragma unroll
    for (int p = 0; p < B::kStage; ++p) {
      const int j = k0 + bln + B::kLinesPerTrip * p;
      sb[p] = tb_chunk<V>(x + (i64)(j < q ? j : 0) * cols, c0 + bch * E, cols, j < q, xwide != 0);
    }
  };
  auto stash = [&](int b) {
#pragma unroll
    for (int p = 0; p < kAbStageA; ++p)
      *reinterpret_cast<TbU4*>(&lds[b][(ln + 32 * p) * kTbLinePitch + ch * 16]) = sa[p];
#pragma unroll
    for (int p = 0; p < B::kStage; ++p)
      *reinterpret_cast<TbU4*>(&lds[b][B::kBase + (bln + B::kLinesPerTrip * p) * B::kPitch + bch * 16]) = sb[p];
  };
  const int nslab = qp / B::KS;
  AbMma<V> mma;
  mma.clear();
  fetch(0);
  stash(0);
  __syncthreads();  // also publishes `local`
  for (int s = 0; s + 1 < nslab; ++s) {
    fetch((s + 1) * B::KS);
    mma.slab(lds[s & 1], wave, lane);
    // slab s + 1's buffer was last read in iteration s - 1, in front of that iteration's barrier
    stash((s + 1) & 1);
    __syncthreads();
  }
  mma.load(data, part.pitch, local, cols, c0, wave, lane);  // in flight over the last slab's instructions
  mma.slab(lds[(nslab - 1) & 1], wave, lane);
  mma.store(data, part.pitch, local, cols, c0, wave, lane);
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the batched row axpy push on st (no host synchronisation): the front end's launches, the
// coefficient run-sum and the product, the last two counted under GLINT_K_PUSH_ROWS_AXPY. rows, coef and x
// are device pointers. Cs lies in s->d_det behind the front end's layout (rows_front_bytes):
// min(n, part.size) * qp values; the scratch is grown before anything is launched. Under the shard's lock.
template <typename V>
int push_rows_axpy_batch(glint_shard* s, const i64* rows, i64 n, const void* coef, const void* x, i64 q,
                         hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !coef || !x || q < 1 || q > GLINT_AXPY_BATCH_MAX_VECTORS) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  constexpr int KS = Xb<V>::KS;
  const i64 qp = (q + KS - 1) / KS * KS;
  const i64 most = n < (i64)s->part.size ? n : (i64)s->part.size;  // distinct rows, at most
  const size_t front = rows_front_bytes(n);
  int rc = grow(&s->d_det, &s->det_bytes, front + (size_t)most * (size_t)qp * sizeof(V));
  if (rc) return rc;
  RowsFront f;
  rc = rows_front(s, rows, n, GLINT_PUSH_DETERMINISTIC, st, &f);  // finds its scratch grown already
  if (rc) return rc;
  V* cs = (V*)((char*)s->d_det + front);
  const bool c16 = (q * (i64)sizeof(V)) % 16 == 0 && aligned(coef, 16);
  const unsigned gs = grid_for(most * row_slices<V>(qp, c16), kTPB / 64, (i64)s->cus * 8);
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS_AXPY, c16 ? axpy_coef_sum_kernel<V, true> : axpy_coef_sum_kernel<V, false>, gs,
                  kTPB, st, f.idx, f.items, f.nitems, (const V*)coef, (int)q, (int)qp, cs));
  const i64 cols = s->part.cols;
  const int xw = (cols * (i64)sizeof(V)) % 16 == 0 && aligned(x, 16);
  const i64 npass = (cols + kTbPass - 1) / kTbPass;
  const i64 grid = (most + kTbRows - 1) / kTbRows * npass;
  if (grid >= ((i64)1 << 31)) return GLINT_EINVAL;
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS_AXPY, rows_axpy_batch_kernel<V>, (unsigned)grid, kTPB, st, f.key, f.items,
                  f.nitems, (const V*)cs, (int)qp, (const V*)x, (int)q, (int)npass, xw, (V*)s->data, s->part));
  return GLINT_OK;
}

template int push_rows_axpy_batch<float>(glint_shard*, const i64*, i64, const void*, const void*, i64, hipStream_t);
template int push_rows_axpy_batch<double>(glint_shard*, const i64*, i64, const void*, const void*, i64, hipStream_t);

}  // namespace glint
