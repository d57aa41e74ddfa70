// glint_axpy_batch.h -- the product t = Cs[tile] * x[:, pass] of the batched row axpy push
// (glint_rowaxpy_batch.hip) and of the batched optimizer row pushes (glint_rowstep_batch.hip,
// glint_rowwise_batch.hip): operand B's LDS layout, the wave's accumulators with the matrix instructions of
// one slab, and the two-slab pipeline around them. All their kernels form the product here, with the same slabs of K and the same instructions in the
// same order on accumulators that start at +0, which is what makes t's bits the same in all of
// them (include/glint_gpu.h); they differ in what their epilogue does with t.
#pragma once
#include "glint_device.h"
#include "glint_host.h"
#include "glint_slab.h"  // the slab geometry of operand A and tb_chunk

namespace glint {

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
constexpr int kAbElems = 32;             // elements of t a lane holds: slots 0 .. 31 of either type

// The wave's accumulators and the matrix instructions of one slab. A lane of the result holds one column
// and several items: slot i is item `item(i, wave, lane)` of the tile's 128 and column `col(i, lane)` of
// the pass's 64, so the lanes of one slot cover 32 (Float) / 16 (Double) consecutive columns of one row.
template <typename V> struct AbMma;

template <> struct AbMma<float> {
  TbF16 acc[2];   // the wave's 32 items x columns [32 b, 32 b + 32)
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
  // slot i = 2 v + b, register v of block b: item 8 (v / 4) + 4 (lane / 32) + v % 4 of the wave's 32,
  // column 32 b + lane % 32. Slots [8 g, 8 g + 8) are four items in both column blocks.
  static __device__ __forceinline__ int item(int i, int wave, int lane) {
    const int v = i >> 1;
    return 32 * wave + 8 * (v >> 2) + 4 * (lane >> 5) + (v & 3);
  }
  static __device__ __forceinline__ int col(int i, int lane) { return 32 * (i & 1) + (lane & 31); }
  __device__ __forceinline__ float get(int i) const { return acc[i & 1][i >> 1]; }
};

template <> struct AbMma<double> {
  TbD4 acc[2][4];  // items [16 m, 16 m + 16) of the wave's 32 x columns [16 b, 16 b + 16)
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
  // slot i = 16 m + 4 v + b, register v of block (m, b): item 16 m + 4 v + lane / 16 of the wave's 32,
  // column 16 b + lane % 16. Slots [8 g, 8 g + 8) are two items in all four column blocks.
  static __device__ __forceinline__ int item(int i, int wave, int lane) {
    return 32 * wave + 16 * (i >> 4) + 4 * ((i >> 2) & 3) + (lane >> 4);
  }
  static __device__ __forceinline__ int col(int i, int lane) { return 16 * (i & 3) + (lane & 15); }
  __device__ __forceinline__ double get(int i) const { return acc[i >> 4][i & 3][(i >> 2) & 3]; }
};

// The product of items [i0, i0 + 128) of the nit lines of Cs with columns [c0, c0 + 64) of x, left in mma
// (cleared here). K is q, walked in slabs of 128 B and never split across workgroups: two slabs resident in
// `lds`, the next slab's global loads issued into registers ahead of the current slab's matrix instructions
// and stored to LDS behind them, one barrier per slab. early() runs in front of the last slab's matrix
// instructions: what the epilogue loads there is in flight over them. The first barrier also publishes what
// the caller wrote to LDS before the call.
template <typename V, typename Early>
__device__ __forceinline__ void ab_product(AbMma<V>& mma, unsigned char (*lds)[kTbSlabBytes],
                                           const V* __restrict__ cs, int qp, const V* __restrict__ x, int q,
                                           int xwide, i64 cols, i64 c0, u32 i0, u32 nit, int tid, int wave, int lane,
                                           Early early) {
  constexpr int E = (int)(16 / sizeof(V));
  typedef Xb<V> B;
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
  mma.clear();
  fetch(0);
  stash(0);
  __syncthreads();
  for (int s = 0; s + 1 < nslab; ++s) {
    fetch((s + 1) * B::KS);
    mma.slab(lds[s & 1], wave, lane);
    // slab s + 1's buffer was last read in iteration s - 1, in front of that iteration's barrier
    stash((s + 1) & 1);
    __syncthreads();
  }
  early();
  mma.slab(lds[(nslab - 1) & 1], wave, lane);
}

// Bytes of s->d_det that axpy_batch_front lays out for n records and q vectors, a multiple of 128:
// rows_front_bytes(n), then Cs -- min(n, part.size) lines of q rounded up to a whole slab of K. A call that
// keeps scratch of its own behind Cs grows s->d_det to the sum first and finds the front's pointers unmoved.
template <typename V>
inline size_t axpy_batch_bytes(const glint_shard* s, i64 n, i64 q) {
  const i64 qp = (q + Xb<V>::KS - 1) / Xb<V>::KS * Xb<V>::KS;
  const i64 most = n < (i64)s->part.size ? n : (i64)s->part.size;
  return rows_front_bytes(n) + (size_t)most * (size_t)qp * sizeof(V);
}

// The product's grid: one workgroup per (tile of 128 of at most `most` items, pass of 64 columns), the pass
// the fast index. 0 when it does not fit a launch.
inline i64 ab_grid(i64 most, i64 cols, i64* npass) {
  *npass = (cols + kTbPass - 1) / kTbPass;
  const i64 grid = (most + kTbRows - 1) / kTbRows * *npass;
  return grid < ((i64)1 << 31) ? grid : 0;
}

}  // namespace glint
