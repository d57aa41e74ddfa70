// glint_rowwise_batch.hip -- batched row-wise Adagrad row push (glint_mat_push_rows_adagrad_rowwise_batch*,
// DESIGN.md "Batched row-wise Adagrad push"): the batched optimizer row pushes' product with row-wise
// Adagrad's step, one accumulator per row in a vector shard. Per distinct row, G = (the row's coefficient
// lines summed to +0 in push order) * x, formed by glint_axpy_batch.h's product; the step needs the self-dot
// of the row's whole G before any element is stepped, and a workgroup holds 64 columns of it. So the product
// is formed twice, in two launches on ab_grid's grid of (tile of 128 items, pass of 64 columns):
//   rows_front, axpy_coef_sum   glint_rowaxpy_batch.hip's, unchanged (axpy_batch_front);
//   rows_rowwise_ss_batch       the product, then per item the sum of the squares of the pass's columns in
//                               the accumulators' own order, one value per (item, pass) to scratch; the
//                               workgroups of pass 0 also copy the items' accumulators h to scratch (hold);
//   rows_rowwise_step_batch     per item the passes' partials added in ascending order, the row scalars from
//                               hold (glint_steps.h's rowwise_scalars) and k left in LDS -- the same bits in
//                               every pass's workgroup; the product again, then w' = rowwise_update(w, k, G).
//                               The workgroup of pass 0 stores h'.
// Both launches form G with ab_product from accumulators at +0, so they hold the same bits of it. G is never
// written anywhere: the scratch is npass + 1 values an item, behind Cs in the weights shard's d_det. No
// workgroup of the second launch reads a state element that another one writes: they read `hold`. No run is
// split and nothing is atomic but the error record of the front end.
//
// The sum of squares. A lane holds 32 slots of G: one column of B = 2 (Float) / 4 (Double) column blocks for
// each of 16 / 8 items, and the W = 32 / 16 lanes that share an item hold W consecutive columns of a block.
// Slot B u + b is the lane's u-th item in block b (AbMma::item, AbMma::col), so per item the lane adds its B
// squares in ascending block order from +0 and the W lanes run the xor butterfly W / 2 .. 1, which stays
// inside the item's lanes. A slot whose column is past the row's end is left out by a select: with an
// infinite coefficient the zero-filled columns of x leave inf * 0 = NaN there.
#include "glint_axpy_batch.h"
#include "glint_dot.h"    // dot_step
#include "glint_steps.h"  // rowwise_scalars, rowwise_update

namespace glint {

template <typename V> struct RbLanes {
  static constexpr int W = 128 / (int)sizeof(V);  // lanes that share an item: consecutive columns of a block
  static constexpr int B = kTbPass / W;           // column blocks of a pass
  static constexpr int U = kAbElems / B;          // items of a lane
};

// ---- phase 1: the partial sums of squares ---------------------------------------------------------
// Workgroup b: items [128 (b / npass), + 128) against columns [64 (b % npass), + 64), as
// rows_axpy_batch_kernel. partial[item * npass + pass] = the pass's part of ss (the header's step 3), item
// the index into `items`; hold[item] = the item's accumulator as it was before the call (pass 0 only).
template <typename V>
__global__ __launch_bounds__(kTPB) void rows_rowwise_ss_batch_kernel(const u32* __restrict__ key,
                                                                     const uint2* __restrict__ items,
                                                                     const u32* __restrict__ nitems,
                                                                     const V* __restrict__ cs, int qp,
                                                                     const V* __restrict__ x, int q, int npass,
                                                                     int xwide, const V* __restrict__ hdata, i64 cols,
                                                                     V* __restrict__ partial, V* __restrict__ hold) {
  typedef AbMma<V> M;
  typedef RbLanes<V> L;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][kTbSlabBytes];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const u32 nit = *nitems;
  const u32 i0 = (blockIdx.x / (unsigned)npass) * kTbRows;
  if (i0 >= nit) return;
  const int pass = (int)(blockIdx.x % (unsigned)npass);
  const i64 c0 = (i64)pass * kTbPass;
  // thread t < 128 of a pass-0 workgroup copies item i0 + t's accumulator
  const bool copies = pass == 0 && tid < kTbRows && i0 + tid < nit;
  const i64 mine = copies ? (i64)key[items[i0 + tid].x] : 0;
  M mma;
  V h = V(0);
  ab_product<V>(mma, lds, cs, qp, x, q, xwide, cols, c0, i0, nit, tid, wave, lane, [&]() {
    if (copies) h = hdata[mine];
  });
  if (copies) hold[i0 + tid] = h;
#pragma unroll
  for (int u = 0; u < L::U; ++u) {
    V a = V(0);
#pragma unroll
    for (int b = 0; b < L::B; ++b) {
      const int i = L::B * u + b;
      const V g = mma.get(i);
      const V a2 = dot_step(a, g, g);
      a = c0 + M::col(i, lane) < cols ? a2 : a;  // a select: the slot may hold a NaN the row does not have
    }
#pragma unroll
    for (int d = L::W / 2; d >= 1; d >>= 1) a = vadd(a, __shfl_xor(a, d, 64));
    const u32 it = i0 + (u32)M::item(L::B * u, wave, lane);
    if ((lane & (L::W - 1)) == 0 && it < nit) partial[(i64)it * npass + pass] = a;
  }
}

// ---- phase 2: the row scalars and the update -------------------------------------------------------
// The same grid. Threads 0 .. 127 settle their item's scalars in front of the product -- ab_product's first
// barrier publishes k -- so nothing of them is live across the matrix instructions and the epilogue needs no
// barrier of its own. Every pass's workgroup computes the same bits of k from the same partials and `hold`;
// the workgroup of pass 0 stores h'. The weights tile is loaded in front of the last slab's matrix
// instructions, as rows_step_batch_kernel loads it.
template <typename V>
__global__ __launch_bounds__(kTPB) void rows_rowwise_step_batch_kernel(const u32* __restrict__ key,
                                                                       const uint2* __restrict__ items,
                                                                       const u32* __restrict__ nitems,
                                                                       const V* __restrict__ cs, int qp,
                                                                       const V* __restrict__ x, int q, int npass,
                                                                       int xwide, V* wdata, V* hdata, PartDesc part,
                                                                       const V* __restrict__ partial,
                                                                       const V* __restrict__ hold, V lr, V eps, V C) {
  typedef AbMma<V> M;
  __shared__ __attribute__((aligned(16))) unsigned char lds[2][kTbSlabBytes];
  __shared__ int local[kTbRows];
  __shared__ V kk[kTbRows];
  const int tid = threadIdx.x, lane = tid & 63;
  const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
  const i64 cols = part.cols;
  const u32 nit = *nitems;
  const u32 i0 = (blockIdx.x / (unsigned)npass) * kTbRows;
  if (i0 >= nit) return;
  const int pass = (int)(blockIdx.x % (unsigned)npass);
  const i64 c0 = (i64)pass * kTbPass;
  if (tid < kTbRows) {
    const u32 it = i0 + tid;
    int l = -1;
    V k = V(0);
    if (it < nit) {
      l = (int)key[items[it].x];
      V ss = V(0);
      for (int p = 0; p < npass; ++p) ss = vadd(ss, partial[(i64)it * npass + p]);
      V h = hold[it];
      k = rowwise_scalars<V>(h, ss, C, lr, eps);
      if (pass == 0) hdata[l] = h;
    }
    local[tid] = l;
    kk[tid] = k;
  }
  M mma;
  V w[kAbElems];
  // slot i of this lane: its row (-1: none, or its column is past the row's end)
  auto row_of = [&](int i) { return c0 + M::col(i, lane) < cols ? local[M::item(i, wave, lane)] : -1; };
  ab_product<V>(mma, lds, cs, qp, x, q, xwide, cols, c0, i0, nit, tid, wave, lane, [&]() {
#pragma unroll
    for (int i = 0; i < kAbElems; ++i) {
      const int l = row_of(i);
      w[i] = l >= 0 ? wdata[(i64)l * part.pitch + c0 + M::col(i, lane)] : V(0);
    }
  });
#pragma unroll
  for (int i = 0; i < kAbElems; ++i) {
    const int l = row_of(i);
    const V w2 = rowwise_update<V>(w[i], kk[M::item(i, wave, lane)], mma.get(i));
    if (l >= 0) wdata[(i64)l * part.pitch + c0 + M::col(i, lane)] = w2;
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues a batched row-wise Adagrad row push of n records on st (no host synchronisation): axpy_batch_front
// on the weights shard (its scratch, error state and profile) and the two launches. The scratch -- `most`
// items x (npass partials + 1 accumulator) values -- lies behind Cs in w->d_det, which is grown to the whole
// before anything is launched, so the front end finds its own part grown already (axpy_batch_bytes). rows,
// coef and x are device pointers. Under both shards' locks; `h` is a vector shard of w's type, size and
// partition. lr, eps and cols are rounded once to V here.
template <typename V>
int push_rows_adagrad_rowwise_batch(glint_shard* w, glint_shard* h, const i64* rows, i64 n, const void* coef,
                                    const void* x, i64 q, double lr, double eps, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !coef || !x || q < 1 || q > GLINT_AXPY_BATCH_MAX_VECTORS) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  if (h->part.cols != 0 || h->part.size != w->part.size) return GLINT_EINVAL;
  const i64 cols = w->part.cols;
  const i64 most = n < (i64)w->part.size ? n : (i64)w->part.size;
  i64 npass;
  const i64 grid = ab_grid(most, cols, &npass);
  if (!grid) return GLINT_EINVAL;
  const size_t front = axpy_batch_bytes<V>(w, n, q);
  if (int rc = grow(&w->d_det, &w->det_bytes, front + (size_t)most * (size_t)(npass + 1) * sizeof(V))) return rc;
  AxpyBatchFront a;
  if (int rc = axpy_batch_front<V>(w, rows, n, coef, q, st, &a)) return rc;
  V* partial = (V*)((char*)w->d_det + front);
  V* hold = partial + most * npass;
  const int xw = (cols * (i64)sizeof(V)) % 16 == 0 && aligned(x, 16);
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, rows_rowwise_ss_batch_kernel<V>, (unsigned)grid, kTPB, st, a.f.key, a.f.items,
                  a.f.nitems, (const V*)a.cs, (int)a.qp, (const V*)x, (int)q, (int)npass, xw, (const V*)h->data, cols,
                  partial, hold));
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, rows_rowwise_step_batch_kernel<V>, (unsigned)grid, kTPB, st, a.f.key,
                  a.f.items, a.f.nitems, (const V*)a.cs, (int)a.qp, (const V*)x, (int)q, (int)npass, xw, (V*)w->data,
                  (V*)h->data, w->part, (const V*)partial, (const V*)hold, (V)lr, (V)eps, (V)cols));
  return GLINT_OK;
}

template int push_rows_adagrad_rowwise_batch<float>(glint_shard*, glint_shard*, const i64*, i64, const void*,
                                                    const void*, i64, double, double, hipStream_t);
template int push_rows_adagrad_rowwise_batch<double>(glint_shard*, glint_shard*, const i64*, i64, const void*,
                                                     const void*, i64, double, double, hipStream_t);

}  // namespace glint
