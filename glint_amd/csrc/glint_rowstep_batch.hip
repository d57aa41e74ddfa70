// glint_rowstep_batch.hip -- batched optimizer row pushes (glint_mat_push_rows_adagrad_batch*,
// _adam_batch*, _ftrl_batch*; DESIGN.md "Batched optimizer row pushes"): the batched row axpy push with an
// optimizer step where it adds. Per distinct row, G = (the row's coefficient lines summed to +0 in push
// order) * x, formed by glint_axpy_batch.h's product exactly as glint_mat_push_rows_axpy_batch forms what
// it adds, then one step of glint_steps.h's policy -- Adagrad, Adam, FTRL-proximal -- with that G, every
// operation rounded on its own. The n x cols gradient is never written anywhere: the tile of G sits in the
// wave's accumulators when the row and its state are read. Three stages on the caller's stream:
//   rows_front, axpy_coef_sum   glint_rowaxpy_batch.hip's, unchanged (axpy_batch_front);
//   rows_step_batch             one workgroup per (tile of 128 items, pass of 64 columns): the product,
//                               then the step of the weights tile and of Step::kParts state tiles.
// No run is split and nothing is atomic but the error record of the front end.
//
// The epilogue. A lane holds 32 elements of G (kAbElems slots: one column, several items), so one load or
// store instruction covers 32 (Float) / 16 (Double) consecutive columns of one row, 128 B, by element: part
// p of the state row starts at column p * cols, which for odd cols has no 16-B alignment. The weights tile
// (32 values a lane) is loaded in front of the last slab's matrix instructions as the plain push loads it.
// The state tiles are not: with two parts in Double they would be 128 more registers a lane on top of 64 of
// weights and 64 of accumulators. They go through the epilogue in four groups of 8 slots, two groups
// resident: group 0 is loaded with the weights in front of the last slab, group g + 1 in front of group g's
// steps and stores, so one group's divisions and square roots cover the next group's loads. A row of either
// shard is this workgroup's alone for the pass's columns (items are distinct rows, and the two shards share
// no memory), so the loads of group g + 1 never see group g's stores.
#include "glint_axpy_batch.h"
#include "glint_steps.h"

namespace glint {

constexpr int kSbGroup = 8;                      // slots of a state group
constexpr int kSbGroups = kAbElems / kSbGroup;   // groups of the epilogue

// Workgroup b: items [128 (b / npass), + 128) against columns [64 (b % npass), + 64), as
// rows_axpy_batch_kernel. `sdata` is the state shard, its rows at a pitch of `spitch`; part p of a row is
// columns [p * cols, + cols) of it.
template <typename V, typename Step>
__global__ __launch_bounds__(kTPB) void rows_step_batch_kernel(const u32* __restrict__ key,
                                                               const uint2* __restrict__ items,
                                                               const u32* __restrict__ nitems,
                                                               const V* __restrict__ cs, int qp,
                                                               const V* __restrict__ x, int q, int npass, int xwide,
                                                               V* wdata, V* sdata, PartDesc part, i64 spitch, Step k) {
  typedef AbMma<V> M;
  constexpr int P = Step::kParts;
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
  M mma;
  V w[kAbElems], s[2][P][kSbGroup];
  // slot i of this lane: its row (-1: none, or its column is past the row's end) and its column
  auto row_of = [&](int i) { return c0 + M::col(i, lane) < cols ? local[M::item(i, wave, lane)] : -1; };
  auto load_state = [&](int g) {
#pragma unroll
    for (int e = 0; e < kSbGroup; ++e) {
      const int i = g * kSbGroup + e, l = row_of(i);
      const V* sp = sdata + (i64)l * spitch + c0 + M::col(i, lane);
#pragma unroll
      for (int p = 0; p < P; ++p) s[g & 1][p][e] = l >= 0 ? sp[p * cols] : V(0);
    }
  };
  ab_product<V>(mma, lds, cs, qp, x, q, xwide, cols, c0, i0, nit, tid, wave, lane, [&]() {
#pragma unroll
    for (int i = 0; i < kAbElems; ++i) {
      const int l = row_of(i);
      w[i] = l >= 0 ? wdata[(i64)l * part.pitch + c0 + M::col(i, lane)] : V(0);
    }
    load_state(0);
  });
#pragma unroll
  for (int g = 0; g < kSbGroups; ++g) {
    if (g + 1 < kSbGroups) load_state(g + 1);
#pragma unroll
    for (int e = 0; e < kSbGroup; ++e) {
      const int i = g * kSbGroup + e, l = row_of(i);
      V se[P];
#pragma unroll
      for (int p = 0; p < P; ++p) se[p] = s[g & 1][p][e];
      k.step(w[i], se, mma.get(i));  // a slot without a row steps zeros and stores nothing
      if (l >= 0) {
        V* sp = sdata + (i64)l * spitch + c0 + M::col(i, lane);
#pragma unroll
        for (int p = 0; p < P; ++p) sp[p * cols] = se[p];
        wdata[(i64)l * part.pitch + c0 + M::col(i, lane)] = w[i];
      }
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues a batched optimizer row push of n records on st (no host synchronisation): axpy_batch_front on
// the weights shard (its scratch, error state and profile) and the stepping product. rows, coef and x are
// device pointers. Under both shards' locks; `s` has w's type and partition and Step::kParts * cols columns.
template <typename V, typename Step>
int push_rows_step_batch(glint_shard* w, glint_shard* s, const i64* rows, i64 n, const void* coef, const void* x,
                         i64 q, const Step& k, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !coef || !x || q < 1 || q > GLINT_AXPY_BATCH_MAX_VECTORS) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  if (s->part.cols != Step::kParts * w->part.cols || s->part.size != w->part.size) return GLINT_EINVAL;
  AxpyBatchFront a;
  if (int rc = axpy_batch_front<V>(w, rows, n, coef, q, st, &a)) return rc;
  const i64 cols = w->part.cols;
  const int xw = (cols * (i64)sizeof(V)) % 16 == 0 && aligned(x, 16);
  i64 npass;
  const i64 grid = ab_grid(a.most, cols, &npass);
  if (!grid) return GLINT_EINVAL;
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, rows_step_batch_kernel<V, Step>, (unsigned)grid, kTPB, st, a.f.key,
                  a.f.items, a.f.nitems, (const V*)a.cs, (int)a.qp, (const V*)x, (int)q, (int)npass, xw, (V*)w->data,
                  (V*)s->data, w->part, (i64)s->part.pitch, k));
  return GLINT_OK;
}

// The scalars are settled as the unbatched pushes settle them (glint_rowadagrad.hip, glint_rowadam.hip,
// glint_rowftrl.hip): each rounded once to V.
template <typename V>
int push_rows_adagrad_batch(glint_shard* w, glint_shard* h, const i64* rows, i64 n, const void* coef, const void* x,
                            i64 q, double lr, double eps, hipStream_t st) {
  return push_rows_step_batch<V>(w, h, rows, n, coef, x, q, AdagradScalars<V>{(V)lr, (V)eps}, st);
}

template <typename V>
int push_rows_adam_batch(glint_shard* w, glint_shard* s, const i64* rows, i64 n, const void* coef, const void* x,
                         i64 q, double lr, double beta1, double beta2, double eps, i64 step, hipStream_t st) {
  if (n > 0 && step < 1) return GLINT_EINVAL;
  return push_rows_step_batch<V>(w, s, rows, n, coef, x, q, adam_scalars<V>(lr, beta1, beta2, eps, step), st);
}

template <typename V>
int push_rows_ftrl_batch(glint_shard* w, glint_shard* s, const i64* rows, i64 n, const void* coef, const void* x,
                         i64 q, double alpha, double beta, double l1, double l2, hipStream_t st) {
  return push_rows_step_batch<V>(w, s, rows, n, coef, x, q, FtrlScalars<V>{(V)alpha, (V)beta, (V)l1, (V)l2}, st);
}

#define GLINT_STEP_BATCH_INSTANCES(V)                                                                                 \
  template int push_rows_adagrad_batch<V>(glint_shard*, glint_shard*, const i64*, i64, const void*, const void*, i64, \
                                          double, double, hipStream_t);                                               \
  template int push_rows_adam_batch<V>(glint_shard*, glint_shard*, const i64*, i64, const void*, const void*, i64,    \
                                       double, double, double, double, i64, hipStream_t);                             \
  template int push_rows_ftrl_batch<V>(glint_shard*, glint_shard*, const i64*, i64, const void*, const void*, i64,    \
                                       double, double, double, double, hipStream_t);
GLINT_STEP_BATCH_INSTANCES(float)
GLINT_STEP_BATCH_INSTANCES(double)
#undef GLINT_STEP_BATCH_INSTANCES

}  // namespace glint
