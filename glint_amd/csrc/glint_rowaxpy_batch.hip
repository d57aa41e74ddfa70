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
#include "glint_axpy_batch.h"  // the product: Xb, AbMma, ab_product
#include "glint_rowstep.h"     // run_sum

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
// Workgroup b: items [128 (b / npass), + 128) against columns [64 (b % npass), + 64). The grid is sized
// from n; a tile at or past *nitems returns at once. An item's row is this workgroup's alone for the
// pass's columns: items are distinct rows. The product is glint_axpy_batch.h's; `local` is the tile's 128
// local rows (-1: no such item). The rows' elements are loaded in front of the last slab's matrix
// instructions, so the adds do not wait on HBM behind them.
template <typename V>
__global__ __launch_bounds__(kTPB) void rows_axpy_batch_kernel(const u32* __restrict__ key,
                                                               const uint2* __restrict__ items,
                                                               const u32* __restrict__ nitems,
                                                               const V* __restrict__ cs, int qp,
                                                               const V* __restrict__ x, int q, int npass, int xwide,
                                                               V* data, PartDesc part) {
  typedef AbMma<V> M;
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
  V row[kAbElems];
  ab_product<V>(mma, lds, cs, qp, x, q, xwide, cols, c0, i0, nit, tid, wave, lane, [&]() {
#pragma unroll
    for (int i = 0; i < kAbElems; ++i) {
      const int l = local[M::item(i, wave, lane)];
      const i64 c = c0 + M::col(i, lane);
      row[i] = (l >= 0 && c < cols) ? data[(i64)l * part.pitch + c] : V(0);
    }
  });
#pragma unroll
  for (int i = 0; i < kAbElems; ++i) {
    const int l = local[M::item(i, wave, lane)];
    const i64 c = c0 + M::col(i, lane);
    if (l >= 0 && c < cols) data[(i64)l * part.pitch + c] = vadd(row[i], mma.get(i));
  }
}

// ---- host side ----------------------------------------------------------------------------------
// The first two stages of a batched push of n records on st: s->d_det is grown to hold Cs behind the front
// end's layout (rows_front_bytes) -- min(n, part.size) * qp values -- before anything is launched, then the
// front end's launches and the coefficient run-sum, counted under GLINT_K_PUSH_ROWS_AXPY.
template <typename V>
int axpy_batch_front(glint_shard* s, const i64* rows, i64 n, const void* coef, i64 q, hipStream_t st,
                     AxpyBatchFront* out) {
  constexpr int KS = Xb<V>::KS;
  const i64 qp = (q + KS - 1) / KS * KS;
  const i64 most = n < (i64)s->part.size ? n : (i64)s->part.size;  // distinct rows, at most
  const size_t front = rows_front_bytes(n);
  int rc = grow(&s->d_det, &s->det_bytes, axpy_batch_bytes<V>(s, n, q));  // a no-op when the caller grew it
  if (rc) return rc;
  RowsFront f;
  rc = rows_front(s, rows, n, GLINT_PUSH_DETERMINISTIC, st, &f);  // finds its scratch grown already
  if (rc) return rc;
  V* cs = (V*)((char*)s->d_det + front);
  const bool c16 = (q * (i64)sizeof(V)) % 16 == 0 && aligned(coef, 16);
  const unsigned gs = grid_for(most * row_slices<V>(qp, c16), kTPB / 64, (i64)s->cus * 8);
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS_AXPY, c16 ? axpy_coef_sum_kernel<V, true> : axpy_coef_sum_kernel<V, false>, gs,
                  kTPB, st, f.idx, f.items, f.nitems, (const V*)coef, (int)q, (int)qp, cs));
  *out = {f, cs, qp, most};
  return GLINT_OK;
}

template int axpy_batch_front<float>(glint_shard*, const i64*, i64, const void*, i64, hipStream_t, AxpyBatchFront*);
template int axpy_batch_front<double>(glint_shard*, const i64*, i64, const void*, i64, hipStream_t, AxpyBatchFront*);

// Enqueues the batched row axpy push on st (no host synchronisation): axpy_batch_front's launches and the
// product, counted under GLINT_K_PUSH_ROWS_AXPY. rows, coef and x are device pointers. Under the shard's lock.
template <typename V>
int push_rows_axpy_batch(glint_shard* s, const i64* rows, i64 n, const void* coef, const void* x, i64 q,
                         hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !coef || !x || q < 1 || q > GLINT_AXPY_BATCH_MAX_VECTORS) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  AxpyBatchFront a;
  if (int rc = axpy_batch_front<V>(s, rows, n, coef, q, st, &a)) return rc;
  const i64 cols = s->part.cols;
  const int xw = (cols * (i64)sizeof(V)) % 16 == 0 && aligned(x, 16);
  i64 npass;
  const i64 grid = ab_grid(a.most, cols, &npass);
  if (!grid) return GLINT_EINVAL;
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS_AXPY, rows_axpy_batch_kernel<V>, (unsigned)grid, kTPB, st, a.f.key, a.f.items,
                  a.f.nitems, (const V*)a.cs, (int)a.qp, (const V*)x, (int)q, (int)npass, xw, (V*)s->data, s->part));
  return GLINT_OK;
}

template int push_rows_axpy_batch<float>(glint_shard*, const i64*, i64, const void*, const void*, i64, hipStream_t);
template int push_rows_axpy_batch<double>(glint_shard*, const i64*, i64, const void*, const void*, i64, hipStream_t);

}  // namespace glint
