// glint_rowsum.hip -- grouped row-sum pull (glint_mat_pull_rows_sum*, DESIGN.md "Row-sum pull"): the
// read-side mirror of rows_fold. The caller names groups of rows (a CSR-style grp_ptr over `rows`); the
// shard answers one row per group, the left-to-right sum of the group's rows in the shard's type, so a
// bag of rows costs g x cols values of answer instead of n x cols and a second pass.
//   rows_sum   one wave per (group, column slice): the first row's slice as it is stored, then every
//              further row's slice added strictly in list order -- ((r0 + r1) + r2) + ... -- with
//              kRowSumDepth row-slice loads in flight, and one store of the slice at the end. With a
//              coefficient per record (glint_mat_pull_rows_wsum*, DESIGN.md "Weighted row-sum pull and
//              grouped row dot") every term is coef[i] * row, the product rounded before the add.
// No atomics and no split of a group: column slices are disjoint and every (group, slice) has one wave,
// so the answer is deterministic and its order is the caller's.
#include "glint_axpy.h"  // axpy_mul, axpy_add, lane_get: the weighted sum's product, shared with the axpy pushes
#include "glint_host.h"

namespace glint {

constexpr int kRowSumDepth = 8;  // row-slice loads in flight per wave (kRowsDepth's pattern: the adds are the only chain)

// The weighted sum's term of the record in lane r of a batch: its row's slice t times the coefficient
// lane r holds, each product rounded on its own. r is wave-uniform. (The lane of a row outside the
// partition holds 1, see the kernel: its slice of zeros stays +0 / 0 without a branch here.)
template <typename V, int VPL>
__device__ __forceinline__ void rows_sum_scale(V (&t)[VPL], V cf, u32 r) {
  const V cd = lane_get(cf, r);
#pragma unroll
  for (int q = 0; q < VPL; ++q) t[q] = axpy_mul(cd, t[q]);
}

// acc + term: the unweighted sum's vadd, and for the weighted sum axpy_add, which no product fuses into
template <bool COEF, typename V>
__device__ __forceinline__ V rows_sum_add(V acc, V term) {
  if (COEF) return axpy_add(acc, term);
  return vadd(acc, term);
}

// Persistent grid; one wave per (group, column slice), the slices of a group on adjacent waves. A slice
// is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple of 16 and `out` 16-B aligned; the shard's
// pitch always is), else one element per lane. Only `cols` elements of a row are read, never the pitch
// padding. Every grp_ptr value is clamped to [0, n] and end < start is an empty group, so a malformed
// grp_ptr never indexes outside `rows`. A row outside the partition is a slice of zeros without a load,
// recorded once (by the wave of slice 0) under its index in `rows`.
//
// COEF (glint_mat_pull_rows_wsum*): the term of record i is coef[i] * its row's slice, the product rounded
// before it is added (axpy_mul / axpy_add: no fused multiply-add), and the first term is the first product
// as computed. Every lane loads its own record's coefficient beside its row id and lane_get hands it round
// with the id (rows_group_batch's pattern). A row outside the partition is the term +0 / 0 whatever its
// coefficient: its row is not loaded and its coefficient is not read -- its lane holds 1 instead, and
// 1 * +0 is +0, so the walk needs no branch per record and an infinite coefficient makes no NaN. Without
// COEF `coef` is not read and the code is the unweighted
// kernel's, instruction for instruction (`coef` is the last argument, so no other argument moves).
template <typename V, bool VEC16, bool COEF>
__global__ __launch_bounds__(kTPB) void rows_sum_kernel(const i64* __restrict__ rows, i64 n,
                                                        const i64* __restrict__ grp_ptr, i64 g,
                                                        const V* __restrict__ data, PartDesc part,
                                                        V* __restrict__ out, ErrState* err,
                                                        const V* __restrict__ coef) {
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the group, its bounds and the row ids handed round are then
  // wave-uniform to the compiler too (scalar loads and addresses, no per-lane copies)
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const u32 nslices = (u32)((cols + 64 * VPL - 1) / (64 * VPL));
  const u64 total = (u64)g * nslices;
  for (u64 w = w0; w < total; w += nw) {
    const i64 k = (i64)(w / nslices);
    const u32 slice = (u32)(w % nslices);
    i64 beg = grp_ptr[k], end = grp_ptr[k + 1];
    beg = beg < 0 ? 0 : (beg > n ? n : beg);
    end = end < 0 ? 0 : (end > n ? n : end);
    if (end < beg) end = beg;
    const i64 c = (i64)slice * 64 * VPL + (i64)lane * VPL;
    V acc[VPL];
#pragma unroll
    for (int q = 0; q < VPL; ++q) acc[q] = V(0);  // an empty group: +0 / 0
    for (i64 b = beg; b < end; b += 64) {
      const u32 m = end - b < 64 ? (u32)(end - b) : 64u;
      // 64 row ids, one per lane: each lane maps and tests its own; -1 = outside the partition
      int32_t mine = -1;
      V cf = V(1);  // COEF: this lane's record's coefficient; 1 for a row outside the partition
      if ((u32)lane < m) {
        const int32_t l = g2l(part, rows[b + lane]);
        if (l >= 0 && l < part.size) mine = l;
        else if (slice == 0) record_error(err, b + lane);
        if (COEF && mine >= 0) cf = coef[b + lane];
      }
      for (u32 j = 0; j < m; j += kRowSumDepth) {
        // the group's first row is the first term as it is stored (not 0 + r0): -0.0, a NaN's bits
        const bool first = b == beg && j == 0;
        V t[kRowSumDepth][VPL];
        if (m - j >= (u32)kRowSumDepth) {
#pragma unroll
          for (int d = 0; d < kRowSumDepth; ++d) {
            const int32_t l = __builtin_amdgcn_readlane(mine, (int)(j + d));
            if (l >= 0) {
              slice_load<V, VPL, VEC16>(t[d], data + (i64)l * part.pitch, c, cols);
            } else {
#pragma unroll
              for (int q = 0; q < VPL; ++q) t[d][q] = V(0);
            }
          }
          if (COEF) {
#pragma unroll
            for (int d = 0; d < kRowSumDepth; ++d) rows_sum_scale<V, VPL>(t[d], cf, j + d);
          }
#pragma unroll
          for (int q = 0; q < VPL; ++q) acc[q] = first ? t[0][q] : rows_sum_add<COEF>(acc[q], t[0][q]);
#pragma unroll
          for (int d = 1; d < kRowSumDepth; ++d)
#pragma unroll
            for (int q = 0; q < VPL; ++q) acc[q] = rows_sum_add<COEF>(acc[q], t[d][q]);
        } else {  // the group's last few rows (wave-uniform tests)
#pragma unroll
          for (int d = 0; d < kRowSumDepth; ++d) {
            if (j + d < m) {
              const int32_t l = __builtin_amdgcn_readlane(mine, (int)(j + d));
              if (l >= 0) {
                slice_load<V, VPL, VEC16>(t[d], data + (i64)l * part.pitch, c, cols);
              } else {
#pragma unroll
                for (int q = 0; q < VPL; ++q) t[d][q] = V(0);
              }
            }
          }
          if (COEF) {
#pragma unroll
            for (int d = 0; d < kRowSumDepth; ++d) {
              if (j + d < m) rows_sum_scale<V, VPL>(t[d], cf, j + d);
            }
          }
#pragma unroll
          for (int q = 0; q < VPL; ++q)
            acc[q] = first ? t[0][q] : rows_sum_add<COEF>(acc[q], t[0][q]);  // (j < m: row j exists)
#pragma unroll
          for (int d = 1; d < kRowSumDepth; ++d) {
            if (j + d < m) {
#pragma unroll
              for (int q = 0; q < VPL; ++q) acc[q] = rows_sum_add<COEF>(acc[q], t[d][q]);
            }
          }
        }
      }
    }
    slice_store<V, VPL, VEC16>(acc, out + k * cols, c, cols);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the row-sum pull on st (no host synchronisation): one launch. coef == nullptr is the unweighted
// sum, else the weighted one. Under the shard's lock.
template <typename V>
int pull_rows_sum(glint_shard* s, const i64* rows, i64 n, const i64* grp_ptr, i64 g, const void* coef, void* out,
                  hipStream_t st) {
  if (g <= 0) return GLINT_OK;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(out, 16);
  const i64 per = v16 ? 64 * (16 / (i64)sizeof(V)) : 64;  // elements per slice
  const i64 slices = ((i64)s->part.cols + per - 1) / per;
  const unsigned grid = grid_for(g * slices, kTPB / 64, (i64)s->cus * 8);
  void (*k)(const i64*, i64, const i64*, i64, const V*, PartDesc, V*, ErrState*, const V*);
  if (coef) k = v16 ? rows_sum_kernel<V, true, true> : rows_sum_kernel<V, false, true>;
  else k = v16 ? rows_sum_kernel<V, true, false> : rows_sum_kernel<V, false, false>;
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SUM, k, grid, kTPB, st, rows, n, grp_ptr, g, (const V*)s->data, s->part,
                  (V*)out, err_of(s), (const V*)coef));
  return GLINT_OK;
}

template int pull_rows_sum<int>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);
template int pull_rows_sum<long long>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);
template int pull_rows_sum<float>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);
template int pull_rows_sum<double>(glint_shard*, const i64*, i64, const i64*, i64, const void*, void*, hipStream_t);

}  // namespace glint
