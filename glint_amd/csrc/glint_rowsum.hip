// glint_rowsum.hip -- grouped row-sum pull (glint_mat_pull_rows_sum*, DESIGN.md "Row-sum pull"): the
// read-side mirror of rows_fold. The caller names groups of rows (a CSR-style grp_ptr over `rows`); the
// shard answers one row per group, the left-to-right sum of the group's rows in the shard's type, so a
// bag of rows costs g x cols values of answer instead of n x cols and a second pass.
//   rows_sum   one wave per (group, column slice): the first row's slice as it is stored, then every
//              further row's slice added strictly in list order -- ((r0 + r1) + r2) + ... -- with
//              kRowSumDepth row-slice loads in flight, and one store of the slice at the end.
// No atomics and no split of a group: column slices are disjoint and every (group, slice) has one wave,
// so the answer is deterministic and its order is the caller's.
#include "glint_device.h"
#include "glint_host.h"

namespace glint {

constexpr int kRowSumDepth = 8;  // row-slice loads in flight per wave (kRowsDepth's pattern: the adds are the only chain)

// Persistent grid; one wave per (group, column slice), the slices of a group on adjacent waves. A slice
// is 64 lanes x 16 B when VEC16 (cols * sizeof(V) a multiple of 16 and `out` 16-B aligned; the shard's
// pitch always is), else one element per lane. Only `cols` elements of a row are read, never the pitch
// padding. Every grp_ptr value is clamped to [0, n] and end < start is an empty group, so a malformed
// grp_ptr never indexes outside `rows`. A row outside the partition is a slice of zeros without a load,
// recorded once (by the wave of slice 0) under its index in `rows`.
template <typename V, bool VEC16>
__global__ __launch_bounds__(kTPB) void rows_sum_kernel(const i64* __restrict__ rows, i64 n,
                                                        const i64* __restrict__ grp_ptr, i64 g,
                                                        const V* __restrict__ data, PartDesc part,
                                                        V* __restrict__ out, ErrState* err) {
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
      if ((u32)lane < m) {
        const int32_t l = g2l(part, rows[b + lane]);
        if (l >= 0 && l < part.size) mine = l;
        else if (slice == 0) record_error(err, b + lane);
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
#pragma unroll
          for (int q = 0; q < VPL; ++q) acc[q] = first ? t[0][q] : vadd(acc[q], t[0][q]);
#pragma unroll
          for (int d = 1; d < kRowSumDepth; ++d)
#pragma unroll
            for (int q = 0; q < VPL; ++q) acc[q] = vadd(acc[q], t[d][q]);
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
#pragma unroll
          for (int q = 0; q < VPL; ++q) acc[q] = first ? t[0][q] : vadd(acc[q], t[0][q]);  // (j < m: row j exists)
#pragma unroll
          for (int d = 1; d < kRowSumDepth; ++d) {
            if (j + d < m) {
#pragma unroll
              for (int q = 0; q < VPL; ++q) acc[q] = vadd(acc[q], t[d][q]);
            }
          }
        }
      }
    }
    slice_store<V, VPL, VEC16>(acc, out + k * cols, c, cols);
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the row-sum pull on st (no host synchronisation): one launch. Under the shard's lock.
template <typename V>
int pull_rows_sum(glint_shard* s, const i64* rows, i64 n, const i64* grp_ptr, i64 g, void* out, hipStream_t st) {
  if (g <= 0) return GLINT_OK;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(out, 16);
  const i64 per = v16 ? 64 * (16 / (i64)sizeof(V)) : 64;  // elements per slice
  const i64 slices = ((i64)s->part.cols + per - 1) / per;
  const unsigned grid = grid_for(g * slices, kTPB / 64, (i64)s->cus * 8);
  HIPCHK(launch_k(s, GLINT_K_PULL_ROWS_SUM, v16 ? rows_sum_kernel<V, true> : rows_sum_kernel<V, false>, grid, kTPB,
                  st, rows, n, grp_ptr, g, (const V*)s->data, s->part, (V*)out, err_of(s)));
  return GLINT_OK;
}

template int pull_rows_sum<int>(glint_shard*, const i64*, i64, const i64*, i64, void*, hipStream_t);
template int pull_rows_sum<long long>(glint_shard*, const i64*, i64, const i64*, i64, void*, hipStream_t);
template int pull_rows_sum<float>(glint_shard*, const i64*, i64, const i64*, i64, void*, hipStream_t);
template int pull_rows_sum<double>(glint_shard*, const i64*, i64, const i64*, i64, void*, hipStream_t);

}  // namespace glint
