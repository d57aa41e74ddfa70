// glint_group.h -- how a device caller's group pointer is read (the contracts in include/glint_gpu.h,
// "Grouped row push" and "Grouped row-dot pull"), shared by the grouped row push (glint_rowgroup.hip) and
// the grouped row-dot pull (glint_rowdot.hip): the clamp of a grp_ptr value and the group of a record.
// One statement of the rule, so the write side and the read side cannot disagree about a record's group.
#pragma once
#include "glint_device.h"

namespace glint {

// grp_ptr[k] clamped to [0, n]: what every read of a device caller's group pointer goes through
__device__ __forceinline__ i64 group_cut(const i64* __restrict__ grp_ptr, i64 k, i64 n) {
  const i64 v = grp_ptr[k];
  return v < 0 ? 0 : (v > n ? n : v);
}

// The group of record i: the k in [0, g) with cut[k] <= i < cut[k+1], or -1 when no group covers it, by
// an upper-bound search over cut[0 .. g] (the first position whose cut exceeds i; at most 32 dependent
// 8-B loads, g < 2^31). Groups that are empty are stepped over: their cuts do not exceed i. Only
// grp_ptr[0 .. g] is read and the answer lies in [-1, g), whatever the array holds.
__device__ __forceinline__ int32_t group_find(const i64* __restrict__ grp_ptr, i64 g, i64 n, i64 i) {
  i64 lo = 0, hi = g + 1;  // the answer lies in [lo, hi]
  while (lo < hi) {
    const i64 mid = lo + (hi - lo) / 2;
    if (group_cut(grp_ptr, mid, n) > i) hi = mid;
    else lo = mid + 1;
  }
  return lo >= 1 && lo <= g ? (int32_t)(lo - 1) : -1;
}

}  // namespace glint
