// glint_sample_plan.h -- the value contract of the seeded weighted row sampler (include/glint_gpu.h, "Row
// sampler") as code: which Philox block a draw takes, how its bits become a point of the cumulative table,
// which entry that point names and how an excluded key is avoided. A draw is a function of (weights,
// first_key, seed, counter, excluded key) only, and this header is the one statement of that function: the
// kernel (glint_sample.hip) and a CPU probe (tests/c/sampler_probe.cpp, for tests/test_sampler_cpu.py) both
// compile it. Everything is integer arithmetic, so every answer is bit-exact everywhere. Plain C++17; the
// functions carry __host__ __device__ only under hipcc. The generator is glint_init_plan.h's.
#pragma once
#include "glint_init_plan.h"

#ifndef GLINT_SAMPLE_MAX_TRIES
#define GLINT_SAMPLE_MAX_TRIES 8  // (include/glint_gpu.h)
#endif

namespace glint {

// floor(a * b / 2^64): the high half of the 128-bit product
GLINT_INIT_FN uint64_t sample_mulhi(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __umul64hi(a, b);
#else
  return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// The point of attempt t of draw d under seed: counter (lo32(d), hi32(d), t, 1) -- word 3 is 1 where the
// uniform init has 0, so the two streams of one seed are disjoint --, key (lo32(seed), hi32(seed)); r = the
// first two output words, low word first; x = floor(r * total / 2^64), so 0 <= x < total.
GLINT_INIT_FN uint64_t sample_point(uint64_t seed, uint64_t d, uint32_t t, uint64_t total) {
  const PhiloxOut p = philox4x32_10((uint32_t)d, (uint32_t)(d >> 32), t, 1u, (uint32_t)seed, (uint32_t)(seed >> 32));
  const uint64_t r = (uint64_t)p.o[0] | ((uint64_t)p.o[1] << 32);
  return sample_mulhi(r, total);
}

// The table as the contract sees it: cdf[i] = w[0] + ... + w[i] for m entries, cdf[m - 1] = total >= 1.
// upper(x) = the smallest i with cdf[i] > x, for x < total (so it exists, and its weight is not zero). A
// search of another shape (the kernel's two-level one) answers the same i for every x.
struct SampleFlat {
  const uint64_t* cdf;
  int64_t m;
  GLINT_INIT_FN uint64_t at(int64_t i) const { return cdf[i]; }
  GLINT_INIT_FN int64_t upper(uint64_t x) const {
    int64_t lo = 0, n = m;  // the answer lies in [lo, lo + n)
    while (n > 1) {
      const int64_t h = n >> 1;
      if (cdf[lo + h - 1] <= x) {
        lo += h;
        n -= h;
      } else {
        n = h;
      }
    }
    return lo;
  }
};

// entry of attempt t of draw d
template <typename Table>
GLINT_INIT_FN int64_t sample_attempt(const Table& tab, uint64_t total, uint64_t seed, uint64_t d, uint32_t t) {
  return tab.upper(sample_point(seed, d, t, total));
}

// The entry of draw d that avoids entry `forb` (an index into the table), given the entry i0 of its attempt
// 0. Attempts 1 .. GLINT_SAMPLE_MAX_TRIES - 1 are made in order and the first that differs from forb is the
// draw; if all hit forb, the draw is the next entry of non-zero weight after it, cyclically:
// upper(cdf[forb] mod total). That is forb again only when forb is the table's only non-zero entry.
template <typename Table>
GLINT_INIT_FN int64_t sample_avoid(const Table& tab, uint64_t total, uint64_t seed, uint64_t d, int64_t forb,
                                   int64_t i0) {
  int64_t i = i0;
  for (uint32_t t = 1; i == forb && t < GLINT_SAMPLE_MAX_TRIES; ++t) i = sample_attempt(tab, total, seed, d, t);
  if (i != forb) return i;
  const uint64_t c = tab.at(forb);
  return tab.upper(c >= total ? c - total : c);  // (c <= total)
}

// The excluded entry of a draw: the global key forb_key as an index of the table, or -1 -- which no attempt
// equals -- when it lies outside [first_key, first_key + m) and so excludes nothing.
GLINT_INIT_FN int64_t sample_forbidden(int64_t forb_key, int64_t first_key, int64_t m) {
  // (in unsigned arithmetic: the difference of two keys far apart must not overflow)
  const uint64_t off = (uint64_t)forb_key - (uint64_t)first_key;
  return off < (uint64_t)m ? (int64_t)off : -1;
}

// Draw d as an entry of the table: attempt 0, or with exclusion (forb >= 0) the rule of sample_avoid.
template <typename Table>
GLINT_INIT_FN int64_t sample_draw(const Table& tab, uint64_t total, uint64_t seed, uint64_t d, int64_t forb) {
  const int64_t i0 = sample_attempt(tab, total, seed, d, 0u);
  return i0 == forb ? sample_avoid(tab, total, seed, d, forb, i0) : i0;
}

// ---- the coarse table's geometry (glint_sample.hip; tests size their cases by it, bits never depend on it) ----
// The m entries are cut into blocks of 2^shift entries, shift the least with coarse << shift >= m, and coarse
// entry j = the cdf at the end of block j, min(((j + 1) << shift) - 1, m - 1): so the entries past the last
// block repeat the total. The smallest j with coarse[j] > x names the block that holds upper(x), because
// every entry of the blocks before it is <= coarse[j - 1] <= x: a run of equal cdf values that spans a
// block boundary is followed to its end by the comparison `<= x` at both levels.
inline int sample_coarse_shift(int64_t m, int coarse) {
  int s = 0;
  while (((int64_t)coarse << s) < m) ++s;
  return s;
}

}  // namespace glint
