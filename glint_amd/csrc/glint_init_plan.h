// glint_init_plan.h -- the value contract of the seeded uniform init (include/glint_gpu.h, "Shard fill and
// uniform init") as code: the counter-based generator, the bits-to-value mapping and the host's rounding
// of the range. An element's value is a function of (seed, global row, column, lo, hi, type) only, and
// this header is the one statement of that function: the kernel (glint_init.hip) and a CPU probe
// (tests/c/init_probe.cpp, for tests/test_init_cpu.py) both compile it. Plain C++17; the functions carry
// __host__ __device__ only under hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GLINT_INIT_FN __host__ __device__ __forceinline__
#else
#define GLINT_INIT_FN inline
#endif

namespace glint {

// Philox4x32-10 (Salmon et al., "Parallel random numbers: as easy as 1, 2, 3", SC'11): the standard
// multipliers and Weyl key increments
constexpr uint32_t kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u;
constexpr uint32_t kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;

struct PhiloxOut {
  uint32_t o[4];
};

// Ten rounds over counter (c0, c1, c2, c3) with key (k0, k1). Each round takes the two 32x32->64 products
// M0 * c0 and M1 * c2; the key is bumped between rounds, and depends on the seed alone (scalar in a kernel).
GLINT_INIT_FN PhiloxOut philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#if defined(__HIPCC__)
#pragma unroll
#endif
  for (int r = 0; r < 10; ++r) {
    const uint64_t p0 = (uint64_t)kPhiloxM0 * c0, p1 = (uint64_t)kPhiloxM1 * c2;
    const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
    c1 = (uint32_t)p1;
    c3 = (uint32_t)p0;
    c0 = n0;
    c2 = n2;
    k0 += kPhiloxW0;
    k1 += kPhiloxW1;
  }
  return PhiloxOut{{c0, c1, c2, c3}};
}

// values per 128-bit block: 4 Floats or 2 Doubles -- one block is one 16-B store for either type
template <typename V>
struct InitBlock;
template <>
struct InitBlock<float> {
  static constexpr int L = 4;
};
template <>
struct InitBlock<double> {
  static constexpr int L = 2;
};

// The block of element (g, c): counter (lo32(g), hi32(g), c / L, 0), key (lo32(seed), hi32(seed)).
template <typename V>
GLINT_INIT_FN PhiloxOut init_block(uint64_t seed, uint64_t g, uint32_t b) {
  return philox4x32_10((uint32_t)g, (uint32_t)(g >> 32), b, 0u, (uint32_t)seed, (uint32_t)(seed >> 32));
}

// Position j of a block as a value: u in [0, 1) from the top 24 (53) bits of one (two) output words --
// both conversions and both scalings by a power of two are exact -- then lo + (u * w) in V, the product
// rounded before the add (no fused multiply-add). The result lies in [lo, lo + w]; rounding may reach
// the upper end itself.
GLINT_INIT_FN float init_value(const PhiloxOut& p, int j, float lo, float w) {
#pragma clang fp contract(off)
  const float u = (float)(p.o[j] >> 8) * 0x1p-24f;
  const float t = u * w;
  return lo + t;
}
GLINT_INIT_FN double init_value(const PhiloxOut& p, int j, double lo, double w) {
#pragma clang fp contract(off)
  const uint64_t x = (uint64_t)p.o[2 * j] | ((uint64_t)p.o[2 * j + 1] << 32);
  const double u = (double)(x >> 11) * 0x1p-53;
  const double t = u * w;
  return lo + t;
}

// element (g, c) of a uniform init on its own (the probe's and a reader's form; the kernel takes a whole
// block at a time through the same two functions)
template <typename V>
GLINT_INIT_FN V init_uniform_elem(uint64_t seed, uint64_t g, uint32_t c, V lo, V w) {
  constexpr uint32_t L = (uint32_t)InitBlock<V>::L;
  return init_value(init_block<V>(seed, g, c / L), (int)(c % L), lo, w);
}

// What the host settles before a uniform init launches: lo and hi rounded once to V, w = hi - lo in V.
// False (GLINT_EINVAL) for a NaN or infinite bound after rounding, lo > hi, or a non-finite w.
template <typename V>
inline bool init_uniform_range(double lo, double hi, V* lo_v, V* w_v) {
  const V l = (V)lo, h = (V)hi;
  const V inf = __builtin_huge_val();
  if (!(l == l) || !(h == h) || l == inf || l == -inf || h == inf || h == -inf || l > h) return false;
  const V w = h - l;
  if (!(w == w) || w == inf) return false;
  *lo_v = l;
  *w_v = w;
  return true;
}

}  // namespace glint
