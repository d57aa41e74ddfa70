// sampler_probe.cpp -- the row sampler's value contract (glint_sample_plan.h) behind a C interface, for
// tests/test_sampler_cpu.py (ctypes): the same attempt, search and exclusion rule the kernel compiles, over a
// cdf in host memory. No GPU, no HIP.
#include "../../glint_amd/csrc/glint_sample_plan.h"

using namespace glint;

extern "C" {

// x of attempt t[i] of draw d[i] under seed[i], for n triples
void sampler_points(const uint64_t* seed, const uint64_t* d, const uint32_t* t, int64_t n, uint64_t total,
                    uint64_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = sample_point(seed[i], d[i], t[i], total);
}

// the smallest i with cdf[i] > x[k], for n points x[k] < cdf[m - 1]
void sampler_upper(const uint64_t* cdf, int64_t m, const uint64_t* x, int64_t n, int64_t* out) {
  const SampleFlat tab{cdf, m};
  for (int64_t i = 0; i < n; ++i) out[i] = tab.upper(x[i]);
}

// entry of attempt t[i] of draw d[i]
void sampler_attempts(const uint64_t* cdf, int64_t m, uint64_t seed, const uint64_t* d, const uint32_t* t, int64_t n,
                      int64_t* out) {
  const SampleFlat tab{cdf, m};
  for (int64_t i = 0; i < n; ++i) out[i] = sample_attempt(tab, cdf[m - 1], seed, d[i], t[i]);
}

// a call: the n draws from counter `first` as global keys; exclude NULL: no exclusion
void sampler_draw(const uint64_t* cdf, int64_t m, int64_t first_key, uint64_t seed, uint64_t first, int64_t n,
                  const int64_t* exclude, int64_t per, int64_t* out) {
  const SampleFlat tab{cdf, m};
  for (int64_t i = 0; i < n; ++i) {
    const int64_t forb = exclude ? sample_forbidden(exclude[i / per], first_key, m) : -1;
    out[i] = first_key + sample_draw(tab, cdf[m - 1], seed, first + (uint64_t)i, forb);
  }
}

int sampler_coarse_shift(int64_t m, int coarse) { return sample_coarse_shift(m, coarse); }

int sampler_max_tries(void) { return GLINT_SAMPLE_MAX_TRIES; }

}  // extern "C"
