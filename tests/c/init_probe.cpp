// init_probe.cpp -- the uniform init's value contract (glint_init_plan.h) behind a C interface, for
// tests/test_init_cpu.py (ctypes): the same generator and bits-to-value mapping the kernel compiles.
// No GPU, no HIP.
#include "../../glint_amd/csrc/glint_init_plan.h"

using namespace glint;

extern "C" {

// Philox4x32-10 of one counter and key
void init_philox(const uint32_t* ctr, const uint32_t* key, uint32_t* out) {
  const PhiloxOut p = philox4x32_10(ctr[0], ctr[1], ctr[2], ctr[3], key[0], key[1]);
  for (int i = 0; i < 4; ++i) out[i] = p.o[i];
}

// element (g[i], c[i]) under seed[i] for n triples; lo and w are already of the shard's type
void init_elems_f32(const uint64_t* seed, const uint64_t* g, const uint32_t* c, int64_t n, float lo, float w,
                    float* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = init_uniform_elem<float>(seed[i], g[i], c[i], lo, w);
}
void init_elems_f64(const uint64_t* seed, const uint64_t* g, const uint32_t* c, int64_t n, double lo, double w,
                    double* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = init_uniform_elem<double>(seed[i], g[i], c[i], lo, w);
}

// every position of a block whose output words are given (forced to all ones or to zero by the test)
void init_values_f32(const uint32_t* words, float lo, float w, float* out) {
  const PhiloxOut p{{words[0], words[1], words[2], words[3]}};
  for (int j = 0; j < 4; ++j) out[j] = init_value(p, j, lo, w);
}
void init_values_f64(const uint32_t* words, double lo, double w, double* out) {
  const PhiloxOut p{{words[0], words[1], words[2], words[3]}};
  for (int j = 0; j < 2; ++j) out[j] = init_value(p, j, lo, w);
}

// the host's rounding of the range: 1 and (lo, w) in the shard's type, or 0 where the call is refused
int init_range_f32(double lo, double hi, float* lo_v, float* w_v) { return init_uniform_range<float>(lo, hi, lo_v, w_v); }
int init_range_f64(double lo, double hi, double* lo_v, double* w_v) {
  return init_uniform_range<double>(lo, hi, lo_v, w_v);
}

}  // extern "C"
