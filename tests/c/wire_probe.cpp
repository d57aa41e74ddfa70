// wire_probe.cpp -- the narrow-format row transport's conversion contract (glint_wire_plan.h) behind a C
// interface, for tests/test_wire_cpu.py (ctypes): the integer conversions the GPU kernels are held to.
// No GPU, no HIP.
#include "../../glint_amd/csrc/glint_wire_plan.h"

using namespace glint;

extern "C" {

int wire_probe_supported(int dtype, int wire) { return wire_supported(dtype, wire) ? 1 : 0; }
int wire_probe_size(int wire) { return wire_size(wire); }

// narrowing: n bit patterns of the shard's type -> n of the wire type
void wire_narrow_f32_f16(const uint32_t* in, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wire_f32_to_f16(in[i]);
}
void wire_narrow_f32_bf16(const uint32_t* in, int64_t n, uint16_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wire_f32_to_bf16(in[i]);
}
void wire_narrow_f64_f32(const uint64_t* in, int64_t n, uint32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wire_f64_to_f32(in[i]);
}

// widening: n bit patterns of the wire type -> n of the shard's type
void wire_widen_f16_f32(const uint16_t* in, int64_t n, uint32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wire_f16_to_f32(in[i]);
}
void wire_widen_bf16_f32(const uint16_t* in, int64_t n, uint32_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wire_bf16_to_f32(in[i]);
}
void wire_widen_f32_f64(const uint32_t* in, int64_t n, uint64_t* out) {
  for (int64_t i = 0; i < n; ++i) out[i] = wire_f32_to_f64(in[i]);
}

}  // extern "C"
