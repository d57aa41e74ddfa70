// glint_wire_plan.h -- the conversion contract of the narrow-format row transport (include/glint_gpu.h,
// "Narrow-format row transport") as code: which (shard type, wire type) pairs exist, and the two
// conversions of each pair on bit patterns, in integer arithmetic only -- no floating-point instruction,
// so neither a rounding mode nor a flush-to-zero mode can change an answer.
//   narrow  V -> W, what a pull does: one IEEE round-to-nearest-even of the stored value straight to W.
//           Subnormal results are kept; a magnitude that rounds beyond W's largest finite value becomes
//           the infinity of its sign; infinities and a zero's sign are kept; a value below half of W's
//           smallest subnormal, and the tie at exactly half of it, becomes the zero of its sign; a NaN
//           becomes a quiet NaN of W (here: the sign kept, the top payload bits kept -- unspecified by the
//           contract).
//   widen   W -> V, what a push does: exact. W's subnormals become the equal (normal) V values, -0 stays
//           -0, infinities stay infinities, a NaN becomes a quiet NaN.
// This header is the one statement of those functions: a CPU probe (tests/c/wire_probe.cpp, for
// tests/test_wire_cpu.py) compiles it, and the kernels (glint_rowwire.hip) are held to it bit for bit by
// tests/test_gpu_wire.py. Plain C++17; the functions carry __host__ __device__ only under hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GLINT_WIRE_FN __host__ __device__ __forceinline__
#else
#define GLINT_WIRE_FN inline
#endif

namespace glint {

// enum glint_wire / enum glint_dtype of include/glint_gpu.h, restated so that the header stands alone
constexpr int kWireF16 = 0, kWireBF16 = 1, kWireF32 = 2;
constexpr int kWireDtypeF32 = 2, kWireDtypeF64 = 3;

// (Float, F16), (Float, BF16), (Double, F32); every other pair -- any Int or Long shard -- does not exist
GLINT_WIRE_FN bool wire_supported(int dtype, int wire) {
  return (dtype == kWireDtypeF32 && (wire == kWireF16 || wire == kWireBF16)) ||
         (dtype == kWireDtypeF64 && wire == kWireF32);
}

// bytes of one wire element; 0 for an unknown wire type
GLINT_WIRE_FN int wire_size(int wire) { return wire == kWireF16 || wire == kWireBF16 ? 2 : (wire == kWireF32 ? 4 : 0); }

// A binary floating format as its field widths: 1 sign bit, E exponent bits, M mantissa bits.
//   f16: E 5, M 10   bf16: E 8, M 7   f32: E 8, M 23   f64: E 11, M 52
// Narrowing (SE, SM) -> (DE, DM) with DE <= SE and DM < SM, on the source's bits in a u64; the result in
// the low 1 + DE + DM bits.
template <int SE, int SM, int DE, int DM>
GLINT_WIRE_FN uint64_t wire_narrow_bits(uint64_t u) {
  constexpr int kShift = SM - DM;                                   // mantissa bits dropped by a normal result
  constexpr int kSBias = (1 << (SE - 1)) - 1, kDBias = (1 << (DE - 1)) - 1;
  constexpr uint64_t kSExpMax = ((uint64_t)1 << SE) - 1, kDExpMax = ((uint64_t)1 << DE) - 1;
  const uint64_t sign = (u >> (SE + SM)) & 1;
  const uint64_t exp = (u >> SM) & kSExpMax;
  const uint64_t man = u & (((uint64_t)1 << SM) - 1);
  const uint64_t dsign = sign << (DE + DM);
  if (exp == kSExpMax) {  // infinity, or a NaN: quiet, its top payload bits kept
    if (man == 0) return dsign | (kDExpMax << DM);
    return dsign | (kDExpMax << DM) | ((uint64_t)1 << (DM - 1)) | (man >> kShift);
  }
  // the value is sig * 2^(e - SM) with e the unbiased exponent of a normal (the smallest one for a
  // subnormal source, whose sig has no hidden bit)
  const int64_t e = (exp ? (int64_t)exp : 1) - kSBias;
  const uint64_t sig = exp ? man | ((uint64_t)1 << SM) : man;
  // the destination's exponent field if the result is normal; <= 0: it is subnormal (or zero), and its
  // mantissa is the value in units of 2^(1 - kDBias - DM)
  const int64_t de = e + kDBias;
  int64_t drop = kShift;  // low bits of sig below the result's last place
  if (de <= 0) drop += 1 - de;
  if (drop > SM + 2) return dsign;  // below half of the smallest subnormal (sig < 2^(SM+1)): the zero
  const uint64_t kept = sig >> drop;
  const uint64_t rest = sig & (((uint64_t)1 << drop) - 1), half = (uint64_t)1 << (drop - 1);
  const uint64_t up = rest > half || (rest == half && (kept & 1)) ? 1 : 0;  // to nearest, ties to even
  // `kept` holds the hidden bit when the result is normal: adding (de - 1) << DM puts the exponent field
  // right, and a carry out of the mantissa steps to the next exponent (up to the infinity) by itself;
  // a subnormal that rounds up to the smallest normal carries into exponent field 1 the same way
  const uint64_t mag = (de > 0 ? (uint64_t)(de - 1) << DM : 0) + kept + up;
  if (mag >= (kDExpMax << DM)) return dsign | (kDExpMax << DM);  // beyond the largest finite value
  return dsign | mag;
}

// Widening (SE, SM) -> (DE, DM) with DE >= SE and DM > SM (DE > SE wherever the source has subnormals
// that the destination must hold as normals: f16 -> f32, f32 -> f64; bf16 -> f32 keeps them subnormal).
template <int SE, int SM, int DE, int DM>
GLINT_WIRE_FN uint64_t wire_widen_bits(uint64_t u) {
  constexpr int kShift = DM - SM;
  constexpr int kSBias = (1 << (SE - 1)) - 1, kDBias = (1 << (DE - 1)) - 1;
  constexpr uint64_t kSExpMax = ((uint64_t)1 << SE) - 1, kDExpMax = ((uint64_t)1 << DE) - 1;
  const uint64_t sign = (u >> (SE + SM)) & 1;
  const uint64_t exp = (u >> SM) & kSExpMax;
  uint64_t man = u & (((uint64_t)1 << SM) - 1);
  const uint64_t dsign = sign << (DE + DM);
  if (exp == kSExpMax)  // infinity, or a NaN made quiet
    return dsign | (kDExpMax << DM) | (man ? ((uint64_t)1 << (DM - 1)) | (man << kShift) : 0);
  if (exp != 0) return dsign | ((exp + (uint64_t)(kDBias - kSBias)) << DM) | (man << kShift);
  if (man == 0) return dsign;
  if (DE == SE) return dsign | (man << kShift);  // the same exponent range: still subnormal
  // a subnormal source: normalise. man * 2^(1 - kSBias - SM), its top set bit moved up to the hidden bit
  int64_t de = 1 - kSBias + kDBias;
  while (!(man & ((uint64_t)1 << SM))) {
    man <<= 1;
    --de;
  }
  return dsign | ((uint64_t)de << DM) | ((man & (((uint64_t)1 << SM) - 1)) << kShift);
}

// ---- the three pairs -----------------------------------------------------------------------------------
GLINT_WIRE_FN uint16_t wire_f32_to_f16(uint32_t u) { return (uint16_t)wire_narrow_bits<8, 23, 5, 10>(u); }
GLINT_WIRE_FN uint32_t wire_f16_to_f32(uint16_t h) { return (uint32_t)wire_widen_bits<5, 10, 8, 23>(h); }

// BF16 is the float's upper half; for every non-NaN the rounding is (u + 0x7FFF + ((u >> 16) & 1)) >> 16
GLINT_WIRE_FN uint16_t wire_f32_to_bf16(uint32_t u) {
  if ((u & 0x7FFFFFFFu) > 0x7F800000u) return (uint16_t)((u >> 16) | 0x0040u);  // a NaN, made quiet
  return (uint16_t)((u + 0x7FFFu + ((u >> 16) & 1u)) >> 16);
}
GLINT_WIRE_FN uint32_t wire_bf16_to_f32(uint16_t b) {
  const uint32_t u = (uint32_t)b << 16;
  return (u & 0x7FFFFFFFu) > 0x7F800000u ? u | 0x00400000u : u;
}

GLINT_WIRE_FN uint32_t wire_f64_to_f32(uint64_t u) { return (uint32_t)wire_narrow_bits<11, 52, 8, 23>(u); }
GLINT_WIRE_FN uint64_t wire_f32_to_f64(uint32_t f) { return wire_widen_bits<8, 23, 11, 52>(f); }

}  // namespace glint
