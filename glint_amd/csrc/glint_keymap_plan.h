// glint_keymap_plan.h -- what the device key map's kernels (glint_keymap.hip) and its host side share
// (include/glint_gpu.h, "Key map"): the slot's two marks, the hash, the default table size and the layout of
// a call's scratch. None of it reaches an answer: rows are a function of the insert calls and their keys
// only, whatever the hash and the table size. Plain C++17; the functions carry __host__ __device__ only
// under hipcc.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define GLINT_KEYMAP_FN __host__ __device__ __forceinline__
#else
#define GLINT_KEYMAP_FN inline
#endif

namespace glint {

// A slot is (key, val), 16 bytes, 16-byte aligned: one probe is one 16-byte load, and linear probing keeps
// the next seven slots of a chain in the same 128-byte line.
//   empty      key = kKeymapEmptyKey (the reserved key), val = kKeymapEmptyVal
//   claimed    key set, val = kKeymapTentative + the lowest index of a record of the running insert that
//              names the key (only while that insert runs)
//   committed  key set, val = the key's row, below kKeymapTentative
constexpr int64_t kKeymapEmptyKey = INT64_MIN;
constexpr uint64_t kKeymapEmptyVal = (uint64_t)INT64_MAX;
constexpr uint64_t kKeymapTentative = (uint64_t)1 << 62;
constexpr int64_t kKeymapMaxSlots = (int64_t)1 << 30;

// where a key's chain starts, before the mask: the splitmix64 finaliser
GLINT_KEYMAP_FN uint64_t keymap_hash(int64_t key) {
  uint64_t x = (uint64_t)key;
  x ^= x >> 30;
  x *= 0xbf58476d1ce4e5b9ull;
  x ^= x >> 27;
  x *= 0x94d049bb133111ebull;
  x ^= x >> 31;
  return x;
}

// the least power of two >= 2 * capacity (capacity >= 1; 0 when that is above kKeymapMaxSlots)
inline int64_t keymap_default_slots(int64_t capacity) {
  int64_t s = 2;
  while (s < kKeymapMaxSlots && s / 2 < capacity) s <<= 1;
  return s / 2 >= capacity ? s : 0;
}

// whether (capacity, first_row, slots) is a table include/glint_gpu.h allows
inline bool keymap_geometry_ok(int64_t capacity, int64_t first_row, int64_t slots) {
  return capacity >= 1 && slots > capacity && slots <= kKeymapMaxSlots && (slots & (slots - 1)) == 0 &&
         first_row >= 0 && first_row <= (int64_t)kKeymapTentative - capacity;
}

// ---- a call's scratch, in 32-bit words: claim[n] | rank[n] | the rank scan's tile sums, level by level ----
constexpr int kKeymapScanTile = 1024;  // records one scan workgroup covers
inline size_t keymap_scan_words(int64_t n) {
  size_t words = 0;
  int64_t t = n;
  while (t > kKeymapScanTile) {
    t = (t + kKeymapScanTile - 1) / kKeymapScanTile;
    words += (size_t)t;
  }
  return words;
}
inline size_t keymap_scratch_words(int64_t n) { return 2 * (size_t)n + keymap_scan_words(n); }

}  // namespace glint
