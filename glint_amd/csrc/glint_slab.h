// glint_slab.h -- the slab geometry and the staging load of the two matrix-instruction kernels, the batched
// top-k pull's scores (glint_topk_batch.hip) and the batched row dot pull (glint_rowdot_batch.hip). A slab is
// 128 bytes of K (32 Float / 16 Double columns) of a tile's 128 table rows and of a pass's 64 caller vectors:
// 192 lines of 128 B, each at a pitch of 144 B in LDS. Thread t stages 16-B chunk t % 8 of lines
// t / 8 + 32 p, p = 0..5. Both kernels walk K in the same slabs, groups and steps, which is what makes a
// score's bits the same in both (include/glint_gpu.h).
#pragma once
#include "glint_kernels.h"

namespace glint {

constexpr int kTbRows = 128;                    // table rows of a tile
constexpr int kTbPass = 64;                     // caller vectors of a pass
constexpr int kTbLines = kTbRows + kTbPass;     // lines of a slab: the tile's rows, then the vectors
constexpr int kTbLineBytes = 128;               // K bytes of a slab
constexpr int kTbLinePitch = kTbLineBytes + 16; // bytes between lines in LDS
constexpr int kTbSlabBytes = kTbLines * kTbLinePitch;
constexpr int kTbStage = kTbLines / 32;         // chunks a thread stages per slab
static_assert(kTbRows == 32 * (kTPB / 64), "a wave owns 32 rows of the tile");
static_assert(kTbLines % 32 == 0 && kTPB == 32 * (kTbLineBytes / 16), "a thread stages one chunk of 32 lines apart");

typedef __attribute__((ext_vector_type(4))) unsigned int TbU4;
typedef __attribute__((ext_vector_type(4))) float TbF4;
typedef __attribute__((ext_vector_type(16))) float TbF16;
typedef __attribute__((ext_vector_type(2))) double TbD2;
typedef __attribute__((ext_vector_type(4))) double TbD4;

// One 16-B chunk of a line, columns [c, c + E): zero when the line is a pad or c >= cols; one 16-B load
// when the chunk is whole and the line allows it; else the elements below cols one by one.
template <typename V>
__device__ __forceinline__ TbU4 tb_chunk(const V* __restrict__ line, i64 c, i64 cols, bool live, bool wide) {
  constexpr int E = (int)(16 / sizeof(V));
  TbU4 r = {0u, 0u, 0u, 0u};
  if (!live || c >= cols) return r;
  if (wide && c + E <= cols) return *reinterpret_cast<const TbU4*>(line + c);
  V e[E];
#pragma unroll
  for (int k = 0; k < E; ++k) e[k] = c + k < cols ? line[c + k] : V(0);
  __builtin_memcpy(&r, e, 16);
  return r;
}

}  // namespace glint
