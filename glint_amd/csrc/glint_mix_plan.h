// glint_mix_plan.h -- how a batched row mix pull (glint_rowmix_batch.hip) splits its K, the request list,
// into chunks: a pure function of n, stated in include/glint_gpu.h because the chunk boundaries are part of
// the answer's bits. Nothing here reads the device, q, cols or the grid. Plain C++17, no HIP.
#pragma once
#include "glint_push_plan.h"  // i64

namespace glint {

static_assert(GLINT_MIX_BATCH_CHUNK >= 32 && (GLINT_MIX_BATCH_CHUNK & (GLINT_MIX_BATCH_CHUNK - 1)) == 0,
              "a chunk is a power-of-two number of whole slabs");
static_assert(GLINT_MIX_BATCH_MAX_CHUNKS >= 1, "at least one chunk");

// L = GLINT_MIX_BATCH_CHUNK * 2^e, e the smallest integer >= 0 with ceil(n / L) <= GLINT_MIX_BATCH_MAX_CHUNKS
inline i64 mix_chunk_len(i64 n) {
  i64 len = GLINT_MIX_BATCH_CHUNK;
  while ((n + len - 1) / len > GLINT_MIX_BATCH_MAX_CHUNKS) len *= 2;
  return len;
}

// chunks of a call of n requests: chunk k takes requests [k L, min(n, (k + 1) L)); n <= 0 has none
inline i64 mix_chunk_count(i64 n) {
  if (n <= 0) return 0;
  const i64 len = mix_chunk_len(n);
  return (n + len - 1) / len;
}

}  // namespace glint
