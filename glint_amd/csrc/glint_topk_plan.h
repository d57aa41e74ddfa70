// glint_topk_plan.h -- what a top-k pull (glint_topk.hip pull_topk) settles on the host before it
// launches: the selection levels, their tiles, what each tile emits and where every buffer lies in the
// shard's scratch. A pure function of (size, q, k, value size): nothing here reads the device or touches
// a glint_shard, so it is tested on a CPU (tests/test_topk_cpu.py through tests/c/topk_probe.cpp).
// Plain C++17, no HIP.
//
// Level 0 selects from the scores: per query, tile t takes rows [t * T, min(size, (t + 1) * T)) and emits
// its best min(k, count) as (rank key, local row) pairs. Every tile but the last of a level is full
// (count == T >= k), so it emits exactly k and tile t's output starts at pair t * k of its query: the
// outputs of a level are dense, and they are the next level's input. A level with one tile per query is
// the last: it writes the caller's arrays instead. A level of more than one tile takes n > T pairs and
// leaves ceil(n / T) * k <= n / 4 + k < n / 2 (k <= T / 4 < n / 4), so the levels end; at k == T / 4 a
// level shrinks its input 4x.
#pragma once
#include "glint_push_plan.h"  // i64 / u64, pad256

namespace glint {

constexpr i64 kTopkTile = GLINT_TOPK_TILE;
static_assert(GLINT_TOPK_MAX_K * 4 <= GLINT_TOPK_TILE, "a full tile emits k <= T / 4 pairs: the levels shrink");
static_assert((GLINT_TOPK_TILE & (GLINT_TOPK_TILE - 1)) == 0, "the bitonic network sorts a power of two");
// n < 2^31 halves per level until it is <= T = 2^12: fewer than 20 levels
constexpr int kTopkMaxLevels = 20;

struct TopkLevel {
  i64 n_in;     // candidates per query this level selects from (level 0: the shard's rows)
  i64 tiles;    // workgroups per query: ceil(n_in / T), at least 1
  i64 n_out;    // pairs per query it emits: k per full tile, min(k, count) for the last
  // byte offsets in the scratch of this level's input and output pair arrays, [q][n] each: keys of
  // key_bytes, rows of 4 bytes. Level 0 has no input arrays (it reads the scores), the last level no
  // output arrays (it writes the caller's): those offsets are 0 and unused.
  u64 in_key, in_row, out_key, out_row;
};

struct TopkPlan {
  int levels;        // 1 .. kTopkMaxLevels; 0 = the arguments are out of range
  u64 scores_bytes;  // the scores [q][size] lie at offset 0
  u64 total_bytes;   // the scratch the call needs
  TopkLevel level[kTopkMaxLevels];
};

// what tile t of a level over n candidates selects from, and what it emits
inline i64 topk_tile_count(i64 n, i64 t) {
  const i64 left = n - t * kTopkTile;
  return left < 0 ? 0 : (left < kTopkTile ? left : kTopkTile);
}
inline i64 topk_tile_emits(i64 n, i64 t, i64 k) {
  const i64 c = topk_tile_count(n, t);
  return c < k ? c : k;
}

// vsize: bytes of a score (4 or 8); the rank key has the same width
inline TopkPlan topk_plan(i64 size, i64 q, i64 k, i64 vsize) {
  TopkPlan p{};
  if (size < 0 || size >= ((i64)1 << 31) || q < 1 || q > GLINT_TOPK_MAX_QUERIES || k < 1 || k > GLINT_TOPK_MAX_K ||
      (vsize != 4 && vsize != 8))
    return p;
  p.scores_bytes = (u64)q * (u64)size * (u64)vsize;
  u64 off = pad256((size_t)p.scores_bytes);
  i64 n = size;
  int l = 0;
  for (;; ++l) {
    if (l == kTopkMaxLevels) {  // (cannot happen: see the bound above)
      p.levels = 0;
      return p;
    }
    TopkLevel& lv = p.level[l];
    lv.n_in = n;
    lv.tiles = n <= kTopkTile ? 1 : (n + kTopkTile - 1) / kTopkTile;
    lv.n_out = (lv.tiles - 1) * k + topk_tile_emits(n, lv.tiles - 1, k);
    if (l > 0) {
      lv.in_key = p.level[l - 1].out_key;
      lv.in_row = p.level[l - 1].out_row;
    }
    if (lv.tiles == 1) break;
    lv.out_key = off;
    off += pad256((size_t)((u64)q * (u64)lv.n_out * (u64)vsize));
    lv.out_row = off;
    off += pad256((size_t)((u64)q * (u64)lv.n_out * 4));
    n = lv.n_out;
  }
  p.levels = l + 1;
  p.total_bytes = off;
  return p;
}

}  // namespace glint
