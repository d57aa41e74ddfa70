// topk_probe.cpp -- the top-k pull's level plan (glint_topk_plan.h topk_plan) behind a C interface, for
// tests/test_topk_cpu.py (ctypes). No GPU, no HIP.
#include "../../glint_amd/csrc/glint_topk_plan.h"

using namespace glint;

extern "C" {

// out: the tile, the largest k, the largest q, the most levels
void topk_constants(int64_t* out) {
  out[0] = kTopkTile;
  out[1] = GLINT_TOPK_MAX_K;
  out[2] = GLINT_TOPK_MAX_QUERIES;
  out[3] = kTopkMaxLevels;
}

// The plan of (size, q, k, vsize): returns its level count (0: refused); head = {scores_bytes,
// total_bytes}; levels = 7 words per level: n_in, tiles, n_out, in_key, in_row, out_key, out_row.
int topk_plan_of(int64_t size, int64_t q, int64_t k, int64_t vsize, uint64_t* head, int64_t* levels) {
  const TopkPlan p = topk_plan(size, q, k, vsize);
  head[0] = p.scores_bytes;
  head[1] = p.total_bytes;
  for (int l = 0; l < p.levels; ++l) {
    const TopkLevel& lv = p.level[l];
    int64_t* o = levels + 7 * l;
    o[0] = lv.n_in;
    o[1] = lv.tiles;
    o[2] = lv.n_out;
    o[3] = (int64_t)lv.in_key;
    o[4] = (int64_t)lv.in_row;
    o[5] = (int64_t)lv.out_key;
    o[6] = (int64_t)lv.out_row;
  }
  return p.levels;
}

// what tile t of a level over n candidates takes and emits (out: count, emitted)
void topk_tile_of(int64_t n, int64_t t, int64_t k, int64_t* out) {
  out[0] = topk_tile_count(n, t);
  out[1] = topk_tile_emits(n, t, k);
}

}  // extern "C"
