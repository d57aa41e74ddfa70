// sweep_probe.cpp -- the affine sweep's ticket arithmetic (glint_push_plan.h sweep_ticket_count,
// sweep_ticket) behind a C interface, for tests/test_sweep_tickets_cpu.py (ctypes). No GPU, no HIP.
#include "../../glint_amd/csrc/glint_push_plan.h"

#include <vector>

using namespace glint;

extern "C" {

// out: records per full ticket, rows per ticket, pairs per row
void sweep_constants(int64_t* out) {
  out[0] = kSweepTicketRecords;
  out[1] = kSweepTicketRows;
  out[2] = kSweepRowPairs;
}

uint64_t sweep_count(int64_t n, uint32_t S) { return sweep_ticket_count(n, S); }

// out: first pair of row 0, pairs between row starts
void sweep_ticket_at(uint64_t t, uint32_t S, int64_t* out) {
  const SweepTicket k = sweep_ticket(t, S);
  out[0] = k.first;
  out[1] = k.stride;
}

// Walks every ticket [0, count) of a push of n records as apply_sweep does (rows of kSweepRowPairs pairs,
// cut at the last pair) and counts the visits of every pair. Returns 0 when each pair of [0, n >> 1) is
// visited exactly once and nothing else is; 1 a pair outside the range; 2 a pair visited twice; 3 a pair
// never visited; 4 a ticket with no pair in range (it should not have been counted).
int sweep_cover(int64_t n, uint32_t S) {
  const i64 npairs = n >> 1;
  std::vector<unsigned char> seen((size_t)npairs, 0);
  const u64 count = sweep_ticket_count(n, S);
  for (u64 t = 0; t < count; ++t) {
    const SweepTicket k = sweep_ticket(t, S);
    if (k.first < 0 || k.first >= npairs) return k.first < 0 ? 1 : 4;
    for (int r = 0; r < kSweepTicketRows; ++r) {
      for (int tid = 0; tid < kSweepRowPairs; ++tid) {
        const i64 p = k.first + (i64)r * k.stride + tid;
        if (p >= npairs) continue;  // the kernel's cut
        if (p < 0) return 1;
        if (seen[(size_t)p]++) return 2;
      }
    }
  }
  for (i64 p = 0; p < npairs; ++p)
    if (!seen[(size_t)p]) return 3;
  return 0;
}

// The tile path's tickets (tile_ticket_count, tile_ticket), walked as push_apply_kernel does: wave w of
// the block takes tile first + r * stride + w of row r, cut at `tiles`. Same return codes, per tile.
uint64_t tile_count(int64_t tiles, uint32_t G) { return tile_ticket_count(tiles, G); }

int tile_cover(int64_t tiles, uint32_t G) {
  std::vector<unsigned char> seen((size_t)tiles, 0);
  const u64 count = tile_ticket_count(tiles, G);
  for (u64 t = 0; t < count; ++t) {
    const SweepTicket k = tile_ticket(t, G);
    if (k.first < 0 || k.first >= tiles) return k.first < 0 ? 1 : 4;
    for (int r = 0; r < kTileTicketRows; ++r) {
      for (int w = 0; w < kTileRowTiles; ++w) {
        const i64 p = k.first + (i64)r * k.stride + w;
        if (p >= tiles) continue;
        if (p < 0) return 1;
        if (seen[(size_t)p]++) return 2;
      }
    }
  }
  for (i64 p = 0; p < tiles; ++p)
    if (!seen[(size_t)p]) return 3;
  return 0;
}

}  // extern "C"
