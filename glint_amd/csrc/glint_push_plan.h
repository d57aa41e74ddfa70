// glint_push_plan.h -- the route of a push, as a pure function of what the host knows when it launches.
//
// launch_push (glint_gpu.hip) fills a PushQuery from the call's flags and pointers, the shard's latched
// hint words and the environment knobs, asks push_route() which kernels the push takes, and launches
// them. Nothing here reads the device or touches a glint_shard, so the choice is tested on a CPU
// (tests/test_plan_cpu.py). Plain C++17, no HIP.
#pragma once
#include "../../include/glint_gpu.h"

#include <stddef.h>
#include <stdint.h>

namespace glint {

typedef long long i64;
typedef unsigned long long u64;
typedef unsigned int u32;

constexpr int kPPT = 8;               // record pairs per lane per wave tile (push_check / push_apply)
constexpr int kTile = 64 * kPPT * 2;  // 1024 records per wave tile
// pushes of up to this many records can take the one-launch order-preserving fold (glint_ordered.hip):
// above the reference's frame cap of 79 999 Double records per message (glint.conf:143)
constexpr i64 kOrderedMax = (i64)1 << 17;
// internal push flag (not in the ABI): the call comes from a host-pointer / wire entry point, i.e.
// from the actor's update(), and keeps the message's summation order unless GLINT_PUSH_UNORDERED
constexpr int kPushHostSequential = 1 << 16;
// records: up to this many, a (non-deterministic) push is the single scatter launch
constexpr i64 kSmallPushMax = 4096;
constexpr i64 kBinMin = (i64)1 << 20;  // records: below this the LDS-hash scatter wins

inline size_t pad256(size_t b) { return (b + 255) & ~(size_t)255; }

struct PushQuery {
  i64 n = 0;            // records
  int flags = 0;        // GLINT_PUSH_* | kPushHostSequential
  bool fp = false;      // a Float/Double shard (Int/Long sums are exact in any order)
  bool vec_ok = false;  // the caller's pointers allow 16-byte record pair loads
  bool gated = false;   // glint_*_push_dev_gated
  bool ring = false;    // a ring launch: one workgroup that signals its own completion
  i64 elems = 0;        // elements allocated in the shard
  bool binnable = false;  // push_binnable(): u32 record indices and element addresses
  u64 hint_tail = 0;    // the previous push's unordered tail, as of the shard's last sync point
  u64 hint_head = 0;    // ... and where that tail started
  u32 whole_probe = 0;  // whole-push scatters so far
  int binned_mode = -1;  // GLINT_BINNED: 0 never bin, 1 bin every large push, -1 by the last tail
  i64 bin_density = 512;  // GLINT_BIN_DENSITY: records per 4096-element slab from which the tail is binned
  bool whole_on = true;  // GLINT_BIN_WHOLE
};

enum class PushKind {
  Invalid,     // GLINT_EINVAL
  Ordered,     // the one-launch order-preserving fold
  BinnedAll,   // the binned pipeline for every record, no check (an UNORDERED push)
  WholeBin,    // the binned pipeline from record 0 in place of check + apply (`validate`: with the hook)
  ScatterAll,  // one scatter launch for every record (scatter_mode 1, or 2 for the whole-push scatter)
  DetAll,      // the stable sort and fold for every record
  Checked      // push_check, push_apply up to the break, then `tail` from the break
};
enum class PushTail { Scatter, Det, Binned };

struct PushRoute {
  PushKind kind = PushKind::Invalid;
  PushTail tail = PushTail::Scatter;  // Checked only
  bool validate = false;     // a gated push that validates its records and writes its own verdict
  bool fuse = false;         // Checked: the verdict and the head come behind the binned tail's count (BinHook)
  bool gate_kernel = false;  // Checked: push_gate_kernel reads the caller's gate word first
  int scatter_mode = 0;      // push_scatter's mode argument: 0 from the break, 1 every record, 2 whole-push
  bool probe_consumed = false;  // the caller advances the shard's whole_probe
};

inline PushRoute push_route(const PushQuery& q) {
  PushRoute r;
  const bool det = (q.flags & GLINT_PUSH_DETERMINISTIC) && q.fp;
  const bool unordered = (q.flags & GLINT_PUSH_UNORDERED) != 0;
  // Message-sized Float/Double pushes that must keep the reference's summation order -- every
  // deterministic one, and host-pointer / wire pushes unless the caller said UNORDERED -- are one
  // launch of the order-preserving fold (glint_ordered.hip). Int/Long sums are exact in any order.
  const bool seq = det || (q.fp && (q.flags & kPushHostSequential) && !unordered);
  // a gated push takes check + apply (+ its tail from the break): those kernels read the gate's
  // verdict from the LaunchCtl (the ordered fold, the unordered hint and the one-launch small push
  // have no such step)
  if (q.gated && (det || !q.vec_ok)) return r;
  // a ring launch is always the ordered fold: for Int/Long it is one more exact summation order
  if (q.ring || (seq && q.n <= kOrderedMax && q.elems < ((i64)1 << 32))) {
    r.kind = PushKind::Ordered;
    return r;
  }
  const i64 last_tail = (i64)q.hint_tail;
  const i64 slabs = (q.elems + 4095) / 4096;
  const bool binned =
      !det && q.vec_ok && q.binnable && q.binned_mode != 0 &&
      (unordered || (q.n >= kBinMin && (q.binned_mode == 1 ||
                                        (last_tail >= kBinMin && last_tail >= q.bin_density * slabs))));
  if (binned && unordered && !q.gated) {
    r.kind = PushKind::BinnedAll;
    return r;
  }
  r.validate = q.gated && (q.flags & GLINT_PUSH_VALIDATE) != 0;
  // Whole-push bin: when the last push (as of the last sync point) broke order in its first tile, the
  // binned pipeline takes this one from record 0 with no push_check (the unordered push's check found
  // only that, at one contended atomic per wave tile) and no head. Sums are the same in any order (this
  // is not a deterministic push); bin_count validates every record of a validating push, zeroes the
  // next push's LaunchCtl slot as push_check does, and notes whether two adjacent records were ever out
  // of order, so an ordered push is followed by the checked path again. GLINT_BIN_WHOLE=0: always check.
  const bool from_zero = q.hint_tail > 0 && q.hint_head == 0;
  if (binned && (!q.gated || r.validate) && from_zero && q.whole_on) {
    r.kind = PushKind::WholeBin;
    return r;
  }
  // Small pushes (an Akka message is ~1000 records, GranularBigVectorSpec.scala:21) are one launch:
  // the scatter handles every record, instead of check + apply + scatter. Launch latency is the
  // whole cost at this size, so two fewer launches is the win; results are those of the scatter
  // path (bit-exact for unique keys and for Int/Long, unordered sums otherwise).
  const bool small = !det && !q.gated && q.n <= kSmallPushMax;
  // Whole-push scatter: the sparse counterpart of the whole-push bin. When the last checked push broke
  // order in its first tile and this one stays below the binned density, the scatter takes every record
  // from 0 with no push_check / push_apply in front (they found only that). Its hint words say so (the
  // push's size, a tail from record 0) without looking, so every 8th such push is checked again (its
  // push_apply writes the measured words: an ordered push returns the shard to the checked path). The
  // probe counts every push that comes this far, whatever the knob then says.
  r.probe_consumed = !binned && !det && !q.gated && q.vec_ok && !small && from_zero;
  const bool whole_scatter = r.probe_consumed && (q.whole_probe & 7u) != 7u && q.whole_on;
  if (!q.vec_ok || small || whole_scatter) {  // unaligned caller pointers or a small push: one path for everything
    r.kind = det ? PushKind::DetAll : PushKind::ScatterAll;
    r.scatter_mode = whole_scatter ? 2 : 1;
    return r;
  }
  r.kind = PushKind::Checked;
  r.gate_kernel = q.gated && !r.validate;
  // a validating push whose tail is binned reads its keys once: push_check validates the records up to
  // the break, the tail's count pass the rest, and the verdict comes after that count (BinHook)
  r.fuse = r.validate && binned && !det;
  r.tail = det ? PushTail::Det : binned ? PushTail::Binned : PushTail::Scatter;
  return r;
}

// ---- the affine sweep's tickets (push_apply's apply_sweep, glint_gpu.hip) ----
// A dense push is swept in one launch by S blocks that take tickets from a device counter. The record
// pairs [0, n >> 1) are cut into rows of kSweepRowPairs pairs (one pair per thread of a block) and into
// super-windows of kSweepTicketRows * S rows. Ticket t is slot t % S of super-window t / S: the rows
// r * S + slot, r < kSweepTicketRows, of that super-window, so the S tickets of a super-window read it
// exactly as a grid-stride loop of S blocks would. A ticket whose first row starts at or past the last
// pair does not exist; a row may reach past the last pair and is cut there by the caller. Usable from
// host and device code (tests/c/sweep_probe.cpp checks the cover on a CPU).
#if defined(__HIPCC__)
#define GLINT_HD __host__ __device__
#else
#define GLINT_HD
#endif
constexpr int kSweepRowPairs = 256;    // pairs per row: the block size of push_apply (kTPB)
constexpr int kSweepTicketRows = 16;   // rows per ticket
constexpr i64 kSweepTicketRecords = 2ll * kSweepTicketRows * kSweepRowPairs;  // 8192 records per full ticket

struct SweepTicket {
  i64 first;   // the first unit of row 0
  i64 stride;  // units from one row's start to the next row's
};

// The arithmetic in units (record pairs for the sweep, wave tiles for the tile path below): rows of
// `row` units, `rows` rows per ticket, S blocks.
GLINT_HD inline u64 ticket_count(i64 units, i64 row, int rows, u32 S) {
  const i64 sw = row * rows * (i64)S;                   // units per super-window
  const i64 rem_rows = (units % sw + row - 1) / row;    // rows of the last, partial one
  return (u64)(units / sw) * S + (u64)(rem_rows < (i64)S ? rem_rows : (i64)S);
}
GLINT_HD inline SweepTicket ticket_at(u64 t, i64 row, int rows, u32 S) {
  SweepTicket k;
  k.stride = (i64)S * row;
  k.first = (i64)(t / S) * rows * k.stride + (i64)(t % S) * row;
  return k;
}

// tickets of a push of n records swept by S blocks (S >= 1), and ticket t's rows of record pairs
GLINT_HD inline u64 sweep_ticket_count(i64 n, u32 S) { return ticket_count(n >> 1, kSweepRowPairs, kSweepTicketRows, S); }
GLINT_HD inline SweepTicket sweep_ticket(u64 t, u32 S) { return ticket_at(t, kSweepRowPairs, kSweepTicketRows, S); }

// The tile path of push_apply (a push that is not one affine run) takes tickets the same way: a row is
// the kTileRowTiles wave tiles of a block's waves, a ticket kTileTicketRows rows of a super-window of
// G blocks' rows, so a super-window is read as the static wave stride reads it.
constexpr int kTileRowTiles = 4;     // waves per block of push_apply (kTPB / 64)
constexpr int kTileTicketRows = 8;   // rows per ticket
GLINT_HD inline u64 tile_ticket_count(i64 tiles, u32 G) { return ticket_count(tiles, kTileRowTiles, kTileTicketRows, G); }
GLINT_HD inline SweepTicket tile_ticket(u64 t, u32 G) { return ticket_at(t, kTileRowTiles, kTileTicketRows, G); }

// ---- the binned front end's history (a member of glint_shard; bin_front_next in glint_bin_plan.h) ----
// Front ends: 0 plain, 1 plain + hot-element split, 2 chunk dedup (+ hot split). What the last dedup
// push measured decides: chunk_ratio = records it kept of the cold records that entered its hash table
// (1.0 = dedup merged nothing), hot_frac = share of the tail taken by the hot elements. A dedup push
// re-measures every 16 pushes. The measurements reach the host only at sync points (latch_hints), so a
// device-resident caller that never calls glint_shard_sync keeps the no-history default: the plain
// front end (ratio 1.0: dedup merged nothing), with a dedup probe every 16 pushes.
struct BinFrontState {
  double chunk_ratio = 1.0;
  double hot_frac = 0.0;
  u32 pushes = 0;
  int last_front = 0;  // the front end of the last binned push
  u32 hot_age = 0;     // binned pushes since the wide hot table was last sampled (0: never)
};

}  // namespace glint
