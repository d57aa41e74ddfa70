// glint_bin_plan.h -- what a binned push (glint_bin.hip push_binned) settles on the host before it
// launches: which front end takes the push, and the sizes, counts and scratch layout of the pipeline.
// Plain C++17, no HIP, tested on a CPU (tests/test_plan_cpu.py). Among the product's sources
// glint_bin.hip alone includes it, so a variant of that one file built with -D knobs stays consistent
// (tools/variant.py).
#pragma once
#include "glint_push_plan.h"

#include <algorithm>

namespace glint {

// ---- build-time knobs and the constants the sizes depend on ---------------------------------------
#ifndef GLINT_SLAB_BITS
#define GLINT_SLAB_BITS 12
#endif
constexpr int kSlabBits = GLINT_SLAB_BITS;  // (a build-time experiment knob; 12 = 32 KiB of Double per slab)
constexpr int kSlab = 1 << kSlabBits;
constexpr int kMaxDigit = 1024;        // coarse buckets and fine slabs per bucket, at most
#ifndef GLINT_PART_TPB
#define GLINT_PART_TPB 1024
#endif
constexpr int kATPB = GLINT_PART_TPB;  // partition workgroup size (a knob in name: >= kMaxDigit, see part_emit)
#ifndef GLINT_PART_PER
#define GLINT_PART_PER 4
#endif
constexpr int kAPer = GLINT_PART_PER;  // records per thread per chunk (build-time knob)
#ifndef GLINT_PART_PER_PLAIN
#define GLINT_PART_PER_PLAIN 8
#endif
// The plain front end of a large push takes chunks of 8 records per thread (no hot or dedup table
// beside its staging in LDS): runs of 64 records per bucket and half the barriers per record. Same box,
// two rounds (profiles/r06/ab_part_per_plain.txt): cfg4b 2.20 -> 2.16 ms; cfg5 (a small push) 0.311 ->
// 0.314, so a small push keeps 4
constexpr int kAPerPlain = GLINT_PART_PER_PLAIN;
// partition workgroups per CU: LDS-bound (the dedup table; the plain front end's staging)
constexpr int kPartWgPerCuDedup = kATPB == 1024 ? 1 : 2;
#ifndef GLINT_PART_WPC
#define GLINT_PART_WPC (kATPB == 1024 ? 1 : 2)
#endif
constexpr int kPartWgPerCuPlain = GLINT_PART_WPC;  // what fits (VGPRs): a second round of
                                                           // workgroups measured 3-9 % slower
#ifndef GLINT_FSORT_TPB
#define GLINT_FSORT_TPB 1024
#endif
// Records per thread of a fine item: 12 for every push, the values held in registers from their load to
// their staging round (two rounds of 8192 through the 64 KiB stage), at two workgroups per CU (64
// VGPRs). Same boxes (profiles/r06/ab_chunk_local.txt): 16 per thread with the values loaded again in
// each staging round measured cfg4b 2.10 against 1.89 ms, cfg3 1.06 against 0.99; 8 per thread 1.92 /
// 0.99 / cfg5 0.339 against 0.328. (Before the chunk-local partition, with contiguous items, 16 late
// had been the best: ab_fsort_per16.txt.) Build-time knobs GLINT_FSORT_PER_SMALL / _LARGE (small: the
// pushes with the plan fused in, see push_binned).
#ifndef GLINT_FSORT_PER_SMALL
#define GLINT_FSORT_PER_SMALL 12
#endif
#ifndef GLINT_FSORT_PER_LARGE
#define GLINT_FSORT_PER_LARGE 12
#endif
constexpr int kSTPB = GLINT_FSORT_TPB;
constexpr int kSPerSmall = GLINT_FSORT_PER_SMALL, kSPerLarge = GLINT_FSORT_PER_LARGE;
constexpr int kRunMax = 128;     // runs per apply unit at most
#ifndef GLINT_UNIT_CAP
#define GLINT_UNIT_CAP 4096
#endif
constexpr u32 kUnitCap = GLINT_UNIT_CAP;  // records per apply unit at most
static_assert(kUnitCap <= 65535, "a unit's record prefix is staged as u16");
constexpr int kHotSlots = 2048;   // direct-mapped hot table (per dedup workgroup: tags + sums in LDS)
constexpr int kWideSlots = 8192;  // the plain + hot front end's hot table (see bin_hot_select)

struct BinGeom {
  u32 fb;     // fine digit bits
  u32 nb;     // coarse buckets (power of two)
  u32 nf;     // fine slabs per bucket (power of two)
  u32 nslab;  // nb * nf
};

// 128 coarse buckets (few enough that a partition chunk's records form runs per bucket, and a fine
// item's runs per slab stay as long: 32 records each way for uniform keys into 2^28), more only when
// the fine digit would exceed 10 bits (slabs < 2^20 for u32 addresses). Same box, two runs each
// (profiles/r03/bench_binned_cb.txt): 2^7 against 2^8 buckets cfg5 0.418 -> 0.398 ms, cfg3 1.648 ->
// 1.636 ms, cfg4b exchange 3.005 -> 3.005 ms; 2^6 slower on all
#ifndef GLINT_BIN_CB
#define GLINT_BIN_CB 7  // (build-time knob: coarse digit bits at least)
#endif
constexpr u32 kCoarseBitsMin = GLINT_BIN_CB;
inline BinGeom bin_geometry(i64 elems, u32 cbmin) {
  const i64 slabs = (elems + kSlab - 1) / kSlab;
  u32 sb = 0;
  while (((i64)1 << sb) < slabs) ++sb;
  const u32 cb = std::min<u32>(sb, std::max<u32>(cbmin, sb > 10u ? sb - 10u : 0u));
  BinGeom g;
  g.fb = sb - cb;
  g.nb = 1u << cb;
  g.nf = 1u << g.fb;
  g.nslab = g.nb * g.nf;
  return g;
}

// ---- front end -------------------------------------------------------------------------------------
// The wide hot table (front 1) is sampled every kHotEvery-th push and kept in between: a push's hot
// set only decides how much work leaves the partition path (any set gives the same sums), and a
// Zipf-like stream keeps its hot elements from push to push. A shard coming from another front end
// samples at once. (tests/test_gpu_parity.py::test_binned_stream_of_batches pushes a stream of
// different batches through the kept table.)
constexpr u32 kHotEvery = 8;

struct BinFront {
  int front;         // 0 plain, 1 plain + hot split, 2 chunk dedup + hot split
  bool hot_refresh;  // front 1: sample the wide hot table again (true for the other front ends)
};

// Front end of the next binned push, from what the last dedup push measured (the device reports m, the
// tail size and the cold records of each push through host-mapped words, taken at the shard's last
// sync point, so the choice does not depend on timing; hint_bin = m << 32 | tail, written by front end
// hint_bin_front): chunk dedup when it kept < 80 % of the cold records it saw; otherwise the plain
// front end, with the hot-element split when the hot elements took >= 25 % of the tail (cfg3 ~65 %;
// cfg5's ~10 % does not pay for the sampling launch and the per-record check). A dedup push
// re-measures every 16 pushes (and the first one). forced >= 0 (GLINT_BIN_FRONT) is taken as it is;
// the history advances all the same.
inline BinFront bin_front_next(BinFrontState& f, u64 hint_bin, u64 hint_bin_cold, int hint_bin_front, int forced) {
  const u32 m = (u32)(hint_bin >> 32), tail = (u32)hint_bin;
  const u32 cold = (u32)hint_bin_cold;
  if (tail > 0 && hint_bin_front == 2) {
    f.chunk_ratio = cold ? (double)m / (double)cold : 1.0;
    f.hot_frac = 1.0 - (double)cold / (double)tail;
  }
  const bool probe = (f.pushes++ & 15) == 0;
  const int chosen = probe || f.chunk_ratio < 0.8 ? 2 : (f.hot_frac >= 0.25 ? 1 : 0);
  BinFront r{forced >= 0 ? forced : chosen, true};
  if (r.front == 1) {
    r.hot_refresh = f.last_front != 1 || f.hot_age == 0 || f.hot_age >= kHotEvery;
    f.hot_age = r.hot_refresh ? 1u : f.hot_age + 1u;
  }
  f.last_front = r.front;
  return r;
}

// ---- sizes and scratch layout ------------------------------------------------------------------------
// The chunk table (a spare row past the last chunk), the buckets' chunk prefixes P and places Q, Bb,
// Ib, the fine items and their first chunks, off2, the apply units and their runs, the dedup front
// end's hot tags, the hot split's per-workgroup sums (front 1 only) and the record buffers (coarse:
// u32 address + A value; fine: u16 slab offset + A value), each at a multiple of 256 bytes of the
// shard's binned scratch, in this order. (The [BinCtl | T] headers and the hot front end's tables live
// in buffers of their own.)
struct BinLayout {
  BinGeom g;
  bool small_push;  // at most ~4 fine items per CU (cfg5): the buckets are planned inside bin_fsort
  int per;          // records per thread of a partition chunk
  u32 kchunk;       // records per partition chunk
  i64 nchunks_max;
  int wpc;          // partition workgroups per CU
  u32 G;            // partition workgroups
  u32 item;         // records per fine item
  i64 max_fitems, max_units;
  u32 nstride, ctstride;  // chunks per row of P / Q, and of the chunk table (a spare column past the last)
  size_t ct, P, Q, Bb, Ib, fitems, cwin, off2, units, runs, hot_tags, wpart, addr_a, val_a, val_b, e_b;  // byte offsets
  size_t need;      // bytes in all
};

// acc_bytes: sizeof of the LDS accumulator type of the shard's values; hot_occ: resident workgroups per
// CU of the hot-split partition kernel (its LDS table allows fewer than the plain one's)
inline BinLayout bin_layout(i64 elems, i64 n, int cus, int front, size_t acc_bytes, int hot_occ) {
  BinLayout L;
  L.small_push = (i64)bin_geometry(elems, kCoarseBitsMin).nb + n / ((i64)kSTPB * kSPerSmall) + 1 <= (i64)4 * cus;
  // records per thread of a partition chunk: 8 for a large push's plain front end, 4 otherwise (the hot
  // and dedup tables share the LDS; a small push wants more chunks)
  L.per = front == 0 && !L.small_push ? kAPerPlain : kAPer;
  // Coarse buckets: 128 for chunks of 8 records per thread, 64 for chunks of 4 -- runs of ~64 records
  // per bucket and chunk either way, which the fine sort gathers. Same box, 2 rounds
  // (profiles/r06/ab_chunk_local.txt): 64 buckets for every push took cfg5 0.316 -> 0.303 ms and cfg3
  // 0.965 -> 0.956, but cfg4b (8-record chunks) 1.85 -> 1.93.
  L.g = bin_geometry(elems, L.per == kAPerPlain ? kCoarseBitsMin : kCoarseBitsMin - 1u);
  const BinGeom& g = L.g;
  L.kchunk = (u32)kATPB * (u32)L.per;
  L.nchunks_max = (n + L.kchunk - 1) / L.kchunk;
  // partition workgroups per CU: what fits at once
  L.wpc = front == 2 ? kPartWgPerCuDedup : front == 1 ? std::min(kPartWgPerCuPlain, hot_occ) : kPartWgPerCuPlain;
  L.G = (u32)std::max<i64>(1, std::min<i64>(L.nchunks_max, (i64)cus * L.wpc));
  L.item = (u32)kSTPB * (u32)(L.small_push ? kSPerSmall : kSPerLarge);
  L.max_fitems = (i64)g.nb + n / L.item + 1;
  // apply units: a slab's units close at kUnitCap records or kRunMax runs, so at most
  // floor(H / cap) + floor(runs / kRunMax) + 1 per non-empty slab
  L.max_units = (i64)g.nslab + n / kUnitCap + std::min<i64>(n, L.max_fitems * g.nf) / kRunMax + 1;
  L.nstride = (u32)L.nchunks_max;
  L.ctstride = L.nstride + 1;
  size_t cur = 0;
  const auto take = [&cur](size_t bytes) {
    const size_t at = cur;
    cur += pad256(bytes);
    return at;
  };
  L.ct = take((size_t)L.ctstride * g.nb * 4);
  L.P = take((size_t)g.nb * (L.nstride + 1) * 4);
  L.Q = take((size_t)g.nb * L.nstride * 4);
  L.Bb = take((size_t)g.nb * 4);
  L.Ib = take((size_t)g.nb * 4);
  L.fitems = take((size_t)L.max_fitems * 8);
  L.cwin = take((size_t)L.max_fitems * 8);
  L.off2 = take((size_t)L.max_fitems * (g.nf + 1) * 4);
  L.units = take((size_t)L.max_units * 16);
  L.runs = take((size_t)L.max_units * kRunMax * 8);
  L.hot_tags = take((size_t)kHotSlots * 4);
  L.wpart = take(front == 1 ? (size_t)L.G * kWideSlots * acc_bytes : 0);
  L.addr_a = take((size_t)n * 4);
  L.val_a = take((size_t)n * acc_bytes);
  L.val_b = take((size_t)n * acc_bytes);
  L.e_b = take((size_t)n * 2);
  L.need = cur;
  return L;
}

}  // namespace glint
