// glint_keymap.hip -- the device key map (glint_keymap_*, DESIGN.md "Key map"): an insert-only open-addressing
// table on one device that turns 64-bit feature ids into table rows, the rows handed out in call order and
// never in race order. glint_keymap_plan.h holds the slot marks, the hash and the scratch layout.
//   lookup   one launch, one key per thread, one 16-byte load per probe.
//   insert   claim  -- a record probes as a lookup does; a committed hit is final and costs no atomic; at an
//                      empty slot it claims the key by a 64-bit compare-and-swap, and every record of a key
//                      that is new in this call leaves the minimum of its index in the slot's val;
//            rank   -- record i is a first occurrence iff its slot's val names i; an exclusive scan of those
//                      flags, tile by tile and level by level, whose top workgroup also decides the call:
//                      commit and advance `size`, or roll back and record why;
//            commit -- a record of a new key answers first_row + size + rank[first occurrence], the first
//                      occurrence also stores that row and the reverse entry; on a roll-back the first
//                      occurrences empty their slots again and only keys present before answer a row.
//   keysOf   a bounds-checked gather from the reverse array.
// No thread waits for another thread's progress, no answer depends on which thread came first, and kernel
// boundaries are the only ordering between the steps. No inline assembly, no LDS beyond the scan's wave sums.
#include "glint_device.h"
#include "glint_host.h"
#include "glint_keymap_plan.h"

#include <new>

namespace glint {

constexpr int kKeymapItems = kKeymapScanTile / kTPB;
static_assert(kKeymapItems * kTPB == kKeymapScanTile, "a scan tile is a whole number of records per thread");

// a record's claim word: its slot (below 2^30), or
constexpr u32 kClaimCommitted = 0x80000000u;  // | slot: the key was in the map before the call
constexpr u32 kClaimNone = 0x40000000u;       // no slot: the reserved key, or a probe that found no empty slot

struct alignas(16) KeymapSlot {
  i64 key;
  u64 val;
};
typedef __attribute__((ext_vector_type(2))) unsigned long long KeymapPair;

__device__ __forceinline__ KeymapSlot keymap_load(const KeymapSlot* p) {
  const KeymapPair v = *reinterpret_cast<const KeymapPair*>(p);
  return KeymapSlot{(i64)v.x, v.y};
}
__device__ __forceinline__ void keymap_store_empty(KeymapSlot* p) {
  *reinterpret_cast<KeymapPair*>(p) = KeymapPair{(u64)kKeymapEmptyKey, kKeymapEmptyVal};
}

// the map's control words, in device memory
enum {
  kCtlSize = 0,  // keys in the map
  kCtlBad,       // the running insert: the lowest index of the reserved key (~0: none)
  kCtlWrap,      // the running insert: a probe went round the table
  kCtlBase,      // the running insert: `size` before it (what its commit numbers from)
  kCtlFail,      // the running insert: rolled back
  kCtlLatBad,    // device-form calls since the last glint_keymap_sync: the lowest refused index (~0: none)
  kCtlLatFree,   // ... and the least free row count of an insert that overflowed (~0: none)
  kCtlHostBad,   // the same pair for the running host-form call, which reads and clears it itself
  kCtlHostFree,
  kCtlWords
};
constexpr u64 kCtlNone = ~(u64)0;

__global__ __launch_bounds__(kTPB) void keymap_fill_kernel(KeymapSlot* slots, u32 nslots, u64* ctl) {
  const u32 t = blockIdx.x * kTPB + threadIdx.x;
  for (u32 i = t; i < nslots; i += gridDim.x * kTPB) keymap_store_empty(slots + i);
  if (t < kCtlWords) ctl[t] = (t == kCtlBad || t >= kCtlLatBad) ? kCtlNone : 0;
}

__global__ void keymap_clear_kernel(u64* pair) {
  if (threadIdx.x < 2) pair[threadIdx.x] = kCtlNone;
}

// ---- lookup ----------------------------------------------------------------------------------------------
// One key per thread: the chain is a run of dependent 16-byte loads, and more resident waves hide its latency
// better than several chains per lane did (measured: DESIGN.md "Key map").
__global__ __launch_bounds__(kTPB) void keymap_lookup_kernel(const KeymapSlot* __restrict__ slots, u32 mask,
                                                             const i64* __restrict__ keys, u32 n, i64 missing,
                                                             i64* __restrict__ out, u64* bad) {
  const u32 i = blockIdx.x * kTPB + threadIdx.x;
  if (i >= n) return;
  const i64 k = keys[i];
  i64 ans = missing;
  if (k == kKeymapEmptyKey) {
    atomicMin(bad, (u64)i);
  } else {
    u32 pos = (u32)keymap_hash(k) & mask;
    for (u32 step = 0; step <= mask; ++step, pos = (pos + 1) & mask) {
      const KeymapSlot s = keymap_load(slots + pos);
      if (s.key == k) {
        if (s.val < kKeymapTentative) ans = (i64)s.val;
        break;
      }
      if (s.key == kKeymapEmptyKey) break;
    }
  }
  out[i] = ans;
}

// ---- insert: claim ---------------------------------------------------------------------------------------
// A slot's key changes once, from empty to its key, and within one insert its val only falls (empty ->
// tentative -> a lower tentative), so a load that sees an older state of a slot only sends the record to an
// atomic that tells it the truth; rows are stored by the commit kernel alone.
__global__ __launch_bounds__(kTPB) void keymap_claim_kernel(KeymapSlot* slots, u32 mask, const i64* __restrict__ keys,
                                                            u32 n, u32* __restrict__ claim, u64* ctl) {
  const u32 i = blockIdx.x * kTPB + threadIdx.x;
  if (i >= n) return;
  const i64 k = keys[i];
  if (k == kKeymapEmptyKey) {
    atomicMin(&ctl[kCtlBad], (u64)i);
    claim[i] = kClaimNone;
    return;
  }
  u32 pos = (u32)keymap_hash(k) & mask;
  for (u32 step = 0; step <= mask; ++step, pos = (pos + 1) & mask) {
    KeymapSlot s = keymap_load(slots + pos);
    if (s.key == kKeymapEmptyKey) {
      const u64 old = atomicCAS(reinterpret_cast<u64*>(&slots[pos].key), (u64)kKeymapEmptyKey, (u64)k);
      s.key = old == (u64)kKeymapEmptyKey ? k : (i64)old;
      s.val = kKeymapEmptyVal;  // claimed in this call, by this record or another: not committed
    }
    if (s.key != k) continue;
    if (s.val < kKeymapTentative) {
      claim[i] = pos | kClaimCommitted;
      return;
    }
    atomicMin(&slots[pos].val, kKeymapTentative + i);
    claim[i] = pos;
    return;
  }
  ctl[kCtlWrap] = 1;  // every slot holds another key: the call overflows
  claim[i] = kClaimNone;
}

// ---- insert: rank ----------------------------------------------------------------------------------------
// What a scan level adds up: at the records, whether record i is the first occurrence of a new key; above
// them, the tile sums of the level below.
struct KeymapFirst {
  const KeymapSlot* slots;
  const u32* claim;
  __device__ __forceinline__ u32 at(u32 i) const {
    const u32 c = claim[i];
    if (c & (kClaimCommitted | kClaimNone)) return 0;
    return slots[c].val == kKeymapTentative + i ? 1u : 0u;
  }
};
struct KeymapSums {
  const u32* x;
  __device__ __forceinline__ u32 at(u32 i) const { return x[i]; }
};

// what the top workgroup of the scan needs to decide the call
struct KeymapDecide {
  u64* ctl;
  i64 capacity;
  int verdict;  // kCtlLatBad or kCtlHostBad: the pair a refusal is recorded in
};

template <typename Src>
__global__ __launch_bounds__(kTPB) void keymap_totals_kernel(Src src, u32 m, u32* __restrict__ tot) {
  __shared__ u32 lds[kTPB / 64];
  const u32 at = blockIdx.x * (u32)kKeymapScanTile + threadIdx.x * (u32)kKeymapItems;
  u32 v = 0;
#pragma unroll
  for (int k = 0; k < kKeymapItems; ++k)
    if (at + k < m) v += src.at(at + k);
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    u32 t = 0;
#pragma unroll
    for (int w = 0; w < kTPB / 64; ++w) t += lds[w];
    tot[blockIdx.x] = t;
  }
}

// out[i] = base[tile] + src[tile start] + ... + src[i - 1]; out may be the array src reads (a thread reads its
// own entries before it writes them). TOP: the single tile at the top of the scan (base == nullptr), whose
// total is the call's count of distinct new keys: thread 0 decides the call with it.
template <typename Src, bool TOP>
__global__ __launch_bounds__(kTPB) void keymap_scan_kernel(Src src, u32* out, u32 m, const u32* base, KeymapDecide d) {
  __shared__ u32 lds[kTPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const u32 at = blockIdx.x * (u32)kKeymapScanTile + threadIdx.x * (u32)kKeymapItems;
  u32 v[kKeymapItems];
  u32 mine = 0;
#pragma unroll
  for (int k = 0; k < kKeymapItems; ++k) {
    v[k] = at + k < m ? src.at(at + k) : 0;
    mine += v[k];
  }
  u32 inc = mine;  // inclusive prefix over the wave's lanes
#pragma unroll
  for (int s = 1; s < 64; s <<= 1) {
    const u32 o = __shfl_up(inc, s, 64);
    if (lane >= s) inc += o;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  u32 run = TOP ? 0 : base[blockIdx.x];
  for (int w = 0; w < wave; ++w) run += lds[w];
  run += inc - mine;
#pragma unroll
  for (int k = 0; k < kKeymapItems; ++k) {
    if (at + k < m) out[at + k] = run;
    run += v[k];
  }
  if (TOP && threadIdx.x == 0) {
    u64 total = 0;
#pragma unroll
    for (int w = 0; w < kTPB / 64; ++w) total += lds[w];
    u64* ctl = d.ctl;
    const u64 size = ctl[kCtlSize], bad = ctl[kCtlBad];
    const bool fail = bad != kCtlNone || ctl[kCtlWrap] != 0 || size + total > (u64)d.capacity;
    ctl[kCtlBase] = size;
    ctl[kCtlFail] = fail ? 1 : 0;
    if (!fail) ctl[kCtlSize] = size + total;
    else if (bad != kCtlNone) atomicMin(&ctl[d.verdict], bad);
    else atomicMin(&ctl[d.verdict + 1], (u64)d.capacity - size);
    ctl[kCtlBad] = kCtlNone;  // for the next insert
    ctl[kCtlWrap] = 0;
  }
}

// ---- insert: commit --------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTPB) void keymap_commit_kernel(KeymapSlot* slots, const i64* keys, u32 n,
                                                             const u32* __restrict__ claim,
                                                             const u32* __restrict__ rank, const u64* __restrict__ ctl,
                                                             i64 first_row, i64 capacity, i64* __restrict__ rev,
                                                             i64* out) {
  const u32 i = blockIdx.x * kTPB + threadIdx.x;
  if (i >= n) return;
  const u32 c = claim[i];
  const i64 k = keys[i];  // (read before out[i] is written: out may be keys)
  i64 ans = -1;
  if (c & kClaimNone) {
  } else if (c & kClaimCommitted) {
    ans = (i64)slots[c & ~kClaimCommitted].val;
  } else {
    u64* val = &slots[c].val;
    // the first occurrence may be storing the row right now: a reader sees the tentative value or the row,
    // and both name the same row
    const u64 v = __hip_atomic_load(val, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if (ctl[kCtlFail]) {
      if (v == kKeymapTentative + i) keymap_store_empty(slots + c);  // the slot was empty before the call
    } else if (v < kKeymapTentative) {
      ans = (i64)v;
    } else {
      const u64 i0 = v - kKeymapTentative;
      if (i0 < n) {
        const u64 r = ctl[kCtlBase] + rank[i0];
        ans = first_row + (i64)r;
        if (i0 == i && r < (u64)capacity) {
          __hip_atomic_store(val, (u64)ans, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
          rev[r] = k;
        }
      }
    }
  }
  out[i] = ans;
}

// ---- keysOf ----------------------------------------------------------------------------------------------
__global__ __launch_bounds__(kTPB) void keymap_keys_of_kernel(const i64* __restrict__ rev, const u64* __restrict__ ctl,
                                                              i64 first_row, const i64* __restrict__ rows, u32 n,
                                                              i64* __restrict__ out, u64* bad) {
  const u32 i = blockIdx.x * kTPB + threadIdx.x;
  if (i >= n) return;
  // (in unsigned arithmetic: a row far below first_row must not overflow the difference)
  const u64 off = (u64)rows[i] - (u64)first_row;
  if (off < ctl[kCtlSize]) {
    out[i] = rev[off];
  } else {
    out[i] = kKeymapEmptyKey;
    atomicMin(bad, (u64)i);
  }
}

}  // namespace glint

struct glint_keymap {
  int device = 0;
  i64 capacity = 0, first_row = 0, slots = 0;
  KeymapSlot* d_slots = nullptr;
  i64* d_rev = nullptr;  // rev[r] = the key of row first_row + r
  u64* d_ctl = nullptr;
  u64* h_ctl = nullptr;  // pinned: the control words as of the last sync or host-form call
  // an insert's scratch (glint_keymap_plan.h), grow-only
  void* d_scratch = nullptr;
  size_t scratch_bytes = 0;
  // host-form calls: a private stream and grow-only staging, ordered after the last device-form call
  hipStream_t stream = nullptr;
  void* d_io = nullptr;
  size_t io_bytes = 0;
  hipStream_t last_dev_stream = nullptr;
  bool dev_dirty = false;
  hipEvent_t order_ev = nullptr;
  std::mutex mu;  // the host side of every call (the launches, not the kernels)
};

namespace {

void keymap_free(glint_keymap* km) {
  if (km->d_slots) (void)hipFree(km->d_slots);
  if (km->d_rev) (void)hipFree(km->d_rev);
  if (km->d_ctl) (void)hipFree(km->d_ctl);
  if (km->h_ctl) (void)hipHostFree(km->h_ctl);
  if (km->d_scratch) (void)hipFree(km->d_scratch);
  if (km->d_io) (void)hipFree(km->d_io);
  if (km->stream) (void)hipStreamDestroy(km->stream);
  if (km->order_ev) (void)hipEventDestroy(km->order_ev);
  (void)hipGetLastError();
  delete km;
}

inline int keymap_call_args(const glint_keymap* km, int64_t n, const void* in, const void* out) {
  if (!km || n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && (!in || !out))) return GLINT_EINVAL;
  return GLINT_OK;
}

inline unsigned keymap_grid(i64 n, i64 per_block) { return (unsigned)((n + per_block - 1) / per_block); }

// the exclusive scan of src[0 .. m) into out on st; sums holds the tile sums of this level and of the levels
// above; the single tile at the top decides the call
template <typename Src>
int keymap_scan(Src src, u32* out, i64 m, u32* sums, const KeymapDecide& d, hipStream_t st) {
  const i64 tiles = (m + kKeymapScanTile - 1) / kKeymapScanTile;
  if (tiles <= 1) {
    hipLaunchKernelGGL((keymap_scan_kernel<Src, true>), dim3(1), dim3(kTPB), 0, st, src, out, (u32)m,
                       (const u32*)nullptr, d);
    HIPCHK(hipGetLastError());
    return GLINT_OK;
  }
  hipLaunchKernelGGL((keymap_totals_kernel<Src>), dim3((unsigned)tiles), dim3(kTPB), 0, st, src, (u32)m, sums);
  HIPCHK(hipGetLastError());
  if (int rc = keymap_scan(KeymapSums{sums}, sums, tiles, sums + tiles, d, st)) return rc;
  hipLaunchKernelGGL((keymap_scan_kernel<Src, false>), dim3((unsigned)tiles), dim3(kTPB), 0, st, src, out, (u32)m,
                     (const u32*)sums, d);
  HIPCHK(hipGetLastError());
  return GLINT_OK;
}

// the three steps of an insert of n >= 1 device keys on st; a refusal goes to the control pair `verdict`
int keymap_insert_launch(glint_keymap* km, const i64* keys, i64 n, i64* out, int verdict, hipStream_t st) {
  // (a call longer than any before it grows the scratch: the free waits for the device, once per high-water mark)
  if (int rc = grow(&km->d_scratch, &km->scratch_bytes, keymap_scratch_words(n) * sizeof(u32))) return rc;
  u32* claim = (u32*)km->d_scratch;
  u32* rank = claim + n;
  u32* sums = rank + n;
  const u32 mask = (u32)(km->slots - 1);
  const unsigned grid = keymap_grid(n, kTPB);
  hipLaunchKernelGGL(keymap_claim_kernel, dim3(grid), dim3(kTPB), 0, st, km->d_slots, mask, keys, (u32)n, claim,
                     km->d_ctl);
  HIPCHK(hipGetLastError());
  const KeymapDecide d{km->d_ctl, km->capacity, verdict};
  if (int rc = keymap_scan(KeymapFirst{km->d_slots, claim}, rank, n, sums, d, st)) return rc;
  hipLaunchKernelGGL(keymap_commit_kernel, dim3(grid), dim3(kTPB), 0, st, km->d_slots, keys, (u32)n,
                     (const u32*)claim, (const u32*)rank, (const u64*)km->d_ctl, km->first_row, km->capacity,
                     km->d_rev, out);
  HIPCHK(hipGetLastError());
  return GLINT_OK;
}

int keymap_lookup_launch(glint_keymap* km, const i64* keys, i64 n, i64 missing, i64* out, int verdict, hipStream_t st) {
  hipLaunchKernelGGL(keymap_lookup_kernel, dim3(keymap_grid(n, kTPB)), dim3(kTPB), 0, st,
                     (const KeymapSlot*)km->d_slots, (u32)(km->slots - 1), keys, (u32)n, missing, out,
                     km->d_ctl + verdict);
  HIPCHK(hipGetLastError());
  return GLINT_OK;
}

int keymap_keys_of_launch(glint_keymap* km, const i64* rows, i64 n, i64* out, int verdict, hipStream_t st) {
  hipLaunchKernelGGL(keymap_keys_of_kernel, dim3(keymap_grid(n, kTPB)), dim3(kTPB), 0, st, (const i64*)km->d_rev,
                     (const u64*)km->d_ctl, km->first_row, rows, (u32)n, out, km->d_ctl + verdict);
  HIPCHK(hipGetLastError());
  return GLINT_OK;
}

// A device-form call: `launch` on the caller's stream, under the map's lock.
template <typename F>
int keymap_dev_call(glint_keymap* km, void* stream, F launch) {
  std::lock_guard<std::mutex> lk(km->mu);
  DeviceGuard g(km->device);
  km->last_dev_stream = (hipStream_t)stream;
  km->dev_dirty = true;
  return launch((hipStream_t)stream);
}

// A host-form call: n values of `in` staged to the device on the map's stream -- after the work enqueued on
// the last device-form call's stream --, `launch` over them, n answers copied back to `out`, the control
// words with them; ends synchronised. A refusal of the call is in its own control pair, cleared here:
// *bad = the refused index or -1, *free_rows = the free rows of an insert that overflowed or -1.
template <typename F>
int keymap_host_call(glint_keymap* km, const int64_t* in, int64_t n, int64_t* out, int64_t* bad, int64_t* free_rows,
                     F launch) {
  std::lock_guard<std::mutex> lk(km->mu);
  DeviceGuard g(km->device);
  hipStream_t st = km->stream;
  if (km->dev_dirty) {
    if (!km->order_ev) HIPCHK(hipEventCreateWithFlags(&km->order_ev, hipEventDisableTiming));
    HIPCHK(hipEventRecord(km->order_ev, km->last_dev_stream));
    HIPCHK(hipStreamWaitEvent(st, km->order_ev, 0));
    km->dev_dirty = false;
  }
  const size_t bytes = (size_t)n * sizeof(i64);
  if (int rc = grow(&km->d_io, &km->io_bytes, 2 * bytes)) return rc;
  i64* d_in = (i64*)km->d_io;
  i64* d_out = d_in + n;
  int rc = GLINT_OK;
  if (hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, st) != hipSuccess) rc = GLINT_EDEVICE;
  if (rc == GLINT_OK) rc = launch((const i64*)d_in, d_out, st);
  if (rc == GLINT_OK && (hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, st) != hipSuccess ||
                         hipMemcpyAsync(km->h_ctl, km->d_ctl, kCtlWords * sizeof(u64), hipMemcpyDeviceToHost, st) !=
                             hipSuccess))
    rc = GLINT_EDEVICE;
  if (rc == GLINT_OK) {
    hipLaunchKernelGGL(keymap_clear_kernel, dim3(1), dim3(64), 0, st, km->d_ctl + kCtlHostBad);
    if (hipGetLastError() != hipSuccess) rc = GLINT_EDEVICE;
  }
  if (hipStreamSynchronize(st) != hipSuccess && rc == GLINT_OK) rc = GLINT_EDEVICE;
  if (rc) {
    (void)hipGetLastError();
    return rc;
  }
  const u64 b = km->h_ctl[kCtlHostBad], f = km->h_ctl[kCtlHostFree];
  if (b != kCtlNone && bad) *bad = (int64_t)b;
  if (b == kCtlNone && f != kCtlNone && free_rows) *free_rows = (int64_t)f;
  return (b != kCtlNone || f != kCtlNone) ? GLINT_EOUTOFRANGE : GLINT_OK;
}

}  // namespace

extern "C" {

int glint_keymap_create(int device, int64_t capacity, int64_t first_row, int64_t slots, glint_keymap_t* out) {
  if (out) *out = nullptr;
  if (!out || capacity < 1 || capacity >= kKeymapMaxSlots) return GLINT_EINVAL;
  if (slots == 0) slots = keymap_default_slots(capacity);
  if (!keymap_geometry_ok(capacity, first_row, slots)) return GLINT_EINVAL;
  DeviceGuard g(device);
  if (!g.ok) {
    (void)hipGetLastError();
    return GLINT_EDEVICE;
  }
  glint_keymap* km = new (std::nothrow) glint_keymap();
  if (!km) return GLINT_ENOMEM;
  km->device = device;
  km->capacity = capacity;
  km->first_row = first_row;
  km->slots = slots;
  int rc = GLINT_OK;
  if (hipMalloc((void**)&km->d_slots, (size_t)slots * sizeof(KeymapSlot)) != hipSuccess ||
      hipMalloc((void**)&km->d_rev, (size_t)capacity * sizeof(i64)) != hipSuccess ||
      hipMalloc((void**)&km->d_ctl, kCtlWords * sizeof(u64)) != hipSuccess ||
      hipHostMalloc((void**)&km->h_ctl, kCtlWords * sizeof(u64), hipHostMallocDefault) != hipSuccess) {
    (void)hipGetLastError();
    rc = GLINT_ENOMEM;
  }
  // (the scratch of calls of up to 2^17 records is allocated here, off every later call's path)
  if (rc == GLINT_OK)
    rc = grow(&km->d_scratch, &km->scratch_bytes, keymap_scratch_words((i64)1 << 17) * sizeof(u32));
  if (rc == GLINT_OK && hipStreamCreateWithFlags(&km->stream, hipStreamNonBlocking) != hipSuccess) rc = GLINT_EDEVICE;
  if (rc == GLINT_OK) {
    hipLaunchKernelGGL(keymap_fill_kernel, dim3(grid_for(slots, kTPB, 4096)), dim3(kTPB), 0, km->stream, km->d_slots,
                       (u32)slots, km->d_ctl);
    if (hipGetLastError() != hipSuccess || hipStreamSynchronize(km->stream) != hipSuccess) rc = GLINT_EDEVICE;
  }
  if (rc) {
    keymap_free(km);
    return rc;
  }
  *out = km;
  return GLINT_OK;
}

int glint_keymap_destroy(glint_keymap_t km) {
  if (!km) return GLINT_EINVAL;
  DeviceGuard g(km->device);
  keymap_free(km);
  return GLINT_OK;
}

int glint_keymap_info(glint_keymap_t km, int64_t* capacity, int64_t* first_row, int64_t* slots, int64_t* size,
                      int* device) {
  if (!km) return GLINT_EINVAL;
  if (capacity) *capacity = km->capacity;
  if (first_row) *first_row = km->first_row;
  if (slots) *slots = km->slots;
  if (device) *device = km->device;
  if (size) {  // lives on the device: read after everything enqueued there
    std::lock_guard<std::mutex> lk(km->mu);
    DeviceGuard g(km->device);
    HIPCHK(hipDeviceSynchronize());
    HIPCHK(hipMemcpy(km->h_ctl, km->d_ctl, sizeof(u64), hipMemcpyDeviceToHost));
    km->dev_dirty = false;
    *size = (int64_t)km->h_ctl[kCtlSize];
  }
  return GLINT_OK;
}

int glint_keymap_sync(glint_keymap_t km, void* stream, int64_t* bad, int64_t* free_rows) {
  if (bad) *bad = -1;
  if (free_rows) *free_rows = -1;
  if (!km) return GLINT_EINVAL;
  std::lock_guard<std::mutex> lk(km->mu);
  DeviceGuard g(km->device);
  hipStream_t st = (hipStream_t)stream;
  HIPCHK(hipMemcpyAsync(km->h_ctl, km->d_ctl, kCtlWords * sizeof(u64), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  if (st == km->last_dev_stream) km->dev_dirty = false;
  const u64 b = km->h_ctl[kCtlLatBad], f = km->h_ctl[kCtlLatFree];
  if (b == kCtlNone && f == kCtlNone) return GLINT_OK;
  if (b != kCtlNone && bad) *bad = (int64_t)b;
  if (b == kCtlNone && free_rows) *free_rows = (int64_t)f;
  hipLaunchKernelGGL(keymap_clear_kernel, dim3(1), dim3(64), 0, st, km->d_ctl + kCtlLatBad);
  HIPCHK(hipGetLastError());
  HIPCHK(hipStreamSynchronize(st));
  return GLINT_EOUTOFRANGE;
}

int glint_keymap_insert_dev(glint_keymap_t km, const int64_t* keys, int64_t n, int64_t* out, void* stream) {
  if (int rc = keymap_call_args(km, n, keys, out)) return rc;
  if (n == 0) return GLINT_OK;
  return keymap_dev_call(km, stream, [&](hipStream_t st) {
    return keymap_insert_launch(km, (const i64*)keys, n, (i64*)out, kCtlLatBad, st);
  });
}

int glint_keymap_lookup_dev(glint_keymap_t km, const int64_t* keys, int64_t n, int64_t missing, int64_t* out,
                            void* stream) {
  if (int rc = keymap_call_args(km, n, keys, out)) return rc;
  if (n == 0) return GLINT_OK;
  return keymap_dev_call(km, stream, [&](hipStream_t st) {
    return keymap_lookup_launch(km, (const i64*)keys, n, missing, (i64*)out, kCtlLatBad, st);
  });
}

int glint_keymap_keys_of_dev(glint_keymap_t km, const int64_t* rows, int64_t n, int64_t* out, void* stream) {
  if (int rc = keymap_call_args(km, n, rows, out)) return rc;
  if (n == 0) return GLINT_OK;
  return keymap_dev_call(km, stream, [&](hipStream_t st) {
    return keymap_keys_of_launch(km, (const i64*)rows, n, (i64*)out, kCtlLatBad, st);
  });
}

int glint_keymap_insert(glint_keymap_t km, const int64_t* keys, int64_t n, int64_t* out, int64_t* bad,
                        int64_t* free_rows) {
  if (bad) *bad = -1;
  if (free_rows) *free_rows = -1;
  if (int rc = keymap_call_args(km, n, keys, out)) return rc;
  if (n == 0) return GLINT_OK;
  return keymap_host_call(km, keys, n, out, bad, free_rows, [&](const i64* d_in, i64* d_out, hipStream_t st) {
    return keymap_insert_launch(km, d_in, n, d_out, kCtlHostBad, st);
  });
}

int glint_keymap_lookup(glint_keymap_t km, const int64_t* keys, int64_t n, int64_t missing, int64_t* out,
                        int64_t* bad) {
  if (bad) *bad = -1;
  if (int rc = keymap_call_args(km, n, keys, out)) return rc;
  if (n == 0) return GLINT_OK;
  return keymap_host_call(km, keys, n, out, bad, nullptr, [&](const i64* d_in, i64* d_out, hipStream_t st) {
    return keymap_lookup_launch(km, d_in, n, missing, d_out, kCtlHostBad, st);
  });
}

int glint_keymap_keys_of(glint_keymap_t km, const int64_t* rows, int64_t n, int64_t* out, int64_t* bad) {
  if (bad) *bad = -1;
  if (int rc = keymap_call_args(km, n, rows, out)) return rc;
  if (n == 0) return GLINT_OK;
  return keymap_host_call(km, rows, n, out, bad, nullptr, [&](const i64* d_in, i64* d_out, hipStream_t st) {
    return keymap_keys_of_launch(km, d_in, n, d_out, kCtlHostBad, st);
  });
}

}  // extern "C"
