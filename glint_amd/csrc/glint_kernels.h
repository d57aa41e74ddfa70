// glint_kernels.h -- gfx950 kernels of the push/pull reduction plane.
//
// The shard is the HBM image of a Glint partial model's `data` array
// (src/main/scala/glint/models/server/PartialVector.scala:27, PartialMatrix.scala:28):
// vector shard = V[size], matrix shard = row-major V[size][pitch] (pitch = cols rounded up to
// 16 B so every row starts 16-B aligned; Array[Array[V]] has no cross-row layout to preserve).
//
// Record "address" = the element a record touches:
//   vector: (int)(key - start)                 RangePartition.globalToLocal (RangePartition.scala:33)
//           (int)((key - index) / P)           CyclicPartition.globalToLocal (CyclicPartition.scala:45-47)
//   matrix: globalToLocal(row) * pitch + col   PartialMatrix.update (PartialMatrix.scala:77-79)
// A record is rejected (GLINT_EOUTOFRANGE) exactly when the JVM would throw
// ArrayIndexOutOfBoundsException: local index outside [0, size) or col outside [0, cols).
//
// Push = up to three stream-ordered kernels:
//   push_check    reads the keys once; finds the first 1024-record wave tile whose record addresses
//                 stop being strictly increasing (within the tile or across its left edge), and
//                 marks AFFINE tiles (record r hits element base + r), whose addresses push_apply
//                 then knows without reading the keys again.
//   push_apply    every tile before that break: the prefix's addresses are strictly increasing,
//                 hence unique, so records are applied with PLAIN coalesced read-modify-write
//                 (16-B accesses when two consecutive records hit adjacent elements) -- bit-exact
//                 with the reference's sequential loop.
//   push_scatter  records [break*TILE, n) -- nothing when the whole call was increasing -- by LDS
//                 hash aggregation (duplicate addresses within a chunk summed in LDS) followed by one
//                 device-scope atomic add per distinct address; or, in deterministic mode, a stable
//                 sort by address and an in-order fold per address.
// Kernel boundaries order check -> apply -> scatter: every plain store precedes every atomic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "glint_push_plan.h"  // i64 / u64 / u32, kPPT, kTile, kOrderedMax, kPushHostSequential

namespace glint {

constexpr int kTPB = 256;          // threads per block (4 waves)
constexpr i64 kNotAffine = (i64)0x8000000000000000ll;  // tile descriptor: addresses not base + r
constexpr int kHashSlots = 4096;   // LDS hash table slots in push_scatter (64 KiB for 8-B V)
constexpr int kScatterChunk = 2048;  // records per block iteration in push_scatter (load <= 0.5)

// per-launch control words, zeroed by one hipMemsetAsync before push_check
struct LaunchCtl {
  u32 brk_enc;    // max over tiles that break the increasing order of (ntiles - t); 0 = none
  u32 nonaffine;  // some tile is not affine or does not continue its predecessor's affine run
  u32 cancel;     // a gated push whose gate word was set: it applies nothing (push_gate_kernel)
  u32 ticket;     // push_apply's ticket counter (sweep_ticket / tile_ticket in glint_push_plan.h)
  u64 bad;        // a validating gated push: max of ~index over its out-of-range records (push_check)
};

// persistent error state, cleared by glint_shard_sync / host-pointer calls
struct ErrState {
  u64 min_bad_enc;  // max of ~index over rejected records; 0 = none
  u64 count;        // number of rejected records
};

// Completion of a single-workgroup launch on the pinned-ring path (message-sized host calls): the
// kernel itself writes the shard's error state and then its ticket to host-mapped words, so the
// host waits on memory -- no event marker and no error copy in the stream (glint_gpu.hip, ring_*).
struct MsgSig {
  u64* done;       // host-mapped ticket word; nullptr = an ordinary launch
  u64 ticket;
  ErrState* herr;  // host-mapped: the error state after this launch
};

// A coalesced ring pull's answer destinations, one per message (the table sits in the slot, after
// the answer section): records [off, off + n) of the batch are written to dst -- a glint_host_alloc
// buffer the caller answers from, or the slot's own answer section.
struct PullDst {
  unsigned int off, n;
  unsigned long long dst;  // device address
};
constexpr int kPullDirectMax = 256;  // messages per batch with a destination table, at most

// Partition -> local index, for both partitioner kinds (kind is launch-uniform)
struct PartDesc {
  int32_t kind;   // 0 range, 1 cyclic
  int32_t size;   // Partition.size: vector elements or matrix rows
  int64_t start;  // RangePartition.start
  int32_t cidx;   // CyclicPartition.index
  int32_t cparts; // CyclicPartition.numberOfPartitions
  int32_t cols;   // 0 = vector
  int32_t pad_;
  int64_t pitch;  // elements per row (matrix)
};

// KIND: 0 range, 1 cyclic (a kernel specialised per layout keeps the cyclic 64-bit division out of
// the range hot path), -1 = read p.kind at run time
template <int KIND = -1>
__device__ __forceinline__ int32_t g2l(const PartDesc& p, i64 key) {
  if (KIND == 0 || (KIND < 0 && p.kind == 0)) return (int32_t)(key - p.start);
  return (int32_t)((key - (i64)p.cidx) / (i64)p.cparts);
}

// Row slices, shared by the row push's fold (glint_rows.hip), the grouped row-sum pull
// (glint_rowsum.hip) and the row dot pull (glint_rowdot.hip).
// A lane's part of a row slice: VPL values. WIDE: one 16-B access at column c (VPL * sizeof(V) == 16,
// cols a multiple of VPL, the row 16-B aligned); else element k at column c + 64 k, so that each
// wave instruction covers 64 consecutive elements.
template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void slice_load(V (&x)[VPL], const V* __restrict__ row, i64 c, i64 cols) {
  typedef __attribute__((ext_vector_type(4))) unsigned int U4;
  if (WIDE) {
    U4 q = {0u, 0u, 0u, 0u};
    if (c < cols) q = *reinterpret_cast<const U4*>(row + c);
    __builtin_memcpy(x, &q, 16);
  } else {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const i64 cc = c + (i64)k * 64;
      x[k] = cc < cols ? row[cc] : V(0);
    }
  }
}

template <typename V, int VPL, bool WIDE>
__device__ __forceinline__ void slice_store(const V (&x)[VPL], V* row, i64 c, i64 cols) {
  typedef __attribute__((ext_vector_type(4))) unsigned int U4;
  if (WIDE) {
    U4 q;
    __builtin_memcpy(&q, x, 16);
    if (c < cols) *reinterpret_cast<U4*>(row + c) = q;
  } else {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const i64 cc = c + (i64)k * 64;
      if (cc < cols) row[cc] = x[k];
    }
  }
}

template <typename V>
struct PushArgs {
  const i64* keys;      // keys (vector) or rows (matrix)
  const int32_t* cols;  // matrix only
  const V* vals;
  i64 n;
  V* data;
  i64 elems;  // elements allocated in the shard
  PartDesc part;
  LaunchCtl* ctl;
  u32 ntiles;
  ErrState* err;
  u32 sweep_blocks;  // blocks of push_apply that take part in the affine sweep (<= grid)
  u64* hint;  // host-mapped word: the unordered-tail size push_apply saw (binned-path heuristic)
  MsgSig sig;  // ring launches only (one workgroup)
};

}  // namespace glint
