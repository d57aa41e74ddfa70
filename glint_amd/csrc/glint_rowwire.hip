// glint_rowwire.hip -- narrow-format row transport (glint_mat_pull_rows_as*, glint_mat_push_rows_as*,
// DESIGN.md "Narrow-format row transport"): whole rows cross the link in a narrower floating type W than
// the shard's type V -- (Float, F16), (Float, BF16), (Double, F32) -- while the shard keeps full precision.
//   rows_pull_as   getRows with the rounding to W done here, so n x cols x sizeof W bytes go back: one wave
//                  per requested row, each lane 16 B of shard row in and the matching 8 B of W out
//                  (mat_pull_rows_kernel's frame);
//   rows_front     the row push's front end unchanged;
//   rows_fold_as   one wave per (item, column slice): shard slice + the run's contribution slices, strictly
//                  in list order (rows_fold_item's frame) -- the contribution a W load widened in registers,
//                  so nothing of size n x cols x sizeof V is ever built. Lane ownership of columns is the V
//                  side's: a lane's 16 B of shard row meet 8 B of contribution row.
// The conversions are glint_wire_plan.h's functions, bit for bit (tests/test_gpu_wire.py): widening is the
// hardware's exact conversion (BF16: a shift); narrowing to F16 and F32 is the hardware's round-to-nearest-even
// conversion with subnormals kept, narrowing to BF16 the contract's integer rule.
// Only `cols` elements of a shard row are read or written, never the pitch padding; the wire side has no pitch.
#include "glint_device.h"
#include "glint_host.h"
#include "glint_wire_plan.h"

namespace glint {

constexpr int kRowsDepth = 8;  // contribution slice loads in flight per wave (glint_rows.hip's kRowsDepth)
typedef uint16_t u16;          // an F16 or BF16 value as it crosses the link

// A wire type: its storage T (the bits as they cross the link), the shard type V it pairs with, and the
// pair's two conversions.
template <int WIRE>
struct Wire;
template <>
struct Wire<GLINT_WIRE_F16> {
  typedef u16 T;
  typedef float V;
  static __device__ __forceinline__ u16 narrow(float x) { return __builtin_bit_cast(u16, (_Float16)x); }
  static __device__ __forceinline__ float widen(u16 b) { return (float)__builtin_bit_cast(_Float16, b); }
};
template <>
struct Wire<GLINT_WIRE_BF16> {
  typedef u16 T;
  typedef float V;
  static __device__ __forceinline__ u16 narrow(float x) { return wire_f32_to_bf16(__builtin_bit_cast(u32, x)); }
  static __device__ __forceinline__ float widen(u16 b) { return __builtin_bit_cast(float, (u32)b << 16); }
};
template <>
struct Wire<GLINT_WIRE_F32> {
  typedef float T;
  typedef double V;
  static __device__ __forceinline__ float narrow(double x) { return (float)x; }
  static __device__ __forceinline__ double widen(float f) { return (double)f; }
};

// ---- pull ---------------------------------------------------------------------------------------------
// Persistent grid, one wave per requested row. VEC (cols * sizeof V a multiple of 16 and `out` 8-B aligned,
// so every wire row is): a lane turns one 16-B chunk of the shard row into 8 B of W -- 1 KiB in and 512 B
// out per wave instruction; else one element per lane. A row outside the partition is answered with zero
// bits by a wave-uniform branch, without a load, and recorded.
template <int WIRE, bool VEC>
__global__ __launch_bounds__(kTPB) void rows_pull_as_kernel(const i64* __restrict__ rows, i64 n,
                                                            const typename Wire<WIRE>::V* __restrict__ data,
                                                            PartDesc part, typename Wire<WIRE>::T* __restrict__ out,
                                                            ErrState* err) {
  typedef typename Wire<WIRE>::V V;
  typedef typename Wire<WIRE>::T T;
  constexpr int VPL = (int)(16 / sizeof(V));
  static_assert(VPL * sizeof(T) == 8, "a 16-B chunk of V is 8 B of W");
  const int lane = threadIdx.x & 63;
  const i64 w0 = (i64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const i64 nw = (i64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  for (i64 i = w0; i < n; i += nw) {
    const int32_t l = g2l(part, rows[i]);
    const bool ok = l >= 0 && l < part.size;  // wave-uniform
    if (!ok && lane == 0) record_error(err, i);
    const V* src = data + (ok ? (i64)l : 0) * part.pitch;
    T* dst = out + i * cols;
    if (VEC) {
      typedef __attribute__((ext_vector_type(4))) unsigned int U4;
      typedef __attribute__((ext_vector_type(2))) unsigned int U2;
      const i64 chunks = cols / VPL;
      if (ok) {
#pragma unroll 4
        for (i64 c = lane; c < chunks; c += 64) {
          const U4 q = reinterpret_cast<const U4*>(src)[c];
          V x[VPL];
          T t[VPL];
          __builtin_memcpy(x, &q, 16);
#pragma unroll
          for (int k = 0; k < VPL; ++k) t[k] = Wire<WIRE>::narrow(x[k]);
          U2 o;
          __builtin_memcpy(&o, t, 8);
          reinterpret_cast<U2*>(dst)[c] = o;
        }
      } else {
        for (i64 c = lane; c < chunks; c += 64) reinterpret_cast<U2*>(dst)[c] = U2{0u, 0u};
      }
    } else if (ok) {
      for (i64 c = lane; c < cols; c += 64) dst[c] = Wire<WIRE>::narrow(src[c]);
    } else {
      for (i64 c = lane; c < cols; c += 64) dst[c] = T(0);
    }
  }
}

// ---- push ---------------------------------------------------------------------------------------------
// A lane's part of a contribution row slice, as it lies on the wire: VPL values of W. WIDE: one 8-B load at
// column c (the columns of the lane's 16-B shard chunk; the row 8-B aligned); else element k at column
// c + 64 k (slice_load's two forms, glint_kernels.h).
template <int WIRE, int VPL, bool WIDE>
__device__ __forceinline__ void wire_slice_load(typename Wire<WIRE>::T (&x)[VPL],
                                                const typename Wire<WIRE>::T* __restrict__ row, i64 c, i64 cols) {
  typedef typename Wire<WIRE>::T T;
  typedef __attribute__((ext_vector_type(2))) unsigned int U2;
  if (WIDE) {
    U2 q = {0u, 0u};
    if (c < cols) q = *reinterpret_cast<const U2*>(row + c);
    __builtin_memcpy(x, &q, 8);
  } else {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const i64 cc = c + (i64)k * 64;
      x[k] = cc < cols ? row[cc] : T(0);
    }
  }
}

// Records [start, start + len) of the sorted list, folded in list order into one slice of row `drow`:
// rows_fold_item with the contribution loaded as W and widened at the add -- kRowsDepth loads in flight,
// held narrow until they are used, and the adds the only chain.
// ATOMIC (a chunk of a split run): the chunk's partial sum starts from zero and is added with device-scope
// atomics, each wave instruction over 64 consecutive elements. Otherwise the shard's slice is the first
// term and the sum is stored once.
template <int WIRE, int VPL, bool WIDE, bool ATOMIC>
__device__ __forceinline__ void rows_fold_as_item(const u32* __restrict__ idx, u32 start, u32 len,
                                                  const typename Wire<WIRE>::T* __restrict__ vals,
                                                  typename Wire<WIRE>::V* drow, i64 c, i64 cols, int lane) {
  typedef typename Wire<WIRE>::V V;
  typedef typename Wire<WIRE>::T T;
  V acc[VPL];
  if (ATOMIC) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) acc[k] = V(0);
  } else {
    slice_load<V, VPL, WIDE>(acc, drow, c, cols);
  }
  for (u32 b = 0; b < len; b += 64) {
    const u32 m = len - b < 64u ? len - b : 64u;
    const u32 mine = (u32)lane < m ? idx[(i64)start + b + lane] : 0u;  // 64 record indices, one per lane
    for (u32 j = 0; j < m; j += kRowsDepth) {
      T t[kRowsDepth][VPL];
      const bool full = m - j >= (u32)kRowsDepth;  // else the run's last few records (wave-uniform tests)
#pragma unroll
      for (int d = 0; d < kRowsDepth; ++d) {
        if (full || j + d < m) {
          const u32 id = (u32)__builtin_amdgcn_readlane((int)mine, (int)(j + d));
          wire_slice_load<WIRE, VPL, WIDE>(t[d], vals + (i64)id * cols, c, cols);
        }
      }
#pragma unroll
      for (int d = 0; d < kRowsDepth; ++d) {
        if (full || j + d < m) {
#pragma unroll
          for (int k = 0; k < VPL; ++k) acc[k] = vadd(acc[k], Wire<WIRE>::widen(t[d][k]));
        }
      }
    }
  }
  if (ATOMIC) {
#pragma unroll
    for (int k = 0; k < VPL; ++k) {
      const i64 cc = c + (i64)k * 64;
      if (cc < cols) gadd(drow + cc, acc[k]);
    }
  } else {
    slice_store<V, VPL, WIDE>(acc, drow, c, cols);
  }
}

// Persistent grid; one wave per (item, column slice), the slices of an item on adjacent waves
// (rows_fold_kernel's frame). A slice is 64 lanes x 16 B of shard row when VEC16 (cols * sizeof V a multiple
// of 16 and `vals` 8-B aligned, so every contribution row is; the shard's pitch always is 16-B aligned), else
// one element per lane.
template <int WIRE, bool VEC16, bool SPLIT>
__global__ __launch_bounds__(kTPB) void rows_fold_as_kernel(const u32* __restrict__ key, const u32* __restrict__ idx,
                                                            const uint2* __restrict__ items,
                                                            const u32* __restrict__ nitems,
                                                            const typename Wire<WIRE>::T* __restrict__ vals,
                                                            typename Wire<WIRE>::V* data, PartDesc part) {
  typedef typename Wire<WIRE>::V V;
  constexpr int VPL = VEC16 ? (int)(16 / sizeof(V)) : 1;
  const int lane = threadIdx.x & 63;
  // the wave's index as a scalar: the item, its run and the record indices are then wave-uniform to the
  // compiler too (rows_fold_kernel's pattern)
  const u64 w0 = (u64)blockIdx.x * (kTPB / 64) + (u32)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  const u64 nw = (u64)gridDim.x * (kTPB / 64);
  const i64 cols = part.cols;
  const u32 nslices = (u32)((cols + 64 * VPL - 1) / (64 * VPL));
  const u64 total = (u64)*nitems * nslices;
  for (u64 w = w0; w < total; w += nw) {
    const u32 it = (u32)(w / nslices), slice = (u32)(w % nslices);
    const uint2 e = items[it];
    const bool chunk = SPLIT && (e.y & kRowsSplitBit) != 0;
    const u32 len = SPLIT ? e.y & ~kRowsSplitBit : e.y;
    V* drow = data + (i64)key[e.x] * part.pitch;
    const i64 c0 = (i64)slice * 64 * VPL;
    if (chunk) rows_fold_as_item<WIRE, VPL, false, true>(idx, e.x, len, vals, drow, c0 + lane, cols, lane);
    else rows_fold_as_item<WIRE, VPL, VEC16, false>(idx, e.x, len, vals, drow, VEC16 ? c0 + (i64)lane * VPL : c0 + lane, cols, lane);
  }
}

// ---- host side ----------------------------------------------------------------------------------------
namespace {

template <int WIRE>
int pull_rows_as(glint_shard* s, const i64* rows, void* out, i64 n, hipStream_t st) {
  typedef typename Wire<WIRE>::V V;
  typedef typename Wire<WIRE>::T T;
  const bool vec = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(out, 8);
  const unsigned g = grid_for(n, kTPB / 64, (i64)s->cus * 8);
  HIPCHK(launch_k(s, GLINT_K_MAT_PULL_ROWS, vec ? rows_pull_as_kernel<WIRE, true> : rows_pull_as_kernel<WIRE, false>, g,
                  kTPB, st, rows, n, (const V*)s->data, s->part, (T*)out, err_of(s)));
  return GLINT_OK;
}

template <int WIRE>
int push_rows_as(glint_shard* s, const i64* rows, const void* vals, i64 n, int flags, hipStream_t st) {
  typedef typename Wire<WIRE>::V V;
  typedef typename Wire<WIRE>::T T;
  RowsFront f;
  int rc = rows_front(s, rows, n, flags, st, &f);
  if (rc) return rc;
  const bool v16 = ((i64)s->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(vals, 8);
  const i64 slices = row_slices<V>(s->part.cols, v16);
  const unsigned gf = grid_for(n * slices, kTPB / 64, (i64)s->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const T*, V*, PartDesc) =
      v16 ? (f.strict ? rows_fold_as_kernel<WIRE, true, false> : rows_fold_as_kernel<WIRE, true, true>)
          : (f.strict ? rows_fold_as_kernel<WIRE, false, false> : rows_fold_as_kernel<WIRE, false, true>);
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, (const T*)vals,
                  (V*)s->data, s->part));
  return GLINT_OK;
}

}  // namespace

// Enqueues a narrow-format row pull of n rows on st (no host synchronisation): one launch. Under the
// shard's lock.
int pull_rows_wire(glint_shard* s, const i64* rows, void* out, i64 n, int wire, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !out || !wire_supported(s->dtype, wire)) return GLINT_EINVAL;
  if (n >= ((i64)1 << 31)) return GLINT_EINVAL;
  switch (wire) {
    case GLINT_WIRE_F16: return pull_rows_as<GLINT_WIRE_F16>(s, rows, out, n, st);
    case GLINT_WIRE_BF16: return pull_rows_as<GLINT_WIRE_BF16>(s, rows, out, n, st);
    default: return pull_rows_as<GLINT_WIRE_F32>(s, rows, out, n, st);
  }
}

// Enqueues a narrow-format row push of n records on st (no host synchronisation): the front end's launches
// and the one fold launch. Under the shard's lock.
int push_rows_wire(glint_shard* s, const i64* rows, const void* vals, i64 n, int wire, int flags, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (!rows || !vals || !wire_supported(s->dtype, wire)) return GLINT_EINVAL;
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  switch (wire) {
    case GLINT_WIRE_F16: return push_rows_as<GLINT_WIRE_F16>(s, rows, vals, n, flags, st);
    case GLINT_WIRE_BF16: return push_rows_as<GLINT_WIRE_BF16>(s, rows, vals, n, flags, st);
    default: return push_rows_as<GLINT_WIRE_F32>(s, rows, vals, n, flags, st);
  }
}

}  // namespace glint
