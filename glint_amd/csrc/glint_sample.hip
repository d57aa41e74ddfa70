// glint_sample.hip -- the seeded weighted row sampler (glint_sampler_*, DESIGN.md "Row sampler"): an
// immutable cumulative table on the device, built once from integer weights, and draws that are a function
// of (table, seed, counter, excluded key) only -- glint_sample_plan.h states that function, and this file
// only decides how the table is built and how the search is shaped.
//   build   sample_totals (the weight check and the tile sums) -> the same two kernels over the tile sums,
//           level by level -> sample_scan (the inclusive cdf, out of place: the weights are only read) ->
//           sample_coarse (every 2^shift-th cdf entry).
//   draw    one launch, a persistent grid: a workgroup loads the coarse table into LDS once, then each thread
//           takes kSampleDraws draws per round -- Philox, the high product, the coarse search in LDS, the rest
//           of the search in global memory with the loads of its draws issued together -- and stores one
//           key per draw, coalesced. Only a draw whose attempt 0 hit its excluded key leaves the lockstep.
// No atomics but the build's record of a bad weight, no inline assembly, no scratch in a draw.
#include "glint_device.h"
#include "glint_host.h"
#include "glint_sample_plan.h"

#include <new>

namespace glint {

constexpr int kSampleCoarse = GLINT_SAMPLE_COARSE;
// (1 is the flat search: a coarse table of the total alone, every step in global memory)
static_assert((kSampleCoarse & (kSampleCoarse - 1)) == 0 && kSampleCoarse >= 1, "the coarse search halves a power of two");
// draws per thread and round (measured: DESIGN.md "Row sampler")
#ifndef GLINT_SAMPLE_DRAWS
#define GLINT_SAMPLE_DRAWS 2
#endif
constexpr int kSampleDraws = GLINT_SAMPLE_DRAWS;
constexpr int kSampleTile = 1024;  // weights one scan workgroup covers
constexpr int kSampleItems = kSampleTile / kTPB;
static_assert(kSampleItems * kTPB == kSampleTile, "a scan tile is a whole number of weights per thread");
constexpr i64 kSampleHostChunk = (i64)1 << 22;  // draws per launch of a host draw (its staging: 32 MiB of keys)

// a weight as the table takes it; false for one outside [0, 2^32)
__device__ __forceinline__ bool sample_weight(long long w, u64& v) {
  v = (u64)w;
  return (v >> 32) == 0;
}
__device__ __forceinline__ bool sample_weight(int w, u64& v) {
  v = (u64)(u32)w;
  return w >= 0;
}
__device__ __forceinline__ bool sample_weight(u64 w, u64& v) {  // a tile sum of a level below: any value
  v = w;
  return true;
}

// tot[b] = the sum of tile b of x[0 .. m); *bad = the lowest index of a weight outside [0, 2^32) (it adds 0)
template <typename W>
__global__ __launch_bounds__(kTPB) void sample_totals_kernel(const W* __restrict__ x, i64 m, u64* __restrict__ tot,
                                                             u64* bad) {
  __shared__ u64 lds[kTPB / 64];
  const i64 at = (i64)blockIdx.x * kSampleTile + (i64)threadIdx.x * kSampleItems;
  u64 v = 0;
#pragma unroll
  for (int k = 0; k < kSampleItems; ++k) {
    if (at + k >= m) break;
    u64 w;
    if (sample_weight(x[at + k], w)) v += w;
    else atomicMin(bad, (u64)(at + k));
  }
#pragma unroll
  for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
  if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) {
    u64 t = 0;
#pragma unroll
    for (int w = 0; w < kTPB / 64; ++w) t += lds[w];
    tot[blockIdx.x] = t;
  }
}

// out[i] = base[tile] + x[tile start] + ... + x[i] (INCL) or ... + x[i - 1] (else); base == nullptr: 0 (a
// single tile). out may be x itself: a thread reads its own entries before it writes them.
template <typename W, bool INCL>
__global__ __launch_bounds__(kTPB) void sample_scan_kernel(const W* x, u64* out, i64 m, const u64* __restrict__ base) {
  __shared__ u64 lds[kTPB / 64];
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const i64 at = (i64)blockIdx.x * kSampleTile + (i64)threadIdx.x * kSampleItems;
  u64 v[kSampleItems];
  u64 mine = 0;
#pragma unroll
  for (int k = 0; k < kSampleItems; ++k) {
    v[k] = 0;
    if (at + k < m) {
      u64 w;
      if (sample_weight(x[at + k], w)) v[k] = w;
    }
    mine += v[k];
  }
  u64 inc = mine;  // inclusive prefix over the wave's lanes
#pragma unroll
  for (int d = 1; d < 64; d <<= 1) {
    const u64 o = __shfl_up(inc, d, 64);
    if (lane >= d) inc += o;
  }
  if (lane == 63) lds[wave] = inc;
  __syncthreads();
  u64 run = base ? base[blockIdx.x] : 0;
  for (int w = 0; w < wave; ++w) run += lds[w];
  run += inc - mine;
#pragma unroll
  for (int k = 0; k < kSampleItems; ++k) {
    if (INCL) run += v[k];
    if (at + k < m) out[at + k] = run;
    if (!INCL) run += v[k];
  }
}

// coarse[j] = the cdf at the end of block j (glint_sample_plan.h, the coarse table's geometry)
__global__ __launch_bounds__(kTPB) void sample_coarse_kernel(const u64* __restrict__ cdf, i64 m, int shift,
                                                             u64* __restrict__ coarse) {
  const int j = blockIdx.x * kTPB + threadIdx.x;
  if (j >= kSampleCoarse) return;
  const i64 e = (((i64)j + 1) << shift) - 1;
  coarse[j] = cdf[e < m - 1 ? e : m - 1];
}

// The table as a draw sees it: glint_sample_plan.h's Table with the two-level search. `lds` holds the coarse
// table. Both levels are branch-free halvings of a power of two with the comparison `<= x`: a level's answer
// is the count of its entries <= x, which is below its length because its last entry -- the total for the
// coarse table, the block's coarse entry for a block; an index past m - 1 reads the total -- is > x.
struct SampleTwoLevel {
  const u64* lds;
  const u64* __restrict__ cdf;
  i64 m;
  int shift;
  __device__ __forceinline__ u64 at(i64 i) const { return cdf[i]; }
  // upper(x[k]) for N points at once: the N loads of a step are independent and issue together
  template <int N>
  __device__ __forceinline__ void upper_n(const u64 (&x)[N], i64 (&idx)[N]) const {
    u32 pos[N];
#pragma unroll
    for (int k = 0; k < N; ++k) pos[k] = 0;
#pragma unroll
    for (u32 h = kSampleCoarse / 2; h > 0; h >>= 1) {
#pragma unroll
      for (int k = 0; k < N; ++k) pos[k] += lds[pos[k] + h - 1] <= x[k] ? h : 0u;
    }
    const i64 last = m - 1;
#pragma unroll
    for (int k = 0; k < N; ++k) idx[k] = (i64)pos[k] << shift;
    for (int s = shift - 1; s >= 0; --s) {
      const i64 h = (i64)1 << s;
      u64 c[N];
#pragma unroll
      for (int k = 0; k < N; ++k) {
        const i64 e = idx[k] + h - 1;
        c[k] = cdf[e < last ? e : last];
      }
#pragma unroll
      for (int k = 0; k < N; ++k) idx[k] += c[k] <= x[k] ? h : 0;
    }
  }
  __device__ __forceinline__ i64 upper(u64 x) const {
    const u64 xs[1] = {x};
    i64 r[1];
    upper_n<1>(xs, r);
    return r[0];
  }
};

struct SampleArgs {
  const u64* cdf;
  const u64* coarse;
  i64 m, first_key;
  u64 total;
  int shift;
  u64 seed, first;  // draw j of the launch has counter first + i0 + j
  u32 i0;           // index of the launch's first draw in its call (a host draw is cut into launches)
  u32 n;
  u32 per;          // min(per, 2^31): a call's draw indices are below 2^31
  u32 ex0;          // exclude[0] of the launch is the call's exclude[ex0]
};

template <bool EXCL>
__global__ __launch_bounds__(kTPB) void sample_draw_kernel(SampleArgs a, const i64* __restrict__ exclude,
                                                           i64* __restrict__ out) {
  __shared__ u64 lds[kSampleCoarse];
  for (int k = threadIdx.x; k < kSampleCoarse; k += kTPB) lds[k] = a.coarse[k];
  __syncthreads();
  const SampleTwoLevel tab{lds, a.cdf, a.m, a.shift};
  constexpr u32 kRound = (u32)kTPB * kSampleDraws;
  // (n < 2^31 and the grid covers at most n + kRound draws: no 32-bit index wraps)
  for (u32 base = blockIdx.x * kRound; base < a.n; base += gridDim.x * kRound) {
    u64 x[kSampleDraws];
    i64 idx[kSampleDraws];
#pragma unroll
    for (int k = 0; k < kSampleDraws; ++k) {
      const u32 j = base + (u32)k * kTPB + threadIdx.x;
      x[k] = j < a.n ? sample_point(a.seed, a.first + a.i0 + j, 0u, a.total) : 0;
    }
    tab.upper_n<kSampleDraws>(x, idx);
#pragma unroll
    for (int k = 0; k < kSampleDraws; ++k) {
      const u32 j = base + (u32)k * kTPB + threadIdx.x;
      if (j >= a.n) continue;
      i64 i = idx[k];
      if (EXCL) {
        const i64 forb = sample_forbidden(exclude[(a.i0 + j) / a.per - a.ex0], a.first_key, a.m);
        if (i == forb) i = sample_avoid(tab, a.total, a.seed, a.first + a.i0 + j, forb, i);
      }
      out[j] = a.first_key + i;
    }
  }
}

}  // namespace glint

struct glint_sampler {
  int device = 0;
  int cus = 256;
  i64 m = 0, first_key = 0;
  u64 total = 0;
  int shift = 0;
  u64* table = nullptr;  // cdf[m], then coarse[kSampleCoarse]
  // host draws only (glint_sampler_draw), under mu: a private stream and grow-only staging
  std::mutex mu;
  hipStream_t stream = nullptr;
  void* d_io = nullptr;
  size_t io_bytes = 0;
};

namespace {

void sampler_free(glint_sampler* sp) {
  if (sp->table) (void)hipFree(sp->table);
  if (sp->d_io) (void)hipFree(sp->d_io);
  if (sp->stream) (void)hipStreamDestroy(sp->stream);
  (void)hipGetLastError();
  delete sp;
}

// the scan of x[0 .. m) into out on st: inclusive at the level of the weights (TOP), exclusive -- in place --
// over the tile sums above it; scratch holds the tile sums of this level and of the levels above
template <typename W, bool TOP>
int sample_scan(const W* x, u64* out, i64 m, u64* scratch, u64* bad, hipStream_t st) {
  const i64 tiles = (m + kSampleTile - 1) / kSampleTile;
  if (tiles <= 1 && !TOP) {
    hipLaunchKernelGGL((sample_scan_kernel<W, TOP>), dim3(1), dim3(kTPB), 0, st, x, out, m, (const u64*)nullptr);
    HIPCHK(hipGetLastError());
    return GLINT_OK;
  }
  // (the level of the weights always runs sample_totals: it is the weight check)
  hipLaunchKernelGGL((sample_totals_kernel<W>), dim3((unsigned)tiles), dim3(kTPB), 0, st, x, m, scratch, bad);
  HIPCHK(hipGetLastError());
  if (int rc = sample_scan<u64, false>(scratch, scratch, tiles, scratch + tiles, bad, st)) return rc;
  hipLaunchKernelGGL((sample_scan_kernel<W, TOP>), dim3((unsigned)tiles), dim3(kTPB), 0, st, x, out, m,
                     (const u64*)scratch);
  HIPCHK(hipGetLastError());
  return GLINT_OK;
}

inline size_t sample_scan_scratch(i64 m) {
  size_t words = 0;
  i64 t = m;
  do {
    t = (t + kSampleTile - 1) / kSampleTile;
    words += (size_t)t;
  } while (t > 1);
  return words;
}

template <typename W>
int sampler_fill(glint_sampler* sp, const W* w, u64* scratch, hipStream_t st, u64 back[2]) {
  u64* bad = scratch;  // then the tile sums
  HIPCHK(hipMemsetAsync(bad, 0xFF, sizeof(u64), st));
  if (int rc = sample_scan<W, true>(w, sp->table, sp->m, scratch + 1, bad, st)) return rc;
  hipLaunchKernelGGL(sample_coarse_kernel, dim3((kSampleCoarse + kTPB - 1) / kTPB), dim3(kTPB), 0, st,
                     (const u64*)sp->table, sp->m, sp->shift, sp->table + sp->m);
  HIPCHK(hipGetLastError());
  HIPCHK(hipMemcpyAsync(&back[0], bad, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIPCHK(hipMemcpyAsync(&back[1], sp->table + sp->m - 1, sizeof(u64), hipMemcpyDeviceToHost, st));
  HIPCHK(hipStreamSynchronize(st));
  return GLINT_OK;
}

}  // namespace

namespace glint {

// Builds a sampler over the m weights at w (device memory of `device`; Int when w32, else Long) with the
// launches on st, and ends with st synchronised: the weight check, the scan, the coarse table. On the
// current device = `device`. *out stays NULL on any error; *first_bad (may be NULL) = the lowest bad index
// or -1.
int sampler_build(int device, const void* w, bool w32, i64 m, i64 first_key, hipStream_t st, int64_t* first_bad,
                  glint_sampler** out) {
  glint_sampler* sp = new (std::nothrow) glint_sampler();
  if (!sp) return GLINT_ENOMEM;
  sp->device = device;
  sp->m = m;
  sp->first_key = first_key;
  sp->shift = sample_coarse_shift(m, kSampleCoarse);
  int cus = 0;
  if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device) == hipSuccess && cus > 0) sp->cus = cus;
  u64* scratch = nullptr;
  int rc = GLINT_OK;
  if (hipMalloc((void**)&sp->table, ((size_t)m + kSampleCoarse) * sizeof(u64)) != hipSuccess ||
      hipMalloc((void**)&scratch, (sample_scan_scratch(m) + 1) * sizeof(u64)) != hipSuccess) {
    (void)hipGetLastError();
    rc = GLINT_ENOMEM;
  }
  u64 back[2] = {0, 0};
  if (rc == GLINT_OK) {
    rc = w32 ? sampler_fill(sp, (const int*)w, scratch, st, back) : sampler_fill(sp, (const long long*)w, scratch, st, back);
    if (rc) (void)hipStreamSynchronize(st);  // (nothing of the failed build may still run when its memory goes)
  }
  if (scratch) (void)hipFree(scratch);
  if (rc == GLINT_OK && back[0] != ~(u64)0) {
    if (first_bad) *first_bad = (int64_t)back[0];
    rc = GLINT_EOUTOFRANGE;
  }
  if (rc == GLINT_OK && back[1] == 0) rc = GLINT_EINVAL;
  if (rc) {
    sampler_free(sp);
    return rc;
  }
  sp->total = back[1];
  *out = sp;
  return GLINT_OK;
}

}  // namespace glint

namespace {

inline int sampler_create_args(const void* weights, int64_t m, int64_t* first_bad, glint_sampler_t* out) {
  if (out) *out = nullptr;
  if (first_bad) *first_bad = -1;
  return (!out || !weights || m < 1 || m >= ((int64_t)1 << 31)) ? GLINT_EINVAL : GLINT_OK;
}

inline int sampler_draw_args(const glint_sampler* sp, int64_t n, const void* exclude, int64_t per, const void* out) {
  if (!sp || n < 0 || n >= ((int64_t)1 << 31) || (n > 0 && !out) || (exclude && per < 1)) return GLINT_EINVAL;
  return GLINT_OK;
}

// one launch: draws [i0, i0 + n) of a call whose exclude[ex0 ..] is at `exclude` (device; nullptr: none)
int sampler_launch(const glint_sampler* sp, u64 seed, u64 first, i64 i0, i64 n, const i64* exclude, i64 per, i64 ex0,
                   i64* out, hipStream_t st) {
  SampleArgs a{};
  a.cdf = sp->table;
  a.coarse = sp->table + sp->m;
  a.m = sp->m;
  a.first_key = sp->first_key;
  a.total = sp->total;
  a.shift = sp->shift;
  a.seed = seed;
  a.first = first;
  a.i0 = (u32)i0;
  a.n = (u32)n;
  a.per = exclude ? (u32)std::min<i64>(per, (i64)1 << 31) : 1u;
  a.ex0 = (u32)ex0;
  const unsigned grid = grid_for(n, (i64)kTPB * kSampleDraws, (i64)sp->cus * 8);
  if (exclude) hipLaunchKernelGGL(sample_draw_kernel<true>, dim3(grid), dim3(kTPB), 0, st, a, exclude, out);
  else hipLaunchKernelGGL(sample_draw_kernel<false>, dim3(grid), dim3(kTPB), 0, st, a, exclude, out);
  HIPCHK(hipGetLastError());
  return GLINT_OK;
}

}  // namespace

extern "C" {

int glint_sampler_create(int device, const int64_t* weights, int64_t m, int64_t first_key, int64_t* first_bad,
                         glint_sampler_t* out) {
  if (int rc = sampler_create_args(weights, m, first_bad, out)) return rc;
  DeviceGuard g(device);
  if (!g.ok) {
    (void)hipGetLastError();
    return GLINT_EDEVICE;
  }
  // staged through a buffer and a stream of the call's own, both gone when it returns
  hipStream_t st = nullptr;
  void* w = nullptr;
  HIPCHK(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
  int rc = GLINT_OK;
  if (hipMalloc(&w, (size_t)m * sizeof(int64_t)) != hipSuccess) {
    (void)hipGetLastError();
    rc = GLINT_ENOMEM;
  } else if (hipMemcpyAsync(w, weights, (size_t)m * sizeof(int64_t), hipMemcpyHostToDevice, st) != hipSuccess) {
    (void)hipGetLastError();
    (void)hipStreamSynchronize(st);
    rc = GLINT_EDEVICE;
  }
  if (rc == GLINT_OK) rc = sampler_build(device, w, false, m, first_key, st, first_bad, out);
  if (w) (void)hipFree(w);
  (void)hipStreamDestroy(st);
  return rc;
}

int glint_sampler_create_dev(int device, const int64_t* weights_dev, int64_t m, int64_t first_key, void* stream,
                             int64_t* first_bad, glint_sampler_t* out) {
  if (int rc = sampler_create_args(weights_dev, m, first_bad, out)) return rc;
  DeviceGuard g(device);
  if (!g.ok) {
    (void)hipGetLastError();
    return GLINT_EDEVICE;
  }
  return sampler_build(device, weights_dev, false, m, first_key, (hipStream_t)stream, first_bad, out);
}

int glint_sampler_destroy(glint_sampler_t sp) {
  if (!sp) return GLINT_EINVAL;
  DeviceGuard g(sp->device);
  sampler_free(sp);
  return GLINT_OK;
}

int glint_sampler_info(glint_sampler_t sp, int64_t* m, int64_t* first_key, int64_t* total, int* device) {
  if (!sp) return GLINT_EINVAL;
  if (m) *m = sp->m;
  if (first_key) *first_key = sp->first_key;
  if (total) *total = (int64_t)sp->total;
  if (device) *device = sp->device;
  return GLINT_OK;
}

int glint_sampler_draw_dev(glint_sampler_t sp, uint64_t seed, uint64_t first, int64_t n, const int64_t* exclude,
                           int64_t per, int64_t* out, void* stream) {
  if (int rc = sampler_draw_args(sp, n, exclude, per, out)) return rc;
  if (n == 0) return GLINT_OK;
  DeviceGuard g(sp->device);
  return sampler_launch(sp, seed, first, 0, n, (const i64*)exclude, per, 0, (i64*)out, (hipStream_t)stream);
}

int glint_sampler_draw(glint_sampler_t sp, uint64_t seed, uint64_t first, int64_t n, const int64_t* exclude,
                       int64_t per, int64_t* out) {
  if (int rc = sampler_draw_args(sp, n, exclude, per, out)) return rc;
  if (n == 0) return GLINT_OK;
  std::lock_guard<std::mutex> lk(sp->mu);
  DeviceGuard g(sp->device);
  if (!sp->stream) HIPCHK(hipStreamCreateWithFlags(&sp->stream, hipStreamNonBlocking));
  // launch by launch of at most kSampleHostChunk draws: the launch's part of exclude in, its keys out
  for (i64 i0 = 0; i0 < n; i0 += kSampleHostChunk) {
    const i64 cn = std::min(kSampleHostChunk, n - i0);
    const i64 ex0 = exclude ? i0 / per : 0;
    const i64 exn = exclude ? (i0 + cn - 1) / per - ex0 + 1 : 0;
    const size_t out_bytes = (size_t)cn * sizeof(i64), ex_bytes = (size_t)exn * sizeof(i64);
    if (int rc = grow(&sp->d_io, &sp->io_bytes, out_bytes + ex_bytes)) return rc;
    i64* d_out = (i64*)sp->d_io;
    i64* d_ex = exclude ? d_out + cn : nullptr;
    int rc = GLINT_OK;
    if (exclude && hipMemcpyAsync(d_ex, exclude + ex0, ex_bytes, hipMemcpyHostToDevice, sp->stream) != hipSuccess)
      rc = GLINT_EDEVICE;
    if (rc == GLINT_OK) rc = sampler_launch(sp, seed, first, i0, cn, d_ex, per, ex0, d_out, sp->stream);
    if (rc == GLINT_OK && hipMemcpyAsync(out + i0, d_out, out_bytes, hipMemcpyDeviceToHost, sp->stream) != hipSuccess)
      rc = GLINT_EDEVICE;
    if (hipStreamSynchronize(sp->stream) != hipSuccess && rc == GLINT_OK) rc = GLINT_EDEVICE;
    if (rc) {
      (void)hipGetLastError();
      return rc;
    }
  }
  return GLINT_OK;
}

}  // extern "C"
