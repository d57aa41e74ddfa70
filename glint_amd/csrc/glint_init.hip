// glint_init.hip -- shard fill and seeded uniform init (glint_shard_fill*, glint_shard_init_uniform*,
// DESIGN.md "Shard fill and uniform init"): every element of the named rows receives a constant, or a
// value that is a function of (seed, global row, column, lo, hi, type) only -- glint_init_plan.h states
// that function, and this file only decides who stores what.
//   shard_init   a persistent grid over (row, 16-B block) work items, flattened so that short rows do not
//                idle lanes. A matrix row starts 16-B aligned and block b is bytes [16 b, 16 b + 16) of
//                it, so every full block is one aligned 16-B store whatever cols is; only a last partial
//                block is written element by element, so the pitch padding is never touched. One Philox
//                block is 128 bits: one store for either type.
// No load of the shard, no atomics but the error record of a row outside the partition; a row named twice
// is written twice with the same bits. A vector shard is the cols = 1 case: one Philox block per element
// and 4- or 8-B stores (a known limit).
#include "glint_device.h"
#include "glint_host.h"
#include "glint_init_plan.h"

// a build-time experiment knob: 1 = the 16-B stores are non-temporal (measured: DESIGN.md)
#ifndef GLINT_INIT_NT
#define GLINT_INIT_NT 0
#endif

namespace glint {

typedef __attribute__((ext_vector_type(4))) unsigned int InitU4;

template <int VS> struct InitElem;
template <> struct InitElem<4> { typedef float F; typedef u32 B; };
template <> struct InitElem<8> { typedef double F; typedef u64 B; };

struct InitArgs {
  u64 seed;   // uniform: the Philox key
  u64 a, b;   // uniform: the bits of lo and w in the shard's type; fill: a = the value's bits
  u32 nb;     // 16-B blocks per row: ceil(cols / L), 1 for a vector
  u32 cols;   // elements per row: 1 for a vector
  u32 step_r, step_b;  // the grid's stride (threads) as rows and blocks: stride = step_r * nb + step_b
  u64 total;  // work items: (rows named) * nb
};

// VS: bytes of an element. UNIFORM: values from the generator, else the constant. LIST: rows[] names the
// rows (global keys, translated with g2l; one outside the partition is skipped and recorded once, by the
// item of its block 0), else item row r is local row r.
template <int VS, bool UNIFORM, bool LIST>
__global__ __launch_bounds__(kTPB) void shard_init_kernel(const i64* __restrict__ rows, char* __restrict__ data,
                                                          PartDesc part, InitArgs a, ErrState* err) {
  typedef typename InitElem<VS>::F F;
  typedef typename InitElem<VS>::B B;
  constexpr u32 L = 16 / VS;
  const u32 t = blockIdx.x * kTPB + threadIdx.x;
  // (row, block) of this thread's first item by one 32-bit division, then advanced by the stride
  u64 r = t / a.nb;
  u32 b = t % a.nb;
  const u64 nrows = a.total / a.nb;
  const u64 row_bytes = (u64)part.pitch * VS;
  F lo, w;
  B fill;
  if (UNIFORM) {
    const B lb = (B)a.a, wb = (B)a.b;
    __builtin_memcpy(&lo, &lb, VS);
    __builtin_memcpy(&w, &wb, VS);
  } else {
    fill = (B)a.a;
  }
  for (; r < nrows; r += a.step_r, b += a.step_b) {
    if (b >= a.nb) {  // (step_b < nb: one carry at most)
      b -= a.nb;
      if (++r >= nrows) break;
    }
    i64 l = (i64)r;
    if (LIST) {
      l = g2l(part, rows[r]);
      if (l < 0 || l >= part.size) {
        if (b == 0) record_error(err, (i64)r);
        continue;
      }
    }
    B v[L];
    if (UNIFORM) {
      // the element's global row, from the layout: the value never depends on how the row was named
      const u64 g = part.kind == 0 ? (u64)(part.start + l) : (u64)((i64)part.cidx + l * (i64)part.cparts);
      const PhiloxOut p = init_block<F>(a.seed, g, b);
#pragma unroll
      for (u32 j = 0; j < L; ++j) {
        const F x = init_value(p, (int)j, lo, w);
        __builtin_memcpy(&v[j], &x, VS);
      }
    } else {
#pragma unroll
      for (u32 j = 0; j < L; ++j) v[j] = fill;
    }
    char* at = data + (u64)l * row_bytes + (u64)b * 16;
    const u32 c0 = b * L;
    if (c0 + L <= a.cols) {  // a full block: one aligned 16-B store (never true for a vector)
      InitU4 q;
      __builtin_memcpy(&q, v, 16);
#if GLINT_INIT_NT
      __builtin_nontemporal_store(q, reinterpret_cast<InitU4*>(at));
#else
      *reinterpret_cast<InitU4*>(at) = q;
#endif
    } else {  // the last, partial block of a row: its elements only, the padding keeps its bits
#pragma unroll
      for (u32 j = 0; j < L; ++j)
        if (c0 + j < a.cols) reinterpret_cast<B*>(at)[j] = v[j];
    }
  }
}

// ---- host side ----------------------------------------------------------------------------------
// Enqueues the fill (uniform false: every element = the low vsize bytes of a) or the uniform init (lo and
// w as bits of the shard's type in a and b) on st: one launch under GLINT_K_PUSH_ROWS, none when nothing
// is named. list false: every row of the partition (rows unused); else rows[0 .. n) (device pointer). No
// host synchronisation; under the shard's lock.
int shard_init(glint_shard* s, const i64* rows, i64 n, bool list, bool uniform, u64 seed, u64 a, u64 b,
               hipStream_t st) {
  const bool vec = s->part.cols == 0;
  const u32 per = (u32)(16 / s->vsize);
  InitArgs ia{};
  ia.seed = seed;
  ia.a = a;
  ia.b = b;
  ia.cols = vec ? 1u : (u32)s->part.cols;
  ia.nb = (ia.cols + per - 1) / per;
  const u64 nrows = list ? (u64)n : (u64)s->part.size;
  ia.total = nrows * ia.nb;
  if (ia.total == 0) return GLINT_OK;
  const unsigned grid = grid_for((i64)ia.total, kTPB, (i64)s->cus * 8);
  const u32 stride = grid * (u32)kTPB;
  ia.step_r = stride / ia.nb;
  ia.step_b = stride % ia.nb;
  void (*k)(const i64*, char*, PartDesc, InitArgs, ErrState*);
  if (s->vsize == 4) {
    k = uniform ? (list ? shard_init_kernel<4, true, true> : shard_init_kernel<4, true, false>)
                : (list ? shard_init_kernel<4, false, true> : shard_init_kernel<4, false, false>);
  } else {
    k = uniform ? (list ? shard_init_kernel<8, true, true> : shard_init_kernel<8, true, false>)
                : (list ? shard_init_kernel<8, false, true> : shard_init_kernel<8, false, false>);
  }
  HIPCHK(launch_k(s, GLINT_K_PUSH_ROWS, k, grid, kTPB, st, rows, (char*)s->data, s->part, ia, err_of(s)));
  return GLINT_OK;
}

}  // namespace glint
