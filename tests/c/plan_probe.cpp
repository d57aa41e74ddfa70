// plan_probe.cpp -- the push planners (glint_push_plan.h, glint_bin_plan.h) behind a C interface of
// plain integer arrays, for tests/test_plan_cpu.py (ctypes). No GPU, no HIP.
//
// Built a second time with -DPLAN_PROBE_MAIN as a program that sweeps the test's layout grid and a few
// routes and front-end histories: the form to run under -fsanitize=address,undefined.
#include "../../glint_amd/csrc/glint_push_plan.h"
#include "../../glint_amd/csrc/glint_bin_plan.h"
#include "../../include/glint_gpu.h"

using namespace glint;

extern "C" {

// in: n, flags, fp, vec_ok, gated, ring, elems, binnable, hint_tail, hint_head, whole_probe, binned_mode,
//     bin_density, whole_on
// out: kind, tail, validate, fuse, gate_kernel, scatter_mode, probe_consumed
void plan_route(const int64_t* in, int32_t* out) {
  PushQuery q;
  q.n = in[0];
  q.flags = (int)in[1];
  q.fp = in[2] != 0;
  q.vec_ok = in[3] != 0;
  q.gated = in[4] != 0;
  q.ring = in[5] != 0;
  q.elems = in[6];
  q.binnable = in[7] != 0;
  q.hint_tail = (u64)in[8];
  q.hint_head = (u64)in[9];
  q.whole_probe = (u32)in[10];
  q.binned_mode = (int)in[11];
  q.bin_density = in[12];
  q.whole_on = in[13] != 0;
  const PushRoute r = push_route(q);
  out[0] = (int32_t)r.kind;
  out[1] = (int32_t)r.tail;
  out[2] = r.validate;
  out[3] = r.fuse;
  out[4] = r.gate_kernel;
  out[5] = r.scatter_mode;
  out[6] = r.probe_consumed;
}

// A fresh shard's front-end history taken through `steps` binned pushes.
// in, per push: hint m, hint tail, hint cold, hint_bin_front, forced
// out, per push: front, hot_refresh, pushes, last_front, hot_age
void plan_front(const int64_t* in, int32_t steps, int32_t* out) {
  BinFrontState f;
  for (int32_t i = 0; i < steps; ++i, in += 5, out += 5) {
    const u64 hint_bin = ((u64)(u32)in[0] << 32) | (u32)in[1];
    const BinFront r = bin_front_next(f, hint_bin, (u64)in[2], (int)in[3], (int)in[4]);
    out[0] = r.front;
    out[1] = r.hot_refresh;
    out[2] = (int32_t)f.pushes;
    out[3] = f.last_front;
    out[4] = (int32_t)f.hot_age;
  }
}

// in: elems, n, cus, front, acc_bytes, hot_occ
// out: small_push, per, kchunk, nchunks_max, wpc, G, item, max_fitems, max_units, nstride, ctstride,
//      g.fb, g.nb, g.nf, g.nslab, then the 16 offsets in buffer order, then need
enum { kPlanLayoutWords = 32 };
void plan_layout(const int64_t* in, int64_t* out) {
  const BinLayout L = bin_layout(in[0], in[1], (int)in[2], (int)in[3], (size_t)in[4], (int)in[5]);
  const int64_t v[kPlanLayoutWords] = {
      L.small_push, L.per, L.kchunk, L.nchunks_max, L.wpc, L.G, L.item, L.max_fitems, L.max_units, L.nstride,
      L.ctstride, L.g.fb, L.g.nb, L.g.nf, L.g.nslab,
      (int64_t)L.ct, (int64_t)L.P, (int64_t)L.Q, (int64_t)L.Bb, (int64_t)L.Ib, (int64_t)L.fitems, (int64_t)L.cwin,
      (int64_t)L.off2, (int64_t)L.units, (int64_t)L.runs, (int64_t)L.hot_tags, (int64_t)L.wpart, (int64_t)L.addr_a,
      (int64_t)L.val_a, (int64_t)L.val_b, (int64_t)L.e_b, (int64_t)L.need};
  for (int i = 0; i < kPlanLayoutWords; ++i) out[i] = v[i];
}

}  // extern "C"

#ifdef PLAN_PROBE_MAIN
#include <stdio.h>

int main() {
  const int64_t elems[] = {1, 4096, 4097, 1ll << 20, 1ll << 28, (1ll << 32) - 2};
  const int64_t ns[] = {1, 4095, 4096, 1ll << 20, 1ll << 26};
  const int64_t cus[] = {1, 256};
  int64_t sum = 0;
  long cases = 0;
  for (int64_t e : elems)
    for (int64_t n : ns)
      for (int64_t c : cus)
        for (int64_t front = 0; front < 3; ++front)
          for (int64_t acc = 4; acc <= 8; acc += 4) {
            const int64_t in[6] = {e, n, c, front, acc, 1};
            int64_t out[kPlanLayoutWords];
            plan_layout(in, out);
            for (int i = 15; i + 1 < kPlanLayoutWords; ++i)
              if (out[i] % 256 || out[i + 1] < out[i]) {
                fprintf(stderr, "layout: offset %d of elems %lld n %lld\n", i, (long long)e, (long long)n);
                return 1;
              }
            sum += out[kPlanLayoutWords - 1];
            ++cases;
          }
  // every route input at its extremes (the decision compares 64-bit hint words with record counts)
  const int64_t big[] = {0, 1, 4096, 4097, 1ll << 20, 1ll << 32, INT64_MAX};
  for (int64_t n : big)
    for (int64_t tail : big)
      for (int flags = 0; flags < 8; ++flags)
        for (int bits = 0; bits < 16; ++bits) {
          const int64_t in[14] = {n, flags | ((bits & 8) ? kPushHostSequential : 0), bits & 1, (bits >> 1) & 1,
                                  (bits >> 2) & 1, 0, 1ll << 22, 1, tail, 0, 7, -1, 512, 1};
          int32_t out[7];
          plan_route(in, out);
          sum += out[0];
          ++cases;
        }
  int64_t steps[40 * 5];
  int32_t fout[40 * 5];
  for (int i = 0; i < 40; ++i) {
    const int64_t st[5] = {0xFFFFFFFFll, i % 3 ? 0xFFFFFFFFll : 0, i % 5 ? 0xFFFFFFFFll : 0, 2, i % 7 ? -1 : 1};
    for (int j = 0; j < 5; ++j) steps[i * 5 + j] = st[j];
  }
  plan_front(steps, 40, fout);
  sum += fout[40 * 5 - 3];
  printf("plan_probe: %ld cases, checksum %lld\n", cases + 40, (long long)sum);
  return 0;
}
#endif
