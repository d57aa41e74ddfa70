// glint_rowstep_group.hip -- grouped optimizer row pushes (glint_mat_push_rows_adagrad_grouped*,
// _adagrad_rowwise_grouped*, _adam_grouped*, _ftrl_grouped*; DESIGN.md "Grouped optimizer row pushes"): the
// embedding bag's backward pass fused with the optimizer's step. The caller names n rows in g groups and
// sends one value row per group, optionally one coefficient per record; per distinct row the shard sums its
// records' contributions vals[group of i] (coef[i] * that, the product rounded before the add) to +0 in push
// order and takes the optimizer's one step -- the optimizer push of the n expanded rows, bit for bit in both
// shards, with nothing of size n x cols built, staged or read:
//   rows_front               the row push's front end unchanged, always strict (GLINT_PUSH_DETERMINISTIC):
//                            one item per distinct row, never a split run, never an atomic;
//   rows_group_ids           the grouped row push's: record i -> its group, into the weights shard's
//                            group-id scratch;
//   rows_step_group_fold     the sliced fold over the step policies of glint_steps.h: Adagrad, Adam, FTRL;
//   rows_rowwise_group_fold  the row-wise fold.
// The kernels are in glint_rowstep_group.h. A value row is read by every record of its group, so most of a
// run's loads hit L2: the g x cols operand is small and reused where dense gradient rows stream.
#include "glint_rowstep_group.h"

namespace glint {

// What the two host halves share, for n > 0 records: the sizes, the group-id scratch of `w`, the front end
// (scratch, error state and profile of `w`) and the group-id launch (uncounted, as the front end's).
static int group_step_front(glint_shard* w, const i64* rows, i64 n, const i64* grp_ptr, i64 g, const void* vals,
                            hipStream_t st, RowsFront* f, const u32** gids) {
  if (!rows || !grp_ptr || (g > 0 && !vals)) return GLINT_EINVAL;
  if (g < 0 || g >= ((i64)1 << 31)) return GLINT_EINVAL;     // 31-bit group ids
  if (n >= ((i64)1 << 32) - kSortTile) return GLINT_EINVAL;  // 32-bit record indices and sort offsets
  int rc = grow(&w->d_grp, &w->grp_bytes, (size_t)n * 4);
  if (rc) return rc;
  rc = rows_front(w, rows, n, GLINT_PUSH_DETERMINISTIC, st, f);
  if (rc) return rc;
  rows_group_ids_kernel<<<grid_for(n, kTPB, (i64)w->cus * 8), kTPB, 0, st>>>(grp_ptr, g, n, (u32*)w->d_grp);
  HIPCHK(hipGetLastError());
  *gids = (const u32*)w->d_grp;
  return GLINT_OK;
}

// Enqueues a grouped sliced optimizer row push of n records in g groups on st (no host synchronisation):
// group_step_front's launches and the one fold launch. Under both shards' locks; `s` has w's type and
// partition and Step::kParts * cols columns.
template <typename V, typename Step>
static int push_rows_step_grouped(glint_shard* w, glint_shard* s, const i64* rows, i64 n, const i64* grp_ptr, i64 g,
                                  const void* vals, const void* coef, const Step& k, hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  if (s->part.cols != Step::kParts * w->part.cols) return GLINT_EINVAL;
  RowsFront f;
  const u32* gids = nullptr;
  if (int rc = group_step_front(w, rows, n, grp_ptr, g, vals, st, &f, &gids)) return rc;
  const bool v16 = ((i64)w->part.cols * (i64)sizeof(V)) % 16 == 0 && aligned(vals, 16);
  const unsigned gf = grid_for(n * row_slices<V>(w->part.cols, v16), kTPB / 64, (i64)w->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const u32*, const V*, const V*, V*, V*, PartDesc,
               i64, Step);
  if (v16) {
    fold = coef ? rows_step_group_fold_kernel<V, true, true, Step> : rows_step_group_fold_kernel<V, true, false, Step>;
  } else {
    fold =
        coef ? rows_step_group_fold_kernel<V, false, true, Step> : rows_step_group_fold_kernel<V, false, false, Step>;
  }
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, gids, (const V*)vals,
                  (const V*)coef, (V*)w->data, (V*)s->data, w->part, (i64)s->part.pitch, k));
  return GLINT_OK;
}

template <typename V>
int push_rows_adagrad_grouped(glint_shard* w, glint_shard* h, const i64* rows, i64 n, const i64* grp_ptr, i64 g,
                              const void* vals, const void* coef, double lr, double eps, hipStream_t st) {
  return push_rows_step_grouped<V>(w, h, rows, n, grp_ptr, g, vals, coef, AdagradScalars<V>{(V)lr, (V)eps}, st);
}

template <typename V>
int push_rows_adam_grouped(glint_shard* w, glint_shard* s, const i64* rows, i64 n, const i64* grp_ptr, i64 g,
                           const void* vals, const void* coef, double lr, double beta1, double beta2, double eps,
                           i64 step, hipStream_t st) {
  if (n > 0 && step < 1) return GLINT_EINVAL;
  return push_rows_step_grouped<V>(w, s, rows, n, grp_ptr, g, vals, coef,
                                   adam_scalars<V>(lr, beta1, beta2, eps, step), st);
}

template <typename V>
int push_rows_ftrl_grouped(glint_shard* w, glint_shard* s, const i64* rows, i64 n, const i64* grp_ptr, i64 g,
                           const void* vals, const void* coef, double alpha, double beta, double l1, double l2,
                           hipStream_t st) {
  return push_rows_step_grouped<V>(w, s, rows, n, grp_ptr, g, vals, coef,
                                   FtrlScalars<V>{(V)alpha, (V)beta, (V)l1, (V)l2}, st);
}

// The row-wise fold for one (VEC16, GW, KEEP): with or without coefficients.
template <typename V, bool VEC16, bool GW, int KEEP>
static auto rowwise_group_fold(bool coef) {
  return coef ? rows_rowwise_group_fold_kernel<V, VEC16, GW, KEEP, true>
              : rows_rowwise_group_fold_kernel<V, VEC16, GW, KEEP, false>;
}

// Enqueues a grouped row-wise Adagrad row push on st (no host synchronisation): group_step_front's launches
// and the one fold launch. Under both shards' locks; `h` is a vector shard of w's type, size and partition.
template <typename V>
int push_rows_adagrad_rowwise_grouped(glint_shard* w, glint_shard* h, const i64* rows, i64 n, const i64* grp_ptr,
                                      i64 g, const void* vals, const void* coef, double lr, double eps,
                                      hipStream_t st) {
  if (n <= 0) return GLINT_OK;
  RowsFront f;
  const u32* gids = nullptr;
  if (int rc = group_step_front(w, rows, n, grp_ptr, g, vals, st, &f, &gids)) return rc;
  const bool v16 = ((i64)w->part.cols * (i64)sizeof(V)) % 16 == 0;
  const bool gw = v16 && aligned(vals, 16);
  const i64 strip = 64 * (v16 ? (i64)(16 / sizeof(V)) : 1);
  const bool keep = ((i64)w->part.cols + strip - 1) / strip <= kRowwiseKeep;
  const unsigned gf = grid_for(n, kTPB / 64, (i64)w->cus * 8);
  void (*fold)(const u32*, const u32*, const uint2*, const u32*, const u32*, const V*, const V*, V*, V*, PartDesc, V,
               V, V);
  const bool cf = coef != nullptr;
  if (keep) {
    fold = !v16 ? rowwise_group_fold<V, false, false, kRowwiseKeep>(cf)
                : (gw ? rowwise_group_fold<V, true, true, kRowwiseKeep>(cf)
                      : rowwise_group_fold<V, true, false, kRowwiseKeep>(cf));
  } else {
    fold = !v16 ? rowwise_group_fold<V, false, false, 0>(cf)
                : (gw ? rowwise_group_fold<V, true, true, 0>(cf) : rowwise_group_fold<V, true, false, 0>(cf));
  }
  // lr, eps and cols are rounded once to V here
  HIPCHK(launch_k(w, GLINT_K_PUSH_ROWS, fold, gf, kTPB, st, f.key, f.idx, f.items, f.nitems, gids, (const V*)vals,
                  (const V*)coef, (V*)w->data, (V*)h->data, w->part, (V)lr, (V)eps, (V)w->part.cols));
  return GLINT_OK;
}

#define GLINT_GROUP_STEP(V)                                                                                           \
  template int push_rows_adagrad_grouped<V>(glint_shard*, glint_shard*, const i64*, i64, const i64*, i64, const void*, \
                                            const void*, double, double, hipStream_t);                                \
  template int push_rows_adagrad_rowwise_grouped<V>(glint_shard*, glint_shard*, const i64*, i64, const i64*, i64,     \
                                                    const void*, const void*, double, double, hipStream_t);           \
  template int push_rows_adam_grouped<V>(glint_shard*, glint_shard*, const i64*, i64, const i64*, i64, const void*,   \
                                         const void*, double, double, double, double, i64, hipStream_t);              \
  template int push_rows_ftrl_grouped<V>(glint_shard*, glint_shard*, const i64*, i64, const i64*, i64, const void*,   \
                                         const void*, double, double, double, double, hipStream_t);
GLINT_GROUP_STEP(float)
GLINT_GROUP_STEP(double)
#undef GLINT_GROUP_STEP

}  // namespace glint
