/*
 * glint_gpu.h -- C ABI of the MI355X push/pull reduction plane for Glint's parameter server.
 *
 * A "shard" is the device-resident replacement of one Glint partial model: the JVM array
 * `data` of PartialVector[V] (src/main/scala/glint/models/server/PartialVector.scala:27) or
 * PartialMatrix[V] (src/main/scala/glint/models/server/PartialMatrix.scala:28), now held in HBM
 * of one MI355X. The entry points below are exactly the methods of those classes that the
 * server actors call (PartialVectorDouble.scala:17-23, PartialMatrixDouble.scala:21-28), plus
 * shard lifetime, device-resident variants for stream-ordered callers, and a raw wire-format
 * ingest of the reference's RequestSerializer payloads.
 *
 * Plain C: pointers, sizes and status codes only. Thread-safety: calls on DIFFERENT shards may
 * run concurrently from any threads; calls on ONE shard are serialized internally (the Akka
 * actor already serializes them, PartialVector.scala:16-17). Every host-pointer call is
 * synchronous: when it returns, its effect is visible to the next call on the same shard.
 */
#ifndef GLINT_GPU_H
#define GLINT_GPU_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Value types of the typed partial models (PartialVector{Int,Long,Float,Double}.scala,
 * PartialMatrix{Int,Long,Float,Double}.scala). */
enum glint_dtype { GLINT_I32 = 0, GLINT_I64 = 1, GLINT_F32 = 2, GLINT_F64 = 3 };

/* Status codes. GLINT_EOUTOFRANGE is where the reference throws
 * ArrayIndexOutOfBoundsException inside update/get (a key whose local index falls outside the
 * partition array); the JNI shim raises that exception type so Akka supervision behaves as in
 * the reference (restart => the actor re-creates a zeroed shard). */
enum glint_status {
  GLINT_OK = 0,
  GLINT_EOUTOFRANGE = 1, /* a key/row/col outside the shard; see glint_shard_last_error */
  GLINT_EDEVICE = 2,     /* HIP runtime error */
  GLINT_EINVAL = 3,      /* bad argument (null handle, wrong dtype, malformed payload ...) */
  GLINT_ENOMEM = 4       /* device or pinned-host allocation failed */
};

/* Push flags. */
enum glint_push_flags {
  GLINT_PUSH_DEFAULT = 0,
  /* Bit-exact reproduction of the reference's strictly sequential `data(k) += v` order for
   * Float/Double even when keys repeat (PartialVector.scala:37-41). Without it, repeated keys in
   * a device-resident push are summed in arbitrary order (<= 1e-6 relative for Double; Int and
   * Long are exact either way). Unique-key pushes are bit-exact in both modes.
   * Host-pointer and wire pushes (glint_vec_push, glint_mat_push, glint_push_wire: what the actor's
   * update() calls) of up to 131 072 records -- above the 79 999-record frame cap, glint.conf:143 --
   * keep the message's order WITHOUT this flag too (one launch, glint_ordered.hip), unless
   * GLINT_PUSH_UNORDERED is given.
   * IEEE edge values: in every mode subnormals are kept (no input or partial sum is flushed) and
   * infinities and NaN propagate as classes, with the NaN's payload unspecified; the ordered paths add
   * in the shard's type and keep the sign of a zero as the sequential loop does, the unordered ones
   * leave it unspecified. */
  GLINT_PUSH_DETERMINISTIC = 1,
  /* Hint: the keys are in no particular order and the caller does not need the reference's
   * summation order. A large push skips the order check and sums the records per shard slab in
   * LDS (partition by slab + one read-modify-write per touched element pair) instead of per-record
   * device atomics; a host-pointer push takes the unordered LDS-hash scatter instead of the
   * order-preserving fold. Without the hint, a large push takes the binned path by itself when the
   * shard's previous push was unordered (environment GLINT_BINNED=0 disables that, =1 forces it
   * for pushes >= 2^20 records). The adaptive choices (binned or not, and the binned front end)
   * follow what earlier pushes measured on the device as of the shard's last sync point
   * (glint_shard_sync, or the end of a host-pointer call): a device-resident caller that never
   * syncs gets the no-history defaults. */
  GLINT_PUSH_UNORDERED = 2,
  /* glint_*_push_dev_gated only: the gate word is the push's OUTPUT. The push checks every record
   * itself before applying any (its order check reads all keys), writes 0 or ~(index of the first
   * out-of-range record) to *gate, and applies nothing when there is one -- the route's validation
   * pass in front of a one-partition push, folded into the push. */
  GLINT_PUSH_VALIDATE = 4
};

typedef struct glint_shard* glint_shard_t;

/* ---- lifetime ------------------------------------------------------------------------------ */

/* Range-partitioned shard = `new PartialVector*(RangePartition(index, start, end))`
 * (RangePartition.scala:8; PartialVectorDouble.scala:15 allocates Array[Double](size), zeroed).
 * cols == 0 creates a vector shard of size (int)(end - start) elements (RangePartition.scala:24);
 * cols > 0 creates a matrix shard of (int)(end - start) rows x cols (PartialMatrixDouble.scala:19).
 * Replaces `Props(classOf[PartialVectorDouble], partition)` (src/main/scala/glint/Client.scala:178)
 * and `Props(classOf[PartialMatrixDouble], partition, cols)` (Client.scala:130). */
int glint_shard_create(int device, int dtype, int64_t start, int64_t end, int32_t cols,
                       glint_shard_t* out);

/* Cyclic-partitioned shard (CyclicPartition(index, numberOfPartitions, numberOfKeys),
 * src/main/scala/glint/partitioning/cyclic/CyclicPartition.scala:12). */
int glint_shard_create_cyclic(int device, int dtype, int32_t index, int32_t num_partitions,
                              int64_t num_keys, int32_t cols, glint_shard_t* out);

/* One device-resident push into several range vector shards of one device and type at once (up to
 * 64, disjoint ranges, any order): each record goes to the shard whose range holds its key -- the
 * partitions one server hosts, applied by one launch sequence where the reference sends a message per
 * partition (AsyncBigVector.scala:96-98) and each partition's actor applies its own
 * (PartialVector.scala:35-43). The batch is checked first: a key in no shard's range applies NOTHING
 * (mapPartitions throws before sending, AsyncBigVector.scala:96-98) and *gate receives ~(first such
 * record), else 0 -- gate is a device word or a glint_host_alloc word the caller reads after waiting on
 * `stream`. Unordered sums (as GLINT_PUSH_UNORDERED; exact for Int/Long). Every shard's lock is held
 * for the call; each is ordered after its host-pointer work and marked for the next sync like any
 * device-resident call (glint_shards_sync / glint_shard_sync on `stream`). A slab with views is not
 * a member (GLINT_EINVAL): push to its views, or to the slab alone. */
int glint_vec_push_dev_shards(glint_shard_t* shards, int n_shards, const int64_t* keys, const void* vals,
                              int64_t n, uint64_t* gate, void* stream);

/* Slabs: the partitions one server hosts, kept in one allocation. A range shard (vector, or matrix
 * rows of the slab's width) over RangePartition(start, end) whose elements are the slab's rows
 * [offset, offset + end - start) -- a view: it reads and writes them as they are, and is a shard like
 * any other (its own partition, key check, stream, error state). The slab keeps its own partition, so
 * a batch whose records all fall in the views can be pushed or pulled as ONE device-resident call on
 * the slab when the views' partitions lie side by side in key order (the Client's partitions of one
 * rank at world size 1: DistributedClient's slab) -- one launch sequence for all of them, where the
 * reference sends one message per partition (AsyncBigVector.scala:96-98, one actor per partition,
 * Client.scala:71-85). The view's first element must be 256-byte aligned in the slab. While it has
 * views the slab takes device-resident calls only (its host-pointer calls, and glint_shard_zero,
 * return GLINT_EINVAL), each ordered after the views' host-pointer work and before their later
 * host-pointer calls; device-resident calls on the slab and its views are ordered by their streams,
 * as for any shard. A view is destroyed before its slab (GLINT_EINVAL until then). */
int glint_shard_create_in(glint_shard_t slab, int64_t offset, int64_t start, int64_t end,
                          glint_shard_t* out);

/* Frees the device memory (actor postStop / `destroy()`, AsyncBigVector.scala:135-140). */
int glint_shard_destroy(glint_shard_t shard);

/* Zeroes the shard: what an Akka restart of the partial-model actor produces. */
int glint_shard_zero(glint_shard_t shard);

/* Shard fill and uniform init (extensions: the reference constructs zeroed models only): what an
 * embedding table starts from, written on the device, so that nothing of size rows x cols crosses the
 * link. glint_shard_fill gives every named element one constant (an Adagrad accumulator's initial
 * value); glint_shard_init_uniform gives it a value drawn from a seeded counter-based generator.
 *   rows   NULL with n == 0: every row (vector: every element) of the partition. Else n global keys in
 *          any order, repeats allowed (a row named twice is written twice with the same bits); a non-NULL
 *          rows with n == 0 names nothing.
 * Element (g, c): g is the global key (vector) or global row (matrix) of the element, c its column (0 for
 * a vector). Local row l has g = start + l in a range partition and g = index + l * numberOfPartitions in
 * a cyclic one; the value is that of the row the element IS, however the key that named it was mapped.
 * Fill: the element receives the sizeof V bytes at `value` as they are: a -0.0 and a NaN's payload and
 * sign are stored unchanged. All four types.
 * Uniform (Float and Double shards only): with L = 4 values per block for Float and 2 for Double, block
 * b = c / L and position j = c % L,
 *   (o0, o1, o2, o3) = Philox4x32-10(counter (lo32(g), hi32(g), b, 0), key (lo32(seed), hi32(seed)))
 * with the standard multipliers 0xD2511F53, 0xCD9E8D57 and Weyl constants 0x9E3779B9, 0xBB67AE85;
 *   Float:  u = (o[j] >> 8) * 2^-24
 *   Double: u = ((o[2j] | (uint64)o[2j+1] << 32) >> 11) * 2^-53
 * (both conversions exact). lo and hi are rounded once, on the host, to V; w = hi - lo is computed once,
 * on the host, in V; the element is lo + (u * w) in V, the product rounded before the add (no fused
 * multiply-add). It lies in [lo, hi]: u < 1, but rounding may give hi itself. The value is a function of
 * (seed, g, c, lo, hi, dtype) only -- not of the partitioner, the number of partitions, the device, the
 * grid or whether the row was named by a list -- so a model initialised under any layout holds the same
 * bits, and initialising a row again is idempotent. A vector is the cols = 1 case: one block per element.
 * Neither call reads or writes a row that is not named, nor the pitch padding of any row.
 * Host calls: the shard is entered as by glint_shard_zero and the other host-pointer calls: the open ring
 * batch is flushed, the call is ordered after the messages enqueued before it and after the last
 * device-resident call, and a slab with views is refused. Every row is checked first: for the lowest i
 * with rows[i] outside the partition the call returns GLINT_EOUTOFRANGE (i in glint_shard_last_error)
 * with nothing written. Then rows is staged, one kernel runs on the shard's stream and the call ends
 * synchronised. They are ordinary writes, not a restart: the error state and the failed tickets are left
 * as they are.
 * GLINT_EINVAL: a NULL shard; a NULL value; rows == NULL with n != 0; n < 0; n >= 2^31; a uniform init of
 * an Int or Long shard; lo or hi NaN or infinite after rounding to V; lo > hi; a w that is not finite.
 * lo == hi is allowed (every element is lo). Kernel timing: the one launch counts under
 * GLINT_K_PUSH_ROWS; a call that names nothing launches nothing. */
int glint_shard_fill(glint_shard_t shard, const int64_t* rows, int64_t n, const void* value);
int glint_shard_init_uniform(glint_shard_t shard, const int64_t* rows, int64_t n, uint64_t seed, double lo,
                             double hi);

/* Shape: size = Partition.size (elements for a vector, rows for a matrix), cols (0 = vector),
 * dtype, device. Any out-pointer may be NULL. */
int glint_shard_info(glint_shard_t shard, int32_t* size, int32_t* cols, int* dtype, int* device);

/* ---- host-pointer hot path (what the JNI shim calls) ---------------------------------------- */

/* PartialVector.update(keys, values) -- PartialVector.scala:35-43. vals: n elements of dtype. */
int glint_vec_push(glint_shard_t shard, const int64_t* keys, const void* vals, int64_t n, int flags);

/* PartialVector.get(keys) -- PartialVector.scala:51-60. out: n elements of dtype. Every pull entry
 * point (host, device, ring and wire forms) moves the stored bits unchanged: -0.0, a NaN's payload
 * and sign, subnormals. */
int glint_vec_pull(glint_shard_t shard, const int64_t* keys, void* out, int64_t n);

/* PartialMatrix.update(rows, cols, values) -- PartialMatrix.scala:74-83. */
int glint_mat_push(glint_shard_t shard, const int64_t* rows, const int32_t* cols, const void* vals,
                   int64_t n, int flags);

/* PartialMatrix.get(rows, cols) -- PartialMatrix.scala:55-65. */
int glint_mat_pull(glint_shard_t shard, const int64_t* rows, const int32_t* cols, void* out, int64_t n);

/* PartialMatrix.getRows(rows) -- PartialMatrix.scala:37-46, written flattened row-major
 * (n x cols) the way ResponseSerializer sends ResponseRows* (ResponseSerializer.scala:52-61). */
int glint_mat_pull_rows(glint_shard_t shard, const int64_t* rows, void* out, int64_t n);

/* The write counterpart of glint_mat_pull_rows (an extension: the reference has no row-push
 * message). PartialMatrix.update (PartialMatrix.scala:74-83) over whole rows: for i in order, for c in
 * [0, cols): data[l(rows[i])][c] += vals[i*cols + c].
 * vals: n x cols values of the shard's type, dense row-major (NO pitch).
 * Matrix shards only; n < 2^32 - 2048; GLINT_PUSH_VALIDATE or an unknown flag is GLINT_EINVAL. Every
 * row is checked before anything is applied: on a row outside the partition nothing is applied
 * (GLINT_EOUTOFRANGE, the record's index in glint_shard_last_error). Float/Double sums of repeated rows
 * keep the push order, bit for bit the sequential loop, unless GLINT_PUSH_UNORDERED is given. */
int glint_mat_push_rows(glint_shard_t shard, const int64_t* rows, const void* vals, int64_t n, int flags);

/* Sparse row pull (an extension: the reference declares ResponseSparseDouble(indices, values) but wires
 * it into no request): the non-zero elements of the requested rows as a CSR triple, compacted on the
 * device so that only they cross the link.
 *   row_ptr   n + 1 int64: row_ptr[0] = 0, row_ptr[i+1] - row_ptr[i] = the number of elements of
 *             requested row i with v != 0 (the type's own test: -0.0 is dropped, NaN is kept);
 *   out_cols  int32 column of entry j of request i at position row_ptr[i] + j, ascending inside a row;
 *   out_vals  its value, the stored bits unchanged (the shard's type).
 * Requests are answered in the caller's order; a row requested twice appears twice. Scattering the
 * triple into zeros gives what glint_mat_pull_rows returns (a dropped -0.0 comes back as +0.0). The
 * answer is deterministic (no atomic decides a position).
 * Capacity as with snprintf: row_ptr is always written in full, so row_ptr[n] is the capacity the
 * answer needs; an entry is stored only if its position is < cap, and nothing at or beyond cap is
 * touched. cap == 0 is a count-only call, and only then may out_cols and out_vals be NULL. *nnz (may
 * be NULL) receives row_ptr[n]. With n == 0, row_ptr[0] = 0 is still written.
 * GLINT_EINVAL: a NULL or vector shard, n < 0, n >= 2^31, cap < 0, a NULL row_ptr, NULL rows with
 * n > 0, NULL out_cols / out_vals with cap > 0. Every row is checked first: a row outside the
 * partition returns GLINT_EOUTOFRANGE (its index in glint_shard_last_error) with nothing written.
 * Device staging and the bytes copied back are (n + 1) * 8 + min(nnz, cap) * (4 + value size) --
 * never cap or n * cols values: the call counts and scans, reads the total, then emits into buffers of
 * that size. */
int glint_mat_pull_rows_sparse(glint_shard_t shard, const int64_t* rows, int64_t n, int64_t* row_ptr,
                               int32_t* out_cols, void* out_vals, int64_t cap, int64_t* nnz);
/* Counts one scan workgroup covers in the sparse pull's prefix sum over the n + 1 row counts: a pull of
 * more requests scans in two levels, of more than its square in three (tests size their cases by it). */
#define GLINT_SPARSE_SCAN_TILE 1024

/* Grouped row-sum pull (an extension: later forks of the reference grew pullSum / pullAverage over row
 * groups; this version has none): the sums of groups of requested rows, reduced next to the data so that
 * g x cols values answer a request that names n rows.
 *   grp_ptr   g + 1 int64, non-decreasing, grp_ptr[0] = 0 and grp_ptr[g] = n: group k is
 *             rows[grp_ptr[k] .. grp_ptr[k+1]);
 *   out       g x cols values of the shard's type, dense row-major (NO pitch).
 * out[k][c] is the left-to-right sum of element c of the group's rows, in the shard's type and in the
 * caller's order: ((r0 + r1) + r2) + ... The first row's stored bits are the first term, not 0 + r0, so a
 * group of one row is glint_mat_pull_rows bit for bit (-0.0, a NaN's payload and sign and subnormals come
 * back unchanged); an empty group is all +0 / 0; Int and Long wrap. A row may occur several times in a
 * group, and in several groups. The answer is deterministic: no atomics, and no group is split. There
 * are no flags: the order is strict in every mode.
 * GLINT_EINVAL: a NULL or vector shard, n < 0, g < 0, n >= 2^31, g >= 2^31, a NULL grp_ptr, NULL rows
 * with n > 0, NULL out with g > 0 and -- in this host call only, before anything is staged -- a grp_ptr
 * that breaks the rule above. g == 0 writes nothing and returns GLINT_OK. Every row is checked first: a
 * row outside the partition returns GLINT_EOUTOFRANGE (its index in `rows` in glint_shard_last_error) with
 * nothing written to out. Staged to the device: rows and grp_ptr; copied back: g * cols values -- never
 * n * cols. */
int glint_mat_pull_rows_sum(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                            int64_t g, void* out);

/* Row dot-product pull (an extension: the reference has no such message): the requested rows times
 * vectors the caller sends, reduced over the columns next to the data, so that n x q values answer a
 * request that names n rows -- scores of candidate rows against query vectors, or row norms.
 *   x     q x cols values of the shard's type, dense row-major; NULL only with q == 1: the self-dot,
 *         out[i] = sum over c of row[c] * row[c], the squared norm;
 *   out   n x q values of the shard's type, dense: out[i*q + j] = dot(row rows[i], x[j]).
 * Requests keep the caller's order; a row requested twice is answered twice. x must not overlap out.
 * There are no flags and no atomics: the answer is deterministic.
 * Arithmetic, all in the shard's type. Int/Long: products and sums wrap (low 32 / 64 bits), so every
 * order gives the same bits. Float/Double: the order is part of the contract, and it is a function of
 * (type, cols) only -- never of pointer alignment, q, how the queries are spread over waves, or the
 * grid. Let E = 16 / sizeof(V) when cols * sizeof(V) is a multiple of 16, else E = 1. Column c belongs to
 * lane L = (c / E) % 64. Each of the 64 lanes starts from +0 and adds its columns' products in ascending
 * c, acc = acc + (row[c] * x[c]), the product rounded before the add (no fused multiply-add). The 64
 * lane sums are then combined by the xor butterfly: for d in 32, 16, 8, 4, 2, 1: acc[L] = acc[L] +
 * acc[L ^ d] (IEEE addition commutes, so every lane ends with the same value: the answer). Subnormal
 * products and sums are kept; infinities and NaN follow IEEE (inf * 0 is NaN; a NaN's payload and sign
 * are unspecified); a zero result's sign is what that order gives.
 * Only `cols` elements of a row are read, never the pitch padding.
 * GLINT_EINVAL: a NULL or vector shard, n < 0, n >= 2^31, q < 1, q > GLINT_DOT_MAX_QUERIES, a NULL x with
 * q != 1, NULL rows or NULL out with n > 0. n == 0 writes nothing and returns GLINT_OK. Every row is
 * checked first: a row outside the partition returns GLINT_EOUTOFRANGE (its index in
 * glint_shard_last_error) with nothing staged and nothing written to out. Staged to the device: rows and
 * x; copied back: n * q values -- never n * cols. */
#define GLINT_DOT_MAX_QUERIES 1024
/* Queries one wave answers for its row when q > 1 (tests size their cases by it; the bits do not
 * depend on it). */
#define GLINT_DOT_QUERY_TILE 4
int glint_mat_pull_rows_dot(glint_shard_t shard, const int64_t* rows, int64_t n, const void* x, int64_t q,
                            void* out);

/* Row axpy push (an extension: the reference has no such message): the write half of a scoring step,
 * whole rows += coefficients times vectors the caller sends, so that n*q + q*cols values cross the link
 * instead of the n x cols outer product glint_mat_push_rows would need.
 *   coef  n x q values of the shard's type, dense row-major;
 *   x     q x cols values of the shard's type, dense row-major; 1 <= q <= GLINT_AXPY_MAX_VECTORS.
 * For i in push order, for c in [0, cols): data[l(rows[i])][c] = data[l(rows[i])][c] + t_i[c], where
 *   t_i[c] = ((coef[i][0] * x[0][c]) + (coef[i][1] * x[1][c])) + ... + (coef[i][q-1] * x[q-1][c]):
 * j ascends, the first product is the first term (not 0 + product), every product is rounded before it is
 * added (no fused multiply-add, neither inside t_i nor between t_i and the element), and all arithmetic is
 * in the shard's type; Int/Long wrap. The call is therefore glint_mat_push_rows with vals[i] = t_i,
 * rounding for rounding. That order is a function of the inputs only -- never of pointer alignment, q, how
 * the vectors are tiled over registers, or the grid. Subnormal products and sums are kept; infinities and
 * NaN follow IEEE (inf * 0 is NaN; a NaN's payload and sign are unspecified). Only `cols` elements of a
 * row are read and written, never the pitch padding.
 * Flags and errors are glint_mat_push_rows's: only GLINT_PUSH_DETERMINISTIC and GLINT_PUSH_UNORDERED are
 * accepted; Float/Double sums of repeated rows keep the push order unless GLINT_PUSH_UNORDERED is given;
 * every row is checked before anything is applied: on a row outside the partition nothing is applied
 * (GLINT_EOUTOFRANGE, the record's index in glint_shard_last_error).
 * GLINT_EINVAL: a NULL or vector shard, n < 0, n >= 2^32 - 2048, q < 1, q > GLINT_AXPY_MAX_VECTORS, any
 * other flag, NULL rows, coef or x with n > 0. n == 0 launches nothing and returns GLINT_OK. Staged to the
 * device: rows, coef and x in one block; nothing is copied back, and nothing of size n x cols exists. */
#define GLINT_AXPY_MAX_VECTORS 64
int glint_mat_push_rows_axpy(glint_shard_t shard, const int64_t* rows, int64_t n, const void* coef, const void* x,
                             int64_t q, int flags);

/* Adagrad row push (an extension: the reference has no such message): a stateful optimizer step next to
 * the rows. `weights` and `state` are two Float or Double matrix shards of one type, device, partition
 * and cols; `state` holds the accumulated squared gradients. One push crosses the link with n x cols
 * gradients and nothing else, and steps both shards with one read-modify-write per touched row.
 *   grads  n x cols values of the shards' type V, dense row-major, no pitch (glint_mat_push_rows's vals).
 * lr and eps are rounded once on the host to V: lr_V, eps_V. For every distinct local row l the push names:
 *   1. G[c] = (((+0 + g_i0[c]) + g_i1[c]) + ...) over the records i0 < i1 < ... with l(rows[i]) == l: the
 *      sum runs in push order, in V, from +0.
 *   2. Per column, with h = state[l][c] and w = weights[l][c], every operation in V and rounded on its own
 *      (no fused multiply-add, no reassociation):
 *        s = G * G;  h' = h + s;  r = sqrt(h');  d = r + eps_V;  u = lr_V * G;  p = u / d;  w' = w - p
 *      h' is stored to state[l][c] and w' to weights[l][c].
 *   3. sqrt and / are IEEE correctly rounded; subnormal inputs and results are kept; infinities and NaN
 *      follow IEEE (a NaN's payload and sign are unspecified): G = 0, h = 0, eps = 0 gives 0 / 0 = NaN, and
 *      an overflowing G * G makes h' infinite and p zero.
 * This is mini-batch Adagrad as the sparse optimizers of the ML frameworks define it -- duplicates are
 * coalesced, then one step is taken -- not one step per record. The step needs a row's whole sum, so no run
 * is ever split and no atomic is used: there are no flags, and the answer is a function of the inputs only,
 * never of pointer alignment, the slice path or the grid. A row the push does not name is neither read nor
 * written in either shard, and neither is the pitch padding.
 * Both shards' locks are held for the call and it is ordered after both shards' earlier work, ring
 * entries and open batches of `state` included; it is synchronous for both: a following host call on
 * either shard sees the step. Every row is checked before anything is staged: a row outside the partition
 * returns GLINT_EOUTOFRANGE (the record's index in glint_shard_last_error(weights)) with both shards
 * unchanged. A slab with views is refused for either shard, as for every host-pointer call.
 * GLINT_EINVAL: a NULL, vector, Int or Long `weights`; a NULL `state`, the same handle as `weights`, one
 * that overlaps it in memory (views of one slab), or one that differs from it in dtype, device, cols, size
 * or partition (kind, start, and index / parts for cyclic); n < 0, n >= 2^32 - 2048; NULL rows or grads
 * with n > 0; a NaN lr; !(eps >= 0). n == 0 launches nothing and returns GLINT_OK. Staged to the device:
 * rows and grads in one block; nothing is copied back. Kernel timing: the one fold launch counts under
 * GLINT_K_PUSH_ROWS on `weights`; nothing is recorded on `state`. */
int glint_mat_push_rows_adagrad(glint_shard_t weights, glint_shard_t state, const int64_t* rows, const void* grads,
                                int64_t n, double lr, double eps);

/* Adam row push (an extension: the reference has no such message): lazy Adam next to the rows, on the
 * Adagrad row push's frame. `weights` is a Float or Double matrix shard of type V; `state` is a matrix
 * shard of the same dtype, device, size and partition with state.cols == 2 * weights.cols that packs both
 * moments: row l holds m in columns [0, cols) and v in [cols, 2 * cols), so a zeroed shard is the right
 * initial state. One push crosses the link with n x cols gradients and nothing else.
 *   grads  n x cols values of V, dense row-major, no pitch (glint_mat_push_rows's vals).
 * The scalars are settled once on the host, in double: c1 = 1 - pow(beta1, (double)step) and c2 = 1 -
 * pow(beta2, (double)step) with the C library's pow, alpha = lr / c1, rc2 = sqrt(c2), a1 = 1 - beta1,
 * a2 = 1 - beta2. Then beta1, beta2, a1, a2, alpha, rc2 and eps are each rounded once to V: b1, b2, a1, a2,
 * alpha, rc2, eps below. For every distinct local row l the push names:
 *   1. G[c] = (((+0 + g_i0[c]) + g_i1[c]) + ...) over the records i0 < i1 < ... with l(rows[i]) == l: the
 *      sum runs in push order, in V, from +0 (the Adagrad push's step 1).
 *   2. Per column, with m = state[l][c], v = state[l][cols + c] and w = weights[l][c], every operation in V
 *      and rounded on its own (no fused multiply-add, no reassociation):
 *        t1 = b1 * m;   t2 = a1 * G;   m' = t1 + t2
 *        q  = G * G;    t3 = b2 * v;   t4 = a2 * q;   v' = t3 + t4
 *        r  = sqrt(v'); s = r / rc2;   d = s + eps
 *        u  = alpha * m';   p = u / d;   w' = w - p
 *      m' is stored to state[l][c], v' to state[l][cols + c] and w' to weights[l][c].
 *   3. sqrt and / are IEEE correctly rounded; subnormal inputs and results are kept; infinities and NaN
 *      follow IEEE (a NaN's payload and sign are unspecified): G = 0, v = 0, eps = 0 gives 0 / 0 = NaN.
 * This is lazy (sparse) Adam as the sparse optimizers of the ML frameworks define it -- duplicates are
 * coalesced, then one step is taken, with a global `step` the caller counts from 1 -- not one step per
 * record. A row the push does not name is neither read nor written in either shard, so its moments do not
 * decay; neither is the pitch padding of either shard. No run is ever split and no atomic is used: there
 * are no flags, and the answer is a function of the inputs only, never of pointer alignment, the slice
 * path or the grid.
 * Locks, ordering, errors and slabs are glint_mat_push_rows_adagrad's: both shards' locks are held, the
 * call is ordered after both shards' earlier work and is synchronous for both; every row is checked before
 * anything is staged, and a row outside the partition returns GLINT_EOUTOFRANGE (the record's index in
 * glint_shard_last_error(weights)) with both shards unchanged. A slab with views is refused for either
 * shard.
 * GLINT_EINVAL: a NULL, vector, Int or Long `weights`; a NULL `state`, the same handle as `weights`, one
 * that overlaps it in memory, or one that differs from it in dtype, device, size or partition (kind, start,
 * and index / parts for cyclic); state.cols != 2 * weights.cols; n < 0, n >= 2^32 - 2048; NULL rows or grads
 * with n > 0; a NaN lr; !(eps >= 0); !(0 <= beta1 && beta1 < 1), likewise beta2 (a NaN beta fails the
 * test); step < 1. n == 0 launches nothing and returns GLINT_OK. Staged to the device: rows and grads in
 * one block; nothing is copied back. Kernel timing: the one fold launch counts under GLINT_K_PUSH_ROWS on
 * `weights`; nothing is recorded on `state`. */
int glint_mat_push_rows_adam(glint_shard_t weights, glint_shard_t state, const int64_t* rows, const void* grads,
                             int64_t n, double lr, double beta1, double beta2, double eps, int64_t step);

/* Row-wise Adagrad row push (an extension: the reference has no such message): Adagrad with one
 * accumulator per row, fed with the mean of the row's squared gradient -- the embedding frameworks' choice
 * for very large tables -- so that the optimizer state is 1 / cols of the table. `weights` is a Float or
 * Double matrix shard of type V; `state` is a VECTOR shard (cols == 0) of the same dtype, device, size and
 * partition: element l of `state` is the accumulator of local row l. A zeroed vector is the right initial
 * state; any other initial value is written with glint_shard_fill. One push crosses the link with n x cols
 * gradients and nothing else.
 *   grads  n x cols values of V, dense row-major, no pitch (glint_mat_push_rows_adagrad's grads).
 * lr and eps are rounded once on the host to V: lr_V, eps_V; C = (V)cols, rounded once. For every distinct
 * local row l the push names:
 *   1. G[c] = (((+0 + g_i0[c]) + g_i1[c]) + ...) over the records i0 < i1 < ... with l(rows[i]) == l: the
 *      sum runs in push order, in V, from +0 (the Adagrad push's step 1).
 *   2. ss = the row dot pull's self-dot of G, with exactly the arithmetic stated at glint_mat_pull_rows_dot:
 *      E = 16 / sizeof(V) when cols * sizeof(V) is a multiple of 16, else 1; column c belongs to lane
 *      (c / E) % 64; each lane starts from +0 and adds acc = acc + (G[c] * G[c]) in ascending c, the product
 *      rounded before the add; then the xor butterfly d = 32 .. 1. ss is a function of (type, cols, G) only.
 *   3. The row scalars, with h = state[l], every operation in V and rounded on its own:
 *        s = ss / C;  h' = h + s;  r = sqrt(h');  d = r + eps_V;  k = lr_V / d
 *      s = ss / C is a division, not a multiplication by a reciprocal, and k = lr_V / d is one division per
 *      row: one multiplier per row, as the frameworks define the step.
 *   4. Per column, with w = weights[l][c]:  p = k * G[c];  w' = w - p  (no fused multiply-add: fma(-k, G, w)
 *      is not the contract's). h' is stored to state[l] once, and w' to weights[l][c].
 *   5. sqrt and / are IEEE correctly rounded; subnormal inputs and results are kept; infinities and NaN
 *      follow IEEE (a NaN's payload and sign are unspecified). The row is coupled: one NaN gradient element
 *      makes ss, h' and every w' of that row NaN. An overflowing G * G makes h' infinite and k zero, so
 *      p = 0 * G, which is NaN where G is infinite. G = 0, h = 0, eps = 0 gives k = lr / 0 and p = inf * 0 =
 *      NaN.
 * Duplicates are coalesced, then one step is taken -- not one step per record. The step needs a row's whole
 * sum, so no run is ever split and no atomic is used: there are no flags, and the answer is a function of
 * the inputs only, never of the alignment of grads, of how wide rows are handled, or of the grid. A row the
 * push does not name is neither read nor written in either shard, and the pitch padding of `weights` is
 * never touched.
 * Locks, ordering, errors and slabs are glint_mat_push_rows_adagrad's: both shards' locks are held, the
 * call is ordered after both shards' earlier work -- the vector shard's ring entries and open batch
 * included -- and is synchronous for both; every row is checked against `weights` before anything is
 * staged, and a row outside the partition returns GLINT_EOUTOFRANGE (the record's index in
 * glint_shard_last_error(weights)) with both shards unchanged. A slab with views is refused for either
 * shard.
 * GLINT_EINVAL: a NULL, vector, Int or Long `weights`; a NULL `state`, one that is a matrix, one that
 * differs from `weights` in dtype, device, size or partition (kind, start, and index / parts for cyclic),
 * or one that shares memory with it; n < 0, n >= 2^32 - 2048; NULL rows or grads with n > 0; a NaN lr;
 * !(eps >= 0). n == 0 launches nothing and returns GLINT_OK. Staged to the device: rows and grads in one
 * block; nothing is copied back. Kernel timing: the front end counts as the row push's does and the one
 * fold launch counts under GLINT_K_PUSH_ROWS on `weights`; nothing is recorded on `state`.
 * Known limit: a run is one wave's chain for the whole row, not one per column slice, so a push dominated
 * by one hot row is bound by it more than the Adagrad row push is. */
/* Strips (64 lanes x E columns each) of a row that the fold keeps in registers between summing the
 * gradients and updating the weights: a row of more strips -- cols > 64 * E * this -- sums its run a second
 * time instead (tests size their cases by it; the bits never depend on it). */
#define GLINT_ROWWISE_KEEP_STRIPS 4
int glint_mat_push_rows_adagrad_rowwise(glint_shard_t weights, glint_shard_t state, const int64_t* rows,
                                        const void* grads, int64_t n, double lr, double eps);

/* FTRL-proximal row push (an extension: the reference has no such message): per-coordinate FTRL-proximal
 * (McMahan et al., "Ad Click Prediction: a View from the Trenches", KDD 2013, algorithm 1) next to the
 * rows, on the Adam row push's frame. Its L1 term writes exact +0 weights, so a table trained with l1 > 0
 * is sparse to glint_mat_pull_rows_sparse. `weights` is a Float or Double matrix shard of type V; `state`
 * is a matrix shard of the same dtype, device, size and partition with state.cols == 2 * weights.cols: row
 * l holds z in columns [0, cols) and n (the accumulated squared gradients) in [cols, 2 * cols). A zeroed
 * state with zeroed weights is the right start. w is a function of (z, n): the step reads w only to keep z
 * consistent with it, and weights filled any other way are simply overwritten by a row's first step. One
 * push crosses the link with n x cols gradients and nothing else.
 *   grads  n x cols values of V, dense row-major, no pitch (glint_mat_push_rows's vals).
 * alpha, beta, l1 and l2 arrive as double and are each rounded once to V: alpha, beta, l1, l2 below (the
 * checks below are made on the doubles: a Float alpha that rounds to 0 or infinity is the caller's). For
 * every distinct local row l the push names:
 *   1. G[c] = (((+0 + g_i0[c]) + g_i1[c]) + ...) over the records i0 < i1 < ... with l(rows[i]) == l: the
 *      sum runs in push order, in V, from +0 (the Adagrad push's step 1).
 *   2. Per column, with z = state[l][c], n = state[l][cols + c] and w = weights[l][c], every operation in V
 *      and rounded on its own (no fused multiply-add, no reassociation):
 *        q  = G * G;       n' = n + q
 *        r0 = sqrt(n);     r1 = sqrt(n')
 *        ds = r1 - r0;     sg = ds / alpha
 *        t  = sg * w;      u  = G - t;        z' = z + u
 *        a  = |z'|
 *        if a <= l1:  w' = +0
 *        else:        s = copysign(l1, z');   y = z' - s
 *                     b = beta + r1;  c = b / alpha;  d = c + l2
 *                     e = y / d;      w' = -e
 *      z' is stored to state[l][c] and n' to state[l][cols + c] on both branches, w' to weights[l][c].
 *      ds / alpha and b / alpha are divisions, not products with a reciprocal; ds is the difference of the
 *      two square roots, not q / (r1 + r0).
 *   3. sqrt and / are IEEE correctly rounded; subnormal inputs and results are kept; infinities and NaN
 *      follow IEEE (a NaN's payload and sign are unspecified). a <= l1 is false for a NaN z', which
 *      therefore takes the second branch and reaches w' through y. An overflowing G * G makes n' and r1
 *      infinite: sg is then infinite, t = sg * w is NaN where w == 0, and z' and w' with it. An n at the
 *      type's maximum stays finite under a small q (r1 == r0, ds = 0). With beta = 0, l2 = 0, n' = 0 and
 *      |z'| > l1, d = 0 and w' is infinite; with |z'| <= l1 the same row gives w' = +0 and d is never
 *      looked at. A negative n (never written by this call from a zeroed state) gives sqrt = NaN.
 * Duplicates are coalesced, then one step is taken -- not one step per record. A row the push does not name
 * is neither read nor written in either shard; neither is the pitch padding of either shard. No run is ever
 * split and no atomic is used: there are no flags, and the answer is a function of the inputs only, never
 * of the alignment of grads, the slice path or the grid.
 * Locks, ordering, errors and slabs are glint_mat_push_rows_adam's: both shards' locks are held, the call
 * is ordered after both shards' earlier work and is synchronous for both; every row is checked against
 * `weights` before anything is staged, and a row outside the partition returns GLINT_EOUTOFRANGE (the
 * record's index in glint_shard_last_error(weights)) with both shards unchanged. A slab with views is
 * refused for either shard.
 * GLINT_EINVAL: a NULL, vector, Int or Long `weights`; a NULL `state`, the same handle as `weights`, one
 * that overlaps it in memory, or one that differs from it in dtype, device, size or partition (kind, start,
 * and index / parts for cyclic); state.cols != 2 * weights.cols; n < 0, n >= 2^32 - 2048; NULL rows or grads
 * with n > 0; !(alpha > 0); !(beta >= 0); !(l1 >= 0); !(l2 >= 0) (a NaN fails each test); an infinite
 * alpha, beta, l1 or l2. n == 0 launches nothing and returns GLINT_OK. Staged to the device: rows and grads
 * in one block; nothing is copied back. Kernel timing: the one fold launch counts under GLINT_K_PUSH_ROWS
 * on `weights`; nothing is recorded on `state`. */
int glint_mat_push_rows_ftrl(glint_shard_t weights, glint_shard_t state, const int64_t* rows, const void* grads,
                             int64_t n, double alpha, double beta, double l1, double l2);

/* Row-pair dot pull (an extension: the reference has no such message): the read half of a two-table
 * scoring step -- skip-gram with negative sampling, matrix factorisation, any two-tower model -- where
 * the other operand is not a vector the caller sends but a row of a second shard on the same device.
 *   out   n values of the shards' type: out[i] = dot(row rows_a[i] of a, row rows_b[i] of b).
 * 2 n row ids cross the link and n values come back; nothing of size cols does.
 * Arithmetic: the row dot pull's, word for word (glint_mat_pull_rows_dot above: E, lane ownership
 * (c / E) % 64, ascending columns per lane from +0, acc = acc + (rowA[c] * rowB[c]) with the product rounded
 * before the add, the xor butterfly, Int/Long wrap): the bits of out[i] are what
 * glint_mat_pull_rows_dot(a, &rows_a[i], 1, x = the stored row rows_b[i] of b, 1, ...) returns. Only `cols`
 * elements of a row of either shard are read, never the pitch padding. No flags, no atomics.
 * Shards: `a` and `b` are matrix shards of one dtype, device and cols. Their partitions are independent
 * -- kind, start, size, cyclic index and parts may all differ -- and each row array is translated with
 * its own shard's partition. `b` may be `a` itself (rows of one table scored against each other;
 * rows_a[i] == rows_b[i] gives the self-dot's bits), and the two may be views of one slab, overlapping or
 * not: nothing is written to either.
 * Both shards' locks are held for the call (the one lock once when b == a) and it is ordered after both
 * shards' earlier work, as glint_mat_push_rows_adagrad: the work runs on a's stream, which waits for b's,
 * and the call ends synchronised. Every pair is checked before anything is staged: for the lowest i with
 * rows_a[i] outside a or rows_b[i] outside b the call returns GLINT_EOUTOFRANGE (i in
 * glint_shard_last_error(a)) with nothing written to out. A slab with views is refused for either shard,
 * as for every host-pointer call.
 * GLINT_EINVAL: a NULL or vector shard; shards that differ in dtype, device or cols; n < 0; n >= 2^31; a
 * NULL array with n > 0. n == 0 writes nothing and returns GLINT_OK. Staged to the device: the two row
 * arrays in one block; copied back: n values. Kernel timing: one launch under GLINT_K_PULL_ROWS_DOT on
 * `a`; nothing is recorded on `b`. */
int glint_mat_pull_pairs_dot(glint_shard_t a, glint_shard_t b, const int64_t* rows_a, const int64_t* rows_b,
                             int64_t n, void* out);

/* Row-pair axpy push (an extension: the reference has no such message): the write half of that step,
 * rows of `dst` += coefficients times rows of a second shard `src` on the same device.
 *   coef  n values of the shards' type, one per pair.
 * For i in push order, for c in [0, cols):
 *   dst[l(rows_dst[i])][c] = dst[l(rows_dst[i])][c] + (coef[i] * src[l_src(rows_src[i])][c]),
 * the product rounded before the add (no fused multiply-add), all arithmetic in the shards' type; Int/Long
 * wrap. The call is glint_mat_push_rows(dst, rows_dst, vals) with vals[i] = coef[i] * (row rows_src[i] of
 * src), rounding for rounding. `src` is read as it was before the call. Subnormal products and sums are
 * kept; infinities and NaN follow IEEE (inf * 0 is NaN; a NaN's payload and sign are unspecified). Only
 * `cols` elements of a row of either shard are read or written, never the pitch padding. 2 n row ids and n
 * coefficients cross the link; nothing of size cols does.
 * Shards: as glint_mat_pull_pairs_dot (one dtype, device and cols; independent partitions, each row array
 * translated with its own shard's), but `src` must share no memory with `dst`: the same handle, or two
 * views of one slab that overlap, is GLINT_EINVAL.
 * Flags, order and sizes are glint_mat_push_rows's: only GLINT_PUSH_DETERMINISTIC and GLINT_PUSH_UNORDERED
 * are accepted; Float/Double sums of repeated destination rows keep the push order unless
 * GLINT_PUSH_UNORDERED is given. Both shards' locks are held and the call is ordered after both shards'
 * earlier work; it runs on dst's stream, which waits for src's, and ends synchronised. Every pair is
 * checked before anything is applied: for the lowest i with rows_dst[i] outside dst or rows_src[i] outside
 * src nothing is applied (GLINT_EOUTOFRANGE, i in glint_shard_last_error(dst)). A slab with views is
 * refused for either shard.
 * GLINT_EINVAL: a NULL or vector shard; shards that differ in dtype, device or cols, or share memory;
 * n < 0; n >= 2^32 - 2048; any other flag; a NULL array with n > 0. n == 0 launches nothing and returns
 * GLINT_OK. Staged to the device: the two row arrays and coef in one block; nothing is copied back. Kernel
 * timing: the front end counts as glint_mat_push_rows_axpy's does and the one fold launch under
 * GLINT_K_PUSH_ROWS_AXPY, both on `dst`; nothing is recorded on `src`. */
int glint_mat_push_pairs_axpy(glint_shard_t dst, glint_shard_t src, const int64_t* rows_dst,
                              const int64_t* rows_src, const void* coef, int64_t n, int flags);

/* Grouped row push (an extension: the reference has no such message): the write side of
 * glint_mat_pull_rows_sum -- the backward pass of an embedding bag. The caller names n rows in g groups and
 * sends ONE value row per group; every record adds its group's row, optionally times a coefficient of its
 * own, so that g x cols values cross the link instead of the n x cols expanded rows glint_mat_push_rows
 * would need.
 *   grp_ptr   g + 1 int64, non-decreasing, grp_ptr[0] = 0 and grp_ptr[g] = n: group k is
 *             rows[grp_ptr[k] .. grp_ptr[k+1]) (glint_mat_pull_rows_sum's rule);
 *   vals      g x cols values of the shard's type, dense row-major (NO pitch): one row per group;
 *   coef      n values of the shard's type, one per record; may be NULL.
 * For i in push order, with k the group of record i, for c in [0, cols):
 *   data[l(rows[i])][c] = data[l(rows[i])][c] + t_i[c].
 * With coef == NULL, t_i[c] = vals[k][c]: the stored bits are used and no multiply is performed. Otherwise
 * t_i[c] = coef[i] * vals[k][c], the product rounded before the add (no fused multiply-add). All arithmetic
 * is in the shard's type; Int/Long wrap. The call is therefore glint_mat_push_rows(shard, rows, expanded, n,
 * flags) with expanded[i] = t_i, rounding for rounding. That order is a function of the inputs only --
 * never of pointer alignment, g, how records are batched over lanes, or the grid. Subnormals are kept;
 * infinities and NaN follow IEEE (inf * 0 is NaN; a NaN's payload and sign are unspecified). Only `cols`
 * elements of a row are read and written, never the pitch padding. A row may occur several times in a
 * group, and in several groups; an empty group contributes nothing.
 * Flags, order and sizes are glint_mat_push_rows's: only GLINT_PUSH_DETERMINISTIC and GLINT_PUSH_UNORDERED
 * are accepted; Float/Double sums of repeated rows keep the push order unless GLINT_PUSH_UNORDERED is given;
 * a row that occurs once is bit-exact in every mode; Int/Long are exact in every mode. Every row is checked
 * before anything is applied: on a row outside the partition nothing is applied (GLINT_EOUTOFRANGE, the
 * record's index in glint_shard_last_error). A slab with views is refused, as for every host-pointer call.
 * GLINT_EINVAL: a NULL or vector shard; n < 0, n >= 2^32 - 2048, g < 0, g >= 2^31; any other flag; a NULL
 * grp_ptr; NULL rows with n > 0; NULL vals with g > 0; and -- in this host call only, before anything is
 * staged -- a grp_ptr that breaks the rule above. n == 0 launches nothing and returns GLINT_OK. Staged to
 * the device in one block: rows, grp_ptr, coef when given, and vals (which starts 16-B aligned there) --
 * 8 n + 8 (g + 1) + n * sizeof V + g * cols * sizeof V bytes; nothing of size n x cols is ever staged, and
 * nothing is copied back. Device scratch: the row push's, and one 32-bit group id per record. Kernel timing:
 * the front end counts as glint_mat_push_rows's does (the launch that writes the group ids belongs to it) and
 * the one fold launch under GLINT_K_PUSH_ROWS. */
int glint_mat_push_rows_grouped(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                                int64_t g, const void* vals, const void* coef, int flags);

/* Weighted row-sum pull (an extension: the reference has no such message): glint_mat_pull_rows_sum with a
 * coefficient per record -- the forward pass of a weighted embedding bag, and the read-side counterpart of
 * glint_mat_push_rows_grouped's coef -- so that g x cols values answer n rows and n weights.
 *   grp_ptr   glint_mat_pull_rows_sum's: g + 1 int64, non-decreasing from 0 to n;
 *   coef      n values of the shard's type, one per record;
 *   out       g x cols values of the shard's type, dense row-major (NO pitch).
 * out[k][c] = ((coef[b] * r_b[c]) + (coef[b+1] * r_b+1[c])) + ... over the group's records b, b + 1, ... in
 * the caller's order, all in the shard's type. Every product is rounded before it is added (no fused
 * multiply-add), and the first term is the first PRODUCT as computed, not 0 + product: a group of the one
 * row -0.0 with coefficient 1 is -0.0. An empty group is all +0 / 0; Int and Long wrap. Subnormal products
 * and sums are kept; infinities and NaN follow IEEE (inf * 0 is NaN; a NaN's payload and sign are
 * unspecified: 1 * sNaN quiets). A row may occur several times in a group, and in several groups. Only
 * `cols` elements of a row are read, never the pitch padding. The answer is deterministic: no atomics, and
 * no group is split; there are no flags. With every coefficient 1 and a table without NaN the bits are
 * glint_mat_pull_rows_sum's.
 * GLINT_EINVAL: glint_mat_pull_rows_sum's cases (the grp_ptr rule in this host call only), and a NULL coef
 * with n > 0 -- an unweighted caller uses glint_mat_pull_rows_sum. g == 0 writes nothing and returns
 * GLINT_OK. Every row is checked first: a row outside the partition returns GLINT_EOUTOFRANGE (its index in
 * `rows` in glint_shard_last_error) with nothing written to out. Staged to the device in one block: rows,
 * grp_ptr and coef; copied back: g * cols values -- never n * cols. Kernel timing: one launch under
 * GLINT_K_PULL_ROWS_SUM. */
int glint_mat_pull_rows_wsum(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                             int64_t g, const void* coef, void* out);

/* Grouped row-dot pull (an extension: the reference has no such message): every record's row times the ONE
 * vector of its group -- the gradient of a weighted bag with respect to its weights, a query's scores over
 * its own candidate list, the scores of attention pooling -- so that n values answer n rows, where
 * glint_mat_pull_rows_dot with a vector per group would answer n x g.
 *   grp_ptr   glint_mat_pull_rows_sum's: g + 1 int64, non-decreasing from 0 to n;
 *   x         g x cols values of the shard's type, dense row-major (NO pitch): one vector per group;
 *   out       n values of the shard's type: out[i] = dot(row rows[i], x[k]), k the group of record i.
 * Arithmetic: glint_mat_pull_rows_dot's with q == 1, bit for bit (E, lane L = (c / E) % 64, ascending
 * columns, the product rounded before the add, the xor butterfly; Int/Long wrap): out[i] is what
 * glint_mat_pull_rows_dot(shard, &rows[i], 1, x + k * cols, 1, ...) returns. It is a function of (type,
 * cols) only -- never of the alignment of x, how records are batched over waves, or the grid. Answers keep
 * the caller's order; a row requested twice is answered twice; an empty group reads nothing of x. g is
 * limited to < 2^31 only (no GLINT_DOT_MAX_QUERIES cap). x must not overlap out.
 * GLINT_EINVAL: a NULL or vector shard, n < 0, g < 0, n >= 2^31, g >= 2^31, a NULL grp_ptr, NULL rows, x or
 * out with n > 0 and -- in this host call only, before anything is staged -- a grp_ptr that breaks the rule.
 * n == 0 writes nothing and returns GLINT_OK. Every row is checked first: a row outside the partition
 * returns GLINT_EOUTOFRANGE (its index in glint_shard_last_error) with nothing written to out. Staged to the
 * device in one block: rows, grp_ptr and x (which starts 16-B aligned there); copied back: n values -- never
 * n * cols or n * g. Kernel timing: one launch under GLINT_K_PULL_ROWS_DOT, no scratch for group ids. */
int glint_mat_pull_rows_gdot(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                             int64_t g, const void* x, void* out);

/* Narrow-format row transport (an extension: the reference has no such message): whole rows cross the link
 * in a narrower floating type W than the shard's type V, while the shard keeps full precision -- a
 * full-precision master table whose rows and gradient rows travel as half or bfloat16. A pull rounds on the
 * device, a push widens inside its fold, so sizeof W bytes per element are staged or copied back, never
 * sizeof V.
 * Pairs (V, W): (Float, F16), (Float, BF16), (Double, F32); glint_wire_supported answers 1 for these and 0 for
 * everything else (any Int or Long shard, any unknown code) and never fails. The conversions are stated, in
 * integer arithmetic, by glint_amd/csrc/glint_wire_plan.h:
 *   narrowing V -> W (a pull): one IEEE round-to-nearest-even of the stored value straight to W. Results that
 *     are subnormal in W are kept, never flushed; a magnitude that rounds beyond W's largest finite value
 *     becomes the infinity of its sign; infinities and the sign of a zero are kept; a value too small for W's
 *     smallest subnormal becomes the zero of its sign, and the tie at half the smallest subnormal goes to zero
 *     (the even result); a NaN becomes a NaN of W, payload and sign unspecified. For BF16 the non-NaN rule on
 *     the float's bits u is (u + 0x7FFF + ((u >> 16) & 1)) >> 16.
 *   widening W -> V (a push): exact. W's subnormals become the equal V values, -0 stays -0, infinities stay
 *     infinities, a NaN becomes a NaN, payload and sign unspecified.
 * F16 and BF16 values are 16-bit patterns (IEEE binary16; the upper half of a binary32), F32 values floats. */
enum glint_wire { GLINT_WIRE_F16 = 0, GLINT_WIRE_BF16 = 1, GLINT_WIRE_F32 = 2 };
int glint_wire_supported(int dtype, int wire); /* 1 or 0; never fails */

/* glint_mat_pull_rows in the wire type `wire`: out is n x cols values of W, dense row-major (NO pitch), in the
 * caller's order -- a row requested twice is answered twice -- and out[i][c] = narrow(the stored element): the
 * bits equal narrowing what glint_mat_pull_rows returns. Only `cols` elements of a row are read, never the
 * pitch padding, and nothing beyond n * cols * sizeof W bytes of out is written. No flags, no atomics, one
 * launch; the answer is a function of the shard and rows only, never of out's alignment.
 * The shard is entered as by the other extensions' host calls (the open ring batch flushed, after enqueued
 * messages and the last device-resident call; a slab with views refused); there is no ring path. Every row is
 * checked before anything is staged: for the lowest i with rows[i] outside the partition the call returns
 * GLINT_EOUTOFRANGE (i in glint_shard_last_error) with nothing written. Staged to the device: 8 n bytes;
 * copied back: n * cols * sizeof W bytes -- never n * cols * sizeof V.
 * GLINT_EINVAL: a NULL or vector shard; a (dtype, wire) pair that is not supported; n < 0; n >= 2^31; NULL rows
 * or out with n > 0. n == 0 launches nothing and returns GLINT_OK. Kernel timing: the one launch counts under
 * GLINT_K_MAT_PULL_ROWS. */
int glint_mat_pull_rows_as(glint_shard_t shard, const int64_t* rows, void* out, int64_t n, int wire);

/* glint_mat_push_rows of rows that arrive in the wire type `wire`: vals is n x cols values of W, dense
 * row-major (NO pitch), and the call is glint_mat_push_rows(shard, rows, widened, n, flags) with
 * widened[i][c] = widen(vals[i][c]), rounding for rounding: the sums run in V, the shard's element is a sum's
 * first term and the contributions are added in list order. Flags, order, the size limit (n < 2^32 - 2048),
 * the row check and the error reporting are glint_mat_push_rows's: repeated rows keep the push order unless
 * GLINT_PUSH_UNORDERED is given, a row that occurs once is bit-exact in every mode, and on a row outside the
 * partition nothing is applied (GLINT_EOUTOFRANGE, the record's index in glint_shard_last_error). A slab with
 * views is refused. Only `cols` elements of a row are read and written, never the pitch padding.
 * Staged to the device in one block: 8 n + n * cols * sizeof W bytes. Nothing of size n * cols * sizeof V is
 * staged or built in device scratch: the widening happens at the contribution load inside the fold. Nothing
 * is copied back.
 * GLINT_EINVAL: a NULL or vector shard; a (dtype, wire) pair that is not supported; n < 0; n >= 2^32 - 2048;
 * NULL rows or vals with n > 0; GLINT_PUSH_VALIDATE or an unknown flag. n == 0 launches nothing and returns
 * GLINT_OK. Kernel timing: the front end counts as glint_mat_push_rows's does and the one fold launch under
 * GLINT_K_PUSH_ROWS. */
int glint_mat_push_rows_as(glint_shard_t shard, const int64_t* rows, const void* vals, int64_t n, int wire,
                           int flags);

/* Top-k row pull (an extension: the reference has no such message): for each of q query vectors, the k
 * rows of the shard that score highest against it -- nearest-row search, candidate retrieval -- answered
 * with q x k (row, score) pairs whatever the shard's size.
 *   x         q x cols values of the shard's type, dense row-major;
 *   out_rows  q x k global row keys, dense; out_vals  q x k scores of the shard's type, dense.
 * Scores. For query j every row of the shard is scored dot(row, x[j]) with the row dot pull's arithmetic
 * (glint_mat_pull_rows_dot above: E, lane ownership and ascending columns, products rounded before the
 * add, the xor butterfly, Int/Long wrap): the score bits of a row are what glint_mat_pull_rows_dot returns
 * for it. Only `cols` elements of a row are read, never the pitch padding.
 * Order. Rows are ordered by rank descending, then global row ascending. Float/Double rank: every NaN
 * ranks below every number (-inf included), all NaNs rank equal, -0 equals +0, otherwise the numeric
 * value. Int/Long rank: the signed value.
 * Answer. Entry t of query j is the t-th row in that order: out_rows[j*k + t] its global key (on a cyclic
 * shard index + local * parts), out_vals[j*k + t] its score (a NaN's payload and sign are unspecified).
 * A shard of fewer than k rows fills the remaining entries with row -1 and value +0 / 0. The call is
 * deterministic -- no atomics -- and the answer is a function of the shard, x and k only. There are no
 * flags and no row errors: the caller names no rows.
 * GLINT_EINVAL: a NULL or vector shard, NULL x, q outside [1, GLINT_TOPK_MAX_QUERIES], k outside
 * [1, GLINT_TOPK_MAX_K], NULL out_rows or out_vals. Staged to the device: x; copied back:
 * q * k * (8 + sizeof V) bytes -- nothing of size `rows` crosses the link. */
#define GLINT_TOPK_MAX_K 1024
#define GLINT_TOPK_MAX_QUERIES 64
/* Candidates one workgroup selects from (tests size their cases by it; the answer never depends on it). */
#define GLINT_TOPK_TILE 4096
int glint_mat_pull_topk(glint_shard_t shard, const void* x, int64_t q, int64_t k, int64_t* out_rows,
                        void* out_vals);

/* After GLINT_EOUTOFRANGE: index (within the failing call) of the first rejected record. */
int glint_shard_last_error(glint_shard_t shard, int64_t* first_bad_record);

/* ---- device-resident variants (stream-ordered, no host synchronisation) --------------------- *
 * All pointers are device pointers on the shard's device; `stream` is a hipStream_t used exactly
 * as given (NULL = the HIP null stream, as in the HIP API). All device-resident calls on one shard
 * must be ordered (one stream, or event-ordered streams), as the actor model orders its messages.
 * Errors are accumulated on the device and reported by glint_shard_sync. */
int glint_vec_push_dev(glint_shard_t shard, const int64_t* keys, const void* vals, int64_t n,
                       int flags, void* stream);
int glint_vec_pull_dev(glint_shard_t shard, const int64_t* keys, void* out, int64_t n, void* stream);
int glint_mat_push_dev(glint_shard_t shard, const int64_t* rows, const int32_t* cols,
                       const void* vals, int64_t n, int flags, void* stream);
int glint_mat_pull_dev(glint_shard_t shard, const int64_t* rows, const int32_t* cols, void* out,
                       int64_t n, void* stream);
int glint_mat_pull_rows_dev(glint_shard_t shard, const int64_t* rows, void* out, int64_t n,
                            void* stream);
/* glint_mat_push_rows, device-resident: a row outside the partition is skipped and reported by
 * glint_shard_sync (the lowest such record index); the other rows are applied. Int/Long sums are
 * exact. Float/Double: a row that occurs once in the push is bit-exact; sums of repeated rows keep the
 * push order with GLINT_PUSH_DETERMINISTIC, else long lists may be split and added unordered. */
int glint_mat_push_rows_dev(glint_shard_t shard, const int64_t* rows, const void* vals, int64_t n, int flags,
                            void* stream);

/* glint_shard_fill / glint_shard_init_uniform, device-resident: the same bits, one launch,
 * stream-ordered on `stream` with no host synchronisation, after the shard's host-pointer work; the
 * shard is marked for its next sync. rows (device memory) as above; a row outside the partition is
 * skipped -- nothing is written for it -- and reported by glint_shard_sync as the lowest such index; the
 * other rows are written. A slab is ordered with its views as in glint_mat_push_rows_dev. `value` is host
 * memory, read before the call returns. */
int glint_shard_fill_dev(glint_shard_t shard, const int64_t* rows, int64_t n, const void* value, void* stream);
int glint_shard_init_uniform_dev(glint_shard_t shard, const int64_t* rows, int64_t n, uint64_t seed, double lo,
                                 double hi, void* stream);

/* glint_mat_pull_rows_sparse, device-resident: the same triple and capacity rule, stream-ordered on
 * `stream` with no host synchronisation, so the caller reads row_ptr[n] itself (and compares it with
 * cap) after waiting on the stream. A row outside the partition has 0 entries and is reported by
 * glint_shard_sync (the lowest such request index), as for glint_mat_pull_rows_dev; the other rows are
 * answered. Scratch is the shard's growable device scratch. */
int glint_mat_pull_rows_sparse_dev(glint_shard_t shard, const int64_t* rows, int64_t n, int64_t* row_ptr,
                                   int32_t* out_cols, void* out_vals, int64_t cap, void* stream);

/* glint_mat_pull_rows_sum, device-resident: the same sums, stream-ordered on `stream` with no host
 * synchronisation, one launch. A row outside the partition contributes a row of zeros (as
 * glint_mat_pull_rows_dev answers such a row with zeros) and is reported by glint_shard_sync as the
 * lowest such index in `rows`; every other row is summed. grp_ptr is not checked on the host: the kernel
 * clamps every grp_ptr value it reads to [0, n] and treats end < start as an empty group, so a malformed
 * grp_ptr can never index outside `rows`. `out` 16-B aligned takes the 16-B path when cols allow;
 * any element-aligned `out` gives the same bits. */
int glint_mat_pull_rows_sum_dev(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                                int64_t g, void* out, void* stream);

/* glint_mat_pull_rows_wsum, device-resident: the same sums, stream-ordered on `stream` with no host
 * synchronisation, one launch. grp_ptr is read as glint_mat_pull_rows_sum_dev reads it: every value
 * clamped to [0, n], end < start an empty group. A row outside the partition contributes the term +0 / 0
 * whatever its coefficient -- its row is not loaded and its coefficient is not used, so an infinite
 * coefficient makes no NaN there -- and
 * is reported by glint_shard_sync as the lowest such index in `rows`; every other record is summed. `out`
 * 16-B aligned takes the 16-B path when cols allow; any element-aligned `out` gives the same bits. */
int glint_mat_pull_rows_wsum_dev(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                                 int64_t g, const void* coef, void* out, void* stream);

/* glint_mat_pull_rows_gdot, device-resident: the same dots in the same order, stream-ordered on `stream`
 * with no host synchronisation, one launch. grp_ptr is not checked on the host: every value the kernel
 * reads is clamped to [0, n], and the group of record i is the k with cut[k] <= i < cut[k+1] found by an
 * upper-bound search over the clamped values (glint_mat_push_rows_grouped_dev's rule, the same code). A
 * record that no group covers answers +0 / 0 and is not an error, as that push skips it. A row outside the
 * partition answers +0 / 0 without a load and is reported by glint_shard_sync as the lowest such request
 * index; every other record is answered. x is read by 16 B when it is 16-B aligned (and cols allow), else
 * element by element: the same bits either way. */
int glint_mat_pull_rows_gdot_dev(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                                 int64_t g, const void* x, void* out, void* stream);

/* glint_mat_pull_rows_dot, device-resident: the same dots in the same order, stream-ordered on `stream`
 * with no host synchronisation, one launch. A row outside the partition answers q zeros without a load
 * (as glint_mat_pull_rows_dev answers such a row with zeros) and is reported by glint_shard_sync as the
 * lowest such request index; every other row is answered. x is read by 16 B when it is 16-B aligned
 * (and cols allow), else element by element: the same bits either way. out is written element by
 * element. */
int glint_mat_pull_rows_dot_dev(glint_shard_t shard, const int64_t* rows, int64_t n, const void* x, int64_t q,
                                void* out, void* stream);

/* glint_mat_pull_topk, device-resident: the same answer, stream-ordered on `stream` with no host
 * synchronisation: one scores launch and one launch per selection level. out_rows and out_vals must not
 * overlap x. x is read by 16 B when it is 16-B aligned (and cols allow), else element by element: the
 * same bits either way. Scratch is the shard's growable device scratch. */
int glint_mat_pull_topk_dev(glint_shard_t shard, const void* x, int64_t q, int64_t k, int64_t* out_rows,
                            void* out_vals, void* stream);

/* glint_mat_push_rows_axpy, device-resident: the same contributions in the same order, stream-ordered on
 * `stream` with no host synchronisation. A row outside the partition is skipped and reported by
 * glint_shard_sync (the lowest such record index); the other rows are applied. Int/Long sums are exact.
 * Float/Double: every t_i is bit-exact in every mode, and a row that occurs once in the push is bit-exact;
 * sums of repeated rows keep the push order with GLINT_PUSH_DETERMINISTIC, else long lists may be split
 * and their partial sums added unordered. x is read by 16 B when it is 16-B aligned (and cols allow), else
 * element by element; coef element by element: the same bits either way. */
int glint_mat_push_rows_axpy_dev(glint_shard_t shard, const int64_t* rows, int64_t n, const void* coef,
                                 const void* x, int64_t q, int flags, void* stream);

/* glint_mat_push_rows_adagrad, device-resident: the same step with the same bits, stream-ordered on
 * `stream` with no host synchronisation, after both shards' host-pointer work; both shards are marked for
 * their next sync. A row outside the partition is skipped -- it contributes to no G -- and is reported by
 * glint_shard_sync(weights, ...) as the lowest such record index; every other row is stepped. grads is
 * read by 16 B when it is 16-B aligned (and cols allow), else element by element: the same bits either
 * way. A slab that has views is GLINT_EINVAL for either shard (the call holds the two shards' locks, not
 * the views'). */
int glint_mat_push_rows_adagrad_dev(glint_shard_t weights, glint_shard_t state, const int64_t* rows,
                                    const void* grads, int64_t n, double lr, double eps, void* stream);

/* glint_mat_push_rows_adam, device-resident: the same step with the same bits, stream-ordered on `stream`
 * with no host synchronisation, after both shards' host-pointer work; both shards are marked for their
 * next sync. A row outside the partition is skipped -- it contributes to no G -- and is reported by
 * glint_shard_sync(weights, ...) as the lowest such record index; every other row is stepped. grads is
 * read by 16 B when it is 16-B aligned (and cols allow), else element by element: the same bits either
 * way. A slab that has views is GLINT_EINVAL for either shard. */
int glint_mat_push_rows_adam_dev(glint_shard_t weights, glint_shard_t state, const int64_t* rows, const void* grads,
                                 int64_t n, double lr, double beta1, double beta2, double eps, int64_t step,
                                 void* stream);

/* glint_mat_push_rows_adagrad_rowwise, device-resident: the same step with the same bits, stream-ordered on
 * `stream` with no host synchronisation, after both shards' host-pointer work; both shards are marked for
 * their next sync. A row outside the partition is skipped -- it contributes to no G -- and is reported by
 * glint_shard_sync(weights, ...) as the lowest such record index; every other row is stepped. grads is
 * read by 16 B when it is 16-B aligned (and cols allow), else element by element: the same bits either
 * way. A slab that has views is GLINT_EINVAL for either shard. */
int glint_mat_push_rows_adagrad_rowwise_dev(glint_shard_t weights, glint_shard_t state, const int64_t* rows,
                                            const void* grads, int64_t n, double lr, double eps, void* stream);

/* glint_mat_push_rows_ftrl, device-resident: the same step with the same bits, stream-ordered on `stream`
 * with no host synchronisation, after both shards' host-pointer work; both shards are marked for their
 * next sync. A row outside the partition is skipped -- it contributes to no G -- and is reported by
 * glint_shard_sync(weights, ...) as the lowest such record index; every other row is stepped. grads is
 * read by 16 B when it is 16-B aligned (and cols allow), else element by element: the same bits either
 * way. A slab that has views is GLINT_EINVAL for either shard. */
int glint_mat_push_rows_ftrl_dev(glint_shard_t weights, glint_shard_t state, const int64_t* rows, const void* grads,
                                 int64_t n, double alpha, double beta, double l1, double l2, void* stream);

/* glint_mat_pull_pairs_dot, device-resident: the same dots with the same bits, one launch, stream-ordered
 * on `stream` with no host synchronisation, after both shards' host-pointer work; both shards are marked
 * for their next sync. A pair with either row outside its partition answers 0 without a load and is
 * reported by glint_shard_sync(a, ...) as the lowest such pair index; every other pair is answered. out is
 * written element by element. A slab that has views is GLINT_EINVAL for either shard (the call holds the
 * two shards' locks, not the views'). */
int glint_mat_pull_pairs_dot_dev(glint_shard_t a, glint_shard_t b, const int64_t* rows_a, const int64_t* rows_b,
                                 int64_t n, void* out, void* stream);

/* glint_mat_push_pairs_axpy, device-resident: the same contributions, stream-ordered on `stream` with no
 * host synchronisation, after both shards' host-pointer work; both shards are marked for their next sync.
 * A record with either row outside its partition contributes nothing -- the destination's bits are as if
 * the record were absent, not as if +0 were added -- and is reported by glint_shard_sync(dst, ...) as the
 * lowest such record index; the other records are applied. Int/Long sums are exact. Float/Double: every
 * contribution is bit-exact in every mode, and a destination row that occurs once in the push is
 * bit-exact; sums of repeated rows keep the push order with GLINT_PUSH_DETERMINISTIC, else runs longer
 * than 128 records are split and their partial sums added with atomics. A slab that has views is
 * GLINT_EINVAL for either shard. */
int glint_mat_push_pairs_axpy_dev(glint_shard_t dst, glint_shard_t src, const int64_t* rows_dst,
                                  const int64_t* rows_src, const void* coef, int64_t n, int flags, void* stream);

/* glint_mat_push_rows_grouped, device-resident: the same contributions, stream-ordered on `stream` with no
 * host synchronisation (a device call like glint_mat_push_rows_dev). A row outside the partition is skipped
 * and reported by glint_shard_sync (the lowest such record index); the other records are applied. Int/Long
 * sums are exact. Float/Double: every contribution is bit-exact in every mode, and a row that occurs once
 * in the push is bit-exact; sums of repeated rows keep the push order with GLINT_PUSH_DETERMINISTIC, else
 * runs longer than 128 records are split and their partial sums added with atomics.
 * grp_ptr is not checked on the host: the kernel clamps every value it reads to [0, n]. If the clamped
 * array c is non-decreasing, record i belongs to the group k with c[k] <= i < c[k+1], or to none; a record
 * that no group covers contributes nothing -- the row's bits are as if the record were absent -- and is not
 * reported. If the clamped array decreases somewhere, which group a record gets is unspecified; the kernel
 * still never reads outside grp_ptr[0 .. g], the g rows of vals, rows or coef.
 * vals is read by 16 B when it is 16-B aligned and cols * sizeof V is a multiple of 16, else element by
 * element; coef element by element: the same bits either way. */
int glint_mat_push_rows_grouped_dev(glint_shard_t shard, const int64_t* rows, int64_t n, const int64_t* grp_ptr,
                                    int64_t g, const void* vals, const void* coef, int flags, void* stream);

/* glint_mat_pull_rows_as, device-resident: the same bits, one launch, stream-ordered on `stream` with no host
 * synchronisation (a device call like glint_mat_pull_rows_dev). A row outside the partition is answered with
 * zeros -- bit pattern 0, written without a load -- and reported by glint_shard_sync as the lowest such
 * request index; the other rows are served. When cols * sizeof V is a multiple of 16 and out is 8-B aligned,
 * a lane turns 16 B of shard row into 8 B of out; else the kernel goes element by element. out may have any
 * W-element alignment: the same bits either way. */
int glint_mat_pull_rows_as_dev(glint_shard_t shard, const int64_t* rows, void* out, int64_t n, int wire,
                               void* stream);
/* glint_mat_push_rows_as, device-resident: the same contributions, stream-ordered on `stream` with no host
 * synchronisation (a device call like glint_mat_push_rows_dev). A row outside the partition is skipped and
 * reported by glint_shard_sync (the lowest such record index); the other records are applied. A row that
 * occurs once in the push is bit-exact; sums of repeated rows keep the push order with
 * GLINT_PUSH_DETERMINISTIC, else runs longer than 128 records are split and their partial sums added with
 * atomics. vals is read by 8 B per lane -- the columns of the lane's 16 B of shard row -- when it is 8-B
 * aligned and cols * sizeof V is a multiple of 16, else element by element; it may have any W-element
 * alignment: the same bits either way. */
int glint_mat_push_rows_as_dev(glint_shard_t shard, const int64_t* rows, const void* vals, int64_t n, int wire,
                               int flags, void* stream);

/* glint_vec_push_dev / glint_mat_push_dev behind a device-side gate: the push is enqueued at once,
 * and when it runs it applies NOTHING if the 64-bit device word *gate is nonzero (a route status word,
 * glint_route_gather_dev's bad_dev: a batch with a key outside the partitioner is not applied, as
 * AsyncBigVector.mapPartitions throws before any message is sent, AsyncBigVector.scala:96-98). The
 * client reads the word after its one wait, so no host synchronisation separates the route from the
 * push. The push takes the check + apply path (GLINT_PUSH_UNORDERED is ignored); deterministic pushes
 * and unaligned arrays (keys not 16-B aligned, values not 2-element aligned) are GLINT_EINVAL. */
/* With GLINT_PUSH_VALIDATE the push writes *gate itself (see the flag): no route in front. The gate
 * word may be device memory or lie in a glint_host_alloc buffer (the caller then reads the verdict
 * from host memory after its wait, with no copy). */
int glint_vec_push_dev_gated(glint_shard_t shard, const int64_t* keys, const void* vals, int64_t n,
                             int flags, uint64_t* gate, void* stream);
int glint_mat_push_dev_gated(glint_shard_t shard, const int64_t* rows, const int32_t* cols,
                             const void* vals, int64_t n, int flags, uint64_t* gate, void* stream);

/* Waits for the shard's pending device work on `stream` and returns GLINT_EOUTOFRANGE if any
 * device-resident call since the last sync saw an out-of-range record (first_bad_record = its
 * index within the call that saw it, may be NULL). Clears the device error state. */
int glint_shard_sync(glint_shard_t shard, void* stream, int64_t* first_bad_record);
/* glint_shard_sync for n DISTINCT shards at once, shard i's calls on streams[i] (the local pushes of one
 * exchange step, each on a stream of its own): every error-state copy is enqueued before the first
 * wait, so the n waits overlap. rcs[i] / first_bad[i] (may be NULL): what glint_shard_sync(shards[i],
 * streams[i], ...) returns and reports. Returns GLINT_OK when every rcs[i] is, else the first other
 * code (GLINT_EINVAL for a NULL or repeated shard, before anything is waited for). */
int glint_shards_sync(glint_shard_t* shards, void** streams, int n, int* rcs, int64_t* first_bad);

/* Device pointer to the shard's data (row-major, row pitch from glint_shard_pitch) for
 * stream-ordered consumers (RCCL exchange buffers, checkpoint dumps, tests). */
int glint_shard_data(glint_shard_t shard, void** device_ptr);
int glint_shard_pitch(glint_shard_t shard, int64_t* elements_per_row);

/* ---- wire ingest (RequestSerializer / ResponseSerializer byte images) ----------------------- *
 * payload is the exact byte image RequestSerializer.toBinary produces
 * (src/main/scala/glint/serialization/RequestSerializer.scala:92-205): native-endian
 * [u8 type][i32 n]([i32 id])[i64 keys x n]([i32 cols x n])([V values x n]); keys start at the
 * unaligned offset 5 or 9. */

/* Applies a Push{Vector,Matrix}{Int,Long,Float,Double} message; *id receives its id. */
int glint_push_wire(glint_shard_t shard, const uint8_t* payload, size_t len, int32_t* id, int flags);

/* Answers a PullVector / PullMatrix / PullMatrixRows message with the ResponseSerializer image
 * [u8 type][i32 n][V x n] (ResponseSerializer.scala:43-117). *out_len receives the image size;
 * if cap is too small nothing is written, *out_len is set and GLINT_EINVAL returned. */
int glint_pull_wire(glint_shard_t shard, const uint8_t* payload, size_t len, uint8_t* response,
                    size_t cap, size_t* out_len);

/* ---- pipelined host ingest ----------------------------------------------------------------------- *
 * For servers whose messages arrive faster than one at a time (GranularBigVector/AsyncBigVector send
 * a batch's messages without waiting for one another, GranularBigVector.scala:39-50): a push is put
 * in one of the shard's GLINT_RING_SLOTS pinned host slots and enqueued on the shard's stream without
 * waiting. Pushes of up to GLINT_ZERO_COPY_MAX records are read by the kernel straight from the
 * pinned slot (no copy command); larger ones cross PCIe in one DMA. Tickets number the enqueued
 * pushes of a shard; glint_shard_wait(ticket) returns once that push and every push enqueued before
 * it are applied -- what the actor needs before it answers AcknowledgeReceipt
 * (PushLogic.scala:40-66). Every other call on the shard is ordered after the enqueued pushes.
 * Errors belong to the call that enqueues a message, as the reference's update/get throw while the
 * actor handles the Push/Pull message itself (PartialVectorDouble.scala:17-23): the enqueueing call
 * checks every record first and returns GLINT_EOUTOFRANGE (first bad record via
 * glint_shard_last_error) with nothing of that message enqueued; a wait reports only a launch that
 * failed on the device (GLINT_EDEVICE, once, to the first wait covering it).
 * Flags as for glint_vec_push (message order kept for Float/Double unless GLINT_PUSH_UNORDERED).
 * An entry of up to GLINT_ZERO_COPY_MAX records is ONE single-workgroup kernel that signals its own
 * completion through a host-mapped word (no event, no copy command): a few microseconds of stream
 * time per message. Pulls can be enqueued the same way (glint_pull_async), so a server answering a
 * burst of Pull messages waits once for all of them. Consecutive message-sized pushes with the same
 * flags, and consecutive message-sized element pulls, are coalesced into one launch per batch (the
 * batch goes to the GPU when it is full or anything else needs the stream); every message keeps its
 * own ticket and its own errors. Tickets number pushes and pulls together. */
#ifndef GLINT_RING_SLOTS
#define GLINT_RING_SLOTS 16
#endif
#define GLINT_ZERO_COPY_MAX 4096

/* A free slot for a push of n records, with the section pointers the caller fills: keys (i64 x n),
 * cols (i32 x n, matrix shards only, else NULL) and vals (n values of the shard's type). Waits for
 * the slot's previous push if it is still in flight. The JNI shim copies the JVM arrays straight in
 * (Get<T>ArrayRegion): no critical region, no second copy. n <= 2^20. */
int glint_stage_acquire(glint_shard_t shard, int64_t n, void** keys, void** cols, void** vals, int* slot);
/* Enqueues the push of the n records staged in `slot`; *ticket receives its ticket. */
int glint_push_staged(glint_shard_t shard, int slot, int64_t n, int flags, uint64_t* ticket);
/* glint_push_wire, enqueued: the payload is copied into a slot before the call returns. A push of more
 * than 4 MiB of records (far above the 79 999-record frame cap) is applied before the call returns
 * instead, through the staged copies, so the ring's pinned memory stays bounded. */
int glint_push_wire_async(glint_shard_t shard, const uint8_t* payload, size_t len, int32_t* id, int flags,
                          uint64_t* ticket);
/* Waits for the entry with this ticket and every earlier one and completes their pulls' answers;
 * GLINT_EDEVICE if one of them failed to launch. */
int glint_shard_wait(glint_shard_t shard, uint64_t ticket, int64_t* first_bad);
/* glint_vec_pull (kind 0), glint_mat_pull (1) or glint_mat_pull_rows (2), enqueued: the keys (and
 * cols) are checked and copied before the call returns; `out` receives the answer by the time
 * glint_shard_wait(*ticket) returns and must stay valid until then. n <= 2^20. An answer of more than
 * 16 MiB (row pulls of wide matrices) is produced before the call returns instead, so the ring's pinned
 * memory stays bounded. */
int glint_pull_async(glint_shard_t shard, int kind, const int64_t* keys, const int32_t* cols, void* out,
                     int64_t n, uint64_t* ticket);
/* glint_pull_wire, enqueued: the response header is written at once, its values by the time
 * glint_shard_wait(*ticket) returns (the response buffer must stay valid until then). */
int glint_pull_wire_async(glint_shard_t shard, const uint8_t* payload, size_t len, uint8_t* response,
                          size_t cap, size_t* out_len, uint64_t* ticket);

/* ---- client routing (device) -------------------------------------------------------------- *
 * Replaces the client-side grouping in AsyncBigVector/AsyncBigMatrix.mapPartitions
 * (src/main/scala/glint/models/client/async/AsyncBigVector.scala:96-98, AsyncBigMatrix.scala:
 * 150-152): a stable counting sort of the n device-resident keys by owning partition under
 * RangePartitioner.apply(nparts, nkeys) (RangePartitioner.scala:27-84) or
 * CyclicPartitioner.apply(nparts, nkeys) (CyclicPartitioner.scala:19-22, 41-50). On return (the
 * call synchronises `stream`): order[0..n) holds the record indices grouped by partition, each
 * group in the caller's order; counts[0..nparts) (device) the group sizes. Out-of-range keys
 * (IndexOutOfBoundsException in partition()) -> GLINT_EOUTOFRANGE with the first bad record index
 * in *first_bad (host), else *first_bad = -1. nparts <= 8192, n < 2^32. */
enum glint_route_kind { GLINT_ROUTE_RANGE = 0, GLINT_ROUTE_CYCLIC = 1 };
int glint_route_dev(const int64_t* keys, int64_t n, int kind, int32_t nparts, int64_t nkeys,
                    int64_t* counts, int64_t* order, int64_t* first_bad, void* stream);

/* The exchange's send buffers in one pass, with no host synchronisation (AsyncBigVector.scala:96-116,
 * AsyncBigMatrix.scala:141-156): records grouped as glint_route_dev groups them -- by partition, or
 * by slot_of[partition] (device array of nparts group indices, e.g. partitions ordered by hosting
 * rank; NULL = identity) -- each group in the caller's order, and written in that order into every
 * non-NULL output: order (record indices), out_keys, out_cols (from cols), out_vals (vsize = 4 or 8
 * bytes per value, from vals). counts[0..nparts) (device) receives the group sizes. The first bad
 * record is left in the device word *bad_dev as ~index (0 = none); bad records are in no group.
 * With every output NULL only counts and *bad_dev are produced (a one-partition batch is its own
 * send buffer). Stream-ordered on `stream`; the caller reads counts and *bad_dev when it needs them. */
int glint_route_gather_dev(const int64_t* keys, const int32_t* cols, const void* vals, int vsize, int64_t n,
                           int kind, int32_t nparts, int64_t nkeys, const int32_t* slot_of, int64_t* counts,
                           int64_t* order, int64_t* out_keys, int32_t* out_cols, void* out_vals,
                           uint64_t* bad_dev, void* stream);

/* glint_route_gather_dev with every key written to out_keys as key + key_delta[group] (device array
 * of nparts int64, indexed like the groups): a partition's keys rebased to their rows in the slab of
 * the rank that hosts it (glint_shard_create_in), so the receiving rank pushes everything it receives
 * as ONE call on its slab instead of one per partition (the reference's one message per partition,
 * AsyncBigVector.scala:96-116). out_keys and key_delta non-NULL, nparts >= 2. */
int glint_route_gather_rebased_dev(const int64_t* keys, const int32_t* cols, const void* vals, int vsize,
                                   int64_t n, int kind, int32_t nparts, int64_t nkeys, const int32_t* slot_of,
                                   const int64_t* key_delta, int64_t* counts, int64_t* order,
                                   int64_t* out_keys, int32_t* out_cols, void* out_vals, uint64_t* bad_dev,
                                   void* stream);

/* ---- exchange glue (device) ----------------------------------------------------------------- *
 * The client side of a routed pull: AsyncBigVector.pull writes each partition's answer back to the
 * positions its keys came from (`result(indices(i)) = values(i)`, AsyncBigVector.scala:61-79;
 * whole rows in AsyncBigMatrix.pull(rows), AsyncBigMatrix.scala:53-86). Stream-ordered on `stream`,
 * no host synchronisation; device pointers.
 * dst[order[i]] = src[i] for i < n, rows of row_bytes bytes (a multiple of 4); order is the record
 * index array glint_route_gather_dev wrote (or a sub-range of it). */
int glint_scatter_rows_dev(const void* src, const int64_t* order, int64_t n, int64_t row_bytes, void* dst,
                           void* stream);
/* A multi-range copy in one launch: segs is a HOST array of nseg (src_offset, dst_offset, bytes)
 * triples (byte offsets, multiples of 4); segment k copies src + src_offset to dst + dst_offset. Used to
 * gather a local partition's records that arrived from several source ranks into one buffer, and to
 * put its answers back into the response buffer's ranges. */
int glint_copy_segments_dev(const void* src, void* dst, const int64_t* segs, int nseg, void* stream);
/* The (rank, local partition) count matrix of a split exchange, from the route's per-partition counts:
 * send[cells[p]] = counts[p] for p < nparts and every other of the ncells entries 0; all ncells
 * entries 0 when the route's status word *bad_dev is nonzero (NULL: no status word) -- a rank with an
 * out-of-range key sends nothing but still joins the collectives. Device arrays, one launch. */
int glint_send_matrix_dev(const int64_t* counts, const int64_t* cells, int32_t nparts, int32_t ncells,
                          const uint64_t* bad_dev, int64_t* send, void* stream);

/* ---- row sampler (device) ------------------------------------------------------------------ *
 * Seeded weighted sampling of rows on the device (an extension: the word2vec forks of the reference draw
 * their negatives on the servers from a seed; the reference itself has no such message): what a skip-gram
 * or two-tower step needs besides the pair calls, so that no sampled id crosses the link. A sampler is an
 * immutable table on one device, built once from integer weights; it is not a shard. Every draw is a
 * function of the table, the seed and the draw's counter only, so the scoring call and the later adjusting
 * call regenerate the same negatives from (seed, first), on any rank, in any batch split.
 * Table: m weights w[0 .. m), 1 <= m < 2^31, each 0 <= w[i] < 2^32, their total T >= 1 (T < 2^63: no sum
 * overflows, in any order). cdf[i] = w[0] + ... + w[i] (inclusive) in 64 bits. Entry i stands for the
 * global key first_key + i.
 * One attempt, for draw counter d (uint64), attempt t (uint32) and seed (uint64):
 *   (o0, o1, o2, o3) = Philox4x32-10(counter (lo32(d), hi32(d), t, 1), key (lo32(seed), hi32(seed)))
 * -- counter word 3 is 1 where glint_shard_init_uniform has 0, so the two streams of one seed are disjoint --
 *   r = o0 | (uint64)o1 << 32;  x = floor(r * T / 2^64), the high 64 bits of the 128-bit product (0 <= x < T);
 *   idx = the smallest i with cdf[i] > x.
 * A zero-weight entry is never drawn; runs of equal cdf values are followed to their end.
 * One draw: draw i of a call has counter d = first + i (mod 2^64). Without exclusion it is attempt 0. With
 * exclusion the caller passes `exclude`, ceil(n / per) global keys, and per >= 1: draw i avoids forb =
 * exclude[i / per] (the positive that the `per` negatives are drawn for). Attempts t = 0 .. GLINT_SAMPLE_MAX_TRIES
 * - 1 are made in order and the first whose key differs from forb is the draw; if all hit forb the draw is
 * the next entry of non-zero weight after it, cyclically (the smallest i with cdf[i] > cdf[forb] mod T), so a
 * draw equals forb only when forb is the table's only non-zero entry. A forb outside [first_key, first_key +
 * m) excludes nothing. The answer is a function of (weights, first_key, seed, first, i, exclude, per) only:
 * never of n, of how a range of counters is split over calls, of the grid, of pointer alignment or of the
 * shape of the search (glint_amd/csrc/glint_sample_plan.h states it as code).
 * Creates (synchronous, one-time calls): glint_sampler_create stages host weights; _create_dev reads device
 * memory after the work already on `stream`; _create_from_shard reads a range vector shard of Int or Long
 * -- counts accumulated by ordinary pushes -- entered as by the host-pointer calls (the open ring batch
 * flushed, after enqueued messages and the last device-resident call, a slab with views refused), with the
 * shard's start as first_key and its size as m; the shard is only read. The weights are checked on the
 * device: for the lowest i with w[i] < 0 or w[i] >= 2^32 the create returns GLINT_EOUTOFRANGE and stores i in
 * *first_bad (which may be NULL; -1 is stored otherwise). GLINT_EINVAL: a NULL `out` or weights pointer, m <
 * 1, m >= 2^31, T == 0; from a shard: a NULL, matrix, Float, Double or cyclic shard. No handle is produced
 * on any error (*out = NULL). The table costs 8 m bytes plus the coarse table; nothing else of the
 * build is kept (a sampler that has served a host draw also keeps that call's stream and staging buffer, at
 * most 2^22 draws' worth).
 * Draws: out receives n global keys. exclude == NULL: no exclusion, per is ignored. GLINT_EINVAL: a NULL
 * sampler; n < 0; n >= 2^31; a NULL out with n > 0; a non-NULL exclude with per < 1. n == 0 launches nothing.
 * glint_sampler_draw (host pointers) stages exclude (8 ceil(n / per) bytes), copies back 8 n bytes and ends
 * synchronised; host calls on one sampler are serialised internally. glint_sampler_draw_dev (device
 * pointers) is one launch on `stream`: no host synchronisation, no scratch, no lock -- a sampler is
 * immutable, so any number of streams may draw from it at once; destroy it after they have drained.
 * Kernel timing: a sampler is not a shard and has no kernel id; time it with events on `stream`. */
typedef struct glint_sampler* glint_sampler_t;
#define GLINT_SAMPLE_MAX_TRIES 8
/* Entries of the coarse table the search narrows in first (tests size their cases by it; the bits never
 * depend on it). */
#define GLINT_SAMPLE_COARSE 4096
int glint_sampler_create(int device, const int64_t* weights, int64_t m, int64_t first_key, int64_t* first_bad,
                         glint_sampler_t* out);
int glint_sampler_create_dev(int device, const int64_t* weights_dev, int64_t m, int64_t first_key, void* stream,
                             int64_t* first_bad, glint_sampler_t* out);
int glint_sampler_create_from_shard(glint_shard_t counts, int64_t* first_bad, glint_sampler_t* out);
int glint_sampler_destroy(glint_sampler_t sampler);
/* Any of the four may be NULL. total = T. */
int glint_sampler_info(glint_sampler_t sampler, int64_t* m, int64_t* first_key, int64_t* total, int* device);
int glint_sampler_draw(glint_sampler_t sampler, uint64_t seed, uint64_t first, int64_t n, const int64_t* exclude,
                       int64_t per, int64_t* out);
int glint_sampler_draw_dev(glint_sampler_t sampler, uint64_t seed, uint64_t first, int64_t n,
                           const int64_t* exclude, int64_t per, int64_t* out, void* stream);

/* ---- kernel timing ------------------------------------------------------------------------- *
 * With profiling on, every kernel launch of the shard is bracketed by HIP events recorded on the
 * stream it is launched on; glint_prof_read waits for them and returns the summed device time and
 * launch count of one kernel kind since the last reset. Used by bench.py for the roofline figure. */
enum glint_kernel_id {
  GLINT_K_PUSH_APPLY = 0,   /* plain-RMW push of the increasing prefix (the dense hot path) */
  GLINT_K_PUSH_SCATTER = 1, /* LDS-aggregated atomic push of the unordered tail */
  GLINT_K_VEC_PULL = 2,
  GLINT_K_MAT_PULL = 3,
  GLINT_K_MAT_PULL_ROWS = 4, /* also the one launch of a narrow-format row pull (glint_mat_pull_rows_as*) */
  GLINT_K_PUSH_CHECK = 5,   /* order / affinity check over the keys in front of push_apply */
  GLINT_K_PUSH_BINNED = 6,  /* the binned unordered-push pipeline (count, partition, apply) */
  GLINT_K_PUSH_ORDERED = 7, /* the order-preserving push of message-sized pushes (one launch) */
  /* the per-destination fold of a whole-row push (glint_mat_push_rows*), and the one fold launch of a
   * non-empty Adagrad, row-wise Adagrad, Adam or FTRL row push (glint_mat_push_rows_adagrad*,
   * glint_mat_push_rows_adagrad_rowwise*, glint_mat_push_rows_adam*, glint_mat_push_rows_ftrl*), recorded on
   * its weights shard only. Also
   * the one launch of a shard fill or uniform init (glint_shard_fill*, glint_shard_init_uniform*), and the
   * one fold launch of a non-empty grouped row push (glint_mat_push_rows_grouped*) or narrow-format row push
   * (glint_mat_push_rows_as*) */
  GLINT_K_PUSH_ROWS = 8,
  /* the sparse row pull (glint_mat_pull_rows_sparse*): its emit kernel, and under the same id its
   * count kernel and the launches of its scan, so the sum is the pull's whole device time */
  GLINT_K_PULL_ROWS_SPARSE = 9,
  /* the grouped row-sum pull (glint_mat_pull_rows_sum*) and the weighted one (glint_mat_pull_rows_wsum*): one
   * launch per call */
  GLINT_K_PULL_ROWS_SUM = 10,
  /* the row dot-product pull (glint_mat_pull_rows_dot*): one launch per call. Also every launch of a top-k
   * pull (glint_mat_pull_topk*), which is a dot pull over every row plus a selection: its scores launch
   * and one launch per selection level, so the sum is that pull's whole device time. Also the one launch
   * of a row-pair dot pull (glint_mat_pull_pairs_dot*), recorded on its first shard only, and the one launch
   * of a grouped row-dot pull (glint_mat_pull_rows_gdot*) */
  GLINT_K_PULL_ROWS_DOT = 11,
  /* the fold of a row axpy push (glint_mat_push_rows_axpy*): one launch per non-empty call. Also the fold
   * of a row-pair axpy push (glint_mat_push_pairs_axpy*), recorded on its destination shard only */
  GLINT_K_PUSH_ROWS_AXPY = 12,
  GLINT_K_COUNT = 13
};
int glint_prof_enable(glint_shard_t shard, int on);
int glint_prof_read(glint_shard_t shard, int kernel_id, double* total_ms, int64_t* launches);
/* The device time of every launch of one kind since the last reset, in launch order: the first
 * min(cap, *launches) of them are written to ms (a call that launches several kernels under one id, as a
 * top-k pull does, is told apart launch by launch). */
int glint_prof_read_launches(glint_shard_t shard, int kernel_id, double* ms, int64_t cap, int64_t* launches);
int glint_prof_reset(glint_shard_t shard);

/* ---- misc ---------------------------------------------------------------------------------- */
const char* glint_strerror(int status);
/* Number of visible devices (0 without a GPU; never fails). */
int glint_device_count(void);
/* Library version (major*10000 + minor*100 + patch). */
int glint_version(void);
/* The library reads its GLINT_* environment overrides (tuning and test knobs) once and caches them;
 * this makes the next call re-read them (tests that change the environment between calls). */
int glint_reload_env(void);

/* Pinned, device-mapped host memory for the buffers a server answers from (the response images it
 * sends). A message-sized pull (glint_pull_async, glint_pull_wire_async) whose answer destination
 * lies in such a buffer, is aligned to the value size and is at least a page (GLINT_DIRECT_MIN_BYTES,
 * default 4096) is answered by the kernel straight into it: no copy out of the ring slot when the
 * entry retires. Free with glint_host_free: it returns GLINT_EINVAL (and frees nothing) while a pull
 * enqueued to answer into the buffer has not retired (glint_shard_wait for its ticket first). */
int glint_host_alloc(size_t bytes, void** host_ptr);
int glint_host_free(void* host_ptr);

/* The glint_push_flags this library implements (a client built against a newer header checks
 * before relying on a flag an older library would ignore, e.g. GLINT_PUSH_VALIDATE). */
int glint_push_flags_supported(void);

#ifdef __cplusplus
}
#endif
#endif /* GLINT_GPU_H */
