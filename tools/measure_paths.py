"""Measures every push/pull path of the plane on one MI355X (besides bench.py's headline):
device-resident rates from HIP events around each kernel (glint_prof_*), and host-pointer
("end-to-end": pageable host memory -> H2D -> kernels -> D2H) rates by wall clock, which is what
the JNI shim sees. One JSON line per measurement on stdout.

    python tools/measure_paths.py [--quick] [--sparse] [--rowsum] [--dot] [--axpy [--out FILE]] [--topk [--out FILE]]
                                  [--adagrad [--out FILE]] [--pairs [--out FILE]] [--init [--out FILE]]
                                  [--groups [--out FILE]] [--adam [--out FILE]] [--sampler [--out FILE]]
                                  [--rowwise [--out FILE]] [--ftrl [--out FILE]] [--wbag [--out FILE]]

--sparse runs only the sparse-row-pull leg (dense getRows against getRowsSparse on a cfg5 shard).
--rowsum runs only the grouped row-sum leg (getRowsSum against a dense row pull plus a reduction by the
caller, on a cfg5 shard).
--dot runs only the row dot-product leg (getRowsDot against a dense row pull plus a matrix product by the
caller, on a cfg5 shard).
--axpy runs only the row axpy push leg (updateRowsAxpy against coef @ x by the caller plus a row push, on
cfg5 shards) and appends its lines to profiles/axpy/axpy_push.jsonl (or FILE).
--topk runs only the top-k pull leg (getTopK against a dot pull over every row plus a selection by the
caller, on a cfg5 shard) and appends its lines to profiles/topk/topk_pull.jsonl (or FILE).
--adagrad runs only the Adagrad row push leg (updateRowsAdagrad against coalescing, two row pulls, the step
and two row pushes by the caller, on cfg5 shards) and appends its lines to profiles/adagrad/adagrad_push.jsonl
(or FILE).
--pairs runs only the row-pair leg (getPairsDot / updatePairsAxpy between two shards against row pulls, the
arithmetic by the caller and a row push, on cfg5-shaped Double and word2vec-shaped Float shards) and appends
its lines to profiles/pairs/pairs.jsonl (or FILE).
--init runs only the shard fill / uniform init leg (fill and initUniform of a whole shard and of a row list
against glint_shard_zero's memset, and against generating the table by the caller plus a row push, on a
cfg5-shaped Double and a word2vec-shaped Float shard) and appends its lines to profiles/init/init.jsonl (or
FILE).
--groups runs only the grouped row push leg (updateRowsGrouped against expanding the value rows by the caller
plus a row push, on a word2vec-shaped Float and a cfg5-shaped Double shard) and appends its lines to
profiles/groups/groups.jsonl (or FILE).
--adam runs only the Adam row push leg (updateRowsAdam against coalescing, row pulls of weights and moments,
the step and two row pushes by the caller, on cfg5 shards, with the Adagrad fold on the same rows beside it)
and appends its lines to profiles/adam/adam_push.jsonl (or FILE).
--rowwise runs only the row-wise Adagrad row push leg (updateRowsAdagradRowwise against coalescing, the mean of
squares, pulls of weight rows and accumulators, the step and two pushes by the caller, on a cfg5 weights shard
and an accumulator vector, with the Adagrad fold on the same rows beside it) and appends its lines to
profiles/rowwise_adagrad/rowwise_push.jsonl (or FILE).
--ftrl runs only the FTRL-proximal row push leg (updateRowsFtrl against coalescing, row pulls of weights and
state, the step and two row pushes by the caller, on cfg5 shards, with the Adam fold on the same rows beside
it) and appends its lines to profiles/ftrl/ftrl_push.jsonl (or FILE).
--wbag runs only the weighted-bag pull leg (the weighted row-sum pull and the grouped row-dot pull against a
dense row pull plus the arithmetic by the caller, and against their unchanged neighbour kernels, on a cfg5
shard) and appends its lines to profiles/wbag/wbag_pull.jsonl (or FILE).
--sampler runs only the row sampler leg (glint_sampler_draw_dev against torch.rand plus torch.searchsorted over a
device cdf, at m = 2^20 Zipf counts and n = 2^24 draws, with and without exclusion; the creates and the host
draw by wall clock) and appends its lines to profiles/sampler/sampler.jsonl (or FILE).
"""
import ctypes as C
import json
import os
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import glint_amd  # noqa: E402
from glint_amd import _native as N  # noqa: E402

QUICK = "--quick" in sys.argv
dev = torch.device("cuda", 0)
lib = N.load()
stream = torch.cuda.current_stream(dev).cuda_stream


def kernel_ms(h, kid):
    ms, cnt = C.c_double(), C.c_int64()
    lib.glint_prof_read(h, kid, C.byref(ms), C.byref(cnt))
    return ms.value / max(cnt.value, 1)


def timed(fn, reps, h):
    fn()
    torch.cuda.synchronize()
    lib.glint_prof_reset(h)
    lib.glint_prof_enable(h, 1)
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    dt = (time.perf_counter() - t0) / reps
    lib.glint_prof_enable(h, 0)
    return dt


def kernel_total_ms(h, kid):
    ms, cnt = C.c_double(), C.c_int64()
    lib.glint_prof_read(h, kid, C.byref(ms), C.byref(cnt))
    return ms.value, cnt.value


def wall(fn, reps):
    fn()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    return (time.perf_counter() - t0) / reps


def dev_ms(fn, reps=10):
    """Mean device time of fn: HIP events around `reps` calls, after one warm-up."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / reps


def emit(**kw):
    print(json.dumps(kw), flush=True)


def zipf_keys(rng, n_keys, n, s):
    """Zipf(s) ranks over [0, n_keys) mapped through a seeded permutation (hot keys scattered).
    s > 1: numpy's sampler, truncated; s == 1: inverse-CDF of the 1/k law, k ~ n_keys^u."""
    if s > 1.0:
        ranks = rng.zipf(s, size=int(n * 1.4))
        ranks = ranks[ranks <= n_keys][:n] - 1
    else:
        ranks = np.minimum(np.floor(np.power(float(n_keys), rng.random(n))).astype(np.int64) - 1, n_keys - 1)
    perm = rng.permutation(n_keys)
    return perm[ranks].astype(np.int64)


def sparse_leg(rng):
    """cfg5 per GPU: a 2^17 x 512 Double shard, 2^14 Zipf(1.0) rows, at element densities 1 %, 10 %
    and 100 %. Host: glint_mat_pull_rows against glint_mat_pull_rows_sparse, wall time and the bytes
    copied back. Device: kernel time (glint_prof) of the dense row pull against the sparse pull's
    count + scan + emit (all under GLINT_K_PULL_ROWS_SPARSE)."""
    shard_rows, cols, n = 1 << 17, 512, 1 << 14
    msh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, shard_rows), cols, "double", 0)
    h = msh.handle
    rows = zipf_keys(rng, shard_rows, n, 1.0)
    qr = torch.from_numpy(rows).to(dev)
    dense_out = np.empty((n, cols), np.float64)
    ptr = np.empty(n + 1, np.int64)
    # room for every element: only the pages the answer lands in are touched
    ocols, ovals = np.empty(n * cols, np.int32), np.empty(n * cols, np.float64)
    nnz = C.c_int64()
    d_dense = torch.empty((n, cols), dtype=torch.float64, device=dev)
    d_ptr = torch.empty(n + 1, dtype=torch.int64, device=dev)
    for density in (0.01, 0.1, 0.5, 0.7, 1.0):  # 0.5 and 0.7 bracket the host crossover
        msh.zero()
        gen = torch.Generator(device=dev)
        gen.manual_seed(int(density * 1000))
        for r0 in range(0, shard_rows, 1 << 14):  # fill in slices: the triplets of a slice fit easily
            mask = torch.rand((1 << 14, cols), device=dev, generator=gen) < density
            rr, cc = mask.nonzero(as_tuple=True)
            vv = torch.rand(rr.numel(), dtype=torch.float64, device=dev, generator=gen) + 0.5
            msh.update((rr + r0).contiguous(), cc.to(torch.int32).contiguous(), vv)
        del mask, rr, cc, vv
        reps = 5
        t_dense = wall(lambda: lib.glint_mat_pull_rows(h, rows.ctypes.data, dense_out.ctypes.data, n), reps)
        t_sparse = wall(lambda: lib.glint_mat_pull_rows_sparse(h, rows.ctypes.data, n, ptr.ctypes.data,
                                                               ocols.ctypes.data, ovals.ctypes.data, n * cols,
                                                               C.byref(nnz)), reps)
        # the Python methods allocate their answers per call: fresh pages, faulted in by the copies
        t_dense_py = wall(lambda: msh.getRows(rows), reps)
        t_sparse_py = wall(lambda: msh.getRowsSparse(rows), reps)
        k = nnz.value
        assert k == int((dense_out != 0).sum())
        # device-resident: one dense row pull against one sparse pull with an exact cap
        d_cols = torch.empty(k, dtype=torch.int32, device=dev)
        d_vals = torch.empty(k, dtype=torch.float64, device=dev)
        timed(lambda: lib.glint_mat_pull_rows_dev(h, qr.data_ptr(), d_dense.data_ptr(), n, stream), 10, h)
        k_dense = kernel_ms(h, N.GLINT_K_MAT_PULL_ROWS)
        timed(lambda: lib.glint_mat_pull_rows_sparse_dev(h, qr.data_ptr(), n, d_ptr.data_ptr(), d_cols.data_ptr(),
                                                         d_vals.data_ptr(), k, stream), 10, h)
        ms_total, launches = kernel_total_ms(h, N.GLINT_K_PULL_ROWS_SPARSE)
        emit(op="mat_pull_rows_sparse", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n, density=density,
             nnz=k, measured_density=k / (n * cols),
             host_dense_ms=t_dense * 1e3, host_sparse_ms=t_sparse * 1e3, host_speedup=t_dense / t_sparse,
             getRows_ms=t_dense_py * 1e3, getRowsSparse_ms=t_sparse_py * 1e3,
             host_dense_bytes_back=n * cols * 8, host_sparse_bytes_back=(n + 1) * 8 + k * 12,
             dev_dense_kernel_ms=k_dense, dev_sparse_kernels_ms=ms_total / 10, dev_sparse_launches_per_pull=launches / 10,
             note="host_*: the C calls into reused pageable numpy buffers, synchronous, mean of 5; getRows*: the "
                  "Python methods, fresh arrays per call (getRowsSparse = a count-only call + the pull); device: HIP-event kernel time, mean of 10; "
                  "the sparse figure sums count + scan + emit")
        del d_cols, d_vals
    msh.destroy()


def rowsum_leg(rng):
    """cfg5 per GPU: a 2^17 x 512 Double shard, 2^14 Zipf(1.0) rows in groups of 1, 16 and 128 rows, and
    as one group of all of them (the known limit: one dependent chain per column slice). Host:
    glint_mat_pull_rows_sum against glint_mat_pull_rows into a reused buffer + np.add.reduceat, wall time.
    Device: glint_mat_pull_rows_sum_dev against glint_mat_pull_rows_dev into an n x cols buffer +
    torch.index_add_ into g x cols, HIP events around each call. The baselines never run the code under
    test."""
    shard_rows, cols, n = 1 << 17, 512, 1 << 14
    msh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, shard_rows), cols, "double", 0)
    h = msh.handle
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)
    for r0 in range(0, shard_rows, 1 << 14):  # fill in slices of whole rows
        vv = torch.rand((1 << 14, cols), dtype=torch.float64, device=dev, generator=gen) + 0.5
        msh.updateRows(all_rows[r0:r0 + (1 << 14)].contiguous(), vv)
    del vv
    rows = zipf_keys(rng, shard_rows, n, 1.0)
    qr = torch.from_numpy(rows).to(dev)
    dense_out = np.empty((n, cols), np.float64)
    d_dense = torch.empty((n, cols), dtype=torch.float64, device=dev)

    for glen in (1, 16, 128, n):
        g = n // glen
        offsets = np.arange(g + 1, dtype=np.int64) * glen
        d_off = torch.from_numpy(offsets).to(dev)
        group = torch.arange(g, dtype=torch.int64, device=dev).repeat_interleave(glen)
        sum_out = np.empty((g, cols), np.float64)
        base_out = np.empty((g, cols), np.float64)
        d_sum = torch.empty((g, cols), dtype=torch.float64, device=dev)
        d_base = torch.empty((g, cols), dtype=torch.float64, device=dev)
        reps = 5

        def host_base():
            assert lib.glint_mat_pull_rows(h, rows.ctypes.data, dense_out.ctypes.data, n) == 0
            np.add.reduceat(dense_out, offsets[:-1], axis=0, out=base_out)

        def host_sum():
            assert lib.glint_mat_pull_rows_sum(h, rows.ctypes.data, n, offsets.ctypes.data, g, sum_out.ctypes.data) == 0

        def dev_base():
            lib.glint_mat_pull_rows_dev(h, qr.data_ptr(), d_dense.data_ptr(), n, stream)
            d_base.zero_()
            d_base.index_add_(0, group, d_dense)

        def dev_sum():
            lib.glint_mat_pull_rows_sum_dev(h, qr.data_ptr(), n, d_off.data_ptr(), g, d_sum.data_ptr(), stream)

        t_base = wall(host_base, reps)
        t_pull_only = wall(lambda: lib.glint_mat_pull_rows(h, rows.ctypes.data, dense_out.ctypes.data, n), reps)
        t_sum = wall(host_sum, reps)
        ms_base = dev_ms(dev_base)
        ms_pull_only = dev_ms(lambda: lib.glint_mat_pull_rows_dev(h, qr.data_ptr(), d_dense.data_ptr(), n, stream))
        ms_sum = dev_ms(dev_sum)
        timed(dev_sum, 10, h)
        k_sum = kernel_ms(h, N.GLINT_K_PULL_ROWS_SUM)
        msh.sync(stream)
        # the two answers agree up to the order of the additions (reduceat and index_add_ choose their own)
        err_host = float(np.max(np.abs(sum_out - base_out) / np.abs(base_out)))
        err_dev = float(torch.max(torch.abs(d_sum - d_base) / torch.abs(d_base)).item())
        same = bool(np.array_equal(d_sum.cpu().numpy(), sum_out))
        emit(op="mat_pull_rows_sum", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n, group_len=glen, groups=g,
             host_baseline_ms=t_base * 1e3, host_baseline_pull_only_ms=t_pull_only * 1e3, host_sum_ms=t_sum * 1e3,
             host_speedup=t_base / t_sum, host_baseline_bytes_back=n * cols * 8, host_sum_bytes_back=g * cols * 8,
             dev_baseline_ms=ms_base, dev_baseline_pull_only_ms=ms_pull_only, dev_sum_ms=ms_sum,
             dev_speedup=ms_base / ms_sum, dev_sum_kernel_ms=k_sum,
             max_rel_diff_host=err_host, max_rel_diff_dev=err_dev, host_and_device_sums_identical=same,
             note="host_*: C calls into reused pageable numpy buffers, synchronous, mean of 5; baseline = "
                  "glint_mat_pull_rows + np.add.reduceat. dev_*: HIP events around 10 calls, mean; baseline = "
                  "glint_mat_pull_rows_dev + zero_ + torch.index_add_. dev_sum_kernel_ms: the kernel alone (glint_prof)")
    msh.destroy()


def dot_leg(rng):
    """cfg5 per GPU: a 2^17 x 512 Double shard, 2^14 Zipf(1.0) rows against q = 1, 8 and 64 query vectors.
    Host: glint_mat_pull_rows_dot into a reused buffer against glint_mat_pull_rows into a reused buffer +
    rows @ x.T in numpy, wall time; the dense pull alone for scale. Device: glint_mat_pull_rows_dot_dev
    against glint_mat_pull_rows_dev + torch.matmul, HIP events around each call; the dot kernel alone by its
    prof id. The baselines never run the code under test; the answers are checked against them within
    1e-9 of each element's sum of |products|."""
    shard_rows, cols, n = 1 << 17, 512, 1 << 14
    msh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, shard_rows), cols, "double", 0)
    h = msh.handle
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)
    for r0 in range(0, shard_rows, 1 << 14):  # fill in slices of whole rows
        vv = torch.rand((1 << 14, cols), dtype=torch.float64, device=dev, generator=gen) - 0.5
        msh.updateRows(all_rows[r0:r0 + (1 << 14)].contiguous(), vv)
    del vv
    rows = zipf_keys(rng, shard_rows, n, 1.0)
    qr = torch.from_numpy(rows).to(dev)
    dense_out = np.empty((n, cols), np.float64)
    d_dense = torch.empty((n, cols), dtype=torch.float64, device=dev)

    for q in (1, 8, 64):
        x = rng.standard_normal((q, cols))
        d_x = torch.from_numpy(x).to(dev)
        dot_out = np.empty((n, q), np.float64)
        base_out = np.empty((n, q), np.float64)
        d_dot = torch.empty((n, q), dtype=torch.float64, device=dev)
        d_base = torch.empty((n, q), dtype=torch.float64, device=dev)
        d_xt = d_x.t()
        reps = 5

        def host_base():
            assert lib.glint_mat_pull_rows(h, rows.ctypes.data, dense_out.ctypes.data, n) == 0
            np.matmul(dense_out, x.T, out=base_out)

        def host_dot():
            assert lib.glint_mat_pull_rows_dot(h, rows.ctypes.data, n, x.ctypes.data, q, dot_out.ctypes.data) == 0

        def dev_base():
            lib.glint_mat_pull_rows_dev(h, qr.data_ptr(), d_dense.data_ptr(), n, stream)
            torch.matmul(d_dense, d_xt, out=d_base)

        def dev_dot():
            lib.glint_mat_pull_rows_dot_dev(h, qr.data_ptr(), n, d_x.data_ptr(), q, d_dot.data_ptr(), stream)

        t_base = wall(host_base, reps)
        t_pull_only = wall(lambda: lib.glint_mat_pull_rows(h, rows.ctypes.data, dense_out.ctypes.data, n), reps)
        t_dot = wall(host_dot, reps)
        ms_base = dev_ms(dev_base)
        ms_pull_only = dev_ms(lambda: lib.glint_mat_pull_rows_dev(h, qr.data_ptr(), d_dense.data_ptr(), n, stream))
        ms_dot = dev_ms(dev_dot)
        timed(dev_dot, 10, h)
        k_dot = kernel_ms(h, N.GLINT_K_PULL_ROWS_DOT)
        msh.sync(stream)
        # the answers agree up to the order of the additions: 1e-9 of each element's sum of |products|
        bound = 1e-9 * np.matmul(np.abs(dense_out), np.abs(x.T))
        d_dot_h = d_dot.cpu().numpy()
        ok_host = bool((np.abs(dot_out - base_out) <= bound).all())
        ok_dev = bool((np.abs(d_dot_h - d_base.cpu().numpy()) <= bound).all())
        assert ok_host and ok_dev
        emit(op="mat_pull_rows_dot", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n, queries=q,
             host_baseline_ms=t_base * 1e3, host_baseline_pull_only_ms=t_pull_only * 1e3, host_dot_ms=t_dot * 1e3,
             host_speedup=t_base / t_dot, host_speedup_over_pull_only=t_pull_only / t_dot,
             host_baseline_bytes_up=n * 8, host_baseline_bytes_back=n * cols * 8,
             host_dot_bytes_up=n * 8 + q * cols * 8, host_dot_bytes_back=n * q * 8,
             dev_baseline_ms=ms_base, dev_baseline_pull_only_ms=ms_pull_only, dev_dot_ms=ms_dot,
             dev_speedup=ms_base / ms_dot, dev_dot_kernel_ms=k_dot,
             dev_dot_row_bytes_read=n * cols * 8, dev_baseline_bytes=3 * n * cols * 8,
             within_bound_host=ok_host, within_bound_dev=ok_dev,
             host_and_device_dots_identical=bool(np.array_equal(d_dot_h, dot_out)),
             note="host_*: C calls into reused pageable numpy buffers, synchronous, mean of 5; baseline = "
                  "glint_mat_pull_rows + np.matmul(rows, x.T). dev_*: HIP events around 10 calls, mean; baseline = "
                  "glint_mat_pull_rows_dev + torch.matmul (n x cols read, written and read again). "
                  "dev_dot_kernel_ms: the kernel alone (glint_prof)")
    msh.destroy()


def axpy_leg(rng, out_path):
    """cfg5 per GPU: a 2^17 x 512 Double shard, 2^14 Zipf(1.0) rows, q = 1, 8 and 64 vectors. The leg under
    test pushes into one shard, its baseline into another, on alternating rounds of one process.
    Host: glint_mat_push_rows_axpy against coef @ x in numpy + glint_mat_push_rows, wall time; the
    baseline's push alone on pre-expanded values (into a third shard) for scale; the bytes staged.
    Device: glint_mat_push_rows_axpy_dev, default and deterministic, against torch.matmul +
    glint_mat_push_rows_dev with the same flags, a HIP event pair around each call; the fold kernel alone
    by its prof id. The baselines never run the code under test; after each q the two shards are compared
    within 1e-9 of each element's sum of |contributions| so far. One JSON line per q, also appended to
    out_path."""
    shard_rows, cols, n, rounds = 1 << 17, 512, 1 << 14, 5
    part = glint_amd.RangePartition(0, 0, shard_rows)
    sh_a, sh_b, sh_c = (glint_amd.PartialMatrix(part, cols, "double", 0) for _ in range(3))
    ha, hb, hc = sh_a.handle, sh_b.handle, sh_c.handle
    rows = zipf_keys(rng, shard_rows, n, 1.0)
    d_rows = torch.from_numpy(rows).to(dev)
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)
    mag = torch.zeros((shard_rows, cols), dtype=torch.float64, device=dev)
    vals = np.empty((n, cols), np.float64)
    d_vals = torch.empty((n, cols), dtype=torch.float64, device=dev)
    DET = N.GLINT_PUSH_DETERMINISTIC

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for q in (1, 8, 64):
        coef = rng.standard_normal((n, q))
        x = rng.standard_normal((q, cols))
        d_coef, d_x = torch.from_numpy(coef).to(dev), torch.from_numpy(x).to(dev)

        def host_axpy():
            assert lib.glint_mat_push_rows_axpy(ha, rows.ctypes.data, n, coef.ctypes.data, x.ctypes.data, q, 0) == 0

        def host_base():
            np.matmul(coef, x, out=vals)
            assert lib.glint_mat_push_rows(hb, rows.ctypes.data, vals.ctypes.data, n, 0) == 0

        def host_push_only():
            assert lib.glint_mat_push_rows(hc, rows.ctypes.data, vals.ctypes.data, n, 0) == 0

        def dev_axpy(flags):
            assert lib.glint_mat_push_rows_axpy_dev(ha, d_rows.data_ptr(), n, d_coef.data_ptr(), d_x.data_ptr(), q,
                                                    flags, stream) == 0

        def dev_base(flags):
            torch.matmul(d_coef, d_x, out=d_vals)
            assert lib.glint_mat_push_rows_dev(hb, d_rows.data_ptr(), d_vals.data_ptr(), n, flags, stream) == 0

        t = {k: [] for k in ("host_axpy", "host_base", "host_push_only", "dev_axpy", "dev_base", "dev_axpy_det",
                             "dev_base_det")}
        pushes = 0
        for rnd in range(rounds + 1):  # round 0 warms up; the two legs alternate inside every round
            got = {"host_base": wall_ms(host_base), "host_axpy": wall_ms(host_axpy),
                   "host_push_only": wall_ms(host_push_only)}
            torch.cuda.synchronize()
            got["dev_base"] = ev_ms(lambda: dev_base(0))
            got["dev_axpy"] = ev_ms(lambda: dev_axpy(0))
            got["dev_base_det"] = ev_ms(lambda: dev_base(DET))
            got["dev_axpy_det"] = ev_ms(lambda: dev_axpy(DET))
            pushes += 3
            if rnd:
                for k, v in got.items():
                    t[k].append(v)
        kern = {}
        for name, flags in (("default", 0), ("det", DET)):  # the fold alone, mirrored on the baseline's shard
            lib.glint_prof_reset(ha)
            lib.glint_prof_enable(ha, 1)
            for _ in range(3):
                dev_axpy(flags)
                dev_base(flags)
            torch.cuda.synchronize()
            kern[name] = kernel_ms(ha, N.GLINT_K_PUSH_ROWS_AXPY)
            lib.glint_prof_enable(ha, 0)
            pushes += 3
        sh_a.sync(stream)
        sh_b.sync(stream)
        mag.index_add_(0, d_rows, torch.matmul(d_coef.abs(), d_x.abs()), alpha=float(pushes))
        diff = (sh_a.getRows(all_rows) - sh_b.getRows(all_rows)).abs()
        ok = bool((diff <= 1e-9 * mag).all().item())
        worst = float((diff / mag.clamp_min(1e-300)).max().item())
        del diff
        assert ok, worst
        m = {k: stats(v) for k, v in t.items()}
        line = dict(
            op="mat_push_rows_axpy", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n, vectors=q,
            distinct_rows=int(np.unique(rows).size), rounds=rounds,
            host_axpy_ms=m["host_axpy"], host_baseline_ms=m["host_base"],
            host_baseline_push_only_ms=m["host_push_only"],
            host_speedup=m["host_base"]["mean"] / m["host_axpy"]["mean"],
            host_speedup_over_push_only=m["host_push_only"]["mean"] / m["host_axpy"]["mean"],
            host_axpy_bytes_staged=n * 8 + n * q * 8 + q * cols * 8, host_baseline_bytes_staged=n * 8 + n * cols * 8,
            dev_axpy_ms=m["dev_axpy"], dev_baseline_ms=m["dev_base"],
            dev_speedup=m["dev_base"]["mean"] / m["dev_axpy"]["mean"],
            dev_axpy_det_ms=m["dev_axpy_det"], dev_baseline_det_ms=m["dev_base_det"],
            dev_det_speedup=m["dev_base_det"]["mean"] / m["dev_axpy_det"]["mean"],
            dev_axpy_kernel_ms=kern["default"], dev_axpy_det_kernel_ms=kern["det"],
            shards_within_bound=ok, worst_fraction_of_sum_abs=worst,
            note="host_*: C calls on pageable numpy arrays, synchronous, wall ms; baseline = np.matmul(coef, x) + "
                 "glint_mat_push_rows, push_only = that push alone on values already built. dev_*: one HIP event "
                 "pair per call; baseline = torch.matmul + glint_mat_push_rows_dev, same flags. Legs alternate "
                 "inside each of `rounds` rounds after one warm-up round. *_kernel_ms: the fold alone (glint_prof)")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    for sh in (sh_a, sh_b, sh_c):
        sh.destroy()


def adagrad_leg(rng, out_path):
    """cfg5 per GPU: two 2^17 x 512 Double shards (weights and accumulator), 2^14 and 2^16 Zipf(1.0) rows of
    gradients. The leg under test steps one pair of shards, its baseline another pair, on alternating
    rounds of one process.
    Device: glint_mat_push_rows_adagrad_dev against what a caller does today -- torch.unique + index_add_
    to coalesce, two glint_mat_pull_rows_dev, the elementwise step in torch, two glint_mat_push_rows_dev of
    deltas -- a HIP event pair around each; the fold kernel alone by its prof id, and its bytes (n x cols
    gradients plus a read and a write of distinct x cols in each shard) over that time as a fraction of the
    HBM peak. Host: glint_mat_push_rows_adagrad against the same done with numpy and the host calls, wall
    time. The baselines never run the code under test; after each n the two pairs are compared (the
    baseline sums in another order and adds deltas, so they agree to rounding, not bit for bit). One JSON
    line per n, also appended to out_path."""
    shard_rows, cols, rounds = 1 << 17, 512, 5
    lr, eps, hbm_peak_gbs = 0.05, 1e-8, 8000.0
    part = glint_amd.RangePartition(0, 0, shard_rows)
    wa, sa, wb, sb = (glint_amd.PartialMatrix(part, cols, "double", 0) for _ in range(4))
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for n in (1 << 14, 1 << 16):
        rows = zipf_keys(rng, shard_rows, n, 1.0)
        g = rng.standard_normal((n, cols))
        d_rows, d_g = torch.from_numpy(rows).to(dev), torch.from_numpy(g).to(dev)
        distinct = int(np.unique(rows).size)

        def dev_adagrad():
            assert lib.glint_mat_push_rows_adagrad_dev(wa.handle, sa.handle, d_rows.data_ptr(), d_g.data_ptr(), n,
                                                       lr, eps, stream) == 0

        def dev_base():
            uniq, inv = torch.unique(d_rows, return_inverse=True)
            G = torch.zeros((uniq.numel(), cols), dtype=torch.float64, device=dev).index_add_(0, inv, d_g)
            w, h = torch.empty_like(G), torch.empty_like(G)
            assert lib.glint_mat_pull_rows_dev(wb.handle, uniq.data_ptr(), w.data_ptr(), uniq.numel(), stream) == 0
            assert lib.glint_mat_pull_rows_dev(sb.handle, uniq.data_ptr(), h.data_ptr(), uniq.numel(), stream) == 0
            s = G * G
            step = (lr * G) / (torch.sqrt(h + s) + eps)
            dw = -step
            assert lib.glint_mat_push_rows_dev(sb.handle, uniq.data_ptr(), s.data_ptr(), uniq.numel(), 0, stream) == 0
            assert lib.glint_mat_push_rows_dev(wb.handle, uniq.data_ptr(), dw.data_ptr(), uniq.numel(), 0, stream) == 0
            # (the temporaries are freed into torch's allocator, which reuses them on this stream only)

        def host_adagrad():
            assert lib.glint_mat_push_rows_adagrad(wa.handle, sa.handle, rows.ctypes.data, g.ctypes.data, n, lr,
                                                   eps) == 0

        def host_base():
            uniq, inv = np.unique(rows, return_inverse=True)
            G = np.zeros((uniq.size, cols))
            np.add.at(G, inv, g)
            w, h = np.empty_like(G), np.empty_like(G)
            assert lib.glint_mat_pull_rows(wb.handle, uniq.ctypes.data, w.ctypes.data, uniq.size) == 0
            assert lib.glint_mat_pull_rows(sb.handle, uniq.ctypes.data, h.ctypes.data, uniq.size) == 0
            s = G * G
            dw = -((lr * G) / (np.sqrt(h + s) + eps))
            assert lib.glint_mat_push_rows(sb.handle, uniq.ctypes.data, s.ctypes.data, uniq.size, 0) == 0
            assert lib.glint_mat_push_rows(wb.handle, uniq.ctypes.data, dw.ctypes.data, uniq.size, 0) == 0

        t = {k: [] for k in ("host_adagrad", "host_base", "dev_adagrad", "dev_base")}
        for rnd in range(rounds + 1):  # round 0 warms up; the two legs alternate inside every round
            got = {"host_base": wall_ms(host_base), "host_adagrad": wall_ms(host_adagrad)}
            torch.cuda.synchronize()
            got["dev_base"] = ev_ms(dev_base)
            got["dev_adagrad"] = ev_ms(dev_adagrad)
            if rnd:
                for k, v in got.items():
                    t[k].append(v)
        lib.glint_prof_reset(wa.handle)  # the fold alone, mirrored on the baseline's shards
        lib.glint_prof_enable(wa.handle, 1)
        for _ in range(3):
            dev_adagrad()
            dev_base()
        torch.cuda.synchronize()
        fold_ms = kernel_ms(wa.handle, N.GLINT_K_PUSH_ROWS)
        lib.glint_prof_enable(wa.handle, 0)
        for sh in (wa, sa, wb, sb):
            sh.sync(stream)
        dw = (wa.getRows(all_rows) - wb.getRows(all_rows)).abs().max().item()
        ha_, hb_ = sa.getRows(all_rows), sb.getRows(all_rows)
        dh = ((ha_ - hb_).abs() / hb_.abs().clamp_min(1e-300)).max().item()
        del ha_, hb_
        assert dw < 1e-6 and dh < 1e-9, (dw, dh)
        m = {k: stats(v) for k, v in t.items()}
        fold_bytes = (n * cols + 4 * distinct * cols) * 8
        line = dict(
            op="mat_push_rows_adagrad", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n,
            distinct_rows=distinct, rounds=rounds, lr=lr, eps=eps,
            host_adagrad_ms=m["host_adagrad"], host_baseline_ms=m["host_base"],
            host_speedup=m["host_base"]["mean"] / m["host_adagrad"]["mean"],
            host_adagrad_bytes_staged=n * 8 + n * cols * 8,
            host_baseline_bytes_over_link=2 * distinct * 8 + 4 * distinct * cols * 8,
            dev_adagrad_ms=m["dev_adagrad"], dev_baseline_ms=m["dev_base"],
            dev_speedup=m["dev_base"]["mean"] / m["dev_adagrad"]["mean"],
            fold_kernel_ms=fold_ms, fold_bytes=fold_bytes, fold_GBps=fold_bytes / (fold_ms * 1e-3) / 1e9,
            fold_fraction_of_hbm_peak=fold_bytes / (fold_ms * 1e-3) / 1e9 / hbm_peak_gbs, hbm_peak_GBps=hbm_peak_gbs,
            max_abs_weight_difference=dw, max_relative_state_difference=dh,
            note="host_*: C calls on pageable numpy arrays, synchronous, wall ms; baseline = np.unique + np.add.at, "
                 "two glint_mat_pull_rows, the step in numpy, two glint_mat_push_rows of deltas. dev_*: one HIP "
                 "event pair per call; baseline = torch.unique + index_add_, two glint_mat_pull_rows_dev, the step "
                 "in torch, two glint_mat_push_rows_dev. "
                 "Legs alternate inside each of `rounds` rounds after one warm-up round. fold_kernel_ms: the fold "
                 "alone (glint_prof, GLINT_K_PUSH_ROWS on the weights shard); fold_bytes = (rows + 4 * "
                 "distinct_rows) * cols * 8")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    for sh in (wa, sa, wb, sb):
        sh.destroy()


# The two Adam legs agree to rounding, not bit for bit: the baseline sums a row's gradients in another order
# and adds deltas. Largest disagreement measured over both sizes (DESIGN.md "Adam row push"), asserted at
# 100 x: absolute for the weights and the first moments, relative for the second moments.
ADAM_AGREE_MEASURED = {"w": 1.8e-12, "m": 3.5e-13, "v": 8.5e-11}
ADAM_AGREE_BOUND = {k: 100 * v for k, v in ADAM_AGREE_MEASURED.items()}


def adam_leg(rng, out_path):
    """The Adagrad leg's method and shapes with one more table: 2^17 x 512 Double weights and a 2^17 x 1024
    moments shard per pair, 2^14 and 2^16 Zipf(1.0) rows of gradients. The leg under test steps one pair of
    shards, its baseline another pair, on alternating rounds of one process; both pairs take the same
    steps with the same step numbers.
    Device: glint_mat_push_rows_adam_dev against what a caller does today -- torch.unique + index_add_ to
    coalesce, glint_mat_pull_rows_dev of the weights and of the moments, the step in torch, two
    glint_mat_push_rows_dev of deltas -- a HIP event pair around each; the fold kernel alone by its prof
    id, and its bytes (n x cols gradients plus a read and a write of distinct x 3 cols) over that time as a
    fraction of the HBM peak; beside it the Adagrad fold on the same rows, on a third pair. Host:
    glint_mat_push_rows_adam against the same done with numpy and the host calls, wall time. The baselines
    never run the code under test; after each n the two pairs are compared to ADAM_AGREE_BOUND. One JSON
    line per n, also appended to out_path."""
    shard_rows, cols, rounds = 1 << 17, 512, 5
    lr, b1, b2, eps, hbm_peak_gbs = 0.05, 0.9, 0.999, 1e-8, 8000.0
    part = glint_amd.RangePartition(0, 0, shard_rows)
    wa, wb, wg, hg = (glint_amd.PartialMatrix(part, cols, "double", 0) for _ in range(4))
    sa, sb = (glint_amd.PartialMatrix(part, 2 * cols, "double", 0) for _ in range(2))
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)
    steps = {"a": 0, "b": 0}  # the next call on a pair is step steps[pair] + 1

    def scalars(pair):
        steps[pair] += 1
        t = steps[pair]
        return t, lr / (1.0 - b1 ** t), (1.0 - b2 ** t) ** 0.5

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for n in (1 << 14, 1 << 16):
        rows = zipf_keys(rng, shard_rows, n, 1.0)
        g = rng.standard_normal((n, cols))
        d_rows, d_g = torch.from_numpy(rows).to(dev), torch.from_numpy(g).to(dev)
        distinct = int(np.unique(rows).size)

        def dev_adam():
            t, _, _ = scalars("a")
            assert lib.glint_mat_push_rows_adam_dev(wa.handle, sa.handle, d_rows.data_ptr(), d_g.data_ptr(), n, lr,
                                                    b1, b2, eps, t, stream) == 0

        def dev_base():
            _, alpha, rc2 = scalars("b")
            uniq, inv = torch.unique(d_rows, return_inverse=True)
            u = uniq.numel()
            G = torch.zeros((u, cols), dtype=torch.float64, device=dev).index_add_(0, inv, d_g)
            w = torch.empty_like(G)
            mv = torch.empty((u, 2 * cols), dtype=torch.float64, device=dev)
            assert lib.glint_mat_pull_rows_dev(wb.handle, uniq.data_ptr(), w.data_ptr(), u, stream) == 0
            assert lib.glint_mat_pull_rows_dev(sb.handle, uniq.data_ptr(), mv.data_ptr(), u, stream) == 0
            m2 = b1 * mv[:, :cols] + (1.0 - b1) * G
            v2 = b2 * mv[:, cols:] + (1.0 - b2) * (G * G)
            dw = -((alpha * m2) / (torch.sqrt(v2) / rc2 + eps))
            ds = torch.cat([m2, v2], 1) - mv
            assert lib.glint_mat_push_rows_dev(sb.handle, uniq.data_ptr(), ds.data_ptr(), u, 0, stream) == 0
            assert lib.glint_mat_push_rows_dev(wb.handle, uniq.data_ptr(), dw.data_ptr(), u, 0, stream) == 0
            # (the temporaries are freed into torch's allocator, which reuses them on this stream only)

        def host_adam():
            t, _, _ = scalars("a")
            assert lib.glint_mat_push_rows_adam(wa.handle, sa.handle, rows.ctypes.data, g.ctypes.data, n, lr, b1, b2,
                                                eps, t) == 0

        def host_base():
            _, alpha, rc2 = scalars("b")
            uniq, inv = np.unique(rows, return_inverse=True)
            G = np.zeros((uniq.size, cols))
            np.add.at(G, inv, g)
            w, mv = np.empty_like(G), np.empty((uniq.size, 2 * cols))
            assert lib.glint_mat_pull_rows(wb.handle, uniq.ctypes.data, w.ctypes.data, uniq.size) == 0
            assert lib.glint_mat_pull_rows(sb.handle, uniq.ctypes.data, mv.ctypes.data, uniq.size) == 0
            m2 = b1 * mv[:, :cols] + (1.0 - b1) * G
            v2 = b2 * mv[:, cols:] + (1.0 - b2) * (G * G)
            dw = -((alpha * m2) / (np.sqrt(v2) / rc2 + eps))
            ds = np.concatenate([m2, v2], 1) - mv
            assert lib.glint_mat_push_rows(sb.handle, uniq.ctypes.data, ds.ctypes.data, uniq.size, 0) == 0
            assert lib.glint_mat_push_rows(wb.handle, uniq.ctypes.data, dw.ctypes.data, uniq.size, 0) == 0

        t = {k: [] for k in ("host_adam", "host_base", "dev_adam", "dev_base")}
        for rnd in range(rounds + 1):  # round 0 warms up; the two legs alternate inside every round
            got = {"host_base": wall_ms(host_base), "host_adam": wall_ms(host_adam)}
            torch.cuda.synchronize()
            got["dev_base"] = ev_ms(dev_base)
            got["dev_adam"] = ev_ms(dev_adam)
            if rnd:
                for k, v in got.items():
                    t[k].append(v)
        assert steps["a"] == steps["b"]
        lib.glint_prof_reset(wa.handle)  # the fold alone, mirrored on the baseline's shards
        lib.glint_prof_enable(wa.handle, 1)
        for _ in range(3):
            dev_adam()
            dev_base()
        torch.cuda.synchronize()
        fold_ms = kernel_ms(wa.handle, N.GLINT_K_PUSH_ROWS)
        lib.glint_prof_enable(wa.handle, 0)
        lib.glint_prof_reset(wg.handle)  # the Adagrad fold on the same rows, for scale
        lib.glint_prof_enable(wg.handle, 1)
        for _ in range(4):
            assert lib.glint_mat_push_rows_adagrad_dev(wg.handle, hg.handle, d_rows.data_ptr(), d_g.data_ptr(), n, lr,
                                                       eps, stream) == 0
        torch.cuda.synchronize()
        adagrad_fold_ms = kernel_ms(wg.handle, N.GLINT_K_PUSH_ROWS)
        lib.glint_prof_enable(wg.handle, 0)
        for sh in (wa, sa, wb, sb, wg, hg):
            sh.sync(stream)
        dw = (wa.getRows(all_rows) - wb.getRows(all_rows)).abs().max().item()
        sa_, sb_ = sa.getRows(all_rows), sb.getRows(all_rows)
        dm = (sa_[:, :cols] - sb_[:, :cols]).abs().max().item()
        dv = ((sa_[:, cols:] - sb_[:, cols:]).abs() / sb_[:, cols:].abs().clamp_min(1e-300)).max().item()
        del sa_, sb_
        agree = {"w": dw, "m": dm, "v": dv}
        print(f"adam legs disagree by {agree}; bound {ADAM_AGREE_BOUND}", file=sys.stderr, flush=True)
        assert all(agree[k] <= ADAM_AGREE_BOUND[k] for k in agree), (agree, ADAM_AGREE_BOUND)
        m = {k: stats(v) for k, v in t.items()}
        fold_bytes = (n + 6 * distinct) * cols * 8
        line = dict(
            op="mat_push_rows_adam", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n,
            distinct_rows=distinct, rounds=rounds, lr=lr, beta1=b1, beta2=b2, eps=eps, steps_taken=steps["a"],
            host_adam_ms=m["host_adam"], host_baseline_ms=m["host_base"],
            host_speedup=m["host_base"]["mean"] / m["host_adam"]["mean"],
            host_adam_bytes_staged=n * 8 + n * cols * 8,
            host_baseline_bytes_over_link=2 * distinct * 8 + 6 * distinct * cols * 8,
            dev_adam_ms=m["dev_adam"], dev_baseline_ms=m["dev_base"],
            dev_speedup=m["dev_base"]["mean"] / m["dev_adam"]["mean"],
            fold_kernel_ms=fold_ms, fold_bytes=fold_bytes, fold_GBps=fold_bytes / (fold_ms * 1e-3) / 1e9,
            fold_fraction_of_hbm_peak=fold_bytes / (fold_ms * 1e-3) / 1e9 / hbm_peak_gbs, hbm_peak_GBps=hbm_peak_gbs,
            adagrad_fold_kernel_ms=adagrad_fold_ms, fold_over_adagrad_fold=fold_ms / adagrad_fold_ms,
            max_abs_weight_difference=dw, max_abs_m_difference=dm, max_relative_v_difference=dv,
            agreement_bound=ADAM_AGREE_BOUND,
            note="host_*: C calls on pageable numpy arrays, synchronous, wall ms; baseline = np.unique + np.add.at, "
                 "glint_mat_pull_rows of weights and moments, the step in numpy, two glint_mat_push_rows of deltas. "
                 "dev_*: one HIP event pair per call; baseline = torch.unique + index_add_, two "
                 "glint_mat_pull_rows_dev, the step in torch, two glint_mat_push_rows_dev. "
                 "Legs alternate inside each of `rounds` rounds after one warm-up round. fold_kernel_ms: the fold "
                 "alone (glint_prof, GLINT_K_PUSH_ROWS on the weights shard); fold_bytes = (rows + 6 * "
                 "distinct_rows) * cols * 8. adagrad_fold_kernel_ms: the Adagrad push's fold on the same rows and "
                 "gradients, on a pair of its own")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    for sh in (wa, sa, wb, sb, wg, hg):
        sh.destroy()


# The two FTRL legs agree to rounding, not bit for bit: the baseline sums a row's gradients in another order
# and adds deltas; w is continuous in z across the threshold, so agreement to rounding is meaningful. Largest
# disagreement measured over both sizes (DESIGN.md "FTRL row push"), asserted at 100 x: absolute for the
# weights and z, relative for n.
FTRL_AGREE_MEASURED = {"w": 1.9e-14, "z": 1.7e-11, "n": 6.8e-11}
FTRL_AGREE_BOUND = {k: 100 * v for k, v in FTRL_AGREE_MEASURED.items()}


def ftrl_leg(rng, out_path):
    """The Adam leg's method and shapes: 2^17 x 512 Double weights and a 2^17 x 1024 state shard (z, n) per
    pair, 2^14 and 2^16 Zipf(1.0) rows of standard-normal gradients, alpha = 0.05, beta = 1, l1 = 1e-3, l2 =
    1e-4. The leg under test steps one pair of shards, its baseline another pair, on alternating rounds of
    one process; both pairs take the same steps.
    Device: glint_mat_push_rows_ftrl_dev against what a caller does today -- torch.unique + index_add_ to
    coalesce, glint_mat_pull_rows_dev of the weights and of the state, the step in torch, two
    glint_mat_push_rows_dev of deltas -- a HIP event pair around each; the fold kernel alone by its prof
    id, and its bytes (n x cols gradients plus a read and a write of distinct x 3 cols) over that time as a
    fraction of the HBM peak; beside it the Adam fold on the same rows, on a third pair. Host:
    glint_mat_push_rows_ftrl against the same done with numpy and the host calls, wall time. The baselines
    never run the code under test; after each n the two pairs are compared to FTRL_AGREE_BOUND. One JSON
    line per n, also appended to out_path."""
    shard_rows, cols, rounds = 1 << 17, 512, 5
    alpha, beta, l1, l2, hbm_peak_gbs = 0.05, 1.0, 1e-3, 1e-4, 8000.0
    part = glint_amd.RangePartition(0, 0, shard_rows)
    wa, wb, wg = (glint_amd.PartialMatrix(part, cols, "double", 0) for _ in range(3))
    sa, sb, sg = (glint_amd.PartialMatrix(part, 2 * cols, "double", 0) for _ in range(3))
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)
    steps = {"a": 0, "b": 0, "g": 0}

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    def step(xp, w, zn, G):
        """(w' - w, [z', n'] - [z, n]) of the pulled rows, in the caller's own arithmetic (xp: torch or numpy)."""
        z, n = zn[:, :cols], zn[:, cols:]
        n2 = n + G * G
        r1 = xp.sqrt(n2)
        z2 = z + G - (r1 - xp.sqrt(n)) / alpha * w
        w2 = xp.where(xp.abs(z2) <= l1, xp.zeros_like(z2), -(z2 - xp.sign(z2) * l1) / ((beta + r1) / alpha + l2))
        return w2 - w, z2 - z, n2 - n

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for n in (1 << 14, 1 << 16):
        rows = zipf_keys(rng, shard_rows, n, 1.0)
        g = rng.standard_normal((n, cols))
        d_rows, d_g = torch.from_numpy(rows).to(dev), torch.from_numpy(g).to(dev)
        distinct = int(np.unique(rows).size)

        def dev_ftrl():
            steps["a"] += 1
            assert lib.glint_mat_push_rows_ftrl_dev(wa.handle, sa.handle, d_rows.data_ptr(), d_g.data_ptr(), n, alpha,
                                                    beta, l1, l2, stream) == 0

        def dev_base():
            steps["b"] += 1
            uniq, inv = torch.unique(d_rows, return_inverse=True)
            u = uniq.numel()
            G = torch.zeros((u, cols), dtype=torch.float64, device=dev).index_add_(0, inv, d_g)
            w = torch.empty_like(G)
            zn = torch.empty((u, 2 * cols), dtype=torch.float64, device=dev)
            assert lib.glint_mat_pull_rows_dev(wb.handle, uniq.data_ptr(), w.data_ptr(), u, stream) == 0
            assert lib.glint_mat_pull_rows_dev(sb.handle, uniq.data_ptr(), zn.data_ptr(), u, stream) == 0
            dw, dz, dn = step(torch, w, zn, G)
            ds = torch.cat([dz, dn], 1)
            assert lib.glint_mat_push_rows_dev(sb.handle, uniq.data_ptr(), ds.data_ptr(), u, 0, stream) == 0
            assert lib.glint_mat_push_rows_dev(wb.handle, uniq.data_ptr(), dw.data_ptr(), u, 0, stream) == 0
            # (the temporaries are freed into torch's allocator, which reuses them on this stream only)

        def host_ftrl():
            steps["a"] += 1
            assert lib.glint_mat_push_rows_ftrl(wa.handle, sa.handle, rows.ctypes.data, g.ctypes.data, n, alpha, beta,
                                                l1, l2) == 0

        def host_base():
            steps["b"] += 1
            uniq, inv = np.unique(rows, return_inverse=True)
            G = np.zeros((uniq.size, cols))
            np.add.at(G, inv, g)
            w, zn = np.empty_like(G), np.empty((uniq.size, 2 * cols))
            assert lib.glint_mat_pull_rows(wb.handle, uniq.ctypes.data, w.ctypes.data, uniq.size) == 0
            assert lib.glint_mat_pull_rows(sb.handle, uniq.ctypes.data, zn.ctypes.data, uniq.size) == 0
            dw, dz, dn = step(np, w, zn, G)
            ds = np.concatenate([dz, dn], 1)
            assert lib.glint_mat_push_rows(sb.handle, uniq.ctypes.data, ds.ctypes.data, uniq.size, 0) == 0
            assert lib.glint_mat_push_rows(wb.handle, uniq.ctypes.data, dw.ctypes.data, uniq.size, 0) == 0

        t = {k: [] for k in ("host_ftrl", "host_base", "dev_ftrl", "dev_base")}
        for rnd in range(rounds + 1):  # round 0 warms up; the two legs alternate inside every round
            got = {"host_base": wall_ms(host_base), "host_ftrl": wall_ms(host_ftrl)}
            torch.cuda.synchronize()
            got["dev_base"] = ev_ms(dev_base)
            got["dev_ftrl"] = ev_ms(dev_ftrl)
            if rnd:
                for k, v in got.items():
                    t[k].append(v)
        assert steps["a"] == steps["b"]
        lib.glint_prof_reset(wa.handle)  # the fold alone, mirrored on the baseline's shards
        lib.glint_prof_enable(wa.handle, 1)
        for _ in range(3):
            dev_ftrl()
            dev_base()
        torch.cuda.synchronize()
        fold_ms = kernel_ms(wa.handle, N.GLINT_K_PUSH_ROWS)
        lib.glint_prof_enable(wa.handle, 0)
        lib.glint_prof_reset(wg.handle)  # the Adam fold on the same rows, for scale
        lib.glint_prof_enable(wg.handle, 1)
        for _ in range(4):
            steps["g"] += 1
            assert lib.glint_mat_push_rows_adam_dev(wg.handle, sg.handle, d_rows.data_ptr(), d_g.data_ptr(), n, alpha,
                                                    0.9, 0.999, 1e-8, steps["g"], stream) == 0
        torch.cuda.synchronize()
        adam_fold_ms = kernel_ms(wg.handle, N.GLINT_K_PUSH_ROWS)
        lib.glint_prof_enable(wg.handle, 0)
        for sh in (wa, sa, wb, sb, wg, sg):
            sh.sync(stream)
        wa_, wb_ = wa.getRows(all_rows), wb.getRows(all_rows)
        dw = (wa_ - wb_).abs().max().item()
        named = (sa.getRows(all_rows)[:, cols:] != 0).any(1)  # a row that was stepped has n != 0
        touched = int(named.sum().item())
        zeros = {"call": int((wa_[named] == 0).sum().item()), "baseline": int((wb_[named] == 0).sum().item())}
        del wa_, wb_, named
        sa_, sb_ = sa.getRows(all_rows), sb.getRows(all_rows)
        dz = (sa_[:, :cols] - sb_[:, :cols]).abs().max().item()
        dn = ((sa_[:, cols:] - sb_[:, cols:]).abs() / sb_[:, cols:].abs().clamp_min(1e-300)).max().item()
        del sa_, sb_
        agree = {"w": dw, "z": dz, "n": dn}
        print(f"ftrl legs disagree by {agree}; bound {FTRL_AGREE_BOUND}", file=sys.stderr, flush=True)
        assert all(agree[k] <= FTRL_AGREE_BOUND[k] for k in agree), (agree, FTRL_AGREE_BOUND)
        m = {k: stats(v) for k, v in t.items()}
        fold_bytes = (n + 6 * distinct) * cols * 8
        line = dict(
            op="mat_push_rows_ftrl", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n,
            distinct_rows=distinct, rounds=rounds, alpha=alpha, beta=beta, l1=l1, l2=l2, steps_taken=steps["a"],
            host_ftrl_ms=m["host_ftrl"], host_baseline_ms=m["host_base"],
            host_speedup=m["host_base"]["mean"] / m["host_ftrl"]["mean"],
            host_ftrl_bytes_staged=n * 8 + n * cols * 8,
            host_baseline_bytes_over_link=2 * distinct * 8 + 6 * distinct * cols * 8,
            dev_ftrl_ms=m["dev_ftrl"], dev_baseline_ms=m["dev_base"],
            dev_speedup=m["dev_base"]["mean"] / m["dev_ftrl"]["mean"],
            fold_kernel_ms=fold_ms, fold_bytes=fold_bytes, fold_GBps=fold_bytes / (fold_ms * 1e-3) / 1e9,
            fold_fraction_of_hbm_peak=fold_bytes / (fold_ms * 1e-3) / 1e9 / hbm_peak_gbs, hbm_peak_GBps=hbm_peak_gbs,
            adam_fold_kernel_ms=adam_fold_ms, fold_over_adam_fold=fold_ms / adam_fold_ms,
            max_abs_weight_difference=dw, max_abs_z_difference=dz, max_relative_n_difference=dn,
            agreement_bound=FTRL_AGREE_BOUND, exact_zero_weights_in_touched_rows=zeros,
            touched_rows=touched,
            note="host_*: C calls on pageable numpy arrays, synchronous, wall ms; baseline = np.unique + np.add.at, "
                 "glint_mat_pull_rows of weights and state, the step in numpy, two glint_mat_push_rows of deltas. "
                 "dev_*: one HIP event pair per call; baseline = torch.unique + index_add_, two "
                 "glint_mat_pull_rows_dev, the step in torch, two glint_mat_push_rows_dev. "
                 "Legs alternate inside each of `rounds` rounds after one warm-up round. fold_kernel_ms: the fold "
                 "alone (glint_prof, GLINT_K_PUSH_ROWS on the weights shard); fold_bytes = (rows + 6 * "
                 "distinct_rows) * cols * 8. adam_fold_kernel_ms: the Adam push's fold on the same rows and "
                 "gradients, on a pair of its own. exact_zero_weights_in_touched_rows counts w == 0 in the rows "
                 "that were ever named (touched_rows: n != 0), of touched_rows * cols weights")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    for sh in (wa, sa, wb, sb, wg, sg):
        sh.destroy()


# The two row-wise Adagrad legs agree to rounding, not bit for bit: the baseline sums a row's gradients and
# their squares in another order and adds deltas. The bound comes from the format, not from a run: a sum of m
# doubles in another order moves by at most about m * 2^-53 of the sum of magnitudes, m is under 10^4 here and
# a weight or an accumulator takes under 100 such steps of order 1, which gives 1e-10; asserted at 10 x that,
# absolute for the weights and relative for the accumulators.
ROWWISE_AGREE_BOUND = {"w": 1e-9, "h": 1e-9}


def rowwise_leg(rng, out_path):
    """The Adagrad leg's method and shapes with a vector for the state: 2^17 x 512 Double weights and a 2^17
    Double accumulator vector per pair, 2^14 and 2^16 Zipf(1.0) rows of gradients. The leg under test steps
    one pair of shards, its baseline another pair, on alternating rounds of one process.
    Device: glint_mat_push_rows_adagrad_rowwise_dev against what a caller does today -- torch.unique +
    index_add_ to coalesce, the mean of squares, glint_mat_pull_rows_dev of the weights and glint_vec_pull_dev
    of the accumulators, the step in torch, a glint_vec_push_dev and a glint_mat_push_rows_dev of deltas -- a
    HIP event pair around each; the fold kernel alone by its prof id, and its bytes (two reads of n x cols
    gradients at most, plus a read and a write of distinct x cols weights) over that time; beside it the
    Adagrad row push's fold on the same rows and gradients, on a third pair. Host:
    glint_mat_push_rows_adagrad_rowwise against the same done with numpy and the host calls, wall time. The
    baselines never run the code under test; after each n the two pairs are compared to ROWWISE_AGREE_BOUND.
    One JSON line per n, also appended to out_path."""
    shard_rows, cols, rounds = 1 << 17, 512, 5
    lr, eps, hbm_peak_gbs = 0.05, 1e-8, 8000.0
    part = glint_amd.RangePartition(0, 0, shard_rows)
    wa, wb, wg, hg = (glint_amd.PartialMatrix(part, cols, "double", 0) for _ in range(4))
    sa, sb = (glint_amd.PartialVector(part, "double", 0) for _ in range(2))
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for n in (1 << 14, 1 << 16):
        rows = zipf_keys(rng, shard_rows, n, 1.0)
        g = rng.standard_normal((n, cols))
        d_rows, d_g = torch.from_numpy(rows).to(dev), torch.from_numpy(g).to(dev)
        uniq_np, counts = np.unique(rows, return_counts=True)
        distinct, longest = int(uniq_np.size), int(counts.max())

        def dev_rowwise():
            assert lib.glint_mat_push_rows_adagrad_rowwise_dev(wa.handle, sa.handle, d_rows.data_ptr(),
                                                               d_g.data_ptr(), n, lr, eps, stream) == 0

        def dev_base():
            uniq, inv = torch.unique(d_rows, return_inverse=True)
            u = uniq.numel()
            G = torch.zeros((u, cols), dtype=torch.float64, device=dev).index_add_(0, inv, d_g)
            w = torch.empty_like(G)
            h = torch.empty(u, dtype=torch.float64, device=dev)
            assert lib.glint_mat_pull_rows_dev(wb.handle, uniq.data_ptr(), w.data_ptr(), u, stream) == 0
            assert lib.glint_vec_pull_dev(sb.handle, uniq.data_ptr(), h.data_ptr(), u, stream) == 0
            s = (G * G).mean(1)
            dw = -((lr / (torch.sqrt(h + s) + eps))[:, None] * G)
            assert lib.glint_vec_push_dev(sb.handle, uniq.data_ptr(), s.data_ptr(), u, 0, stream) == 0
            assert lib.glint_mat_push_rows_dev(wb.handle, uniq.data_ptr(), dw.data_ptr(), u, 0, stream) == 0
            # (the temporaries are freed into torch's allocator, which reuses them on this stream only)

        def host_rowwise():
            assert lib.glint_mat_push_rows_adagrad_rowwise(wa.handle, sa.handle, rows.ctypes.data, g.ctypes.data, n,
                                                           lr, eps) == 0

        def host_base():
            uniq, inv = np.unique(rows, return_inverse=True)
            G = np.zeros((uniq.size, cols))
            np.add.at(G, inv, g)
            w, h = np.empty_like(G), np.empty(uniq.size)
            assert lib.glint_mat_pull_rows(wb.handle, uniq.ctypes.data, w.ctypes.data, uniq.size) == 0
            assert lib.glint_vec_pull(sb.handle, uniq.ctypes.data, h.ctypes.data, uniq.size) == 0
            s = (G * G).mean(1)
            dw = -((lr / (np.sqrt(h + s) + eps))[:, None] * G)
            assert lib.glint_vec_push(sb.handle, uniq.ctypes.data, s.ctypes.data, uniq.size, 0) == 0
            assert lib.glint_mat_push_rows(wb.handle, uniq.ctypes.data, dw.ctypes.data, uniq.size, 0) == 0

        def host_adagrad():  # the Adagrad row push's host call on the same rows: the same bytes staged
            assert lib.glint_mat_push_rows_adagrad(wg.handle, hg.handle, rows.ctypes.data, g.ctypes.data, n, lr,
                                                   eps) == 0

        t = {k: [] for k in ("host_rowwise", "host_base", "host_adagrad", "dev_rowwise", "dev_base")}
        for rnd in range(rounds + 1):  # round 0 warms up; the legs alternate inside every round
            got = {"host_base": wall_ms(host_base), "host_rowwise": wall_ms(host_rowwise),
                   "host_adagrad": wall_ms(host_adagrad)}
            torch.cuda.synchronize()
            got["dev_base"] = ev_ms(dev_base)
            got["dev_rowwise"] = ev_ms(dev_rowwise)
            if rnd:
                for k, v in got.items():
                    t[k].append(v)
        lib.glint_prof_reset(wa.handle)  # the fold alone, mirrored on the baseline's shards
        lib.glint_prof_enable(wa.handle, 1)
        for _ in range(4):
            dev_rowwise()
            dev_base()
        torch.cuda.synchronize()
        fold_ms = kernel_ms(wa.handle, N.GLINT_K_PUSH_ROWS)
        lib.glint_prof_enable(wa.handle, 0)
        lib.glint_prof_reset(wg.handle)  # the Adagrad row push's fold on the same rows, with its cols-wide state
        lib.glint_prof_enable(wg.handle, 1)
        for _ in range(4):
            assert lib.glint_mat_push_rows_adagrad_dev(wg.handle, hg.handle, d_rows.data_ptr(), d_g.data_ptr(), n, lr,
                                                       eps, stream) == 0
        torch.cuda.synchronize()
        adagrad_fold_ms = kernel_ms(wg.handle, N.GLINT_K_PUSH_ROWS)
        lib.glint_prof_enable(wg.handle, 0)
        for sh in (wa, sa, wb, sb, wg, hg):
            sh.sync(stream)
        dw = (wa.getRows(all_rows) - wb.getRows(all_rows)).abs().max().item()
        ha_, hb_ = sa.get(all_rows), sb.get(all_rows)
        dh = ((ha_ - hb_).abs() / hb_.abs().clamp_min(1e-300)).max().item()
        del ha_, hb_
        agree = {"w": dw, "h": dh}
        print(f"rowwise legs disagree by {agree}; bound {ROWWISE_AGREE_BOUND}", file=sys.stderr, flush=True)
        assert all(agree[k] <= ROWWISE_AGREE_BOUND[k] for k in agree), (agree, ROWWISE_AGREE_BOUND)
        m = {k: stats(v) for k, v in t.items()}
        shard_bytes = (2 * distinct * cols + 2 * distinct) * 8
        adagrad_shard_bytes = 4 * distinct * cols * 8
        line = dict(
            op="mat_push_rows_adagrad_rowwise", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n,
            distinct_rows=distinct, longest_run=longest, rounds=rounds, lr=lr, eps=eps,
            keep_strips=N.GLINT_ROWWISE_KEEP_STRIPS, lib=os.environ.get("GLINT_GPU_LIB", "in-tree"),
            host_rowwise_ms=m["host_rowwise"], host_baseline_ms=m["host_base"],
            host_speedup=m["host_base"]["mean"] / m["host_rowwise"]["mean"],
            host_adagrad_ms=m["host_adagrad"], host_rowwise_bytes_staged=n * 8 + n * cols * 8,
            host_baseline_bytes_over_link=4 * distinct * 8 + 2 * distinct * cols * 8,
            dev_rowwise_ms=m["dev_rowwise"], dev_baseline_ms=m["dev_base"],
            dev_speedup=m["dev_base"]["mean"] / m["dev_rowwise"]["mean"],
            fold_kernel_ms=fold_ms, fold_gradient_bytes=n * cols * 8, fold_shard_bytes=shard_bytes,
            fold_GBps=(n * cols * 8 + shard_bytes) / (fold_ms * 1e-3) / 1e9,
            fold_fraction_of_hbm_peak=(n * cols * 8 + shard_bytes) / (fold_ms * 1e-3) / 1e9 / hbm_peak_gbs,
            hbm_peak_GBps=hbm_peak_gbs,
            adagrad_fold_kernel_ms=adagrad_fold_ms, adagrad_fold_shard_bytes=adagrad_shard_bytes,
            fold_over_adagrad_fold=fold_ms / adagrad_fold_ms,
            state_bytes_per_row={"rowwise_adagrad": 8, "adagrad": cols * 8, "adam": 2 * cols * 8},
            max_abs_weight_difference=dw, max_relative_state_difference=dh, agreement_bound=ROWWISE_AGREE_BOUND,
            note="host_*: C calls on pageable numpy arrays, synchronous, wall ms; baseline = np.unique + np.add.at, "
                 "the mean of squares, glint_mat_pull_rows and glint_vec_pull, the step in numpy, glint_vec_push "
                 "and glint_mat_push_rows of deltas. dev_*: one HIP event pair per call; baseline = torch.unique + "
                 "index_add_, the same with the _dev calls. Legs alternate inside each of `rounds` rounds after "
                 "one warm-up round. host_adagrad_ms: glint_mat_push_rows_adagrad on the same rows and gradients, on "
                 "the third pair. fold_kernel_ms: the fold alone (glint_prof, GLINT_K_PUSH_ROWS on the weights "
                 "shard); fold_gradient_bytes = rows * cols * 8, read once (rows of at most keep_strips strips) or "
                 "twice; fold_shard_bytes = (2 * distinct * cols + 2 * distinct) * 8; fold_GBps counts the "
                 "gradients once. adagrad_fold_kernel_ms: the Adagrad row push's fold (glint_rowadagrad.hip, the "
                 "parent commit's source unchanged) on the same rows and gradients in the same process, on a pair "
                 "of its own; its shard bytes are 4 * distinct * cols * 8")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    for sh in (wa, sa, wb, sb, wg, hg):
        sh.destroy()


def pairs_leg(rng, out_path):
    """Two tables per shape -- cfg5's per-GPU 2^17 x 512 Double, and word2vec-shaped 2^17 x 128 Float (short
    rows under one wave per pair) -- and n = 2^14 and 2^16 pairs, rows_a Zipf(1.0), rows_b uniform. The legs
    under test use one pair of shards (a1, b1), their baselines another (a2, b2) with the same content, on
    alternating rounds of one process; the baselines never run the code under test.
    Dot: glint_mat_pull_pairs_dot* against what a caller does today -- two glint_mat_pull_rows* and
    (A * B).sum(1) in torch / numpy. Axpy (dst = a, src = b): glint_mat_push_pairs_axpy* against
    glint_mat_pull_rows* of src, the scale by the caller, glint_mat_push_rows*. Device legs: a HIP event pair
    around each call; the two kernels alone by their prof ids, and their algorithmic bytes over that time
    as a fraction of the HBM peak. Host legs: wall time and the bytes over the link. After each n the two
    legs are compared: they sum in other orders, so they agree to rounding, not bit for bit. One JSON line
    per (shape, n, op), also appended to out_path."""
    shard_rows, rounds, hbm_peak_gbs = 1 << 17, 5, 8000.0
    part = glint_amd.RangePartition(0, 0, shard_rows)
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    def rounds_of(legs):
        """legs: name -> (timer, fn), run in the order given inside every round; round 0 warms up."""
        t = {k: [] for k in legs}
        for rnd in range(rounds + 1):
            for k, (timer, fn) in legs.items():
                torch.cuda.synchronize()
                v = timer(fn)
                if rnd:
                    t[k].append(v)
        return {k: stats(v) for k, v in t.items()}

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for dtype, cols in (("double", 512), ("float", 128)):
        a1, b1, a2, b2 = (glint_amd.PartialMatrix(part, cols, dtype, 0) for _ in range(4))
        tdt, npd, vs = a1.torch_dtype, a1.np_dtype, np.dtype(a1.np_dtype).itemsize
        tol = 1e-12 if dtype == "double" else 1e-4
        for x, y in ((a1, a2), (b1, b2)):
            v = torch.randn((shard_rows, cols), dtype=tdt, device=dev)
            x.updateRows(all_rows, v)
            y.updateRows(all_rows, v)
            del v
        for n in (1 << 14, 1 << 16):
            ra = zipf_keys(rng, shard_rows, n, 1.0)
            rb = rng.integers(0, shard_rows, n).astype(np.int64)
            coef = (rng.standard_normal(n) * 1e-3).astype(npd)
            d_ra, d_rb, d_coef = (torch.from_numpy(x).to(dev) for x in (ra, rb, coef))
            distinct = int(np.unique(ra).size)
            d_out = torch.empty(n, dtype=tdt, device=dev)
            h_out = np.empty(n, npd)
            res = {}

            # ---- dot ----------------------------------------------------------------------------
            def dev_dot():
                assert lib.glint_mat_pull_pairs_dot_dev(a1.handle, b1.handle, d_ra.data_ptr(), d_rb.data_ptr(), n,
                                                        d_out.data_ptr(), stream) == 0

            def dev_dot_base():
                A = torch.empty((n, cols), dtype=tdt, device=dev)
                B = torch.empty((n, cols), dtype=tdt, device=dev)
                assert lib.glint_mat_pull_rows_dev(a2.handle, d_ra.data_ptr(), A.data_ptr(), n, stream) == 0
                assert lib.glint_mat_pull_rows_dev(b2.handle, d_rb.data_ptr(), B.data_ptr(), n, stream) == 0
                res["dev_dot"] = (A * B).sum(1)

            def host_dot():
                assert lib.glint_mat_pull_pairs_dot(a1.handle, b1.handle, ra.ctypes.data, rb.ctypes.data, n,
                                                    h_out.ctypes.data) == 0

            def host_dot_base():
                A, B = np.empty((n, cols), npd), np.empty((n, cols), npd)
                assert lib.glint_mat_pull_rows(a2.handle, ra.ctypes.data, A.ctypes.data, n) == 0
                assert lib.glint_mat_pull_rows(b2.handle, rb.ctypes.data, B.ctypes.data, n) == 0
                res["host_dot"] = (A * B).sum(1)

            m = rounds_of({"host_base": (wall_ms, host_dot_base), "host_pairs": (wall_ms, host_dot),
                           "dev_base": (ev_ms, dev_dot_base), "dev_pairs": (ev_ms, dev_dot)})
            lib.glint_prof_reset(a1.handle)
            lib.glint_prof_enable(a1.handle, 1)
            for _ in range(3):
                dev_dot()
            torch.cuda.synchronize()
            k_ms = kernel_ms(a1.handle, N.GLINT_K_PULL_ROWS_DOT)
            lib.glint_prof_enable(a1.handle, 0)
            for sh in (a1, b1, a2, b2):
                sh.sync(stream)
            mag = (a2.getRows(d_ra).abs() * b2.getRows(d_rb).abs()).sum(1).clamp_min(1e-300)  # per pair: sum |a b|
            d_dev = ((d_out - res["dev_dot"]).abs() / mag).max().item()
            d_host = (np.abs(h_out - res["host_dot"]) / mag.cpu().numpy()).max()
            assert d_dev < tol and d_host < tol, (d_dev, d_host)
            k_bytes = 2 * n * cols * vs + 2 * n * 8 + n * vs
            line = dict(
                op="mat_pull_pairs_dot", dtype=dtype, pattern="rows_a zipf1.0, rows_b uniform", shape=[shard_rows, cols],
                pairs=n, rounds=rounds,
                host_pairs_ms=m["host_pairs"], host_baseline_ms=m["host_base"],
                host_speedup=m["host_base"]["mean"] / m["host_pairs"]["mean"],
                host_pairs_bytes_over_link=2 * n * 8 + n * vs, host_baseline_bytes_over_link=2 * n * 8 + 2 * n * cols * vs,
                dev_pairs_ms=m["dev_pairs"], dev_baseline_ms=m["dev_base"],
                dev_speedup=m["dev_base"]["mean"] / m["dev_pairs"]["mean"],
                kernel_ms=k_ms, kernel_bytes=k_bytes, kernel_GBps=k_bytes / (k_ms * 1e-3) / 1e9,
                kernel_fraction_of_hbm_peak=k_bytes / (k_ms * 1e-3) / 1e9 / hbm_peak_gbs, hbm_peak_GBps=hbm_peak_gbs,
                max_difference_over_sum_of_magnitudes=max(d_dev, float(d_host)),
                note="baseline = two glint_mat_pull_rows* and (A * B).sum(1) by the caller (torch on the device, "
                     "numpy on the host). host_*: C calls on pageable numpy arrays, synchronous, wall ms. dev_*: "
                     "one HIP event pair per call. Legs alternate inside each of `rounds` rounds after one "
                     "warm-up round. kernel_ms: the one launch alone (glint_prof, GLINT_K_PULL_ROWS_DOT on a); "
                     "kernel_bytes = 2 * pairs * cols * sizeof V plus ids and answers")
            emit(**line)
            with open(out_path, "a") as f:
                f.write(json.dumps(line) + "\n")
            res.clear()

            # ---- axpy (dst = a, src = b) -----------------------------------------------------------
            def dev_axpy():
                assert lib.glint_mat_push_pairs_axpy_dev(a1.handle, b1.handle, d_ra.data_ptr(), d_rb.data_ptr(),
                                                         d_coef.data_ptr(), n, 0, stream) == 0

            def dev_axpy_base():
                S = torch.empty((n, cols), dtype=tdt, device=dev)
                assert lib.glint_mat_pull_rows_dev(b2.handle, d_rb.data_ptr(), S.data_ptr(), n, stream) == 0
                T = d_coef[:, None] * S
                assert lib.glint_mat_push_rows_dev(a2.handle, d_ra.data_ptr(), T.data_ptr(), n, 0, stream) == 0

            def host_axpy():
                assert lib.glint_mat_push_pairs_axpy(a1.handle, b1.handle, ra.ctypes.data, rb.ctypes.data,
                                                     coef.ctypes.data, n, 0) == 0

            def host_axpy_base():
                S = np.empty((n, cols), npd)
                assert lib.glint_mat_pull_rows(b2.handle, rb.ctypes.data, S.ctypes.data, n) == 0
                T = coef[:, None] * S
                assert lib.glint_mat_push_rows(a2.handle, ra.ctypes.data, T.ctypes.data, n, 0) == 0

            m = rounds_of({"host_base": (wall_ms, host_axpy_base), "host_pairs": (wall_ms, host_axpy),
                           "dev_base": (ev_ms, dev_axpy_base), "dev_pairs": (ev_ms, dev_axpy)})
            lib.glint_prof_reset(a1.handle)
            lib.glint_prof_enable(a1.handle, 1)
            for _ in range(3):  # (both legs: the two destinations stay comparable)
                dev_axpy()
                dev_axpy_base()
            torch.cuda.synchronize()
            k_ms = kernel_ms(a1.handle, N.GLINT_K_PUSH_ROWS_AXPY)
            lib.glint_prof_enable(a1.handle, 0)
            for sh in (a1, b1, a2, b2):
                sh.sync(stream)
            g1, g2 = a1.getRows(all_rows), a2.getRows(all_rows)
            diff = ((g1 - g2).abs() / g2.abs().clamp_min(1.0)).max().item()
            del g1, g2
            assert diff < tol * 100, diff  # sums of up to thousands of terms per hot row, in other orders
            k_bytes = (n + 2 * distinct) * cols * vs + n * (4 + 8 + vs)
            line = dict(
                op="mat_push_pairs_axpy", dtype=dtype, pattern="rows_dst zipf1.0, rows_src uniform",
                shape=[shard_rows, cols], pairs=n, distinct_dst_rows=distinct, rounds=rounds,
                host_pairs_ms=m["host_pairs"], host_baseline_ms=m["host_base"],
                host_speedup=m["host_base"]["mean"] / m["host_pairs"]["mean"],
                host_pairs_bytes_over_link=2 * n * 8 + n * vs,
                host_baseline_bytes_over_link=2 * n * 8 + 2 * n * cols * vs,
                dev_pairs_ms=m["dev_pairs"], dev_baseline_ms=m["dev_base"],
                dev_speedup=m["dev_base"]["mean"] / m["dev_pairs"]["mean"],
                fold_kernel_ms=k_ms, fold_bytes=k_bytes, fold_GBps=k_bytes / (k_ms * 1e-3) / 1e9,
                fold_fraction_of_hbm_peak=k_bytes / (k_ms * 1e-3) / 1e9 / hbm_peak_gbs, hbm_peak_GBps=hbm_peak_gbs,
                max_relative_difference=diff,
                note="baseline = glint_mat_pull_rows* of src, coef[:, None] * rows by the caller (torch on the device, "
                     "numpy on the host), glint_mat_push_rows*. host_*: C calls on pageable numpy arrays, synchronous, "
                     "wall ms. dev_*: one HIP event pair per call (front end and fold), default order flags. Legs "
                     "alternate inside each of `rounds` rounds after one warm-up round. fold_kernel_ms: the fold "
                     "alone (glint_prof, GLINT_K_PUSH_ROWS_AXPY on dst); fold_bytes = (pairs + 2 * "
                     "distinct_dst_rows) * cols * sizeof V plus ids and coefficients")
            emit(**line)
            with open(out_path, "a") as f:
                f.write(json.dumps(line) + "\n")
        for sh in (a1, b1, a2, b2):
            sh.destroy()
        torch.cuda.empty_cache()


def groups_leg(rng, out_path):
    """Grouped row push on a word2vec / CBOW-shaped 2^17 x 128 Float shard and cfg5's per-GPU 2^17 x 512
    Double shard: g = 2^12 and 2^14 groups of 8 rows (n = 2^15 and 2^17 records), rows Zipf(1.0), value rows
    1e-3 x standard normal, with and without per-record weights. The call under test runs on one shard
    (s1), the baseline -- what a caller does today -- on another (s2) with the same content, on alternating
    rounds of one process; the baseline never runs the code under test.
    Device baseline: values.index_select(0, group), times the weights when weighted, in torch, then
    glint_mat_push_rows_dev. Host baseline: np.repeat, times the weights, then glint_mat_push_rows; wall
    clock. Device legs: a HIP event pair around each call; the fold alone by its prof id, and its
    algorithmic bytes over that time as a fraction of the HBM peak (the g x cols value rows are re-read from
    cache, so those bytes overstate HBM traffic). After each case the two shards are compared: the default
    order flags split long runs, so they agree to rounding, not bit for bit. One JSON line per (shape, g,
    weighted), also appended to out_path."""
    shard_rows, rounds, hbm_peak_gbs, per = 1 << 17, 5, 8000.0, 8
    part = glint_amd.RangePartition(0, 0, shard_rows)
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    def rounds_of(legs):
        """legs: name -> (timer, fn), run in the order given inside every round; round 0 warms up."""
        t = {k: [] for k in legs}
        for rnd in range(rounds + 1):
            for k, (timer, fn) in legs.items():
                torch.cuda.synchronize()
                v = timer(fn)
                if rnd:
                    t[k].append(v)
        return {k: stats(v) for k, v in t.items()}

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for dtype, cols in (("float", 128), ("double", 512)):
        s1, s2 = (glint_amd.PartialMatrix(part, cols, dtype, 0) for _ in range(2))
        tdt, npd, vs = s1.torch_dtype, s1.np_dtype, np.dtype(s1.np_dtype).itemsize
        tol = 1e-10 if dtype == "double" else 1e-2
        v = torch.randn((shard_rows, cols), dtype=tdt, device=dev)
        s1.updateRows(all_rows, v)
        s2.updateRows(all_rows, v)
        del v
        for g in (1 << 12, 1 << 14):
            n = g * per
            rows = zipf_keys(rng, shard_rows, n, 1.0)
            offsets = np.arange(g + 1, dtype=np.int64) * per
            group = np.repeat(np.arange(g, dtype=np.int64), per)
            vals = (rng.standard_normal((g, cols)) * 1e-3).astype(npd)
            wts = rng.random(n).astype(npd)
            d_rows, d_off, d_group, d_vals, d_wts = (torch.from_numpy(x).to(dev) for x in (rows, offsets, group, vals, wts))
            distinct = int(np.unique(rows).size)
            for weighted in (False, True):
                pw, dw = (wts.ctypes.data, d_wts.data_ptr()) if weighted else (None, None)

                def dev_grouped():
                    assert lib.glint_mat_push_rows_grouped_dev(s1.handle, d_rows.data_ptr(), n, d_off.data_ptr(), g,
                                                               d_vals.data_ptr(), dw, 0, stream) == 0

                def dev_base():
                    T = d_vals.index_select(0, d_group)
                    if weighted:
                        T = d_wts[:, None] * T
                    assert lib.glint_mat_push_rows_dev(s2.handle, d_rows.data_ptr(), T.data_ptr(), n, 0, stream) == 0

                def host_grouped():
                    assert lib.glint_mat_push_rows_grouped(s1.handle, rows.ctypes.data, n, offsets.ctypes.data, g,
                                                           vals.ctypes.data, pw, 0) == 0

                def host_base():
                    T = np.repeat(vals, per, axis=0)
                    if weighted:
                        T = wts[:, None] * T
                    assert lib.glint_mat_push_rows(s2.handle, rows.ctypes.data, T.ctypes.data, n, 0) == 0

                m = rounds_of({"host_base": (wall_ms, host_base), "host_grouped": (wall_ms, host_grouped),
                               "dev_base": (ev_ms, dev_base), "dev_grouped": (ev_ms, dev_grouped)})
                for sh in (s1, s2):
                    lib.glint_prof_reset(sh.handle)
                    lib.glint_prof_enable(sh.handle, 1)
                for _ in range(3):  # (both legs: the two shards stay comparable)
                    dev_grouped()
                    dev_base()
                torch.cuda.synchronize()
                k_ms = kernel_ms(s1.handle, N.GLINT_K_PUSH_ROWS)
                base_k_ms = kernel_ms(s2.handle, N.GLINT_K_PUSH_ROWS)  # the row push's fold over the expanded rows
                for sh in (s1, s2):
                    lib.glint_prof_enable(sh.handle, 0)
                for sh in (s1, s2):
                    sh.sync(stream)
                g1, g2 = s1.getRows(all_rows), s2.getRows(all_rows)
                diff = ((g1 - g2).abs() / g2.abs().clamp_min(1.0)).max().item()
                del g1, g2
                assert diff < tol, diff  # sums of up to thousands of terms per hot row, in other orders
                idx_bytes = n * 4 + (g + 1) * 8 + (n * vs if weighted else 0)
                k_bytes = (n + 2 * distinct) * cols * vs + idx_bytes
                link = n * 8 + (g + 1) * 8 + (n * vs if weighted else 0) + g * cols * vs
                line = dict(
                    op="mat_push_rows_grouped", dtype=dtype, weighted=weighted, pattern="rows zipf1.0, groups of 8",
                    shape=[shard_rows, cols], groups=g, records=n, distinct_rows=distinct, rounds=rounds,
                    host_grouped_ms=m["host_grouped"], host_baseline_ms=m["host_base"],
                    host_speedup=m["host_base"]["mean"] / m["host_grouped"]["mean"],
                    host_grouped_bytes_over_link=link, host_baseline_bytes_over_link=n * 8 + n * cols * vs,
                    dev_grouped_ms=m["dev_grouped"], dev_baseline_ms=m["dev_base"],
                    dev_speedup=m["dev_base"]["mean"] / m["dev_grouped"]["mean"],
                    fold_kernel_ms=k_ms, fold_bytes=k_bytes, fold_GBps=k_bytes / (k_ms * 1e-3) / 1e9,
                    fold_fraction_of_hbm_peak=k_bytes / (k_ms * 1e-3) / 1e9 / hbm_peak_gbs, hbm_peak_GBps=hbm_peak_gbs,
                    baseline_fold_kernel_ms=base_k_ms, max_relative_difference=diff,
                    note="baseline = the caller expands values to n x cols (index_select in torch on the device, "
                         "np.repeat on the host), times the weights when weighted, then glint_mat_push_rows*. host_*: C "
                         "calls on pageable numpy arrays, synchronous, wall ms. dev_*: one HIP event pair per call "
                         "(front end and fold), default order flags. Legs alternate inside each of `rounds` rounds "
                         "after one warm-up round. fold_kernel_ms: the fold alone (glint_prof, GLINT_K_PUSH_ROWS on "
                         "the shard under test); baseline_fold_kernel_ms: the row push's fold over the expanded rows, the "
                         "same id on the baseline's shard. fold_bytes = (records + 2 * distinct_rows) * cols * sizeof V plus "
                         "the per-record index, the group pointer and the weights; the g x cols value rows are "
                         "re-read from cache, so this overstates HBM traffic")
                emit(**line)
                with open(out_path, "a") as f:
                    f.write(json.dumps(line) + "\n")
        for sh in (s1, s2):
            sh.destroy()
        torch.cuda.empty_cache()


def wbag_leg(rng, out_path):
    """Weighted row-sum pull and grouped row-dot pull on cfg5's per-GPU 2^17 x 512 Double shard: 2^14
    Zipf(1.0) rows in groups of 1, 16 and 128 rows and as one group of all of them (the row-sum leg's request
    shapes), weights uniform in [0, 1), one standard-normal vector per group. The baselines are what a
    caller does today and never run the code under test: for the weighted sum a dense row pull into an
    n x cols buffer, a multiply and a segment reduction (torch index_add_ on the device, np.add.reduceat on
    the host); for the grouped dot a dense row pull and (rows * x[group]).sum(1). Beside them the unchanged
    neighbour kernels on the same request in the same process: the unweighted row-sum pull, and the row dot
    pull with one vector over the same rows. All legs alternate inside each of 5 rounds after a warm-up
    round; host legs by wall clock, device legs by one HIP event pair per call; the four kernels alone by
    their prof ids. One JSON line per group length, also appended to out_path."""
    shard_rows, cols, n, rounds = 1 << 17, 512, 1 << 14, 5
    msh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, shard_rows), cols, "double", 0)
    h = msh.handle
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    all_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev)
    for r0 in range(0, shard_rows, 1 << 14):  # fill in slices of whole rows
        vv = torch.rand((1 << 14, cols), dtype=torch.float64, device=dev, generator=gen) - 0.5
        msh.updateRows(all_rows[r0:r0 + (1 << 14)].contiguous(), vv)
    del vv
    rows = zipf_keys(rng, shard_rows, n, 1.0)
    wts = rng.random(n)
    d_rows, d_wts = torch.from_numpy(rows).to(dev), torch.from_numpy(wts).to(dev)
    dense_out = np.empty((n, cols), np.float64)
    d_dense = torch.empty((n, cols), dtype=torch.float64, device=dev)

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    def prof_ms(kid, fn, reps=5):
        """The kernel alone: mean over `reps` launches after a warm-up, by its prof id."""
        fn()
        torch.cuda.synchronize()
        lib.glint_prof_reset(h)
        lib.glint_prof_enable(h, 1)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms = kernel_ms(h, kid)
        lib.glint_prof_enable(h, 0)
        return ms

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for glen in (1, 16, 128, n):
        g = n // glen
        offsets = np.arange(g + 1, dtype=np.int64) * glen
        group = np.repeat(np.arange(g, dtype=np.int64), glen)
        x = rng.standard_normal((g, cols))
        d_off, d_group, d_x = (torch.from_numpy(a).to(dev) for a in (offsets, group, x))
        wsum_out, wsum_base = np.empty((g, cols)), np.empty((g, cols))
        gdot_out, gdot_base = np.empty(n), np.empty(n)
        d_wsum, d_wsum_base, d_sum = (torch.empty((g, cols), dtype=torch.float64, device=dev) for _ in range(3))
        d_gdot, d_gdot_base, d_dot1 = (torch.empty(n, dtype=torch.float64, device=dev) for _ in range(3))

        def host_wsum():
            assert lib.glint_mat_pull_rows_wsum(h, rows.ctypes.data, n, offsets.ctypes.data, g, wts.ctypes.data,
                                                wsum_out.ctypes.data) == 0

        def host_wsum_base():
            assert lib.glint_mat_pull_rows(h, rows.ctypes.data, dense_out.ctypes.data, n) == 0
            np.add.reduceat(wts[:, None] * dense_out, offsets[:-1], axis=0, out=wsum_base)

        def host_gdot():
            assert lib.glint_mat_pull_rows_gdot(h, rows.ctypes.data, n, offsets.ctypes.data, g, x.ctypes.data,
                                                gdot_out.ctypes.data) == 0

        def host_gdot_base():
            assert lib.glint_mat_pull_rows(h, rows.ctypes.data, dense_out.ctypes.data, n) == 0
            np.sum(dense_out * x[group], axis=1, out=gdot_base)

        def dev_wsum():
            assert lib.glint_mat_pull_rows_wsum_dev(h, d_rows.data_ptr(), n, d_off.data_ptr(), g, d_wts.data_ptr(),
                                                    d_wsum.data_ptr(), stream) == 0

        def dev_wsum_base():
            assert lib.glint_mat_pull_rows_dev(h, d_rows.data_ptr(), d_dense.data_ptr(), n, stream) == 0
            d_wsum_base.zero_()
            d_wsum_base.index_add_(0, d_group, d_wts[:, None] * d_dense)

        def dev_sum():  # the unchanged neighbour of the weighted sum
            assert lib.glint_mat_pull_rows_sum_dev(h, d_rows.data_ptr(), n, d_off.data_ptr(), g, d_sum.data_ptr(),
                                                   stream) == 0

        def dev_gdot():
            assert lib.glint_mat_pull_rows_gdot_dev(h, d_rows.data_ptr(), n, d_off.data_ptr(), g, d_x.data_ptr(),
                                                    d_gdot.data_ptr(), stream) == 0

        def dev_gdot_base():
            assert lib.glint_mat_pull_rows_dev(h, d_rows.data_ptr(), d_dense.data_ptr(), n, stream) == 0
            torch.sum(d_dense * d_x.index_select(0, d_group), dim=1, out=d_gdot_base)

        def dev_dot1():  # the unchanged neighbour of the grouped dot: one vector over the same rows
            assert lib.glint_mat_pull_rows_dot_dev(h, d_rows.data_ptr(), n, d_x.data_ptr(), 1, d_dot1.data_ptr(),
                                                   stream) == 0

        legs = {"host_wsum_base": (wall_ms, host_wsum_base), "host_wsum": (wall_ms, host_wsum),
                "host_gdot_base": (wall_ms, host_gdot_base), "host_gdot": (wall_ms, host_gdot),
                "dev_wsum_base": (ev_ms, dev_wsum_base), "dev_wsum": (ev_ms, dev_wsum), "dev_sum": (ev_ms, dev_sum),
                "dev_gdot_base": (ev_ms, dev_gdot_base), "dev_gdot": (ev_ms, dev_gdot), "dev_dot1": (ev_ms, dev_dot1)}
        t = {k: [] for k in legs}
        for rnd in range(rounds + 1):  # round 0 warms up; the legs alternate inside every round
            for k, (timer, fn) in legs.items():
                torch.cuda.synchronize()
                v = timer(fn)
                if rnd:
                    t[k].append(v)
        m = {k: stats(v) for k, v in t.items()}
        k_wsum, k_sum = prof_ms(N.GLINT_K_PULL_ROWS_SUM, dev_wsum), prof_ms(N.GLINT_K_PULL_ROWS_SUM, dev_sum)
        k_gdot, k_dot1 = prof_ms(N.GLINT_K_PULL_ROWS_DOT, dev_gdot), prof_ms(N.GLINT_K_PULL_ROWS_DOT, dev_dot1)
        msh.sync(stream)
        # the answers agree with the baselines up to the order of the additions and the fused products the
        # baselines may use: 1e-9 of each element's sum of |terms|
        ok_wsum = bool((np.abs(wsum_out - wsum_base) <=
                        1e-9 * np.add.reduceat(wts[:, None] * np.abs(dense_out), offsets[:-1], axis=0)).all())
        ok_gdot = bool((np.abs(gdot_out - gdot_base) <= 1e-9 * np.sum(np.abs(dense_out * x[group]), axis=1)).all())
        assert ok_wsum and ok_gdot
        same = bool(np.array_equal(d_wsum.cpu().numpy(), wsum_out) and np.array_equal(d_gdot.cpu().numpy(), gdot_out))
        assert same
        vs = 8
        line = dict(
            op="wbag_pull", pattern="zipf1.0 rows", shape=[shard_rows, cols], rows=n, group_len=glen, groups=g,
            rounds=rounds,
            host_wsum_ms=m["host_wsum"], host_wsum_baseline_ms=m["host_wsum_base"],
            host_wsum_speedup=m["host_wsum_base"]["mean"] / m["host_wsum"]["mean"],
            host_wsum_bytes_staged=n * 8 + (g + 1) * 8 + n * vs, host_wsum_bytes_back=g * cols * vs,
            host_gdot_ms=m["host_gdot"], host_gdot_baseline_ms=m["host_gdot_base"],
            host_gdot_speedup=m["host_gdot_base"]["mean"] / m["host_gdot"]["mean"],
            host_gdot_bytes_staged=n * 8 + (g + 1) * 8 + g * cols * vs, host_gdot_bytes_back=n * vs,
            host_baseline_bytes_staged=n * 8, host_baseline_bytes_back=n * cols * vs,
            dev_wsum_ms=m["dev_wsum"], dev_wsum_baseline_ms=m["dev_wsum_base"],
            dev_wsum_speedup=m["dev_wsum_base"]["mean"] / m["dev_wsum"]["mean"], dev_sum_ms=m["dev_sum"],
            dev_gdot_ms=m["dev_gdot"], dev_gdot_baseline_ms=m["dev_gdot_base"],
            dev_gdot_speedup=m["dev_gdot_base"]["mean"] / m["dev_gdot"]["mean"], dev_dot1_ms=m["dev_dot1"],
            wsum_kernel_ms=k_wsum, sum_kernel_ms=k_sum, wsum_over_sum_kernel=k_wsum / k_sum,
            gdot_kernel_ms=k_gdot, dot1_kernel_ms=k_dot1, gdot_over_dot1_kernel=k_gdot / k_dot1,
            within_bound=True, host_and_device_answers_identical=same,
            note="host_*: C calls on pageable numpy arrays into reused buffers, synchronous, wall ms; dev_*: one HIP "
                 "event pair per call. Baselines: glint_mat_pull_rows[_dev] into an n x cols buffer, then weights * "
                 "rows and np.add.reduceat (torch: zero_ + index_add_) for the weighted sum, (rows * "
                 "x[group]).sum(1) for the grouped dot. dev_sum / dev_dot1: the unchanged neighbours on the same "
                 "request -- glint_mat_pull_rows_sum_dev, and glint_mat_pull_rows_dot_dev with one vector. Legs "
                 "alternate inside each of `rounds` rounds after one warm-up round. *_kernel_ms: the kernel alone "
                 "(glint_prof), mean of 5 launches after a warm-up")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    msh.destroy()


def init_leg(rng, out_path):
    """Shard fill and uniform init on cfg5's per-GPU shard (2^17 x 512 Double) and a word2vec-shaped one
    (2^17 x 128 Float): the whole shard, and a list of 2^14 distinct rows in random order. The calls under
    test run on one shard (s1), the floor and the baselines on another (s2), all inside each of 5 rounds of
    one process after one warm-up round; the baselines never run the code under test.
    Floor: glint_shard_zero of the same shard (a memset and one synchronisation), wall time, next to the
    wall time of the whole-shard host calls, which end with the same synchronisation. Kernel: the one launch
    alone (GLINT_K_PUSH_ROWS, glint_prof_read) and the bytes it stores over that time. Device baseline, what
    a caller does today: torch.rand into an n x cols buffer, scale, glint_mat_push_rows_dev into the zeroed
    shard (HIP events around the three; the zeroing is not timed). Host baseline: numpy random, scale,
    glint_mat_push_rows (wall). link_bytes is what each sends over the host link. One JSON line per (shape,
    rows named), also appended to out_path."""
    shard_rows, n_list, rounds, hbm_peak_gbs = 1 << 17, 1 << 14, 5, 8000.0
    part = glint_amd.RangePartition(0, 0, shard_rows)
    lo, hi = -0.5 / 100, 0.5 / 100

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for dtype, cols in (("double", 512), ("float", 128)):
        s1, s2 = (glint_amd.PartialMatrix(part, cols, dtype, 0) for _ in range(2))
        tdt, npd, vs = s1.torch_dtype, s1.np_dtype, np.dtype(s1.np_dtype).itemsize
        lib.glint_prof_enable(s1.handle, 1)
        some = rng.permutation(shard_rows)[:n_list].astype(np.int64)
        for label, rows in (("whole", None), ("list", some)):
            n = shard_rows if rows is None else rows.size
            d_rows = torch.arange(shard_rows, dtype=torch.int64, device=dev) if rows is None else \
                torch.from_numpy(rows).to(dev)
            h_rows = np.arange(shard_rows, dtype=np.int64) if rows is None else rows
            stored = n * cols * vs
            one = np.full(1, 0.1, npd)
            seed = [0]

            def uniform_host():
                seed[0] += 1
                s1.initUniform(seed[0], lo, hi, rows=rows)

            def fill_host():
                s1.fill(one[0], rows=rows)

            def uniform_dev():
                seed[0] += 1
                assert lib.glint_shard_init_uniform_dev(s1.handle, None if rows is None else d_rows.data_ptr(),
                                                        0 if rows is None else n, seed[0], lo, hi, stream) == 0

            def zero_floor():
                s2.zero()

            def dev_base():
                v = torch.rand((n, cols), dtype=tdt, device=dev)
                v = v * (hi - lo) + lo
                assert lib.glint_mat_push_rows_dev(s2.handle, d_rows.data_ptr(), v.data_ptr(), n, 0, stream) == 0

            def host_base():
                v = (np.random.default_rng(seed[0]).random((n, cols), dtype=npd) * npd(hi - lo) + npd(lo))
                s2.updateRows(h_rows, v)

            t = {k: [] for k in ("zero", "uniform_host", "fill_host", "uniform_dev", "dev_base", "host_base",
                                 "uniform_kernel", "fill_kernel")}
            for rnd in range(rounds + 1):
                def rec(k, v):
                    if rnd:
                        t[k].append(v)
                torch.cuda.synchronize()
                rec("zero", wall_ms(zero_floor))
                lib.glint_prof_reset(s1.handle)
                rec("uniform_host", wall_ms(uniform_host))
                rec("uniform_kernel", kernel_total_ms(s1.handle, N.GLINT_K_PUSH_ROWS)[0])
                rec("zero", wall_ms(zero_floor))
                lib.glint_prof_reset(s1.handle)
                rec("fill_host", wall_ms(fill_host))
                rec("fill_kernel", kernel_total_ms(s1.handle, N.GLINT_K_PUSH_ROWS)[0])
                torch.cuda.synchronize()
                rec("uniform_dev", ev_ms(uniform_dev))
                s1.sync(stream)
                s2.zero()
                torch.cuda.synchronize()
                rec("dev_base", ev_ms(dev_base))
                s2.sync(stream)
                s2.zero()
                rec("host_base", wall_ms(host_base))
            r = {k: stats(v) for k, v in t.items()}
            uk, fk = r["uniform_kernel"]["mean"], r["fill_kernel"]["mean"]
            line = dict(
                op="shard_init", dtype=dtype, shard_rows=shard_rows, cols=cols, rows_named=label, n=n,
                rounds=rounds, stored_bytes=stored,
                zero_wall_ms=r["zero"], uniform_host_wall_ms=r["uniform_host"], fill_host_wall_ms=r["fill_host"],
                uniform_dev_call_ms=r["uniform_dev"], uniform_kernel_ms=r["uniform_kernel"],
                fill_kernel_ms=r["fill_kernel"],
                uniform_kernel_GBps=stored / (uk * 1e-3) / 1e9, fill_kernel_GBps=stored / (fk * 1e-3) / 1e9,
                uniform_kernel_fraction_of_hbm_peak=stored / (uk * 1e-3) / 1e9 / hbm_peak_gbs,
                uniform_host_over_zero=r["uniform_host"]["mean"] / r["zero"]["mean"],
                fill_host_over_zero=r["fill_host"]["mean"] / r["zero"]["mean"],
                uniform_kernel_over_zero=uk / r["zero"]["mean"],
                device_baseline_ms=r["dev_base"], host_baseline_wall_ms=r["host_base"],
                speedup_device=r["dev_base"]["mean"] / r["uniform_dev"]["mean"],
                speedup_host=r["host_base"]["mean"] / r["uniform_host"]["mean"],
                link_bytes={"uniform": 0 if rows is None else n * 8, "device_baseline": 0,
                            "host_baseline": n * 8 + stored},
                note="zero_wall_ms is glint_shard_zero of the whole shard in both rows: the floor of the whole-shard "
                     "rows only; the device baseline also writes and reads an n x cols buffer in HBM")
            emit(**line)
            with open(out_path, "a") as f:
                f.write(json.dumps(line) + "\n")
        s1.destroy()
        s2.destroy()


def sampler_leg(rng, out_path):
    """The row sampler at word2vec size: m = 2^20 Zipf(1.0) counts, n = 2^24 draws, without exclusion and with
    it at per = 5 (the positives drawn from the same table, so the hot keys are excluded often). HIP-event time
    of glint_sampler_draw_dev against what a device caller does today -- torch.rand, a scale to the total and
    torch.searchsorted over a device cdf; with exclusion, one redraw of the draws that hit their positive --
    alternating inside each of 5 rounds of one process after one warm-up round. Also the wall time of the
    creates (host weights, device weights) and of a host draw of the same n. One JSON line per case, also
    appended to out_path."""
    m, n, per, rounds = 1 << 20, 1 << 24, 5, 5
    counts = np.maximum((1 << 24) // rng.permutation(np.arange(1, m + 1, dtype=np.int64)), 1)  # ~ 1 / rank, shuffled
    d_counts = torch.from_numpy(counts).to(dev)
    cdf = torch.cumsum(d_counts, 0)
    total = int(cdf[-1])

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    create_host, create_dev = [], []
    for rnd in range(3):
        ms, s = wall_ms(lambda: glint_amd.Sampler(counts, device=0))
        s.destroy()
        create_host.append(ms)
        ms, s = wall_ms(lambda: glint_amd.Sampler(d_counts))
        create_dev.append(ms)
        if rnd < 2:
            s.destroy()
    assert s.info() == (m, 0, total, 0)
    out = torch.empty(n, dtype=torch.int64, device=dev)
    pos = s.draw(-(-n // per), 1, 1 << 40, out=torch.empty(-(-n // per), dtype=torch.int64, device=dev))
    pos_rep = pos.repeat_interleave(per)[:n]
    seed = [0]
    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for label, ex in (("plain", None), ("exclude_per5", pos)):
        def draw():
            seed[0] += 1
            assert lib.glint_sampler_draw_dev(s.handle, seed[0], seed[0] * n, n, None if ex is None else ex.data_ptr(),
                                              per, out.data_ptr(), stream) == 0

        def base_once():
            x = (torch.rand(n, dtype=torch.float64, device=dev) * total).to(torch.int64)
            return torch.searchsorted(cdf, x, right=True)

        def base():
            idx = base_once()
            if ex is not None:
                idx = torch.where(idx == pos_rep, base_once(), idx)
            return idx

        def host_draw():
            return s.draw(n, 7, 0, exclude=None if ex is None else pos.cpu().numpy(), per=per)

        t = {"draw": [], "base": [], "host": []}
        for rnd in range(rounds + 1):
            for k, fn in (("draw", draw), ("base", base)):
                torch.cuda.synchronize()
                v = ev_ms(fn)
                if rnd:
                    t[k].append(v)
            if rnd in (1, 2):
                t["host"].append(wall_ms(host_draw)[0])
        got = out.cpu().numpy()
        assert got.min() >= 0 and got.max() < m and (counts[got[:100000]] > 0).all()
        if ex is not None:
            assert not bool((out == pos_rep).any())  # (every excluded key has company in this table)
        r = {k: stats(v) for k, v in t.items()}
        line = dict(op="sampler_draw", m=m, n=n, exclusion=label, per=per if ex is not None else None, rounds=rounds,
                    library=os.path.basename(os.environ.get("GLINT_GPU_LIB", "in-tree")),
                    draw_dev_ms=r["draw"], device_baseline_ms=r["base"], host_draw_wall_ms=r["host"],
                    Gdraws_per_s=n / (r["draw"]["mean"] * 1e-3) / 1e9,
                    speedup_device=r["base"]["mean"] / r["draw"]["mean"],
                    create_host_wall_ms=stats(create_host[1:]), create_dev_wall_ms=stats(create_dev[1:]),
                    link_bytes={"draw_dev": 0, "host_draw": 8 * n + (8 * (-(-n // per)) if ex is not None else 0)},
                    note="the baseline draws float64 uniforms (53 bits, not reproducible across batch splits) and, with "
                         "exclusion, redraws once; it also writes and reads n x 8 B of uniforms in HBM")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    s.destroy()


def topk_leg(rng, out_path):
    """cfg5 per GPU: a 2^17 x 512 Double shard, the k = 16 best rows against q = 1, 8 and 64 query vectors.
    Host: glint_mat_pull_topk against glint_mat_pull_rows_dot over arange(size) + np.argpartition, wall time;
    the dense host pull of the whole shard alone for scale. Device: glint_mat_pull_topk_dev against
    glint_mat_pull_rows_dot_dev over arange(size) + torch.topk, a HIP event pair around each call. The legs
    alternate inside each of 5 rounds after a warm-up round, in this one process. The baselines never run
    the code under test, and both legs must name the same rows. The launches of a top-k call apart
    (glint_prof_read_launches): its scores launch against the dot kernel over the same rows at q = 1 and at
    this q, and its selection launches summed. One JSON line per q, also appended to out_path."""
    shard_rows, cols, k, rounds = 1 << 17, 512, 16, 5
    msh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, shard_rows), cols, "double", 0)
    h = msh.handle
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    d_all = torch.arange(shard_rows, dtype=torch.int64, device=dev)
    for r0 in range(0, shard_rows, 1 << 14):  # fill in slices of whole rows
        vv = torch.rand((1 << 14, cols), dtype=torch.float64, device=dev, generator=gen) - 0.5
        msh.updateRows(d_all[r0:r0 + (1 << 14)].contiguous(), vv)
    del vv
    all_rows = np.arange(shard_rows, dtype=np.int64)
    dense_out = np.empty((shard_rows, cols), np.float64)
    DOT = N.GLINT_K_PULL_ROWS_DOT

    def ev_ms(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b)

    def wall_ms(fn):
        t0 = time.perf_counter()
        fn()
        return (time.perf_counter() - t0) * 1e3

    def stats(ms):
        return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}

    def launches(reps, fn):
        """Per-launch device ms of `reps` calls of fn, as (reps, launches per call)."""
        lib.glint_prof_reset(h)
        lib.glint_prof_enable(h, 1)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        cnt = C.c_int64()
        lib.glint_prof_read_launches(h, DOT, None, 0, C.byref(cnt))
        ms = (C.c_double * cnt.value)()
        lib.glint_prof_read_launches(h, DOT, ms, cnt.value, C.byref(cnt))
        lib.glint_prof_enable(h, 0)
        return np.array(ms[:]).reshape(reps, -1)

    Path(out_path).parent.mkdir(parents=True, exist_ok=True)
    for q in (1, 8, 64):
        x = rng.standard_normal((q, cols))
        d_x = torch.from_numpy(x).to(dev)
        top_rows, top_vals = np.empty((q, k), np.int64), np.empty((q, k), np.float64)
        dot_out = np.empty((shard_rows, q), np.float64)
        base_rows = np.empty((q, k), np.int64)
        d_top_rows = torch.empty((q, k), dtype=torch.int64, device=dev)
        d_top_vals = torch.empty((q, k), dtype=torch.float64, device=dev)
        d_dot = torch.empty((shard_rows, q), dtype=torch.float64, device=dev)
        d_base = {}

        def host_topk():
            assert lib.glint_mat_pull_topk(h, x.ctypes.data, q, k, top_rows.ctypes.data, top_vals.ctypes.data) == 0

        def host_base():
            assert lib.glint_mat_pull_rows_dot(h, all_rows.ctypes.data, shard_rows, x.ctypes.data, q,
                                               dot_out.ctypes.data) == 0
            base_rows[:] = np.argpartition(-dot_out.T, k - 1, axis=1)[:, :k]

        def host_dense_pull():
            assert lib.glint_mat_pull_rows(h, all_rows.ctypes.data, dense_out.ctypes.data, shard_rows) == 0

        def dev_topk():
            assert lib.glint_mat_pull_topk_dev(h, d_x.data_ptr(), q, k, d_top_rows.data_ptr(), d_top_vals.data_ptr(),
                                               stream) == 0

        def dev_dot(qq=q):
            assert lib.glint_mat_pull_rows_dot_dev(h, d_all.data_ptr(), shard_rows, d_x.data_ptr(), qq,
                                                   d_dot.data_ptr(), stream) == 0

        def dev_base():
            dev_dot()
            d_base["vals"], d_base["rows"] = torch.topk(d_dot.t(), k, dim=1)

        t = {name: [] for name in ("host_topk", "host_base", "host_dense_pull", "dev_topk", "dev_base")}
        for rnd in range(rounds + 1):  # round 0 warms up; the legs alternate inside every round
            got = {"host_base": wall_ms(host_base), "host_topk": wall_ms(host_topk)}
            if q == 1:
                got["host_dense_pull"] = wall_ms(host_dense_pull)
            torch.cuda.synchronize()
            got["dev_base"] = ev_ms(dev_base)
            got["dev_topk"] = ev_ms(dev_topk)
            if rnd:
                for name, v in got.items():
                    t[name].append(v)
        msh.sync(stream)
        # both legs name the same rows (random Double scores: no ties), and the two calls the same bits
        d_rows_h = d_top_rows.cpu().numpy()
        same_host = bool(np.array_equal(np.sort(base_rows, axis=1), np.sort(top_rows, axis=1)))
        same_dev = bool(np.array_equal(np.sort(d_base["rows"].cpu().numpy(), axis=1), np.sort(d_rows_h, axis=1)))
        assert same_host and same_dev
        identical = bool(np.array_equal(d_rows_h, top_rows) and np.array_equal(d_top_vals.cpu().numpy(), top_vals))
        each = launches(5, dev_topk)
        k_scores, k_select = float(each[:, 0].mean()), float(each[:, 1:].sum(axis=1).mean())
        k_dot_q = float(launches(5, dev_dot).mean())
        k_dot_1 = float(launches(5, lambda: dev_dot(1)).mean())
        m = {name: stats(v) for name, v in t.items() if v}
        line = dict(
            op="mat_pull_topk", shape=[shard_rows, cols], k=k, queries=q, rounds=rounds,
            host_topk_ms=m["host_topk"], host_baseline_ms=m["host_base"],
            host_dense_pull_ms=m.get("host_dense_pull"),
            host_speedup=m["host_base"]["mean"] / m["host_topk"]["mean"],
            host_topk_bytes_up=q * cols * 8, host_topk_bytes_back=q * k * 16,
            host_baseline_bytes_up=shard_rows * 8 + q * cols * 8, host_baseline_bytes_back=shard_rows * q * 8,
            dev_topk_ms=m["dev_topk"], dev_baseline_ms=m["dev_base"],
            dev_speedup=m["dev_base"]["mean"] / m["dev_topk"]["mean"],
            launches_per_call=int(each.shape[1]), scores_kernel_ms=k_scores, selection_kernels_ms=k_select,
            dot_kernel_same_q_ms=k_dot_q, dot_kernel_q1_ms=k_dot_1,
            scores_over_dot_q1=k_scores / k_dot_1, scores_over_dot_same_q=k_scores / k_dot_q,
            selection_over_scores=k_select / k_scores,
            scores_GBps=shard_rows * cols * 8 / (k_scores * 1e-3) / 1e9,
            same_rows_host=same_host, same_rows_dev=same_dev, host_and_device_answers_identical=identical,
            note="host_*: C calls on pageable numpy arrays, synchronous, wall ms; baseline = glint_mat_pull_rows_dot "
                 "over arange(size) + np.argpartition; host_dense_pull = glint_mat_pull_rows of the whole shard "
                 "(measured with q = 1 only). dev_*: one HIP event pair per call; baseline = "
                 "glint_mat_pull_rows_dot_dev over arange(size) + torch.topk. Legs alternate inside each of `rounds` "
                 "rounds after one warm-up round. *_kernel*_ms: launches apart (glint_prof_read_launches), mean of 5 "
                 "calls; scores_GBps counts the shard's rows once")
        emit(**line)
        with open(out_path, "a") as f:
            f.write(json.dumps(line) + "\n")
    msh.destroy()


def main():
    if "--sampler" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "sampler" / "sampler.jsonl")
        sampler_leg(np.random.default_rng(42), out)
        return
    if "--topk" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "topk" / "topk_pull.jsonl")
        topk_leg(np.random.default_rng(42), out)
        return
    if "--init" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "init" / "init.jsonl")
        init_leg(np.random.default_rng(42), out)
        return
    if "--adagrad" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "adagrad" / "adagrad_push.jsonl")
        adagrad_leg(np.random.default_rng(42), out)
        return
    if "--adam" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "adam" / "adam_push.jsonl")
        adam_leg(np.random.default_rng(42), out)
        return
    if "--wbag" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "wbag" / "wbag_pull.jsonl")
        wbag_leg(np.random.default_rng(42), out)
        return
    if "--ftrl" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "ftrl" / "ftrl_push.jsonl")
        ftrl_leg(np.random.default_rng(42), out)
        return
    if "--rowwise" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "rowwise_adagrad" / "rowwise_push.jsonl")
        rowwise_leg(np.random.default_rng(42), out)
        return
    if "--groups" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "groups" / "groups.jsonl")
        groups_leg(np.random.default_rng(42), out)
        return
    if "--pairs" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "pairs" / "pairs.jsonl")
        pairs_leg(np.random.default_rng(42), out)
        return
    if "--axpy" in sys.argv:
        out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
            str(Path(__file__).resolve().parent.parent / "profiles" / "axpy" / "axpy_push.jsonl")
        axpy_leg(np.random.default_rng(42), out)
        return
    if "--dot" in sys.argv:
        dot_leg(np.random.default_rng(42))
        return
    if "--sparse" in sys.argv:
        sparse_leg(np.random.default_rng(42))
        return
    if "--rowsum" in sys.argv:
        rowsum_leg(np.random.default_rng(42))
        return
    lg = 26 if QUICK else 28
    n = 1 << lg
    rng = np.random.default_rng(42)

    # ---- vector pull (device-resident), dense and random ------------------------------------------
    sh = glint_amd.PartialVector(glint_amd.RangePartition(0, 0, n), "double", 0)
    h = sh.handle
    keys = torch.arange(n, dtype=torch.int64, device=dev)
    vals = torch.rand(n, dtype=torch.float64, device=dev)
    out = torch.empty_like(vals)
    sh.update(keys, vals)
    dt = timed(lambda: lib.glint_vec_pull_dev(h, keys.data_ptr(), out.data_ptr(), n, stream), 10, h)
    k = kernel_ms(h, N.GLINT_K_VEC_PULL)
    emit(op="vec_pull_dev", pattern="dense", records=n, ms=dt * 1e3, kernel_ms=k,
         algorithmic_GBps=24.0 * n / (k * 1e-3) / 1e9, note="24 B/record: key 8 + shard 8 + out 8")
    rkeys = torch.randint(0, n, (n,), dtype=torch.int64, device=dev)
    dt = timed(lambda: lib.glint_vec_pull_dev(h, rkeys.data_ptr(), out.data_ptr(), n, stream), 5, h)
    k = kernel_ms(h, N.GLINT_K_VEC_PULL)
    emit(op="vec_pull_dev", pattern="uniform random", records=n, ms=dt * 1e3, kernel_ms=k,
         algorithmic_GBps=24.0 * n / (k * 1e-3) / 1e9, Grecords_per_s=n / (k * 1e-3) / 1e9)

    # ---- deterministic push of a dense run (same bytes as default mode) --------------------------
    dt = timed(lambda: lib.glint_vec_push_dev(h, keys.data_ptr(), vals.data_ptr(), n, 1, stream), 5, h)
    emit(op="vec_push_dev", mode="deterministic", pattern="dense", records=n, ms=dt * 1e3,
         algorithmic_GBps=32.0 * n / dt / 1e9)

    # ---- end-to-end host-pointer push / pull (pageable numpy, what the JNI shim passes) -----------
    m = 1 << (24 if QUICK else 26)
    hk = np.arange(m, dtype=np.int64)
    hv = np.random.default_rng(1).uniform(-1, 1, m)
    ho = np.empty(m, np.float64)
    lib.glint_vec_push(h, hk.ctypes.data, hv.ctypes.data, m, 0)
    t0 = time.perf_counter()
    for _ in range(5):
        lib.glint_vec_push(h, hk.ctypes.data, hv.ctypes.data, m, 0)
    dt = (time.perf_counter() - t0) / 5
    emit(op="vec_push_host", pattern="dense", records=m, ms=dt * 1e3, host_bytes_per_s=16.0 * m / dt / 1e9,
         algorithmic_GBps=32.0 * m / dt / 1e9, note="pageable H2D of keys+values + push kernels, synchronous")
    t0 = time.perf_counter()
    for _ in range(5):
        lib.glint_vec_pull(h, hk.ctypes.data, ho.ctypes.data, m)
    dt = (time.perf_counter() - t0) / 5
    emit(op="vec_pull_host", pattern="dense", records=m, ms=dt * 1e3, host_bytes_per_s=16.0 * m / dt / 1e9,
         note="pageable H2D of keys + gather + D2H of values, synchronous")
    sh.destroy()
    del keys, vals, out, rkeys

    # ---- client routing: stable grouping of a 2^26-record batch by owning partition ----------------
    m = 1 << 26
    rkeys = torch.randint(0, 1 << 30, (m,), dtype=torch.int64, device=dev)
    counts = torch.empty(4096, dtype=torch.int64, device=dev)
    order = torch.empty(m, dtype=torch.int64, device=dev)
    bad = C.c_int64()
    for nparts in (8, 64, 4096):
        fn = lambda: lib.glint_route_dev(rkeys.data_ptr(), m, N.GLINT_ROUTE_RANGE, nparts, 1 << 30,  # noqa: E731
                                         counts.data_ptr(), order.data_ptr(), C.byref(bad), stream)
        fn()
        t0 = time.perf_counter()
        for _ in range(5):
            assert fn() == 0
        dt = (time.perf_counter() - t0) / 5
        emit(op="route_dev", nparts=nparts, records=m, ms=dt * 1e3, Grecords_per_s=m / dt / 1e9,
             algorithmic_GBps=(8.0 * 2 + 8.0) * m / dt / 1e9,
             note="keys read twice (histogram, scatter) + 8 B index written; includes the D2H status sync")
    del rkeys, order

    # ---- cfg3: Zipf(1.1) sparse push with duplicates into a 2^28 shard -----------------------------
    sh = glint_amd.PartialVector(glint_amd.RangePartition(0, 0, n), "double", 0)
    h = sh.handle
    nz = n // 4
    zk = zipf_keys(rng, n, nz, 1.1)
    U = int(np.unique(zk).size)
    zkeys = torch.from_numpy(zk).to(dev)
    zvals = torch.rand(zk.size, dtype=torch.float64, device=dev)
    uk = torch.randint(0, n, (nz,), dtype=torch.int64, device=dev)
    for pat, kt, Uk in (("zipf1.1", zkeys, U), ("uniform random", uk, None)):
        for mode, flags, env in (("atomic", 0, "0"), ("binned (UNORDERED hint)", N.GLINT_PUSH_UNORDERED, ""),
                                 ("adaptive (no hint)", 0, "")):
            os.environ["GLINT_BINNED"] = env
            glint_amd._native.reload_env()  # the library caches its knobs
            dt = timed(lambda: lib.glint_vec_push_dev(h, kt.data_ptr(), zvals.data_ptr(), nz, flags, stream), 5, h)
            rec = dict(op="vec_push_dev", pattern=pat, path=mode, records=nz, ms=dt * 1e3,
                       Grecords_per_s=nz / dt / 1e9,
                       scatter_kernel_ms=kernel_ms(h, N.GLINT_K_PUSH_SCATTER),
                       binned_pipeline_ms=kernel_ms(h, N.GLINT_K_PUSH_BINNED))
            if Uk is not None:
                rec.update(distinct=Uk, dup_ratio=1 - Uk / nz, algorithmic_GBps=(16.0 * nz + 16.0 * Uk) / dt / 1e9)
            else:
                rec.update(algorithmic_GBps=32.0 * nz / dt / 1e9)
            emit(**rec)
        os.environ["GLINT_BINNED"] = ""
        glint_amd._native.reload_env()  # the library caches its knobs
    dt = timed(lambda: lib.glint_vec_push_dev(h, zkeys.data_ptr(), zvals.data_ptr(), zk.size, 1, stream), 2, h)
    emit(op="vec_push_dev", mode="deterministic", pattern="zipf1.1", records=int(zk.size), ms=dt * 1e3,
         algorithmic_GBps=(16.0 * zk.size + 16.0 * U) / dt / 1e9)
    sh.destroy()
    del zkeys, zvals, uk

    # ---- cfg5 (one of 8 shards): 2^17 x 512 Double matrix, Zipf(1.0) rows, row pull -----------------
    rows_total, cols = 1 << 20, 512
    shard_rows = rows_total // 8
    msh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, shard_rows), cols, "double", 0)
    h = msh.handle
    npush = (1 << 26) // 8
    r = zipf_keys(rng, shard_rows, npush, 1.0)
    c = rng.integers(0, cols, r.size).astype(np.int32)
    U = int(np.unique(r.astype(np.int64) * cols + c).size)
    mr = torch.from_numpy(r).to(dev)
    mc = torch.from_numpy(c).to(dev)
    mv = torch.rand(r.size, dtype=torch.float64, device=dev)
    dt = timed(lambda: lib.glint_mat_push_dev(h, mr.data_ptr(), mc.data_ptr(), mv.data_ptr(), r.size, 0, stream),
               5, h)
    emit(op="mat_push_dev", pattern="zipf1.0 rows x uniform cols", shape=[shard_rows, cols], records=int(r.size),
         distinct=U, ms=dt * 1e3, algorithmic_GBps=(20.0 * r.size + 16.0 * U) / dt / 1e9,
         Grecords_per_s=r.size / dt / 1e9)
    for mode, flags, env in (("atomic", 0, "0"), ("binned (UNORDERED hint)", N.GLINT_PUSH_UNORDERED, "")):
        os.environ["GLINT_BINNED"] = env
        glint_amd._native.reload_env()  # the library caches its knobs
        dt = timed(lambda: lib.glint_mat_push_dev(h, mr.data_ptr(), mc.data_ptr(), mv.data_ptr(), r.size, flags,
                                                  stream), 5, h)
        emit(op="mat_push_dev", pattern="zipf1.0 rows x uniform cols", path=mode, records=int(r.size), distinct=U,
             ms=dt * 1e3, algorithmic_GBps=(20.0 * r.size + 16.0 * U) / dt / 1e9, Grecords_per_s=r.size / dt / 1e9)
    os.environ["GLINT_BINNED"] = ""
    glint_amd._native.reload_env()  # the library caches its knobs
    nrow = (1 << 16) // 8
    qr = torch.from_numpy(zipf_keys(rng, shard_rows, nrow, 1.0)).to(dev)
    rout = torch.empty((qr.numel(), cols), dtype=torch.float64, device=dev)
    dt = timed(lambda: lib.glint_mat_pull_rows_dev(h, qr.data_ptr(), rout.data_ptr(), qr.numel(), stream), 10, h)
    k = kernel_ms(h, N.GLINT_K_MAT_PULL_ROWS)
    emit(op="mat_pull_rows_dev", pattern="zipf1.0 rows", rows=qr.numel(), cols=cols, ms=dt * 1e3, kernel_ms=k,
         algorithmic_GBps=qr.numel() * (8 + 2 * cols * 8) / (k * 1e-3) / 1e9)
    # dense row-major sweep push of the whole shard (affine: the ordered plain path)
    dr = torch.arange(shard_rows, dtype=torch.int64, device=dev).repeat_interleave(cols)
    dc = torch.arange(cols, dtype=torch.int32, device=dev).repeat(shard_rows)
    dv = torch.rand(dr.numel(), dtype=torch.float64, device=dev)
    dt = timed(lambda: lib.glint_mat_push_dev(h, dr.data_ptr(), dc.data_ptr(), dv.data_ptr(), dr.numel(), 0, stream),
               5, h)
    emit(op="mat_push_dev", pattern="dense row-major sweep", records=dr.numel(), ms=dt * 1e3,
         algorithmic_GBps=36.0 * dr.numel() / dt / 1e9, note="36 B/record: row 8 + col 4 + value 8 + shard 16")
    msh.destroy()

    # ---- sparse row pull against the dense one (cfg5 shard, three densities) ------------------------
    sparse_leg(rng)

    # ---- configs[0] end to end over loopback TCP: HBM shards behind the wire ingest ----------------
    import subprocess
    from glint_amd.build import LIB, LOOPBACK_BIN
    for servers, keys, msg in ((2, 1_000_000, 1000), (2, 1 << 24, 79_999)):
        r = subprocess.run([str(LOOPBACK_BIN), "--backend", "gpu", "--lib", str(LIB), "--servers", str(servers),
                            "--keys", str(keys), "--msg", str(msg)], capture_output=True, text=True, timeout=300)
        rec = json.loads(r.stdout.strip().splitlines()[-1]) if r.returncode == 0 else {"error": r.stderr[-300:]}
        emit(op="loopback_tcp", **rec)


if __name__ == "__main__":
    main()
