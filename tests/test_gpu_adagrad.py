"""Adagrad row push (PartialMatrix.updateRowsAdagrad, glint_mat_push_rows_adagrad*) against the replay.

The call is deterministic on every path -- no run is split, no atomic -- so the bar is one: both shards
equal adagrad_cases.replay_adagrad bit for bit (a NaN by class), on the host and on the device path.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import (ArrayIndexOutOfBoundsException, Client, CyclicPartition, PartialMatrix, PartialVector,
                       RangePartition)
from oracle import oracle as O
from adagrad_cases import (NOFMA, adagrad_inputs, adagrad_step, assert_bits, bits, replay_adagrad, start_tables,
                           sweep_inputs)
from ieee_cases import write_image
import test_gpu_rows as R  # the sort ladder's case builders

pytestmark = pytest.mark.gpu
DT = ["double", "float"]
START, SIZE = 1_000_003, 1500
PATTERNS = ["sorted_once", "permutation", "duplicates", "one_row", "single", "empty"]
REPEATS = ("duplicates", "one_row")
PATHS = ["host", "dev"]
LR, EPS = 0.05, 1e-6


def npd_of(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def make_rows(rng, pattern):
    if pattern == "sorted_once":
        return np.arange(START, START + SIZE, dtype=np.int64)
    if pattern == "permutation":
        return rng.permutation(SIZE).astype(np.int64) + START
    if pattern == "duplicates":
        return rng.choice(rng.choice(SIZE, 40, replace=False), 3000).astype(np.int64) + START
    if pattern == "one_row":  # crosses the sort's 2048-key tile and the 64-id batch
        return np.full(2100, START + 777, np.int64)
    if pattern == "single":
        return np.array([START + 17], np.int64)
    return np.zeros(0, np.int64)


def pair(gpu, cols, dtype, size=SIZE, start=START):
    part = RangePartition(2, start, start + size)
    return PartialMatrix(part, cols, dtype, gpu), PartialMatrix(part, cols, dtype, gpu)


def fill(sh, table, start=START):
    """The table into a zero shard: 0 + x is x (the tables hold no -0.0)."""
    sh.updateRows(np.arange(start, start + table.shape[0], dtype=np.int64), table)


def push(w, h, gpu, rows, g, path, lr=LR, eps=EPS, sync=True):
    if path == "host":
        assert w.updateRowsAdagrad(h, rows, g, lr, eps)
        return
    import torch
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    assert w.updateRowsAdagrad(h, t(rows), t(g), lr, eps, sync=sync)


@functools.lru_cache(maxsize=None)
def case(dtype, cols, pattern):
    """(rows, grads, weights and state after the push applied twice from start_tables): computed once and
    shared by the paths; read-only."""
    rng = np.random.default_rng(zlib.crc32(f"adagrad/{dtype}/{cols}/{pattern}".encode()))
    rows = make_rows(rng, pattern)
    name = np.dtype(npd_of(dtype)).name
    g = adagrad_inputs(name, rows.size, cols)
    w, h = start_tables(name, SIZE, cols)
    for _ in range(2):
        w, h = replay_adagrad(w, h, rows - START, g, LR, EPS)
    for a in (rows, w, h):
        a.setflags(write=False)
    return rows, g, w, h


# every instance on the scalar slice (3, 67: less than and more than one slice) and the 16-B slice (128)
# over the runs that repeat; the other patterns and sizes on a thinner grid
CORE = {(dt, c, pat) for dt in DT for c in (3, 67, 128) for pat in REPEATS}
WIDE = {(dt, c, pat) for dt, c in (("double", 1), ("float", 1), ("double", 130), ("float", 130), ("double", 513),
                                   ("float", 513), ("double", 67), ("float", 128))
        for pat in PATTERNS}
GRID = sorted(CORE | WIDE)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols,pattern", GRID)
def test_adagrad_push_parity(gpu, dtype, cols, pattern, path):
    rows, g, want_w, want_h = case(dtype, cols, pattern)
    name = np.dtype(npd_of(dtype)).name
    w0, h0 = start_tables(name, SIZE, cols)
    w, h = pair(gpu, cols, dtype)
    with w, h:
        fill(w, w0)
        fill(h, h0)
        for _ in range(2):  # the second push steps from the first one's state
            push(w, h, gpu, rows, g, path)
        assert_bits(h.to_numpy(), want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- the sort's geometry ------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("size", R.SORT_SIZES[:-1])
def test_adagrad_push_sort_passes(gpu, size, path):
    """The row push's ladder of shard sizes (test_gpu_rows.sort_rows: one to three passes of the shared
    sort, either buffer pair, the runs of RUNS). Double; three pushes onto one pair of zero shards; two
    records outside on the device path: skipped, raised at the sync with the first one's index."""
    import torch
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    cols = R.sort_cols(size)
    rng = np.random.default_rng(zlib.crc32(f"adagrad/sort/{size}/{path}".encode()))
    want_w, want_h = np.zeros((size, cols)), np.zeros((size, cols))
    w, h = pair(gpu, cols, "double", size)
    with w, h:
        for n in R.SORT_N:
            local, _, _ = R.sort_rows(rng, size, n, path != "host")
            g = adagrad_inputs("float64", n, cols, f"sort/{size}/{path}")
            inside = (local >= 0) & (local < size)
            want_w, want_h = replay_adagrad(want_w, want_h, local[inside], g[inside], LR, EPS)
            if path == "host":
                assert w.updateRowsAdagrad(h, local + START, g, LR, EPS)
                continue
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                w.updateRowsAdagrad(h, t(local + START), t(g), LR, EPS)
            assert ei.value.record == int(np.flatnonzero(~inside)[0])
        assert_bits(h.to_numpy(), want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- correctly rounded sqrt and divide, subnormals kept ----------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", [0.0, 2.0 ** -30])
@pytest.mark.parametrize("dtype", DT)
def test_adagrad_rounding_sweep(gpu, dtype, eps, path):
    """One push, every row once, cols 128: h over the type's whole exponent range, G over the issue's span
    and a band below it (adagrad_cases.sweep_inputs). A fast sqrt or divide, or flushed subnormals, would
    show here. The premises are asserted first, on the CPU."""
    npd = npd_of(dtype)
    cols = 128
    h0, G, w0 = sweep_inputs(np.dtype(npd).name, SIZE, cols)
    want_w, want_h = adagrad_step(w0, h0, G, LR, eps)
    tiny = np.finfo(npd).tiny
    sub = lambda a: int(((a != 0) & (np.abs(a) < tiny)).sum())  # noqa: E731
    with np.errstate(all="ignore"):
        d = np.add(np.sqrt(want_h, dtype=npd), npd(eps), dtype=npd)
        u = np.multiply(npd(LR), G, dtype=npd)
        p = np.divide(u, d, dtype=npd)
    inexact = int((np.multiply(p, d, dtype=npd) != u).sum())  # p * d rounds away from u: the quotient was rounded
    print(f"{dtype} eps {eps}: subnormal h' {sub(want_h)}, subnormal p {sub(p)}, p * d != u {inexact}")
    assert sub(want_h) > 1000 and sub(p) > 1000 and inexact > 1000 and sub(h0) > 1000 and (h0 == 0).sum() > 100
    rows = np.random.default_rng(4).permutation(SIZE).astype(np.int64) + START
    w, h = pair(gpu, cols, dtype)
    with w, h:
        write_image(w, gpu, w0, npd(0))
        write_image(h, gpu, h0, npd(0))
        push(w, h, gpu, rows, G[rows - START], path, LR, eps)
        assert_bits(h.to_numpy(), want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- no fused multiply-add ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("run", [1, 3])
@pytest.mark.parametrize("dtype,cols", [("double", 2), ("double", 67), ("float", 2), ("float", 4), ("float", 67)])
def test_adagrad_is_unfused(gpu, dtype, cols, run, path):
    """h = -b, G = a, eps = 1: h' = -b + a * a is exactly +0 with a rounded product and 2^-54 / 2^-24 fused.
    As a single record, and as the middle record of a run of three for one row (the others zero)."""
    npd = npd_of(dtype)
    a, b, fused = NOFMA[npd]
    c = cols - 1  # column 66: the second slice of the scalar path
    rows = np.full(run, START + 5, np.int64)
    g = np.zeros((run, cols), npd)
    g[run // 2, c] = a
    h0, w0 = np.zeros((SIZE, cols), npd), np.zeros((SIZE, cols), npd)
    h0[5, c] = -b
    w0[5] = 3.0
    want_w, want_h = replay_adagrad(w0, h0, rows - START, g, 0.5, 1.0)
    assert bits(want_h)[5, c] == 0
    w, h = pair(gpu, cols, dtype)
    with w, h:
        fill(h, h0)
        fill(w, w0)
        assert h.to_numpy()[5, c] == -b
        push(w, h, gpu, rows, g, path, 0.5, 1.0)
        got = h.to_numpy()
        assert bits(got)[5, c] == 0, f"{got[5, c]!r}: a fused h + G * G would leave {fused!r}"
        assert_bits(got, want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- the bits do not depend on the alignment of grads -------------------------------------------------
def test_adagrad_path_independence(gpu):
    import torch
    cols = 128
    rows, g, want_w, want_h = case("double", cols, "duplicates")
    w0, h0 = start_tables("float64", SIZE, cols)
    d = torch.device("cuda", gpu)
    buf = torch.zeros(g.size + 3, dtype=torch.float64, device=d)
    v = buf[1:1 + g.size]  # the same values one element into a buffer: 8-B aligned only
    v.copy_(torch.from_numpy(np.array(g)).to(d).view(-1))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    w, h = pair(gpu, cols, "double")
    with w, h:
        fill(w, w0)
        fill(h, h0)
        for _ in range(2):
            w.updateRowsAdagrad(h, torch.from_numpy(np.array(rows)).to(d), v, LR, EPS)
        assert_bits(h.to_numpy(), want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- IEEE edges and padding -----------------------------------------------------------------------------
def read_image(sh, gpu, rows, pitch):
    import torch
    d = torch.device("cuda", gpu)
    dst = torch.empty((rows, pitch), dtype=sh.torch_dtype, device=d)
    segs = np.array([0, 0, dst.numel() * dst.element_size()], np.int64)
    assert N.load().glint_copy_segments_dev(sh.data_ptr(), dst.data_ptr(), segs.ctypes.data_as(C.POINTER(C.c_int64)),
                                            1, torch.cuda.current_stream(d).cuda_stream) == N.GLINT_OK
    torch.cuda.synchronize(d)
    return dst.cpu().numpy()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("double", 6), ("float", 67), ("float", 12)])
def test_adagrad_ieee_edges(gpu, dtype, cols, path):
    """0 / 0 is NaN, an overflowing G * G, the sign of a zero step, an unnamed row's bits and the pitch
    padding of both shards; each against the replay, a NaN by class."""
    npd = npd_of(dtype)
    big = npd(1e200 if dtype == "double" else 1e30)
    nan_bits = 0x7FF8000000000123 if dtype == "double" else 0x7FC00123
    payload = np.array([nan_bits], np.uint64 if dtype == "double" else np.uint32).view(npd)[0]
    w0, h0 = np.full((7, cols), 1.5, npd), np.ones((7, cols), npd)
    h0[0] = 0          # row 0: G = 0, h = 0, eps = 0 -> 0 / 0
    w0[2:5] = -0.0     # rows 2, 3 (lr > 0) and 4 (lr < 0): the sign of w - p with p a zero
    for t in (w0, h0):  # row 5 is not named: its bits stay, whatever they are
        t[5, 0::2], t[5, 1::2] = -0.0, payload
    rows = np.array([START, START + 1, START + 2, START + 3, START + 1], np.int64)
    g = np.zeros((5, cols), npd)
    g[1], g[4] = big, big / 4  # row 1 twice: G = 1.25 big, G * G overflows
    g[3] = -0.0                # +0 + -0 is +0: G is +0 for row 2 and row 3 alike
    w1, h1 = replay_adagrad(w0, h0, rows - START, g, 0.5, 0.0)
    rows2, g2 = np.array([START + 4], np.int64), np.zeros((1, cols), npd)
    w2, h2 = replay_adagrad(w1, h1, rows2 - START, g2, -0.5, 0.0)  # u = -0, p = -0
    # the premises, from the replay
    assert np.isnan(w1[0]).all() and (h1[0] == 0).all()
    assert np.isinf(h1[1]).all() and (w1[1] == w0[1]).all()
    assert (bits(w1[2:4]) == bits(npd(-0.0))).all()  # -0 - (+0) = -0
    assert (bits(w2[4]) == 0).all()                  # -0 - (-0) = +0
    np.testing.assert_array_equal(bits(w2[5:]), bits(w0[5:]))
    pad = npd(777.0)
    w, h = pair(gpu, cols, dtype, 7)
    with w, h:
        write_image(w, gpu, w0, pad)
        write_image(h, gpu, h0, pad)
        push(w, h, gpu, rows, g, path, 0.5, 0.0)
        push(w, h, gpu, rows2, g2, path, -0.5, 0.0)
        pitch = C.c_int64()
        assert N.load().glint_shard_pitch(w.handle, C.byref(pitch)) == N.GLINT_OK
        assert (pitch.value > cols) == (cols == 67)  # only a row that is no multiple of 16 B is padded
        for sh, want, was in ((w, w2, w0), (h, h2, h0)):
            raw = read_image(sh, gpu, 7, pitch.value)
            assert_bits(raw[:5, :cols], want[:5])
            np.testing.assert_array_equal(bits(raw[5:, :cols]), bits(was[5:]))  # payload and sign kept
            assert (raw[:, cols:] == pad).all()  # neither read (no NaN) nor written


# ---- errors and arguments -------------------------------------------------------------------------------
def _error_input():
    rng = np.random.default_rng(3)
    cols = 6
    rows = rng.integers(START, START + SIZE, 100).astype(np.int64)
    rows[7] = START - 1
    rows[60] = START + SIZE
    return cols, rows, rng.standard_normal((100, cols))


def test_adagrad_push_errors_host(gpu):
    cols, rows, g = _error_input()
    w0, h0 = start_tables("float64", SIZE, cols)
    w, h = pair(gpu, cols, "double")
    with w, h:
        fill(w, w0)
        fill(h, h0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            w.updateRowsAdagrad(h, rows, g, LR, EPS)
        assert ei.value.record == 7
        assert_bits(w.to_numpy(), w0)  # a rejected message changes neither shard
        assert_bits(h.to_numpy(), h0)


def test_adagrad_push_errors_device(gpu):
    cols, rows, g = _error_input()
    w0, h0 = start_tables("float64", SIZE, cols)
    keep = np.ones(100, bool)
    keep[[7, 60]] = False
    want_w, want_h = replay_adagrad(w0, h0, rows[keep] - START, g[keep], LR, EPS)
    w, h = pair(gpu, cols, "double")
    with w, h:
        fill(w, w0)
        fill(h, h0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push(w, h, gpu, rows, g, "dev")
        assert ei.value.record == 7
        h.sync()  # the state shard was marked too; it has no error of its own
        assert_bits(w.to_numpy(), want_w)  # the other 98 records were applied
        assert_bits(h.to_numpy(), want_h)


def test_adagrad_push_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    g = np.ones(4, np.float64)
    rd, gd = torch.from_numpy(r).to(d), torch.from_numpy(g).to(d)
    host = lib.glint_mat_push_rows_adagrad
    devc = lambda *args: lib.glint_mat_push_rows_adagrad_dev(*args, None)  # noqa: E731
    calls = ((host, r.ctypes.data, g.ctypes.data), (devc, rd.data_ptr(), gd.data_ptr()))
    part = RangePartition(0, START, START + 10)
    w, h = pair(gpu, 4, "double", 10)
    with w, h:
        others = {
            "cols": PartialMatrix(part, 5, "double", gpu),
            "size": PartialMatrix(RangePartition(0, START, START + 11), 4, "double", gpu),
            "dtype": PartialMatrix(part, 4, "float", gpu),
            "start": PartialMatrix(RangePartition(0, START + 1, START + 11), 4, "double", gpu),
            "kind": PartialMatrix(CyclicPartition(0, 2, 20), 4, "double", gpu),
            "int": PartialMatrix(part, 4, "int", gpu), "int2": PartialMatrix(part, 4, "int", gpu),
            "long": PartialMatrix(part, 4, "long", gpu), "long2": PartialMatrix(part, 4, "long", gpu),
            "vector": PartialVector(part, "double", gpu), "vector2": PartialVector(part, "double", gpu),
        }
        cyc = [PartialMatrix(CyclicPartition(i, 2, 20), 4, "double", gpu) for i in (0, 1)]
        assert cyc[0].size == cyc[1].size == others["kind"].size == 10
        try:
            for call, pr, pg in calls:
                def ok(a, b, n=1, rows=pr, grads=pg, lr=0.1, eps=0.0, call=call):
                    return call(a, b, rows, grads, n, lr, eps)

                assert ok(None, h.handle) == N.GLINT_EINVAL
                assert ok(w.handle, None) == N.GLINT_EINVAL
                assert ok(w.handle, w.handle) == N.GLINT_EINVAL  # state is weights
                for name in ("cols", "size", "dtype", "start", "kind"):
                    assert ok(w.handle, others[name].handle) == N.GLINT_EINVAL, name
                    assert ok(others[name].handle, w.handle) == N.GLINT_EINVAL, name
                assert ok(cyc[0].handle, cyc[1].handle) == N.GLINT_EINVAL  # another cyclic index
                for name in ("int", "long", "vector"):
                    assert ok(others[name].handle, others[name + "2"].handle) == N.GLINT_EINVAL, name
                    assert ok(others[name].handle, h.handle) == N.GLINT_EINVAL, name
                assert ok(w.handle, h.handle, n=-1) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, n=(1 << 32) - 2048) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, rows=None) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, grads=None) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, lr=float("nan")) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, eps=-1e-300) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, eps=float("nan")) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, n=0, rows=None, grads=None) == N.GLINT_OK
            assert not w.to_numpy().any() and not h.to_numpy().any()
            # the Python layer: types, then shapes, before any call
            with pytest.raises(TypeError):
                others["int"].updateRowsAdagrad(others["long"], r, np.ones(4, np.int32), 0.1)
            with pytest.raises(TypeError):
                w.updateRowsAdagrad(h.handle, r, g, 0.1)  # state is a PartialMatrix
            with pytest.raises(TypeError):
                w.updateRowsAdagrad(h, rd, g, 0.1)  # grads on the host
            with pytest.raises(TypeError):
                w.updateRowsAdagrad(h, r, gd, 0.1)  # rows on the host
            with pytest.raises(TypeError):
                w.updateRowsAdagrad(h, rd, gd.to(torch.float32), 0.1)
            for bad in (np.ones(3), np.ones((2, 4)), np.ones(5)):
                with pytest.raises(ValueError):
                    w.updateRowsAdagrad(h, r, bad, 0.1)
            with pytest.raises(ValueError):
                w.updateRowsAdagrad(h, rd, torch.ones(5, dtype=torch.float64, device=d), 0.1)
            assert not w.to_numpy().any() and not h.to_numpy().any()
            # and what is valid: the default eps, a cyclic pair
            assert w.updateRowsAdagrad(h, r, g, 0.5) and w.updateRowsAdagrad(h, rd, gd, 0.5)
            zero = np.zeros((10, 4))
            want = replay_adagrad(*replay_adagrad(zero, zero, [0], g[None], 0.5, 1e-10), [0], g[None], 0.5, 1e-10)
            assert_bits(w.to_numpy(), want[0])
            assert_bits(h.to_numpy(), want[1])
            same = PartialMatrix(CyclicPartition(0, 2, 20), 4, "double", gpu)
            with same:
                assert cyc[0].updateRowsAdagrad(same, np.array([6], np.int64), g, 0.5, 0.0)  # local row 3
                want = replay_adagrad(zero, zero, [3], g[None], 0.5, 0.0)
                assert_bits(cyc[0].to_numpy(), want[0])
                assert_bits(same.to_numpy(), want[1])
        finally:
            for sh in list(others.values()) + cyc:
                sh.destroy()


def test_adagrad_push_views_of_one_slab(gpu):
    """Two views of one slab: overlapping rows are refused, disjoint rows work."""
    lib = N.load()
    cols = 32  # a row is 256 B: every row offset is a valid view offset
    r = np.array([START + 3, START + 3, START + 9], np.int64)
    g = np.random.default_rng(2).standard_normal((3, cols))
    slab = PartialMatrix(RangePartition(0, START, START + 30), cols, "double", gpu)
    views = [PartialMatrix.view(slab, RangePartition(1, START, START + 10), off) for off in (0, 5, 10)]
    try:
        a, over, b = views
        for x, y in ((a, over), (over, a), (over, b)):
            assert lib.glint_mat_push_rows_adagrad(x.handle, y.handle, r.ctypes.data, g.ctypes.data, 3, 0.1,
                                                   0.0) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows_adagrad(slab.handle, a.handle, r.ctypes.data, g.ctypes.data, 3, 0.1,
                                               0.0) == N.GLINT_EINVAL
        assert not a.to_numpy().any() and not b.to_numpy().any()
        assert a.updateRowsAdagrad(b, r, g, LR, EPS)
        zero = np.zeros((10, cols))
        want_w, want_h = replay_adagrad(zero, zero, r - START, g, LR, EPS)
        assert_bits(a.to_numpy(), want_w)
        assert_bits(b.to_numpy(), want_h)
    finally:
        for v in views:
            v.destroy()
        slab.destroy()


# ---- ordering across the two shards -----------------------------------------------------------------------
def _ordering_input(cols):
    rng = np.random.default_rng(12)
    er = rng.integers(START, START + 200, 1000).astype(np.int64)
    ec = rng.integers(0, cols, 1000).astype(np.int32)
    ev = rng.integers(1, 50, 1000).astype(np.float64)  # small integers: their sums are exact in any order
    rows = rng.integers(START, START + 200, 900).astype(np.int64)
    g = adagrad_inputs("float64", 900, cols, "ordering")
    h1 = np.zeros((SIZE, cols))
    np.add.at(h1, (er - START, ec), ev)
    want_w, want_h = replay_adagrad(np.zeros((SIZE, cols)), h1, rows - START, g, LR, EPS)
    assert (bits(want_w) != bits(replay_adagrad(np.zeros((SIZE, cols)), np.zeros((SIZE, cols)), rows - START, g, LR,
                                                EPS)[0])).mean() > 0.05  # the state push shows in the weights
    return er, ec, ev, rows, g, want_w, want_h


def test_adagrad_push_after_unwaited_state_push_host(gpu):
    """A message-sized push into the state shard, staged and not waited for, then the host Adagrad push:
    the step reads the state after that push."""
    cols = 9
    er, ec, ev, rows, g, want_w, want_h = _ordering_input(cols)
    w, h = pair(gpu, cols, "double")
    with w, h:
        ticket = h.push_async(er, ec, ev)
        assert w.updateRowsAdagrad(h, rows, g, LR, EPS)
        q = np.arange(START, START + SIZE, dtype=np.int64)
        got_h, got_w = h.getRows(q), w.getRows(q)
        h.wait(ticket)
        assert_bits(np.asarray(got_h), want_h, "state")
        assert_bits(np.asarray(got_w), want_w, "weights")


def test_adagrad_push_after_state_push_device(gpu):
    """The same with a device element push into the state shard on the stream, one sync at the end."""
    import torch
    cols = 9
    er, ec, ev, rows, g, want_w, want_h = _ordering_input(cols)
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    w, h = pair(gpu, cols, "double")
    with w, h:
        dev = [t(a) for a in (er, ec, ev, rows, g)]
        h.update(dev[0], dev[1], dev[2], sync=False)
        w.updateRowsAdagrad(h, dev[3], dev[4], LR, EPS, sync=False)
        w.sync(w._stream_of(dev[3]))
        h.sync(h._stream_of(dev[3]))
        assert_bits(h.to_numpy(), want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- launch count, stream order, client -------------------------------------------------------------------
def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_adagrad_push_profiling_id(gpu):
    rows = np.arange(START, START + 100, dtype=np.int64)
    w, h = pair(gpu, 4, "double")
    with w, h:
        for sh in (w, h):
            assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        counts = lambda: (_launches(w, N.GLINT_K_PUSH_ROWS), _launches(h, N.GLINT_K_PUSH_ROWS),  # noqa: E731
                          _launches(w, N.GLINT_K_PUSH_ROWS_AXPY), _launches(h, N.GLINT_K_PUSH_ROWS_AXPY))
        assert counts() == (0, 0, 0, 0)
        push(w, h, gpu, np.repeat(rows, 3), np.ones((300, 4)), "host")
        assert counts() == (1, 0, 0, 0)  # one fold launch, on the weights shard
        push(w, h, gpu, rows, np.ones((100, 4)), "dev")
        assert counts() == (2, 0, 0, 0)
        push(w, h, gpu, rows[:0], np.ones((0, 4)), "host")  # an empty call launches nothing
        push(w, h, gpu, rows[:0], np.ones((0, 4)), "dev")
        assert counts() == (2, 0, 0, 0)
        for sh in (w, h):
            assert sum(_launches(sh, k) for k in range(N.GLINT_K_COUNT)) == (2 if sh is w else 0)


def test_adagrad_push_stream_order(gpu):
    """An Adagrad push, an element push into the weights, an Adagrad push and two row pulls on one stream,
    one sync per shard at the end."""
    import torch
    cols = 9
    rng = np.random.default_rng(21)
    d = torch.device("cuda", gpu)
    r1, g1 = rng.integers(START, START + 200, 700).astype(np.int64), adagrad_inputs("float64", 700, cols, "stream1")
    er = rng.integers(START, START + 200, 1000).astype(np.int64)  # the same rows, by element
    ec = rng.integers(0, cols, 1000).astype(np.int32)
    ev = rng.standard_normal(1000)
    r2, g2 = rng.integers(START + 100, START + 300, 900).astype(np.int64), adagrad_inputs("float64", 900, cols,
                                                                                         "stream2")
    q = np.arange(START, START + 300, dtype=np.int64)
    zero = np.zeros((SIZE, cols))
    want_w, want_h = replay_adagrad(zero, zero, r1 - START, g1, LR, EPS)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["double"])
    ref.data[:] = want_w
    assert ref.update(er, ec, ev) == -1
    want_w, want_h = replay_adagrad(ref.data, want_h, r2 - START, g2, LR, EPS)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    w, h = pair(gpu, cols, "double")
    with w, h:
        dev = [t(a) for a in (r1, g1, er, ec, ev, r2, g2, q)]
        w.updateRowsAdagrad(h, dev[0], dev[1], LR, EPS, sync=False)
        w.update(dev[2], dev[3], dev[4], deterministic=True, sync=False)
        w.updateRowsAdagrad(h, dev[5], dev[6], LR, EPS, sync=False)
        out_w, out_h = w.getRows(dev[7], sync=False), h.getRows(dev[7], sync=False)
        w.sync(w._stream_of(dev[7]))
        h.sync(h._stream_of(dev[7]))
        assert_bits(out_w.cpu().numpy(), want_w[:300], "weights")
        assert_bits(out_h.cpu().numpy(), want_h[:300], "state")


def test_adagrad_push_client(gpu):
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 1000, 5000).astype(np.int64)
    g = adagrad_inputs("float64", 5000, 7, "client")
    c = Client([gpu] * 3)
    m, st = c.matrix(1000, 7, "double", modelsPerServer=2), c.matrix(1000, 7, "double", modelsPerServer=2)
    other = c.matrix(1000, 8, "double", modelsPerServer=2)
    try:
        assert m.nrOfPartitions == 6
        with pytest.raises(ValueError):
            m.pushAdagrad(other, rows, g, LR)
        zero = np.zeros((1000, 7))
        want_w, want_h = zero, zero
        for _ in range(2):
            assert m.pushAdagrad(st, rows, g, LR, EPS)
            want_w, want_h = replay_adagrad(want_w, want_h, rows, g, LR, EPS)
        assert_bits(m.pull(np.arange(1000)), want_w, "weights")
        assert_bits(st.pull(np.arange(1000)), want_h, "state")
    finally:
        for x in (m, st, other):
            x.destroy()
