"""Shard fill and seeded uniform init on the GPU (glint_shard_fill*, glint_shard_init_uniform*): every
result is compared as bits with the numpy replay (init_cases), over the whole allocation -- the named
elements hold the contract's values, every other row and the pitch padding keep a sentinel's bits."""
import ctypes as C

import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import (ArrayIndexOutOfBoundsException, BigMatrix, CyclicPartition, CyclicPartitioner, PartialMatrix,
                       PartialVector, RangePartition, RangePartitioner)
from adagrad_cases import replay_adagrad
from init_cases import bits, global_rows, replay_fill, replay_uniform, uniform_rows
from pair_cases import replay_pair_dot

pytestmark = pytest.mark.gpu

SEED = (0xC0FFEE << 32) | 0x1234567  # above 2^32: the second key word carries
LO, HI = -0.5 / 100, 0.5 / 100
UNIFORM = ("uniform", SEED, LO, HI)
PARTS = ["range", "range33", "cyclic"]
NAN = {4: 0x7FC12345, 8: 0x7FF8000012345678}


def make_part(kind, size):
    if kind == "range":
        return RangePartition(0, 1_000_003, 1_000_003 + size)
    if kind == "range33":
        return RangePartition(1, (1 << 33) + 5, (1 << 33) + 5 + size)  # the second counter word carries
    return CyclicPartition(2, 3, 3 * size)  # keys 2, 5, 8, ...


def make_shard(kind, size, cols, dtype, gpu):
    part = make_part(kind, size)
    return PartialVector(part, dtype, gpu) if cols == 0 else PartialMatrix(part, cols, dtype, gpu)


def pitch_of(sh):
    p = C.c_int64()
    assert N.load().glint_shard_pitch(sh.handle, C.byref(p)) == N.GLINT_OK
    return p.value


def _copy(src, dst, nbytes):
    segs = np.array([0, 0, nbytes], np.int64)
    assert N.load().glint_copy_segments_dev(src, dst, segs.ctypes.data_as(C.POINTER(C.c_int64)), 1, None) == N.GLINT_OK


def read_image(sh, gpu):
    """The shard's whole allocation through glint_shard_data: (size, pitch) raw bits."""
    import torch
    d = torch.device("cuda", gpu)
    dst = torch.empty((sh.size, pitch_of(sh)), dtype=sh.torch_dtype, device=d)
    _copy(sh.data_ptr(), dst.data_ptr(), dst.numel() * dst.element_size())
    torch.cuda.synchronize(d)
    return bits(dst.cpu().numpy())


def prefill(sh, gpu, salt=0):
    """Every element of the allocation, padding included, = a sentinel pattern with NaNs in it; returns it."""
    import torch
    it = np.dtype(sh.np_dtype).itemsize
    ut = {4: np.uint32, 8: np.uint64}[it]
    rng = np.random.default_rng(1000 + salt)
    img = rng.integers(0, np.iinfo(ut).max, (sh.size, pitch_of(sh)), dtype=ut, endpoint=True)
    img.reshape(-1)[::3] = NAN[it] ^ 0xBAD  # NaNs with payloads, in rows and padding alike
    d = torch.device("cuda", gpu)
    src = torch.from_numpy(img.view(sh.np_dtype)).to(d)
    _copy(src.data_ptr(), sh.data_ptr(), img.nbytes)
    torch.cuda.synchronize(d)
    return img


def expected(sh, img, op, local):
    """The allocation after `op` on local rows `local` (None: all): the replay on the first cols columns."""
    cols = max(sh.cols, 1)
    table = img[:, :cols].view(sh.np_dtype)
    local = np.arange(sh.size) if local is None else np.asarray(local, np.int64)
    if op[0] == "uniform":
        new = replay_uniform(table, local, global_rows(sh.partition, local), *op[1:])
    else:
        new = replay_fill(table, local, op[1])
    exp = img.copy()
    exp[:, :cols] = bits(new)
    return exp


def call(sh, gpu, op, local, path, sync=True):
    """op on local rows `local` (None: rows=None) through the Python methods, host arrays or device tensors."""
    import torch
    rows = None
    if local is not None:
        rows = np.ascontiguousarray(global_rows(sh.partition, np.asarray(local, np.int64)))
        if path == "dev":
            rows = torch.from_numpy(rows).to(torch.device("cuda", gpu))
    elif path == "dev":
        return call_dev_all(sh, gpu, op)
    if op[0] == "uniform":
        return sh.initUniform(op[1], op[2], op[3], rows=rows, sync=sync)
    return sh.fill(op[1], rows=rows, sync=sync)


def call_dev_all(sh, gpu, op):
    """rows == NULL, n == 0 through the device-resident C entry point on torch's current stream."""
    import torch
    lib = N.load()
    st = torch.cuda.current_stream(torch.device("cuda", gpu)).cuda_stream
    if op[0] == "uniform":
        rc = lib.glint_shard_init_uniform_dev(sh.handle, None, 0, op[1], op[2], op[3], st)
    else:
        v = np.asarray(op[1]).astype(sh.np_dtype).reshape(1)
        rc = lib.glint_shard_fill_dev(sh.handle, None, 0, v.ctypes.data, st)
    assert rc == N.GLINT_OK
    sh.sync(st)
    return True


def check(sh, gpu, op, local, path, salt=0):
    img = prefill(sh, gpu, salt)
    assert call(sh, gpu, op, local, path)
    got = read_image(sh, gpu)
    exp = expected(sh, img, op, local)
    bad = np.argwhere(got != exp)
    assert bad.size == 0, f"{bad.shape[0]} elements differ, first at (row, col) {bad[0].tolist()} of pitch {got.shape[1]}"


def row_lists(size):
    """Unordered with repeats, a strict subset, all rows (shuffled), n = 0."""
    rng = np.random.default_rng(size)
    some = rng.integers(0, size, max(1, size // 2))
    lists = [np.concatenate([some, some[:3], [size - 1, 0]]), np.arange(size)[::3][::-1], rng.permutation(size),
             np.zeros(0, np.int64)]
    return lists


# ---- shapes, partitions, padding, row lists -----------------------------------------------------------
@pytest.mark.parametrize("kind", PARTS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("cols", [1, 3, 4, 5, 67, 128, 130])
def test_uniform_shapes(gpu, cols, dtype, kind):
    for size in (1, 63, 64, 65, 1000):
        with make_shard(kind, size, cols, dtype, gpu) as sh:
            check(sh, gpu, UNIFORM, None, "host")
            check(sh, gpu, UNIFORM, None, "dev", 1)
            lists = row_lists(size)
            pick = lists if size == 65 else [lists[(size + cols) % 3]]
            for k, local in enumerate(pick):
                check(sh, gpu, UNIFORM, local, "host", 2 + k)
                check(sh, gpu, UNIFORM, local, "dev", 6 + k)


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_uniform_more_than_one_grid_pass(gpu, dtype):
    """cols = 130 with more (row, block) work items than the persistent grid has threads (8 blocks of 256
    per compute unit), and a stride that is no multiple of the blocks per row: a thread's (row, block)
    advance carries. The row count follows the device, so the case stays larger than one pass."""
    import torch
    threads = torch.cuda.get_device_properties(gpu).multi_processor_count * 8 * 256
    nb = (130 * np.dtype(dtype).itemsize + 15) // 16
    size = threads // nb + 1500
    assert threads % nb != 0
    with make_shard("range33" if dtype == "float32" else "cyclic", size, 130, dtype, gpu) as sh:
        check(sh, gpu, UNIFORM, None, "host")
        local = np.random.default_rng(2).permutation(size)
        check(sh, gpu, UNIFORM, np.concatenate([local, local[:100]])[:size - 7], "dev")


@pytest.mark.parametrize("kind", PARTS)
@pytest.mark.parametrize("dtype", ["float32", "float64"])
@pytest.mark.parametrize("size", [1, 1000])
def test_uniform_vector(gpu, size, dtype, kind):
    with make_shard(kind, size, 0, dtype, gpu) as sh:
        for path in ("host", "dev"):
            check(sh, gpu, UNIFORM, None, path)
            for k, local in enumerate(row_lists(size)):
                check(sh, gpu, UNIFORM, local, path, k)


def test_uniform_ranges(gpu):
    """lo == hi, a range rounded to Float on the host, a wide one; re-initialising is idempotent."""
    with make_shard("range", 65, 5, "float32", gpu) as sh:
        for lo, hi in ((0.1, 0.1), (-1e6, 3e7), (0.1, 0.7), (-3.0, -3.0 + 1e-7)):
            check(sh, gpu, ("uniform", 7, lo, hi), None, "host")
        img = prefill(sh, gpu)
        for _ in range(2):
            sh.initUniform(9, -1.0, 1.0, rows=np.array([1_000_003 + 4, 1_000_003 + 4, 1_000_003]))
        assert (read_image(sh, gpu) == expected(sh, img, ("uniform", 9, -1.0, 1.0), [4, 0])).all()


# ---- fill ---------------------------------------------------------------------------------------------
def fill_values(dtype):
    npd = np.dtype(dtype)
    if npd.kind == "f":
        ut = {4: np.uint32, 8: np.uint64}[npd.itemsize]
        return [npd.type(-0.0), np.array([NAN[npd.itemsize]], ut).view(npd)[0], npd.type(0.1)]
    return [npd.type(np.iinfo(npd).min), npd.type(-1), npd.type(7)]


@pytest.mark.parametrize("kind", ["range", "cyclic"])
@pytest.mark.parametrize("dtype", ["int32", "int64", "float32", "float64"])
def test_fill(gpu, dtype, kind):
    for cols, size in ((0, 1000), (1, 65), (5, 64), (67, 65), (130, 1000)):
        with make_shard(kind, size, cols, dtype, gpu) as sh:
            for k, v in enumerate(fill_values(dtype)):
                path = ("host", "dev")[k % 2]
                check(sh, gpu, ("fill", v), None, path, k)
                check(sh, gpu, ("fill", v), row_lists(size)[k], ("dev", "host")[k % 2], k + 3)
            check(sh, gpu, ("fill", fill_values(dtype)[0]), np.zeros(0, np.int64), "host")


def test_fill_int64_min_bits(gpu):
    with make_shard("range", 3, 3, "int64", gpu) as sh:
        sh.fill(np.iinfo(np.int64).min)
        assert (sh.to_numpy() == np.iinfo(np.int64).min).all()
    with make_shard("range", 3, 3, "float32", gpu) as sh:
        sh.fill(np.float32(-0.0))
        assert (bits(sh.to_numpy()) == 0x80000000).all()


@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_adagrad_from_filled_accumulator(gpu, dtype):
    """An Adagrad step on an accumulator filled with 0.1 equals the replay from that state."""
    size, cols, start = 200, 67, 1_000_003
    rng = np.random.default_rng(4)
    part = RangePartition(0, start, start + size)
    with PartialMatrix(part, cols, dtype, gpu) as w, PartialMatrix(part, cols, dtype, gpu) as h:
        w.initUniform(3, LO, HI)
        h.fill(0.1)
        w0 = uniform_rows(3, np.arange(size) + start, cols, LO, HI, dtype)
        h0 = np.full((size, cols), 0.1, dtype)
        local = rng.integers(0, size, 300)
        g = rng.standard_normal((300, cols)).astype(dtype)
        w.updateRowsAdagrad(h, local + start, g, 0.05, 1e-8)
        w1, h1 = replay_adagrad(w0, h0, local, g, 0.05, 1e-8)
        np.testing.assert_array_equal(bits(h.to_numpy()), bits(h1))
        np.testing.assert_array_equal(bits(w.to_numpy()), bits(w1))
        assert (h1 != h0).any() and np.isfinite(w1).all()


# ---- errors -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["range", "cyclic"])
@pytest.mark.parametrize("op", [UNIFORM, ("fill", 2.5)])
def test_bad_rows(gpu, kind, op):
    import torch
    size = 65
    with make_shard(kind, size, 5, "float64", gpu) as sh:
        good = global_rows(sh.partition, np.array([3, 64, 0, 7]))
        outside = [int(global_rows(sh.partition, size)), int(global_rows(sh.partition, 0)) - 3 * 7]
        rows = np.array([good[0], good[1], outside[0], good[2], outside[1], good[3]], np.int64)
        img = prefill(sh, gpu)
        with pytest.raises(ArrayIndexOutOfBoundsException) as e:  # host: the lowest index, nothing written
            (sh.initUniform(op[1], op[2], op[3], rows=rows) if op[0] == "uniform" else sh.fill(op[1], rows=rows))
        assert e.value.record == 2
        assert (read_image(sh, gpu) == img).all()
        t = torch.from_numpy(rows).to(torch.device("cuda", gpu))  # device: skipped, reported at sync
        with pytest.raises(ArrayIndexOutOfBoundsException) as e:
            (sh.initUniform(op[1], op[2], op[3], rows=t) if op[0] == "uniform" else sh.fill(op[1], rows=t))
        assert e.value.record == 2
        assert (read_image(sh, gpu) == expected(sh, img, op, [3, 64, 0, 7])).all()
        sh.sync()  # the error state was cleared by the sync that reported it


def test_einval(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    one = np.ones(1, np.float64)
    r = np.array([5], np.int64)
    rd = torch.from_numpy(r).to(d)
    inf, nan = float("inf"), float("nan")
    with make_shard("range", 10, 4, "float64", gpu) as f64, make_shard("range", 10, 4, "float32", gpu) as f32, \
            make_shard("range", 10, 4, "int32", gpu) as i32, make_shard("range", 10, 0, "int64", gpu) as i64:
        fills = [(lambda h, rows, n, v: lib.glint_shard_fill(h, rows, n, v), r.ctypes.data),
                 (lambda h, rows, n, v: lib.glint_shard_fill_dev(h, rows, n, v, None), rd.data_ptr())]
        unis = [(lambda h, rows, n, lo, hi: lib.glint_shard_init_uniform(h, rows, n, 1, lo, hi), r.ctypes.data),
                (lambda h, rows, n, lo, hi: lib.glint_shard_init_uniform_dev(h, rows, n, 1, lo, hi, None),
                 rd.data_ptr())]
        img = {sh: prefill(sh, gpu) for sh in (f64, f32, i32, i64)}
        for fn, rp in fills:
            assert fn(None, None, 0, one.ctypes.data) == N.GLINT_EINVAL
            assert fn(f64.handle, None, 0, None) == N.GLINT_EINVAL
            assert fn(f64.handle, None, 1, one.ctypes.data) == N.GLINT_EINVAL
            assert fn(f64.handle, rp, -1, one.ctypes.data) == N.GLINT_EINVAL
            assert fn(f64.handle, rp, 1 << 31, one.ctypes.data) == N.GLINT_EINVAL
        for fn, rp in unis:
            assert fn(None, None, 0, 0.0, 1.0) == N.GLINT_EINVAL
            assert fn(f64.handle, None, 1, 0.0, 1.0) == N.GLINT_EINVAL
            assert fn(f64.handle, rp, -1, 0.0, 1.0) == N.GLINT_EINVAL
            assert fn(f64.handle, rp, 1 << 31, 0.0, 1.0) == N.GLINT_EINVAL
            for sh in (i32, i64):
                assert fn(sh.handle, None, 0, 0.0, 1.0) == N.GLINT_EINVAL
            big = float(np.finfo(np.float64).max)
            for lo, hi in ((nan, 1.0), (0.0, nan), (-inf, 0.0), (0.0, inf), (1.0, 0.5), (-big, big)):
                assert fn(f64.handle, None, 0, lo, hi) == N.GLINT_EINVAL, (lo, hi)
                assert fn(f32.handle, None, 0, lo, hi) == N.GLINT_EINVAL, (lo, hi)
            # finite doubles that are infinite, or whose width is, after rounding to Float
            for lo, hi in ((0.0, 1e39), (-1e39, 0.0), (-3e38, 3e38)):
                assert fn(f32.handle, None, 0, lo, hi) == N.GLINT_EINVAL, (lo, hi)
        torch.cuda.synchronize(d)
        for sh in (f64, f32, i32, i64):
            assert (read_image(sh, gpu) == img[sh]).all()  # a refused call writes nothing
        with pytest.raises(ValueError):
            i32.initUniform(1, 0.0, 1.0)
        with pytest.raises(ValueError):
            f64.initUniform(-1, 0.0, 1.0)
        with pytest.raises(ValueError):
            f64.initUniform(1 << 64, 0.0, 1.0)
        with pytest.raises(TypeError):
            f64.fill(1.0, rows=rd.to(torch.int32))
        f64.initUniform(1, 0.25, 0.25)  # lo == hi is allowed
        assert (f64.to_numpy() == 0.25).all()


def test_slab_with_views(gpu):
    """A slab that has views refuses the host calls and takes the device calls, which its views then see."""
    import torch
    d = torch.device("cuda", gpu)
    start = 1 << 20
    with PartialMatrix(RangePartition(0, start, start + 64), 4, "float32", gpu) as slab:
        view = PartialMatrix.view(slab, RangePartition(1, start + 32, start + 64), 32)
        try:
            with pytest.raises(ValueError):
                slab.initUniform(1, 0.0, 1.0)
            with pytest.raises(ValueError):
                slab.fill(1.0)
            rows = torch.arange(start + 30, start + 40, dtype=torch.int64, device=d)
            slab.initUniform(5, 0.0, 1.0, rows=rows)
            want = uniform_rows(5, np.arange(start + 32, start + 40), 4, 0.0, 1.0, np.float32)
            np.testing.assert_array_equal(bits(view.getRows(np.arange(start + 32, start + 40))), bits(want))
            view.fill(2.0, rows=np.array([start + 33]))  # a view takes host calls
            assert (view.getRows(np.array([start + 33])) == 2.0).all()
        finally:
            view.destroy()


# ---- layout independence ------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", ["float32", "float64"])
def test_layout_independence(gpu, dtype):
    nrows, cols = 301, 67
    want = uniform_rows(SEED, np.arange(nrows), cols, LO, HI, dtype)
    got = []
    for partitioner in (RangePartitioner.apply(2, nrows), CyclicPartitioner.apply(3, nrows)):
        shards = [PartialMatrix(p, cols, dtype, gpu) for p in partitioner.all()]
        m = BigMatrix(partitioner, shards, nrows, cols)
        try:
            assert m.initUniform(SEED, LO, HI)
            got.append(m.pull(np.arange(nrows)))
            # a row list over both layouts: another seed on some rows, a fill on others
            some = np.array([300, 0, 150, 151, 299, 0, 17], np.int64)
            m.initUniform(SEED + 1, LO, HI, rows=some)
            m.fill(0.5, rows=np.array([2, 200], np.int64))
            exp = replay_uniform(want, some, some, SEED + 1, LO, HI)
            exp = replay_fill(exp, [2, 200], 0.5)
            np.testing.assert_array_equal(bits(m.pull(np.arange(nrows))), bits(exp))
        finally:
            m.destroy()
    np.testing.assert_array_equal(bits(got[0]), bits(got[1]))
    np.testing.assert_array_equal(bits(got[0]), bits(want))


# ---- order with the other calls -----------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "dev"])
def test_order_with_pushes_and_pulls(gpu, path):
    """push_async rows, initUniform on a row list that overlaps them, updateRows, getRows: the same sequence
    replayed. The device variant runs on a torch stream of its own."""
    import torch
    d = torch.device("cuda", gpu)
    size, cols, start = 100, 5, 1_000_003
    rng = np.random.default_rng(8)
    with PartialMatrix(RangePartition(0, start, start + size), cols, "float64", gpu) as sh:
        table = np.zeros((size, cols))
        pl = np.repeat(np.arange(0, 40), cols)  # whole rows 0..39 as element records, through the ring
        pc = np.tile(np.arange(cols, dtype=np.int32), 40)
        pv = rng.standard_normal(pl.size)
        ticket = sh.push_async(pl + start, pc, pv)
        table[pl, pc] += pv
        named = np.array([35, 20, 60, 20, 99], np.int64)  # overlaps the pushed rows
        ul = np.array([20, 21, 60, 61], np.int64)
        uv = rng.standard_normal((ul.size, cols))
        if path == "host":
            sh.initUniform(SEED, LO, HI, rows=named + start)
            sh.updateRows(ul + start, uv)
        else:
            stream = torch.cuda.Stream(d)
            with torch.cuda.stream(stream):
                sh.initUniform(SEED, LO, HI, rows=torch.from_numpy(named + start).to(d), sync=False)
                sh.updateRows(torch.from_numpy(ul + start).to(d), torch.from_numpy(uv).to(d), deterministic=True,
                              sync=False)
                sh.sync(stream.cuda_stream)
        table = replay_uniform(table, named, named + start, SEED, LO, HI)
        table[ul] += uv
        sh.wait(ticket)
        np.testing.assert_array_equal(bits(sh.getRows(np.arange(size) + start)), bits(table))


# ---- profiling ----------------------------------------------------------------------------------------
def launches(sh):
    out = []
    for kid in range(N.GLINT_K_COUNT):
        ms, cnt = C.c_double(), C.c_int64()
        assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
        out.append(cnt.value)
    return out


def test_profiling(gpu):
    import torch
    d = torch.device("cuda", gpu)
    with make_shard("range", 100, 5, "float32", gpu) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        rows = global_rows(sh.partition, np.array([5, 6, 5]))
        want = [0] * N.GLINT_K_COUNT
        for n_call, f in enumerate((lambda: sh.initUniform(1, 0.0, 1.0), lambda: sh.fill(1.0),
                                    lambda: sh.initUniform(1, 0.0, 1.0, rows=rows), lambda: sh.fill(1.0, rows=rows),
                                    lambda: sh.fill(1.0, rows=torch.from_numpy(rows).to(d)),
                                    lambda: sh.initUniform(1, 0.0, 1.0, rows=torch.from_numpy(rows).to(d))), 1):
            f()
            want[N.GLINT_K_PUSH_ROWS] = n_call  # one launch per call, under the row push's id only
            assert launches(sh) == want
        sh.fill(1.0, rows=np.zeros(0, np.int64))  # names nothing: launches nothing
        assert launches(sh) == want


# ---- end to end ---------------------------------------------------------------------------------------
def test_two_tables_score(gpu):
    """Two tables initialised with different seeds: the pair dot is non-zero and equals the replay."""
    na, nb, cols = 300, 200, 128
    pa, pb = RangePartitioner.apply(2, na), CyclicPartitioner.apply(2, nb)
    a = BigMatrix(pa, [PartialMatrix(p, cols, "float32", gpu) for p in pa.all()], na, cols)
    b = BigMatrix(pb, [PartialMatrix(p, cols, "float32", gpu) for p in pb.all()], nb, cols)
    try:
        a.initUniform(11, -0.5 / cols, 0.5 / cols)
        b.initUniform(12, -0.5 / cols, 0.5 / cols)
        A = uniform_rows(11, np.arange(na), cols, -0.5 / cols, 0.5 / cols, np.float32)
        B = uniform_rows(12, np.arange(nb), cols, -0.5 / cols, 0.5 / cols, np.float32)
        rng = np.random.default_rng(1)
        ra, rb = rng.integers(0, na, 500), rng.integers(0, nb, 500)
        got = a.pullPairDot(b, ra, rb)
        np.testing.assert_array_equal(bits(got), bits(replay_pair_dot(A[ra], B[rb])))
        assert (got != 0).all()
    finally:
        a.destroy()
        b.destroy()
