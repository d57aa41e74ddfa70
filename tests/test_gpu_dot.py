"""Row dot-product pull (PartialMatrix.getRowsDot, glint_mat_pull_rows_dot*) on the GPU.

Expected values never come from the code under test: the shard's contents are read with to_numpy()
(pinned by the oracle elsewhere) and every dot is replayed on the host in the contract's order, in the
shard's dtype (dot_cases.replay_dot). Everything is compared bit for bit, as raw integers; a NaN by
class.
"""
import ctypes as C
import functools

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from glint_amd.shard import check as check_rc
from dot_cases import (NOFMA_PLACES, assert_dot_bits, bits, fill_values, lane_width, nofma_case, replay_dot,
                       replay_self)
from ieee_cases import write_image

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
# 16-B path with whole strips (512); 16-B path with a partial last strip (300: Float has E = 4, Double and
# Long E = 2, Int E = 4); scalar path with two strips (67), with one (7) and with one column
COLS = [512, 300, 67, 7, 1]
START, SIZE = 1_000_003, 300
TILE = N.GLINT_DOT_QUERY_TILE
QS = [1, 3, TILE + 1]  # one query (its own kernel), a partial tile, a full tile and a partial one
NS = [0, 1, 5, 64, 65, 1000]
SENTINEL = 0x5A


def np_dtype(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


@functools.lru_cache(maxsize=None)
def request(seed, n, size=SIZE):
    """n local rows drawn with repeats (1000 requests of 300 rows repeat; short ones are made to)."""
    local = np.random.default_rng(seed).integers(0, size, n).astype(np.int64)
    if n >= 5:
        local[3] = local[1]
    local.setflags(write=False)
    return local


def queries(dtype, cols, q):
    return fill_values(np_dtype(dtype), cols, q, "x")


def filled_shard(dtype, cols, gpu, size=SIZE):
    sh = PartialMatrix(RangePartition(2, START, START + size), cols, dtype, gpu)
    assert sh.updateRows(np.arange(START, START + size, dtype=np.int64), fill_values(np_dtype(dtype), cols, size))
    return sh


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", gpu))


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", DT)
def test_row_dot_parity(gpu, dtype, cols):
    npd = np_dtype(dtype)
    with filled_shard(dtype, cols, gpu) as sh:
        table = sh.to_numpy()
        np.testing.assert_array_equal(bits(table), bits(fill_values(npd, cols, SIZE)))
        if dtype in ("long", "int"):  # the dots do wrap: some exact dot leaves the type
            exact = (table[:8].astype(object) * queries(dtype, cols, 1)[0].astype(object)).sum(axis=1)
            info = np.iinfo(npd)
            assert any(v < info.min or v > info.max for v in exact)
        for q in QS:
            x = queries(dtype, cols, q)
            full = replay_dot(table, x)  # every row of the shard against every query, once
            d_x = dev(gpu, x)
            for n in NS:
                local = request(100 * q + n, n)
                rows, exp = local + START, full[local]
                assert exp.shape == (n, q)
                assert_dot_bits(sh.getRowsDot(rows, x), exp, f"host q={q} n={n}")
                assert_dot_bits(sh.getRowsDot(dev(gpu, rows), d_x), exp, f"device q={q} n={n}")
            # x of shape (cols,) answers (n,)
            local = request(7, 65)
            assert_dot_bits(sh.getRowsDot(local + START, x[0]), full[local, 0], "host 1-d")
            assert_dot_bits(sh.getRowsDot(dev(gpu, local + START), d_x[0]), full[local, 0], "device 1-d")


@pytest.mark.parametrize("dtype,cols", [("double", 4100), ("float", 4100), ("double", 4099), ("float", 4099)])
def test_row_dot_long_rows(gpu, dtype, cols):
    """More strips than loads in flight, ending in a partial batch: 4100 is the 16-B path (Double 33
    strips, Float 17), 4099 the scalar path (65 strips); every count is odd, so both the batches of 8
    (one query per wave) and of 2 (a tile of queries) end in a partial one."""
    npd = np_dtype(dtype)
    assert lane_width(npd, cols) == (1 if cols % 2 else 16 // np.dtype(npd).itemsize)
    rows = np.array([START + 2, START, START + 2], np.int64)
    with filled_shard(dtype, cols, gpu, 3) as sh:
        table = sh.to_numpy()
        for q in (1, TILE + 1):
            x = queries(dtype, cols, q)
            exp = replay_dot(table, x)[rows - START]
            assert_dot_bits(sh.getRowsDot(rows, x), exp, f"host q={q}")
            assert_dot_bits(sh.getRowsDot(dev(gpu, rows), dev(gpu, x)), exp, f"device q={q}")
        assert_dot_bits(sh.getRowsDot(rows), replay_self(table)[rows - START], "self")


@pytest.mark.parametrize("dtype", ["double", "float"])
def test_row_dot_products_are_not_fused(gpu, dtype):
    """-b * 1 + a * a is exactly +0 when a * a is rounded (to b) before the add; a contracted
    multiply-add gives 2^-54 (Double) or 2^-24 (Float). Both paths, q = 1 and a tile of queries."""
    npd = np_dtype(dtype)
    for cols, c0, c1 in NOFMA_PLACES[npd]:
        row, x, fused = nofma_case(npd, cols, c0, c1)
        rows = np.array([START + 1, START], np.int64)
        with PartialMatrix(RangePartition(2, START, START + 2), cols, dtype, gpu) as sh:
            assert sh.updateRows(rows, np.stack([row, np.zeros(cols, npd)]))
            assert_dot_bits(sh.to_numpy()[1], row)
            exp = replay_dot(np.stack([row, np.zeros(cols, npd)]), x)
            assert bits(exp).tolist() == [0, 0] and fused > 0
            xs = np.stack([x] * (TILE + 1))
            for what, got in (("host", sh.getRowsDot(rows, x)), ("device", sh.getRowsDot(dev(gpu, rows), dev(gpu, x))),
                              ("host tile", sh.getRowsDot(rows, xs)[:, TILE]),
                              ("device tile", sh.getRowsDot(dev(gpu, rows), dev(gpu, xs))[:, 1])):
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                assert got[0] != fused, f"{what} cols={cols}: the product was fused into the add"
                assert_dot_bits(np.ascontiguousarray(got), exp, f"{what} cols={cols}")


@pytest.mark.parametrize("dtype,cols", [("double", 512), ("float", 300), ("double", 67), ("long", 7), ("int", 300)])
def test_row_dot_self(gpu, dtype, cols):
    local = request(21, 65)
    rows = local + START
    with filled_shard(dtype, cols, gpu) as sh:
        table = sh.to_numpy()
        exp = replay_self(table)[local]
        host = sh.getRowsDot(rows)
        assert host.shape == (65,)
        assert_dot_bits(host, exp, "host")
        assert_dot_bits(sh.getRowsDot(dev(gpu, rows)), exp, "device")
        for i in (0, 1, 64):  # the row against itself as a caller vector: the same bits
            assert_dot_bits(sh.getRowsDot(rows[i:i + 1], table[local[i]]), exp[i:i + 1], f"row {i} as x")
        if np.issubdtype(table.dtype, np.floating):
            assert (exp > 0).all()


@pytest.mark.parametrize("dtype,cols", [("double", 512), ("float", 300), ("int", 8), ("long", 300)])
def test_row_dot_unaligned_x_gives_the_same_bits(gpu, dtype, cols):
    """The device call with x one element past a 16-B boundary reads it element by element."""
    import torch
    lib = N.load()
    local = request(22, 65)
    with filled_shard(dtype, cols, gpu) as sh:
        table = sh.to_numpy()
        t_rows = dev(gpu, local + START)
        st = sh._stream_of(t_rows)
        for q in (1, TILE + 1):
            x = queries(dtype, cols, q)
            exp = replay_dot(table[local], x)
            buf = torch.zeros(q * cols + 4, dtype=sh.torch_dtype, device=t_rows.device)
            assert buf.data_ptr() % 16 == 0
            out = torch.empty((65, q), dtype=sh.torch_dtype, device=t_rows.device)
            for shift in (0, 1):
                view = buf[shift:shift + q * cols]
                view.copy_(dev(gpu, x).reshape(-1))
                assert view.data_ptr() % 16 == (0 if shift == 0 else view.element_size())
                assert lib.glint_mat_pull_rows_dot_dev(sh.handle, t_rows.data_ptr(), 65, view.data_ptr(), q,
                                                       out.data_ptr(), st) == N.GLINT_OK
                sh.sync(st)
                assert_dot_bits(out, exp, f"q={q} shift {shift}")
                assert_dot_bits(sh.getRowsDot(t_rows, view.view(q, cols)), exp, f"getRowsDot q={q} shift {shift}")


@pytest.mark.parametrize("dtype,cols", [("double", 300), ("float", 67), ("float", 512)])
def test_row_dot_answers_do_not_depend_on_q(gpu, dtype, cols):
    local = request(23, 65)
    rows = local + START
    with filled_shard(dtype, cols, gpu) as sh:
        x = queries(dtype, cols, 9)
        host = sh.getRowsDot(rows, x)
        device = sh.getRowsDot(dev(gpu, rows), dev(gpu, x)).cpu().numpy()
        assert host.shape == (65, 9)
        for j in range(9):
            one = sh.getRowsDot(rows, x[j])
            assert_dot_bits(np.ascontiguousarray(host[:, j]), one, f"host column {j}")
            assert_dot_bits(np.ascontiguousarray(device[:, j]), one, f"device column {j}")


@pytest.mark.parametrize("dtype,cols", [("double", 67), ("float", 67), ("double", 7), ("float", 7)])
def test_row_dot_never_reads_the_padding(gpu, dtype, cols):
    npd = np_dtype(dtype)
    img = np.array(fill_values(npd, cols, SIZE))
    rows = np.arange(START, START + SIZE, dtype=np.int64)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        write_image(sh, gpu, img, np.nan)
        assert_dot_bits(sh.to_numpy(), img)
        for q in (1, TILE + 1):
            x = queries(dtype, cols, q)
            exp = replay_dot(img, x)
            assert not np.isnan(exp).any()
            for what, got in (("host", sh.getRowsDot(rows, x)), ("device", sh.getRowsDot(dev(gpu, rows), dev(gpu, x)))):
                got = got.cpu().numpy() if hasattr(got, "cpu") else got
                assert not np.isnan(got).any(), what
                assert_dot_bits(got, exp, what)
        got = sh.getRowsDot(rows)
        assert not np.isnan(got).any()
        assert_dot_bits(got, replay_self(img), "self")


@pytest.mark.parametrize("cols", [8, 7])
def test_row_dot_edge_values(gpu, cols):
    """A subnormal product is kept, inf * 0 is NaN, an all-zero row (of either sign) gives +0."""
    table = np.zeros((4, cols), np.float32)
    table[0, 1] = 1e-30
    table[1, 2], table[1, 3] = np.inf, 1.0
    table[2] = -0.0
    x = np.zeros(cols, np.float32)
    x[1], x[2], x[3] = 1e-10, 0.0, 1.0
    rows = np.arange(START, START + 4, dtype=np.int64)
    with PartialMatrix(RangePartition(2, START, START + 4), cols, "float", gpu) as sh:
        write_image(sh, gpu, table, 1)
        exp = replay_dot(table, x)
        sub = np.float32(1e-30) * np.float32(1e-10)
        assert 0 < sub < np.finfo(np.float32).tiny and exp[0] == sub  # a subnormal, kept by the replay
        assert np.isnan(exp[1]) and bits(exp)[[2, 3]].tolist() == [0, 0]
        for what, got in (("host", sh.getRowsDot(rows, x)), ("device", sh.getRowsDot(dev(gpu, rows), dev(gpu, x)))):
            got = got.cpu().numpy() if hasattr(got, "cpu") else got
            assert got[0] == sub and np.isnan(got[1]), what
            assert_dot_bits(got, exp, what)
        # -0 * -0 = +0; the all-zero rows against any x and against themselves
        assert_dot_bits(sh.getRowsDot(rows), replay_self(table), "self")
        assert bits(sh.getRowsDot(rows[2:]))[:].tolist() == [0, 0]
        assert bits(sh.getRowsDot(rows[2:], -x)).tolist() == bits(replay_dot(table[2:], -x)).tolist() == [0, 0]


def test_row_dot_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    x = np.ones(4 * 2, np.float64)
    out = np.zeros(4, np.float64)
    rd, xd, outd = (torch.from_numpy(a).to(d) for a in (r, x, out))
    host = lambda h, rows, n, xp, q, dst: lib.glint_mat_pull_rows_dot(h, rows, n, xp, q, dst)  # noqa: E731
    devc = lambda h, rows, n, xp, q, dst: lib.glint_mat_pull_rows_dot_dev(h, rows, n, xp, q, dst, None)  # noqa: E731
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        assert host(vec.handle, r.ctypes.data, 1, x.ctypes.data, 1, out.ctypes.data) == N.GLINT_EINVAL
        assert devc(vec.handle, rd.data_ptr(), 1, xd.data_ptr(), 1, outd.data_ptr()) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        h = sh.handle
        for call, (rows_p, x_p, out_p) in ((host, (r.ctypes.data, x.ctypes.data, out.ctypes.data)),
                                           (devc, (rd.data_ptr(), xd.data_ptr(), outd.data_ptr()))):
            assert call(None, rows_p, 1, x_p, 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, -1, x_p, 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1 << 31, x_p, 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, x_p, 0, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, x_p, -1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, x_p, N.GLINT_DOT_MAX_QUERIES + 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, None, 2, out_p) == N.GLINT_EINVAL
            assert call(h, None, 1, x_p, 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, x_p, 1, None) == N.GLINT_EINVAL
            assert call(h, None, 0, x_p, 2, None) == N.GLINT_OK  # n == 0 writes nothing
            assert call(h, rows_p, 1, x_p, 2, out_p) == N.GLINT_OK
            assert call(h, rows_p, 1, None, 1, out_p) == N.GLINT_OK  # the self-dot
        sh.sync(None)
        assert not out.any() and not outd.cpu().numpy().any()  # an all-zero shard
        with pytest.raises(TypeError):  # x of the wrong dtype: no call is made
            sh.getRowsDot(rd, xd[:4].to(torch.float32))
        with pytest.raises(TypeError):  # mixing device rows and a host x
            sh.getRowsDot(rd, x[:4])
        with pytest.raises(ValueError):
            sh.getRowsDot(rd, xd[:3])
        with pytest.raises(ValueError):
            sh.getRowsDot(r, x[:3])
        with pytest.raises(ValueError):  # out of the wrong size
            sh.getRowsDot(rd, xd.view(2, 4), out=outd)


def test_row_dot_errors_host(gpu):
    lib = N.load()
    cols, q = 6, 3
    local = request(30, 1000)
    rows = local + START
    with filled_shard("long", cols, gpu) as sh:
        h = sh.handle
        x = queries("long", cols, q)
        untouched = np.zeros((1000, q), np.int64)
        untouched.view(np.uint8)[:] = SENTINEL
        out = untouched.copy()
        bad = rows.copy()
        bad[40], bad[700] = START - 1, START + SIZE
        rc = lib.glint_mat_pull_rows_dot(h, bad.ctypes.data, 1000, x.ctypes.data, q, out.ctypes.data)
        assert rc == N.GLINT_EOUTOFRANGE
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            check_rc(rc, h)
        assert ei.value.record == 40
        assert_dot_bits(out, untouched, "nothing written")
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.getRowsDot(bad, x)
        assert ei.value.record == 40
        # the shard answers the next pull
        assert_dot_bits(sh.getRowsDot(rows, x), replay_dot(sh.to_numpy(), x)[local])


def test_row_dot_errors_device(gpu):
    cols, q = 6, TILE + 1
    local = request(31, 1000)
    bad = local + START
    where = [700, 40, 41]
    bad[where] = [START + SIZE, START - 1, START + 10 * SIZE]
    with filled_shard("long", cols, gpu) as sh:
        x = queries("long", cols, q)
        exp = replay_dot(sh.to_numpy(), x)[local]
        assert exp[where].any(axis=1).all()
        exp[where] = 0  # a bad row answers q zeros
        got = sh.getRowsDot(dev(gpu, bad), dev(gpu, x), sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(got))
        assert ei.value.record == 40  # the lowest bad request, recorded once per request
        assert_dot_bits(got, exp)
        sh.sync(sh._stream_of(got))  # the error state was cleared
        norms = sh.getRowsDot(dev(gpu, bad), sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(got))
        assert ei.value.record == 40
        exp1 = replay_self(sh.to_numpy())[local]
        exp1[where] = 0
        assert_dot_bits(norms, exp1)


def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_row_dot_profiling_id(gpu):
    local = request(32, 65)
    rows = local + START
    with filled_shard("double", 300, gpu) as sh:
        x = queries("double", 300, TILE + 1)
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        sh.getRows(rows)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 0  # a dense row pull is not a dot pull
        sh.getRowsDot(rows, x)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 1  # one call, one launch
        sh.getRowsDot(dev(gpu, rows), dev(gpu, x))
        assert _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 2
        sh.getRowsDot(rows)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 3
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 0 and _launches(sh, N.GLINT_K_PULL_ROWS_SPARSE) == 0


def test_row_dot_cyclic(gpu):
    part = CyclicPartition(1, 3, 900)
    cols, size = 67, 300
    local = request(33, 1000)
    rows = local * 3 + 1  # keys = 1 (mod 3)
    with PartialMatrix(part, cols, "double", gpu) as sh:
        assert sh.size == size
        assert sh.updateRows(np.arange(size, dtype=np.int64) * 3 + 1, fill_values(np.float64, cols, size))
        x = queries("double", cols, 3)
        exp = replay_dot(sh.to_numpy(), x)[local]
        assert_dot_bits(sh.getRowsDot(rows, x), exp, "host")
        assert_dot_bits(sh.getRowsDot(dev(gpu, rows), dev(gpu, x)), exp, "device")


def test_row_dot_client(gpu):
    rng = np.random.default_rng(34)
    table = rng.integers(-2**62, 2**62, (1000, 7)).astype(np.int64)
    m = glint_amd.Client([gpu] * 3).matrix(1000, 7, "long", modelsPerServer=1)
    assert m.nrOfPartitions == 3
    m.pushRows(np.arange(1000, dtype=np.int64), table)
    rows = rng.integers(0, 1000, 500).astype(np.int64)
    x = rng.integers(-2**62, 2**62, (3, 7)).astype(np.int64)
    stored = m.pull(np.arange(1000, dtype=np.int64))
    assert_dot_bits(m.pullDot(rows, x), replay_dot(stored[rows], x))
    assert_dot_bits(m.pullDot(rows, x[1]), replay_dot(stored[rows], x[1]))
    assert_dot_bits(m.pullDot(rows), replay_self(stored[rows]))
    m.destroy()
