"""Grouped row-sum pull (PartialMatrix.getRowsSum, glint_mat_pull_rows_sum*) on the GPU.

Expected values never come from the code under test: the shard's contents are read with to_numpy() /
getRows (pinned by the oracle elsewhere) and each group is replayed on the host, left to right from its
first row, in the shard's dtype (rowsum_cases.replay). Everything is compared bit for bit, as raw
integers.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from glint_amd.shard import check as check_rc
from ieee_cases import write_image
from rowsum_cases import ORDER_VECTORS, bits, replay, replay_groups

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
# 16-B path with 4 slices (Double) and with 3, the last one partial (Double 300); scalar path with 2
# slices, with 1 slice and with 1 column
COLS = [512, 300, 67, 7, 1]
START, SIZE = 1_000_003, 300
# 0 first, in the middle and last; one row; around the depth of 8 loads in flight; around the 64 row ids
# a wave reads at a time; several such blocks
LENS = [0, 1, 7, 0, 8, 9, 63, 64, 65, 129, 1000, 0]
SENTINEL = 0x5A


def np_dtype(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


@functools.lru_cache(maxsize=None)
def fill_values(dtype, cols, size=SIZE):
    """Random rows to push into a zeroed shard; read-only, shared. Int/Long lie near the type's limits
    so that sums of a few rows wrap; Float/Double span magnitudes so that the order of a sum shows."""
    rng = np.random.default_rng(zlib.crc32(f"rowsum/{dtype}/{cols}".encode()))
    npd = np_dtype(dtype)
    if np.issubdtype(npd, np.floating):
        v = (rng.standard_normal((size, cols)) * 10.0 ** rng.integers(-4, 5, (size, cols))).astype(npd)
    else:
        info = np.iinfo(npd)
        v = rng.integers(info.min, info.max, (size, cols), dtype=npd, endpoint=True)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def request(seed, size=SIZE):
    """(local rows, offsets) for LENS: rows drawn with repeats."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(LENS)]).astype(np.int64)
    local = rng.integers(0, size, int(offsets[-1])).astype(np.int64)
    local[offsets[4]:offsets[4] + 3] = local[offsets[4]]  # a row three times in a row in one group
    local.setflags(write=False)
    offsets.setflags(write=False)
    return local, offsets


def filled_shard(dtype, cols, gpu):
    sh = PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu)
    assert sh.updateRows(np.arange(START, START + SIZE, dtype=np.int64), fill_values(dtype, cols))
    return sh


def dev_tensors(gpu, *arrays):
    import torch
    d = torch.device("cuda", gpu)
    return [torch.from_numpy(np.array(a)).to(d) for a in arrays]


def assert_bits(got, exp, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    np.testing.assert_array_equal(bits(got), bits(exp), err_msg=what)


@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", DT)
def test_row_sum_parity(gpu, dtype, cols):
    local, offsets = request(7)
    rows = local + START
    with filled_shard(dtype, cols, gpu) as sh:
        table = sh.to_numpy()
        assert_bits(table, fill_values(dtype, cols), "the push of a zeroed shard stores the values")
        exp = replay_groups(table, local, offsets)
        if dtype in ("long", "int"):  # the sums did wrap: the exact sum of some group leaves the type
            exact = table[local[offsets[10]:offsets[11]]].astype(object).sum(axis=0)
            info = np.iinfo(table.dtype)
            assert any(x < info.min or x > info.max for x in exact)
        assert not exp[[0, 3, 11]].any()
        assert_bits(sh.getRowsSum(rows, offsets), exp, "host")
        t_rows, t_off = dev_tensors(gpu, rows, offsets)
        assert_bits(sh.getRowsSum(t_rows, t_off), exp, "device")


@pytest.mark.parametrize("dtype", ["double", "float"])
def test_row_sum_order_is_left_to_right(gpu, dtype):
    npd = np_dtype(dtype)
    v = ORDER_VECTORS[npd]
    rows = np.array([START + 5, START + 100, START + 7, START + 299], np.int64)
    vals = np.zeros((4, 3), npd)
    vals[:, 1] = v
    with PartialMatrix(RangePartition(2, START, START + SIZE), 3, dtype, gpu) as sh:
        assert sh.updateRows(rows, vals)
        stored = sh.getRows(rows)
        assert_bits(stored, vals)
        req = np.concatenate([rows, rows[::-1]])
        offsets = np.array([0, 4, 8], np.int64)
        exp = np.stack([replay(stored), replay(stored[::-1])])
        assert exp[0, 1] == 1 and exp[1, 1] == 0
        got = sh.getRowsSum(req, offsets)
        assert got[0, 1] == 1 and got[1, 1] == 0
        assert_bits(got, exp, "host")
        assert_bits(sh.getRowsSum(*dev_tensors(gpu, req, offsets)), exp, "device")


@pytest.mark.parametrize("dtype,cols", [("double", 4), ("float", 8), ("float", 7), ("double", 67)])
def test_row_sum_group_of_one_returns_stored_bits(gpu, dtype, cols):
    """-0.0, NaNs with a payload (quiet and signalling, either sign) and subnormals: a group of one row
    is the row pull, bit for bit. Written through the device pointer; the pitch padding is non-zero."""
    npd = np_dtype(dtype)
    if npd == np.float32:
        special = np.array([0x80000000, 0x7FC00001, 0xFFC00123, 0x7F800001, 0x00000001, 0x80000001, 0x807FFFFF],
                           np.uint32).view(np.float32)
    else:
        special = np.array([0x8000000000000000, 0x7FF8000000000123, 0xFFF8000000000123, 0x7FF0000000000001,
                            0x0000000000000001, 0x8000000000000001, 0x800FFFFFFFFFFFFF], np.uint64).view(np.float64)
    rng = np.random.default_rng(cols)
    img = special[rng.integers(0, special.size, (SIZE, cols))]
    img[3], img[4, 0] = special[0], special[1]
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        write_image(sh, gpu, img, 1)
        rows = np.arange(START, START + SIZE, dtype=np.int64)
        stored = sh.getRows(rows)
        assert_bits(stored, img)
        offsets = np.arange(SIZE + 1, dtype=np.int64)
        assert_bits(sh.getRowsSum(rows, offsets), stored, "host")
        assert_bits(sh.getRowsSum(*dev_tensors(gpu, rows, offsets)), stored, "device")


def test_row_sum_empty_calls(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    with filled_shard("double", 7, gpu) as sh:
        h = sh.handle
        zero = np.zeros(1, np.int64)
        out = np.full((3, 7), 9.0)
        # g == 0 writes nothing (out may be NULL, rows may be NULL)
        assert lib.glint_mat_pull_rows_sum(h, None, 0, zero.ctypes.data, 0, None) == N.GLINT_OK
        d_zero = torch.zeros(4, dtype=torch.int64, device=d)
        assert lib.glint_mat_pull_rows_sum_dev(h, None, 0, d_zero.data_ptr(), 0, None, None) == N.GLINT_OK
        assert sh.getRowsSum(np.zeros(0, np.int64), zero).shape == (0, 7)
        # n == 0 with g == 3: all +0
        z4 = np.zeros(4, np.int64)
        assert lib.glint_mat_pull_rows_sum(h, None, 0, z4.ctypes.data, 3, out.ctypes.data) == N.GLINT_OK
        assert_bits(out, np.zeros((3, 7)), "host")
        d_out = torch.full((3, 7), 9.0, dtype=torch.float64, device=d)
        st = torch.cuda.current_stream(d).cuda_stream
        assert lib.glint_mat_pull_rows_sum_dev(h, None, 0, d_zero.data_ptr(), 3, d_out.data_ptr(), st) == N.GLINT_OK
        sh.sync(st)
        assert_bits(d_out, np.zeros((3, 7)), "device")


@pytest.mark.parametrize("dtype,cols", [("double", 512), ("float", 300), ("int", 8)])
def test_row_sum_unaligned_out_gives_the_same_bits(gpu, dtype, cols):
    """The device call with `out` one element past a 16-B boundary takes the scalar path."""
    import torch
    lib = N.load()
    local, offsets = request(8)
    g = offsets.size - 1
    with filled_shard(dtype, cols, gpu) as sh:
        exp = replay_groups(sh.to_numpy(), local, offsets)
        t_rows, t_off = dev_tensors(gpu, local + START, offsets)
        st = sh._stream_of(t_rows)
        buf = torch.zeros(g * cols + 4, dtype=sh.torch_dtype, device=t_rows.device)
        assert buf.data_ptr() % 16 == 0
        for shift in (0, 1):
            view = buf[shift:shift + g * cols]
            assert lib.glint_mat_pull_rows_sum_dev(sh.handle, t_rows.data_ptr(), t_rows.numel(), t_off.data_ptr(), g,
                                                   view.data_ptr(), st) == N.GLINT_OK
            sh.sync(st)
            assert_bits(view.reshape(g, cols), exp, f"shift {shift}")


def test_row_sum_cyclic(gpu):
    part = CyclicPartition(1, 3, 900)
    cols, size = 67, 300
    local, offsets = request(9)
    rows = local * 3 + 1  # keys = 1 (mod 3)
    with PartialMatrix(part, cols, "long", gpu) as sh:
        assert sh.size == size
        assert sh.updateRows(np.arange(size, dtype=np.int64) * 3 + 1, fill_values("long", cols))
        table = sh.to_numpy()
        assert_bits(table, fill_values("long", cols))
        exp = replay_groups(table, local, offsets)
        assert_bits(sh.getRowsSum(rows, offsets), exp, "host")
        assert_bits(sh.getRowsSum(*dev_tensors(gpu, rows, offsets)), exp, "device")


def test_row_sum_errors_host(gpu):
    lib = N.load()
    cols = 6
    local, offsets = request(10)
    rows = local + START
    g = offsets.size - 1
    with filled_shard("long", cols, gpu) as sh:
        h = sh.handle

        def call(r, o, n=None, groups=g):
            out = np.zeros((g, cols), np.int64)
            out.view(np.uint8)[:] = SENTINEL
            rc = lib.glint_mat_pull_rows_sum(h, r.ctypes.data, r.size if n is None else n, o.ctypes.data, groups,
                                             out.ctypes.data)
            return rc, out

        untouched = np.zeros((g, cols), np.int64)
        untouched.view(np.uint8)[:] = SENTINEL
        bad = rows.copy()
        bad[40], bad[700] = START - 1, START + SIZE
        rc, out = call(bad, offsets)
        assert rc == N.GLINT_EOUTOFRANGE
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            check_rc(rc, h)
        assert ei.value.record == 40
        assert_bits(out, untouched, "nothing written")
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.getRowsSum(bad, offsets)
        assert ei.value.record == 40
        # a grp_ptr that breaks the rule: decreasing, grp_ptr[0] != 0, grp_ptr[g] != n
        dec = offsets.copy()
        dec[5], dec[6] = offsets[6], offsets[5]
        assert dec[6] < dec[5]
        first = offsets.copy()
        first[0] = 1
        last = offsets.copy()
        last[-1] -= 1
        for o in (dec, first, last):
            rc, out = call(rows, o)
            assert rc == N.GLINT_EINVAL
            assert_bits(out, untouched, "nothing written")
        with pytest.raises(ValueError):
            sh.getRowsSum(rows, dec)
        # the shard answers the next pull
        assert_bits(sh.getRowsSum(rows, offsets), replay_groups(sh.to_numpy(), local, offsets))


def test_row_sum_errors_device(gpu):
    cols = 6
    local, offsets = request(11)
    rows = local + START
    bad = rows.copy()
    where = [int(offsets[4]) + 2, int(offsets[9]) + 70, int(offsets[10]) + 500]  # three groups, first at 10
    bad[where] = [START + SIZE, START - 1, START + 10 * SIZE]
    with filled_shard("long", cols, gpu) as sh:
        table = np.concatenate([sh.to_numpy(), np.zeros((1, cols), np.int64)])  # row SIZE: the zeros a bad row counts as
        stand_in = local.copy()
        stand_in[where] = SIZE
        exp = replay_groups(table, stand_in, offsets)
        clean = replay_groups(table, local, offsets)
        assert (exp[[4, 9, 10]] != clean[[4, 9, 10]]).any(axis=1).all()
        t_rows, t_off = dev_tensors(gpu, bad, offsets)
        got = sh.getRowsSum(t_rows, t_off, sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(t_rows))
        assert ei.value.record == min(where)
        assert_bits(got, exp)  # the bad rows count as zeros; every other group is right
        sh.sync(sh._stream_of(t_rows))  # the error state was cleared
        # a malformed device grp_ptr is clamped to [0, n]; end < start is an empty group
        wild = offsets.copy()
        wild[0], wild[3], wild[-1] = -5, offsets[2] - 1, offsets[-1] + 1000
        t_good, t_wild = dev_tensors(gpu, rows, wild)
        fixed = np.clip(wild, 0, rows.size)
        exp = np.stack([replay(table[local[fixed[k]:max(fixed[k], fixed[k + 1])]]) for k in range(wild.size - 1)])
        assert_bits(sh.getRowsSum(t_good, t_wild), exp, "clamped")


def test_row_sum_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    o = np.array([0, 1], np.int64)
    out = np.zeros(4, np.float64)
    rd, od, outd = (torch.from_numpy(a).to(d) for a in (r, o, out))
    host = lambda h, rows, n, p, g, dst: lib.glint_mat_pull_rows_sum(h, rows, n, p, g, dst)  # noqa: E731
    dev = lambda h, rows, n, p, g, dst: lib.glint_mat_pull_rows_sum_dev(h, rows, n, p, g, dst, None)  # noqa: E731
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        assert host(vec.handle, r.ctypes.data, 1, o.ctypes.data, 1, out.ctypes.data) == N.GLINT_EINVAL
        assert dev(vec.handle, rd.data_ptr(), 1, od.data_ptr(), 1, outd.data_ptr()) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        h = sh.handle
        for call, (rows_p, off_p, out_p) in ((host, (r.ctypes.data, o.ctypes.data, out.ctypes.data)),
                                             (dev, (rd.data_ptr(), od.data_ptr(), outd.data_ptr()))):
            assert call(h, rows_p, -1, off_p, 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, -1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1 << 31, off_p, 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, 1 << 31, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, None, 1, out_p) == N.GLINT_EINVAL
            assert call(h, None, 1, off_p, 1, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, 1, None) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, 1, out_p) == N.GLINT_OK
        sh.sync(None)
        with pytest.raises(TypeError):  # offsets of the wrong dtype: no call is made
            sh.getRowsSum(rd, od.to(torch.int32))
        with pytest.raises(TypeError):  # mixing device rows and host offsets
            sh.getRowsSum(rd, o)


def test_row_sum_stream_order(gpu):
    """Row push, sum pull, row push, sum pull on one stream without a synchronisation in between: each
    pull sees exactly the pushes before it. The shard's contents at each point are read with the dense
    row pull on the same stream."""
    import torch
    cols = 67
    local, offsets = request(12)
    d = torch.device("cuda", gpu)
    all_rows = torch.arange(START, START + SIZE, dtype=torch.int64, device=d)
    v1 = torch.from_numpy(np.array(fill_values("long", cols))).to(d)
    v2 = torch.from_numpy(np.ascontiguousarray(fill_values("long", 300)[:, :cols])).to(d)
    t_rows, t_off = dev_tensors(gpu, local + START, offsets)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        stream = torch.cuda.Stream(d)
        stream.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(stream):
            sh.updateRows(all_rows, v1, sync=False)
            sum1 = sh.getRowsSum(t_rows, t_off, sync=False)
            snap1 = sh.getRows(all_rows, sync=False)
            sh.updateRows(all_rows, v2, sync=False)
            sum2 = sh.getRowsSum(t_rows, t_off, sync=False)
            snap2 = sh.getRows(all_rows, sync=False)
            sh.sync(stream.cuda_stream)
        snap1, snap2 = snap1.cpu().numpy(), snap2.cpu().numpy()
        assert (snap1 != snap2).any()
        assert_bits(sum1, replay_groups(snap1, local, offsets), "after the first push")
        assert_bits(sum2, replay_groups(snap2, local, offsets), "after the second push")


def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_row_sum_profiling_id(gpu):
    local, offsets = request(13)
    rows = local + START
    with filled_shard("double", 300, gpu) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        sh.getRows(rows)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 0  # a dense row pull is not a sum pull
        sh.getRowsSum(rows, offsets)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 1  # one call, one launch
        sh.getRowsSum(*dev_tensors(gpu, rows, offsets))
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 2
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SPARSE) == 0


def test_row_sum_client(gpu):
    rng = np.random.default_rng(14)
    table = rng.integers(-2**62, 2**62, (1000, 7)).astype(np.int64)
    m = glint_amd.Client([gpu] * 3).matrix(1000, 7, "long", modelsPerServer=2)
    assert m.nrOfPartitions == 6
    m.pushRows(np.arange(1000, dtype=np.int64), table)
    lens = rng.integers(0, 40, 200)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.integers(0, 1000, int(offsets[-1])).astype(np.int64)
    stored = m.pull(np.arange(1000, dtype=np.int64))
    assert_bits(m.pullSum(rows, offsets), replay_groups(stored, rows, offsets))  # wrapping adds commute
    m.destroy()
