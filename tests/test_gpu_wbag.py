"""Weighted row-sum pull (PartialMatrix.getRowsSum(weights=...), glint_mat_pull_rows_wsum*) and grouped
row-dot pull (PartialMatrix.getRowsGroupDot, glint_mat_pull_rows_gdot*) on the GPU.

Expected values never come from the code under test: the shard's contents are read with to_numpy() /
getRows (pinned by the oracle elsewhere) and replayed on the host in the shard's dtype (wbag_cases): a
weighted sum left to right from its first rounded product, a grouped dot in the row dot's lane order.
Everything is compared bit for bit, as raw integers.
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
from dot_cases import NOFMA_PLACES, nofma_case, replay_dot
from group_cases import group_of
from ieee_cases import write_image
from wbag_cases import (ORDER_WEIGHTS, bits, clamped_groups, nofma_wcase, replay_gdot, replay_gdot_groups,
                        replay_wgroups)

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
# 16-B path with 4 slices (Double) and with a partial last slice (300); scalar path with 2 slices, with 1
# slice and with 1 column
COLS = [512, 300, 67, 7, 1]
START, SIZE = 1_000_003, 300
# 0 first, in the middle and last; one row; around the depth of 8 loads in flight; around the 64 row ids a
# sum's wave reads at a time; several batches; around the 4 records of a grouped dot's wave batch (3, 4, 5)
LENS = [0, 1, 7, 0, 8, 9, 63, 64, 65, 129, 1000, 3, 4, 5, 0]
SENTINEL = 0x5A


def np_dtype(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


@functools.lru_cache(maxsize=None)
def fill_values(dtype, rows, cols, what="table"):
    """Random values; read-only, shared. Int/Long lie anywhere in the type, so products and sums wrap;
    Float/Double span nine decades, so the order of a sum shows."""
    rng = np.random.default_rng(zlib.crc32(f"wbag/{what}/{dtype}/{rows}/{cols}".encode()))
    npd = np_dtype(dtype)
    if np.issubdtype(npd, np.floating):
        v = (rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-4, 5, (rows, cols))).astype(npd)
    else:
        info = np.iinfo(npd)
        v = rng.integers(info.min, info.max, (rows, cols), dtype=npd, endpoint=True)
    v.setflags(write=False)
    return v


def weights_for(dtype, n, what="weights"):
    return fill_values(dtype, n, 1, what).reshape(-1)


@functools.lru_cache(maxsize=None)
def request(seed, size=SIZE, lens=tuple(LENS)):
    """(local rows, offsets) for the lengths: rows drawn with repeats."""
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    local = rng.integers(0, size, int(offsets[-1])).astype(np.int64)
    if len(lens) > 4 and lens[4] >= 3:
        local[offsets[4]:offsets[4] + 3] = local[offsets[4]]  # a row three times in a row in one group
    local.setflags(write=False)
    offsets.setflags(write=False)
    return local, offsets


def filled_shard(dtype, cols, gpu):
    sh = PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu)
    assert sh.updateRows(np.arange(START, START + SIZE, dtype=np.int64), fill_values(dtype, SIZE, cols))
    return sh


def dev_tensors(gpu, *arrays):
    import torch
    d = torch.device("cuda", gpu)
    return [torch.from_numpy(np.array(a)).to(d) for a in arrays]


def assert_bits(got, exp, what=""):
    got = got.cpu().numpy() if hasattr(got, "cpu") else got
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    np.testing.assert_array_equal(bits(got), bits(exp), err_msg=what)


def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


# ---- weighted sum --------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", DT)
def test_wsum_parity(gpu, dtype, cols):
    local, offsets = request(7)
    rows = local + START
    w = weights_for(dtype, rows.size)
    with filled_shard(dtype, cols, gpu) as sh:
        table = sh.to_numpy()
        assert_bits(table, fill_values(dtype, SIZE, cols), "the push of a zeroed shard stores the values")
        exp = replay_wgroups(table, local, offsets, w)
        if dtype in ("long", "int"):  # the sums did wrap: the exact sum of some group leaves the type
            grp = slice(offsets[10], offsets[11])
            exact = (table[local[grp]].astype(object) * w[grp, None].astype(object)).sum(axis=0)
            info = np.iinfo(table.dtype)
            assert any(x < info.min or x > info.max for x in exact)
        assert not exp[[0, 3, 14]].any()
        assert_bits(sh.getRowsSum(rows, offsets, weights=w), exp, "host")
        t_rows, t_off, t_w = dev_tensors(gpu, rows, offsets, w)
        assert_bits(sh.getRowsSum(t_rows, t_off, weights=t_w), exp, "device")


@pytest.mark.parametrize("dtype", ["double", "float"])
def test_wsum_order_is_left_to_right(gpu, dtype):
    npd = np_dtype(dtype)
    w = ORDER_WEIGHTS[npd]
    rows = np.array([START + 5, START + 100, START + 7, START + 299], np.int64)
    with PartialMatrix(RangePartition(2, START, START + SIZE), 3, dtype, gpu) as sh:
        assert sh.updateRows(rows, np.ones((4, 3), npd))
        table = sh.to_numpy()
        req = np.concatenate([rows, rows[::-1]])
        ws = np.concatenate([w, w[::-1]])
        offsets = np.array([0, 4, 8], np.int64)
        exp = replay_wgroups(table, req - START, offsets, ws)
        assert (exp[0] == 1).all() and (exp[1] == 0).all()
        got = sh.getRowsSum(req, offsets, weights=ws)
        assert (got[0] == 1).all() and (got[1] == 0).all()
        assert_bits(got, exp, "host")
        t_req, t_off, t_w = dev_tensors(gpu, req, offsets, ws)
        assert_bits(sh.getRowsSum(t_req, t_off, weights=t_w), exp, "device")


@pytest.mark.parametrize("dtype,cols,col", [("double", 4, 1), ("double", 67, 64), ("float", 8, 5), ("float", 67, 66)])
def test_wsum_has_no_fused_multiply_add(gpu, dtype, cols, col):
    """The case's column sits in a 16-B lane (cols 4 / 8) and in a scalar-path column (cols 67)."""
    npd = np_dtype(dtype)
    w, r, fused = nofma_wcase(npd)
    rows = np.array([START + 1, START + 40], np.int64)
    vals = np.zeros((2, cols), npd)
    vals[:, col] = r
    offsets = np.array([0, 2], np.int64)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        assert sh.updateRows(rows, vals)
        exp = replay_wgroups(sh.to_numpy(), rows - START, offsets, w)
        assert not bits(exp).any() and fused > 0
        t_rows, t_off, t_w = dev_tensors(gpu, rows, offsets, w)
        for what, got in (("host", sh.getRowsSum(rows, offsets, weights=w)),
                          ("device", sh.getRowsSum(t_rows, t_off, weights=t_w).cpu().numpy())):
            assert got[0, col] != fused, f"{what}: the product was fused into the add"
            assert_bits(got, exp, what)


def finite_image(npd, cols):
    """-0.0, +/-0, subnormals of both signs, the smallest normal, +/-MAX and ordinary values; no NaN, no inf."""
    if npd == np.float32:
        special = np.array([0x80000000, 0x00000000, 0x00000001, 0x80000001, 0x807FFFFF, 0x007FFFFF, 0x00800000,
                            0x7F7FFFFF, 0xFF7FFFFF, 0x3F800000, 0xC0490FDB], np.uint32).view(np.float32)
    else:
        special = np.array([0x8000000000000000, 0, 0x0000000000000001, 0x8000000000000001, 0x800FFFFFFFFFFFFF,
                            0x000FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF,
                            0x3FF0000000000000, 0xC00921FB54442D18], np.uint64).view(np.float64)
    rng = np.random.default_rng(cols)
    img = special[rng.integers(0, special.size, (SIZE, cols))]
    img[3], img[4, 0] = special[0], special[2]
    return img, special


@pytest.mark.parametrize("dtype,cols", [("double", 4), ("float", 8), ("float", 7), ("double", 67)])
def test_wsum_of_ones_weights_is_the_unweighted_sum(gpu, dtype, cols):
    """On a finite table 1 * r is r bit for bit, so weights of ones reproduce getRowsSum: the new path tied
    to the pinned one. Written through the device pointer; the pitch padding is non-zero."""
    npd = np_dtype(dtype)
    img, _ = finite_image(npd, cols)
    local, offsets = request(15)
    rows = local + START
    ones = np.ones(rows.size, npd)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        write_image(sh, gpu, img, 1)
        assert_bits(sh.to_numpy(), img)
        plain = sh.getRowsSum(rows, offsets)
        assert_bits(plain, replay_wgroups(img, local, offsets, ones), "the replay agrees")
        assert_bits(sh.getRowsSum(rows, offsets, weights=ones), plain, "host")
        t_rows, t_off, t_w = dev_tensors(gpu, rows, offsets, ones)
        assert_bits(sh.getRowsSum(t_rows, t_off, weights=t_w), plain, "device")


@pytest.mark.parametrize("dtype,cols", [("double", 4), ("float", 7)])
def test_wsum_group_of_one_returns_stored_bits(gpu, dtype, cols):
    """Every non-NaN special: a group of one row with weight 1 is the row's stored bits (the first term is
    the product, not 0 + product), and weight -1 on +0.0 gives -0.0."""
    npd = np_dtype(dtype)
    img, special = finite_image(npd, cols)
    inf = np.array([np.inf, -np.inf], npd)
    img[5, :2], img[6] = inf, special[1]  # +/-inf, and a row of +0.0
    rows = np.arange(START, START + SIZE, dtype=np.int64)
    offsets = np.arange(SIZE + 1, dtype=np.int64)
    w = np.ones(SIZE, npd)
    w[6] = -1
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        write_image(sh, gpu, img, 1)
        stored = sh.getRows(rows)
        assert_bits(stored, img)
        exp = stored.copy()
        exp[6] = -0.0
        assert (bits(exp[6]) == bits(special[:1])[0]).all() and not bits(stored[6]).any()
        assert_bits(sh.getRowsSum(rows, offsets, weights=w), exp, "host")
        assert_bits(sh.getRowsSum(*dev_tensors(gpu, rows, offsets), weights=dev_tensors(gpu, w)[0]), exp, "device")


def test_wsum_empty_calls(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    with filled_shard("double", 7, gpu) as sh:
        h = sh.handle
        zero = np.zeros(1, np.int64)
        out = np.full((3, 7), 9.0)
        # g == 0 writes nothing (out, rows and coef may be NULL)
        assert lib.glint_mat_pull_rows_wsum(h, None, 0, zero.ctypes.data, 0, None, None) == N.GLINT_OK
        d_zero = torch.zeros(4, dtype=torch.int64, device=d)
        assert lib.glint_mat_pull_rows_wsum_dev(h, None, 0, d_zero.data_ptr(), 0, None, None, None) == N.GLINT_OK
        assert sh.getRowsSum(np.zeros(0, np.int64), zero, weights=np.zeros(0)).shape == (0, 7)
        # n == 0 with g == 3: all +0
        z4 = np.zeros(4, np.int64)
        assert lib.glint_mat_pull_rows_wsum(h, None, 0, z4.ctypes.data, 3, None, out.ctypes.data) == N.GLINT_OK
        assert_bits(out, np.zeros((3, 7)), "host")
        d_out = torch.full((3, 7), 9.0, dtype=torch.float64, device=d)
        st = torch.cuda.current_stream(d).cuda_stream
        assert lib.glint_mat_pull_rows_wsum_dev(h, None, 0, d_zero.data_ptr(), 3, None, d_out.data_ptr(),
                                                st) == N.GLINT_OK
        sh.sync(st)
        assert_bits(d_out, np.zeros((3, 7)), "device")
        empty = torch.zeros(0, dtype=torch.int64, device=d)
        got = sh.getRowsSum(empty, d_zero, weights=torch.zeros(0, dtype=torch.float64, device=d))
        assert_bits(got, np.zeros((3, 7)), "device, through the shard")


@pytest.mark.parametrize("dtype,cols", [("double", 512), ("float", 300), ("int", 8)])
def test_wsum_unaligned_out_gives_the_same_bits(gpu, dtype, cols):
    """The device call with `out` one element past a 16-B boundary takes the scalar path."""
    import torch
    lib = N.load()
    local, offsets = request(8)
    g = offsets.size - 1
    w = weights_for(dtype, local.size)
    with filled_shard(dtype, cols, gpu) as sh:
        exp = replay_wgroups(sh.to_numpy(), local, offsets, w)
        t_rows, t_off, t_w = dev_tensors(gpu, local + START, offsets, w)
        st = sh._stream_of(t_rows)
        buf = torch.zeros(g * cols + 4, dtype=sh.torch_dtype, device=t_rows.device)
        assert buf.data_ptr() % 16 == 0
        for shift in (0, 1):
            view = buf[shift:shift + g * cols]
            assert lib.glint_mat_pull_rows_wsum_dev(sh.handle, t_rows.data_ptr(), t_rows.numel(), t_off.data_ptr(), g,
                                                    t_w.data_ptr(), view.data_ptr(), st) == N.GLINT_OK
            sh.sync(st)
            assert_bits(view.reshape(g, cols), exp, f"shift {shift}")


def cyclic_shard(gpu, cols):
    sh = PartialMatrix(CyclicPartition(1, 3, 900), cols, "long", gpu)
    assert sh.size == SIZE
    assert sh.updateRows(np.arange(SIZE, dtype=np.int64) * 3 + 1, fill_values("long", SIZE, cols))
    return sh


def test_wsum_cyclic(gpu):
    cols = 67
    local, offsets = request(9)
    rows = local * 3 + 1  # keys = 1 (mod 3)
    w = weights_for("long", rows.size)
    with cyclic_shard(gpu, cols) as sh:
        exp = replay_wgroups(sh.to_numpy(), local, offsets, w)
        assert_bits(sh.getRowsSum(rows, offsets, weights=w), exp, "host")
        t_rows, t_off, t_w = dev_tensors(gpu, rows, offsets, w)
        assert_bits(sh.getRowsSum(t_rows, t_off, weights=t_w), exp, "device")


def test_wbag_stream_order(gpu):
    """Row push, both pulls, row push, both pulls on one stream without a synchronisation in between: each
    pull sees exactly the pushes before it. The shard's contents at each point are read with the dense row
    pull on the same stream."""
    import torch
    cols = 67
    local, offsets = request(12)
    g = offsets.size - 1
    d = torch.device("cuda", gpu)
    all_rows = torch.arange(START, START + SIZE, dtype=torch.int64, device=d)
    v1 = torch.from_numpy(np.array(fill_values("long", SIZE, cols))).to(d)
    v2 = torch.from_numpy(np.array(fill_values("long", SIZE, cols, "second"))).to(d)
    w, x = weights_for("long", local.size), fill_values("long", g, cols, "x")
    t_rows, t_off, t_w, t_x = dev_tensors(gpu, local + START, offsets, w, x)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        stream = torch.cuda.Stream(d)
        stream.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(stream):
            sh.updateRows(all_rows, v1, sync=False)
            sum1 = sh.getRowsSum(t_rows, t_off, sync=False, weights=t_w)
            dot1 = sh.getRowsGroupDot(t_rows, t_off, t_x, sync=False)
            snap1 = sh.getRows(all_rows, sync=False)
            sh.updateRows(all_rows, v2, sync=False)
            sum2 = sh.getRowsSum(t_rows, t_off, sync=False, weights=t_w)
            dot2 = sh.getRowsGroupDot(t_rows, t_off, t_x, sync=False)
            snap2 = sh.getRows(all_rows, sync=False)
            sh.sync(stream.cuda_stream)
        snap1, snap2 = snap1.cpu().numpy(), snap2.cpu().numpy()
        assert (snap1 != snap2).any()
        assert_bits(sum1, replay_wgroups(snap1, local, offsets, w), "sum after the first push")
        assert_bits(sum2, replay_wgroups(snap2, local, offsets, w), "sum after the second push")
        assert_bits(dot1, replay_gdot_groups(snap1, local, offsets, x), "dot after the first push")
        assert_bits(dot2, replay_gdot_groups(snap2, local, offsets, x), "dot after the second push")


def test_wbag_profiling_ids(gpu):
    local, offsets = request(13)
    rows = local + START
    w, x = weights_for("double", rows.size), fill_values("double", offsets.size - 1, 300, "x")
    pulls = (N.GLINT_K_VEC_PULL, N.GLINT_K_MAT_PULL, N.GLINT_K_MAT_PULL_ROWS, N.GLINT_K_PULL_ROWS_SPARSE)
    with filled_shard("double", 300, gpu) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        sh.getRowsSum(rows, offsets, weights=w)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 1  # one call, one launch
        t_rows, t_off, t_w, t_x = dev_tensors(gpu, rows, offsets, w, x)
        sh.getRowsSum(t_rows, t_off, weights=t_w)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 2
        assert _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 0
        sh.getRowsGroupDot(rows, offsets, x)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 1
        sh.getRowsGroupDot(t_rows, t_off, t_x)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 2
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 2
        assert all(_launches(sh, k) == 0 for k in pulls)


# ---- grouped dot ---------------------------------------------------------------------------------
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", DT)
def test_gdot_parity(gpu, dtype, cols):
    local, offsets = request(21)
    rows = local + START
    x = fill_values(dtype, offsets.size - 1, cols, "x")
    with filled_shard(dtype, cols, gpu) as sh:
        table = sh.to_numpy()
        exp = replay_gdot_groups(table, local, offsets, x)
        group = group_of(offsets, rows.size)
        for i in (0, 1, 8, 700):  # the vectorised replay is replay_dot per record
            assert bits(exp[i:i + 1])[0] == bits(replay_dot(table[local[i]][None, :], x[group[i]]))[0]
        assert_bits(sh.getRowsGroupDot(rows, offsets, x), exp, "host")
        assert_bits(sh.getRowsGroupDot(rows, offsets, x.reshape(-1)), exp, "host, x flat")
        t_rows, t_off, t_x = dev_tensors(gpu, rows, offsets, x)
        assert_bits(sh.getRowsGroupDot(t_rows, t_off, t_x), exp, "device")


@pytest.mark.parametrize("dtype,cols", [("double", 512), ("float", 300), ("double", 67), ("int", 7)])
def test_gdot_is_the_row_dot_per_record(gpu, dtype, cols):
    """Equality with getRowsDot of one row and its group's vector: the new path tied to the pinned one."""
    local, offsets = request(22)
    rows = local + START
    x = fill_values(dtype, offsets.size - 1, cols, "x")
    group = group_of(offsets, rows.size)
    with filled_shard(dtype, cols, gpu) as sh:
        got = sh.getRowsGroupDot(rows, offsets, x)
        dev = sh.getRowsGroupDot(*dev_tensors(gpu, rows, offsets, x)).cpu().numpy()
        assert rows.size == 1358
        for i in (0, 1, 3, 4, 5, 7, 8, 9, 16, 88, 89, 346, 1345, 1346, 1357):  # batch and group edges, the last record
            one = sh.getRowsDot(rows[i:i + 1], x[group[i]])
            assert bits(got[i:i + 1])[0] == bits(one)[0] == bits(dev[i:i + 1])[0], i


@pytest.mark.parametrize("dtype", ["double", "float"])
def test_gdot_has_no_fused_multiply_add(gpu, dtype):
    npd = np_dtype(dtype)
    for cols, c0, c1 in NOFMA_PLACES[npd]:
        row, x, fused = nofma_case(npd, cols, c0, c1)
        rows = np.array([START + 1, START, START + 1], np.int64)
        offsets = np.array([0, 1, 3], np.int64)
        xs = np.stack([x, x])
        with PartialMatrix(RangePartition(2, START, START + 2), cols, dtype, gpu) as sh:
            assert sh.updateRows(rows[:2], np.stack([row, np.zeros(cols, npd)]))
            exp = replay_gdot_groups(sh.to_numpy(), rows - START, offsets, xs)
            assert bits(exp).tolist() == [0, 0, 0] and fused > 0
            for what, got in (("host", sh.getRowsGroupDot(rows, offsets, xs)),
                              ("device", sh.getRowsGroupDot(*dev_tensors(gpu, rows, offsets, xs)).cpu().numpy())):
                assert got[0] != fused and got[2] != fused, f"{what} cols={cols}: the product was fused into the add"
                assert_bits(got, exp, f"{what} cols={cols}")


@pytest.mark.parametrize("dtype,cols", [("double", 512), ("float", 300), ("int", 8)])
def test_gdot_unaligned_x_gives_the_same_bits(gpu, dtype, cols):
    """The device call with `x` one element past a 16-B boundary reads it element by element."""
    import torch
    lib = N.load()
    local, offsets = request(23)
    g, n = offsets.size - 1, local.size
    x = fill_values(dtype, g, cols, "x")
    with filled_shard(dtype, cols, gpu) as sh:
        exp = replay_gdot_groups(sh.to_numpy(), local, offsets, x)
        t_rows, t_off = dev_tensors(gpu, local + START, offsets)
        st = sh._stream_of(t_rows)
        buf = torch.zeros(g * cols + 4, dtype=sh.torch_dtype, device=t_rows.device)
        assert buf.data_ptr() % 16 == 0
        for shift in (0, 1):
            view = buf[shift:shift + g * cols]
            view.copy_(torch.from_numpy(np.array(x)).reshape(-1))
            out = torch.zeros(n, dtype=sh.torch_dtype, device=t_rows.device)
            assert lib.glint_mat_pull_rows_gdot_dev(sh.handle, t_rows.data_ptr(), n, t_off.data_ptr(), g,
                                                    view.data_ptr(), out.data_ptr(), st) == N.GLINT_OK
            sh.sync(st)
            assert_bits(out, exp, f"shift {shift}")


def test_gdot_groups_of_one(gpu):
    """130 groups of one record: the group changes at every record of every wave batch."""
    cols = 67
    local, offsets = request(24, lens=(1,) * 130)
    rows = local + START
    x = fill_values("double", 130, cols, "x")
    with filled_shard("double", cols, gpu) as sh:
        exp = replay_gdot_groups(sh.to_numpy(), local, offsets, x)
        assert_bits(sh.getRowsGroupDot(rows, offsets, x), exp, "host")
        assert_bits(sh.getRowsGroupDot(*dev_tensors(gpu, rows, offsets, x)), exp, "device")


def test_gdot_cyclic(gpu):
    cols = 67
    local, offsets = request(25)
    rows = local * 3 + 1
    x = fill_values("long", offsets.size - 1, cols, "x")
    with cyclic_shard(gpu, cols) as sh:
        exp = replay_gdot_groups(sh.to_numpy(), local, offsets, x)
        assert_bits(sh.getRowsGroupDot(rows, offsets, x), exp, "host")
        assert_bits(sh.getRowsGroupDot(*dev_tensors(gpu, rows, offsets, x)), exp, "device")


def test_gdot_empty_calls(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    with filled_shard("double", 7, gpu) as sh:
        h = sh.handle
        z4 = np.zeros(4, np.int64)
        d_z4 = torch.zeros(4, dtype=torch.int64, device=d)
        # n == 0 writes nothing (rows, x and out may be NULL)
        assert lib.glint_mat_pull_rows_gdot(h, None, 0, z4.ctypes.data, 3, None, None) == N.GLINT_OK
        assert lib.glint_mat_pull_rows_gdot_dev(h, None, 0, d_z4.data_ptr(), 3, None, None, None) == N.GLINT_OK
        assert sh.getRowsGroupDot(np.zeros(0, np.int64), z4, np.zeros((3, 7))).shape == (0,)
        with pytest.raises(ValueError):
            sh.getRowsGroupDot(np.zeros(0, np.int64), z4, np.zeros((3, 6)))
        with pytest.raises(ValueError):
            sh.getRowsGroupDot(np.zeros(0, np.int64), z4, np.zeros((2, 7)))


# ---- errors, both operations ---------------------------------------------------------------------
def test_wbag_errors_host(gpu):
    lib = N.load()
    cols = 6
    local, offsets = request(10)
    rows = local + START
    g, n = offsets.size - 1, rows.size
    w, x = weights_for("long", n), fill_values("long", g, cols, "x")
    with filled_shard("long", cols, gpu) as sh:
        h = sh.handle

        def wsum(r, o):
            out = np.zeros((g, cols), np.int64)
            out.view(np.uint8)[:] = SENTINEL
            return lib.glint_mat_pull_rows_wsum(h, r.ctypes.data, r.size, o.ctypes.data, g, w.ctypes.data,
                                                out.ctypes.data), out

        def gdot(r, o):
            out = np.zeros(n, np.int64)
            out.view(np.uint8)[:] = SENTINEL
            return lib.glint_mat_pull_rows_gdot(h, r.ctypes.data, r.size, o.ctypes.data, g, x.ctypes.data,
                                                out.ctypes.data), out

        bad = rows.copy()
        bad[40], bad[700] = START - 1, START + SIZE
        dec = offsets.copy()
        dec[5], dec[6] = offsets[6], offsets[5]
        assert dec[6] < dec[5]
        first = offsets.copy()
        first[0] = 1
        last = offsets.copy()
        last[-1] -= 1
        for call, pull in ((wsum, lambda r, o: sh.getRowsSum(r, o, weights=w)),
                           (gdot, lambda r, o: sh.getRowsGroupDot(r, o, x))):
            rc, out = call(bad, offsets)
            assert rc == N.GLINT_EOUTOFRANGE
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                check_rc(rc, h)
            assert ei.value.record == 40
            assert (out.view(np.uint8) == SENTINEL).all(), "nothing written"
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                pull(bad, offsets)
            assert ei.value.record == 40
            for o in (dec, first, last):  # a grp_ptr that breaks the rule
                rc, out = call(rows, o)
                assert rc == N.GLINT_EINVAL
                assert (out.view(np.uint8) == SENTINEL).all(), "nothing written"
            with pytest.raises(ValueError):
                pull(rows, dec)
        # the shard answers the next pull
        table = sh.to_numpy()
        assert_bits(sh.getRowsSum(rows, offsets, weights=w), replay_wgroups(table, local, offsets, w))
        assert_bits(sh.getRowsGroupDot(rows, offsets, x), replay_gdot_groups(table, local, offsets, x))


def test_wsum_errors_device(gpu):
    cols = 6
    local, offsets = request(11)
    rows = local + START
    n = rows.size
    bad = rows.copy()
    where = [int(offsets[4]) + 2, int(offsets[9]) + 70, int(offsets[10]) + 500]  # three groups, first at 10
    bad[where] = [START + SIZE, START - 1, START + 10 * SIZE]
    is_bad = np.zeros(n, bool)
    is_bad[where] = True
    w = np.array(fill_values("double", n, 1, "weights")).reshape(-1)
    w[where[0]], w[where[1]] = np.inf, -np.inf  # an infinite coefficient on a bad row makes no NaN
    with filled_shard("double", cols, gpu) as sh:
        table = sh.to_numpy()
        exp = replay_wgroups(table, local, offsets, w, bad=is_bad)
        assert np.isfinite(exp).all()
        t_rows, t_off, t_w = dev_tensors(gpu, bad, offsets, w)
        got = sh.getRowsSum(t_rows, t_off, sync=False, weights=t_w)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(t_rows))
        assert ei.value.record == min(where)
        assert not np.isnan(got.cpu().numpy()).any()
        assert_bits(got, exp)  # the bad rows are zero terms; every other record is summed
        sh.sync(sh._stream_of(t_rows))  # the error state was cleared
        # a malformed device grp_ptr is clamped to [0, n]; end < start is an empty group
        wild = offsets.copy()
        wild[0], wild[3], wild[-1] = -5, offsets[2] - 1, offsets[-1] + 1000
        t_good, t_wild = dev_tensors(gpu, rows, wild)
        fixed = np.clip(wild, 0, n)
        finite = np.array(fill_values("double", n, 1, "weights")).reshape(-1)
        exp = replay_wgroups(table, local, fixed, finite)
        assert_bits(sh.getRowsSum(t_good, t_wild, weights=dev_tensors(gpu, finite)[0]), exp, "clamped")


def test_gdot_errors_device(gpu):
    cols = 6
    local, offsets = request(11)
    rows = local + START
    n, g = rows.size, offsets.size - 1
    x = fill_values("long", g, cols, "x")
    bad = rows.copy()
    where = [int(offsets[4]) + 2, int(offsets[9]) + 70, int(offsets[10]) + 500]
    bad[where] = [START + SIZE, START - 1, START + 10 * SIZE]
    with filled_shard("long", cols, gpu) as sh:
        table = sh.to_numpy()
        group = group_of(offsets, n)
        exp = replay_gdot(table, local, np.where(np.isin(np.arange(n), where), -1, group), x)
        assert not exp[where].any() and (exp != 0).sum() > n - 10
        t_rows, t_off, t_x = dev_tensors(gpu, bad, offsets, x)
        got = sh.getRowsGroupDot(t_rows, t_off, t_x, sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(t_rows))
        assert ei.value.record == min(where)
        assert_bits(got, exp)  # the bad rows answer zero; every other record is right
        sh.sync(sh._stream_of(t_rows))
        # a malformed device grp_ptr: every value clamped, the group by the grouped push's search; records
        # that no group covers answer zero and no error is raised
        wild = offsets.copy()
        wild[0], wild[3], wild[-1] = 3, offsets[2] - 1, offsets[-1] + 1000
        short = np.minimum(offsets, n - 200)  # the last 200 records lie behind the last cut
        assert (clamped_groups(wild, n) != group).any() and (clamped_groups(short, n) < 0).sum() == 200
        for o in (wild, short):
            grp = clamped_groups(o, n)
            t_good, t_o = dev_tensors(gpu, rows, o)
            got = sh.getRowsGroupDot(t_good, t_o, t_x)  # sync=True: no error
            assert_bits(got, replay_gdot(table, local, grp, x), "clamped")


def test_wbag_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    o = np.array([0, 1], np.int64)
    v = np.ones(4, np.float64)  # coef (1 value read) / x (4 values)
    out = np.zeros(4, np.float64)
    rd, od, vd, outd = (torch.from_numpy(a).to(d) for a in (r, o, v, out))
    calls = [
        (lambda h, rows, n, p, g, a, dst: lib.glint_mat_pull_rows_wsum(h, rows, n, p, g, a, dst), False),
        (lambda h, rows, n, p, g, a, dst: lib.glint_mat_pull_rows_wsum_dev(h, rows, n, p, g, a, dst, None), True),
        (lambda h, rows, n, p, g, a, dst: lib.glint_mat_pull_rows_gdot(h, rows, n, p, g, a, dst), False),
        (lambda h, rows, n, p, g, a, dst: lib.glint_mat_pull_rows_gdot_dev(h, rows, n, p, g, a, dst, None), True),
    ]
    host_p = (r.ctypes.data, o.ctypes.data, v.ctypes.data, out.ctypes.data)
    dev_p = (rd.data_ptr(), od.data_ptr(), vd.data_ptr(), outd.data_ptr())
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        for call, on_dev in calls:
            rows_p, off_p, arg_p, out_p = dev_p if on_dev else host_p
            assert call(vec.handle, rows_p, 1, off_p, 1, arg_p, out_p) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        h = sh.handle
        for call, on_dev in calls:
            rows_p, off_p, arg_p, out_p = dev_p if on_dev else host_p
            assert call(h, rows_p, -1, off_p, 1, arg_p, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, -1, arg_p, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1 << 31, off_p, 1, arg_p, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, 1 << 31, arg_p, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, None, 1, arg_p, out_p) == N.GLINT_EINVAL
            assert call(h, None, 1, off_p, 1, arg_p, out_p) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, 1, arg_p, None) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, off_p, 1, None, out_p) == N.GLINT_EINVAL  # a NULL coef / x
            assert call(h, rows_p, 1, off_p, 1, arg_p, out_p) == N.GLINT_OK
        sh.sync(None)
        # wrong dtype or host / device mixing of weights, x or offsets: TypeError, and no call is made
        assert N.load().glint_prof_enable(h, 1) == N.GLINT_OK
        w1 = vd[:1].contiguous()
        for bad in (lambda: sh.getRowsSum(rd, od.to(torch.int32), weights=w1),
                    lambda: sh.getRowsSum(rd, o, weights=w1),
                    lambda: sh.getRowsSum(rd, od, weights=w1.to(torch.float32)),
                    lambda: sh.getRowsSum(rd, od, weights=v[:1]),
                    lambda: sh.getRowsSum(r, o, weights=w1),
                    lambda: sh.getRowsSum(r, od, weights=v[:1]),
                    lambda: sh.getRowsSum(r, o, weights=v[:1].astype(np.float32)),
                    lambda: sh.getRowsGroupDot(rd, od.to(torch.int32), vd),
                    lambda: sh.getRowsGroupDot(rd, o, vd),
                    lambda: sh.getRowsGroupDot(rd, od, vd.to(torch.float32)),
                    lambda: sh.getRowsGroupDot(rd, od, v),
                    lambda: sh.getRowsGroupDot(r, o, vd),
                    lambda: sh.getRowsGroupDot(r, od, v),
                    lambda: sh.getRowsGroupDot(r, o, v.astype(np.float32))):
            with pytest.raises(TypeError):
                bad()
        with pytest.raises(ValueError):
            sh.getRowsSum(r, o, weights=v[:2])
        with pytest.raises(ValueError):
            sh.getRowsGroupDot(r, o, v[:3])
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SUM) == 0 and _launches(sh, N.GLINT_K_PULL_ROWS_DOT) == 0


# ---- the forward, its weight gradient and the backward as one triple ------------------------------
def test_wbag_adjoint(gpu):
    """<wsum(rows, offsets, w), y> == <w, gdot(rows, offsets, y)> == <pushGroups(y, w) into zeros, table>
    modulo 2^64 on a Long shard, where every order gives the same bits."""
    cols = 7
    rng = np.random.default_rng(31)
    lens = rng.integers(0, 30, 60)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    n, g = int(offsets[-1]), lens.size
    local = rng.integers(0, SIZE, n).astype(np.int64)
    rows = local + START
    w = rng.integers(-2**63, 2**63 - 1, n).astype(np.int64)
    y = rng.integers(-2**63, 2**63 - 1, (g, cols)).astype(np.int64)
    u = lambda a: np.asarray(a).astype(np.uint64)  # noqa: E731  (wrapping arithmetic)
    with filled_shard("long", cols, gpu) as sh:
        table = sh.to_numpy()
        pooled = sh.getRowsSum(rows, offsets, weights=w)
        scores = sh.getRowsGroupDot(rows, offsets, y)
        with np.errstate(over="ignore"):
            forward = (u(pooled) * u(y)).sum(dtype=np.uint64)
            gradient = (u(w) * u(scores)).sum(dtype=np.uint64)
        assert forward == gradient and forward != 0
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as z:
        assert z.updateRowsGrouped(rows, offsets, y, weights=w)
        with np.errstate(over="ignore"):
            backward = (u(z.to_numpy()) * u(table)).sum(dtype=np.uint64)
        assert backward == forward


def test_wbag_client(gpu):
    rng = np.random.default_rng(14)
    table = rng.integers(-2**62, 2**62, (1000, 7)).astype(np.int64)
    m = glint_amd.Client([gpu] * 3).matrix(1000, 7, "long", modelsPerServer=2)
    assert m.nrOfPartitions == 6
    m.pushRows(np.arange(1000, dtype=np.int64), table)
    lens = rng.integers(0, 40, 200)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.integers(0, 1000, int(offsets[-1])).astype(np.int64)
    w = rng.integers(-2**62, 2**62, rows.size).astype(np.int64)
    x = rng.integers(-2**62, 2**62, (200, 7)).astype(np.int64)
    stored = m.pull(np.arange(1000, dtype=np.int64))
    assert_bits(m.pullSum(rows, offsets, weights=w), replay_wgroups(stored, rows, offsets, w))  # wrapping adds commute
    assert_bits(m.pullGroupDot(rows, offsets, x), replay_gdot_groups(stored, rows, offsets, x))
    m.destroy()
