"""Top-k row pull (PartialMatrix.getTopK, glint_mat_pull_topk*) on the GPU.

Expected values never come from the code under test: the shard's image is written as it lies
(ieee_cases.write_image), every score is replayed on the host in the row dot pull's order and the order
is topk_cases' stable sort. Rows are compared exactly, scores bit for bit (a NaN by class), and the host
call and the device call against the same expected answer, so against each other.
"""
import ctypes as C

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartition, PartialMatrix, PartialVector, RangePartition
from dot_cases import bits, fill_values
from ieee_cases import write_image
from topk_cases import (assert_topk_bits, expected_topk, global_rows, scores_of, topk_of_score_table,
                        topk_of_scores)

pytestmark = pytest.mark.gpu
T = N.GLINT_TOPK_TILE
KMAX = N.GLINT_TOPK_MAX_K
START = 1_000_003  # a range shard whose first row is not 0
DT = ["double", "float", "long", "int"]
COLS = [2, 67, 300]  # 16-B path in one strip; scalar path in two strips; 16-B path with a partial strip
# one row; less than a wave; one tile short of full; two tiles, the second of one row (two levels); four
# tiles, the last of five rows
SIZES = [1, 63, T - 1, T + 1, 3 * T + 5]
KS = [1, 37, KMAX]
SENTINEL = 0x5A


def np_dtype(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", gpu))


def shard_of(gpu, dtype, img, pad_value=0, part=None):
    sh = PartialMatrix(part or RangePartition(2, START, START + img.shape[0]), img.shape[1], dtype, gpu)
    assert sh.size == img.shape[0]
    write_image(sh, gpu, np.ascontiguousarray(img), pad_value)
    return sh


def both(sh, gpu, x, k):
    """(what, answer) of the host call and of the device call."""
    return (("host", sh.getTopK(x, k)), ("device", sh.getTopK(dev(gpu, x), k)))


# every dtype at every size, the column counts rotating so that each dtype meets each of them
SHAPES = [(dt, COLS[(i + j) % 3], size) for i, dt in enumerate(DT) for j, size in enumerate(SIZES)]


@pytest.mark.parametrize("dtype,cols,size", SHAPES)
def test_topk_parity(gpu, dtype, cols, size):
    npd = np_dtype(dtype)
    img = fill_values(npd, cols, size, "topk")
    x5 = fill_values(npd, cols, 5, "topk-x")
    sc = scores_of(img, x5)  # every row against every query, once
    rows = global_rows(size, START)
    with shard_of(gpu, dtype, img) as sh:
        if size == 63:
            np.testing.assert_array_equal(bits(sh.to_numpy()), bits(img))
        for q in (1, 5):
            for k in KS:  # 37 and 1024 exceed the two small sizes: the -1 fill
                exp = topk_of_score_table(sc[:, :q], rows, k)
                assert (exp[0] >= 0).sum() == q * min(k, size)
                for what, got in both(sh, gpu, x5[:q], k):
                    assert_topk_bits(got, exp, f"{what} q={q} k={k}")
        # x of shape (cols,) answers (k,)
        exp = topk_of_scores(np.ascontiguousarray(sc[:, 3]), rows, 37)
        for what, got in both(sh, gpu, x5[3], 37):
            assert got[0].shape == (37,)
            assert_topk_bits(got, exp, f"{what} 1-d")


def _assert_tiebreak_decides(sc, rows, k):
    """On the expected answer: a run of equal scores that reaches the answer has rows on both sides of a
    tile border, and a run is cut at position k -- so the tiebreak decides who is in."""
    more_rows, more_vals = topk_of_scores(sc, rows, k + 1)
    assert more_rows[k] >= 0 and more_vals[k] == more_vals[k - 1], "no run is cut at k"
    crossing = False
    for v in np.unique(more_vals[:k]):
        tiles = np.flatnonzero(sc == v) // T  # the run in the whole table (no NaN here; -0 == +0)
        crossing |= bool(tiles.min() != tiles.max())
    assert crossing, "no run of equal scores crosses a tile border"


def _tie_tables():
    rng = np.random.default_rng(71)
    ints = rng.integers(-1, 2, (2 * T + 7, 3)).astype(np.int32)
    five = (rng.standard_normal((5, 2)) * 10.0 ** rng.integers(-2, 3, (5, 2)))
    repeated = five[rng.integers(0, 5, 2 * T + 9)]
    zeros = np.zeros((T + 9, 2), np.float32)
    return [("int", ints, np.array([[1, 1, 1], [-1, -1, -1]], np.int32)), ("double", repeated, rng.standard_normal((2, 2))),
            ("float", zeros, rng.standard_normal((2, 2)).astype(np.float32))]


@pytest.mark.parametrize("case", [0, 1, 2], ids=["int-small-values", "double-five-rows", "all-zero"])
def test_topk_ties_go_to_the_lower_row(gpu, case):
    dtype, img, x = _tie_tables()[case]
    sc = scores_of(img, x)
    rows = global_rows(img.shape[0], START)
    for j in range(2):  # before any GPU call
        _assert_tiebreak_decides(np.ascontiguousarray(sc[:, j]), rows, KMAX)
    exp = topk_of_score_table(sc, rows, KMAX)
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, x, KMAX):
            assert_topk_bits(got, exp, what)


@pytest.mark.parametrize("dtype", ["double", "float"])
def test_topk_special_scores(gpu, dtype):
    """+inf, -inf, NaN (inf * 0), a subnormal and the largest finite value as scores: the NaNs rank
    last, in row order, below -inf."""
    npd = np_dtype(dtype)
    fi = np.finfo(npd)
    size = 70
    img = np.zeros((size, 2), npd)
    img[:, 0] = np.linspace(-3, 3, size).astype(npd)
    img[5] = [np.inf, 1]
    img[[9, 33, 69]] = [np.inf, np.inf]  # inf * 1 + inf * 0
    img[12] = [-np.inf, 1]
    img[20] = [fi.smallest_subnormal, 0]
    img[21] = [-fi.smallest_subnormal, 0]
    img[40] = [fi.max, 0]
    img[41] = [-0.0, 0]
    x = np.array([1, 0], npd)
    sc = scores_of(img, x)
    assert np.isnan(sc[[9, 33, 69]]).all() and np.isnan(sc).sum() == 3
    assert sc[5] == np.inf and sc[12] == -np.inf and sc[40] == fi.max and 0 < sc[20] < fi.tiny
    rows = global_rows(size, START)
    with shard_of(gpu, dtype, img) as sh:
        exp = topk_of_scores(sc, rows, size)  # k = size: the NaNs come last, in row order
        assert (exp[0][-3:] - START).tolist() == [9, 33, 69] and exp[0][-4] - START == 12
        assert (exp[0][:3] - START).tolist() == [5, 40, 69 - 1]
        for what, got in both(sh, gpu, x, size):
            assert_topk_bits(got, exp, what)
        exp = topk_of_scores(sc, rows, size - 3)  # k = the non-NaN count: no NaN appears
        assert not np.isnan(exp[1]).any()
        for what, got in both(sh, gpu, x, size - 3):
            assert not np.isnan(np.asarray(got[1].cpu() if hasattr(got[1], "cpu") else got[1])).any(), what
            assert_topk_bits(got, exp, what)


def _launches(sh):
    out = []
    for kid in range(N.GLINT_K_COUNT):
        ms, cnt = C.c_double(), C.c_int64()
        assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
        out.append(cnt.value)
    return out


def test_topk_three_levels(gpu):
    """5T + 3 rows at k = 1024: level 0 emits 5 * 1024 + 3 > T candidates, so a third level runs. The
    winners stand at both ends of the shard and on both sides of the first tile border."""
    size = 5 * T + 3
    rng = np.random.default_rng(72)
    img = rng.uniform(-1, 1, (size, 2))
    planted = [0, T - 1, T, size - 1]
    img[planted] = [[50, 50], [40, 40], [30, 30], [20, 20]]
    x = np.array([[1.0, 1.0], [-1.0, -1.0]])
    sc = scores_of(img, x)
    rows = global_rows(size, START)
    exp = topk_of_score_table(sc, rows, KMAX)
    assert (exp[0][0, :4] - START).tolist() == planted
    with shard_of(gpu, "double", img) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        before = _launches(sh)
        for n, (what, got) in enumerate(both(sh, gpu, x, KMAX)):
            assert_topk_bits(got, exp, what)
        after = _launches(sh)
        assert after[N.GLINT_K_PULL_ROWS_DOT] - before[N.GLINT_K_PULL_ROWS_DOT] == 2 * (1 + 3)  # scores + 3 levels
        # launch by launch: each call's four in order, every one with a time
        cnt, ms = C.c_int64(), (C.c_double * 16)(*([-1.0] * 16))
        assert N.load().glint_prof_read_launches(sh.handle, N.GLINT_K_PULL_ROWS_DOT, ms, 16, C.byref(cnt)) == N.GLINT_OK
        assert cnt.value == 8 and all(v > 0 for v in ms[:8]) and all(v == -1.0 for v in ms[8:])
        assert N.load().glint_prof_read_launches(sh.handle, N.GLINT_K_PUSH_APPLY, ms, 16, C.byref(cnt)) == N.GLINT_OK
        assert cnt.value == 0
        # the lowest k of query 1 are the highest of its negation: the planted rows come last there
        low = topk_of_scores(np.ascontiguousarray(-sc[:, 0]), rows, KMAX)
        np.testing.assert_array_equal(exp[0][1], low[0])


def test_topk_cyclic_layout(gpu):
    part = CyclicPartition(1, 3, 3 * (T + 1))
    cols, size = 67, T + 1
    img = fill_values(np.float64, cols, size, "topk-cyclic")
    x = fill_values(np.float64, cols, 2, "topk-x")
    with shard_of(gpu, "double", img, part=part) as sh:
        exp = expected_topk(img, x, 37, cyclic=(1, 3))
        assert (exp[0] % 3 == 1).all() and exp[0].max() > size  # keys index + local * parts
        for what, got in both(sh, gpu, x, 37):
            assert_topk_bits(got, exp, what)


@pytest.mark.parametrize("dtype", ["double", "float"])
@pytest.mark.parametrize("pad", [np.inf, np.nan])
def test_topk_never_reads_the_padding(gpu, dtype, pad):
    npd = np_dtype(dtype)
    cols, size = 67, 300
    img = fill_values(npd, cols, size, "topk")
    x = fill_values(npd, cols, 5, "topk-x")
    exp = expected_topk(img, x, 37, START)
    assert np.isfinite(exp[1]).all()
    with shard_of(gpu, dtype, img, pad_value=pad) as sh:
        for what, got in both(sh, gpu, x, 37):
            assert_topk_bits(got, exp, what)


@pytest.mark.parametrize("dtype,cols", [("double", 300), ("float", 300), ("int", 2), ("long", 300)])
def test_topk_unaligned_x_gives_the_same_bits(gpu, dtype, cols):
    """The device call with x one element past a 16-B boundary reads it element by element."""
    import torch
    npd = np_dtype(dtype)
    img = fill_values(npd, cols, 300, "topk")
    with shard_of(gpu, dtype, img) as sh:
        for q in (1, 5):
            x = fill_values(npd, cols, q, "topk-x")
            exp = expected_topk(img, x, 37, START)
            buf = torch.zeros(q * cols + 4, dtype=sh.torch_dtype, device=torch.device("cuda", gpu))
            assert buf.data_ptr() % 16 == 0
            for shift in (0, 1):
                view = buf[shift:shift + q * cols]
                view.copy_(dev(gpu, x).reshape(-1))
                assert view.data_ptr() % 16 == (0 if shift == 0 else view.element_size())
                assert_topk_bits(sh.getTopK(view.view(q, cols), 37), exp, f"q={q} shift {shift}")


def test_topk_device_call_is_stream_ordered_and_writes_only_its_answer(gpu):
    import torch
    lib = N.load()
    cols, size, q, k = 67, T + 1, 5, 37
    img = np.array(fill_values(np.float64, cols, size, "topk"))
    x = fill_values(np.float64, cols, q, "topk-x")
    push_rows = np.array([START + 7, START + T, START + 7], np.int64)
    push_vals = fill_values(np.float64, cols, 3, "topk-push") * 1e6  # rows 7 and T come to dominate
    after = img.copy()
    for r, v in zip(push_rows - START, push_vals):
        after[r] = after[r] + v
    exp = expected_topk(after, x, k, START)
    assert not np.array_equal(exp[0], expected_topk(img, x, k, START)[0])  # the push shows in the answer
    d = torch.device("cuda", gpu)
    with shard_of(gpu, "double", img) as sh:
        pad = 64
        out_rows = torch.full((q * k + 2 * pad,), SENTINEL, dtype=torch.int64, device=d)
        out_vals = torch.full((q * k + 2 * pad,), float(SENTINEL), dtype=torch.float64, device=d)
        d_x, d_rows, d_vals = dev(gpu, x), dev(gpu, push_rows), dev(gpu, push_vals)
        st = sh._stream_of(d_x)
        # a push and the pull behind it on one stream, no synchronisation between them
        assert sh.updateRows(d_rows, d_vals, deterministic=True, sync=False)
        assert lib.glint_mat_pull_topk_dev(sh.handle, d_x.data_ptr(), q, k, out_rows[pad:].data_ptr(),
                                           out_vals[pad:].data_ptr(), st) == N.GLINT_OK
        sh.sync(st)
        np.testing.assert_array_equal(bits(sh.to_numpy()), bits(after))
        got_rows, got_vals = out_rows.cpu().numpy(), out_vals.cpu().numpy()
        assert_topk_bits((got_rows[pad:-pad].reshape(q, k), got_vals[pad:-pad].reshape(q, k)), exp)
        for edge in (got_rows[:pad], got_rows[-pad:]):  # nothing outside q * k is touched
            assert (edge == SENTINEL).all()
        for edge in (got_vals[:pad], got_vals[-pad:]):
            assert (edge == float(SENTINEL)).all()
        # launch accounting: everything under the row dot pull's id, nothing under another
        assert lib.glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        before = _launches(sh)
        rows2, vals2 = sh.getTopK(d_x, k)
        now = _launches(sh)
        assert_topk_bits((rows2, vals2), exp, "second call")
        assert now[N.GLINT_K_PULL_ROWS_DOT] - before[N.GLINT_K_PULL_ROWS_DOT] >= 2
        assert now[N.GLINT_K_PULL_ROWS_DOT] - before[N.GLINT_K_PULL_ROWS_DOT] == 1 + 2  # scores + two levels
        for kid in range(N.GLINT_K_COUNT):
            if kid != N.GLINT_K_PULL_ROWS_DOT:
                assert now[kid] == before[kid], kid
        # the host call right behind device work sees the same shard
        assert_topk_bits(sh.getTopK(x, k), exp, "host after device")


def test_topk_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    x = np.ones((2, 4), np.float64)
    rows, vals = np.zeros(2 * 3, np.int64), np.zeros(2 * 3, np.float64)
    xd, rowsd, valsd = (torch.from_numpy(a).to(d) for a in (x, rows, vals))
    host = lambda h, xp, q, k, r, v: lib.glint_mat_pull_topk(h, xp, q, k, r, v)  # noqa: E731
    devc = lambda h, xp, q, k, r, v: lib.glint_mat_pull_topk_dev(h, xp, q, k, r, v, None)  # noqa: E731
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        assert host(vec.handle, x.ctypes.data, 1, 1, rows.ctypes.data, vals.ctypes.data) == N.GLINT_EINVAL
        assert devc(vec.handle, xd.data_ptr(), 1, 1, rowsd.data_ptr(), valsd.data_ptr()) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        h = sh.handle
        for call, (xp, rp, vp) in ((host, (x.ctypes.data, rows.ctypes.data, vals.ctypes.data)),
                                   (devc, (xd.data_ptr(), rowsd.data_ptr(), valsd.data_ptr()))):
            assert call(None, xp, 2, 3, rp, vp) == N.GLINT_EINVAL
            assert call(h, None, 2, 3, rp, vp) == N.GLINT_EINVAL
            for q in (0, -1, N.GLINT_TOPK_MAX_QUERIES + 1):
                assert call(h, xp, q, 3, rp, vp) == N.GLINT_EINVAL
            for k in (0, -1, KMAX + 1):
                assert call(h, xp, 2, k, rp, vp) == N.GLINT_EINVAL
            assert call(h, xp, 2, 3, None, vp) == N.GLINT_EINVAL
            assert call(h, xp, 2, 3, rp, None) == N.GLINT_EINVAL
            assert call(h, xp, 2, 3, rp, vp) == N.GLINT_OK
        sh.sync(None)
        for r, v in ((rows, vals), (rowsd.cpu().numpy(), valsd.cpu().numpy())):  # an all-zero shard
            assert r.tolist() == [START, START + 1, START + 2] * 2 and not v.any()
        with pytest.raises(TypeError):  # x of the wrong dtype: no call is made
            sh.getTopK(xd.to(torch.float32), 3)
        for bad in (x[:, :3], np.ones((N.GLINT_TOPK_MAX_QUERIES + 1, 4)), np.ones((1, 2, 4))):
            with pytest.raises(ValueError):
                sh.getTopK(bad, 3)
            with pytest.raises(ValueError):
                sh.getTopK(dev(gpu, bad), 3)
        for k in (0, KMAX + 1):
            with pytest.raises(ValueError):
                sh.getTopK(x, k)


def test_topk_python_shapes_and_client(gpu):
    import torch
    rng = np.random.default_rng(73)
    table = rng.integers(-2**62, 2**62, (1000, 7)).astype(np.int64)
    m = glint_amd.Client([gpu] * 3).matrix(1000, 7, "long", modelsPerServer=1)
    assert m.nrOfPartitions == 3
    m.pushRows(np.arange(1000, dtype=np.int64), table)
    x = rng.integers(-2**62, 2**62, (3, 7)).astype(np.int64)
    sh = m.shards[1]
    r, v = sh.getTopK(x[0], 5)
    assert isinstance(r, np.ndarray) and r.shape == v.shape == (5,) and r.dtype == np.int64 and v.dtype == np.int64
    r, v = sh.getTopK(x, 5)
    assert r.shape == v.shape == (3, 5)
    r, v = sh.getTopK(dev(gpu, x), 5, sync=False)
    sh.sync(sh._stream_of(r))
    assert isinstance(r, torch.Tensor) and r.is_cuda and tuple(r.shape) == tuple(v.shape) == (3, 5)
    assert r.dtype == torch.int64 and v.dtype == torch.int64
    r, v = sh.getTopK(dev(gpu, x[0]), 1024)  # more than the partition's 333 or 334 rows
    assert tuple(r.shape) == (1024,) and (r.cpu().numpy()[sh.size:] == -1).all()
    # the whole matrix: the merge of three partitions is the table's own answer
    stored = m.pull(np.arange(1000, dtype=np.int64))
    np.testing.assert_array_equal(stored, table)
    for k in (1, 37, 1024):  # 1024 exceeds both a partition and the matrix
        assert_topk_bits(m.pullTopK(x, k), expected_topk(table, x, k), f"k={k}")
    one = m.pullTopK(x[2], 37)
    assert one[0].shape == (37,)
    assert_topk_bits(one, expected_topk(table, x[2], 37))
    m.destroy()
