"""Batched row dot pull (PartialMatrix.getRowsDotBatch, glint_mat_pull_rows_dot_batch*) on the GPU. Expected
values never come from the code under test: scores are float64 / longdouble products on the host, and the
bits are compared with what getTopKBatch reports. Every shard's pitch padding is NaN (ieee_cases.write_image),
so a read of it poisons a score. The host and the device call are checked against one expectation."""
import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from dot_cases import bits
from ieee_cases import write_image
from topk_cases import global_rows

pytestmark = pytest.mark.gpu
R, QMAX, START = N.GLINT_DOT_BATCH_ROWS, N.GLINT_DOT_MAX_QUERIES, 1_000_003  # a range shard's first row is not 0
DT = ["double", "float"]
COLS = [2, 67, 300]  # below one K step; the element-wise path with a tail; the 16-B path with a partial slab
NS = [1, R - 1, R + 1, 3 * R + 5]
QS = [1, 64, 65, 130]  # one vector; a full pass; a second pass of one vector; three passes
SIZE = 300
SHAPES = [(dt, COLS[(i + j) % 3], n) for i, dt in enumerate(DT) for j, n in enumerate(NS)]

np_dtype = {"double": np.float64, "float": np.float32}.get


def ints(rng, shape, npd):
    return rng.integers(-8, 9, shape).astype(npd)


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", gpu))


def shard_of(gpu, dtype, img, part=None):
    sh = PartialMatrix(part or RangePartition(2, START, START + img.shape[0]), img.shape[1], dtype, gpu)
    write_image(sh, gpu, np.ascontiguousarray(img), np.nan)
    return sh


def request(rng, n, size):  # local rows, shuffled, with repeats
    local = rng.integers(0, size, n).astype(np.int64)
    local[n // 2] = local[0]
    return local


def both(sh, gpu, rows, x):  # (what, answer) of the host call and of the device call, as numpy arrays
    return (("host", sh.getRowsDotBatch(rows, x)), ("device", sh.getRowsDotBatch(dev(gpu, rows), dev(gpu, x)).cpu().numpy()))


@pytest.mark.parametrize("dtype,cols,n", SHAPES)
def test_exact_answer_on_integer_data(gpu, dtype, cols, n):
    """Every partial sum is an integer below 2^24: any order is exact."""
    npd, rng = np_dtype(dtype), np.random.default_rng(n * 1000 + cols)
    img, x, local = ints(rng, (SIZE, cols), npd), ints(rng, (QS[-1], cols), npd), request(rng, n, SIZE)
    exp = (img[local].astype(np.float64) @ x.T.astype(np.float64)).astype(npd)
    with shard_of(gpu, dtype, img) as sh:
        for q in QS:
            for what, got in both(sh, gpu, local + START, x[:q]):
                assert got.dtype == npd and got.shape == (n, q), what
                np.testing.assert_array_equal(got, exp[:, :q], err_msg=f"{what} q={q}")
        for what, got in both(sh, gpu, local + START, x[3]):  # x of shape (cols,) answers (n,)
            np.testing.assert_array_equal(got, exp[:, 3], err_msg=f"{what} 1-d")


@pytest.mark.parametrize("dtype,cols,n", [(dt, COLS[(i + j) % 3], n) for i, dt in enumerate(DT)
                                          for j, n in enumerate((R - 1, R + 1, R + 1))])
def test_scores_within_the_bound_on_general_data(gpu, dtype, cols, n):
    npd, rng = np_dtype(dtype), np.random.default_rng(n + cols)
    if dtype == "double" and np.finfo(np.longdouble).eps > 2.0 ** -63:
        pytest.skip("longdouble is no wider than double here")
    img, x = rng.standard_normal((SIZE, cols)).astype(npd), rng.standard_normal((65, cols)).astype(npd)
    local = request(rng, n, SIZE)
    wide_img, wide_x = img[local].astype(np.longdouble), x.astype(np.longdouble)  # the reference, and the bound's sum
    ref, mag = wide_img @ wide_x.T, np.abs(wide_img) @ np.abs(wide_x).T
    cu = cols * np.longdouble(2.0) ** (-24 if dtype == "float" else -53)
    g = cu / (1 - cu)
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, local + START, x):
            err = np.abs(got.astype(np.longdouble) - ref)
            print(f"{what} {dtype} cols={cols}: max err / bound = {float((err / (g * mag)).max()):.3g}")
            assert (err <= g * mag).all(), what


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cols", [67, 300])
def test_score_bits_are_the_batched_topk_pulls(gpu, dtype, cols):
    npd, rng, size, q = np_dtype(dtype), np.random.default_rng(cols), R + 2, 130
    img, x = rng.standard_normal((size, cols)).astype(npd), rng.standard_normal((q, cols)).astype(npd)
    n = 2 * R + 7
    local = request(rng, n, size)
    at_requests, at_vectors = [0, R - 1, R, n - 1], [0, 63, 64, q - 1]
    local[at_requests], x[at_vectors] = 5, x[7]
    with shard_of(gpu, dtype, img) as sh:
        t_rows, t_vals = sh.getTopKBatch(x, size)  # k = size: every row once per vector
        exp = np.empty((size, q), npd)
        for j in range(q):
            assert sorted(t_rows[j].tolist()) == list(range(START, START + size))
            exp[t_rows[j] - START, j] = t_vals[j]
        alone = sh.getRowsDotBatch(np.array([START + 5]), x[7:8])
        assert alone.shape == (1, 1)
        for what, got in both(sh, gpu, local + START, x):
            np.testing.assert_array_equal(bits(got), bits(exp[local]), err_msg=what)
            same = bits(np.ascontiguousarray(got[np.ix_(at_requests, at_vectors + [7])]))
            assert (same == bits(alone)[0, 0]).all(), what


@pytest.mark.parametrize("dtype", DT)
def test_non_finite_values_and_rows_outside_the_partition(gpu, dtype):
    npd, rng, cols, q, n = np_dtype(dtype), np.random.default_rng(4), 67, 65, R + 9
    img, x, local = ints(rng, (SIZE, cols), npd), ints(rng, (q, cols), npd), request(rng, n, SIZE)
    x[:, 1], img[:, 5] = 0, 1
    x[3, 5], x[64, 6] = np.inf, np.nan
    local[local == 9] = 10
    local[[7, R + 1]] = 9
    img[9, 1] = np.inf  # times x[j][1] == 0: NaN in the scores of requests 7 and R + 1 only
    with np.errstate(invalid="ignore"):
        exp = (img[local][:, None, :].astype(np.float64) * x[None].astype(np.float64)).sum(-1).astype(npd)
    assert np.isnan(exp[[7, R + 1]]).all() and np.isnan(np.delete(exp, [7, R + 1], 0)[:, :64]).sum() == 0
    assert np.isinf(np.delete(exp, [7, R + 1], 0)[:, 3]).all() and np.isnan(exp[:, 64]).all()
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, local + START, x):
            np.testing.assert_array_equal(got, exp, err_msg=what)
        bad = local + START
        bad[[40, R + 3]] = START - 1, START + SIZE
        out = np.full((n, q), 77, npd)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.getRowsDotBatch(bad, x, out=out)
        assert ei.value.record == 40 and (out == 77).all()  # nothing written
        got = sh.getRowsDotBatch(dev(gpu, bad), dev(gpu, x), sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(got))
        assert ei.value.record == 40  # the lowest such request
        got = got.cpu().numpy()
        assert not bits(got[[40, R + 3]]).any()  # q values of +0, also against the inf and the NaN of x
        exp[[40, R + 3]] = 0
        np.testing.assert_array_equal(got, exp)


def test_cyclic_keys_and_unaligned_x(gpu):
    import torch
    size, cols, q, n, rng = R + 1, 300, 65, R + 5, np.random.default_rng(5)
    img, x, local = rng.standard_normal((size, cols)), rng.standard_normal((q, cols)), request(rng, n, size)
    rows = global_rows(size, cyclic=(1, 3))[local]
    with shard_of(gpu, "double", img, part=CyclicPartition(1, 3, 3 * size)) as sh:
        buf = torch.zeros(q * cols + 4, dtype=torch.float64, device=torch.device("cuda", gpu))
        answers = []
        for shift in (0, 1):  # one element past a 16-B boundary: x is read element by element
            view = buf[shift:shift + q * cols].copy_(dev(gpu, x).reshape(-1))
            assert view.data_ptr() % 16 == 8 * shift
            answers.append(sh.getRowsDotBatch(dev(gpu, rows), view.view(q, cols)).cpu().numpy())
        np.testing.assert_array_equal(bits(answers[0]), bits(answers[1]))
        np.testing.assert_array_equal(bits(answers[0]), bits(sh.getRowsDotBatch(rows, x)))
        # the contract's bound, twice: the float64 reference has the same one
        bound = 2 * cols * 2.0 ** -53 / (1 - cols * 2.0 ** -53) * (np.abs(img[local]) @ np.abs(x).T)
        assert (np.abs(answers[0] - img[local] @ x.T) <= bound).all()


def test_argument_errors(gpu):
    lib, x, rows, out = N.load(), np.ones((2, 4)), np.full(3, START, np.int64), np.zeros((3, 2))
    xd, rowsd, outd = dev(gpu, x), dev(gpu, rows), dev(gpu, out)
    devc = lambda h, r, n, xp, q, o: lib.glint_mat_pull_rows_dot_batch_dev(h, r, n, xp, q, o, None)  # noqa: E731
    calls = ((lib.glint_mat_pull_rows_dot_batch, [a.ctypes.data for a in (rows, x, out)]),
             (devc, [a.data_ptr() for a in (rowsd, xd, outd)]))
    for dtype in ("int", "long"):
        with PartialMatrix(RangePartition(0, START, START + 10), 4, dtype, gpu) as sh:
            for call, (rp, xp, op) in calls:
                assert call(sh.handle, rp, 3, xp, 2, op) == N.GLINT_EINVAL
            with pytest.raises(TypeError):
                sh.getRowsDotBatch(rows, np.ones((2, 4), sh.np_dtype))
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        for call, (rp, xp, op) in calls:
            assert call(vec.handle, rp, 3, xp, 1, op) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        for call, (rp, xp, op) in calls:
            for n, q in ((3, 0), (3, QMAX + 1), (-1, 2)):
                assert call(sh.handle, rp, n, xp, q, op) == N.GLINT_EINVAL
            assert call(sh.handle, rp, 3, None, 1, op) == N.GLINT_EINVAL  # no self-dot
            assert call(sh.handle, None, 0, xp, 2, None) == N.GLINT_OK  # n == 0 writes nothing
            assert call(sh.handle, rp, 3, xp, 2, op) == N.GLINT_OK
        sh.sync(None)
        assert not out.any() and not outd.cpu().numpy().any()  # an all-zero shard
        with pytest.raises(TypeError):
            sh.getRowsDotBatch(rows, None)
        with pytest.raises(ValueError):
            sh.getRowsDotBatch(rows, np.ones((QMAX + 1, 4)))
