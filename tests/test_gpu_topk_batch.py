"""Batched top-k row pull (PartialMatrix.getTopKBatch, glint_mat_pull_topk_batch*) on the GPU. Expected
values never come from the code under test: scores are float64 / longdouble products on the host, the order
is topk_cases' stable sort. Every shard's pitch padding is NaN (ieee_cases.write_image), so a read of it
poisons a score. The host and the device call are checked against one expectation."""
import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import CyclicPartition, PartialMatrix, RangePartition
from dot_cases import bits
from ieee_cases import write_image
from topk_cases import global_rows, topk_of_score_table, topk_of_scores

pytestmark = pytest.mark.gpu
R, T, KMAX = N.GLINT_TOPK_BATCH_ROWS, N.GLINT_TOPK_TILE, N.GLINT_TOPK_MAX_K
QMAX, START = N.GLINT_TOPK_BATCH_MAX_QUERIES, 1_000_003  # a range shard whose first row is not 0
DT = ["double", "float"]
COLS = [2, 67, 300]  # below one K step; the scalar path with a tail; the 16-B path with a partial slab
SIZES = [1, R - 1, R + 1, 3 * R + 5, T + 1]
QS = [1, 64, 65, 130]  # one query; a full pass; a second pass of one query; three passes
SHAPES = [(dt, COLS[(i + j) % 3], size) for i, dt in enumerate(DT) for j, size in enumerate(SIZES)]


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


def both(sh, gpu, x, k):  # (what, (rows, vals)) of the host call and of the device call, as numpy arrays
    r, v = sh.getTopKBatch(dev(gpu, x), k)
    return (("host", sh.getTopKBatch(x, k)), ("device", (r.cpu().numpy(), v.cpu().numpy())))


def assert_answer(got, exp, what):  # rows exactly, values numerically (NaN by class, -0 equal to +0)
    assert got[0].dtype == np.int64 and got[1].dtype == exp[1].dtype, what
    for g, e in zip(got, exp):
        np.testing.assert_array_equal(g, e, err_msg=what)


@pytest.mark.parametrize("dtype,cols,size", SHAPES)
def test_exact_answer_on_integer_data(gpu, dtype, cols, size):
    """Every partial sum is an integer below 2^24: any order is exact. Every other row repeats one of five."""
    npd, rng = np_dtype(dtype), np.random.default_rng(size * 1000 + cols)
    img = ints(rng, (size, cols), npd)
    img[::2] = ints(rng, (5, cols), npd)[rng.integers(0, 5, (size + 1) // 2)]
    x = ints(rng, (QS[-1], cols), npd)
    sc = (img.astype(np.float64) @ x.T.astype(np.float64)).astype(npd)
    rows = global_rows(size, START)
    if size > 37:  # on the expectation, before any GPU call: a run of equal scores is cut at k
        cut = [topk_of_scores(np.ascontiguousarray(sc[:, j]), rows, 38)[1] for j in range(QS[-1])]
        assert any(v[36] == v[37] for v in cut)
    with shard_of(gpu, dtype, img) as sh:
        for q in QS:
            for k in (1, 37, KMAX):
                exp = topk_of_score_table(sc[:, :q], rows, k)
                for what, got in both(sh, gpu, x[:q], k):
                    assert_answer(got, exp, f"{what} q={q} k={k}")
        for what, got in both(sh, gpu, x[3], 37):  # x of shape (cols,) answers (k,)
            assert_answer(got, topk_of_scores(np.ascontiguousarray(sc[:, 3]), rows, 37), f"{what} 1-d")


def scores_by_row(got, size):  # of an answer with k = size: it names every row once, in the contract's order
    rows, vals = got
    out = np.empty_like(vals)
    for j in range(rows.shape[0]):
        assert sorted(rows[j].tolist()) == list(range(START, START + size))
        out[j, rows[j] - START] = vals[j]
        np.testing.assert_array_equal(topk_of_scores(out[j], global_rows(size, START), size)[0], rows[j])
    return out


@pytest.mark.parametrize("dtype,cols,size", [(dt, COLS[(i + j) % 3], s) for i, dt in enumerate(DT)
                                             for j, s in enumerate((R - 1, R + 1, R + 1))])
def test_scores_within_the_bound_on_general_data(gpu, dtype, cols, size):
    npd, rng = np_dtype(dtype), np.random.default_rng(size + cols)
    if dtype == "double" and np.finfo(np.longdouble).eps > 2.0 ** -63:
        pytest.skip("longdouble is no wider than double here")
    img, x = rng.standard_normal((size, cols)).astype(npd), rng.standard_normal((65, cols)).astype(npd)
    wide_img, wide_x = img.astype(np.longdouble), x.astype(np.longdouble)  # the reference, and the bound's sum
    ref, mag = wide_x @ wide_img.T, np.abs(wide_x) @ np.abs(wide_img).T
    cu = cols * np.longdouble(2.0) ** (-24 if dtype == "float" else -53)
    g = cu / (1 - cu)
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, x, size):
            err = np.abs(scores_by_row(got, size).astype(np.longdouble) - ref)
            print(f"{what} {dtype} cols={cols}: max err / bound = {float((err / (g * mag)).max()):.3g}")
            assert (err <= g * mag).all(), what


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cols", [67, 300])
def test_score_bits_do_not_depend_on_position(gpu, dtype, cols):
    npd, rng, size, q = np_dtype(dtype), np.random.default_rng(cols), R + 2, 130
    img, x = rng.standard_normal((size, cols)).astype(npd), rng.standard_normal((q, cols)).astype(npd)
    at_rows, at_queries = [0, R - 1, R, size - 1], [0, 63, 64, q - 1]
    img[at_rows], x[at_queries] = img[5], x[7]
    with shard_of(gpu, dtype, img) as sh:
        alone = scores_by_row(sh.getTopKBatch(x[7:8], size), size)[0, 5]
        for what, got in both(sh, gpu, x, size):
            sc = scores_by_row(got, size)
            same = bits(np.ascontiguousarray(sc[np.ix_(at_queries + [7], at_rows + [5])]))
            assert (same == bits(np.array([alone]))[0]).all(), what


@pytest.mark.parametrize("dtype", DT)
def test_non_finite_scores(gpu, dtype):
    """+inf first, -inf last of the numbers, inf * 0 = NaN behind it in row order; the pads make no other NaN."""
    npd, rng, size, cols = np_dtype(dtype), np.random.default_rng(4), R + 2, 67
    img, x = ints(rng, (size, cols), npd), ints(rng, (2, cols), npd)
    img[:, cols - 1] = 1
    x[:, :2], x[1, cols - 1] = [1, 0], np.inf  # query 1: every ordinary score is +inf
    img[[R, 3], 0] = [np.inf, -np.inf]
    img[[9, R - 1, size - 1], 1] = np.inf  # times x[j][1] == 0
    with np.errstate(invalid="ignore"):
        sc = (img[:, None, :].astype(np.float64) * x[None].astype(np.float64)).sum(-1).astype(npd)
    exp = topk_of_score_table(sc, global_rows(size, START), size)
    assert (exp[0][0, [0, -4, -3, -2, -1]] - START).tolist() == [R, 3, 9, R - 1, size - 1]
    assert np.isnan(sc[:, 0]).sum() == 3 and np.isnan(sc[:, 1]).sum() == 4 and (sc[:, 1] == np.inf).sum() == size - 4
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, x, size):
            assert_answer(got, exp, what)


def test_cyclic_keys_and_unaligned_x(gpu):
    import torch
    size, cols, q, rng = R + 1, 300, 65, np.random.default_rng(5)
    img, x = rng.standard_normal((size, cols)), rng.standard_normal((q, cols))
    with shard_of(gpu, "double", img, part=CyclicPartition(1, 3, 3 * size)) as sh:
        buf = torch.zeros(q * cols + 4, dtype=torch.float64, device=torch.device("cuda", gpu))
        answers = []
        for shift in (0, 1):  # one element past a 16-B boundary: x is read element by element
            view = buf[shift:shift + q * cols].copy_(dev(gpu, x).reshape(-1))
            assert view.data_ptr() % 16 == 8 * shift
            answers.append([a.cpu().numpy() for a in sh.getTopKBatch(view.view(q, cols), 37)])
        assert (answers[0][0] % 3 == 1).all() and answers[0][0].max() > size  # keys index + local * parts
        for a, b in zip(*answers):
            np.testing.assert_array_equal(bits(a), bits(b))
        ref = topk_of_score_table(img @ x.T, global_rows(size, cyclic=(1, 3)), 1)  # the winners are clear
        np.testing.assert_array_equal(answers[0][0][:, :1], ref[0])


def test_argument_errors(gpu):
    lib, x, rows, vals = N.load(), np.ones((2, 4)), np.zeros(6, np.int64), np.zeros(6)
    xd, rowsd, valsd = dev(gpu, x), dev(gpu, rows), dev(gpu, vals)
    devc = lambda h, xp, q, k, r, v: lib.glint_mat_pull_topk_batch_dev(h, xp, q, k, r, v, None)  # noqa: E731
    calls = ((lib.glint_mat_pull_topk_batch, [a.ctypes.data for a in (x, rows, vals)]),
             (devc, [a.data_ptr() for a in (xd, rowsd, valsd)]))
    for dtype in ("int", "long"):
        with PartialMatrix(RangePartition(0, START, START + 10), 4, dtype, gpu) as sh:
            for call, (xp, rp, vp) in calls:
                assert call(sh.handle, xp, 2, 3, rp, vp) == N.GLINT_EINVAL
            with pytest.raises(TypeError):
                sh.getTopKBatch(np.ones((2, 4), sh.np_dtype), 3)
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        for call, (xp, rp, vp) in calls:
            for q, k in ((0, 3), (QMAX + 1, 3), (2, 0), (2, KMAX + 1)):
                assert call(sh.handle, xp, q, k, rp, vp) == N.GLINT_EINVAL
            assert call(sh.handle, None, 2, 3, rp, vp) == N.GLINT_EINVAL
            assert call(sh.handle, xp, 2, 3, rp, vp) == N.GLINT_OK
        sh.sync(None)
        assert rows.tolist() == rowsd.cpu().tolist() == [START, START + 1, START + 2] * 2  # an all-zero shard
        for bad_x, k in ((np.ones((QMAX + 1, 4)), 3), (x, 0), (x, KMAX + 1)):
            with pytest.raises(ValueError):
                sh.getTopKBatch(bad_x, k)
