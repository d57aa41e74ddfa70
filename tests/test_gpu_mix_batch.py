"""Batched row mix pull (PartialMatrix.getRowsMixBatch, glint_mat_pull_rows_mix_batch*) on the GPU. Expected
values never come from the code under test: they are float64 / longdouble products on the host. Every shard's
pitch padding is NaN (ieee_cases.write_image), so a read of it poisons a column. The host and the device call
are checked against one expectation."""
import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from dot_cases import bits
from ieee_cases import write_image
from topk_cases import global_rows

pytestmark = pytest.mark.gpu
S, QMAX, START = N.GLINT_MIX_BATCH_CHUNK, N.GLINT_MIX_BATCH_MAX_VECTORS, 1_000_003  # a range shard's first row is not 0
DT = ["double", "float"]
KS = {"double": 16, "float": 32}  # requests of a slab
COLS = [2, 67, 300]  # one partial tile; the element-wise path with a tail; three column tiles, the last partial
QS = [1, 64, 65, 130]  # one vector; a full tile; a second tile of one vector; three tiles
SIZE = 300
# one request; a second slab of one; a chunk short of one; a second chunk of one; three chunks, the last 5 requests
SHAPES = [(dt, COLS[(i + j) % 3], n) for i, dt in enumerate(DT)
          for j, n in enumerate((1, KS[dt] + 1, S - 1, S + 1, 2 * S + 5))]

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


def both(sh, gpu, rows, coef):  # (what, answer) of the host call and of the device call, as numpy arrays
    return (("host", sh.getRowsMixBatch(rows, coef)),
            ("device", sh.getRowsMixBatch(dev(gpu, rows), dev(gpu, coef)).cpu().numpy()))


def chunks(n):  # the header's rule: ceil(n / L)
    length = S
    while -(-n // length) > N.GLINT_MIX_BATCH_MAX_CHUNKS:
        length *= 2
    return -(-n // length)


@pytest.mark.parametrize("dtype,cols,n", SHAPES + [("float", 2, 64 * S + 1)])
def test_exact_answer_on_integer_data(gpu, dtype, cols, n):
    """Every partial sum is an integer below 2^24: any order is exact. 64 S + 1 is the first n whose chunk
    doubles (33 chunks of 2 S)."""
    npd, rng = np_dtype(dtype), np.random.default_rng(n * 1000 + cols)
    qs = QS if n <= 2 * S + 5 else [1]
    assert chunks(n) == (33 if n == 64 * S + 1 else -(-n // S))
    img, coef, local = ints(rng, (SIZE, cols), npd), ints(rng, (n, qs[-1]), npd), request(rng, n, SIZE)
    exp = (coef.T.astype(np.float64) @ img[local].astype(np.float64)).astype(npd)
    with shard_of(gpu, dtype, img) as sh:
        for q in qs:
            for what, got in both(sh, gpu, local + START, np.ascontiguousarray(coef[:, :q])):
                assert got.dtype == npd and got.shape == (q, cols), what
                np.testing.assert_array_equal(got, exp[:q], err_msg=f"{what} q={q}")
        for what, got in both(sh, gpu, local + START, np.ascontiguousarray(coef[:, 0])):  # (n,) answers (cols,)
            assert got.shape == (cols,), what
            np.testing.assert_array_equal(got, exp[0], err_msg=f"{what} 1-d")


@pytest.mark.parametrize("dtype,cols,n", [(dt, COLS[(i + j) % 3], n) for i, dt in enumerate(DT)
                                          for j, n in enumerate((S - 1, 2 * S + 5))])
def test_within_the_bound_on_general_data(gpu, dtype, cols, n):
    npd, rng, q = np_dtype(dtype), np.random.default_rng(n + cols), 65
    if dtype == "double" and np.finfo(np.longdouble).eps > 2.0 ** -63:
        pytest.skip("longdouble is no wider than double here")
    img, coef = rng.standard_normal((SIZE, cols)).astype(npd), rng.standard_normal((n, q)).astype(npd)
    local = request(rng, n, SIZE)
    wide_rows, wide_coef = img[local].astype(np.longdouble), coef.astype(np.longdouble)
    ref, mag = wide_coef.T @ wide_rows, np.abs(wide_coef).T @ np.abs(wide_rows)
    mu = (n + chunks(n) - 1) * np.longdouble(2.0) ** (-24 if dtype == "float" else -53)
    g = mu / (1 - mu)
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, local + START, coef):
            err = np.abs(got.astype(np.longdouble) - ref)
            print(f"{what} {dtype} cols={cols} n={n}: max err / bound = {float((err / (g * mag)).max()):.3g}")
            assert (err <= g * mag).all(), what


@pytest.mark.parametrize("dtype", DT)
def test_bits_do_not_depend_on_the_position(gpu, dtype):
    npd, rng, cols, q, n = np_dtype(dtype), np.random.default_rng(6), 300, 130, 2 * S + 5
    img, coef = rng.standard_normal((SIZE, cols)).astype(npd), rng.standard_normal((n, q)).astype(npd)
    local = request(rng, n, SIZE)
    at_vectors, at_cols = [0, 63, 64, q - 1], [0, 127, 128, cols - 1]
    coef[:, at_vectors], img[:, at_cols] = coef[:, [7]], img[:, [9]]
    with shard_of(gpu, dtype, img[:, 9:10]) as one:
        alone = one.getRowsMixBatch(local + START, np.ascontiguousarray(coef[:, 7:8]))
    assert alone.shape == (1, 1)
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, local + START, coef):
            same = bits(np.ascontiguousarray(got[np.ix_(at_vectors + [7], at_cols + [9])]))
            assert (same == bits(alone)[0, 0]).all(), what


@pytest.mark.parametrize("dtype", DT)
def test_non_finite_values_and_rows_outside_the_partition(gpu, dtype):
    npd, rng, cols, q, n = np_dtype(dtype), np.random.default_rng(4), 67, 65, S + 9
    img, coef, local = ints(rng, (SIZE, cols), npd), ints(rng, (n, q), npd), request(rng, n, SIZE)
    local[local == 9] = 10
    local[7], img[9, 1] = 9, np.inf  # request 7 alone reaches the inf ...
    coef[7], coef[7, 3] = 1, 0       # ... and makes inf * 0 for vector 3 only

    def expect(keep):
        with np.errstate(invalid="ignore"):
            return (coef[keep].T[:, :, None].astype(np.float64) * img[local[keep]][None].astype(np.float64)).sum(1).astype(npd)
    everyone = np.ones(n, bool)
    exp = expect(everyone)
    assert np.isnan(exp).sum() == 1 and np.isnan(exp[3, 1]) and np.isinf(np.delete(exp[:, 1], 3)).all()
    assert np.isfinite(np.delete(exp, 1, 1)).all()
    with shard_of(gpu, dtype, img) as sh:
        for what, got in both(sh, gpu, local + START, coef):
            np.testing.assert_array_equal(got, exp, err_msg=what)
        bad = local + START
        bad[[40, S + 3]] = START - 1, START + SIZE
        coef[40], coef[S + 3] = np.inf, np.nan  # a dead request contributes 0 * 0 whatever coef holds
        out = np.full((q, cols), 77, npd)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.getRowsMixBatch(bad, coef, out=out)
        assert ei.value.record == 40 and (out == 77).all()  # nothing written
        got = sh.getRowsMixBatch(dev(gpu, bad), dev(gpu, coef), sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(got))
        assert ei.value.record == 40  # the lowest such request
        everyone[[40, S + 3]] = False
        np.testing.assert_array_equal(got.cpu().numpy(), expect(everyone))


def test_cyclic_keys_and_unaligned_coef(gpu):
    import torch
    size, cols, q, n, rng = SIZE, 300, 66, S + 5, np.random.default_rng(5)  # q * 8 is a multiple of 16
    img, coef, local = rng.standard_normal((size, cols)), rng.standard_normal((n, q)), request(rng, n, size)
    rows = global_rows(size, cyclic=(1, 3))[local]
    with shard_of(gpu, "double", img, part=CyclicPartition(1, 3, 3 * size)) as sh:
        buf = torch.zeros(n * q + 4, dtype=torch.float64, device=torch.device("cuda", gpu))
        answers = []
        for shift in (0, 1):  # one element past a 16-B boundary: coef is read element by element
            view = buf[shift:shift + n * q].copy_(dev(gpu, coef).reshape(-1))
            assert view.data_ptr() % 16 == 8 * shift
            answers.append(sh.getRowsMixBatch(dev(gpu, rows), view.view(n, q)).cpu().numpy())
        np.testing.assert_array_equal(bits(answers[0]), bits(answers[1]))
        np.testing.assert_array_equal(bits(answers[0]), bits(sh.getRowsMixBatch(rows, coef)))
        # the contract's bound, twice: the float64 reference has the same one
        mu = (n + 1) * 2.0 ** -53
        assert (np.abs(answers[0] - coef.T @ img[local]) <= 2 * mu / (1 - mu) * (np.abs(coef).T @ np.abs(img[local]))).all()


def test_argument_errors(gpu):
    lib, coef, rows, out = N.load(), np.ones((3, 2)), np.full(3, START, np.int64), np.full((2, 4), 77.0)
    coefd, rowsd, outd = dev(gpu, coef), dev(gpu, rows), dev(gpu, out)
    devc = lambda h, r, n, cp, q, o: lib.glint_mat_pull_rows_mix_batch_dev(h, r, n, cp, q, o, None)  # noqa: E731
    calls = ((lib.glint_mat_pull_rows_mix_batch, [a.ctypes.data for a in (rows, coef, out)]),
             (devc, [a.data_ptr() for a in (rowsd, coefd, outd)]))
    for dtype in ("int", "long"):
        with PartialMatrix(RangePartition(0, START, START + 10), 4, dtype, gpu) as sh:
            for call, (rp, cp, op) in calls:
                assert call(sh.handle, rp, 3, cp, 2, op) == N.GLINT_EINVAL
            with pytest.raises(TypeError):
                sh.getRowsMixBatch(rows, np.ones((3, 2), sh.np_dtype))
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        for call, (rp, cp, op) in calls:
            assert call(vec.handle, rp, 3, cp, 1, op) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        for call, (rp, cp, op) in calls:
            for n, q in ((3, 0), (3, QMAX + 1), (-1, 2)):
                assert call(sh.handle, rp, n, cp, q, op) == N.GLINT_EINVAL
            assert call(sh.handle, rp, 3, None, 2, op) == N.GLINT_EINVAL  # NULL coef
            assert call(sh.handle, None, 0, None, 2, op) == N.GLINT_OK  # n == 0 writes q x cols zeros
        sh.sync(None)
        assert not bits(out).any() and not bits(outd.cpu().numpy()).any()
        assert sh.getRowsMixBatch(rows[:0], coef[:0]).shape == (2, 4)
        with pytest.raises(TypeError):
            sh.getRowsMixBatch(rows, None)
        for wrong in (np.ones((2, 2)), np.ones((3, 0)), np.ones((3, QMAX + 1)), np.ones(4)):
            with pytest.raises(ValueError):
                sh.getRowsMixBatch(rows, wrong)
