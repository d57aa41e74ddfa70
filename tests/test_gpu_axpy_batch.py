"""Batched row axpy push (PartialMatrix.updateRowsAxpyBatch, glint_mat_push_rows_axpy_batch*) on the GPU.
Expected values never come from the code under test: they are float64 / longdouble sums on the host, record
by record in push order. Every shard's pitch padding is NaN (ieee_cases.write_image) and the whole image,
padding included, is read back, so a touched padding element or a touched row that was not named shows. The
host call and the device call are checked against one expectation."""
import ctypes as C

import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from dot_cases import bits
from ieee_cases import write_image
from topk_cases import global_rows

pytestmark = pytest.mark.gpu
R, QMAX, START = 128, N.GLINT_AXPY_BATCH_MAX_VECTORS, 1_000_003  # the tile is R distinct rows
DT = ["double", "float"]
COLS = [2, 67, 300]  # below one column block; by element with a partial second pass; by 16 B, the fifth pass partial
US = [1, R - 1, R + 1, 2 * R + 3]  # distinct rows
QS = [1, 16, 17, 33, 130]  # a whole Double slab at 16, one into the next at 17, one into the second Float slab at 33
SIZE = 300
HOW = ["host", "device"]

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


def image(sh, gpu, size):  # the shard's memory as it lies: (size, pitch)
    import torch
    pitch = C.c_int64()
    assert N.load().glint_shard_pitch(sh.handle, C.byref(pitch)) == N.GLINT_OK
    dst = torch.empty((size, pitch.value), dtype=sh.torch_dtype, device=torch.device("cuda", gpu))
    segs = np.array([0, 0, dst.numel() * dst.element_size()], np.int64)
    assert N.load().glint_copy_segments_dev(sh.data_ptr(), dst.data_ptr(), segs.ctypes.data_as(C.POINTER(C.c_int64)),
                                            1, torch.cuda.current_stream(dst.device).cuda_stream) == N.GLINT_OK
    torch.cuda.synchronize(dst.device)
    return dst.cpu().numpy()


def records(rng, u, size):  # local rows of u distinct rows, 1 to 3 records each and 70 of one, shuffled
    named = rng.permutation(size)[:u]
    times = rng.integers(1, 4, u)
    times[u // 2] = 70  # past run_sum's block of 64 records
    return rng.permutation(np.repeat(named, times)).astype(np.int64)


def push(sh, gpu, how, rows, coef, x, **kw):
    if how == "device":
        rows, coef, x = dev(gpu, rows), dev(gpu, coef), dev(gpu, x)
    sh.updateRowsAxpyBatch(rows, coef, x, **kw)
    return rows


def reference(start, local, coef, x, wide):  # start + the records' contributions, one by one in push order
    exp, coef, x = start.astype(wide), coef.astype(wide), x.astype(wide)
    with np.errstate(invalid="ignore"):
        for i, l in enumerate(local):
            exp[l] += (coef[i][:, None] * x).sum(0)  # every product is formed: 0 * inf is NaN
    return exp


def check_image(sh, gpu, exp, what):
    raw, cols = image(sh, gpu, exp.shape[0]), exp.shape[1]
    np.testing.assert_array_equal(raw[:, :cols], exp.astype(raw.dtype), err_msg=what)
    assert np.isnan(raw[:, cols:]).all(), what  # the padding is neither read into a sum nor written


@pytest.mark.parametrize("dtype,cols,u", [(dt, COLS[(i + j) % 3], u) for i, dt in enumerate(DT) for j, u in enumerate(US)])
def test_exact_on_integer_data(gpu, dtype, cols, u):
    """Every partial sum is an integer far below 2^24: any order is exact. The pushes accumulate on one shard."""
    npd, rng = np_dtype(dtype), np.random.default_rng(u * 1000 + cols)
    exp, local = ints(rng, (SIZE, cols), npd).astype(np.float64), records(rng, u, SIZE)
    coef, x = ints(rng, (local.size, QS[-1]), npd), ints(rng, (QS[-1], cols), npd)
    with shard_of(gpu, dtype, exp.astype(npd)) as sh:
        for q in QS:
            for how in HOW:
                push(sh, gpu, how, local + START, np.ascontiguousarray(coef[:, :q]), x[:q])
                exp = reference(exp, local, coef[:, :q], x[:q], np.float64)
                check_image(sh, gpu, exp, f"{how} q={q}")
        push(sh, gpu, "host", local + START, coef[:, 3].copy(), x[3])  # x of shape (cols,), coef (n,): q = 1
        check_image(sh, gpu, reference(exp, local, coef[:, 3:4], x[3:4], np.float64), "1-d")
        assert np.abs(exp).max() < 2 ** 23


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("cols", COLS)
def test_within_the_bound_on_general_data(gpu, dtype, cols):
    npd, rng, q = np_dtype(dtype), np.random.default_rng(cols), 65
    if dtype == "double" and np.finfo(np.longdouble).eps > 2.0 ** -63:
        pytest.skip("longdouble is no wider than double here")
    local = records(rng, R + 1, SIZE)
    img, coef, x = (rng.standard_normal(s).astype(npd) for s in ((SIZE, cols), (local.size, q), (q, cols)))
    ref = reference(img, local, coef, x, np.longdouble)
    mag = reference(np.abs(img), local, np.abs(coef), np.abs(x), np.longdouble)  # |row| + |coef| (.) |x|
    mu = (np.bincount(local, minlength=SIZE) + q) * np.longdouble(2.0) ** (-24 if dtype == "float" else -53)
    bound = (mu / (1 - mu))[:, None] * mag  # each row's own m
    for how in HOW:
        with shard_of(gpu, dtype, img) as sh:
            push(sh, gpu, how, local + START, coef, x)
            err = np.abs(image(sh, gpu, SIZE)[:, :cols].astype(np.longdouble) - ref)
        named = np.bincount(local, minlength=SIZE) > 0
        print(f"{how} {dtype} cols={cols}: max err / bound = {float((err[named] / bound[named]).max()):.3g}")
        assert (err <= bound).all() and not err[~named].any(), how


@pytest.mark.parametrize("dtype,cols,cyclic", [("float", 300, None), ("double", 300, (1, 3)), ("float", 67, None)])
def test_bits_do_not_depend_on_the_batch(gpu, dtype, cols, cyclic):
    """One row's three records, alone and as the first, the R-th and the last distinct row of a larger push with
    the other rows' records between its own; then coef and x one element past a 16-B boundary."""
    import torch
    npd, rng, q, size = np_dtype(dtype), np.random.default_rng(cols), 68, 2 * R + 20  # 68 vectors: coef by 16 B
    x, mine = rng.standard_normal((q, cols)).astype(npd), rng.standard_normal((3, q)).astype(npd)
    named = np.arange(5, 5 + 2 * R + 3)
    part = CyclicPartition(cyclic[0], cyclic[1], cyclic[1] * size) if cyclic else None
    glob = global_rows(size, START, cyclic)
    zeros = np.zeros((size, cols), npd)

    def row_after(how, local, coef, target, shift=0):
        with shard_of(gpu, dtype, zeros, part=part) as sh:
            if shift is None:
                push(sh, gpu, how, glob[local], coef, x)
            else:  # device tensors at `shift` elements past an aligned address
                bufs = [torch.zeros(a.size + 4, dtype=sh.torch_dtype, device=torch.device("cuda", gpu)) for a in (coef, x)]
                views = [b[shift:shift + a.size].copy_(dev(gpu, a).reshape(-1)).view(a.shape) for b, a in zip(bufs, (coef, x))]
                assert all(v.data_ptr() % 16 == shift * v.element_size() for v in views)
                sh.updateRowsAxpyBatch(dev(gpu, glob[local]), *views)
            return bits(image(sh, gpu, size)[target, :cols])

    alone = row_after("host", np.full(3, 7), mine, 7, shift=None)
    assert alone.any()
    for target in (named[0], named[R - 1], named[-1]):
        others = rng.permutation(np.repeat(named[named != target], 2))
        at = np.sort(rng.choice(others.size + 3, 3, replace=False))  # its records keep their order
        local, coef = np.empty(others.size + 3, np.int64), rng.standard_normal((others.size + 3, q)).astype(npd)
        local[at], coef[at] = target, mine
        local[np.setdiff1d(np.arange(local.size), at)] = others
        for how, shift in (("host", None), ("device", 0), ("device", 1)) if cols == 300 else (("host", None),):
            np.testing.assert_array_equal(row_after(how, local, coef, target, shift), alone, err_msg=f"{target} {how} {shift}")


@pytest.mark.parametrize("dtype", DT)
def test_non_finite_values_and_rows_outside_the_partition(gpu, dtype):
    npd, rng, cols, q = np_dtype(dtype), np.random.default_rng(4), 67, 33
    local = records(rng, R + 9, SIZE)
    img, coef, x = ints(rng, (SIZE, cols), npd), ints(rng, (local.size, q), npd), ints(rng, (q, cols), npd)
    x[x == 0], coef[:, 7] = 1, 0
    hot = np.flatnonzero(local == local[0])
    coef[hot[0], 2], coef[hot[-1], 5] = np.inf, np.nan  # one row's coefficients: that row only
    x[7, 11] = np.inf  # against zero coefficients: NaN in column 11 of every named row
    exp = reference(img, local, coef, x, np.float64)
    named = np.bincount(local, minlength=SIZE) > 0
    assert np.isnan(exp[local[0]]).all() and (np.isnan(exp).sum(1) == named)[np.arange(SIZE) != local[0]].all()
    for how in HOW:
        with shard_of(gpu, dtype, img) as sh:
            push(sh, gpu, how, local + START, coef, x)
            check_image(sh, gpu, exp, how)
    bad = local + START
    bad[[40, R + 3]] = START - 1, START + SIZE
    with shard_of(gpu, dtype, img) as sh:
        before = bits(image(sh, gpu, SIZE))
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.updateRowsAxpyBatch(bad, coef, x)
        assert ei.value.record == 40
        np.testing.assert_array_equal(bits(image(sh, gpu, SIZE)), before)  # nothing applied
        rows = push(sh, gpu, "device", bad, coef, x, sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.sync(sh._stream_of(rows))
        assert ei.value.record == 40  # the lowest such record
        keep = np.setdiff1d(np.arange(local.size), [40, R + 3])
        check_image(sh, gpu, reference(img, local[keep], coef[keep], x, np.float64), "skipped")


def test_argument_errors(gpu):
    lib, x, rows, coef = N.load(), np.ones((2, 4)), np.full(3, START, np.int64), np.ones((3, 2))
    devc = lambda h, r, n, c, xp, q, f: lib.glint_mat_push_rows_axpy_batch_dev(h, r, n, c, xp, q, f, None)  # noqa: E731
    calls = ((lib.glint_mat_push_rows_axpy_batch, [a.ctypes.data for a in (rows, coef, x)]),
             (devc, [a.data_ptr() for a in (dev(gpu, rows), dev(gpu, coef), dev(gpu, x))]))
    for dtype in ("int", "long"):
        with PartialMatrix(RangePartition(0, START, START + 10), 4, dtype, gpu) as sh:
            for call, (rp, cp, xp) in calls:
                assert call(sh.handle, rp, 3, cp, xp, 2, 0) == N.GLINT_EINVAL
            with pytest.raises(TypeError):
                sh.updateRowsAxpyBatch(rows, np.ones((3, 2), sh.np_dtype), np.ones((2, 4), sh.np_dtype))
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        for call, (rp, cp, xp) in calls:
            assert call(vec.handle, rp, 3, cp, xp, 1, 0) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        for call, (rp, cp, xp) in calls:
            for n, q, flag in ((3, 0, 0), (3, QMAX + 1, 0), (-1, 2, 0), (3, 2, N.GLINT_PUSH_DETERMINISTIC), (3, 2, 64)):
                assert call(sh.handle, rp, n, cp, xp, q, flag) == N.GLINT_EINVAL
            assert call(sh.handle, rp, 3, None, xp, 2, 0) == N.GLINT_EINVAL
            assert call(sh.handle, rp, 3, cp, None, 2, 0) == N.GLINT_EINVAL
            assert call(sh.handle, None, 0, None, None, 2, 0) == N.GLINT_OK  # n == 0 launches nothing
        sh.sync(None)
        assert not sh.to_numpy().any()
        for call, (rp, cp, xp) in calls:
            assert call(sh.handle, rp, 3, cp, xp, 2, 0) == N.GLINT_OK
        sh.sync(None)
        assert (sh.to_numpy()[0] == 12).all() and not sh.to_numpy()[1:].any()  # 2 calls x 3 records x 2 vectors of ones
        with pytest.raises(ValueError):
            sh.updateRowsAxpyBatch(rows, np.ones((3, 3)), x)
        with pytest.raises(ValueError):
            sh.updateRowsAxpyBatch(rows, np.ones((3, QMAX + 1)), np.ones((QMAX + 1, 4)))
