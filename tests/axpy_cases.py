"""Expected values of the row axpy push, shared by test_axpy_cpu.py and test_gpu_axpy.py.

Nothing here calls the code under test. A push's contribution rows are replayed in the order
include/glint_gpu.h fixes, in the shard's dtype: t_i = ((coef[i][0] * x[0]) + (coef[i][1] * x[1])) + ...,
every product an elementwise numpy product (rounded on its own), added left to right from the first
product. The push is then the row push of those rows."""
import functools
import zlib

import numpy as np

from dot_cases import NOFMA, bits  # noqa: F401  (re-exported for the tests)


def replay_contrib(coef, x):
    """coef (n, q) or (n,), x (q, cols) or (cols,) -> the (n, cols) contribution rows, in x's dtype; int
    dtypes wrap."""
    x = np.asarray(x)
    dt = x.dtype
    if x.ndim == 1:
        x = x[None]
    coef = np.asarray(coef, dtype=dt).reshape(-1, x.shape[0])
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        t = np.multiply(coef[:, 0:1], x[0][None, :], dtype=dt)
        for j in range(1, x.shape[0]):
            t = np.add(t, np.multiply(coef[:, j:j + 1], x[j][None, :], dtype=dt), dtype=dt)
    return t


def fold_rows(table, local, contrib, order=None):
    """table (size, cols) with contribution row i added into row local[i], record by record in `order`
    (default: as given), in the table's dtype: the sequential loop a strict push equals."""
    out = np.array(table)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for i in (range(len(local)) if order is None else order):
            out[local[i]] = np.add(out[local[i]], contrib[i], dtype=out.dtype)
    return out


def assert_bits(got, exp, what=""):
    """Bit for bit; a NaN is compared by class (its payload and sign are unspecified)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    if np.issubdtype(exp.dtype, np.floating):
        nan = np.isnan(exp)
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
        got, exp = np.where(nan, 0, got), np.where(nan, 0, exp)
    np.testing.assert_array_equal(bits(got), bits(exp), err_msg=what)


# ---- known answers: a fused multiply-add shows (NOFMA: a * a rounds to b) ---------------------------
def nofma_element(npd, cols, c):
    """(element row, coef (1, 1), x (1, cols), fused): the element -b plus the contribution a * a is
    exactly +0 in column c; a fused add of the product to the element would leave `fused`."""
    a, b, fused = NOFMA[npd]
    row, x = np.zeros(cols, npd), np.zeros((1, cols), npd)
    row[c], x[0, c] = -b, a
    return row, np.full((1, 1), a, npd), x, npd(fused)


def nofma_inner(npd, cols, c):
    """(coef (1, 2), x (2, cols), fused): (1 * -b) + (a * a) is exactly 0 in column c; a fused second
    term would leave `fused`."""
    a, b, fused = NOFMA[npd]
    x = np.zeros((2, cols), npd)
    x[0, c], x[1, c] = -b, a
    return np.array([[1, a]], npd), x, npd(fused)


# ---- the inputs that show the order -----------------------------------------------------------------
def order_inputs(npd):
    """600 records over 40 rows, q = 3, cols = 67, magnitudes over nine decades."""
    rng = np.random.default_rng(5)
    n, rows_n, q, cols = 600, 40, 3, 67
    local = rng.integers(0, rows_n, n)
    coef = (rng.standard_normal((n, q)) * 10.0 ** rng.integers(-4, 5, (n, q))).astype(npd)
    x = (rng.standard_normal((q, cols)) * 10.0 ** rng.integers(-4, 5, (q, cols))).astype(npd)
    return local, coef, x, rows_n


# ---- shared inputs of the GPU tests -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def axpy_inputs(dtype_name, n, q, cols, what="case"):
    """(coef (n, q), x (q, cols)); read-only, shared. Int/Long lie anywhere in the type, so products and
    sums wrap; Float/Double span nine decades, so the order of a sum shows."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"axpy/{what}/{dtype_name}/{n}/{q}/{cols}".encode()))
    if np.issubdtype(npd, np.floating):
        coef = (rng.standard_normal((n, q)) * 10.0 ** rng.integers(-4, 5, (n, q))).astype(npd)
        x = (rng.standard_normal((q, cols)) * 10.0 ** rng.integers(-4, 5, (q, cols))).astype(npd)
    else:
        info = np.iinfo(npd)
        coef = rng.integers(info.min, info.max, (n, q), dtype=npd, endpoint=True)
        x = rng.integers(info.min, info.max, (q, cols), dtype=npd, endpoint=True)
    coef.setflags(write=False)
    x.setflags(write=False)
    return coef, x
