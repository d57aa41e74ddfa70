"""Expected values of the row dot-product pull, shared by test_dot_cpu.py and test_gpu_dot.py.

Nothing here calls the code under test. A dot is replayed in the order include/glint_gpu.h fixes, in the
shard's dtype: elementwise numpy products (each rounded), 64 lane sums that start from +0 and take their
own columns' products in ascending column order -- column c belongs to lane (c // E) % 64 -- and then the
six steps of the xor butterfly."""
import functools
import zlib

import numpy as np

LANES = 64


def lane_width(dtype, cols):
    """E: the columns a lane holds per strip -- 16 bytes' worth when a row is a whole number of 16-B
    pieces, else one."""
    size = np.dtype(dtype).itemsize
    return 16 // size if (cols * size) % 16 == 0 else 1


def reduce_products(prod, E):
    """The contract's sum over the last axis of `prod` (..., cols), in prod's dtype; int dtypes wrap."""
    prod = np.asarray(prod)
    dt, cols = prod.dtype, prod.shape[-1]
    acc = np.zeros(prod.shape[:-1] + (LANES,), dt)
    lane = np.arange(LANES)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        for s in range(0, cols, LANES * E):  # strip by strip
            for e in range(E):  # a lane's columns of the strip, ascending
                c = s + lane * E + e
                k = int((c < cols).sum())  # the lanes that have such a column: a prefix
                acc[..., :k] = np.add(acc[..., :k], prod[..., c[:k]], dtype=dt)
        for d in (32, 16, 8, 4, 2, 1):
            acc = np.add(acc, acc[..., lane ^ d], dtype=dt)
    assert (bits(acc) == bits(acc[..., :1])).all() or np.isnan(acc).any()  # addition commutes
    return np.ascontiguousarray(acc[..., 0])


def replay_dot(table_rows, x, E=None):
    """table_rows (n, cols) against x: (cols,) -> (n,); (q, cols) -> (n, q). E defaults to the
    contract's for (dtype, cols)."""
    rows = np.asarray(table_rows)
    x = np.asarray(x, dtype=rows.dtype)
    if E is None:
        E = lane_width(rows.dtype, rows.shape[1])
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        if x.ndim == 1:
            return reduce_products(np.multiply(rows, x, dtype=rows.dtype), E)
        return reduce_products(np.multiply(rows[:, None, :], x[None, :, :], dtype=rows.dtype), E)


def replay_self(table_rows, E=None):
    """(n,): every row against itself."""
    rows = np.asarray(table_rows)
    if E is None:
        E = lane_width(rows.dtype, rows.shape[1])
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return reduce_products(np.multiply(rows, rows, dtype=rows.dtype), E)


def bits(a):
    """Raw integer view, so that -0.0 and subnormals compare by their bits."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def assert_dot_bits(got, exp, what=""):
    """Bit for bit; a NaN is compared by class (its payload and sign are unspecified)."""
    got = got.cpu().numpy() if hasattr(got, "cpu") else np.asarray(got)
    assert got.dtype == exp.dtype and got.shape == exp.shape, what
    if np.issubdtype(exp.dtype, np.floating):
        nan = np.isnan(exp)
        np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
        got, exp = np.where(nan, 0, got), np.where(nan, 0, exp)
    np.testing.assert_array_equal(bits(got), bits(exp), err_msg=what)


# ---- known answers: a fused multiply-add shows ---------------------------------------------------
# a * a = 1 + 2u + u^2 rounds to b = 1 + 2u (u^2 is a quarter of an ulp), so -b * 1 + a * a is exactly 0
# with rounded products, while a fused a * a + (-b) keeps the u^2: 2^-54 (Double), 2^-24 (Float).
NOFMA = {
    np.float64: (1.0 + 2.0 ** -27, 1.0 + 2.0 ** -26, 2.0 ** -54),
    np.float32: (np.float32(1.0 + 2.0 ** -12), np.float32(1.0 + 2.0 ** -11), 2.0 ** -24),
}
# (cols, column of -b / 1, column of a / a): both columns in lane 0, so one lane's chain adds them --
# in one strip on the 16-B path (Double cols 2, Float cols 4), in strips 0 and 1 otherwise. The
# issue's (cols 2) and (cols 67, columns 0 and 64) cases are the first two of each type.
NOFMA_PLACES = {
    np.float64: [(2, 0, 1), (67, 0, 64), (512, 0, 128)],
    np.float32: [(2, 0, 1), (67, 0, 64), (4, 0, 1), (512, 0, 256)],
}


def nofma_case(npd, cols, c0, c1):
    """(row, x, fused): row . x is 0 by the contract; `fused` is what contraction would give."""
    a, b, fused = NOFMA[npd]
    row, x = np.zeros(cols, npd), np.zeros(cols, npd)
    row[c0], x[c0] = -b, 1
    row[c1], x[c1] = a, a
    return row, x, npd(fused)


# ---- shard contents and requests of the GPU tests ------------------------------------------------
@functools.lru_cache(maxsize=None)
def fill_values(npd, cols, size, what="table"):
    """Random rows; read-only, shared. Int/Long lie anywhere in the type, so products and sums wrap;
    Float/Double span nine decades, so the order of a sum shows."""
    npd = np.dtype(npd).type
    rng = np.random.default_rng(zlib.crc32(f"dot/{what}/{np.dtype(npd).name}/{cols}".encode()))
    if np.issubdtype(npd, np.floating):
        v = (rng.standard_normal((size, cols)) * 10.0 ** rng.integers(-4, 5, (size, cols))).astype(npd)
    else:
        info = np.iinfo(npd)
        v = rng.integers(info.min, info.max, (size, cols), dtype=npd, endpoint=True)
    v.setflags(write=False)
    return v
