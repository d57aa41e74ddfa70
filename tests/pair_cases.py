"""Expected values of the row-pair dot pull and the row-pair axpy push, shared by test_pair_cpu.py and
test_gpu_pair.py.

Nothing here calls the code under test. A pair dot is the row dot pull's replay (dot_cases) with the second
shard's stored row in the place of the caller's vector: elementwise numpy products, each rounded, reduced in
the contract's order. A pair axpy is the row push's replay (axpy_cases.fold_rows) of the contribution rows
``coef[i] * (source row i)``, one numpy multiply, each product rounded on its own."""
import functools
import zlib

import numpy as np

from axpy_cases import fold_rows
from dot_cases import bits, lane_width, reduce_products  # noqa: F401  (bits: re-exported for the tests)


def replay_pair_dot(a_rows, b_rows, E=None):
    """a_rows, b_rows (n, cols), the rows of the two shards pair by pair -> (n,) dots in their dtype. E
    defaults to the contract's for (dtype, cols)."""
    a = np.asarray(a_rows)
    b = np.asarray(b_rows, dtype=a.dtype)
    assert a.shape == b.shape and a.ndim == 2
    if E is None:
        E = lane_width(a.dtype, a.shape[1])
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return reduce_products(np.multiply(a, b, dtype=a.dtype), E)


def pair_contrib(coef, src_rows):
    """coef (n,), src_rows (n, cols) -> the (n, cols) contribution rows coef[i] * src_rows[i], one rounded
    product per element, in src_rows' dtype; int dtypes wrap."""
    src = np.asarray(src_rows)
    coef = np.asarray(coef, dtype=src.dtype).reshape(-1)
    assert src.ndim == 2 and coef.size == src.shape[0]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.multiply(coef[:, None], src, dtype=src.dtype)


def replay_pair_axpy(table, local, coef, src_rows, order=None):
    """table (size, cols) with coef[i] * src_rows[i] added into row local[i], record by record in `order`
    (default: as given): the sequential loop a strict pair axpy equals. src_rows (n, cols) are the source
    rows as they were before the call."""
    return fold_rows(table, local, pair_contrib(coef, src_rows), order)


# ---- the inputs that show what the contract fixes -----------------------------------------------------
def order_inputs(npd):
    """600 pairs over 40 destination rows and 40 source rows, cols = 67, magnitudes over nine decades:
    (dst local rows, src local rows, coef, dst table, src table)."""
    rng = np.random.default_rng(11)
    n, rows_n, cols = 600, 40, 67
    mixed = lambda *shape: (rng.standard_normal(shape) * 10.0 ** rng.integers(-4, 5, shape)).astype(npd)  # noqa: E731
    ld = rng.integers(0, rows_n, n)
    ls = rng.integers(0, rows_n, n)
    return ld, ls, mixed(n), mixed(rows_n, cols), mixed(rows_n, cols)


# ---- shared inputs of the GPU tests -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def pair_values(dtype_name, rows, cols, what="table"):
    """A (rows, cols) table; read-only, shared. Int/Long lie anywhere in the type, so products and sums
    wrap; Float/Double span nine decades, so the order of a sum shows."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"pair/{what}/{dtype_name}/{rows}/{cols}".encode()))
    if np.issubdtype(npd, np.floating):
        v = (rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-4, 5, (rows, cols))).astype(npd)
    else:
        info = np.iinfo(npd)
        v = rng.integers(info.min, info.max, (rows, cols), dtype=npd, endpoint=True)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def pair_coef(dtype_name, n, what="coef"):
    """(n,) coefficients of the same kind; read-only, shared."""
    v = np.array(pair_values(dtype_name, n, 1, what)).reshape(-1)
    v.setflags(write=False)
    return v
