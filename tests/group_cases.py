"""Expected values of the grouped row push, shared by test_group_cpu.py and test_gpu_group.py.

Nothing here calls the code under test. A grouped push is the row push's replay (axpy_cases.fold_rows) of
the contribution rows ``values[group of record i]`` -- as they are stored, no arithmetic -- or, with
coefficients, ``coef[i] * values[group of record i]``: one numpy multiply, each product rounded on its own."""
import functools
import zlib

import numpy as np

from axpy_cases import fold_rows
from dot_cases import bits  # noqa: F401  (re-exported for the tests)


def group_of(offsets, n):
    """offsets (g + 1,), non-decreasing from 0 to n -> (n,) the group of every record."""
    offsets = np.asarray(offsets, np.int64).reshape(-1)
    assert offsets.size >= 1 and offsets[0] == 0 and offsets[-1] == n and (np.diff(offsets) >= 0).all()
    return np.repeat(np.arange(offsets.size - 1, dtype=np.int64), np.diff(offsets))


def group_contrib(values, group, coef=None):
    """values (g, cols), group (n,) -> the (n, cols) contribution rows: values[group] as stored or, with
    coef (n,), coef[i] * values[group[i]], one rounded product per element; int dtypes wrap."""
    values = np.asarray(values)
    assert values.ndim == 2
    t = values[np.asarray(group, np.int64)]
    if coef is None:
        return t
    coef = np.asarray(coef, dtype=values.dtype).reshape(-1)
    assert coef.size == t.shape[0]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.multiply(coef[:, None], t, dtype=values.dtype)


def replay_grouped(table, local, offsets, values, coef=None, order=None):
    """table (size, cols) with record i's contribution added into row local[i], record by record in `order`
    (default: as given): the sequential loop a strict grouped push equals."""
    return fold_rows(table, local, group_contrib(values, group_of(offsets, len(local)), coef), order)


# ---- the inputs that show what the contract fixes -----------------------------------------------------
def order_inputs(npd):
    """600 records over 40 rows in 48 groups of random cut points, several of them forced empty (the first,
    the last and some in the middle), cols = 67, magnitudes over nine decades:
    (local rows, offsets, values (48, 67), coef (600,), table (40, 67))."""
    rng = np.random.default_rng(23)
    n, rows_n, g, cols = 600, 40, 48, 67
    mixed = lambda *shape: (rng.standard_normal(shape) * 10.0 ** rng.integers(-4, 5, shape)).astype(npd)  # noqa: E731
    local = rng.integers(0, rows_n, n)
    cuts = np.sort(rng.integers(0, n + 1, g - 1))
    offsets = np.concatenate(([0], cuts, [n])).astype(np.int64)
    for k in (0, 7, 8, 30, g - 1):  # empty groups: the cut behind k falls on the one in front of it
        if k == g - 1:
            offsets[k] = n
        else:
            offsets[k + 1] = offsets[k]
    offsets = np.maximum.accumulate(offsets)
    return local, offsets, mixed(g, cols), mixed(n), mixed(rows_n, cols)


# ---- shared inputs of the GPU tests -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def group_values(dtype_name, rows, cols, what="values"):
    """A (rows, cols) array; read-only, shared. Int/Long lie anywhere in the type, so products and sums
    wrap; Float/Double span nine decades, so the order of a sum shows."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"group/{what}/{dtype_name}/{rows}/{cols}".encode()))
    if np.issubdtype(npd, np.floating):
        v = (rng.standard_normal((rows, cols)) * 10.0 ** rng.integers(-4, 5, (rows, cols))).astype(npd)
    else:
        info = np.iinfo(npd)
        v = rng.integers(info.min, info.max, (rows, cols), dtype=npd, endpoint=True)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def group_coef(dtype_name, n, what="coef"):
    """(n,) coefficients of the same kind; read-only, shared."""
    v = np.array(group_values(dtype_name, n, 1, what)).reshape(-1)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def group_records(size):
    """(local rows (n,), offsets (g + 1,)) of the GPU parity grid, about 700 records over a shard of `size`
    >= 300 rows; read-only, shared. Runs (records per destination row) of length 1 (many), 2, 9 -- past the
    8 loads in flight --, 70 -- past one 64-record batch -- and 300 -- split into chunks when the order is
    free. Groups that are empty (the first, two in the middle, the last), of one record, and of more than
    64 records; a row repeated inside a group and across groups."""
    rng = np.random.default_rng(42)
    hot = [(5, 300), (17, 70), (29, 9), (41, 2)]  # (local row, run length)
    rest = rng.permutation(np.setdiff1d(np.arange(size), [r for r, _ in hot]))
    local = np.concatenate([np.full(k, r, np.int64) for r, k in hot] +
                           [rest[:150].astype(np.int64),                        # rows named once
                            rng.choice(rest[150:210], 169).astype(np.int64)])   # short runs
    local = local[rng.permutation(local.size)]
    n = local.size  # 700
    sizes = [0, 1, 1, 100, 0, 0, 3, 70, 8, 1, 65]  # the first empty, of one record, of more than 64, ...
    while sum(sizes) < n - 40:
        sizes.append(int(rng.integers(1, 40)))
    sizes += [n - sum(sizes), 0]  # ... and the last empty
    offsets = np.concatenate(([0], np.cumsum(sizes))).astype(np.int64)
    assert offsets[-1] == n
    local.setflags(write=False)
    offsets.setflags(write=False)
    return local, offsets
