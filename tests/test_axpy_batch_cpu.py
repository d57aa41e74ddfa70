"""Batched row axpy push without a GPU: the ABI's symbols, constants and NULL-shard check, and
BigMatrix.pushAxpyBatch's bucketing and shape checks over fake shards."""
from pathlib import Path

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix


def test_symbols_constants_and_version():
    lib = N.load()
    text = (Path(__file__).resolve().parent.parent / "include" / "glint_gpu.h").read_text()
    assert f"#define GLINT_AXPY_BATCH_MAX_VECTORS {N.GLINT_AXPY_BATCH_MAX_VECTORS}\n" in text
    assert N.GLINT_AXPY_BATCH_MAX_VECTORS == 1024 == N.GLINT_DOT_MAX_QUERIES
    assert N.GLINT_AXPY_MAX_VECTORS == 64 and "#define GLINT_AXPY_MAX_VECTORS 64\n" in text and N.GLINT_K_COUNT == 13
    assert lib.glint_version() > 2100  # glint_version() at the parent of the batched row axpy push
    assert callable(glint_amd.PartialMatrix.updateRowsAxpyBatch) and callable(glint_amd.BigMatrix.pushAxpyBatch)
    rows, coef, x = np.zeros(1, np.int64), np.zeros(1), np.zeros(4)  # a NULL shard
    args = (None, rows.ctypes.data, 1, coef.ctypes.data, x.ctypes.data, 1, 0)
    assert lib.glint_mat_push_rows_axpy_batch(*args) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_axpy_batch_dev(*args, None) == N.GLINT_EINVAL


class FakeShard:
    """Applies updateRowsAxpyBatch to its rows of an integer-valued table (exact sums) and counts the calls."""
    def __init__(self, start, size, cols):
        self.start, self.table, self.calls, self.np_dtype = start, np.zeros((size, cols)), 0, np.float64

    def updateRowsAxpyBatch(self, rows, coef, x):
        self.calls += 1
        np.add.at(self.table, rows - self.start, coef.reshape(rows.size, -1) @ x.reshape(-1, self.table.shape[1]))
        return True


def model(cols=7):
    partitioner = RangePartitioner.apply(3, 300)
    shards = [FakeShard(p.start, p.end - p.start, cols) for p in partitioner.all()]
    return shards, BigMatrix(partitioner, shards, 300, cols)


def test_push_axpy_batch_buckets_as_push_axpy():
    shards, m = model()
    rng = np.random.default_rng(8)
    rows = np.concatenate([rng.integers(100, 300, 150), rng.integers(100, 300, 30)])  # nothing from partition 0
    coef, x = rng.integers(-2, 3, (180, 70)).astype(np.float64), rng.integers(-2, 3, (70, 7)).astype(np.float64)
    assert m.pushAxpyBatch(rows, coef, x) and m.pushAxpyBatch(rows, coef[:, 4], x[4])  # x of shape (cols,): q = 1
    want = np.zeros((300, 7))
    np.add.at(want, rows, coef @ x + np.outer(coef[:, 4], x[4]))
    np.testing.assert_array_equal(np.concatenate([sh.table for sh in shards]), want)
    assert [sh.calls for sh in shards] == [0, 2, 2]  # one call per partition that owns a row
    assert m.pushAxpyBatch(np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros((4, 7)))
    assert [sh.calls for sh in shards] == [0, 2, 2]


def test_push_axpy_batch_rejects_before_any_shard_is_called():
    shards, m = model()
    z = np.zeros
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAxpyBatch(np.array([3, 299, 300, 5], np.int64), z(4), z(7))
    for coef, x in ((z(2), z(6)), (z((2, 2)), z((2, 8))), (z((2, 0)), z((0, 7))), (z(2), z((2, 7))), (z((3, 2)), z((2, 7)))):
        with pytest.raises(ValueError):
            m.pushAxpyBatch(np.array([3, 4], np.int64), coef, x)
    assert not any(sh.calls for sh in shards)
