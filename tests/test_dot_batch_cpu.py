"""Batched row dot pull without a GPU: the ABI's symbols, constant and NULL-shard check, and
BigMatrix.pullDotBatch's fan-out and scatter over fake shards."""
from pathlib import Path

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix


def test_symbols_constant_and_version():
    lib = N.load()
    assert callable(lib.glint_mat_pull_rows_dot_batch) and callable(lib.glint_mat_pull_rows_dot_batch_dev)
    text = (Path(__file__).resolve().parent.parent / "include" / "glint_gpu.h").read_text()
    assert f"#define GLINT_DOT_BATCH_ROWS {N.GLINT_DOT_BATCH_ROWS}\n" in text
    assert N.GLINT_DOT_BATCH_ROWS == 128 and N.GLINT_K_COUNT == 13
    assert lib.glint_version() > 2000  # glint_version() at the parent of the batched row dot pull
    assert callable(glint_amd.PartialMatrix.getRowsDotBatch) and callable(glint_amd.BigMatrix.pullDotBatch)
    rows, x, out = np.zeros(1, np.int64), np.zeros(4), np.zeros(1)  # a NULL shard
    args = (None, rows.ctypes.data, 1, x.ctypes.data, 1, out.ctypes.data)
    assert lib.glint_mat_pull_rows_dot_batch(*args) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_dot_batch_dev(*args, None) == N.GLINT_EINVAL


class FakeShard:
    """Answers getRowsDotBatch from the whole integer-valued table (exact scores) for the rows it owns, and
    counts the calls."""
    def __init__(self, table, owned):
        self.table, self.owned, self.calls, self.np_dtype = table, set(owned.tolist()), 0, table.dtype.type

    def getRowsDotBatch(self, rows, x):
        self.calls += 1
        assert set(rows.tolist()) <= self.owned
        return self.table[rows] @ x.T


@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("parts", [1, 3, 7])
def test_pull_dot_batch_answers_in_the_callers_order(parts, cyclic):
    rng = np.random.default_rng(23)
    table, x = rng.integers(-2, 3, (60, 5)).astype(np.float64), rng.integers(-2, 3, (70, 5)).astype(np.float64)
    partitioner = (CyclicPartitioner if cyclic else RangePartitioner).apply(parts, 60)
    owner = partitioner.partition_indices(np.arange(60, dtype=np.int64))
    shards = [FakeShard(table, np.flatnonzero(owner == p)) for p in range(parts)]
    m = BigMatrix(partitioner, shards, 60, 5)
    rows = rng.permutation(np.concatenate([np.arange(60), rng.integers(0, 60, 30)]))  # shuffled, with repeats
    np.testing.assert_array_equal(m.pullDotBatch(rows, x), table[rows] @ x.T)
    assert [sh.calls for sh in shards] == [1] * parts  # exactly one getRowsDotBatch each
    few = np.flatnonzero(owner == parts - 1)[[2, 0, 2]]  # rows of the last partition only
    np.testing.assert_array_equal(m.pullDotBatch(few, x[4]), table[few] @ x[4])  # x of shape (cols,) answers (n,)
    assert [sh.calls for sh in shards] == [1] * (parts - 1) + [2]  # none for a partition that owns none
