"""Sparse row pull, the parts that need no GPU: the ABI's argument checks, the constants the binding
mirrors, and BigMatrix.pullSparse's bucketing and merge over fake shards."""
import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix

# glint_version() at the parent of the sparse row pull ("Sparse row pull")
PARENT_VERSION = 200


def to_csr(dense):
    """CSR of a dense (n, cols) array with the `!= 0` mask, row-major."""
    mask = dense != 0
    indptr = np.zeros(dense.shape[0] + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(mask)[1].astype(np.int32), dense[mask]


def test_null_shard_is_einval():
    lib = N.load()
    assert lib.glint_mat_pull_rows_sparse(None, None, 0, None, None, None, 0, None) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_sparse_dev(None, None, 0, None, None, None, 0, None) == N.GLINT_EINVAL


def test_kernel_id_and_version():
    assert N.GLINT_K_PULL_ROWS_SPARSE == 9
    assert N.load().glint_version() > PARENT_VERSION


def test_get_rows_sparse_is_public():
    assert callable(glint_amd.PartialMatrix.getRowsSparse)
    assert callable(glint_amd.BigMatrix.pullSparse)


class FakeShard:
    """Answers getRowsSparse from its slice of a numpy table and records the calls."""
    np_dtype = np.int64

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, []

    def getRowsSparse(self, rows):
        rows = np.array(rows)
        self.calls.append(rows)
        local = rows - self.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        return to_csr(self.table[local])


def _model():
    """3 range partitions of 100 rows, 7 columns, about a third of the elements non-zero and a few rows empty."""
    rng = np.random.default_rng(31)
    table = rng.integers(-5, 6, (300, 7)).astype(np.int64) * (rng.random((300, 7)) < 0.35)
    table[[0, 17, 150, 299]] = 0
    partitioner = RangePartitioner.apply(3, 300)
    shards = [FakeShard(table[p.start:p.end], p.start) for p in partitioner.all()]
    assert [sh.table.shape[0] for sh in shards] == [100, 100, 100]
    return table, partitioner, shards, BigMatrix(partitioner, shards, 300, 7)


def test_pull_sparse_merges_in_caller_order():
    table, partitioner, shards, m = _model()
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 300, 400).astype(np.int64)  # with repeats, every partition hit
    assert np.unique(rows).size < rows.size
    indptr, cols, vals = m.pullSparse(rows)
    e_ptr, e_cols, e_vals = to_csr(table[rows])
    assert indptr.dtype == np.int64 and cols.dtype == np.int32 and vals.dtype == np.int64
    np.testing.assert_array_equal(indptr, e_ptr)
    np.testing.assert_array_equal(cols, e_cols)
    np.testing.assert_array_equal(vals, e_vals)
    owner = partitioner.partition_indices(rows)
    for p, sh in enumerate(shards):
        assert len(sh.calls) == 1
        np.testing.assert_array_equal(sh.calls[0], rows[owner == p])  # its rows only, in the caller's order


def test_pull_sparse_skips_partitions_without_rows():
    table, _, shards, m = _model()
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1; rows 299 and 0 are empty
    indptr, cols, vals = m.pullSparse(rows)
    e_ptr, e_cols, e_vals = to_csr(table[rows])
    np.testing.assert_array_equal(indptr, e_ptr)
    np.testing.assert_array_equal(cols, e_cols)
    np.testing.assert_array_equal(vals, e_vals)
    assert len(shards[0].calls) == 1 and not shards[1].calls and len(shards[2].calls) == 1
    # no rows at all, and rows that are all empty
    indptr, cols, vals = m.pullSparse(np.zeros(0, np.int64))
    assert indptr.tolist() == [0] and cols.size == 0 and vals.size == 0
    indptr, cols, vals = m.pullSparse(np.array([17, 150, 17], np.int64))
    assert indptr.tolist() == [0, 0, 0, 0] and cols.size == 0 and vals.size == 0


def test_pull_sparse_rejects_before_any_shard_is_called():
    _, _, shards, m = _model()
    with pytest.raises(IndexOutOfBoundsException):
        m.pullSparse(np.array([3, 299, 300, 5], np.int64))
    with pytest.raises(IndexOutOfBoundsException):
        m.pullSparse(np.array([-1], np.int64))
    assert all(not sh.calls for sh in shards)
