"""Whole-row matrix push, the parts that need no GPU: the ABI's argument checks, the constants the
binding mirrors, and BigMatrix.pushRows' bucketing over fake shards."""
import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix

# glint_version() at the parent of the row push ("Row push")
PARENT_VERSION = 100


def test_null_shard_is_einval():
    lib = N.load()
    assert lib.glint_mat_push_rows(None, None, None, 0, 0) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_dev(None, None, None, 0, 0, None) == N.GLINT_EINVAL


def test_kernel_id_and_version():
    assert N.GLINT_K_PUSH_ROWS == 8
    assert N.load().glint_version() > PARENT_VERSION


class FakeShard:
    """Records updateRows calls (what BigMatrix.pushRows hands each partition)."""
    np_dtype = np.int64

    def __init__(self):
        self.calls = []

    def updateRows(self, rows, values, deterministic=False):
        self.calls.append((np.array(rows), np.array(values), deterministic))
        return True


def _model():
    partitioner = RangePartitioner.apply(3, 100)
    shards = [FakeShard() for _ in partitioner.all()]
    return partitioner, shards, BigMatrix(partitioner, shards, 100, 7)


def test_push_rows_buckets_by_partition():
    partitioner, shards, m = _model()
    rng = np.random.default_rng(5)
    rows = rng.integers(0, 100, 400).astype(np.int64)  # with repeats
    assert np.unique(rows).size < rows.size
    values = rng.integers(-1000, 1000, (400, 7)).astype(np.int64)
    assert m.pushRows(rows, values, deterministic=True)
    owner = partitioner.partition_indices(rows)
    for p, sh in enumerate(shards):
        assert len(sh.calls) == 1
        r, v, det = sh.calls[0]
        np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
        np.testing.assert_array_equal(v, values[owner == p])
        assert v.shape == (r.size, 7) and det is True
    assert sum(sh.calls[0][0].size for sh in shards) == 400

    # flat values are the same push; a partition without rows gets no call
    partitioner, shards, m = _model()
    part0 = partitioner.all()[0]
    mine = rows[owner == 0]
    m.pushRows(mine, values[owner == 0].reshape(-1))
    assert part0.contains(int(mine[0])) and len(shards[0].calls) == 1 and not shards[1].calls and not shards[2].calls
    np.testing.assert_array_equal(shards[0].calls[0][1], values[owner == 0])


def test_push_rows_rejects_before_any_shard_is_called():
    _, shards, m = _model()
    rows = np.array([3, 99, 100, 5], np.int64)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushRows(rows, np.ones((4, 7), np.int64))
    assert all(not sh.calls for sh in shards)
    with pytest.raises(ValueError):
        m.pushRows(rows[:2], np.ones(13, np.int64))
    assert all(not sh.calls for sh in shards)


def test_update_rows_is_public():
    assert callable(glint_amd.PartialMatrix.updateRows)
