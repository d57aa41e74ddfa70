"""Whole-row matrix push, the parts that need no GPU: the ABI's argument checks, the constants the
binding mirrors, and BigMatrix.pushRows' bucketing over fake shards."""
import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix
import test_gpu_rows as R  # the case builders only: its tests need a GPU

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


@pytest.mark.parametrize("size", R.SORT_SIZES)
def test_sort_cases_hold_their_conditions(size):
    """What test_gpu_rows.test_row_push_sort_passes relies on, checked on the cases themselves."""
    assert R.sort_passes(size) == R.SORT_PASSES[size]
    assert [R.sort_passes(s) % 2 for s in (255, 256, 65_537)] == [1, 0, 1]  # both buffer pairs
    for dtype, bad in (("long", True), ("double", True), ("double", False)):
        pushes, want = R.sort_case(size, dtype, bad)
        assert [p[0].size for p in pushes] == list(R.SORT_N) and want.shape == (size, R.sort_cols(size))
        for rows, values, low, local in pushes:
            n = rows.size
            inside = (local >= 0) & (local < size)
            assert sorted(local[~inside]) == ([-1, size] if bad else [])
            assert low == (int(np.flatnonzero(~inside)[0]) if bad else None)
            assert set(rows[~inside]) == ({R.START - 1, R.START + size} if bad else set())
            if size < len(R.RUNS):
                assert set(local[inside]) == set(range(size))  # every record on the rows there are
                continue
            # the sorted list as rows_prepare and the stable sort leave it: the sentinel block last
            order = np.argsort(np.where(inside, local, size), kind="stable")
            last_valid = order[inside.sum() - 1]
            assert local[last_valid] == size - 1 and last_valid == n - 1  # ... and the record pushed last
            runs = dict(zip(*np.unique(local[inside], return_counts=True)))
            assert runs[0] in R.RUNS and runs[size - 1] in R.RUNS
            if size >= 1 << 15:  # rows enough: RUNS on distinct rows, every other record alone on its row
                lengths = sorted(runs.values())
                assert lengths[-14:] == sorted(R.RUNS)[1:] and set(lengths[:-14]) == {1}
            else:
                assert sorted(runs.values())[-9:] == sorted(R.RUNS)[6:]  # (the fillers share the other rows)
            if dtype == "double":
                assert R.order_shows(local[inside], values[inside])
                assert sum(c >= 8 for c in runs.values()) >= sum(r >= 8 for r in R.RUNS)


def test_update_rows_is_public():
    assert callable(glint_amd.PartialMatrix.updateRows)
