"""Batched row-wise Adagrad row push without a GPU: the ABI's symbols and NULL-shard check, and
BigMatrix.pushAdagradRowwiseBatch's state check, bucketing and shape checks over fake shards."""
import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import CyclicPartitioner, IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix, BigVector
from test_step_batch_cpu import FakeShard as Recorder


def test_symbols_and_version():
    lib = N.load()
    assert lib.glint_version() > 2400 and N.GLINT_K_COUNT == 13  # glint_version() at the parent of this push
    rows, coef, x = np.zeros(1, np.int64), np.zeros(1), np.zeros(4)  # a NULL shard
    args = (None, None, rows.ctypes.data, 1, coef.ctypes.data, x.ctypes.data, 1, 0.05, 1e-6, 0)
    assert lib.glint_mat_push_rows_adagrad_rowwise_batch(*args) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_adagrad_rowwise_batch_dev(*args, None) == N.GLINT_EINVAL


class FakeShard(Recorder):  # records what the batched push hands to it
    updateRowsAdagradRowwiseBatch = Recorder._record


def models(cols, partitioner=None, size=300):
    partitioner = partitioner or RangePartitioner.apply(3, size)
    shards, states = ([FakeShard(c) for _ in partitioner.all()] for c in (cols, 0))
    return shards, BigMatrix(partitioner, shards, size, cols), states, BigVector(partitioner, states, size)


def test_one_call_per_non_empty_partition_with_its_state_shard_and_errors_before_any():
    shards, m, states, st = models(7)
    rng = np.random.default_rng(8)
    rows = rng.integers(100, 300, 180)  # nothing from partition 0
    coef, x = rng.standard_normal((180, 70)), rng.standard_normal((70, 7))
    assert m.pushAdagradRowwiseBatch(st, rows, coef, x, 0.05)
    assert [len(sh.calls) for sh in shards] == [0, 1, 1] and not any(s.calls for s in states)
    for p in (1, 2):
        state, r, c, xs, scalars = shards[p].calls[0]
        mine = (rows >= 100 * p) & (rows < 100 * (p + 1))
        assert state is states[p] and scalars == (0.05, 1e-10)
        np.testing.assert_array_equal(r, rows[mine])  # the caller's order kept
        np.testing.assert_array_equal(c, coef[mine])
        np.testing.assert_array_equal(xs, x)
    assert m.pushAdagradRowwiseBatch(st, rows[:5], coef[:5, 4], x[4], 0.05)  # x of shape (cols,): q = 1
    assert m.pushAdagradRowwiseBatch(st, np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros((4, 7)), 0.05)
    assert sum(len(sh.calls) for sh in shards) == 2 + len({int(r) // 100 for r in rows[:5]})

    shards, m, _, st = models(7)  # then the errors: each is raised before any shard is called
    z, push = np.zeros, m.pushAdagradRowwiseBatch
    with pytest.raises(IndexOutOfBoundsException):
        push(st, np.array([3, 299, 300, 5], np.int64), z(4), z(7), 0.05)
    for coef, x in ((z(2), z(6)), (z((2, 2)), z((2, 8))), (z((2, 0)), z((0, 7))), (z(2), z((2, 7))), (z((3, 2)), z((2, 7)))):
        with pytest.raises(ValueError):
            push(st, np.array([3, 4], np.int64), coef, x, 0.05)
    for state in (models(7)[1], models(7, CyclicPartitioner.apply(3, 300))[3], models(7, size=299)[3], shards[0]):
        with pytest.raises(ValueError):  # a matrix; a vector of another partitioner; of another size; a shard
            push(state, np.array([3, 4], np.int64), z((2, 1)), z((1, 7)), 0.05)
    assert not any(sh.calls for sh in shards)
