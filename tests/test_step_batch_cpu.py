"""Batched optimizer row pushes without a GPU: the ABI's symbols and NULL-shard check, and
BigMatrix.pushAdagradBatch / pushAdamBatch / pushFtrlBatch's state check, bucketing and shape checks over fake
shards."""
import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartitioner, IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix

OPTS = ["Adagrad", "Adam", "Ftrl"]
SCALARS = dict(Adagrad=(0.05, 1e-6), Adam=(0.01, 0.9, 0.999, 1e-8, 3), Ftrl=(0.05, 1.0, 0.3, 1e-4))  # the C calls'
ARGS = dict(Adagrad=(0.05,), Adam=(0.01, 3), Ftrl=(0.05,))  # the methods', the rest defaulted
FACTOR = dict(Adagrad=1, Adam=2, Ftrl=2)


@pytest.mark.parametrize("opt", OPTS)
def test_symbols_and_version(opt):
    lib = N.load()
    assert lib.glint_version() > 2300 and N.GLINT_K_COUNT == 13  # glint_version() at the parent of these pushes
    assert callable(getattr(glint_amd.PartialMatrix, f"updateRows{opt}Batch"))
    rows, coef, x = np.zeros(1, np.int64), np.zeros(1), np.zeros(4)  # a NULL shard
    args = (None, None, rows.ctypes.data, 1, coef.ctypes.data, x.ctypes.data, 1, *SCALARS[opt], 0)
    fn = f"glint_mat_push_rows_{opt.lower()}_batch"
    assert getattr(lib, fn)(*args) == N.GLINT_EINVAL and getattr(lib, fn + "_dev")(*args, None) == N.GLINT_EINVAL


class FakeShard:
    """Records what the batched optimizer pushes hand to it."""
    def __init__(self, cols):
        self.cols, self.np_dtype, self.calls = cols, np.float64, []

    def _record(self, state, rows, coef, x, *scalars):
        self.calls.append((state, rows.copy(), coef.copy(), x, scalars))
        return True

    updateRowsAdagradBatch = updateRowsAdamBatch = updateRowsFtrlBatch = _record


def model(cols, partitioner=None):
    partitioner = partitioner or RangePartitioner.apply(3, 300)
    shards = [FakeShard(cols) for _ in partitioner.all()]
    return shards, BigMatrix(partitioner, shards, 300, cols)


@pytest.mark.parametrize("opt", OPTS)
def test_one_call_per_non_empty_partition_with_its_state_shard(opt):
    shards, m = model(7)
    states, st = model(7 * FACTOR[opt])
    rng = np.random.default_rng(8)
    rows = rng.integers(100, 300, 180)  # nothing from partition 0
    coef, x = rng.standard_normal((180, 70)), rng.standard_normal((70, 7))
    assert getattr(m, f"push{opt}Batch")(st, rows, coef, x, *ARGS[opt])
    assert [len(sh.calls) for sh in shards] == [0, 1, 1] and not any(s.calls for s in states)
    for p in (1, 2):
        state, r, c, xs, scalars = shards[p].calls[0]
        mine = (rows >= 100 * p) & (rows < 100 * (p + 1))
        assert state is states[p] and xs.shape == (70, 7) and scalars[:len(ARGS[opt])] == ARGS[opt]
        np.testing.assert_array_equal(r, rows[mine])  # the caller's order kept
        np.testing.assert_array_equal(c, coef[mine])
        np.testing.assert_array_equal(xs, x)
    assert getattr(m, f"push{opt}Batch")(st, rows[:5], coef[:5, 4], x[4], *ARGS[opt])  # x of shape (cols,): q = 1
    assert getattr(m, f"push{opt}Batch")(st, np.zeros(0, np.int64), np.zeros((0, 4)), np.zeros((4, 7)), *ARGS[opt])
    assert sum(len(sh.calls) for sh in shards) == 2 + len({int(r) // 100 for r in rows[:5]})


@pytest.mark.parametrize("opt", OPTS)
def test_errors_are_raised_before_any_shard_is_called(opt):
    shards, m = model(7)
    _, st = model(7 * FACTOR[opt])
    z, push = np.zeros, getattr(m, f"push{opt}Batch")
    with pytest.raises(IndexOutOfBoundsException):
        push(st, np.array([3, 299, 300, 5], np.int64), z(4), z(7), *ARGS[opt])
    for coef, x in ((z(2), z(6)), (z((2, 2)), z((2, 8))), (z((2, 0)), z((0, 7))), (z(2), z((2, 7))), (z((3, 2)), z((2, 7)))):
        with pytest.raises(ValueError):
            push(st, np.array([3, 4], np.int64), coef, x, *ARGS[opt])
    wrong_cols = model(7 * (3 - FACTOR[opt]))[1]
    wrong_partitioner = model(7 * FACTOR[opt], CyclicPartitioner.apply(3, 300))[1]
    for state in (wrong_cols, wrong_partitioner, shards[0]):
        with pytest.raises(ValueError):
            push(state, np.array([3, 4], np.int64), z((2, 1)), z((1, 7)), *ARGS[opt])
    assert not any(sh.calls for sh in shards)
