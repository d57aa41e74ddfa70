"""Grouped row-sum pull, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay
helper the GPU tests take their expected values from, and BigMatrix.pullSum's bucketing and combine
over fake shards."""
import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix
from rowsum_cases import ORDER_VECTORS, bits, replay, replay_groups, replay_pairwise, replay_reversed

# glint_version() at the parent of the row-sum pull ("Row-sum pull")
PARENT_VERSION = 300


def test_kernel_id_and_version():
    assert N.GLINT_K_PULL_ROWS_SUM == 10
    assert N.load().glint_version() > PARENT_VERSION


def test_null_shard_is_einval():
    lib = N.load()
    assert lib.glint_mat_pull_rows_sum(None, None, 0, None, 0, None) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_sum_dev(None, None, 0, None, 0, None, None) == N.GLINT_EINVAL


def test_get_rows_sum_is_public():
    assert callable(glint_amd.PartialMatrix.getRowsSum)
    assert callable(glint_amd.BigMatrix.pullSum)


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_tells_orders_apart(npd):
    v = ORDER_VECTORS[npd]
    assert v.dtype == npd
    assert replay(v) == 1 and replay(v).dtype == npd
    assert replay_reversed(v) == 0
    assert replay_pairwise(v) == 0


def test_replay_starts_from_the_first_term_and_wraps():
    neg_zero = np.array([[-0.0]], np.float64)
    assert bits(replay(neg_zero))[0] == 0x8000000000000000  # not 0 + (-0.0) = +0.0
    assert replay(np.zeros((0, 3), np.int32)).tolist() == [0, 0, 0]
    big = np.array([[2**31 - 1], [1]], np.int32)
    assert replay(big)[0] == -2**31


class FakeShard:
    """Answers getRowsSum from its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, []
        self.np_dtype = table.dtype.type

    def getRowsSum(self, rows, offsets):
        rows, offsets = np.array(rows), np.array(offsets)
        self.calls.append((rows, offsets))
        local = rows - self.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        assert offsets[0] == 0 and offsets[-1] == rows.size and (np.diff(offsets) >= 0).all()
        return replay_groups(self.table, local, offsets)


def _model(table):
    """3 range partitions of 100 rows over the table."""
    partitioner = RangePartitioner.apply(3, 300)
    shards = [FakeShard(table[p.start:p.end], p.start) for p in partitioner.all()]
    assert [sh.table.shape[0] for sh in shards] == [100, 100, 100]
    return partitioner, shards, BigMatrix(partitioner, shards, 300, table.shape[1])


def _int_table():
    rng = np.random.default_rng(41)
    return rng.integers(-2**62, 2**62, (300, 7)).astype(np.int64)  # sums of a few rows wrap


def test_pull_sum_spanning_groups():
    table = _int_table()
    partitioner, shards, m = _model(table)
    rng = np.random.default_rng(6)
    lens = [0, 5, 1, 0, 40, 3, 0, 17, 0]  # empty groups first, in the middle and last
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.integers(0, 300, offsets[-1]).astype(np.int64)  # every partition hit, with repeats
    rows[1:4] = rows[1]  # a row three times in one group
    assert np.unique(rows).size < rows.size
    got = m.pullSum(rows, offsets)
    assert got.dtype == np.int64 and got.shape == (len(lens), 7)
    np.testing.assert_array_equal(got, replay_groups(table, rows, offsets))  # wrapping adds commute
    assert not got[[0, 3, 6, 8]].any()
    owner = partitioner.partition_indices(rows)
    group = np.repeat(np.arange(len(lens)), lens)
    for p, sh in enumerate(shards):
        assert len(sh.calls) == 1  # one call per partition
        r, o = sh.calls[0]
        np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
        assert o.size == len(lens) + 1  # every group kept, the empty ones too
        np.testing.assert_array_equal(np.diff(o), np.bincount(group[owner == p], minlength=len(lens)))


def test_pull_sum_skips_partitions_without_rows():
    table = _int_table()
    _, shards, m = _model(table)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    offsets = np.array([0, 2, 2, 6], np.int64)
    np.testing.assert_array_equal(m.pullSum(rows, offsets), replay_groups(table, rows, offsets))
    assert len(shards[0].calls) == 1 and not shards[1].calls and len(shards[2].calls) == 1
    # no rows at all: zeros, and no shard is asked
    for sh in shards:
        sh.calls.clear()
    got = m.pullSum(np.zeros(0, np.int64), np.zeros(4, np.int64))
    assert got.shape == (3, 7) and not got.any() and all(not sh.calls for sh in shards)
    assert m.pullSum(np.zeros(0, np.int64), np.zeros(1, np.int64)).shape == (0, 7)


def test_pull_sum_rejects_before_any_shard_is_called():
    _, shards, m = _model(_int_table())
    with pytest.raises(IndexOutOfBoundsException):
        m.pullSum(np.array([3, 299, 300, 5], np.int64), np.array([0, 2, 4], np.int64))
    with pytest.raises(IndexOutOfBoundsException):
        m.pullSum(np.array([-1], np.int64), np.array([0, 1], np.int64))
    for bad in ([1, 2], [0, 1], [0, 2, 1, 2], []):  # offsets[0] != 0, offsets[g] != n, decreasing, none
        with pytest.raises(ValueError):
            m.pullSum(np.array([3, 4], np.int64), np.array(bad, np.int64))
    assert all(not sh.calls for sh in shards)


def test_pull_sum_multi_partition_order_is_partition_major():
    """The documented order: per partition the caller's order, then the partials of the partitions that
    hold a row of the group in partition-index order, starting from the first such partial."""
    table = np.zeros((300, 2), np.float64)
    v = ORDER_VECTORS[np.float64]
    rows = np.array([10, 110, 20, 120], np.int64)  # partitions 0, 1, 0, 1
    table[rows, 1] = v
    table[rows, 0] = [-0.0, -0.0, -0.0, -0.0]
    table[250] = [-0.0, 5.0]
    offsets = np.array([0, 4, 5, 5], np.int64)
    rows = np.append(rows, 250)  # a group held by partition 2 alone: its partial as it is, not 0 + it
    _, shards, m = _model(table)
    got = m.pullSum(rows, offsets)
    # exactly that order, replayed: (1e16 + -1e16) + (1 + 1) = 2, where the caller's order gives 1
    p0 = replay(table[[10, 20]])
    p1 = replay(table[[110, 120]])
    exp0 = replay(np.stack([p0, p1]))
    assert exp0[1] == 2 and replay(table[rows[:4]])[1] == 1
    np.testing.assert_array_equal(bits(got[0]), bits(exp0))
    assert bits(got[0])[0] == 0x8000000000000000  # -0.0 + -0.0: no +0 was mixed in
    np.testing.assert_array_equal(bits(got[1]), bits(table[250]))
    assert not got[2].any() and not np.signbit(got[2]).any()
    # one partition: the strict caller order
    single = BigMatrix(RangePartitioner.apply(1, 300), [FakeShard(table, 0)], 300, 2)
    assert single.pullSum(rows[:4], np.array([0, 4], np.int64))[0, 1] == 1


def test_pull_average():
    table = np.arange(600, dtype=np.float32).reshape(300, 2)
    _, _, m = _model(table)
    rows = np.array([1, 150, 299], np.int64)
    got = m.pullAverage(rows, np.array([0, 3, 3], np.int64))
    assert got.dtype == np.float32
    np.testing.assert_array_equal(got, np.stack([table[rows].sum(0) / np.float32(3), np.zeros(2, np.float32)]))
