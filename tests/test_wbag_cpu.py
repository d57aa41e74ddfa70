"""Weighted row-sum pull and grouped row-dot pull, the parts that need no GPU: the ABI's symbols and
NULL-shard checks, the replay helpers the GPU tests take their expected values from, and
BigMatrix.pullSum(weights=...) / pullGroupDot's validation, bucketing and combine over fake shards."""
from fractions import Fraction

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix
from rowsum_cases import replay, replay_groups, replay_pairwise, replay_reversed
from wbag_cases import (NOFMA_W, ORDER_WEIGHTS, bits, clamped_groups, nofma_wcase, replay_gdot_groups, replay_wgroups,
                        replay_wsum, weighted_terms)

# glint_version() at the parent of the two pulls ("Weighted row-sum pull and grouped row dot")
PARENT_VERSION = 1600


def test_version_and_kernel_ids():
    assert N.load().glint_version() > PARENT_VERSION
    assert N.GLINT_K_COUNT == 13  # no id was added
    assert N.GLINT_K_PULL_ROWS_SUM == 10 and N.GLINT_K_PULL_ROWS_DOT == 11


def test_null_shard_is_einval():
    lib = N.load()
    assert lib.glint_mat_pull_rows_wsum(None, None, 0, None, 0, None, None) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_wsum_dev(None, None, 0, None, 0, None, None, None) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_gdot(None, None, 0, None, 0, None, None) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_gdot_dev(None, None, 0, None, 0, None, None, None) == N.GLINT_EINVAL


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.getRowsGroupDot)
    assert callable(glint_amd.BigMatrix.pullGroupDot)
    import inspect
    p = inspect.signature(glint_amd.PartialMatrix.getRowsSum).parameters
    assert p["weights"].kind is inspect.Parameter.KEYWORD_ONLY and p["weights"].default is None
    assert list(p)[:5] == ["self", "rows", "offsets", "out", "sync"]  # positional calls mean what they meant
    assert inspect.signature(glint_amd.BigMatrix.pullSum).parameters["weights"].default is None


# ---- the replays ---------------------------------------------------------------------------------
@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_weighted_replay_tells_orders_apart(npd):
    w = ORDER_WEIGHTS[npd]
    ones = np.ones((4, 1), npd)
    terms = weighted_terms(ones, w)
    assert terms.dtype == npd
    assert replay_wsum(ones, w)[0] == 1 and replay_wsum(ones, w).dtype == npd
    assert replay_reversed(terms)[0] == 0
    assert replay_pairwise(terms)[0] == 0


def test_weighted_replay_starts_from_the_first_product_and_wraps():
    neg_zero = np.array([[-0.0]], np.float64)
    assert bits(replay_wsum(neg_zero, [1.0]))[0] == 0x8000000000000000  # 1 * -0.0, not 0 + that
    assert bits(replay_wsum(np.array([[0.0]]), [-1.0]))[0] == 0x8000000000000000
    assert replay_wsum(np.zeros((0, 3), np.int32), np.zeros(0, np.int32)).tolist() == [0, 0, 0]
    big = np.array([[2**30], [1]], np.int32)
    assert replay_wsum(big, np.array([2, 5], np.int32))[0] == -2**31 + 5  # the product wraps, then the sum
    table = np.array([[7, 1], [2**31 - 1, 3]], np.int32)
    got = replay_wgroups(table, [1, 0, 1], [0, 0, 3, 3], np.array([1, 1, 1], np.int32))
    assert got.tolist() == [[0, 0], [5, 7], [0, 0]]  # 2 * (2^31 - 1) + 7 = 2^32 + 5


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_weighted_replay_has_no_fused_multiply_add(npd):
    w, r, fused = nofma_wcase(npd)
    assert fused == NOFMA_W[npd][3] and fused > 0
    unfused = replay_wsum(r[:, None], w)
    assert unfused.dtype == npd and unfused[0] == 0 and not np.signbit(unfused[0])
    # the fused value, exactly: the first product is exact, the second is not rounded before the add
    p0 = Fraction(float(w[0])) * Fraction(float(r[0]))
    assert Fraction(float(npd(w[0] * r[0]))) == p0
    assert p0 + Fraction(float(w[1])) * Fraction(float(r[1])) == Fraction(float(fused))
    assert unfused[0] != fused  # the two differ: the case tells a contraction


def test_replay_bad_rows_are_zero_terms():
    table = np.array([[1.0, 2.0], [3.0, 4.0]])
    got = replay_wgroups(table, [0, 99, 1], [0, 3], [2.0, np.inf, 1.0], bad=np.array([False, True, False]))
    assert got.tolist() == [[5.0, 8.0]]  # no inf * 0


@pytest.mark.parametrize("npd,cols", [(np.float64, 300), (np.float32, 67), (np.int32, 7), (np.float64, 1)])
def test_grouped_dot_replay_is_the_row_dot_per_record(npd, cols):
    from dot_cases import fill_values, replay_dot
    table, x = fill_values(npd, cols, 40), fill_values(npd, cols, 5, "x")
    offsets = np.array([0, 0, 9, 10, 10, 30], np.int64)
    local = np.random.default_rng(3).integers(0, 40, 30)
    got = replay_gdot_groups(table, local, offsets, x)
    group = np.repeat(np.arange(5), np.diff(offsets))
    exp = np.array([replay_dot(table[local[i]][None, :], x[group[i]])[0] for i in range(30)], npd)
    np.testing.assert_array_equal(bits(got), bits(exp))


def test_clamped_groups():
    assert clamped_groups([0, 2, 2, 5], 5).tolist() == [0, 0, 2, 2, 2]
    # clamped to [0, 4]: cuts 0, 3, 1, 4, which are not sorted -- the search's own path decides. Record 0:
    # positions 2 and 1 exceed it, 0 does not: group 0. Records 1 to 3: position 2 does not exceed them, 3
    # does: group 2
    assert clamped_groups([-5, 3, 1, 9], 4).tolist() == [0, 2, 2, 2]
    assert clamped_groups([2, 3], 4).tolist() == [-1, -1, 0, -1]  # records no group covers


# ---- the client over fake shards -----------------------------------------------------------------
class FakeShard:
    """Answers getRowsSum / getRowsGroupDot from its slice of a numpy table by the replays, and records the
    calls."""

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, []
        self.np_dtype = table.dtype.type

    def _local(self, rows, offsets):
        local = rows - self.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        assert offsets[0] == 0 and offsets[-1] == rows.size and (np.diff(offsets) >= 0).all()
        return local

    def getRowsSum(self, rows, offsets, *, weights=None):
        rows, offsets = np.array(rows), np.array(offsets)
        self.calls.append(("sum", rows, offsets, None if weights is None else np.array(weights)))
        local = self._local(rows, offsets)
        if weights is None:
            return replay_groups(self.table, local, offsets)
        assert weights.shape == (rows.size,) and weights.dtype == self.table.dtype
        return replay_wgroups(self.table, local, offsets, weights)

    def getRowsGroupDot(self, rows, offsets, x):
        rows, offsets, x = np.array(rows), np.array(offsets), np.array(x)
        self.calls.append(("gdot", rows, offsets, x))
        assert x.shape == (offsets.size - 1, self.table.shape[1]) and x.dtype == self.table.dtype
        assert (np.diff(offsets) > 0).all()  # only the groups with a record here are sent
        return replay_gdot_groups(self.table, self._local(rows, offsets), offsets, x)


class UnweightedShard:
    """A shard whose getRowsSum takes exactly (rows, offsets), as before the weighted pull."""

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, 0
        self.np_dtype = table.dtype.type

    def getRowsSum(self, rows, offsets):
        self.calls += 1
        return replay_groups(self.table, np.array(rows) - self.start, np.array(offsets))


def _model(table, cls=FakeShard):
    """3 range partitions of 100 rows over the table."""
    partitioner = RangePartitioner.apply(3, 300)
    shards = [cls(table[p.start:p.end], p.start) for p in partitioner.all()]
    assert [sh.table.shape[0] for sh in shards] == [100, 100, 100]
    return partitioner, shards, BigMatrix(partitioner, shards, 300, table.shape[1])


def _int_table():
    rng = np.random.default_rng(41)
    return rng.integers(-2**62, 2**62, (300, 7)).astype(np.int64)  # products and sums wrap


def _request(seed, lens):
    rng = np.random.default_rng(seed)
    offsets = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rows = rng.integers(0, 300, offsets[-1]).astype(np.int64)  # every partition hit, with repeats
    rows[1:4] = rows[1]
    weights = rng.integers(-2**62, 2**62, rows.size).astype(np.int64)
    return rows, offsets, weights


def test_pull_sum_weighted_bucketing():
    table = _int_table()
    partitioner, shards, m = _model(table)
    lens = [0, 5, 1, 0, 40, 3, 0, 17, 0]  # empty groups first, in the middle and last
    rows, offsets, weights = _request(6, lens)
    got = m.pullSum(rows, offsets, weights=weights)
    assert got.dtype == np.int64 and got.shape == (len(lens), 7)
    np.testing.assert_array_equal(got, replay_wgroups(table, rows, offsets, weights))  # wrapping adds commute
    assert not got[[0, 3, 6, 8]].any()
    exact = (table[rows[offsets[4]:offsets[5]]].astype(object) *
             weights[offsets[4]:offsets[5], None].astype(object)).sum(axis=0)
    assert any(abs(int(v)) >= 2**63 for v in exact)  # it did wrap
    owner = partitioner.partition_indices(rows)
    group = np.repeat(np.arange(len(lens)), lens)
    for p, sh in enumerate(shards):
        assert len(sh.calls) == 1  # one call per partition
        _, r, o, w = sh.calls[0]
        np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
        np.testing.assert_array_equal(w, weights[owner == p])  # and their weights
        assert o.size == len(lens) + 1  # every group kept, the empty ones too
        np.testing.assert_array_equal(np.diff(o), np.bincount(group[owner == p], minlength=len(lens)))
    assert np.array_equal(m.pullSum(rows, offsets, weights), got)  # weights is the third positional argument


def test_pull_sum_weighted_skips_partitions_without_rows():
    table = _int_table()
    _, shards, m = _model(table)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    offsets = np.array([0, 2, 2, 6], np.int64)
    weights = np.array([3, -1, 2**62, 7, -2**63, 1], np.int64)
    np.testing.assert_array_equal(m.pullSum(rows, offsets, weights=weights),
                                  replay_wgroups(table, rows, offsets, weights))
    assert len(shards[0].calls) == 1 and not shards[1].calls and len(shards[2].calls) == 1
    for sh in shards:
        sh.calls.clear()
    got = m.pullSum(np.zeros(0, np.int64), np.zeros(4, np.int64), weights=np.zeros(0, np.int64))
    assert got.shape == (3, 7) and not got.any() and all(not sh.calls for sh in shards)


def test_pull_sum_weighted_combine_order_is_partition_major():
    table = np.ones((300, 2), np.float64)
    w = ORDER_WEIGHTS[np.float64]
    rows = np.array([10, 110, 20, 120, 250], np.int64)  # partitions 0, 1, 0, 1, 2
    weights = np.append(w, -1.0)
    table[250] = [0.0, 5.0]
    offsets = np.array([0, 4, 5, 5], np.int64)
    _, shards, m = _model(table)
    got = m.pullSum(rows, offsets, weights=weights)
    p0 = replay_wsum(table[[10, 20]], w[[0, 2]])
    p1 = replay_wsum(table[[110, 120]], w[[1, 3]])
    exp0 = replay(np.stack([p0, p1]))
    assert exp0[1] == 2 and replay_wsum(table[rows[:4]], w)[1] == 1  # (1e16 - 1e16) + (1 + 1), not the caller's 1
    np.testing.assert_array_equal(bits(got[0]), bits(exp0))
    np.testing.assert_array_equal(bits(got[1]), bits(np.array([-0.0, -5.0])))  # the partial as it is: -1 * +0 = -0
    assert not got[2].any() and not np.signbit(got[2]).any()
    single = BigMatrix(RangePartitioner.apply(1, 300), [FakeShard(table, 0)], 300, 2)
    assert single.pullSum(rows[:4], np.array([0, 4], np.int64), weights=w)[0, 1] == 1


def test_pull_sum_weighted_rejects_before_any_shard_is_called():
    _, shards, m = _model(_int_table())
    w2, w4 = np.ones(2, np.int64), np.ones(4, np.int64)
    with pytest.raises(IndexOutOfBoundsException):
        m.pullSum(np.array([3, 299, 300, 5], np.int64), np.array([0, 2, 4], np.int64), weights=w4)
    for bad in ([1, 2], [0, 1], [0, 2, 1, 2], []):  # offsets[0] != 0, offsets[g] != n, decreasing, none
        with pytest.raises(ValueError):
            m.pullSum(np.array([3, 4], np.int64), np.array(bad, np.int64), weights=w2)
    for bad in (np.ones(1, np.int64), np.ones(3, np.int64), np.ones(0, np.int64)):  # a wrong length
        with pytest.raises(ValueError):
            m.pullSum(np.array([3, 4], np.int64), np.array([0, 2], np.int64), weights=bad)
    assert all(not sh.calls for sh in shards)


def test_pull_sum_without_weights_calls_the_shard_as_before():
    table = _int_table()
    _, shards, m = _model(table, UnweightedShard)
    rows, offsets, _ = _request(8, [3, 0, 30])
    np.testing.assert_array_equal(m.pullSum(rows, offsets), replay_groups(table, rows, offsets))
    np.testing.assert_array_equal(m.pullSum(rows, offsets, None), replay_groups(table, rows, offsets))
    assert all(sh.calls == 2 for sh in shards)


def test_pull_group_dot():
    table = _int_table()
    partitioner, shards, m = _model(table)
    lens = [0, 5, 1, 0, 40, 3, 0, 17, 0]
    rows, offsets, _ = _request(9, lens)
    rows[offsets[2]] = 150  # the group of one record lives in partition 1 alone
    g = len(lens)
    x = np.random.default_rng(10).integers(-2**62, 2**62, (g, 7)).astype(np.int64)
    got = m.pullGroupDot(rows, offsets, x)
    assert got.dtype == np.int64 and got.shape == (rows.size,)
    np.testing.assert_array_equal(got, replay_gdot_groups(table, rows, offsets, x))  # at the caller's positions
    np.testing.assert_array_equal(m.pullGroupDot(rows, offsets, x.reshape(-1)), got)  # x flat
    owner = partitioner.partition_indices(rows)
    group = np.repeat(np.arange(g), lens)
    for p, sh in enumerate(shards):
        assert len(sh.calls) == 2  # one call per partition and pull
        _, r, o, xs = sh.calls[0]
        np.testing.assert_array_equal(r, rows[owner == p])
        here = np.unique(group[owner == p])  # only its groups, ascending, their vectors compacted
        np.testing.assert_array_equal(xs, x[here])
        np.testing.assert_array_equal(np.diff(o), np.bincount(group[owner == p], minlength=g)[here])
    assert 2 not in np.unique(group[owner == 0]) and shards[0].calls[0][3].shape[0] < g


def test_pull_group_dot_skips_rejects_and_empty():
    table = _int_table()
    _, shards, m = _model(table)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    offsets = np.array([0, 2, 2, 6], np.int64)
    x = np.arange(21, dtype=np.int64).reshape(3, 7)
    np.testing.assert_array_equal(m.pullGroupDot(rows, offsets, x), replay_gdot_groups(table, rows, offsets, x))
    assert len(shards[0].calls) == 1 and not shards[1].calls and len(shards[2].calls) == 1
    for sh in shards:
        sh.calls.clear()
    got = m.pullGroupDot(np.zeros(0, np.int64), np.zeros(4, np.int64), np.zeros((3, 7), np.int64))
    assert got.shape == (0,) and got.dtype == np.int64
    assert m.pullGroupDot(np.zeros(0, np.int64), np.zeros(1, np.int64), np.zeros((0, 7), np.int64)).shape == (0,)
    for bad in (np.zeros((2, 7), np.int64), np.zeros((3, 6), np.int64), np.zeros(20, np.int64),
                np.zeros((7, 3), np.int64)):
        with pytest.raises(ValueError):
            m.pullGroupDot(rows, offsets, bad)
    with pytest.raises(ValueError):
        m.pullGroupDot(rows, np.array([0, 2, 1, 6], np.int64), x)
    with pytest.raises(IndexOutOfBoundsException):
        m.pullGroupDot(np.array([3, 300], np.int64), np.array([0, 2], np.int64), x[:1])
    assert all(not sh.calls for sh in shards)
