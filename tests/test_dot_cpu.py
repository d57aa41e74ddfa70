"""Row dot-product pull, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay
helper the GPU tests take their expected values from, and BigMatrix.pullDot's bucketing over fake
shards."""
from fractions import Fraction

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix
from dot_cases import NOFMA, NOFMA_PLACES, bits, lane_width, nofma_case, replay_dot, replay_self

# glint_version() at the parent of the row dot pull ("Row dot pull")
PARENT_VERSION = 400


def test_kernel_id_and_version():
    assert N.GLINT_K_PULL_ROWS_DOT == 11
    assert N.GLINT_K_PULL_ROWS_SUM == 10  # not renumbered
    assert N.load().glint_version() > PARENT_VERSION


def test_null_shard_is_einval():
    lib = N.load()
    assert lib.glint_mat_pull_rows_dot(None, None, 0, None, 1, None) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_dot_dev(None, None, 0, None, 1, None, None) == N.GLINT_EINVAL


def test_get_rows_dot_is_public():
    assert callable(glint_amd.PartialMatrix.getRowsDot)
    assert callable(glint_amd.BigMatrix.pullDot)


def test_lane_width():
    assert lane_width(np.float64, 512) == 2 and lane_width(np.float64, 67) == 1
    assert lane_width(np.float32, 300) == 4 and lane_width(np.float32, 7) == 1
    assert lane_width(np.int64, 300) == 2 and lane_width(np.int32, 67) == 1


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_known_answers_are_unfused(npd):
    a, b, fused = NOFMA[npd]
    # the premise, in exact arithmetic: a * a rounds to b, and a fused a * a - b keeps the rest
    assert npd(a) * npd(a) == npd(b)
    assert Fraction(float(a)) ** 2 - Fraction(float(b)) == Fraction(fused)
    for cols, c0, c1 in NOFMA_PLACES[npd]:
        row, x, f = nofma_case(npd, cols, c0, c1)
        got = replay_dot(row[None], x)
        assert got.dtype == npd and got.shape == (1,)
        assert bits(got)[0] == 0 and f > 0  # exactly +0, where a fused chain gives f
        # the two terms do meet in one lane's chain: that is where a fused add would show
        E = lane_width(npd, cols)
        assert (c0 // E) % 64 == (c1 // E) % 64 or cols == 2


def test_replay_order_differs_from_a_plain_sum():
    rng = np.random.default_rng(3)
    for npd in (np.float64, np.float32):
        rows = (rng.standard_normal((50, 300)) * 10.0 ** rng.integers(-4, 5, (50, 300))).astype(npd)
        x = (rng.standard_normal(300) * 10.0 ** rng.integers(-4, 5, 300)).astype(npd)
        got = replay_dot(rows, x)
        prod = rows * x
        plain = np.zeros(50, npd)
        for c in range(300):
            plain = plain + prod[:, c]
        assert (bits(got) != bits(plain)).sum() > 20  # another order shows in most rows
        bound = np.abs(prod).sum(axis=1, dtype=np.float64) * (1e-9 if npd == np.float64 else 1e-4)
        assert (np.abs(got.astype(np.float64) - plain) <= bound).all()  # yet both are sums of the same products
        # (q, cols) is the (cols,) answer per query; the self-dot is the row against itself
        x3 = np.stack([x, x[::-1], -x])
        both = replay_dot(rows, x3)
        assert both.shape == (50, 3)
        for j in range(3):
            np.testing.assert_array_equal(bits(both[:, j]), bits(replay_dot(rows, x3[j])))
        np.testing.assert_array_equal(bits(replay_self(rows[:1])), bits(replay_dot(rows[:1], rows[0])))


def test_replay_wraps_and_starts_from_plus_zero():
    assert replay_dot(np.array([[2**31 - 1, 2]], np.int32), np.array([2, 1], np.int32)).tolist() == [0]
    assert replay_dot(np.array([[2**62, 1]], np.int64), np.array([4, -3], np.int64)).tolist() == [-3]
    z = replay_dot(np.array([[-0.0, 0.0, -0.0]]), np.array([1.0, 1.0, 1.0]))
    assert bits(z)[0] == 0  # +0 + -0 = +0 in every lane
    assert np.isnan(replay_dot(np.array([[np.inf, 1.0]]), np.array([0.0, 1.0])))[0]


class FakeShard:
    """Answers getRowsDot from its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, []
        self.np_dtype = table.dtype.type

    def getRowsDot(self, rows, x=None):
        rows = np.array(rows)
        self.calls.append((rows, None if x is None else np.array(x)))
        local = rows - self.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        return replay_self(self.table[local]) if x is None else replay_dot(self.table[local], x)


def _model(table):
    """3 range partitions of 100 rows over the table."""
    partitioner = RangePartitioner.apply(3, 300)
    shards = [FakeShard(table[p.start:p.end], p.start) for p in partitioner.all()]
    assert [sh.table.shape[0] for sh in shards] == [100, 100, 100]
    return partitioner, shards, BigMatrix(partitioner, shards, 300, table.shape[1])


def _table():
    rng = np.random.default_rng(41)
    return (rng.standard_normal((300, 7)) * 10.0 ** rng.integers(-4, 5, (300, 7))).astype(np.float64)


def test_pull_dot_buckets_and_scatters_back():
    table = _table()
    partitioner, shards, m = _model(table)
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 300, 200).astype(np.int64)  # every partition hit, interleaved, with repeats
    rows[10:13] = rows[10]
    assert np.unique(rows).size < rows.size
    owner = partitioner.partition_indices(rows)
    assert set(owner.tolist()) == {0, 1, 2} and (np.diff(owner) != 0).sum() > 50
    x1 = rng.standard_normal(7)
    x3 = rng.standard_normal((3, 7))
    for x, exp in ((x1, replay_dot(table[rows], x1)), (x3, replay_dot(table[rows], x3)),
                   (None, replay_self(table[rows])), (x1[None], replay_dot(table[rows], x1[None]))):
        for sh in shards:
            sh.calls.clear()
        got = m.pullDot(rows, x)
        assert got.dtype == np.float64 and got.shape == exp.shape
        np.testing.assert_array_equal(bits(got), bits(exp))
        for p, sh in enumerate(shards):
            assert len(sh.calls) == 1  # one call per partition
            r, sx = sh.calls[0]
            np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
            assert (sx is None) if x is None else np.array_equal(sx, x)  # the same x for every shard
    assert m.pullDot(rows, x1).shape == (200,) and m.pullDot(rows, x1[None]).shape == (200, 1)


def test_pull_dot_skips_partitions_without_rows_and_empty_requests():
    table = _table()
    _, shards, m = _model(table)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    x = np.arange(7, dtype=np.float64)
    np.testing.assert_array_equal(bits(m.pullDot(rows, x)), bits(replay_dot(table[rows], x)))
    assert len(shards[0].calls) == 1 and not shards[1].calls and len(shards[2].calls) == 1
    for sh in shards:
        sh.calls.clear()
    none = np.zeros(0, np.int64)
    assert m.pullDot(none, x).shape == (0,)
    assert m.pullDot(none, np.zeros((4, 7))).shape == (0, 4)
    assert m.pullDot(none).shape == (0,)
    assert all(not sh.calls for sh in shards)


def test_pull_dot_rejects_before_any_shard_is_called():
    _, shards, m = _model(_table())
    with pytest.raises(IndexOutOfBoundsException):
        m.pullDot(np.array([3, 299, 300, 5], np.int64), np.zeros(7))
    with pytest.raises(IndexOutOfBoundsException):
        m.pullDot(np.array([-1], np.int64))
    for bad in (np.zeros(6), np.zeros((2, 8)), np.zeros((0, 7)), np.zeros((1, 2, 7))):
        with pytest.raises(ValueError):
            m.pullDot(np.array([3, 4], np.int64), bad)
    assert all(not sh.calls for sh in shards)
