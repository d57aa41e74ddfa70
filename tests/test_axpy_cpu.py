"""Row axpy push, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay helper
the GPU tests take their expected values from, and BigMatrix.pushAxpy's bucketing over fake shards."""
from fractions import Fraction

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix
from axpy_cases import NOFMA, bits, fold_rows, nofma_element, nofma_inner, order_inputs, replay_contrib


def test_kernel_id_and_version():
    assert N.GLINT_K_PUSH_ROWS_AXPY == 12
    assert N.GLINT_K_PULL_ROWS_DOT == 11  # not renumbered
    assert N.GLINT_K_COUNT == 13
    assert N.GLINT_AXPY_MAX_VECTORS == 64
    assert N.load().glint_version() > 500


def test_null_shard_is_einval():
    lib = N.load()
    assert lib.glint_mat_push_rows_axpy(None, None, 0, None, None, 1, 0) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_axpy_dev(None, None, 0, None, None, 1, 0, None) == N.GLINT_EINVAL


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.updateRowsAxpy)
    assert callable(glint_amd.BigMatrix.pushAxpy)


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_known_answers_are_unfused(npd):
    a, b, fused = NOFMA[npd]
    assert npd(a) * npd(a) == npd(b)  # the premise: a * a rounds to b, and a fused chain keeps the rest
    assert Fraction(float(a)) ** 2 - Fraction(float(b)) == Fraction(fused)
    # element -b, coef a, x a: exactly +0 where a fused add of the product gives `fused`
    row, coef, x, f = nofma_element(npd, 5, 2)
    got = fold_rows(row[None], [0], replay_contrib(coef, x))
    assert got.dtype == npd and bits(got)[0, 2] == 0 and f > 0
    # coef (1, a), x0 -b, x1 a: a contribution of exactly 0
    coef, x, f = nofma_inner(npd, 5, 3)
    t = replay_contrib(coef, x)
    assert t.dtype == npd and t.shape == (1, 5) and t[0, 3] == 0 and f > 0


def test_replay_wraps():
    t = replay_contrib(np.array([[2**31 - 1, 2]], np.int32), np.array([[2], [1]], np.int32))
    assert t.dtype == np.int32 and t.tolist() == [[0]]  # (2^32 - 2) + 2 wraps to 0
    t = replay_contrib(np.array([[2**62, -3]], np.int64), np.array([[4, 2], [1, 1]], np.int64))
    assert t.dtype == np.int64 and t.tolist() == [[-3, -2**63 - 3 + 2**64]]
    got = fold_rows(np.array([[2**63 - 1]], np.int64), [0], np.array([[1]], np.int64))
    assert got.tolist() == [[-2**63]]


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_q1_coef_one_returns_x_bits(npd):
    x = np.array([-0.0, 0.0, 1.5, -2.0 ** -1060 if npd == np.float64 else -2.0 ** -140, np.inf], npd)
    for xs, cf in ((x, np.ones(2, npd)), (x[None], np.ones((2, 1), npd))):
        t = replay_contrib(cf, xs)
        assert t.shape == (2, 5)
        np.testing.assert_array_equal(bits(t), bits(np.stack([x, x])))  # -0.0 included: no 0 + product


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_order_shows(npd):
    local, coef, x, nrows = order_inputs(npd)
    assert coef.shape == (600, 3) and x.shape == (3, 67) and np.unique(local).size == 40
    zero = np.zeros((nrows, 67), npd)
    want = fold_rows(zero, local, replay_contrib(coef, x))
    differ = lambda other: (bits(other) != bits(want)).mean()  # noqa: E731
    j_reversed = fold_rows(zero, local, replay_contrib(coef[:, ::-1], x[::-1]))
    records_reversed = fold_rows(zero, local, replay_contrib(coef, x), order=range(599, -1, -1))
    summed = np.zeros((nrows, 3), npd)  # the coefficients summed per row first, then one multiply per row
    for i in range(600):
        summed[local[i]] = summed[local[i]] + coef[i]
    coef_first = fold_rows(zero, np.arange(nrows), replay_contrib(summed, x))
    print(f"{np.dtype(npd).name}: j reversed {differ(j_reversed):.3f}, records reversed "
          f"{differ(records_reversed):.3f}, coefficients summed first {differ(coef_first):.3f}")
    assert differ(j_reversed) > 0.05
    assert differ(records_reversed) > 0.5
    assert differ(coef_first) > 0.5
    # yet all are sums of the same products
    mag = fold_rows(np.zeros((nrows, 67)), local, np.abs(coef.astype(np.float64)) @ np.abs(x.astype(np.float64)))
    tol = mag * (1e-9 if npd == np.float64 else 600 * 2.0 ** -22)
    for other in (j_reversed, records_reversed, coef_first):
        assert (np.abs(other.astype(np.float64) - want.astype(np.float64)) <= tol).all()


class FakeShard:
    """Applies updateRowsAxpy to its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, []
        self.np_dtype = table.dtype.type

    def updateRowsAxpy(self, rows, coef, x, deterministic=False):
        rows = np.array(rows)
        self.calls.append((rows, np.array(coef), np.array(x), deterministic))
        local = rows - self.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        self.table[:] = fold_rows(self.table, local, replay_contrib(coef, x))
        return True


def _model(cols=7):
    """3 range partitions of 100 rows over a zero table."""
    partitioner = RangePartitioner.apply(3, 300)
    shards = [FakeShard(np.zeros((p.end - p.start, cols)), p.start) for p in partitioner.all()]
    assert [sh.table.shape[0] for sh in shards] == [100, 100, 100]
    return partitioner, shards, BigMatrix(partitioner, shards, 300, cols)


def test_push_axpy_buckets_by_partition():
    partitioner, shards, m = _model()
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 300, 200).astype(np.int64)  # every partition hit, interleaved, with repeats
    rows[10:13] = rows[10]
    owner = partitioner.partition_indices(rows)
    assert set(owner.tolist()) == {0, 1, 2} and (np.diff(owner) != 0).sum() > 50
    x3, c3 = rng.standard_normal((3, 7)), rng.standard_normal((200, 3))
    x1, c1 = rng.standard_normal(7), rng.standard_normal(200)
    want = np.zeros((300, 7))
    for x, coef, det in ((x3, c3, False), (x1, c1, True), (x1[None], c1[:, None], False)):
        for sh in shards:
            sh.calls.clear()
        assert m.pushAxpy(rows, coef, x, deterministic=det)
        want = fold_rows(want, rows, replay_contrib(coef, x))
        for p, sh in enumerate(shards):
            assert len(sh.calls) == 1  # one call per partition
            r, sc, sx, sdet = sh.calls[0]
            np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
            np.testing.assert_array_equal(sc, coef[owner == p])  # with their coefficient rows
            assert np.array_equal(sx, x) and sx.shape == x.shape and sdet == det  # the same x for every shard
        np.testing.assert_array_equal(bits(np.concatenate([sh.table for sh in shards])), bits(want))


def test_push_axpy_skips_partitions_without_rows_and_empty_pushes():
    _, shards, m = _model()
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    m.pushAxpy(rows, np.arange(12.0).reshape(6, 2), np.ones((2, 7)))
    assert len(shards[0].calls) == 1 and not shards[1].calls and len(shards[2].calls) == 1
    for sh in shards:
        sh.calls.clear()
    none = np.zeros(0, np.int64)
    assert m.pushAxpy(none, np.zeros((0, 4)), np.zeros((4, 7)))
    assert m.pushAxpy(none, np.zeros(0), np.zeros(7))
    assert all(not sh.calls for sh in shards)


def test_push_axpy_rejects_before_any_shard_is_called():
    _, shards, m = _model()
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAxpy(np.array([3, 299, 300, 5], np.int64), np.zeros(4), np.zeros(7))
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAxpy(np.array([-1], np.int64), np.zeros((1, 2)), np.zeros((2, 7)))
    two = np.array([3, 4], np.int64)
    z = np.zeros
    for coef, x in ((z(2), z(6)), (z((2, 2)), z((2, 8))), (z((2, 0)), z((0, 7))), (z((2, 1, 1)), z((1, 1, 7))),
                    (z(2), z((2, 7))), (z((2, 3)), z((2, 7))), (z((3, 2)), z((2, 7))), (z(3), z(7))):
        with pytest.raises(ValueError):
            m.pushAxpy(two, coef, x)
    assert all(not sh.calls for sh in shards)
