"""Grouped row push, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay the GPU
tests take their expected values from, and BigMatrix.pushGroups' bucketing over fake shards."""
from fractions import Fraction

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix
from axpy_cases import fold_rows
from group_cases import bits, group_contrib, group_of, order_inputs, replay_grouped


def test_abi():
    lib = N.load()
    for name in ("glint_mat_push_rows_grouped", "glint_mat_push_rows_grouped_dev"):
        assert callable(getattr(lib, name)) and name in N.SIGNATURES
    assert lib.glint_version() > 1000
    assert N.GLINT_K_COUNT == 13  # no new kernel id
    assert lib.glint_mat_push_rows_grouped(None, None, 0, None, 0, None, None, 0) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_grouped_dev(None, None, 0, None, 0, None, None, 0, None) == N.GLINT_EINVAL


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.updateRowsGrouped) and callable(glint_amd.BigMatrix.pushGroups)


# ---- known answers ---------------------------------------------------------------------------------------
def test_replay_known_answers():
    np.testing.assert_array_equal(group_of([0, 0, 2, 2, 3], 3), [1, 1, 3])
    vals = np.array([[9.0, 9.0], [1.0, 2.0], [7.0, 7.0], [10.0, 20.0]])
    t = np.zeros((3, 2), np.float64)
    # groups: {} {rows 2, 0} {} {row 2}; the empty groups' value rows are never added
    got = replay_grouped(t, [2, 0, 2], [0, 0, 2, 2, 3], vals)
    np.testing.assert_array_equal(got, [[1.0, 2.0], [0.0, 0.0], [11.0, 22.0]])
    got = replay_grouped(t, [2, 0, 2], [0, 0, 2, 2, 3], vals, coef=[2.0, -1.0, 0.5])
    np.testing.assert_array_equal(got, [[-1.0, -2.0], [0.0, 0.0], [7.0, 14.0]])
    # Int wraps, in the product and in the sum
    iv = np.array([[2**30, 1]], np.int32)
    assert group_contrib(iv, [0], np.array([3], np.int32)).tolist() == [[-2**30, 3]]
    it = np.array([[2**31 - 1, 0]], np.int32)
    assert replay_grouped(it, [0, 0], [0, 2], np.array([[1, 5]], np.int32)).tolist() == [[-2**31 + 1, 10]]
    # without coefficients the stored bits pass through: no arithmetic touches them
    z = np.array([[-0.0, np.float64(5e-324)]])
    assert (bits(group_contrib(z, [0, 0])) == bits(np.array([z[0], z[0]]))).all()


# ---- the replay is sensitive to what the contract fixes --------------------------------------------------
def fma(a, b, c, dt):
    """a * b + c rounded once, elementwise. Double: exact rationals, rounded by float(). Float: the product
    of two floats is exact in double and the sum is rounded to double, then to float -- fused up to that
    second rounding, which is enough to show where fusing changes bits."""
    if dt == np.float32:
        return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)
    a, b, c = np.broadcast_arrays(a, b, c)
    out = np.empty(a.shape, np.float64)
    for i in np.ndindex(a.shape):
        out[i] = float(Fraction(float(a[i])) * Fraction(float(b[i])) + Fraction(float(c[i])))
    return out


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_shows_what_the_contract_fixes(npd):
    local, offsets, values, coef, table = order_inputs(npd)
    n, cols = 600, 67
    assert local.size == n and offsets.size == 49 and values.shape == (48, cols) and table.shape == (40, cols)
    assert values.dtype == npd and coef.dtype == npd and table.dtype == npd
    sizes = np.diff(offsets)
    assert sizes[0] == 0 and sizes[-1] == 0 and (sizes[1:-1] == 0).sum() >= 2  # empty: first, middle, last
    group = group_of(offsets, n)
    differ = lambda got, want: float((bits(got) != bits(want)).mean())  # noqa: E731
    rev_order = range(n - 1, -1, -1)
    # -- unweighted: reversed records; each row's contributions summed from +0 first, then added once
    want_u = replay_grouped(table, local, offsets, values)
    rev_u = replay_grouped(table, local, offsets, values, order=rev_order)
    sums = fold_rows(np.zeros_like(table), local, group_contrib(values, group))
    pre_u = np.array(table)
    touched = np.unique(local)
    pre_u[touched] = np.add(table[touched], sums[touched], dtype=npd)
    # -- weighted: a fused product; reversed records; coefficients summed per (row, group) first
    want_w = replay_grouped(table, local, offsets, values, coef)
    fused = np.array(table)
    for i in range(n):
        fused[local[i]] = fma(np.full(cols, coef[i], npd), values[group[i]], fused[local[i]], npd)
    rev_w = replay_grouped(table, local, offsets, values, coef, order=rev_order)
    first, summed = {}, []  # one record per distinct (row, group), in the order of its first occurrence
    for i in range(n):
        key = (int(local[i]), int(group[i]))
        if key in first:
            summed[first[key]][2] = npd(summed[first[key]][2] + coef[i])
        else:
            first[key] = len(summed)
            summed.append([key[0], key[1], coef[i]])
    assert len(summed) < n  # some (row, group) pair repeats: the variant is a different sum
    pre_w = fold_rows(table, np.array([s[0] for s in summed]),
                      group_contrib(values, np.array([s[1] for s in summed]), np.array([s[2] for s in summed], npd)))
    shares = {"unweighted, reversed": differ(rev_u[touched], want_u[touched]),
              "unweighted, summed first": differ(pre_u[touched], want_u[touched]),
              "weighted, fused": differ(fused[touched], want_w[touched]),
              "weighted, reversed": differ(rev_w[touched], want_w[touched]),
              "weighted, coefficients summed first": differ(pre_w[touched], want_w[touched])}
    print(np.dtype(npd).name, {k: round(v, 3) for k, v in shares.items()})
    assert all(v > 0 for v in shares.values()), shares
    for a in (want_u, rev_u, pre_u, want_w, fused, rev_w, pre_w):
        assert np.isfinite(a).all()


# ---- BigMatrix.pushGroups over fake shards ---------------------------------------------------------------
class FakeShard:
    """A slice of a numpy table behind PartialMatrix.updateRowsGrouped, by the replay; records its calls."""

    def __init__(self, table, part, log, name):
        self.table, self.part, self.log, self.name = table, part, log, name
        self.np_dtype = table.dtype.type

    def updateRowsGrouped(self, rows, offsets, values, weights=None, deterministic=False, sync=True,
                          unordered=False):
        self.log.append((self.name, np.array(rows), np.array(offsets), np.array(values),
                         None if weights is None else np.array(weights)))
        loc = np.array([self.part.globalToLocal(int(r)) for r in rows], np.int64)
        assert ((loc >= 0) & (loc < self.table.shape[0])).all()
        self.table[:] = replay_grouped(self.table, loc, offsets, np.asarray(values).reshape(-1, self.table.shape[1]),
                                       weights)
        return True


def _model(partitioner, nrows, log, cols=7, dtype=np.float64, seed=1):
    rng = np.random.default_rng(seed)
    full = (rng.standard_normal((nrows, cols)) * 10.0 ** rng.integers(-4, 5, (nrows, cols))).astype(dtype)
    shards, keys_of = [], []
    for i, p in enumerate(partitioner.all()):
        keys = np.array([k for k in range(nrows) if p.contains(k)], np.int64)
        assert all(p.globalToLocal(int(k)) == j for j, k in enumerate(keys))
        shards.append(FakeShard(np.array(full[keys]), p, log, i))
        keys_of.append(keys)
    return full, shards, keys_of, BigMatrix(partitioner, shards, nrows, cols)


def _whole(shards, keys_of, nrows):
    out = np.empty((nrows, shards[0].table.shape[1]), shards[0].table.dtype)
    for s, keys in zip(shards, keys_of):
        out[keys] = s.table
    return out


@pytest.mark.parametrize("make", [RangePartitioner.apply, CyclicPartitioner.apply])
@pytest.mark.parametrize("weighted", [False, True])
def test_push_groups_buckets_by_partition(make, weighted):
    log = []
    nrows, cols, n, g = 300, 7, 400, 60
    full, shards, keys_of, M = _model(make(3, nrows), nrows, log)
    rng = np.random.default_rng(9)
    rows = rng.integers(0, nrows, n).astype(np.int64)
    rows[10:20] = rows[10]  # a row repeated inside a group and across groups
    offsets = np.concatenate(([0, 0], np.sort(rng.integers(0, n + 1, g - 3)), [n, n])).astype(np.int64)
    values = (rng.standard_normal((g, cols)) * 10.0 ** rng.integers(-4, 5, (g, cols)))
    weights = rng.standard_normal(n) if weighted else None
    assert M.pushGroups(rows, offsets, values, weights)
    # the whole table, in the caller's order, bit for bit: a row lives in one partition
    want = replay_grouped(full, rows, offsets, values, weights)
    np.testing.assert_array_equal(bits(_whole(shards, keys_of, nrows)), bits(want))
    own = M.partitioner.partition_indices(rows)
    group = group_of(offsets, n)
    assert [c[0] for c in log] == [0, 1, 2]
    for p, r, sub, vals, w in log:
        sel = own == p
        np.testing.assert_array_equal(r, rows[sel])  # its own records only, in the caller's order
        has = np.unique(group[sel])
        assert has.size < g  # only the groups with a record here are sent ...
        np.testing.assert_array_equal(bits(vals), bits(values[has]))  # ... their value rows compacted
        assert sub.dtype == np.int64 and sub[0] == 0 and sub[-1] == r.size and (np.diff(sub) > 0).all()
        np.testing.assert_array_equal(has[group_of(sub, r.size)], group[sel])  # consistent sub-offsets
        if weighted:
            np.testing.assert_array_equal(w, weights[sel])
        else:
            assert w is None


def test_push_groups_skips_empty_partitions_and_empty_calls():
    log = []
    _, _, _, M = _model(RangePartitioner.apply(3, 300), 300, log)
    rows = np.array([250, 3, 299, 0], np.int64)  # nothing from partition 1
    M.pushGroups(rows, [0, 1, 1, 4], np.ones((3, 7)))
    assert [c[0] for c in log] == [0, 2]
    np.testing.assert_array_equal(log[0][1], [3, 0])
    np.testing.assert_array_equal(log[0][2], [0, 2])       # group 2 only
    np.testing.assert_array_equal(log[1][1], [250, 299])
    np.testing.assert_array_equal(log[1][2], [0, 1, 2])    # groups 0 and 2; the empty group 1 is not sent
    assert log[1][3].shape == (2, 7)
    log.clear()
    assert M.pushGroups(np.zeros(0, np.int64), [0], np.zeros((0, 7)))
    assert M.pushGroups(np.zeros(0, np.int64), [0, 0, 0], np.zeros((2, 7)), np.zeros(0))
    assert not log


def test_push_groups_rejects_before_any_shard_is_called():
    log = []
    _, _, _, M = _model(RangePartitioner.apply(3, 300), 300, log)
    rows, vals = np.array([3, 299, 7], np.int64), np.ones((2, 7))
    for bad in ([0, 2], [1, 2, 3], [0, 3, 2, 3], [0, 1, 4], []):  # offsets: end, start, order, end, none
        with pytest.raises(ValueError):
            M.pushGroups(rows, bad, np.ones((max(len(bad) - 1, 0), 7)))
    for bad_rows in (np.array([3, 300, 7], np.int64), np.array([-1, 3, 7], np.int64)):
        with pytest.raises(IndexOutOfBoundsException):
            M.pushGroups(bad_rows, [0, 1, 3], vals)
    with pytest.raises(ValueError):
        M.pushGroups(rows, [0, 1, 3], np.ones((3, 7)))  # one value row too many
    with pytest.raises(ValueError):
        M.pushGroups(rows, [0, 1, 3], np.ones((2, 8)))  # other cols
    with pytest.raises(ValueError):
        M.pushGroups(rows, [0, 1, 3], vals, np.ones(2))  # weights: one per record
    assert not log
