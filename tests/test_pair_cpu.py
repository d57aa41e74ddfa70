"""Row-pair dot pull and row-pair axpy push, the parts that need no GPU: the ABI's symbols and NULL-shard
checks, the replays the GPU tests take their expected values from, and BigMatrix's bucketing by (own
partition, other partition) over fake shards."""
from fractions import Fraction

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix
from dot_cases import LANES, lane_width
from pair_cases import bits, order_inputs, pair_contrib, replay_pair_axpy, replay_pair_dot


def test_abi():
    lib = N.load()
    for name in ("glint_mat_pull_pairs_dot", "glint_mat_pull_pairs_dot_dev", "glint_mat_push_pairs_axpy",
                 "glint_mat_push_pairs_axpy_dev"):
        assert callable(getattr(lib, name)) and name in N.SIGNATURES
    assert lib.glint_version() > 800
    assert N.GLINT_K_COUNT == 13  # no new kernel id
    assert lib.glint_mat_pull_pairs_dot(None, None, None, None, 0, None) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_pairs_dot_dev(None, None, None, None, 0, None, None) == N.GLINT_EINVAL
    assert lib.glint_mat_push_pairs_axpy(None, None, None, None, None, 0, 0) == N.GLINT_EINVAL
    assert lib.glint_mat_push_pairs_axpy_dev(None, None, None, None, None, 0, 0, None) == N.GLINT_EINVAL


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.getPairsDot) and callable(glint_amd.PartialMatrix.updatePairsAxpy)
    assert callable(glint_amd.BigMatrix.pullPairDot) and callable(glint_amd.BigMatrix.pushPairAxpy)


# ---- the replays are sensitive to what the contract fixes ------------------------------------------------
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


def fused_pair_dot(a, b):
    """replay_pair_dot with every lane step acc = fma(a, b, acc): dot_cases.reduce_products' loop."""
    dt, cols = a.dtype.type, a.shape[1]
    E = lane_width(a.dtype, cols)
    acc = np.zeros((a.shape[0], LANES), dt)
    lane = np.arange(LANES)
    for s in range(0, cols, LANES * E):
        for e in range(E):
            c = s + lane * E + e
            k = int((c < cols).sum())
            acc[:, :k] = fma(a[:, c[:k]], b[:, c[:k]], acc[:, :k], dt)
    for d in (32, 16, 8, 4, 2, 1):
        acc = np.add(acc, acc[:, lane ^ d], dtype=dt)
    return acc[:, 0]


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replays_show_what_the_contract_fixes(npd):
    ld, ls, coef, dst, src = order_inputs(npd)
    assert ld.size == 600 and dst.shape == src.shape == (40, 67) and dst.dtype == npd and coef.dtype == npd
    differ = lambda got, want: float((bits(got) != bits(want)).mean())  # noqa: E731
    # -- pair dot: a fused product
    dots = replay_pair_dot(dst[ld], src[ls])
    assert dots.dtype == npd and dots.shape == (600,)
    dot_fused = differ(fused_pair_dot(dst[ld], src[ls]), dots)
    # -- pair axpy: a fused product, reversed record order, coefficients summed per (dst, src) pair first
    want = replay_pair_axpy(dst, ld, coef, src[ls])
    assert want.dtype == npd
    fused = np.array(dst)
    for i in range(600):
        fused[ld[i]] = fma(np.full(67, coef[i], npd), src[ls[i]], fused[ld[i]], npd)
    rev = replay_pair_axpy(dst, ld, coef, src[ls], order=range(599, -1, -1))
    # one record per distinct (dst, src) pair, in the order of its first occurrence, its coefficients
    # added left to right first
    first, summed = {}, []
    for i in range(600):
        key = (int(ld[i]), int(ls[i]))
        if key in first:
            summed[first[key]][2] = npd(summed[first[key]][2] + coef[i])
        else:
            first[key] = len(summed)
            summed.append([key[0], key[1], coef[i]])
    assert len(summed) < 600  # some pair repeats: the variant is a different sum
    pre = replay_pair_axpy(dst, np.array([s[0] for s in summed]), np.array([s[2] for s in summed], npd),
                           src[np.array([s[1] for s in summed])])
    touched = np.unique(ld)
    shares = {"dot fused": dot_fused, "axpy fused": differ(fused[touched], want[touched]),
              "axpy reversed": differ(rev[touched], want[touched]),
              "axpy coefficients summed first": differ(pre[touched], want[touched])}
    print(np.dtype(npd).name, {k: round(v, 3) for k, v in shares.items()})
    # each must change bits. (With 67 columns only lanes 0 .. 2 hold a second product, and a lane's first
    # step fma(a, b, +0) is the rounded product: the fused dot differs in few answers, but it differs.)
    assert all(v > 0 for v in shares.values()), shares
    assert shares["axpy fused"] > 0.2 and shares["axpy reversed"] > 0.5  # most sums of several terms move
    for a in (dots, want, fused, rev, pre):
        assert np.isfinite(a).all()


def test_replay_known_answers():
    a = np.array([[1, 2, 3], [4, 5, 6]], np.int64)
    b = np.array([[7, 8, 9], [1, 0, -1]], np.int64)
    np.testing.assert_array_equal(replay_pair_dot(a, b), [50, -2])
    big = np.array([[2**62, 2**62]], np.int64)
    np.testing.assert_array_equal(replay_pair_dot(big, np.array([[2, 2]], np.int64)), [0])  # wraps
    t = np.zeros((3, 2), np.float64)
    got = replay_pair_axpy(t, [2, 0, 2], [2.0, -1.0, 0.5], np.array([[1.0, 2.0], [3.0, 4.0], [8.0, 8.0]]))
    np.testing.assert_array_equal(got, [[-3.0, -4.0], [0.0, 0.0], [6.0, 8.0]])
    assert pair_contrib(np.array([3], np.int32), np.array([[2**30, 1]], np.int32)).tolist() == [[-2**30, 3]]


# ---- BigMatrix bucketing over fake shards ----------------------------------------------------------------
class FakeShard:
    """A slice of a numpy table behind PartialMatrix's two pair methods, by the replays; records its calls."""

    def __init__(self, table, part, log, name, device=0):
        self.table, self.part, self.log, self.name, self.device = table, part, log, name, device
        self.np_dtype = table.dtype.type

    def local(self, rows):
        loc = np.array([self.part.globalToLocal(int(r)) for r in rows], np.int64)
        assert ((loc >= 0) & (loc < self.table.shape[0])).all()
        return loc

    def getPairsDot(self, other, rows, other_rows, out=None, sync=True):
        self.log.append(("dot", self.name, other.name, np.array(rows), np.array(other_rows), None))
        return replay_pair_dot(self.table[self.local(rows)], other.table[other.local(other_rows)])

    def updatePairsAxpy(self, src, rows, src_rows, coef, deterministic=False, sync=True, unordered=False):
        self.log.append(("axpy", self.name, src.name, np.array(rows), np.array(src_rows), np.array(coef)))
        self.table[:] = replay_pair_axpy(self.table, self.local(rows), coef, src.table[src.local(src_rows)])
        return True


def _model(tag, partitioner, nrows, log, cols=7, dtype=np.float64, seed=1, devices=(0,)):
    rng = np.random.default_rng(seed)
    full = rng.standard_normal((nrows, cols)).astype(dtype)
    shards = []
    for i, p in enumerate(partitioner.all()):
        keys = np.array([k for k in range(nrows) if p.contains(k)], np.int64)
        table = np.array(full[keys])
        assert all(p.globalToLocal(int(k)) == j for j, k in enumerate(keys))
        shards.append(FakeShard(table, p, log, (tag, i), devices[i % len(devices)]))
    return full, shards, BigMatrix(partitioner, shards, nrows, cols)


def test_pair_calls_bucket_by_own_and_other_partition():
    log = []
    fa, sa, A = _model("a", RangePartitioner.apply(3, 300), 300, log, seed=1)
    fb, sb, B = _model("b", CyclicPartitioner.apply(2, 211), 211, log, seed=2)  # other rows, other partitioner
    rng = np.random.default_rng(4)
    ra = rng.integers(0, 300, 400).astype(np.int64)
    rb = rng.integers(0, 211, 400).astype(np.int64)
    own, oth = A.partitioner.partition_indices(ra), B.partitioner.partition_indices(rb)
    assert len(set(zip(own.tolist(), oth.tolist()))) == 6
    got = A.pullPairDot(B, ra, rb)
    np.testing.assert_array_equal(bits(got), bits(replay_pair_dot(fa[ra], fb[rb])))
    assert [(c[1], c[2]) for c in log] == [(("a", p), ("b", o)) for p in range(3) for o in range(2)]  # ascending
    for kind, a, b, r, orows, _ in log:
        sel = (own == a[1]) & (oth == b[1])
        assert kind == "dot"
        np.testing.assert_array_equal(r, ra[sel])      # the bucket's pairs only, in the caller's order
        np.testing.assert_array_equal(orows, rb[sel])
    # the push: buckets in ascending (own, source) order, so a destination row's additions run
    # source-partition-major with the caller's order inside a bucket
    log.clear()
    coef = rng.standard_normal(400)
    assert A.pushPairAxpy(B, ra, rb, coef)
    assert [(c[1], c[2]) for c in log] == [(("a", p), ("b", o)) for p in range(3) for o in range(2)]
    order = np.lexsort((np.arange(400), oth, own))
    want = replay_pair_axpy(fa, ra, coef, fb[rb], order=order)
    np.testing.assert_array_equal(bits(np.concatenate([s.table for s in sa])), bits(want))
    for kind, a, b, r, orows, cf in log:
        sel = (own == a[1]) & (oth == b[1])
        assert kind == "axpy"
        np.testing.assert_array_equal(r, ra[sel])
        np.testing.assert_array_equal(orows, rb[sel])
        np.testing.assert_array_equal(cf, coef[sel])
    # the source in one partition: the caller's order
    log.clear()
    fc, sc, Cm = _model("c", RangePartitioner.apply(1, 50), 50, log, seed=3)
    rc = rng.integers(0, 50, 400).astype(np.int64)
    before = np.concatenate([s.table for s in sa])
    A.pushPairAxpy(Cm, ra, rc, coef)
    np.testing.assert_array_equal(bits(np.concatenate([s.table for s in sa])),
                                  bits(replay_pair_axpy(before, ra, coef, fc[rc])))
    # a matrix against itself: the dot is allowed
    log.clear()
    now = np.concatenate([s.table for s in sa])
    got = A.pullPairDot(A, ra, ra[::-1].copy())
    np.testing.assert_array_equal(bits(got), bits(replay_pair_dot(now[ra], now[ra[::-1]])))


def test_pair_calls_skip_empty_buckets_and_empty_calls():
    log = []
    _, _, A = _model("a", RangePartitioner.apply(3, 300), 300, log, seed=1)
    _, _, B = _model("b", RangePartitioner.apply(2, 100), 100, log, seed=2)
    ra = np.array([250, 3, 299, 0], np.int64)   # nothing from own partition 1
    rb = np.array([99, 1, 98, 60], np.int64)    # (2, 1), (0, 0), (2, 1), (0, 1)
    A.pullPairDot(B, ra, rb)
    assert [(c[1][1], c[2][1]) for c in log] == [(0, 0), (0, 1), (2, 1)]
    np.testing.assert_array_equal(log[2][3], [250, 299])
    log.clear()
    assert A.pullPairDot(B, np.zeros(0, np.int64), np.zeros(0, np.int64)).shape == (0,)
    assert A.pushPairAxpy(B, np.zeros(0, np.int64), np.zeros(0, np.int64), np.zeros(0))
    assert not log


def test_pair_calls_reject_before_any_shard_is_called():
    log = []
    _, _, A = _model("a", RangePartitioner.apply(3, 300), 300, log, seed=1)
    _, _, B = _model("b", RangePartitioner.apply(2, 100), 100, log, seed=2)
    ok_a, ok_b = np.array([3, 299], np.int64), np.array([5, 99], np.int64)
    for ra, rb in ((np.array([3, 300], np.int64), ok_b), (ok_a, np.array([5, 100], np.int64)),
                   (np.array([-1, 3], np.int64), ok_b), (ok_a, np.array([5, -1], np.int64))):
        with pytest.raises(IndexOutOfBoundsException):  # either array, validated by its own partitioner
            A.pullPairDot(B, ra, rb)
        with pytest.raises(IndexOutOfBoundsException):
            A.pushPairAxpy(B, ra, rb, np.ones(2))
    with pytest.raises(ValueError):
        A.pullPairDot(B, ok_a, np.array([5], np.int64))  # lengths differ
    with pytest.raises(ValueError):
        A.pushPairAxpy(B, ok_a, ok_b, np.ones(3))
    with pytest.raises(ValueError):
        A.pushPairAxpy(A, ok_a, ok_a, np.ones(2))  # the source shares memory with the destination
    others = [_model("c", RangePartitioner.apply(2, 100), 100, log, cols=8)[2],            # other cols
              _model("d", RangePartitioner.apply(2, 100), 100, log, dtype=np.float32)[2]]  # another dtype
    for other in others:
        with pytest.raises(ValueError):
            A.pullPairDot(other, ok_a, ok_b)
        with pytest.raises(ValueError):
            A.pushPairAxpy(other, ok_a, ok_b, np.ones(2))
    with pytest.raises(ValueError):
        A.pullPairDot(B.shards[0], ok_a, ok_b)  # not a BigMatrix
    assert not log


def test_pair_calls_refuse_a_bucket_across_devices():
    log = []
    _, _, A = _model("a", RangePartitioner.apply(2, 200), 200, log, devices=(0, 1))
    _, _, B = _model("b", RangePartitioner.apply(2, 100), 100, log, seed=2, devices=(0, 1))
    same = (np.array([5, 150, 7], np.int64), np.array([3, 80, 9], np.int64))  # (0, 0) and (1, 1): one device each
    A.pullPairDot(B, *same)
    A.pushPairAxpy(B, *same, np.ones(3))
    assert len(log) == 4
    log.clear()
    cross = (np.array([5, 150, 7], np.int64), np.array([3, 80, 90], np.int64))  # (0, 1): devices 0 and 1
    with pytest.raises(ValueError, match="device 0.*device 1"):
        A.pullPairDot(B, *cross)
    with pytest.raises(ValueError, match="device 0.*device 1"):
        A.pushPairAxpy(B, *cross, np.ones(3))
    assert not log  # not even the buckets in front of the cross-device one
