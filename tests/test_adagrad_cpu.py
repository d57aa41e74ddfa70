"""Adagrad row push, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay the
GPU tests take their expected values from, and BigMatrix.pushAdagrad's bucketing over fake shards."""
import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix
from adagrad_cases import (NOFMA, adagrad_step, bits, order_inputs, replay_adagrad, sum_gradients, sweep_inputs)


def test_abi():
    lib = N.load()
    assert lib.glint_mat_push_rows_adagrad(None, None, None, None, 0, 0.1, 0.0) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_adagrad_dev(None, None, None, None, 0, 0.1, 0.0, None) == N.GLINT_EINVAL
    assert lib.glint_version() > 700
    assert N.GLINT_K_COUNT == 13 and N.GLINT_K_PUSH_ROWS == 8  # no new kernel id


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.updateRowsAdagrad)
    assert callable(glint_amd.BigMatrix.pushAdagrad)


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_known_answer_is_unfused(npd):
    a, b, fused = NOFMA[npd]
    assert npd(a) * npd(a) == npd(b) and fused > 0  # a * a rounds to b; a fused h + a * a keeps `fused`
    w, h = np.zeros((3, 4), npd), np.zeros((3, 4), npd)
    h[1, 2] = -b
    g = np.zeros((1, 4), npd)
    g[0, 2] = a
    w2, h2 = replay_adagrad(w, h, [1], g, 0.5, 1.0)
    assert h2.dtype == npd and w2.dtype == npd
    assert bits(h2)[1, 2] == 0  # exactly +0
    assert w2[1, 2] == -npd(npd(0.5) * a)  # r = 0, d = 1, p = u
    np.testing.assert_array_equal(bits(h2[[0, 2]]), bits(h[[0, 2]]))  # untouched rows are copied
    np.testing.assert_array_equal(bits(w2[[0, 2]]), bits(w[[0, 2]]))


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_sum_starts_from_plus_zero(npd):
    g = np.array([[-0.0, 0.0, -0.0]], npd)
    G = sum_gradients([0], g, np.dtype(npd))[0]
    assert bits(G).tolist() == [0, 0, 0]  # +0 + -0 is +0
    w, h = np.full((1, 3), -0.0, npd), np.zeros((1, 3), npd)
    w2, _ = replay_adagrad(w, h, [0], g, 0.1, 1.0)
    np.testing.assert_array_equal(bits(w2), bits(w))  # -0 - (+0) = -0
    w2, _ = replay_adagrad(w, h, [0], g, -0.1, 1.0)  # u = -0, p = -0: -0 - (-0) = +0
    assert bits(w2).tolist() == [[0, 0, 0]]


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_order_shows(npd):
    local, g, w0, h0, lr, eps = order_inputs(npd)
    assert g.shape == (600, 67) and np.unique(local).size == 40 and g.dtype == npd and w0.dtype == npd
    w, h = replay_adagrad(w0, h0, local, g, lr, eps)
    differ = lambda got, want: (bits(got) != bits(want)).mean()  # noqa: E731
    dt = np.dtype(npd)
    # the records of a row summed in reverse
    wr, hr = np.array(w0), np.array(h0)
    for l, G in sum_gradients(local, g, dt, order=range(599, -1, -1)).items():
        wr[l], hr[l] = adagrad_step(wr[l], hr[l], G, lr, eps)
    # one step per record: a different function
    wp, hp = np.array(w0), np.array(h0)
    for i in range(600):
        l = local[i]
        wp[l], hp[l] = adagrad_step(wp[l], hp[l], np.add(np.zeros(67, npd), g[i], dtype=dt), lr, eps)
    # w - (lr / d) * G: the same h, another rounding of the step
    wq = np.array(w0)
    for l, G in sum_gradients(local, g, dt).items():
        d = np.add(np.sqrt(h[l], dtype=dt), eps, dtype=dt)
        wq[l] = np.subtract(w0[l], np.multiply(np.divide(lr, d, dtype=dt), G, dtype=dt), dtype=dt)
    print(f"{dt.name}: reversed h {differ(hr, h):.3f} w {differ(wr, w):.3f}; per record h {differ(hp, h):.3f} "
          f"w {differ(wp, w):.3f}; lr / d form w {differ(wq, w):.4f}")
    assert differ(hr, h) > 0.5 and differ(wr, w) > 0.02
    assert differ(hp, h) > 0.9 and differ(wp, w) > 0.9
    assert differ(wq, w) > 0.02
    for a in (w, h, wr, hr, wp, hp, wq):
        assert np.isfinite(a).all()


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_sweep_inputs_reach_the_subnormals(npd):
    """What the GPU rounding sweep relies on: subnormal h', subnormal p, inexact quotients and roots."""
    from fractions import Fraction
    h0, G, w0 = sweep_inputs(np.dtype(npd).name, 1500, 128)
    tiny = np.finfo(npd).tiny
    sub = lambda a: ((a != 0) & (np.abs(a) < tiny))  # noqa: E731
    assert sub(h0).sum() > 1000 and (h0 == 0).sum() > 1000 and h0.max() > np.finfo(npd).max / 16
    ge = 60 if npd == np.float64 else 20
    span = np.abs(G[1500 // 4:])
    assert span.min() < 2.0 ** (-ge + 1) and span.max() > 2.0 ** (ge - 1) and (G < 0).any() and (G > 0).any()
    for eps in (0.0, 2.0 ** -30):
        w, h = adagrad_step(w0, h0, G, 0.05, eps)
        with np.errstate(all="ignore"):
            d = np.add(np.sqrt(h, dtype=npd), npd(eps), dtype=npd)
            u = np.multiply(npd(0.05), G, dtype=npd)
            p = np.divide(u, d, dtype=npd)
        assert sub(h).sum() > 1000, "subnormal h'"
        assert sub(p).sum() > 1000, "subnormal p"
        # quotients and roots that are not representable: checked exactly on a sample
        idx = np.flatnonzero(np.isfinite(p) & (p != 0) & np.isfinite(d) & (d != 0))[::997][:200]
        inexact_q = sum(Fraction(float(p.flat[i])) * Fraction(float(d.flat[i])) != Fraction(float(u.flat[i]))
                        for i in idx)
        r = np.sqrt(h, dtype=npd)
        inexact_r = sum(Fraction(float(r.flat[i])) ** 2 != Fraction(float(h.flat[i])) for i in idx)
        assert inexact_q > 100 and inexact_r > 100


class FakeShard:
    """Applies updateRowsAdagrad to its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, []
        self.np_dtype = table.dtype.type

    def updateRowsAdagrad(self, state, rows, grads, lr, eps=1e-10, sync=True):
        rows = np.array(rows)
        self.calls.append((state, rows, np.array(grads), lr, eps))
        local = rows - self.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        self.table[:], state.table[:] = replay_adagrad(self.table, state.table, local, grads, lr, eps)
        return True


def _model(cols=7, dtype=np.float64, partitioner=None, nrows=300, seed=1):
    """3 partitions over random weights or |random| accumulators."""
    partitioner = partitioner or RangePartitioner.apply(3, nrows)
    rng = np.random.default_rng(seed)
    shards = [FakeShard(np.abs(rng.standard_normal((p.size, cols))).astype(dtype), getattr(p, "start", 0))
              for p in partitioner.all()]
    return partitioner, shards, BigMatrix(partitioner, shards, nrows, cols)


def test_push_adagrad_buckets_by_partition():
    partitioner, wsh, m = _model(seed=1)
    _, hsh, st = _model(seed=2)
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 300, 200).astype(np.int64)  # every partition hit, interleaved, with repeats
    rows[10:13] = rows[10]
    owner = partitioner.partition_indices(rows)
    assert set(owner.tolist()) == {0, 1, 2} and (np.diff(owner) != 0).sum() > 50
    w_want = np.concatenate([s.table for s in wsh])
    h_want = np.concatenate([s.table for s in hsh])
    for lr, eps, g in ((0.1, 1e-8, rng.standard_normal((200, 7))), (0.01, 0.0, rng.standard_normal(200 * 7))):
        for s in wsh + hsh:
            s.calls.clear()
        assert m.pushAdagrad(st, rows, g, lr, eps)
        w_want, h_want = replay_adagrad(w_want, h_want, rows, g, lr, eps)
        for p, s in enumerate(wsh):
            assert len(s.calls) == 1 and not hsh[p].calls  # one call per partition, on the weights shard
            state, r, sg, slr, seps = s.calls[0]
            assert state is hsh[p] and (slr, seps) == (lr, eps)  # with that partition's state shard
            np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
            np.testing.assert_array_equal(sg, g.reshape(200, 7)[owner == p])  # with their gradient rows
        np.testing.assert_array_equal(bits(np.concatenate([s.table for s in wsh])), bits(w_want))
        np.testing.assert_array_equal(bits(np.concatenate([s.table for s in hsh])), bits(h_want))


def test_push_adagrad_skips_partitions_without_rows_and_empty_pushes():
    _, wsh, m = _model(seed=1)
    _, hsh, st = _model(seed=2)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    m.pushAdagrad(st, rows, np.ones((6, 7)), 0.1)
    assert len(wsh[0].calls) == 1 and not wsh[1].calls and len(wsh[2].calls) == 1
    assert wsh[0].calls[0][4] == 1e-10  # the default eps
    for s in wsh:
        s.calls.clear()
    assert m.pushAdagrad(st, np.zeros(0, np.int64), np.zeros((0, 7)), 0.1)
    assert all(not s.calls for s in wsh + hsh)


def test_push_adagrad_rejects_before_any_shard_is_called():
    _, wsh, m = _model(seed=1)
    _, hsh, st = _model(seed=2)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAdagrad(st, np.array([3, 299, 300, 5], np.int64), np.zeros((4, 7)), 0.1)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAdagrad(st, np.array([-1], np.int64), np.zeros((1, 7)), 0.1)
    two = np.array([3, 4], np.int64)
    for g in (np.zeros((2, 6)), np.zeros((3, 7)), np.zeros(13)):
        with pytest.raises(ValueError):
            m.pushAdagrad(st, two, g, 0.1)
    others = [_model(partitioner=CyclicPartitioner.apply(3, 300))[2],  # another partitioner
              _model(partitioner=RangePartitioner.apply(2, 300))[2],  # other partitions
              _model(nrows=301)[2], _model(cols=8)[2],               # another shape
              _model(dtype=np.float32)[2]]                            # another dtype
    for other in others:
        with pytest.raises(ValueError):
            m.pushAdagrad(other, two, np.zeros((2, 7)), 0.1)
    with pytest.raises(ValueError):
        m.pushAdagrad(wsh[0], two, np.zeros((2, 7)), 0.1)  # not a BigMatrix
    assert all(not s.calls for s in wsh + hsh)
