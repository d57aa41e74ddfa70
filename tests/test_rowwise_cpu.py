"""Row-wise Adagrad row push, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay
the GPU tests take their expected values from (known answers by exact rational arithmetic), the premises
those tests rest on -- asserted from the replay alone, so that a GPU test cannot pass by accident -- and
BigMatrix.pushAdagradRowwise's bucketing over fake shards."""
import ctypes as C

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix, BigVector
from rowwise_cases import (EPS, FUSED_SS_COLS, LR, F, bits, cancel_inputs, fused_ss, fused_update, lane_width,
                           premise_pushes, premise_rows, replay_rowwise, replay_self, round_fraction, round_sqrt, rowwise_terms)

NPD = [np.float64, np.float32]
KINDS = [RangePartitioner.apply, CyclicPartitioner.apply]


def test_abi():
    lib = N.load()
    P, I64, D = C.c_void_p, C.c_int64, C.c_double
    assert lib.glint_mat_push_rows_adagrad_rowwise.argtypes == [P, P, P, P, I64, D, D]
    assert lib.glint_mat_push_rows_adagrad_rowwise_dev.argtypes == [P, P, P, P, I64, D, D, P]
    assert lib.glint_mat_push_rows_adagrad_rowwise(None, None, None, None, 0, 0.1, 0.0) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_adagrad_rowwise_dev(None, None, None, None, 0, 0.1, 0.0, None) == N.GLINT_EINVAL
    assert lib.glint_version() > 1400
    assert N.GLINT_K_COUNT == 13 and N.GLINT_K_PUSH_ROWS == 8  # no new kernel id


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.updateRowsAdagradRowwise)
    assert callable(glint_amd.BigMatrix.pushAdagradRowwise)


# ---- known answers ------------------------------------------------------------------------------------
def _exact_row(npd, w, h, G, lr, eps):
    """(w', h') of one row of cols = 3 by exact rational arithmetic, rounded once per operation. With E = 1
    the three columns sit in lanes 0, 1, 2 with one product each; the butterfly adds lane 2 to lane 0 at
    d = 2 and lane 1 at d = 1 (every other partner is +0, which changes nothing)."""
    R = lambda x: round_fraction(x, npd)  # noqa: E731
    assert len(G) == 3
    prod = [R(F(g) * F(g)) for g in G]
    ss = R(F(R(F(prod[0]) + F(prod[2]))) + F(prod[1]))
    s = R(F(ss) / 3)
    h2 = R(F(h) + F(s))
    r = round_sqrt(F(h2), npd)
    d = R(F(r) + F(npd(eps)))
    k = R(F(npd(lr)) / F(d))
    return np.array([R(F(wi) - F(R(F(k) * F(gi)))) for wi, gi in zip(w, G)], npd), h2


@pytest.mark.parametrize("npd", NPD)
def test_replay_known_answer(npd):
    G = np.array([0.1, -0.7, 1.3], npd)
    w0 = np.array([[9, 9, 9], [0.5, -0.25, 2.0], [7, 7, 7]], npd)
    h0 = np.array([3.0, 0.37, 5.0], npd)
    want_w, want_h = _exact_row(npd, w0[1], h0[1], G, 0.05, 1e-6)
    w, h = replay_rowwise(w0, h0, [1], G[None], 0.05, 1e-6)
    assert w.dtype == npd and h.dtype == npd
    assert bits(w[1]).tolist() == bits(want_w).tolist() and bits(h)[1] == bits(want_h)
    assert abs(float(h[1]) - (0.37 + (0.01 + 0.49 + 1.69) / 3)) < 1e-6  # and it is the step that was meant
    np.testing.assert_allclose(w[1], w0[1] - 0.05 / (np.sqrt(float(h[1])) + 1e-6) * G, rtol=1e-6)
    # two records that add up to the same G give the same step (halves are exact)
    w2, h2 = replay_rowwise(w0, h0, [1, 1], np.stack([G / 2, G / 2]), 0.05, 1e-6)
    np.testing.assert_array_equal(bits(w2), bits(w))
    np.testing.assert_array_equal(bits(h2), bits(h))
    # unnamed rows are copied
    np.testing.assert_array_equal(bits(w[[0, 2]]), bits(w0[[0, 2]]))
    np.testing.assert_array_equal(bits(h[[0, 2]]), bits(h0[[0, 2]]))


@pytest.mark.parametrize("npd", NPD)
def test_replay_ieee_cases(npd):
    """The header's coupled-row cases, from the replay."""
    big = npd(1e200 if npd == np.float64 else 1e30)
    w0, h0 = np.full((5, 4), 1.5, npd), np.array([1, 1, 0, 1, 1], npd)
    g = np.zeros((5, 4), npd)
    g[0, 2] = np.nan   # one NaN column: the whole row and h'
    g[1] = big         # G * G overflows: h' inf, k 0, p = 0 * G = 0
    g[3] = big
    g[3, 1] = np.inf   # ... and NaN where G is infinite (here ss is inf already, so k = 0 for the row)
    w, h = replay_rowwise(w0, h0, np.arange(4), g[:4], 0.5, 0.0)  # row 2: G = 0, h = 0, eps = 0
    assert np.isnan(w[0]).all() and np.isnan(h[0])
    assert np.isinf(h[1]) and (bits(w[1]) == bits(w0[1])).all()
    assert np.isnan(w[2]).all() and h[2] == 0
    assert np.isinf(h[3]) and np.isnan(w[3, 1]) and (bits(w[3, [0, 2, 3]]) == bits(w0[3, [0, 2, 3]])).all()
    assert (bits(w[4]) == bits(w0[4])).all() and h[4] == 1


# ---- premises of the GPU tests ------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [67, 256])
@pytest.mark.parametrize("npd", NPD)
def test_premise_order_of_ss(npd, cols):
    name = np.dtype(npd).name
    G = premise_rows(name, cols, "order")
    ss = replay_self(G)
    ltr = np.zeros(16, npd)
    for c in range(cols):  # left to right over the columns
        ltr = np.add(ltr, np.multiply(G[:, c], G[:, c], dtype=npd), dtype=npd)
    print(f"{name} cols {cols}: contract vs left-to-right differ in {(bits(ss) != bits(ltr)).sum()} of 16 rows")
    assert (bits(ss) != bits(ltr)).any()
    zero = np.zeros(16, npd)  # and it reaches the state: h' = 0 + ss / C differs too
    h2 = rowwise_terms(np.zeros_like(G), zero, G, LR, EPS)["h2"]
    assert (bits(rowwise_terms(np.zeros_like(G), zero, G, LR, EPS, ss=ltr)["h2"]) != bits(h2)).any()
    E = lane_width(npd, cols)
    assert (E > 1) == (cols == 256)
    if E > 1:
        one = replay_self(G, E=1)
        print(f"  contract (E = {E}) vs E = 1 differ in {(bits(ss) != bits(one)).sum()} of 16 rows")
        assert (bits(ss) != bits(one)).any()
        assert (bits(rowwise_terms(np.zeros_like(G), zero, G, LR, EPS, ss=one)["h2"]) != bits(h2)).any()
    assert np.isfinite(ss).all()


@pytest.mark.parametrize("cols", [3, 67])
@pytest.mark.parametrize("npd", NPD)
def test_premise_divide_not_reciprocal(npd, cols):
    name = np.dtype(npd).name
    G = premise_rows(name, cols, "divide")
    h0 = np.abs(premise_rows(name, cols, "divide-h")[:, 0])
    t = rowwise_terms(np.zeros_like(G), h0, G, LR, EPS)
    C_ = npd(cols)
    recip = np.multiply(t["ss"], np.divide(npd(1), C_, dtype=npd), dtype=npd)
    assert (bits(recip) != bits(t["s"])).any(), "ss * (1 / C) never differs from ss / C"
    # the Adagrad form (lr * G) / d rounds differently from (lr / d) * G
    other = np.divide(np.multiply(npd(LR), G, dtype=npd), t["d"][:, None], dtype=npd)
    frac = (bits(other) != bits(t["p"])).mean()
    print(f"{name} cols {cols}: reciprocal differs in {(bits(recip) != bits(t['s'])).sum()} of 16 rows; "
          f"(lr * G) / d differs on {frac:.3f} of the elements")
    assert frac > 0.02


@pytest.mark.parametrize("npd", NPD)
def test_premise_fused_update_shows(npd):
    name = np.dtype(npd).name
    G, h0, w0 = cancel_inputs(name)
    assert [p[0] for p in premise_pushes(name)] == ["order/67", "order/256", "divide/3", "divide/67", "cancel",
                                                    "fused-ss"]  # what test_gpu_rowwise.py pushes
    t = rowwise_terms(w0, h0, G, LR, EPS)
    fused = np.stack([fused_update(w0[i], t["k"][i], G[i]) for i in range(G.shape[0])])
    frac = (bits(fused) != bits(t["w2"])).mean()
    print(f"{name}: fma(-k, G, w) differs from w - k * G on {frac:.3f} of {G.size} elements")
    assert frac > 0.5
    assert (np.abs(t["w2"]) < np.abs(w0) * 2.0 ** -9).all()  # the update cancels


@pytest.mark.parametrize("npd", NPD)
def test_premise_fused_ss_shows(npd):
    name = np.dtype(npd).name
    cols = FUSED_SS_COLS[name]
    # one strip of the 16-B layout: a lane's chain has 4 (float) or 2 (double) products, and every one
    # after the first can show a fused add
    assert cols == 64 * lane_width(npd, cols) and lane_width(npd, cols) >= 2
    G = premise_rows(name, cols, "fused")
    ss = replay_self(G)
    differ = sum(int(bits(fused_ss(G[i]))[0] != bits(ss)[i]) for i in range(16))
    print(f"{name} cols {cols}: a fused lane chain changes ss in {differ} of 16 rows")
    assert differ >= 1
    fs = np.array([fused_ss(G[i]) for i in range(16)], npd)
    zero = np.zeros(16, npd)  # and it reaches the state
    assert (bits(rowwise_terms(np.zeros_like(G), zero, G, LR, EPS, ss=fs)["h2"])
            != bits(rowwise_terms(np.zeros_like(G), zero, G, LR, EPS)["h2"])).any()


# ---- BigMatrix.pushAdagradRowwise over fake shards ----------------------------------------------------
class FakeMat:
    """Applies updateRowsAdagradRowwise to its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, part):
        self.table, self.part, self.calls = table, part, []
        self.np_dtype = table.dtype.type

    def updateRowsAdagradRowwise(self, state, rows, grads, lr, eps=1e-10, sync=True):
        rows = np.array(rows)
        self.calls.append((state, rows, np.array(grads), lr, eps))
        local = np.array([self.part.globalToLocal(r) for r in rows], np.int64)
        assert all(self.part.contains(int(r)) for r in rows) and (local < self.table.shape[0]).all()
        self.table[:], state.table[:] = replay_rowwise(self.table, state.table, local, grads, lr, eps)
        return True


class FakeVec:
    def __init__(self, table):
        self.table, self.np_dtype, self.calls = table, table.dtype.type, []


def _model(make, cols=7, dtype=np.float64, nparts=3, nrows=300, seed=1):
    """(partitioner, matrix shards, BigMatrix, vector shards, BigVector) over random tables."""
    partitioner = make(nparts, nrows)
    rng = np.random.default_rng(seed)
    msh = [FakeMat(rng.standard_normal((p.size, cols)).astype(dtype), p) for p in partitioner.all()]
    vsh = [FakeVec(np.abs(rng.standard_normal(p.size)).astype(dtype)) for p in partitioner.all()]
    return partitioner, msh, BigMatrix(partitioner, msh, nrows, cols), vsh, BigVector(make(nparts, nrows), vsh, nrows)


def _whole(partitioner, shards, nrows):
    """The model's table in global row order."""
    first = shards[0].table
    out = np.zeros((nrows,) + first.shape[1:], first.dtype)
    for p, sh in zip(partitioner.all(), shards):
        keys = [k for k in range(nrows) if p.contains(k)]
        out[keys] = sh.table[[p.globalToLocal(k) for k in keys]]
    return out


@pytest.mark.parametrize("make", KINDS, ids=["range", "cyclic"])
def test_push_rowwise_buckets_by_partition(make):
    partitioner, msh, m, vsh, st = _model(make)
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 300, 200).astype(np.int64)  # every partition hit, interleaved, with repeats
    rows[10:13] = rows[10]
    owner = partitioner.partition_indices(rows)
    assert set(owner.tolist()) == {0, 1, 2} and (np.diff(owner) != 0).sum() > 50
    w_want, h_want = _whole(partitioner, msh, 300), _whole(partitioner, vsh, 300)
    for lr, eps, g in ((0.1, 1e-8, rng.standard_normal((200, 7))), (0.01, 0.0, rng.standard_normal(200 * 7))):
        for s in msh:
            s.calls.clear()
        assert m.pushAdagradRowwise(st, rows, g, lr, eps)
        w_want, h_want = replay_rowwise(w_want, h_want, rows, g, lr, eps)
        for p, s in enumerate(msh):
            assert len(s.calls) == 1  # one call per partition, on the weights shard
            state, r, sg, slr, seps = s.calls[0]
            assert state is vsh[p] and (slr, seps) == (lr, eps)  # with that partition's state shard
            np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
            np.testing.assert_array_equal(sg, g.reshape(200, 7)[owner == p])  # with their gradient rows
        np.testing.assert_array_equal(bits(_whole(partitioner, msh, 300)), bits(w_want))
        np.testing.assert_array_equal(bits(_whole(partitioner, vsh, 300)), bits(h_want))


def test_push_rowwise_skips_partitions_without_rows_and_empty_pushes():
    _, msh, m, vsh, st = _model(RangePartitioner.apply)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    m.pushAdagradRowwise(st, rows, np.ones((6, 7)), 0.1)
    assert len(msh[0].calls) == 1 and not msh[1].calls and len(msh[2].calls) == 1
    assert msh[0].calls[0][4] == 1e-10  # the default eps
    for s in msh:
        s.calls.clear()
    assert m.pushAdagradRowwise(st, np.zeros(0, np.int64), np.zeros((0, 7)), 0.1)
    assert all(not s.calls for s in msh)


@pytest.mark.parametrize("make", KINDS, ids=["range", "cyclic"])
def test_push_rowwise_rejects_before_any_shard_is_called(make):
    _, msh, m, vsh, st = _model(make)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAdagradRowwise(st, np.array([3, 299, 300, 5], np.int64), np.zeros((4, 7)), 0.1)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAdagradRowwise(st, np.array([-1], np.int64), np.zeros((1, 7)), 0.1)
    two = np.array([3, 4], np.int64)
    for g in (np.zeros((2, 6)), np.zeros((3, 7)), np.zeros(13)):
        with pytest.raises(ValueError):
            m.pushAdagradRowwise(st, two, g, 0.1)
    other_kind = KINDS[1 - KINDS.index(make)]
    others = [_model(other_kind)[4],                 # another partitioner
              _model(make, nparts=2)[4],             # other partitions
              _model(make, nrows=301)[4],            # a wrong size
              _model(make, dtype=np.float32)[4],     # a wrong dtype
              _model(make)[2]]                       # a BigMatrix
    for other in others:
        with pytest.raises(ValueError):
            m.pushAdagradRowwise(other, two, np.zeros((2, 7)), 0.1)
    with pytest.raises(ValueError):
        m.pushAdagradRowwise(vsh[0], two, np.zeros((2, 7)), 0.1)  # a shard, not a BigVector
    assert all(not s.calls for s in msh)
