"""FTRL-proximal row push, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay
the GPU tests take their expected values from (a known answer by exact rational arithmetic, its bits written
out), the premises those tests rest on -- asserted from the replay alone, on the inputs the GPU tests push,
so that a GPU test cannot pass by accident -- and BigMatrix.pushFtrl's bucketing over fake shards."""
import ctypes as C

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix, BigVector
from ftrl_cases import (ALPHA, ALTS, BETA, L1, L2, SIZE, SWEEP_COLS, TH_L1, TH_L2, F, bits, duplicates_push,
                        ftrl_scalars, ftrl_sweep_inputs, ftrl_terms, fusion_inputs, replay_ftrl,
                        replay_ftrl_per_record, round_fraction, round_sqrt, sweep_premises, sweep_scalars,
                        threshold_inputs)

NPD = [np.float64, np.float32]
KINDS = [RangePartitioner.apply, CyclicPartitioner.apply]


def test_abi():
    lib = N.load()
    P, I64, D = C.c_void_p, C.c_int64, C.c_double
    assert lib.glint_mat_push_rows_ftrl.argtypes == [P, P, P, P, I64, D, D, D, D]
    assert lib.glint_mat_push_rows_ftrl_dev.argtypes == [P, P, P, P, I64, D, D, D, D, P]
    assert lib.glint_mat_push_rows_ftrl(None, None, None, None, 0, 0.1, 1.0, 0.0, 0.0) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_ftrl_dev(None, None, None, None, 0, 0.1, 1.0, 0.0, 0.0, None) == N.GLINT_EINVAL
    assert lib.glint_version() >= 1600
    assert N.GLINT_K_COUNT == 13 and N.GLINT_K_PUSH_ROWS == 8  # no new kernel id


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.updateRowsFtrl)
    assert callable(glint_amd.BigMatrix.pushFtrl)


# ---- known answer -------------------------------------------------------------------------------------
def _exact_column(npd, w, z, n, G, alpha, beta, l1, l2):
    """(w', z', n', case) of one column by exact rational arithmetic, rounded once per operation; each
    square root proved by squaring the midpoints to its neighbours (rowwise_cases.round_sqrt)."""
    R = lambda x: round_fraction(x, npd)  # noqa: E731
    alpha, beta, l1, l2 = (npd(x) for x in (alpha, beta, l1, l2))
    q = R(F(G) * F(G))
    n2 = R(F(n) + F(q))
    r0, r1 = round_sqrt(F(n), npd), round_sqrt(F(n2), npd)
    ds = R(F(r1) - F(r0))
    sg = R(F(ds) / F(alpha))
    t = R(F(sg) * F(w))
    u = R(F(G) - F(t))
    z2 = R(F(z) + F(u))
    if abs(F(z2)) <= F(l1):
        return npd(0), z2, n2, "zero"
    s = l1 if z2 > 0 else -l1
    y = R(F(z2) - F(s))
    b = R(F(beta) + F(r1))
    c = R(F(b) / F(alpha))
    d = R(F(c) + F(l2))
    e = R(F(y) / F(d))
    return npd(-e), z2, n2, "positive" if z2 > 0 else "negative"


# (w', z', n') of the row below, by the exact arithmetic above: the bits, as hexadecimal integers
KNOWN = {
    np.float64: [[0x0, 0xbf99dde667fd8954, 0x3faa3e13383b08df],                 # w': +0, negative, positive
                 [0x3fd227a4faf5df98, 0x3ffa608dc274f36d, 0xc00caf2fa33e8ec4],  # z': below l1, past +l1, past -l1
                 [0x3fd851eb851eb852, 0x3ff970a3d70a3d71, 0x400feb851eb851ec]],  # n'
    np.float32: [[0x0, 0xbcceef33, 0x3d51f098],
                 [0x3e913d2a, 0x3fd3046e, 0xc065797c],
                 [0x3ec28f5c, 0x3fcb851f, 0x407f5c28]],
}


@pytest.mark.parametrize("npd", NPD)
def test_replay_known_answer(npd):
    w0 = np.array([[9, 9, 9], [0.1, -0.2, 0.3], [7, 7, 7]], npd)
    z0 = np.array([[3, 3, 3], [0.2, 1.5, -2.0], [5, 5, 5]], npd)
    n0 = np.array([[1, 1, 1], [0.37, 1.1, 2.3], [2, 2, 2]], npd)
    G = np.array([0.1, -0.7, 1.3], npd)
    s0 = np.concatenate([z0, n0], 1)
    exact = [_exact_column(npd, w0[1, c], z0[1, c], n0[1, c], G[c], 0.05, 1.0, 0.5, 0.25) for c in range(3)]
    assert [e[3] for e in exact] == ["zero", "positive", "negative"]  # one column in each case
    want = [np.array([e[i] for e in exact], npd) for i in range(3)]
    print(np.dtype(npd).name, [[hex(int(b)) for b in bits(a)] for a in want])
    assert [[int(b) for b in bits(a)] for a in want] == KNOWN[npd]  # the exact arithmetic is pinned too
    w, s = replay_ftrl(w0, s0, [1], G[None], 0.05, 1.0, 0.5, 0.25)
    assert w.dtype == npd and s.dtype == npd
    assert bits(w[1]).tolist() == bits(want[0]).tolist()
    assert bits(s[1, :3]).tolist() == bits(want[1]).tolist() and bits(s[1, 3:]).tolist() == bits(want[2]).tolist()
    assert bits(w[1, 0]) == 0  # +0, not -0
    # and it is the step that was meant (McMahan et al. 2013, algorithm 1), in double arithmetic
    zd, nd, wd, Gd = (a.astype(np.float64) for a in (z0[1], n0[1], w0[1], G))
    n2 = nd + Gd * Gd
    z2 = zd + Gd - (np.sqrt(n2) - np.sqrt(nd)) / 0.05 * wd
    w2 = np.where(np.abs(z2) <= 0.5, 0.0, -(z2 - np.sign(z2) * 0.5) / ((1.0 + np.sqrt(n2)) / 0.05 + 0.25))
    np.testing.assert_allclose(w[1], w2, rtol=2e-5)
    np.testing.assert_allclose(s[1], np.concatenate([z2, n2]), rtol=2e-5)
    # two records that add up to the same G give the same step (halves are exact)
    w_2, s_2 = replay_ftrl(w0, s0, [1, 1], np.stack([G / 2, G / 2]), 0.05, 1.0, 0.5, 0.25)
    np.testing.assert_array_equal(bits(w_2), bits(w))
    np.testing.assert_array_equal(bits(s_2), bits(s))
    # unnamed rows are copied
    np.testing.assert_array_equal(bits(w[[0, 2]]), bits(w0[[0, 2]]))
    np.testing.assert_array_equal(bits(s[[0, 2]]), bits(s0[[0, 2]]))


@pytest.mark.parametrize("npd", NPD)
def test_replay_ieee_cases(npd):
    """The header's consequences, from the replay."""
    info = np.finfo(npd)
    big = npd(1e200 if npd == np.float64 else 1e30)
    cols = 2
    w0 = np.array([[0.0, 1.5]] * 6, npd)
    s0 = np.concatenate([np.full((6, cols), 2.0, npd), np.ones((6, cols), npd)], 1)
    s0[2, cols:] = info.max  # n at the type's maximum, a small q: n' == n, ds = 0
    s0[3] = 0                # z = 0, n = 0 with G = 0 and beta = l2 = 0
    s0[4, :cols] = [2.0, -2.0]
    s0[4, cols:] = 0         # n' = 0, |z'| > l1, beta = l2 = 0: d = 0, w' infinite
    g = np.zeros((5, cols), npd)
    g[0] = np.nan
    g[1] = big               # G * G overflows: n' inf, sg inf, t = inf * w
    g[2] = 1.0
    w, s = replay_ftrl(w0, s0, np.arange(5), g, 0.5, 0.0, 0.25, 0.0)
    assert np.isnan(w[0]).all() and np.isnan(s[0]).all()  # a NaN z' is not <= l1: it reaches w'
    assert np.isinf(s[1, cols:]).all() and np.isnan(s[1, 0]) and np.isnan(w[1, 0])  # inf * 0
    assert np.isinf(s[1, 1]) and s[1, 1] < 0  # w = 1.5: u = G - inf
    assert (s[2, cols:] == info.max).all() and (s[2, :cols] == 3.0).all() and np.isfinite(w[2]).all()
    assert (bits(w[3]) == 0).all() and (s[3] == 0).all()  # |z'| = 0 <= l1: +0, d = 0 never looked at
    assert np.isinf(w[4]).all() and w[4, 0] < 0 < w[4, 1]
    assert (bits(w[5]) == bits(w0[5])).all() and (bits(s[5]) == bits(s0[5])).all()


# ---- what the bits pin: every form the contract rules out shows on what the GPU tests push --------------
def _differ(got, want):
    """Share of elements of (w', state') whose bits differ."""
    a = np.concatenate([bits(got[0]).ravel(), bits(got[1]).ravel()])
    b = np.concatenate([bits(want[0]).ravel(), bits(want[1]).ravel()])
    return float((a != b).mean())


def _pushes(name):
    """{label: (w0, state0, local, grads, scalars)}: the duplicates push, the fusion push (cols 67) and the
    rounding sweep (l1 = l2 = 0), as test_gpu_ftrl.py pushes them."""
    npd = np.dtype(name).type
    out = {"duplicates": duplicates_push(name) + ((ALPHA, BETA, L1, L2),)}
    G, w, z, n = (a[:7 * 67].reshape(7, 67) for a in fusion_inputs(npd))
    out["fusion"] = (w, np.concatenate([z, n], 1), np.arange(7), G, (ALPHA, BETA, L1, L2))
    w, z, n, G = ftrl_sweep_inputs(name, SIZE, SWEEP_COLS)
    out["sweep"] = (w, np.concatenate([z, n], 1), np.arange(SIZE), G, sweep_scalars(npd, False))
    return out


@pytest.mark.parametrize("alt", ALTS)
@pytest.mark.parametrize("npd", NPD)
def test_premise_alternative_step_shows(npd, alt):
    name = np.dtype(npd).name
    shares = {}
    for label, (w0, s0, local, g, k) in _pushes(name).items():
        if alt.startswith("fma") and label != "fusion":
            continue  # the exact fused forms are computed element by element: on the fusion push only
        shares[label] = _differ(replay_ftrl(w0, s0, local, g, *k, alt=alt), replay_ftrl(w0, s0, local, g, *k))
    print(f"{name}: {alt} differs from the contract on {shares}")
    assert max(shares.values()) > 0, "the form is not told from the contract by any push"


@pytest.mark.parametrize("npd", NPD)
def test_premise_order_and_coalescing_show(npd):
    name = np.dtype(npd).name
    w0, s0, local, g = duplicates_push(name)
    k = (ALPHA, BETA, L1, L2)
    want = replay_ftrl(w0, s0, local, g, *k)
    rev = _differ(replay_ftrl(w0, s0, local, g, *k, order=range(len(local) - 1, -1, -1)), want)
    per = _differ(replay_ftrl_per_record(w0, s0, local, g, *k), want)
    print(f"{name}: gradients summed in reverse differ on {rev:.3f}, one step per record on {per:.3f}")
    assert rev > 0 and per > 0


@pytest.mark.parametrize("npd", NPD)
def test_premise_fusion_inputs_cancel(npd):
    G, w, z, n = fusion_inputs(npd)
    t = ftrl_terms(w, z, n, G, ftrl_scalars(npd, ALPHA, BETA, L1, L2))
    assert (np.abs(t["u"]) < np.abs(G) * 2.0 ** -9).all() and np.isfinite(t["w2"]).all()


# ---- threshold and sweep premises ---------------------------------------------------------------------
@pytest.mark.parametrize("cols", [3, 128])
@pytest.mark.parametrize("npd", NPD)
def test_premise_threshold_sides(npd, cols):
    name = np.dtype(npd).name
    w0, s0, local, g = threshold_inputs(name, SIZE, cols)
    k = ftrl_scalars(npd, ALPHA, BETA, TH_L1, TH_L2)
    w, s = replay_ftrl(w0, s0, local, g, ALPHA, BETA, TH_L1, TH_L2)
    z2 = s[:, :cols]
    a = np.abs(z2)
    below, at, above = int((a < k[2]).sum()), int((a == k[2]).sum()), int((a > k[2]).sum())
    print(f"{name} cols {cols}: |z'| < l1 {below}, == l1 {at}, > l1 {above}; z' < 0 and past l1 "
          f"{int((z2 < -k[2]).sum())}; exact zeros {int((w == 0).sum())}")
    assert below >= 1 and above >= 1 and at >= 2 * cols  # rows 0 and 1 sit on the threshold
    assert (a[:2] == k[2]).all() and (bits(w[:2]) == 0).all()  # ... and are +0
    assert (z2 < -k[2]).any() and (z2 > k[2]).any()
    assert ((w == 0) == (a <= k[2])).all() and (bits(w[w == 0]) == 0).all()
    assert (w[z2 > k[2]] < 0).all() and (w[z2 < -k[2]] > 0).all()
    # with l1 = 0 the same push leaves (nearly) no zero: the zeros above are the threshold's
    assert (replay_ftrl(w0, s0, local, g, ALPHA, BETA, 0.0, 0.0)[0][2:] != 0).all()


@pytest.mark.parametrize("tiny_l1", [False, True])
@pytest.mark.parametrize("npd", NPD)
def test_premise_sweep_counts(npd, tiny_l1):
    name = np.dtype(npd).name
    w0, z0, n0, G = ftrl_sweep_inputs(name, SIZE, SWEEP_COLS)
    k = ftrl_scalars(npd, *sweep_scalars(npd, tiny_l1))
    got = sweep_premises(npd, w0, z0, n0, G, k)
    t = ftrl_terms(w0, z0, n0, G, k)
    print(f"{name} tiny_l1 {tiny_l1}: {got}; zeros {int(t['zero'].sum())} of {G.size}")
    assert min(got.values()) >= 1, got
    if tiny_l1:
        assert 0 < k[2] < 2.0 ** -60 and t["zero"].sum() >= 10 and (~t["zero"]).sum() >= 10


# ---- BigMatrix.pushFtrl over fake shards --------------------------------------------------------------
class FakeMat:
    """Applies updateRowsFtrl to its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, part):
        self.table, self.part, self.calls = table, part, []
        self.np_dtype = table.dtype.type

    def updateRowsFtrl(self, state, rows, grads, alpha, beta=1.0, l1=0.0, l2=0.0, sync=True):
        rows = np.array(rows)
        self.calls.append((state, rows, np.array(grads), alpha, beta, l1, l2))
        local = np.array([self.part.globalToLocal(r) for r in rows], np.int64)
        assert all(self.part.contains(int(r)) for r in rows) and (local < self.table.shape[0]).all()
        self.table[:], state.table[:] = replay_ftrl(self.table, state.table, local, grads, alpha, beta, l1, l2)
        return True


def _model(make, cols=7, scols=14, dtype=np.float64, nparts=3, nrows=300, seed=1):
    """(partitioner, weights shards, weights, state shards, state) over random tables."""
    partitioner = make(nparts, nrows)
    rng = np.random.default_rng(seed)
    wsh = [FakeMat(rng.standard_normal((p.size, cols)).astype(dtype), p) for p in partitioner.all()]
    ssh = [FakeMat(np.abs(rng.standard_normal((p.size, scols))).astype(dtype), p) for p in partitioner.all()]
    return (partitioner, wsh, BigMatrix(partitioner, wsh, nrows, cols), ssh,
            BigMatrix(make(nparts, nrows), ssh, nrows, scols))


def _whole(partitioner, shards, nrows):
    """The model's table in global row order."""
    first = shards[0].table
    out = np.zeros((nrows,) + first.shape[1:], first.dtype)
    for p, sh in zip(partitioner.all(), shards):
        keys = [k for k in range(nrows) if p.contains(k)]
        out[keys] = sh.table[[p.globalToLocal(k) for k in keys]]
    return out


@pytest.mark.parametrize("make", KINDS, ids=["range", "cyclic"])
def test_push_ftrl_buckets_by_partition(make):
    partitioner, wsh, m, ssh, st = _model(make)
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 300, 200).astype(np.int64)  # every partition hit, interleaved, with repeats
    rows[10:13] = rows[10]
    owner = partitioner.partition_indices(rows)
    assert set(owner.tolist()) == {0, 1, 2} and (np.diff(owner) != 0).sum() > 50
    w_want, s_want = _whole(partitioner, wsh, 300), _whole(partitioner, ssh, 300)
    for k, g in (((0.1, 1.0, 0.5, 0.01), rng.standard_normal((200, 7))),
                 ((0.01, 0.0, 0.0, 0.0), rng.standard_normal(200 * 7))):
        for s in wsh:
            s.calls.clear()
        assert m.pushFtrl(st, rows, g, *k)
        w_want, s_want = replay_ftrl(w_want, s_want, rows, g, *k)
        for p, s in enumerate(wsh):
            assert len(s.calls) == 1  # one call per partition, on the weights shard
            assert s.calls[0][0] is ssh[p] and s.calls[0][3:] == k  # with that partition's state shard
            np.testing.assert_array_equal(s.calls[0][1], rows[owner == p])  # its rows only, in the caller's order
            np.testing.assert_array_equal(s.calls[0][2], g.reshape(200, 7)[owner == p])  # with their gradient rows
        np.testing.assert_array_equal(bits(_whole(partitioner, wsh, 300)), bits(w_want))
        np.testing.assert_array_equal(bits(_whole(partitioner, ssh, 300)), bits(s_want))
    assert all(not s.calls for s in ssh)


def test_push_ftrl_skips_partitions_without_rows_and_empty_pushes():
    _, wsh, m, ssh, st = _model(RangePartitioner.apply)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    m.pushFtrl(st, rows, np.ones((6, 7)), 0.1)
    assert len(wsh[0].calls) == 1 and not wsh[1].calls and len(wsh[2].calls) == 1
    assert wsh[0].calls[0][3:] == (0.1, 1.0, 0.0, 0.0)  # the defaults
    for s in wsh:
        s.calls.clear()
    assert m.pushFtrl(st, np.zeros(0, np.int64), np.zeros((0, 7)), 0.1)
    assert all(not s.calls for s in wsh)


@pytest.mark.parametrize("make", KINDS, ids=["range", "cyclic"])
def test_push_ftrl_rejects_before_any_shard_is_called(make):
    _, wsh, m, ssh, st = _model(make)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushFtrl(st, np.array([3, 299, 300, 5], np.int64), np.zeros((4, 7)), 0.1)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushFtrl(st, np.array([-1], np.int64), np.zeros((1, 7)), 0.1)
    two = np.array([3, 4], np.int64)
    for g in (np.zeros((2, 6)), np.zeros((3, 7)), np.zeros(13)):
        with pytest.raises(ValueError):
            m.pushFtrl(st, two, g, 0.1)
    other_kind = KINDS[1 - KINDS.index(make)]
    others = [_model(other_kind)[4],                 # another partitioner
              _model(make, nparts=2)[4],             # other partitions
              _model(make, nrows=301)[4],            # other rows
              _model(make, dtype=np.float32)[4],     # another dtype
              _model(make, scols=7)[4],              # cols, not 2 * cols
              _model(make, scols=15)[4],
              BigVector(make(3, 300), [s for s in ssh], 300)]  # a BigVector
    for other in others:
        with pytest.raises(ValueError):
            m.pushFtrl(other, two, np.zeros((2, 7)), 0.1)
    with pytest.raises(ValueError):
        m.pushFtrl(ssh[0], two, np.zeros((2, 7)), 0.1)  # a shard, not a BigMatrix
    assert all(not s.calls for s in wsh)
