"""Adam row push, the parts that need no GPU: the ABI's symbols and NULL-shard checks, the replay the GPU
tests take their expected values from, and BigMatrix.pushAdam's bucketing over fake shards."""
import ctypes as C

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import IndexOutOfBoundsException, CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix
from adam_cases import (BETA1, BETA2, EPS, adam_scalars, adam_step, adam_sweep_inputs, adam_terms, bits, fused_states,
                        fusion_inputs, order_inputs, replay_adam, sum_gradients, sweep_premises)

_D, _I64, _P, _I = C.c_double, C.c_int64, C.c_void_p, C.c_int


def test_abi():
    lib = N.load()
    host, dev = lib.glint_mat_push_rows_adam, lib.glint_mat_push_rows_adam_dev
    assert host.restype is _I and dev.restype is _I
    assert list(host.argtypes) == [_P, _P, _P, _P, _I64, _D, _D, _D, _D, _I64]
    assert list(dev.argtypes) == [_P, _P, _P, _P, _I64, _D, _D, _D, _D, _I64, _P]
    assert host(None, None, None, None, 0, 0.1, 0.9, 0.999, 1e-8, 1) == N.GLINT_EINVAL
    assert dev(None, None, None, None, 0, 0.1, 0.9, 0.999, 1e-8, 1, None) == N.GLINT_EINVAL
    assert lib.glint_version() > 1100
    assert N.GLINT_K_COUNT == 13 and N.GLINT_K_PUSH_ROWS == 8  # no new kernel id


def test_methods_are_public():
    assert callable(glint_amd.PartialMatrix.updateRowsAdam)
    assert callable(glint_amd.BigMatrix.pushAdam)


# beta1 = 0.5, beta2 = 0.75, step = 3: both powers are exact in double (1/8, 27/64), so c1 = 0.875 and c2 =
# 0.578125 whatever the C library's pow does; lr = 0.875 makes alpha exactly 1. The expected bits come from
# exact rational arithmetic, every operation rounded once to nearest even (not from adam_step).
KNOWN = {
    np.float64: dict(rc2=0x3FE854BFB363DC39,
                     w=[0x3FC07000308CE83C, 0xBFF866F5D1A92D02, 0x3FC64EAC6DE4657C, 0x4001FB8A024C4A43],
                     m=[0x3FF4000000000000, 0xBFE4000000000000, 0x3FE8000000000000, 0x3FF8000000000000],
                     v=[0x3FF3000000000000, 0x3FF0000000000000, 0x4008800000000000, 0x4002600000000000]),
    np.float32: dict(rc2=0x3F42A5FE,
                     w=[0x3E038000, 0xBFC337AE, 0x3E327562, 0x400FDC50],
                     m=[0x3FA00000, 0xBF200000, 0x3F400000, 0x3FC00000],
                     v=[0x3F980000, 0x3F800000, 0x40440000, 0x40130000]),
}


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_known_answer(npd):
    k = adam_scalars(npd, 0.875, 0.5, 0.75, 2.0 ** -10, 3)
    assert all(type(x) is npd for x in k)
    b1, b2, a1, a2, alpha, rc2, eps = k
    assert (b1, b2, a1, a2, alpha, eps) == (0.5, 0.75, 0.5, 0.25, 1.0, 2.0 ** -10)
    assert int(bits(np.array([rc2]))[0]) == KNOWN[npd]["rc2"]  # sqrt(0.578125), rounded to double, then to the type
    w = np.array([[1.0, -2.0, 0.5, 3.0]], npd)
    state = np.array([[0.5, -0.25, 1.0, 0.0, 0.25, 1.0, 4.0, 0.0625]], npd)  # m | v
    g = np.array([[2.0, -1.0, 0.5, 3.0]], npd)
    w2, s2 = replay_adam(w, state, [0], g, 0.875, 3, 0.5, 0.75, 2.0 ** -10)
    assert w2.dtype == npd and s2.dtype == npd
    assert [int(x) for x in bits(w2)[0]] == KNOWN[npd]["w"]
    assert [int(x) for x in bits(s2)[0, :4]] == KNOWN[npd]["m"]
    assert [int(x) for x in bits(s2)[0, 4:]] == KNOWN[npd]["v"]
    # two records of the row that add up to g give the same step; rows that are not named are copied
    w3 = np.concatenate([w, w, w])
    s3 = np.concatenate([state, state, state])
    half = np.array([[1.5, -0.25, 0.25, 1.0], [0.5, -0.75, 0.25, 2.0]], npd)
    w4, s4 = replay_adam(w3, s3, [1, 1], half, 0.875, 3, 0.5, 0.75, 2.0 ** -10)
    np.testing.assert_array_equal(bits(w4[1]), bits(w2[0]))
    np.testing.assert_array_equal(bits(s4[1]), bits(s2[0]))
    np.testing.assert_array_equal(bits(w4[[0, 2]]), bits(w3[[0, 2]]))
    np.testing.assert_array_equal(bits(s4[[0, 2]]), bits(s3[[0, 2]]))


def _order_case(npd):
    local, g, w0, h0, lr, _ = order_inputs(npd)
    m0 = np.random.default_rng(15).standard_normal(w0.shape).astype(npd)
    return local, g, w0, np.concatenate([m0, h0], 1), lr


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_order_shows(npd):
    """Coalesce-then-step is not step-per-record, and the order of a row's sum shows."""
    local, g, w0, s0, lr = _order_case(npd)
    dt = np.dtype(npd)
    cols = w0.shape[1]
    k = adam_scalars(npd, lr, BETA1, BETA2, EPS, 2)
    w, s = replay_adam(w0, s0, local, g, lr, 2)
    differ = lambda got, want: (bits(got) != bits(want)).mean()  # noqa: E731
    # the records of a row summed in reverse
    wr, sr = np.array(w0), np.array(s0)
    for l, G in sum_gradients(local, g, dt, order=range(len(local) - 1, -1, -1)).items():
        wr[l], sr[l, :cols], sr[l, cols:] = adam_step(wr[l], sr[l, :cols], sr[l, cols:], G, k)
    # one step per record: a different function
    wp, sp = np.array(w0), np.array(s0)
    for i in range(len(local)):
        l = local[i]
        wp[l], sp[l, :cols], sp[l, cols:] = adam_step(wp[l], sp[l, :cols], sp[l, cols:],
                                                     np.add(np.zeros(cols, npd), g[i], dtype=dt), k)
    print(f"{dt.name}: reversed state {differ(sr, s):.3f} w {differ(wr, w):.3f}; per record state {differ(sp, s):.3f} "
          f"w {differ(wp, w):.3f}")
    assert differ(sp, s) > 0.5 and differ(wp, w) > 0.5  # most elements
    assert differ(sr, s) > 0.25 and differ(wr, w) > 0.02
    for a in (w, s, wr, sr, wp, sp):
        assert np.isfinite(a).all()


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_form_of_the_step_shows(npd):
    """m' * (alpha / d) is not (alpha * m') / d, and sqrt(v' / c2) + eps is not sqrt(v') / rc2 + eps: from
    zero weights, where w' = -p shows every bit of the step."""
    local, g, _, s0, lr = _order_case(npd)
    dt = np.dtype(npd)
    cols = s0.shape[1] // 2
    sums = sum_gradients(local, g, dt)
    G = np.stack([sums[l] for l in sorted(sums)])
    m0, v0 = s0[sorted(sums), :cols], s0[sorted(sums), cols:]
    k = adam_scalars(npd, lr, BETA1, BETA2, EPS, 2)
    t = adam_terms(np.zeros_like(m0), m0, v0, G, k)
    alpha, eps = k[4], k[6]
    c2 = npd(1.0 - BETA2 ** 2)
    p_a = np.multiply(t["m2"], np.divide(alpha, t["d"], dtype=dt), dtype=dt)
    d_b = np.add(np.sqrt(np.divide(t["v2"], c2, dtype=dt), dtype=dt), eps, dtype=dt)
    p_b = np.divide(t["u"], d_b, dtype=dt)
    changed = [float((bits(-p) != bits(t["w2"])).mean()) for p in (p_a, p_b)]
    print(f"{dt.name}: m' * (alpha / d) changes {changed[0]:.3f}, sqrt(v' / c2) changes {changed[1]:.3f}")
    assert min(changed) >= 0.05


@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_replay_fusion_shows(npd):
    """On cancelling operands each of the four possible fused multiply-adds of the moments differs from the
    contract in at least 90 % of the elements."""
    G, m, v = fusion_inputs(npd)
    assert G.shape == m.shape == v.shape == (512,) and G.dtype == npd
    k = adam_scalars(npd, 0.05, BETA1, BETA2, EPS, 1)
    _, m2, v2 = adam_step(np.zeros_like(m), m, v, G, k)
    assert (np.abs(m2) < np.abs(m) * 2.0 ** -8).all() and (np.abs(v2) < np.abs(v) * 2.0 ** -8).all()  # they cancel
    for name, (fm, fv) in fused_states(m, v, G, k).items():
        frac = float(((bits(fm) != bits(m2)) | (bits(fv) != bits(v2))).mean())
        print(f"{np.dtype(npd).name} {name}: {frac:.3f}")
        assert frac >= 0.9, name


@pytest.mark.parametrize("eps", [0.0, 2.0 ** -30])
@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_sweep_inputs_reach_the_subnormals(npd, eps):
    """What the GPU rounding sweep relies on: subnormal v', subnormal p, rounded quotients s and p."""
    m0, v0, G, w0 = adam_sweep_inputs(np.dtype(npd).name, 1500, 128)
    tiny = np.finfo(npd).tiny
    sub = lambda a: ((a != 0) & (np.abs(a) < tiny))  # noqa: E731
    assert sub(v0).sum() > 1000 and (v0 == 0).sum() > 1000 and v0.max() > np.finfo(npd).max / 16
    assert sub(m0).sum() > 1000
    ge = 60 if npd == np.float64 else 20
    span = np.abs(G[1500 // 4:])
    assert span.min() < 2.0 ** (-ge + 1) and span.max() > 2.0 ** (ge - 1) and (G < 0).any() and (G > 0).any()
    got = sweep_premises(npd, m0, v0, G, w0, adam_scalars(npd, 0.05, BETA1, BETA2, eps, 1))
    print(np.dtype(npd).name, eps, got)
    assert min(got.values()) > 1000, got


class FakeShard:
    """Applies updateRowsAdam to its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, start):
        self.table, self.start, self.calls = table, start, []
        self.np_dtype = table.dtype.type

    def updateRowsAdam(self, state, rows, grads, lr, step, beta1=0.9, beta2=0.999, eps=1e-8, sync=True):
        rows = np.array(rows)
        self.calls.append((state, rows, np.array(grads), lr, step, beta1, beta2, eps))
        local = rows - self.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        self.table[:], state.table[:] = replay_adam(self.table, state.table, local, grads, lr, step, beta1, beta2, eps)
        return True


class CyclicFake(FakeShard):
    """A cyclic partition's fake: global key k lives at local row k // parts."""

    def __init__(self, table, index, parts):
        super().__init__(table, 0)
        self.index, self.parts = index, parts

    def updateRowsAdam(self, state, rows, grads, *a, **kw):
        rows = np.array(rows)
        assert (rows % self.parts == self.index).all()
        self.calls.append((state, rows, np.array(grads)) + a)
        self.table[:], state.table[:] = replay_adam(self.table, state.table, rows // self.parts, grads, *a, **kw)
        return True


def _model(cols=7, dtype=np.float64, partitioner=None, nrows=300, seed=1):
    """3 partitions over |random| tables."""
    partitioner = partitioner or RangePartitioner.apply(3, nrows)
    rng = np.random.default_rng(seed)
    tables = [np.abs(rng.standard_normal((p.size, cols))).astype(dtype) for p in partitioner.all()]
    if isinstance(partitioner, CyclicPartitioner):
        shards = [CyclicFake(t, i, len(tables)) for i, t in enumerate(tables)]
    else:
        shards = [FakeShard(t, p.start) for t, p in zip(tables, partitioner.all())]
    return partitioner, shards, BigMatrix(partitioner, shards, nrows, cols)


@pytest.mark.parametrize("kind", ["range", "cyclic"])
def test_push_adam_buckets_by_partition(kind):
    make = (lambda: RangePartitioner.apply(3, 300)) if kind == "range" else (lambda: CyclicPartitioner.apply(3, 300))
    partitioner, wsh, m = _model(seed=1, partitioner=make())
    _, ssh, st = _model(seed=2, cols=14, partitioner=make())
    rng = np.random.default_rng(6)
    rows = rng.integers(0, 300, 200).astype(np.int64)  # every partition hit, interleaved, with repeats
    rows[10:13] = rows[10]
    owner = partitioner.partition_indices(rows)
    assert set(owner.tolist()) == {0, 1, 2} and (np.diff(owner) != 0).sum() > 50
    # the whole table in global row order, whatever the layout
    if kind == "range":
        glob = lambda shards: np.concatenate([s.table for s in shards])  # noqa: E731
    else:
        def glob(shards):
            out = np.empty((300, shards[0].table.shape[1]))
            for i, s in enumerate(shards):
                out[i::3] = s.table
            return out
    w_want, s_want = glob(wsh), glob(ssh)
    pushes = ((0.1, 1, dict(), rng.standard_normal((200, 7))),
              (0.01, 2, dict(beta1=0.5, beta2=0.75, eps=0.0), rng.standard_normal(200 * 7)))
    for lr, step, kw, g in pushes:
        for s in wsh + ssh:
            s.calls.clear()
        assert m.pushAdam(st, rows, g, lr, step, **kw)
        w_want, s_want = replay_adam(w_want, s_want, rows, g, lr, step, **kw)
        for p, s in enumerate(wsh):
            assert len(s.calls) == 1 and not ssh[p].calls  # one call per partition, on the weights shard
            state, r, sg, slr, sstep, sb1, sb2, seps = s.calls[0]
            assert state is ssh[p] and (slr, sstep) == (lr, step)  # with that partition's state shard
            assert (sb1, sb2, seps) == (kw.get("beta1", 0.9), kw.get("beta2", 0.999), kw.get("eps", 1e-8))
            np.testing.assert_array_equal(r, rows[owner == p])  # its rows only, in the caller's order
            np.testing.assert_array_equal(sg, g.reshape(200, 7)[owner == p])  # with their gradient rows
        np.testing.assert_array_equal(bits(glob(wsh)), bits(w_want))
        np.testing.assert_array_equal(bits(glob(ssh)), bits(s_want))


def test_push_adam_skips_partitions_without_rows_and_empty_pushes():
    _, wsh, m = _model(seed=1)
    _, ssh, st = _model(seed=2, cols=14)
    rows = np.array([250, 203, 250, 299, 3, 0], np.int64)  # nothing from partition 1
    m.pushAdam(st, rows, np.ones((6, 7)), 0.1, 1)
    assert len(wsh[0].calls) == 1 and not wsh[1].calls and len(wsh[2].calls) == 1
    for s in wsh:
        s.calls.clear()
    assert m.pushAdam(st, np.zeros(0, np.int64), np.zeros((0, 7)), 0.1, 1)
    assert all(not s.calls for s in wsh + ssh)


def test_push_adam_rejects_before_any_shard_is_called():
    _, wsh, m = _model(seed=1)
    _, ssh, st = _model(seed=2, cols=14)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAdam(st, np.array([3, 299, 300, 5], np.int64), np.zeros((4, 7)), 0.1, 1)
    with pytest.raises(IndexOutOfBoundsException):
        m.pushAdam(st, np.array([-1], np.int64), np.zeros((1, 7)), 0.1, 1)
    two = np.array([3, 4], np.int64)
    for g in (np.zeros((2, 6)), np.zeros((3, 7)), np.zeros(13), np.zeros((2, 14))):
        with pytest.raises(ValueError):
            m.pushAdam(st, two, g, 0.1, 1)
    others = [_model(cols=7)[2], _model(cols=15)[2],                              # state.cols != 2 * cols
              _model(cols=14, partitioner=CyclicPartitioner.apply(3, 300))[2],  # another partitioner
              _model(cols=14, partitioner=RangePartitioner.apply(2, 300))[2],   # other partitions
              _model(cols=14, nrows=301)[2],                                     # another row count
              _model(cols=14, dtype=np.float32)[2]]                              # another dtype
    for other in others:
        with pytest.raises(ValueError):
            m.pushAdam(other, two, np.zeros((2, 7)), 0.1, 1)
    with pytest.raises(ValueError):
        m.pushAdam(wsh[0], two, np.zeros((2, 7)), 0.1, 1)  # not a BigMatrix
    assert all(not s.calls for s in wsh + ssh)
