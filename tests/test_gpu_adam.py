"""Adam row push (PartialMatrix.updateRowsAdam, glint_mat_push_rows_adam*) against the replay.

The call is deterministic on every path -- no run is split, no atomic -- so the bar is one: both shards
equal adam_cases.replay_adam bit for bit (a NaN by class), on the host and on the device path.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import (ArrayIndexOutOfBoundsException, Client, CyclicPartition, CyclicPartitioner, PartialMatrix,
                       PartialVector, RangePartition, RangePartitioner)
from adam_cases import (BETA1, BETA2, EPS, adam_grads, adam_scalars, adam_start, adam_step, adam_sweep_inputs,
                        assert_bits, bits, fused_states, fusion_inputs, replay_adam, sweep_premises)
from ieee_cases import write_image

pytestmark = pytest.mark.gpu
DT = ["double", "float"]
START, SIZE = 1_000_003, 1500
RUNS = (15, 16, 17, 63, 64, 65)  # around the loads in flight (16) and the record ids per batch (64)
PATTERNS = ["sorted_once", "permutation", "duplicates", "one_row", "single", "empty"]
REPEATS = ("duplicates", "one_row")
PATHS = ["host", "dev"]
LR = 0.05


def npd_of(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def make_rows(rng, pattern):
    if pattern == "sorted_once":
        return np.arange(START, START + SIZE, dtype=np.int64)
    if pattern == "permutation":
        return rng.permutation(SIZE).astype(np.int64) + START
    if pattern == "duplicates":
        return rng.choice(rng.choice(SIZE, 40, replace=False), 3000).astype(np.int64) + START
    if pattern == "one_row":  # crosses the sort's 2048-key tile, the 64-id batch and the depth
        return np.full(2100, START + 777, np.int64)
    if pattern == "runs":  # one row per length of RUNS, their records interleaved
        return rng.permutation(np.repeat(np.arange(len(RUNS)) * 7 + 100, RUNS)).astype(np.int64) + START
    if pattern == "single":
        return np.array([START + 17], np.int64)
    return np.zeros(0, np.int64)


def pair(gpu, cols, dtype, size=SIZE, start=START):
    """(weights, state): the state shard has 2 * cols columns."""
    part = RangePartition(2, start, start + size)
    return PartialMatrix(part, cols, dtype, gpu), PartialMatrix(part, 2 * cols, dtype, gpu)


def fill(sh, table, start=START):
    """The table into a zero shard: 0 + x is x (the tables hold no -0.0)."""
    sh.updateRows(np.arange(start, start + table.shape[0], dtype=np.int64), table)


def push(w, s, gpu, rows, g, path, lr=LR, step=1, sync=True, **kw):
    if path == "host":
        assert w.updateRowsAdam(s, rows, g, lr, step, **kw)
        return
    import torch
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    assert w.updateRowsAdam(s, t(rows), t(g), lr, step, sync=sync, **kw)


@functools.lru_cache(maxsize=None)
def case(dtype, cols, pattern):
    """(rows, grads, weights and state after the pushes of step 1 and step 2 from adam_start): computed once
    and shared by the paths; read-only."""
    rng = np.random.default_rng(zlib.crc32(f"adam/{dtype}/{cols}/{pattern}".encode()))
    rows = make_rows(rng, pattern)
    name = np.dtype(npd_of(dtype)).name
    g = adam_grads(name, rows.size, cols)
    w, s = adam_start(name, SIZE, cols)
    for step in (1, 2):
        w, s = replay_adam(w, s, rows - START, g, LR, step)
    for a in (rows, w, s):
        a.setflags(write=False)
    return rows, g, w, s


# cols 1 and 3: less than a scalar slice; 67: two scalar slices; 128: the 16-B path, one slice; 130: Double
# two 16-B slices, Float the scalar path (520 B is no multiple of 16); 260 Float: two 16-B slices
COLS = [(dt, c) for dt in DT for c in (1, 3, 67, 128, 130)] + [("float", 260)]
CORE = {(dt, c, pat) for dt, c in COLS for pat in REPEATS}
WIDE = {(dt, c, pat) for dt, c in (("double", 1), ("float", 1), ("double", 130), ("float", 130), ("float", 260),
                                   ("double", 67), ("float", 128))
        for pat in PATTERNS}
EDGES = {(dt, c, "runs") for dt in DT for c in (67, 128)}
GRID = sorted(CORE | WIDE | EDGES)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols,pattern", GRID)
def test_adam_push_parity(gpu, dtype, cols, pattern, path):
    rows, g, want_w, want_s = case(dtype, cols, pattern)
    if pattern == "runs":
        assert sorted(np.unique(rows, return_counts=True)[1].tolist()) == list(RUNS)
    name = np.dtype(npd_of(dtype)).name
    w0, s0 = adam_start(name, SIZE, cols)
    w, s = pair(gpu, cols, dtype)
    with w, s:
        fill(w, w0)
        fill(s, s0)
        for step in (1, 2):  # the second push steps from the first one's state
            push(w, s, gpu, rows, g, path, step=step)
        assert_bits(s.to_numpy(), want_s, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- the two halves of a state row ----------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols", [(dt, c) for dt in DT for c in (3, 128)])
def test_adam_halves(gpu, dtype, cols, path):
    """m negative and v huge: a swap of the halves, or a v half read at another offset (at cols 3 it starts
    at no multiple of 16 B), would show in every element."""
    npd = npd_of(dtype)
    rng = np.random.default_rng(zlib.crc32(f"adam/halves/{dtype}/{cols}".encode()))
    w0 = rng.standard_normal((SIZE, cols)).astype(npd)
    m0 = -(1.0 + rng.random((SIZE, cols))).astype(npd)
    v0 = ((1.0 + rng.random((SIZE, cols))) * 2.0 ** 40).astype(npd)
    s0 = np.concatenate([m0, v0], 1)
    rows = rng.permutation(SIZE)[:700].astype(np.int64) + START
    g = rng.standard_normal((700, cols)).astype(npd)
    want_w, want_s = replay_adam(w0, s0, rows - START, g, LR, 1)
    swapped = replay_adam(w0, np.concatenate([v0, m0], 1), rows - START, g, LR, 1)
    named = np.unique(rows - START)
    assert (bits(swapped[0][named]) != bits(want_w[named])).all()  # the premise: the halves are told apart
    w, s = pair(gpu, cols, dtype)
    with w, s:
        fill(w, w0)
        fill(s, s0)
        push(w, s, gpu, rows, g, path)
        assert_bits(s.to_numpy(), want_s, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- a large step count: both corrections are 1 ------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DT)
def test_adam_large_step(gpu, dtype, path):
    npd = npd_of(dtype)
    cols = 67
    k = adam_scalars(npd, LR, 0.0, BETA2, EPS, 10 ** 6)
    assert k[0] == 0 and k[2] == 1 and k[4] == npd(LR) and k[5] == 1  # beta1 = 0: m' = G; alpha = lr; rc2 = 1
    rows, g, _, _ = case(dtype, cols, "duplicates")
    w0, s0 = adam_start(np.dtype(npd).name, SIZE, cols)
    want_w, want_s = replay_adam(w0, s0, rows - START, g, LR, 10 ** 6, beta1=0.0)
    w, s = pair(gpu, cols, dtype)
    with w, s:
        fill(w, w0)
        fill(s, s0)
        push(w, s, gpu, rows, g, path, step=10 ** 6, beta1=0.0)
        assert_bits(s.to_numpy(), want_s, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- correctly rounded sqrt and divide, subnormals kept ----------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("eps", [0.0, 2.0 ** -30])
@pytest.mark.parametrize("dtype", DT)
def test_adam_rounding_sweep(gpu, dtype, eps, path):
    """One push, every row once, cols 128: v over the type's whole exponent range, G over the Adagrad spans
    and the band near the square root of the smallest normal, m with a band of subnormals
    (adam_cases.adam_sweep_inputs). A fast sqrt or divide, or flushed subnormals, would show here. The
    premises are asserted first, on the CPU."""
    npd = npd_of(dtype)
    cols = 128
    m0, v0, G, w0 = adam_sweep_inputs(np.dtype(npd).name, SIZE, cols)
    k = adam_scalars(npd, LR, BETA1, BETA2, eps, 1)
    got = sweep_premises(npd, m0, v0, G, w0, k)
    print(f"{dtype} eps {eps}: {got}")
    assert min(got.values()) > 1000, got
    want_w, want_m, want_v = adam_step(w0, m0, v0, G, k)
    rows = np.random.default_rng(4).permutation(SIZE).astype(np.int64) + START
    w, s = pair(gpu, cols, dtype)
    with w, s:
        write_image(w, gpu, w0, npd(0))
        write_image(s, gpu, np.concatenate([m0, v0], 1), npd(0))
        push(w, s, gpu, rows, G[rows - START], path, LR, 1, eps=eps)
        assert_bits(s.to_numpy(), np.concatenate([want_m, want_v], 1), "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- no fused multiply-add ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("run", [1, 3])
@pytest.mark.parametrize("dtype,cols", [("double", 2), ("double", 67), ("float", 4), ("float", 67)])
def test_adam_is_unfused(gpu, dtype, cols, run, path):
    """adam_cases.fusion_inputs: the moments' sums cancel, so a product that was not rounded before its add
    shows in nearly every element. As a single record per row, and as the middle record of a run of three
    for the row (the others zero). cols 2 (Double) and 4 (Float) take the 16-B slice, 67 the scalar one."""
    npd = npd_of(dtype)
    G, m, v = fusion_inputs(npd)
    R = G.size // cols
    G, m, v = (a[:R * cols].reshape(R, cols) for a in (G, m, v))
    w0, s0 = np.zeros((SIZE, cols), npd), np.zeros((SIZE, 2 * cols), npd)
    w0[:R] = 3.0
    s0[:R] = np.concatenate([m, v], 1)
    local = np.arange(R, dtype=np.int64)
    if run == 1:
        rows, g = local + START, G
    else:
        rows = np.concatenate([local, local, local]) + START
        g = np.concatenate([np.zeros_like(G), G, np.zeros_like(G)])
    want_w, want_s = replay_adam(w0, s0, rows - START, g, LR, 1)
    k = adam_scalars(npd, LR, BETA1, BETA2, EPS, 1)
    fused = fused_states(m, v, G, k)
    for fm, fv in fused.values():  # the premise: every fused variant would be told from the contract
        assert (bits(np.concatenate([fm, fv], 1)) != bits(want_s[:R])).mean() > 0.45
    w, s = pair(gpu, cols, dtype)
    with w, s:
        fill(s, s0)
        fill(w, w0)
        assert_bits(s.to_numpy(), s0)
        push(w, s, gpu, rows, g, path)
        got = s.to_numpy()
        if (bits(got) != bits(want_s)).any():
            match = [name for name, (fm, fv) in fused.items()
                     if (bits(got[:R]) == bits(np.concatenate([fm, fv], 1))).all()]
            pytest.fail(f"the state is not the contract's; fused variants its bits match: {match or 'none'}")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- the bits do not depend on the alignment of grads -------------------------------------------------
def test_adam_path_independence(gpu):
    import torch
    cols = 128
    rows, g, want_w, want_s = case("double", cols, "duplicates")
    w0, s0 = adam_start("float64", SIZE, cols)
    d = torch.device("cuda", gpu)
    buf = torch.zeros(g.size + 3, dtype=torch.float64, device=d)
    v = buf[1:1 + g.size]  # the same values one element into a buffer: 8-B aligned only
    v.copy_(torch.from_numpy(np.array(g)).to(d).view(-1))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    w, s = pair(gpu, cols, "double")
    with w, s:
        fill(w, w0)
        fill(s, s0)
        for step in (1, 2):
            w.updateRowsAdam(s, torch.from_numpy(np.array(rows)).to(d), v, LR, step)
        assert_bits(s.to_numpy(), want_s, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- IEEE edges and padding -----------------------------------------------------------------------------
def read_image(sh, gpu, rows):
    """The shard's memory as it lies, pitch padding included: (rows, pitch)."""
    import torch
    pitch = C.c_int64()
    assert N.load().glint_shard_pitch(sh.handle, C.byref(pitch)) == N.GLINT_OK
    d = torch.device("cuda", gpu)
    dst = torch.empty((rows, pitch.value), dtype=sh.torch_dtype, device=d)
    segs = np.array([0, 0, dst.numel() * dst.element_size()], np.int64)
    assert N.load().glint_copy_segments_dev(sh.data_ptr(), dst.data_ptr(), segs.ctypes.data_as(C.POINTER(C.c_int64)),
                                            1, torch.cuda.current_stream(d).cuda_stream) == N.GLINT_OK
    torch.cuda.synchronize(d)
    return dst.cpu().numpy()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("double", 6), ("float", 67), ("float", 12)])
def test_adam_ieee_edges(gpu, dtype, cols, path):
    """0 / 0 is NaN, infinite and NaN gradients, an overflowing G * G, the sign of a zero step, an unnamed
    row's bits and the pitch padding of both shards; each against the replay, a NaN by class."""
    npd = npd_of(dtype)
    big = npd(1e200 if dtype == "double" else 1e30)
    nan_bits = 0x7FF8000000000123 if dtype == "double" else 0x7FC00123
    payload = np.array([nan_bits], np.uint64 if dtype == "double" else np.uint32).view(npd)[0]
    w0 = np.full((8, cols), 1.5, npd)
    s0 = np.concatenate([np.full((8, cols), 0.25, npd), np.ones((8, cols), npd)], 1)
    s0[0] = 0         # row 0: G = 0, m = 0, v = 0, eps = 0 -> 0 / 0
    w0[4] = -0.0      # row 4: m = 0 and G = 0 give u = +0 and p = +0: -0 - (+0) = -0
    s0[4, :cols] = 0
    for t in (w0, s0):  # row 6 is not named: its bits stay, whatever they are
        t[6, 0::2], t[6, 1::2] = -0.0, payload
    rows = np.array([START, START + 1, START + 2, START + 3, START + 4, START + 3, START + 5], np.int64)
    g = np.zeros((7, cols), npd)
    g[1] = np.inf              # row 1: m', v' and d infinite, p = inf / inf
    g[2, 0::2], g[2, 1::2] = np.nan, -np.inf
    g[3], g[5] = big, big / 4  # row 3 twice: G = 1.25 big, G * G overflows, d is infinite, p = 0
    g[4] = -0.0                # +0 + -0 is +0
    g[6] = 1.0                 # row 5: an ordinary step next to them
    want_w, want_s = replay_adam(w0, s0, rows - START, g, 0.5, 1, eps=0.0)
    # the premises, from the replay
    assert np.isnan(want_w[0]).all() and (want_s[0] == 0).all()
    assert np.isnan(want_w[1]).all() and np.isinf(want_s[1]).all()
    assert np.isnan(want_w[2]).all()
    assert np.isnan(want_s[2, :cols][0::2]).all() and np.isnan(want_s[2, cols:][0::2]).all()
    assert np.isinf(want_s[2, :cols][1::2]).all() and np.isinf(want_s[2, cols:][1::2]).all()
    assert np.isinf(want_s[3, cols:]).all() and np.isfinite(want_s[3, :cols]).all() and (want_w[3] == w0[3]).all()
    assert (bits(want_w[4]) == bits(npd(-0.0))).all()
    assert np.isfinite(want_w[5]).all() and (want_w[5] != w0[5]).all()
    pad = npd(777.0)
    w, s = pair(gpu, cols, dtype, 8)
    with w, s:
        write_image(w, gpu, w0, pad)
        write_image(s, gpu, s0, pad)
        push(w, s, gpu, rows, g, path, 0.5, 1, eps=0.0)
        padded = 0
        for sh, want, was, width in ((w, want_w, w0, cols), (s, want_s, s0, 2 * cols)):
            raw = read_image(sh, gpu, 8)
            assert_bits(raw[:6, :width], want[:6])
            np.testing.assert_array_equal(bits(raw[6:, :width]), bits(was[6:]))  # payload and sign kept
            assert (raw[:, width:] == pad).all()  # neither read (no NaN) nor written
            padded += raw.shape[1] > width
        assert padded == {("double", 67): 1, ("float", 67): 2}.get((dtype, cols), 0)  # a row of 16 B multiples has none


# ---- errors and arguments -------------------------------------------------------------------------------
def _error_input():
    rng = np.random.default_rng(3)
    cols = 6
    rows = rng.integers(START, START + SIZE, 100).astype(np.int64)
    rows[7] = START - 1
    rows[60] = START + SIZE
    return cols, rows, rng.standard_normal((100, cols))


def test_adam_push_errors_host(gpu):
    cols, rows, g = _error_input()
    w0, s0 = adam_start("float64", SIZE, cols)
    w, s = pair(gpu, cols, "double")
    with w, s:
        fill(w, w0)
        fill(s, s0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            w.updateRowsAdam(s, rows, g, LR, 1)
        assert ei.value.record == 7
        assert_bits(w.to_numpy(), w0)  # a rejected message changes neither shard
        assert_bits(s.to_numpy(), s0)


def test_adam_push_errors_device(gpu):
    cols, rows, g = _error_input()
    w0, s0 = adam_start("float64", SIZE, cols)
    keep = np.ones(100, bool)
    keep[[7, 60]] = False
    want_w, want_s = replay_adam(w0, s0, rows[keep] - START, g[keep], LR, 1)
    w, s = pair(gpu, cols, "double")
    with w, s:
        fill(w, w0)
        fill(s, s0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push(w, s, gpu, rows, g, "dev")
        assert ei.value.record == 7
        s.sync()  # the state shard was marked too; it has no error of its own
        assert_bits(w.to_numpy(), want_w)  # the other 98 records were applied
        assert_bits(s.to_numpy(), want_s)


def test_adam_push_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    g = np.ones(4, np.float64)
    rd, gd = torch.from_numpy(r).to(d), torch.from_numpy(g).to(d)
    host = lib.glint_mat_push_rows_adam
    devc = lambda *args: lib.glint_mat_push_rows_adam_dev(*args, None)  # noqa: E731
    calls = ((host, r.ctypes.data, g.ctypes.data), (devc, rd.data_ptr(), gd.data_ptr()))
    part = RangePartition(0, START, START + 10)
    nan = float("nan")
    w, s = pair(gpu, 4, "double", 10)
    with w, s:
        others = {
            "cols": PartialMatrix(part, 4, "double", gpu), "cols+1": PartialMatrix(part, 9, "double", gpu),
            "size": PartialMatrix(RangePartition(0, START, START + 11), 8, "double", gpu),
            "dtype": PartialMatrix(part, 8, "float", gpu),
            "start": PartialMatrix(RangePartition(0, START + 1, START + 11), 8, "double", gpu),
            "kind": PartialMatrix(CyclicPartition(0, 2, 20), 8, "double", gpu),
            "int": PartialMatrix(part, 4, "int", gpu), "int2": PartialMatrix(part, 8, "int", gpu),
            "long": PartialMatrix(part, 4, "long", gpu), "long2": PartialMatrix(part, 8, "long", gpu),
            "vector": PartialVector(part, "double", gpu), "vector2": PartialVector(part, "double", gpu),
        }
        cyc = [PartialMatrix(CyclicPartition(0, 2, 20), 4, "double", gpu),
               PartialMatrix(CyclicPartition(1, 2, 20), 8, "double", gpu)]
        assert cyc[0].size == cyc[1].size == others["kind"].size == 10
        try:
            for call, pr, pg in calls:
                def ok(a, b, n=1, rows=pr, grads=pg, lr=0.1, beta1=0.9, beta2=0.999, eps=0.0, step=1, call=call):
                    return call(a, b, rows, grads, n, lr, beta1, beta2, eps, step)

                assert ok(None, s.handle) == N.GLINT_EINVAL
                assert ok(w.handle, None) == N.GLINT_EINVAL
                assert ok(w.handle, w.handle) == N.GLINT_EINVAL  # state is weights
                assert ok(s.handle, w.handle) == N.GLINT_EINVAL  # the two the wrong way round
                for name in ("cols", "cols+1", "size", "dtype", "start", "kind"):
                    assert ok(w.handle, others[name].handle) == N.GLINT_EINVAL, name
                assert ok(cyc[0].handle, cyc[1].handle) == N.GLINT_EINVAL  # another cyclic index
                for name in ("int", "long", "vector"):
                    assert ok(others[name].handle, others[name + "2"].handle) == N.GLINT_EINVAL, name
                    assert ok(others[name].handle, s.handle) == N.GLINT_EINVAL, name
                assert ok(w.handle, s.handle, n=-1) == N.GLINT_EINVAL
                assert ok(w.handle, s.handle, n=(1 << 32) - 2048) == N.GLINT_EINVAL
                assert ok(w.handle, s.handle, rows=None) == N.GLINT_EINVAL
                assert ok(w.handle, s.handle, grads=None) == N.GLINT_EINVAL
                assert ok(w.handle, s.handle, lr=nan) == N.GLINT_EINVAL
                assert ok(w.handle, s.handle, eps=-1e-300) == N.GLINT_EINVAL
                assert ok(w.handle, s.handle, eps=nan) == N.GLINT_EINVAL
                for bad in (1.0, -0.1, nan, 1.5):
                    assert ok(w.handle, s.handle, beta1=bad) == N.GLINT_EINVAL, bad
                    assert ok(w.handle, s.handle, beta2=bad) == N.GLINT_EINVAL, bad
                for bad in (0, -1):
                    assert ok(w.handle, s.handle, step=bad) == N.GLINT_EINVAL, bad
                assert ok(w.handle, s.handle, n=0, rows=None, grads=None) == N.GLINT_OK
            assert not w.to_numpy().any() and not s.to_numpy().any()
            # the Python layer: types, then shapes, before any call
            with pytest.raises(TypeError):
                others["int"].updateRowsAdam(others["int2"], r, np.ones(4, np.int32), 0.1, 1)
            with pytest.raises(TypeError):
                w.updateRowsAdam(s.handle, r, g, 0.1, 1)  # state is a PartialMatrix
            with pytest.raises(TypeError):
                w.updateRowsAdam(s, rd, g, 0.1, 1)  # grads on the host
            with pytest.raises(TypeError):
                w.updateRowsAdam(s, r, gd, 0.1, 1)  # rows on the host
            with pytest.raises(TypeError):
                w.updateRowsAdam(s, rd, gd.to(torch.float32), 0.1, 1)
            for bad in (np.ones(3), np.ones((2, 4)), np.ones(5), np.ones(8)):
                with pytest.raises(ValueError):
                    w.updateRowsAdam(s, r, bad, 0.1, 1)
            with pytest.raises(ValueError):
                w.updateRowsAdam(s, rd, torch.ones(5, dtype=torch.float64, device=d), 0.1, 1)
            assert not w.to_numpy().any() and not s.to_numpy().any()
            # and what is valid: the default betas and eps, beta = 0, a cyclic pair
            assert w.updateRowsAdam(s, r, g, 0.5, 1) and w.updateRowsAdam(s, rd, gd, 0.5, 2)
            zero, zero2 = np.zeros((10, 4)), np.zeros((10, 8))
            want = replay_adam(*replay_adam(zero, zero2, [0], g[None], 0.5, 1), [0], g[None], 0.5, 2)
            assert_bits(w.to_numpy(), want[0])
            assert_bits(s.to_numpy(), want[1])
            same = PartialMatrix(CyclicPartition(0, 2, 20), 8, "double", gpu)
            with same:
                assert cyc[0].updateRowsAdam(same, np.array([6], np.int64), g, 0.5, 1, beta1=0.0, beta2=0.0)  # local 3
                want = replay_adam(zero, zero2, [3], g[None], 0.5, 1, beta1=0.0, beta2=0.0)
                assert_bits(cyc[0].to_numpy(), want[0])
                assert_bits(same.to_numpy(), want[1])
        finally:
            for sh in list(others.values()) + cyc:
                sh.destroy()


def test_adam_push_slabs_with_views(gpu):
    """A slab that has views is refused as either shard, on both paths; its views hold the slab's cols, so
    two of them never make a weights / state pair."""
    import torch
    lib = N.load()
    cols = 32  # a row is 256 B: every row offset is a valid view offset
    d = torch.device("cuda", gpu)
    r = np.array([START + 3], np.int64)
    g = np.ones(cols)
    rd, gd = torch.from_numpy(r).to(d), torch.from_numpy(g).to(d)
    part = RangePartition(0, START, START + 10)
    slab = PartialMatrix(part, cols, "double", gpu)
    slab2 = PartialMatrix(part, 2 * cols, "double", gpu)
    plain_w, plain_s = PartialMatrix(part, cols, "double", gpu), PartialMatrix(part, 2 * cols, "double", gpu)
    views = [PartialMatrix.view(slab, RangePartition(1, START, START + 5), 0),
             PartialMatrix.view(slab, RangePartition(1, START, START + 5), 5),
             PartialMatrix.view(slab2, RangePartition(1, START, START + 5), 0)]
    try:
        args = (0.1, 0.9, 0.999, 0.0, 1)
        for a, b in ((slab, plain_s), (plain_w, slab2), (views[0], views[1])):
            assert lib.glint_mat_push_rows_adam(a.handle, b.handle, r.ctypes.data, g.ctypes.data, 1,
                                                *args) == N.GLINT_EINVAL
            assert lib.glint_mat_push_rows_adam_dev(a.handle, b.handle, rd.data_ptr(), gd.data_ptr(), 1, *args,
                                                    None) == N.GLINT_EINVAL
        assert not views[0].to_numpy().any() and not views[2].to_numpy().any() and not plain_w.to_numpy().any()
        assert views[0].updateRowsAdam(views[2], r, g, LR, 1)  # views of two slabs are a pair
        want_w, want_s = replay_adam(np.zeros((5, cols)), np.zeros((5, 2 * cols)), r - START, g[None], LR, 1)
        assert_bits(views[0].to_numpy(), want_w)
        assert_bits(views[2].to_numpy(), want_s)
    finally:
        for v in views:
            v.destroy()
        for sh in (slab, slab2, plain_w, plain_s):
            sh.destroy()


# ---- ordering across the two shards -----------------------------------------------------------------------
def _ordering_input(cols):
    rng = np.random.default_rng(12)
    er = rng.integers(START, START + 200, 1000).astype(np.int64)
    ec = rng.integers(0, 2 * cols, 1000).astype(np.int32)
    ev = rng.integers(1, 50, 1000).astype(np.float64)  # small integers: their sums are exact in any order
    rows = rng.integers(START, START + 200, 900).astype(np.int64)
    g = adam_grads("float64", 900, cols, "ordering")
    s1 = np.zeros((SIZE, 2 * cols))
    np.add.at(s1, (er - START, ec), ev)
    zero = np.zeros((SIZE, cols))
    want_w, want_s = replay_adam(zero, s1, rows - START, g, LR, 1)
    assert (bits(want_w) != bits(replay_adam(zero, np.zeros((SIZE, 2 * cols)), rows - START, g, LR, 1)[0])).mean() \
        > 0.05  # the state push shows in the weights
    return er, ec, ev, rows, g, want_w, want_s


def test_adam_push_after_unwaited_state_push_host(gpu):
    """A message-sized push into the state shard, staged and not waited for, then the host Adam push: the
    step reads the state after that push."""
    cols = 9
    er, ec, ev, rows, g, want_w, want_s = _ordering_input(cols)
    w, s = pair(gpu, cols, "double")
    with w, s:
        ticket = s.push_async(er, ec, ev)
        assert w.updateRowsAdam(s, rows, g, LR, 1)
        q = np.arange(START, START + SIZE, dtype=np.int64)
        got_s, got_w = s.getRows(q), w.getRows(q)
        s.wait(ticket)
        assert_bits(np.asarray(got_s), want_s, "state")
        assert_bits(np.asarray(got_w), want_w, "weights")


def test_adam_push_after_state_push_device(gpu):
    """A device element push into the state shard on a second stream; the Adam push on the current stream
    behind an event of that one; one sync per shard at the end."""
    import torch
    cols = 9
    er, ec, ev, rows, g, want_w, want_s = _ordering_input(cols)
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    w, s = pair(gpu, cols, "double")
    with w, s:
        dev = [t(a) for a in (er, ec, ev, rows, g)]
        torch.cuda.synchronize(d)
        side = torch.cuda.Stream(d)
        with torch.cuda.stream(side):
            s.update(dev[0], dev[1], dev[2], sync=False)
            done = side.record_event()
        torch.cuda.current_stream(d).wait_event(done)
        w.updateRowsAdam(s, dev[3], dev[4], LR, 1, sync=False)
        w.sync(w._stream_of(dev[3]))
        s.sync(side.cuda_stream)
        s.sync(s._stream_of(dev[3]))  # the stream of the last call that marked it
        assert_bits(s.to_numpy(), want_s, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


def test_adam_push_then_pull_on_one_stream(gpu):
    """Two Adam pushes with sync=False and two row pulls on one stream, one sync per shard at the end."""
    import torch
    cols = 9
    rng = np.random.default_rng(21)
    d = torch.device("cuda", gpu)
    r1, g1 = rng.integers(START, START + 200, 700).astype(np.int64), adam_grads("float64", 700, cols, "stream1")
    r2, g2 = rng.integers(START + 100, START + 300, 900).astype(np.int64), adam_grads("float64", 900, cols, "stream2")
    q = np.arange(START, START + 300, dtype=np.int64)
    want_w, want_s = replay_adam(np.zeros((SIZE, cols)), np.zeros((SIZE, 2 * cols)), r1 - START, g1, LR, 1)
    want_w, want_s = replay_adam(want_w, want_s, r2 - START, g2, LR, 2)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    w, s = pair(gpu, cols, "double")
    with w, s:
        dev = [t(a) for a in (r1, g1, r2, g2, q)]
        w.updateRowsAdam(s, dev[0], dev[1], LR, 1, sync=False)
        w.updateRowsAdam(s, dev[2], dev[3], LR, 2, sync=False)
        out_w, out_s = w.getRows(dev[4], sync=False), s.getRows(dev[4], sync=False)
        w.sync(w._stream_of(dev[4]))
        s.sync(s._stream_of(dev[4]))
        assert_bits(out_w.cpu().numpy(), want_w[:300], "weights")
        assert_bits(out_s.cpu().numpy(), want_s[:300], "state")


# ---- launch count, client -----------------------------------------------------------------------------------
def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_adam_push_profiling_id(gpu):
    rows = np.arange(START, START + 100, dtype=np.int64)
    w, s = pair(gpu, 4, "double")
    ref = PartialMatrix(RangePartition(2, START, START + SIZE), 4, "double", gpu)  # a plain row push beside it
    with w, s, ref:
        for sh in (w, s, ref):
            assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        total = lambda sh: sum(_launches(sh, k) for k in range(N.GLINT_K_COUNT))  # noqa: E731
        assert (total(w), total(s), total(ref)) == (0, 0, 0)
        ref.updateRows(np.repeat(rows, 3), np.ones((300, 4)), deterministic=True)
        push(w, s, gpu, np.repeat(rows, 3), np.ones((300, 4)), "host")
        # the front end's launches are not timed, in either call: one fold launch each, under the row push's id
        assert _launches(w, N.GLINT_K_PUSH_ROWS) == _launches(ref, N.GLINT_K_PUSH_ROWS) == 1
        assert total(w) == total(ref) == 1 and total(s) == 0
        push(w, s, gpu, rows, np.ones((100, 4)), "dev", step=2)
        assert _launches(w, N.GLINT_K_PUSH_ROWS) == 2 and total(w) == 2 and total(s) == 0
        push(w, s, gpu, rows[:0], np.ones((0, 4)), "host")  # an empty call launches nothing
        push(w, s, gpu, rows[:0], np.ones((0, 4)), "dev")
        assert total(w) == 2 and total(s) == 0


@pytest.mark.parametrize("kind", ["range", "cyclic"])
def test_adam_push_client(gpu, kind):
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 1000, 5000).astype(np.int64)
    make = RangePartitioner.apply if kind == "range" else CyclicPartitioner.apply
    c = Client([gpu] * 3)
    m = c.matrix(1000, 7, "double", createPartitioner=make)
    st = c.matrix(1000, 14, "double", createPartitioner=make)
    other = c.matrix(1000, 7, "double", createPartitioner=make)
    try:
        assert m.nrOfPartitions == 3
        with pytest.raises(ValueError):
            m.pushAdam(other, rows, np.zeros((5000, 7)), LR, 1)
        want_w, want_s = np.zeros((1000, 7)), np.zeros((1000, 14))
        for step in (1, 2, 3):
            g = adam_grads("float64", 5000, 7, f"client{step}")
            assert m.pushAdam(st, rows, g, LR, step)
            want_w, want_s = replay_adam(want_w, want_s, rows, g, LR, step)
        assert_bits(m.pull(np.arange(1000)), want_w, "weights")
        assert_bits(st.pull(np.arange(1000)), want_s, "state")
        assert not other.pull(np.arange(1000)).any()
    finally:
        for x in (m, st, other):
            x.destroy()
