"""Row-wise Adagrad row push (PartialMatrix.updateRowsAdagradRowwise, glint_mat_push_rows_adagrad_rowwise*)
against the replay.

The call is deterministic on every path -- no run is split, no atomic -- so the bar is one: the weights
shard and the state vector equal rowwise_cases.replay_rowwise bit for bit (a NaN by class), on the host and
on the device path. test_rowwise_cpu.py asserts, from the replay alone, that the inputs used here tell the
contract's order, divisions and unfused operations from their alternatives.
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
from ieee_cases import write_image
from rowwise_cases import (EPS, LR, adagrad_inputs, assert_bits, bits, lane_width, premise_pushes, replay_rowwise, rowwise_step,
                           rowwise_terms, start_state)

pytestmark = pytest.mark.gpu
DT = ["double", "float"]
KINDS = ["range", "cyclic"]
PATHS = ["host", "dev"]
START, SIZE = 1_000_003, 300
PATTERNS = ["once", "hot150", "repeats", "run64_65"]


def npd_of(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def name_of(dtype):
    return np.dtype(npd_of(dtype)).name


def partition(kind, size=SIZE):
    return RangePartition(2, START, START + size) if kind == "range" else CyclicPartition(1, 3, 3 * size)


def keys_of(kind, local):
    """The global keys of local rows under partition(kind)."""
    local = np.asarray(local, np.int64)
    return local + START if kind == "range" else local * 3 + 1


def pair(gpu, cols, dtype, kind="range", size=SIZE):
    part = partition(kind, size)
    w, h = PartialMatrix(part, cols, dtype, gpu), PartialVector(part, dtype, gpu)
    assert w.size == h.size == size
    return w, h


def fill(w, h, w0, h0, kind="range"):
    """The tables into zero shards: 0 + x is x (the tables hold no -0.0)."""
    keys = keys_of(kind, np.arange(w0.shape[0]))
    w.updateRows(keys, w0)
    h.update(keys, h0)


def push(w, h, gpu, keys, g, path, lr=LR, eps=EPS, sync=True):
    if path == "host":
        assert w.updateRowsAdagradRowwise(h, keys, g, lr, eps)
        return
    import torch
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    assert w.updateRowsAdagradRowwise(h, t(keys), t(g), lr, eps, sync=sync)


def make_local(rng, pattern):
    if pattern == "once":
        return rng.permutation(SIZE).astype(np.int64)
    if pattern == "hot150":  # crosses the 64-id batch twice and leaves 22 = 16 + 6: a tail under the load depth
        return np.full(150, 177, np.int64)
    if pattern == "repeats":
        return rng.choice(rng.choice(SIZE, 40, replace=False), 2000).astype(np.int64)
    local = np.concatenate([np.full(64, 5), np.full(65, 250), rng.integers(0, SIZE, 30)]).astype(np.int64)
    local[-30:][np.isin(local[-30:], (5, 250))] = 6  # the two runs stay exactly 64 and 65
    return rng.permutation(local)


@functools.lru_cache(maxsize=None)
def case(dtype, cols, pattern):
    """(local rows, grads, weights and state after the push applied twice from start_state): computed once
    and shared by the paths and partition kinds; read-only."""
    rng = np.random.default_rng(zlib.crc32(f"rowwise/{dtype}/{cols}/{pattern}".encode()))
    local = make_local(rng, pattern)
    if pattern == "run64_65":
        assert (local == 5).sum() == 64 and (local == 250).sum() == 65
    g = adagrad_inputs(name_of(dtype), local.size, cols, "rowwise/case")
    w, h = start_state(name_of(dtype), SIZE, cols)
    for _ in range(2):
        w, h = replay_rowwise(w, h, local, g, LR, EPS)
    for a in (local, w, h):
        a.setflags(write=False)
    return local, g, w, h


KEEP = N.GLINT_ROWWISE_KEEP_STRIPS  # rows of more strips take the fold's other path


# E = 1 with a second strip of 3 live lanes (1, 3, 67); E > 1 with one partial strip (4 / 2, 128, 260); and
# both sides of the fold's width boundary in either layout: KEEP strips and one lane more.
def grid_cols(dtype):
    E = 4 if dtype == "float" else 2
    return (1, 3, 67, E, 128, 260, 64 * KEEP - 1, 64 * KEEP + 1, 64 * E * KEEP, 64 * E * KEEP + E)


GRID = [(dt, c, pat) for dt in DT for c in grid_cols(dt) for pat in PATTERNS]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dtype,cols,pattern", GRID)
def test_rowwise_push_parity(gpu, dtype, cols, pattern, kind, path):
    E = lane_width(npd_of(dtype), cols)
    assert (E > 1) == (cols in grid_cols(dtype)[3:6] + grid_cols(dtype)[8:])  # the layout the case is there for
    local, g, want_w, want_h = case(dtype, cols, pattern)
    w0, h0 = start_state(name_of(dtype), SIZE, cols)
    w, h = pair(gpu, cols, dtype, kind)
    with w, h:
        fill(w, h, w0, h0, kind)
        for _ in range(2):  # the second push steps from the first one's state
            push(w, h, gpu, keys_of(kind, local), g, path)
        assert_bits(h.to_numpy(), want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


# ---- the bits do not depend on the alignment of grads -------------------------------------------------
@pytest.mark.parametrize("eps", [0.0, 2.0 ** -30])
@pytest.mark.parametrize("dtype", DT)
def test_rowwise_alignment_independence(gpu, dtype, eps):
    import torch
    cols = 128
    npd = npd_of(dtype)
    local, g, _, _ = case(dtype, cols, "repeats")
    w0, h0 = start_state(name_of(dtype), SIZE, cols)
    want_w, want_h = replay_rowwise(w0, h0, local, g, LR, eps)
    d = torch.device("cuda", gpu)
    size = np.dtype(npd).itemsize
    buf = torch.zeros(g.size + 16, dtype=getattr(torch, name_of(dtype)), device=d)
    v = buf[1:1 + g.size]  # the same values one element into a buffer: not 16-B aligned
    v.copy_(torch.from_numpy(np.array(g)).to(d).view(-1))
    assert v.data_ptr() % 16 == size and v.is_contiguous()
    keys = torch.from_numpy(keys_of("range", local)).to(d)
    got = []
    for grads in (v, torch.from_numpy(np.array(g)).to(d)):
        assert (grads.data_ptr() % 16 == 0) == (grads is not v)
        w, h = pair(gpu, cols, dtype)
        with w, h:
            fill(w, h, w0, h0)
            w.updateRowsAdagradRowwise(h, keys, grads, LR, eps)
            got.append((w.to_numpy(), h.to_numpy()))
    for gw, gh in got:
        assert_bits(gh, want_h, "state")
        assert_bits(gw, want_w, "weights")
    np.testing.assert_array_equal(bits(got[0][0]), bits(got[1][0]))
    np.testing.assert_array_equal(bits(got[0][1]), bits(got[1][1]))


# ---- unfused and ordered --------------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype", DT)
def test_rowwise_is_unfused_and_ordered(gpu, dtype, path):
    """The premise inputs of test_rowwise_cpu.py, pushed: the order of ss, ss / C and lr / d as divisions, the
    cancelling update, the lane chains a fused add would change. The shards equal the unfused,
    contract-order replay."""
    for label, G, h0, w0 in premise_pushes(name_of(dtype)):
        m, cols = G.shape
        want_w, want_h = rowwise_step(w0, h0, G, LR, EPS)
        w, h = pair(gpu, cols, dtype, "range", m)
        with w, h:
            write_image(w, gpu, w0, npd_of(dtype)(0))
            fill_state(h, h0)
            order = np.random.default_rng(3).permutation(m)
            push(w, h, gpu, keys_of("range", order), G[order], path)
            assert_bits(h.to_numpy(), want_h, f"{label}: state")
            assert_bits(w.to_numpy(), want_w, f"{label}: weights")


def fill_state(h, h0, kind="range"):
    """Every element of the state vector = h0's, bits kept (-0.0, a NaN's payload): one fill per element."""
    for l, v in enumerate(h0):
        h.fill(v, keys_of(kind, [l]))


# ---- row coupling, IEEE edges, untouched memory -------------------------------------------------------------
def read_image(sh, gpu, rows, pitch):
    import torch
    d = torch.device("cuda", gpu)
    dst = torch.empty((rows, pitch), dtype=sh.torch_dtype, device=d)
    segs = np.array([0, 0, dst.numel() * dst.element_size()], np.int64)
    assert N.load().glint_copy_segments_dev(sh.data_ptr(), dst.data_ptr(), segs.ctypes.data_as(C.POINTER(C.c_int64)),
                                            1, torch.cuda.current_stream(d).cuda_stream) == N.GLINT_OK
    torch.cuda.synchronize(d)
    return dst.cpu().numpy()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("double", 6), ("float", 67), ("float", 12)])
def test_rowwise_ieee_edges_and_untouched_memory(gpu, dtype, cols, path):
    """The coupled row: a NaN column, an infinite element, an overflowing G * G, subnormals, 0 / 0; the rows
    between them, which the push does not name, and the pitch padding of the weights keep their bits."""
    npd = npd_of(dtype)
    info = np.finfo(npd)
    big = npd(1e200 if dtype == "double" else 1e30)
    nan_bits = 0x7FF8000000000123 if dtype == "double" else 0x7FC00123
    payload = np.array([nan_bits], np.uint64 if dtype == "double" else np.uint32).view(npd)[0]
    m = 12
    w0, h0 = np.full((m, cols), 1.5, npd), np.ones(m, npd)
    for r in range(1, m, 2):  # the odd rows are not named: their bits stay, whatever they are
        w0[r, 0::2], w0[r, 1::2] = -0.0, payload
        h0[r] = payload if r % 4 == 1 else -0.0
    named = np.array([0, 2, 4, 6, 8, 4], np.int64)
    g = np.zeros((6, cols), npd)
    g[0] = 0.25
    g[0, cols // 2] = np.nan            # row 0: one NaN column
    g[1] = 0.5
    g[1, cols - 1] = np.inf             # row 2: one infinite element
    g[2], g[5] = big, big / 4           # row 4 twice: G = 1.25 big, G * G overflows
    tiny_root = np.ldexp(npd(1.5), info.minexp // 2 - 6)  # its square is subnormal, and so is a row's sum
    g[3, 0::2] = tiny_root              # row 6: subnormal products, subnormal G elements, subnormal h
    g[3, 1::2] = -info.smallest_subnormal * 9
    h0[6] = info.smallest_subnormal * 5
    w0[6] = 0                           # (weights that a subnormal p changes)
    h0[8] = 0                           # row 8: G = 0, h = 0, eps = 0
    want_w, want_h = replay_rowwise(w0, h0, named, g, 0.5, 0.0)
    # the premises, from the replay
    assert np.isnan(want_w[0]).all() and np.isnan(want_h[0])
    assert np.isinf(want_h[2]) and np.isnan(want_w[2, cols - 1]) and (want_w[2, :cols - 1] == 1.5).all()
    assert np.isinf(want_h[4]) and (bits(want_w[4]) == bits(w0[4])).all()
    sub = lambda a: (a != 0) & (np.abs(a) < info.tiny)  # noqa: E731
    t6 = rowwise_terms(w0[6:7], h0[6:7], g[3:4], 0.5, 0.0)
    assert sub(want_h[6]) and want_h[6] != h0[6] and sub(t6["ss"]).all() and (want_w[6] != 0).all()
    assert np.isnan(want_w[8]).all() and want_h[8] == 0
    pad = npd(777.0)
    w, h = pair(gpu, cols, dtype, "range", m)
    with w, h:
        write_image(w, gpu, w0, pad)
        fill_state(h, h0)
        np.testing.assert_array_equal(bits(h.to_numpy()), bits(h0))  # the payload and -0.0 are in place
        push(w, h, gpu, keys_of("range", named), g, path, 0.5, 0.0)
        pitch = C.c_int64()
        assert N.load().glint_shard_pitch(w.handle, C.byref(pitch)) == N.GLINT_OK
        assert (pitch.value > cols) == (cols == 67)  # only a row that is no multiple of 16 B is padded
        raw = read_image(w, gpu, m, pitch.value)
        got_h = h.to_numpy()
        assert_bits(raw[0::2, :cols], want_w[0::2], "weights")
        assert_bits(got_h[0::2], want_h[0::2], "state")
        np.testing.assert_array_equal(bits(raw[1::2, :cols]), bits(w0[1::2]))  # payload and sign kept
        np.testing.assert_array_equal(bits(got_h[1::2]), bits(h0[1::2]))
        assert (raw[:, cols:] == pad).all()  # neither read (no NaN) nor written


@pytest.mark.parametrize("path", PATHS)
def test_rowwise_unnamed_rows_untouched(gpu, path):
    """A push that names a tenth of the rows: every other row of both shards keeps its bits."""
    cols = 67
    rng = np.random.default_rng(15)
    local = rng.choice(SIZE, 30, replace=False).astype(np.int64)
    g = adagrad_inputs("float32", 30, cols, "rowwise/unnamed")
    w0, h0 = start_state("float32", SIZE, cols)
    want_w, want_h = replay_rowwise(w0, h0, local, g, LR, EPS)
    rest = np.setdiff1d(np.arange(SIZE), local)
    w, h = pair(gpu, cols, "float")
    with w, h:
        fill(w, h, w0, h0)
        push(w, h, gpu, keys_of("range", local), g, path)
        got_w, got_h = w.to_numpy(), h.to_numpy()
        np.testing.assert_array_equal(bits(got_w[rest]), bits(w0[rest]))
        np.testing.assert_array_equal(bits(got_h[rest]), bits(h0[rest]))
        assert (bits(got_w[local]) != bits(w0[local])).any() and (bits(got_h[local]) != bits(h0[local])).all()
        assert_bits(got_w, want_w, "weights")
        assert_bits(got_h, want_h, "state")


# ---- errors and arguments -------------------------------------------------------------------------------
def _error_input():
    rng = np.random.default_rng(3)
    cols = 6
    rows = rng.integers(START, START + SIZE, 100).astype(np.int64)
    rows[7] = START - 1
    rows[60] = START + SIZE
    return cols, rows, rng.standard_normal((100, cols))


def test_rowwise_push_errors_host(gpu):
    cols, rows, g = _error_input()
    w0, h0 = start_state("float64", SIZE, cols)
    w, h = pair(gpu, cols, "double")
    with w, h:
        fill(w, h, w0, h0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            w.updateRowsAdagradRowwise(h, rows, g, LR, EPS)
        assert ei.value.record == 7
        assert_bits(w.to_numpy(), w0)  # a rejected message changes neither shard
        assert_bits(h.to_numpy(), h0)


def test_rowwise_push_errors_device(gpu):
    cols, rows, g = _error_input()
    w0, h0 = start_state("float64", SIZE, cols)
    keep = np.ones(100, bool)
    keep[[7, 60]] = False
    want_w, want_h = replay_rowwise(w0, h0, rows[keep] - START, g[keep], LR, EPS)
    w, h = pair(gpu, cols, "double")
    with w, h:
        fill(w, h, w0, h0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push(w, h, gpu, rows, g, "dev")
        assert ei.value.record == 7
        h.sync()  # the state shard was marked too; it has no error of its own
        assert_bits(w.to_numpy(), want_w)  # the other 98 records were applied
        assert_bits(h.to_numpy(), want_h)


def test_rowwise_push_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    g = np.ones(4, np.float64)
    rd, gd = torch.from_numpy(r).to(d), torch.from_numpy(g).to(d)
    host = lib.glint_mat_push_rows_adagrad_rowwise
    devc = lambda *args: lib.glint_mat_push_rows_adagrad_rowwise_dev(*args, None)  # noqa: E731
    calls = ((host, r.ctypes.data, g.ctypes.data), (devc, rd.data_ptr(), gd.data_ptr()))
    part = RangePartition(0, START, START + 10)
    w, h = pair(gpu, 4, "double", "range", 10)
    with w, h:
        others = {
            "matrix": PartialMatrix(part, 4, "double", gpu),  # a state that is a matrix
            "matrix1": PartialMatrix(part, 1, "double", gpu),
            "size": PartialVector(RangePartition(0, START, START + 11), "double", gpu),
            "dtype": PartialVector(part, "float", gpu),
            "start": PartialVector(RangePartition(0, START + 1, START + 11), "double", gpu),
            "kind": PartialVector(CyclicPartition(0, 2, 20), "double", gpu),  # a cyclic state, range weights
            "int": PartialMatrix(part, 4, "int", gpu), "intv": PartialVector(part, "int", gpu),
            "long": PartialMatrix(part, 4, "long", gpu), "longv": PartialVector(part, "long", gpu),
            "vector2": PartialVector(part, "double", gpu),
        }
        cyc = PartialMatrix(CyclicPartition(0, 2, 20), 4, "double", gpu)
        cycv = [PartialVector(CyclicPartition(i, 2, 20), "double", gpu) for i in (0, 1)]
        assert cyc.size == cycv[0].size == cycv[1].size == others["kind"].size == 10
        try:
            for call, pr, pg in calls:
                def ok(a, b, n=1, rows=pr, grads=pg, lr=0.1, eps=0.0, call=call):
                    return call(a, b, rows, grads, n, lr, eps)

                assert ok(None, h.handle) == N.GLINT_EINVAL
                assert ok(w.handle, None) == N.GLINT_EINVAL
                assert ok(w.handle, w.handle) == N.GLINT_EINVAL  # state is weights
                for name in ("matrix", "matrix1", "size", "dtype", "start", "kind"):
                    assert ok(w.handle, others[name].handle) == N.GLINT_EINVAL, name
                assert ok(cyc.handle, cycv[1].handle) == N.GLINT_EINVAL  # another cyclic index
                assert ok(cyc.handle, h.handle) == N.GLINT_EINVAL        # a range state, cyclic weights
                assert ok(h.handle, others["vector2"].handle) == N.GLINT_EINVAL  # weights is a vector
                for name in ("int", "long"):
                    assert ok(others[name].handle, others[name + "v"].handle) == N.GLINT_EINVAL, name
                assert ok(w.handle, h.handle, n=-1) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, n=(1 << 32) - 2048) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, rows=None) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, grads=None) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, lr=float("nan")) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, eps=-1e-300) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, eps=float("nan")) == N.GLINT_EINVAL
                assert ok(w.handle, h.handle, n=0, rows=None, grads=None) == N.GLINT_OK
            assert not w.to_numpy().any() and not h.to_numpy().any()
            # the Python layer: types, then shapes, before any call
            with pytest.raises(TypeError):
                others["int"].updateRowsAdagradRowwise(others["intv"], r, np.ones(4, np.int32), 0.1)
            with pytest.raises(TypeError):
                w.updateRowsAdagradRowwise(others["matrix"], r, g, 0.1)  # state is a PartialVector
            with pytest.raises(TypeError):
                w.updateRowsAdagradRowwise(h.handle, r, g, 0.1)
            with pytest.raises(TypeError):
                w.updateRowsAdagradRowwise(h, rd, g, 0.1)  # grads on the host
            with pytest.raises(TypeError):
                w.updateRowsAdagradRowwise(h, r, gd, 0.1)  # rows on the host
            with pytest.raises(TypeError):
                w.updateRowsAdagradRowwise(h, rd, gd.to(torch.float32), 0.1)
            for bad in (np.ones(3), np.ones((2, 4)), np.ones(5)):
                with pytest.raises(ValueError):
                    w.updateRowsAdagradRowwise(h, r, bad, 0.1)
            with pytest.raises(ValueError):
                w.updateRowsAdagradRowwise(h, rd, torch.ones(5, dtype=torch.float64, device=d), 0.1)
            assert not w.to_numpy().any() and not h.to_numpy().any()
            # and what is valid: the default eps, a cyclic pair
            assert w.updateRowsAdagradRowwise(h, r, g, 0.5) and w.updateRowsAdagradRowwise(h, rd, gd, 0.5)
            zw, zh = np.zeros((10, 4)), np.zeros(10)
            want = replay_rowwise(*replay_rowwise(zw, zh, [0], g[None], 0.5, 1e-10), [0], g[None], 0.5, 1e-10)
            assert_bits(w.to_numpy(), want[0])
            assert_bits(h.to_numpy(), want[1])
            assert cyc.updateRowsAdagradRowwise(cycv[0], np.array([6], np.int64), g, 0.5, 0.0)  # local row 3
            want = replay_rowwise(zw, zh, [3], g[None], 0.5, 0.0)
            assert_bits(cyc.to_numpy(), want[0])
            assert_bits(cycv[0].to_numpy(), want[1])
        finally:
            for sh in list(others.values()) + [cyc] + cycv:
                sh.destroy()


def test_rowwise_push_slabs_with_views(gpu):
    """A slab that has views is refused as weights and as state, on both paths; views of two slabs work."""
    import torch
    lib = N.load()
    cols = 32  # a row is 256 B: every row offset is a valid view offset
    d = torch.device("cuda", gpu)
    r = np.array([START + 3, START + 3, START + 9], np.int64)
    g = np.random.default_rng(2).standard_normal((3, cols))
    rd, gd = torch.from_numpy(r).to(d), torch.from_numpy(g).to(d)
    whole = RangePartition(0, START, START + 64)
    wslab, hslab = PartialMatrix(whole, cols, "double", gpu), PartialVector(whole, "double", gpu)
    wfree, hfree = PartialMatrix(whole, cols, "double", gpu), PartialVector(whole, "double", gpu)
    first = RangePartition(1, START, START + 32)
    wview, hview = PartialMatrix.view(wslab, first, 0), PartialVector.view(hslab, first, 32)  # 32 doubles = 256 B
    try:
        for a, b in ((wslab, hfree), (wfree, hslab)):
            assert lib.glint_mat_push_rows_adagrad_rowwise(a.handle, b.handle, r.ctypes.data, g.ctypes.data, 3, 0.1,
                                                           0.0) == N.GLINT_EINVAL
            assert lib.glint_mat_push_rows_adagrad_rowwise_dev(a.handle, b.handle, rd.data_ptr(), gd.data_ptr(), 3,
                                                               0.1, 0.0, None) == N.GLINT_EINVAL
        assert wfree.updateRowsAdagradRowwise(hfree, r, g, LR, EPS)  # (the same pair without views is fine)
        assert not wview.to_numpy().any() and not hview.to_numpy().any()
        assert wview.updateRowsAdagradRowwise(hview, r, g, LR, EPS)
        assert wview.updateRowsAdagradRowwise(hview, rd, gd, LR, EPS)
        want_w, want_h = np.zeros((32, cols)), np.zeros(32)
        for _ in range(2):
            want_w, want_h = replay_rowwise(want_w, want_h, r - START, g, LR, EPS)
        assert_bits(wview.to_numpy(), want_w)
        assert_bits(hview.to_numpy(), want_h)
    finally:
        for v in (wview, hview):
            v.destroy()
        for s in (wslab, hslab, wfree, hfree):
            s.destroy()


# ---- ordering across the two shards -----------------------------------------------------------------------
def _ordering_input(cols):
    rng = np.random.default_rng(12)
    ek = rng.integers(START, START + 200, 1000).astype(np.int64)
    ev = rng.integers(1, 50, 1000).astype(np.float64)  # small integers: their sums are exact in any order
    rows = rng.integers(START, START + 200, 900).astype(np.int64)
    g = adagrad_inputs("float64", 900, cols, "rowwise/ordering")
    h1 = np.zeros(SIZE)
    np.add.at(h1, ek - START, ev)
    zero = np.zeros((SIZE, cols))
    want_w, want_h = replay_rowwise(zero, h1, rows - START, g, LR, EPS)
    assert (bits(want_w) != bits(replay_rowwise(zero, np.zeros(SIZE), rows - START, g, LR, EPS)[0])).mean() > 0.05
    return ek, ev, rows, g, want_w, want_h  # (the state push shows in the weights)


def test_rowwise_push_after_unwaited_state_push_host(gpu):
    """A message-sized push into the state vector, staged and not waited for, then the host push: the step
    reads the state after that push."""
    cols = 9
    ek, ev, rows, g, want_w, want_h = _ordering_input(cols)
    w, h = pair(gpu, cols, "double")
    with w, h:
        ticket = h.push_async(ek, ev)
        assert w.updateRowsAdagradRowwise(h, rows, g, LR, EPS)
        q = np.arange(START, START + SIZE, dtype=np.int64)
        got_h, got_w = h.get(q), w.getRows(q)
        h.wait(ticket)
        assert_bits(np.asarray(got_h), want_h, "state")
        assert_bits(np.asarray(got_w), want_w, "weights")


def test_rowwise_push_stream_order(gpu):
    """A device push into the state vector, two pushes and the pulls of both shards on one stream, one sync
    per shard at the end: the second push steps from the first one's accumulators."""
    import torch
    cols = 9
    ek, ev, rows, g, want_w, want_h = _ordering_input(cols)
    rng = np.random.default_rng(22)
    r2 = rng.integers(START + 100, START + 300, 700).astype(np.int64)
    g2 = adagrad_inputs("float64", 700, cols, "rowwise/stream2")
    want_w2, want_h2 = replay_rowwise(want_w, want_h, r2 - START, g2, LR, EPS)
    both = np.intersect1d(rows, r2) - START
    assert both.size > 20 and (want_h2[both] > want_h[both]).all()  # h accumulates over the two pushes
    q = np.arange(START, START + SIZE, dtype=np.int64)
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    w, h = pair(gpu, cols, "double")
    with w, h:
        dev = [t(a) for a in (ek, ev, rows, g, r2, g2, q)]
        h.update(dev[0], dev[1], sync=False)
        w.updateRowsAdagradRowwise(h, dev[2], dev[3], LR, EPS, sync=False)
        mid_w, mid_h = w.getRows(dev[6], sync=False), h.get(dev[6], sync=False)
        w.updateRowsAdagradRowwise(h, dev[4], dev[5], LR, EPS, sync=False)
        out_w, out_h = w.getRows(dev[6], sync=False), h.get(dev[6], sync=False)
        w.sync(w._stream_of(dev[6]))
        h.sync(h._stream_of(dev[6]))
        assert_bits(mid_w.cpu().numpy(), want_w, "weights after the first push")
        assert_bits(mid_h.cpu().numpy(), want_h, "state after the first push")
        assert_bits(out_w.cpu().numpy(), want_w2, "weights")
        assert_bits(out_h.cpu().numpy(), want_h2, "state")


# ---- launch count, client -----------------------------------------------------------------------------------
def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_rowwise_push_profiling_id(gpu):
    rows = np.arange(START, START + 100, dtype=np.int64)
    w, h = pair(gpu, 4, "double")
    with w, h:
        for sh in (w, h):
            assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        counts = lambda: (_launches(w, N.GLINT_K_PUSH_ROWS), _launches(h, N.GLINT_K_PUSH_ROWS),  # noqa: E731
                          _launches(w, N.GLINT_K_PUSH_ROWS_AXPY), _launches(h, N.GLINT_K_PUSH_ROWS_AXPY))
        assert counts() == (0, 0, 0, 0)
        push(w, h, gpu, np.repeat(rows, 3), np.ones((300, 4)), "host")
        assert counts() == (1, 0, 0, 0)  # one fold launch, on the weights shard
        push(w, h, gpu, rows, np.ones((100, 4)), "dev")
        assert counts() == (2, 0, 0, 0)
        push(w, h, gpu, rows[:0], np.ones((0, 4)), "host")  # an empty call launches nothing
        push(w, h, gpu, rows[:0], np.ones((0, 4)), "dev")
        assert counts() == (2, 0, 0, 0)
        for sh in (w, h):
            assert sum(_launches(sh, k) for k in range(N.GLINT_K_COUNT)) == (2 if sh is w else 0)


@pytest.mark.parametrize("make", [RangePartitioner.apply, CyclicPartitioner.apply], ids=KINDS)
def test_rowwise_push_client(gpu, make):
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 400, 3000).astype(np.int64)
    g = adagrad_inputs("float64", 3000, 7, "rowwise/client")
    c = Client([gpu] * 3)
    m = c.matrix(400, 7, "double", modelsPerServer=1, createPartitioner=make)
    st = c.vector(400, "double", modelsPerServer=1, createPartitioner=make)
    wrong = c.vector(401, "double", modelsPerServer=1, createPartitioner=make)
    try:
        assert m.nrOfPartitions == st.nrOfPartitions == 3
        with pytest.raises(ValueError):
            m.pushAdagradRowwise(wrong, rows, g, LR)
        want_w, want_h = np.zeros((400, 7)), np.zeros(400)
        for _ in range(2):
            assert m.pushAdagradRowwise(st, rows, g, LR, EPS)
            want_w, want_h = replay_rowwise(want_w, want_h, rows, g, LR, EPS)
        assert_bits(m.pull(np.arange(400)), want_w, "weights")
        assert_bits(st.pull(np.arange(400)), want_h, "state")
    finally:
        for x in (m, st, wrong):
            x.destroy()
