"""FTRL-proximal row push (PartialMatrix.updateRowsFtrl, glint_mat_push_rows_ftrl*) against the replay.

The call is deterministic on every path -- no run is split, no atomic -- so the bar is one: both shards
equal ftrl_cases.replay_ftrl bit for bit (a NaN by class), on the host and on the device path, and the pitch
padding of both keeps the value it was given. The premises of the constructed inputs are asserted from the
replay alone in test_ftrl_cpu.py.
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
from ftrl_cases import (ALPHA, ALTS, BETA, L1, L2, SIZE, SWEEP_COLS, TH_L1, TH_L2, assert_bits, bits,
                        duplicates_push, ftrl_grads, ftrl_scalars, ftrl_start, ftrl_step, ftrl_sweep_inputs,
                        fusion_inputs, replay_ftrl, sweep_premises, sweep_scalars, threshold_inputs)
from ieee_cases import write_image

pytestmark = pytest.mark.gpu
DT = ["double", "float"]
START = 1_000_003
RUNS = (15, 16, 17, 63, 64, 65)  # around the loads in flight (16) and the record ids per batch (64)
PATTERNS = ["sorted_once", "permutation", "duplicates", "one_row", "single", "empty"]
REPEATS = ("duplicates", "one_row")
PATHS = ["host", "dev"]
K = (ALPHA, BETA, L1, L2)
PAD = 777.0


def npd_of(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def make_local(rng, pattern):
    if pattern == "sorted_once":
        return np.arange(SIZE, dtype=np.int64)
    if pattern == "permutation":
        return rng.permutation(SIZE).astype(np.int64)
    if pattern == "duplicates":
        return rng.choice(rng.choice(SIZE, 12, replace=False), 300).astype(np.int64)
    if pattern == "one_row":  # crosses the sort's 2048-key tile, the 64-id batch and the depth
        return np.full(2100, 31, np.int64)
    if pattern == "runs":  # one row per length of RUNS, their records interleaved
        return rng.permutation(np.repeat(np.arange(len(RUNS)) * 7 + 3, RUNS)).astype(np.int64)
    if pattern == "single":
        return np.array([17], np.int64)
    return np.zeros(0, np.int64)


def pair(gpu, cols, dtype, size=SIZE, part=None):
    """(weights, state): the state shard has 2 * cols columns."""
    part = part or RangePartition(2, START, START + size)
    return PartialMatrix(part, cols, dtype, gpu), PartialMatrix(part, 2 * cols, dtype, gpu)


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


def load(w, s, gpu, w0, s0):
    """Both tables into the shards' memory as it lies, the pitch padding set to PAD."""
    write_image(w, gpu, np.array(w0), w0.dtype.type(PAD))
    write_image(s, gpu, np.array(s0), s0.dtype.type(PAD))


def check(w, s, gpu, want_w, want_s):
    """Both shards against the replay, bit for bit, and the padding of both untouched. Returns the images."""
    out = []
    for sh, want, what in ((s, want_s, "state"), (w, want_w, "weights")):
        raw = read_image(sh, gpu, want.shape[0])
        assert_bits(raw[:, :want.shape[1]], want, what)
        assert (raw[:, want.shape[1]:] == PAD).all(), f"{what}: the pitch padding was written"
        out.append(raw)
    return out


def push(w, s, gpu, rows, g, path, k=K, sync=True):
    if path == "host":
        assert w.updateRowsFtrl(s, rows, g, *k)
        return
    import torch
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    assert w.updateRowsFtrl(s, t(rows), t(g), *k, sync=sync)


@functools.lru_cache(maxsize=None)
def case(dtype, cols, pattern):
    """(local rows, grads, weights and state after two pushes from ftrl_start): computed once and shared by
    the paths; read-only. The `duplicates` case at cols 67 is ftrl_cases.duplicates_push, whose premises
    test_ftrl_cpu.py asserts."""
    name = np.dtype(npd_of(dtype)).name
    if pattern == "duplicates":
        _, _, local, g = duplicates_push(name, cols)
    else:
        rng = np.random.default_rng(zlib.crc32(f"ftrl/{dtype}/{cols}/{pattern}".encode()))
        local = make_local(rng, pattern)
        g = ftrl_grads(name, local.size, cols)
    w, s = ftrl_start(name, SIZE, cols)
    for _ in range(2):
        w, s = replay_ftrl(w, s, local, g, *K)
    for a in (local, w, s):
        a.setflags(write=False)
    return local, g, w, s


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
def test_ftrl_push_parity(gpu, dtype, cols, pattern, path):
    local, g, want_w, want_s = case(dtype, cols, pattern)
    if pattern == "runs":
        assert sorted(np.unique(local, return_counts=True)[1].tolist()) == list(RUNS)
    w0, s0 = ftrl_start(np.dtype(npd_of(dtype)).name, SIZE, cols)
    w, s = pair(gpu, cols, dtype)
    with w, s:
        load(w, s, gpu, w0, s0)
        for _ in range(2):  # the second push steps from the first one's state
            push(w, s, gpu, local + START, g, path)
        check(w, s, gpu, want_w, want_s)


# ---- the threshold: exact zeros, and what a sparse pull then moves -----------------------------------------
def _same_triple(got, want):
    for a, b in zip(got[:2], want[:2]):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
    np.testing.assert_array_equal(bits(np.asarray(got[2])), bits(np.asarray(want[2])))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols", [(dt, c) for dt in DT for c in (3, 128)])
def test_ftrl_threshold_zeros(gpu, dtype, cols, path):
    """ftrl_cases.threshold_inputs with l1 = TH_L1: |z'| on both sides of l1 and exactly on it, z' of both
    signs. The exact zeros are the replay's, and a sparse pull of the rows returns what a sparse pull of a
    shard holding the replay's weights returns. With l1 = l2 = 0 the same push leaves the replay's zeros
    only."""
    npd = npd_of(dtype)
    w0, s0, local, g = threshold_inputs(np.dtype(npd).name, SIZE, cols)
    q = np.arange(START, START + SIZE, dtype=np.int64)
    for l1, l2 in ((TH_L1, TH_L2), (0.0, 0.0)):
        want_w, want_s = replay_ftrl(w0, s0, local, g, ALPHA, BETA, l1, l2)
        zeros = int((bits(want_w) == 0).sum())
        assert (zeros > cols) == (l1 > 0)  # a third of the table, or none but what z' == 0 gives
        w, s = pair(gpu, cols, dtype)
        ref = PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu)
        with w, s, ref:
            load(w, s, gpu, w0, s0)
            push(w, s, gpu, local + START, g, path, (ALPHA, BETA, l1, l2))
            got_w = check(w, s, gpu, want_w, want_s)[1][:, :cols]
            np.testing.assert_array_equal(bits(got_w) == 0, bits(want_w) == 0)  # +0 where the replay has +0
            assert int((got_w == 0).sum()) == zeros  # and no -0 anywhere else
            write_image(ref, gpu, want_w, npd(PAD))
            got, want = w.getRowsSparse(q), ref.getRowsSparse(q)
            _same_triple(got, want)
            assert int(np.asarray(got[0])[-1]) == SIZE * cols - zeros  # the zeros do not cross the link


# ---- the two halves of a state row ----------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols", [(dt, c) for dt in DT for c in (3, 128)])
def test_ftrl_halves(gpu, dtype, cols, path):
    """z negative and n huge: a swap of the halves, or an n half read at another offset (at cols 3 it starts
    at no multiple of 16 B), would show in every element. Rows that are not named keep both halves."""
    npd = npd_of(dtype)
    rng = np.random.default_rng(zlib.crc32(f"ftrl/halves/{dtype}/{cols}".encode()))
    w0 = rng.standard_normal((SIZE, cols)).astype(npd)
    z0 = -(1.0 + rng.random((SIZE, cols))).astype(npd)
    n0 = ((1.0 + rng.random((SIZE, cols))) * 2.0 ** 40).astype(npd)
    s0 = np.concatenate([z0, n0], 1)
    local = rng.permutation(SIZE)[:30].astype(np.int64)
    g = rng.standard_normal((30, cols)).astype(npd)
    want_w, want_s = replay_ftrl(w0, s0, local, g, *K)
    swapped = replay_ftrl(w0, np.concatenate([n0, z0], 1), local, g, *K)
    assert (bits(swapped[1][local]) != bits(want_s[local])).all()  # the premise: the halves are told apart
    rest = np.setdiff1d(np.arange(SIZE), local)
    assert rest.size == SIZE - 30 and (bits(want_s[rest]) == bits(s0[rest])).all()
    w, s = pair(gpu, cols, dtype)
    with w, s:
        load(w, s, gpu, w0, s0)
        push(w, s, gpu, local + START, g, path)
        check(w, s, gpu, want_w, want_s)


# ---- correctly rounded sqrt and divide, subnormals kept ----------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("tiny_l1", [False, True])
@pytest.mark.parametrize("aligned", [True, False], ids=["16B", "scalar"])
@pytest.mark.parametrize("dtype", DT)
def test_ftrl_rounding_sweep(gpu, dtype, aligned, tiny_l1, path):
    """One push, every row once, cols 128: n over the type's whole exponent range, G over the Adagrad spans
    and the band near the square root of the smallest normal, z with a band of subnormals
    (ftrl_cases.ftrl_sweep_inputs). A fast sqrt or divide, or flushed subnormals, would show here. On the
    device path the gradients sit 16-B aligned (the 16-B slices) or one element off (the scalar slices);
    the host path stages them aligned, so it takes the sweep at cols 128 (16 B) and, for the scalar
    slices, the first 127 columns."""
    import torch
    npd = npd_of(dtype)
    cols = SWEEP_COLS if (aligned or path == "dev") else SWEEP_COLS - 1
    w0, z0, n0, G = (a[:, :cols] for a in ftrl_sweep_inputs(np.dtype(npd).name, SIZE, SWEEP_COLS))
    kd = sweep_scalars(npd, tiny_l1)
    k = ftrl_scalars(npd, *kd)
    got = sweep_premises(npd, w0, z0, n0, G, k)
    print(f"{dtype} cols {cols} tiny_l1 {tiny_l1}: {got}")
    assert min(got.values()) >= 1, got
    want_w, want_z, want_n = ftrl_step(w0, z0, n0, G, k)
    local = np.random.default_rng(4).permutation(SIZE).astype(np.int64)
    w, s = pair(gpu, cols, dtype)
    with w, s:
        load(w, s, gpu, w0, np.concatenate([z0, n0], 1))
        if path == "host":
            push(w, s, gpu, local + START, G[local], path, kd)
        else:
            d = torch.device("cuda", gpu)
            off = 0 if aligned else 1
            buf = torch.zeros(local.size * cols + 4, dtype=w.torch_dtype, device=d)
            v = buf[off:off + local.size * cols]
            v.copy_(torch.from_numpy(np.ascontiguousarray(G[local])).to(d).view(-1))
            assert v.data_ptr() % 16 == off * v.element_size()
            assert w.updateRowsFtrl(s, torch.from_numpy(local + START).to(d), v, *kd)
        check(w, s, gpu, want_w, np.concatenate([want_z, want_n], 1))


# ---- no fused multiply-add ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("run", [1, 3])
@pytest.mark.parametrize("dtype,cols", [("double", 2), ("double", 67), ("float", 4), ("float", 67)])
def test_ftrl_is_unfused(gpu, dtype, cols, run, path):
    """ftrl_cases.fusion_inputs: G - sg * w cancels and n + G * G rounds twice, so a product that was not
    rounded before its add shows. As a single record per row, and as the middle record of a run of three
    for the row (the others zero). cols 2 (Double) and 4 (Float) take the 16-B slice, 67 the scalar one."""
    npd = npd_of(dtype)
    G, wf, z, n = fusion_inputs(npd)
    R = min(G.size // cols, SIZE)
    G, wf, z, n = (a[:R * cols].reshape(R, cols) for a in (G, wf, z, n))
    w0, s0 = np.zeros((SIZE, cols), npd), np.zeros((SIZE, 2 * cols), npd)
    w0[:R] = wf
    s0[:R] = np.concatenate([z, n], 1)
    local = np.arange(R, dtype=np.int64)
    if run == 1:
        rows, g = local, G
    else:
        rows = np.concatenate([local, local, local])
        g = np.concatenate([np.zeros_like(G), G, np.zeros_like(G)])
    want_w, want_s = replay_ftrl(w0, s0, rows, g, *K)
    w, s = pair(gpu, cols, dtype)
    with w, s:
        load(w, s, gpu, w0, s0)
        push(w, s, gpu, rows + START, g, path)
        got = read_image(s, gpu, SIZE)[:, :2 * cols]
        if (bits(got) != bits(want_s)).any():
            match = [alt for alt in ALTS if (bits(got) == bits(replay_ftrl(w0, s0, rows, g, *K, alt=alt)[1])).all()]
            pytest.fail(f"the state is not the contract's; ruled-out forms its bits match: {match or 'none'}")
        check(w, s, gpu, want_w, want_s)


# ---- the bits do not depend on the alignment of grads, the path or the partition kind ---------------------
@pytest.mark.parametrize("dtype", DT)
def test_ftrl_path_independence(gpu, dtype):
    """The same local rows and gradients into a range shard and a cyclic shard, from the host, from a 16-B
    aligned device buffer (the 16-B slices at cols 128) and from one that is one element off (the scalar
    slices): six results, one set of bits."""
    import torch
    cols = 128
    local, g, _, _ = case(dtype, cols, "duplicates")
    name = np.dtype(npd_of(dtype)).name
    w0, s0 = ftrl_start(name, SIZE, cols)
    want_w, want_s = replay_ftrl(w0, s0, local, g, *K)
    d = torch.device("cuda", gpu)
    cyc = CyclicPartition(1, 3, 3 * SIZE)
    parts = {"range": (None, local + START), "cyclic": (cyc, 1 + 3 * local)}
    images = []
    for kind, (part, rows) in parts.items():
        for place in ("host", 0, 1):
            w, s = pair(gpu, cols, dtype, part=part)
            with w, s:
                assert w.size == SIZE
                load(w, s, gpu, w0, s0)
                if place == "host":
                    assert w.updateRowsFtrl(s, rows, g, *K)
                else:
                    buf = torch.zeros(g.size + 4, dtype=w.torch_dtype, device=d)
                    v = buf[place:place + g.size]
                    v.copy_(torch.from_numpy(np.array(g)).to(d).view(-1))
                    assert v.data_ptr() % 16 == place * v.element_size() and v.is_contiguous()
                    assert w.updateRowsFtrl(s, torch.from_numpy(rows).to(d), v, *K)
                images.append(check(w, s, gpu, want_w, want_s))
    assert len(images) == 6
    for si, wi in images[1:]:
        np.testing.assert_array_equal(bits(si), bits(images[0][0]))
        np.testing.assert_array_equal(bits(wi), bits(images[0][1]))


# ---- IEEE edges and padding -----------------------------------------------------------------------------
@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("l1", [0.0, 0.25])
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("double", 6), ("float", 67), ("float", 12)])
def test_ftrl_ieee_edges(gpu, dtype, cols, l1, path):
    """NaN and infinite gradients, an overflowing G * G, n at the type's maximum, a subnormal z, beta = 0
    and l2 = 0 with G = 0 (d = 0: an infinite w' past the threshold, +0 inside it), an unnamed row's bits and
    the pitch padding of both shards; each against the replay, a NaN by class."""
    npd = npd_of(dtype)
    info = np.finfo(npd)
    big = npd(1e200 if dtype == "double" else 1e30)
    nan_bits = 0x7FF8000000000123 if dtype == "double" else 0x7FC00123
    payload = np.array([nan_bits], np.uint64 if dtype == "double" else np.uint32).view(npd)[0]
    sub = npd(info.smallest_subnormal * 5)
    R = 10
    w0 = np.full((R, cols), 1.5, npd)
    w0[:, 0::2] = 0
    z0, n0 = np.full((R, cols), 2.0, npd), np.ones((R, cols), npd)
    z0[0], n0[0] = 0, 0                         # row 0: G = 0, z = 0, n = 0: |z'| = 0 <= l1, w' = +0
    n0[4] = info.max                            # row 4: n at the maximum, q = 1: n' = n, ds = 0
    z0[5, 0::2], z0[5, 1::2], w0[5] = sub, -sub, 0  # row 5: z' = z subnormal; e = z' / 2 is subnormal too
    z0[6, 0::2], z0[6, 1::2], n0[6] = 2.0, -2.0, 0  # row 6: n' = 0, beta = l2 = 0: d = 0, w' = -+inf
    s0 = np.concatenate([z0, n0], 1)
    for t in (w0, s0):  # row 7 is not named: its bits stay, whatever they are
        t[7, 0::2], t[7, 1::2] = -0.0, payload
    local = np.array([0, 1, 2, 3, 4, 3, 5, 6, 8], np.int64)
    g = np.zeros((9, cols), npd)
    g[1] = np.inf                # row 1: n', sg infinite; t = inf * 0 where w = 0
    g[2, 0::2], g[2, 1::2] = np.nan, -np.inf
    g[3], g[5] = big, big / 4    # row 3 twice: G = 1.25 big, G * G overflows
    g[4] = 1.0
    g[8] = 1.0                   # row 8: an ordinary step next to them
    kd = (0.5, 0.0, l1, 0.0)
    want_w, want_s = replay_ftrl(w0, s0, local, g, *kd)
    # the premises, from the replay
    assert (bits(want_w[0]) == 0).all() and (want_s[0] == 0).all()
    assert np.isinf(want_s[1, cols:]).all() and np.isnan(want_w[1]).all() and np.isnan(want_s[1, :cols]).all()
    assert (want_s[2, 1:cols:2] == -np.inf).all() and np.isnan(want_w[2, 1::2]).all()  # y / d = inf / inf
    assert np.isnan(want_w[2, 0::2]).all() and np.isnan(want_s[2, 0:cols:2]).all() and np.isnan(want_s[2, cols::2]).all()
    assert np.isinf(want_s[3, cols:]).all()
    assert (want_s[4, cols:] == info.max).all() and (want_s[4, :cols] == 3.0).all() and np.isfinite(want_w[4]).all()
    assert (bits(want_s[5, :cols]) == bits(z0[5])).all()
    if l1 == 0:
        assert ((want_w[5] != 0) & (np.abs(want_w[5]) < info.tiny)).all()  # subnormal weights, kept
    else:
        assert (bits(want_w[5]) == 0).all()
    assert np.isinf(want_w[6]).all() and (want_w[6, 0::2] < 0).all() and (want_w[6, 1::2] > 0).all()
    assert np.isfinite(want_w[8]).all() and (want_w[8] != w0[8]).all()
    for t, t0 in ((want_w, w0), (want_s, s0)):
        assert (bits(t[[7, 9]]) == bits(t0[[7, 9]])).all()
    w, s = pair(gpu, cols, dtype, R)
    with w, s:
        load(w, s, gpu, w0, s0)
        push(w, s, gpu, local + START, g, path, kd)
        imgs = check(w, s, gpu, want_w, want_s)
        np.testing.assert_array_equal(bits(imgs[1][[7, 9], :cols]), bits(w0[[7, 9]]))  # payload and sign kept
        np.testing.assert_array_equal(bits(imgs[0][[7, 9], :2 * cols]), bits(s0[[7, 9]]))
        padded = sum(img.shape[1] > width for img, width in zip(imgs, (2 * cols, cols)))
        assert padded == {("double", 67): 1, ("float", 67): 2}.get((dtype, cols), 0)  # a row of 16 B multiples has none


# ---- errors and arguments -------------------------------------------------------------------------------
def _error_input():
    rng = np.random.default_rng(3)
    cols = 6
    rows = rng.integers(START, START + SIZE, 100).astype(np.int64)
    rows[7] = START - 1
    rows[60] = START + SIZE
    return cols, rows, rng.standard_normal((100, cols))


def test_ftrl_push_errors_host(gpu):
    cols, rows, g = _error_input()
    w0, s0 = ftrl_start("float64", SIZE, cols)
    w, s = pair(gpu, cols, "double")
    with w, s:
        load(w, s, gpu, w0, s0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            w.updateRowsFtrl(s, rows, g, *K)
        assert ei.value.record == 7
        check(w, s, gpu, w0, s0)  # a rejected message changes neither shard


def test_ftrl_push_errors_device(gpu):
    cols, rows, g = _error_input()
    w0, s0 = ftrl_start("float64", SIZE, cols)
    keep = np.ones(100, bool)
    keep[[7, 60]] = False
    want_w, want_s = replay_ftrl(w0, s0, rows[keep] - START, g[keep], *K)
    w, s = pair(gpu, cols, "double")
    with w, s:
        load(w, s, gpu, w0, s0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push(w, s, gpu, rows, g, "dev")
        assert ei.value.record == 7
        s.sync()  # the state shard was marked too; it has no error of its own
        check(w, s, gpu, want_w, want_s)  # the other 98 records were applied


def test_ftrl_push_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    g = np.ones(4, np.float64)
    rd, gd = torch.from_numpy(r).to(d), torch.from_numpy(g).to(d)
    host = lib.glint_mat_push_rows_ftrl
    devc = lambda *args: lib.glint_mat_push_rows_ftrl_dev(*args, None)  # noqa: E731
    calls = ((host, r.ctypes.data, g.ctypes.data), (devc, rd.data_ptr(), gd.data_ptr()))
    part = RangePartition(0, START, START + 10)
    nan, inf = float("nan"), float("inf")
    w, s = pair(gpu, 4, "double", part=part)
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
                def ok(a, b, n=1, rows=pr, grads=pg, alpha=0.1, beta=1.0, l1=0.0, l2=0.0, call=call):
                    return call(a, b, rows, grads, n, alpha, beta, l1, l2)

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
                for bad in (0.0, -0.0, -0.1, nan, inf, -inf):
                    assert ok(w.handle, s.handle, alpha=bad) == N.GLINT_EINVAL, bad
                for bad in (-1e-300, -1.0, nan, inf, -inf):
                    assert ok(w.handle, s.handle, beta=bad) == N.GLINT_EINVAL, bad
                    assert ok(w.handle, s.handle, l1=bad) == N.GLINT_EINVAL, bad
                    assert ok(w.handle, s.handle, l2=bad) == N.GLINT_EINVAL, bad
                assert ok(w.handle, s.handle, n=0, rows=None, grads=None) == N.GLINT_OK
            assert not w.to_numpy().any() and not s.to_numpy().any()
            # the Python layer: types, then shapes, before any call
            with pytest.raises(TypeError):
                others["int"].updateRowsFtrl(others["int2"], r, np.ones(4, np.int32), 0.1)
            with pytest.raises(TypeError):
                others["long"].updateRowsFtrl(others["long2"], r, np.ones(4, np.int64), 0.1)
            with pytest.raises(TypeError):
                w.updateRowsFtrl(s.handle, r, g, 0.1)  # state is a PartialMatrix
            with pytest.raises(TypeError):
                w.updateRowsFtrl(s, rd, g, 0.1)  # grads on the host
            with pytest.raises(TypeError):
                w.updateRowsFtrl(s, r, gd, 0.1)  # rows on the host
            with pytest.raises(TypeError):
                w.updateRowsFtrl(s, rd, gd.to(torch.float32), 0.1)
            for bad in (np.ones(3), np.ones((2, 4)), np.ones(5), np.ones(8)):
                with pytest.raises(ValueError):
                    w.updateRowsFtrl(s, r, bad, 0.1)
            with pytest.raises(ValueError):
                w.updateRowsFtrl(s, rd, torch.ones(5, dtype=torch.float64, device=d), 0.1)
            assert not w.to_numpy().any() and not s.to_numpy().any()
            # and what is valid: the defaults (beta 1, l1 = l2 = 0), beta = 0, a cyclic pair
            assert w.updateRowsFtrl(s, r, g, 0.5) and w.updateRowsFtrl(s, rd, gd, 0.5)
            zero, zero2 = np.zeros((10, 4)), np.zeros((10, 8))
            want = replay_ftrl(*replay_ftrl(zero, zero2, [0], g[None], 0.5), [0], g[None], 0.5)
            assert want[0][0].all()
            assert_bits(w.to_numpy(), want[0])
            assert_bits(s.to_numpy(), want[1])
            same = PartialMatrix(CyclicPartition(0, 2, 20), 8, "double", gpu)
            with same:
                assert cyc[0].updateRowsFtrl(same, np.array([6], np.int64), g, 0.5, 0.0, 0.5, 0.0)  # local 3
                want = replay_ftrl(zero, zero2, [3], g[None], 0.5, 0.0, 0.5, 0.0)
                assert_bits(cyc[0].to_numpy(), want[0])
                assert_bits(same.to_numpy(), want[1])
        finally:
            for sh in list(others.values()) + cyc:
                sh.destroy()


def test_ftrl_push_slabs_with_views(gpu):
    """A slab that has views is refused as either shard, on both paths; its views hold the slab's cols, so
    two of them never make a weights / state pair. Views of two slabs are a pair."""
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
        for a, b in ((slab, plain_s), (plain_w, slab2), (views[0], views[1])):
            assert lib.glint_mat_push_rows_ftrl(a.handle, b.handle, r.ctypes.data, g.ctypes.data, 1,
                                                *K) == N.GLINT_EINVAL
            assert lib.glint_mat_push_rows_ftrl_dev(a.handle, b.handle, rd.data_ptr(), gd.data_ptr(), 1, *K,
                                                    None) == N.GLINT_EINVAL
        assert not views[0].to_numpy().any() and not views[2].to_numpy().any() and not plain_w.to_numpy().any()
        assert views[0].updateRowsFtrl(views[2], r, g, *K)  # views of two slabs are a pair
        assert views[0].updateRowsFtrl(views[2], rd, gd, *K)
        want = replay_ftrl(np.zeros((5, cols)), np.zeros((5, 2 * cols)), r - START, g[None], *K)
        want = replay_ftrl(*want, r - START, g[None], *K)
        assert_bits(views[0].to_numpy(), want[0])
        assert_bits(views[2].to_numpy(), want[1])
    finally:
        for v in views:
            v.destroy()
        for sh in (slab, slab2, plain_w, plain_s):
            sh.destroy()


# ---- ordering across the two shards -----------------------------------------------------------------------
def _ordering_input(cols):
    rng = np.random.default_rng(12)
    er = rng.integers(START, START + SIZE, 1000).astype(np.int64)
    ec = rng.integers(0, 2 * cols, 1000).astype(np.int32)
    ev = rng.integers(1, 50, 1000).astype(np.float64)  # small integers: their sums are exact in any order
    rows = rng.integers(START, START + SIZE, 400).astype(np.int64)
    g = ftrl_grads("float64", 400, cols, "ordering")
    s1 = np.zeros((SIZE, 2 * cols))
    np.add.at(s1, (er - START, ec), ev)
    zero = np.zeros((SIZE, cols))
    want_w, want_s = replay_ftrl(zero, s1, rows - START, g, *K)
    assert (bits(want_w) != bits(replay_ftrl(zero, np.zeros((SIZE, 2 * cols)), rows - START, g, *K)[0])).mean() \
        > 0.05  # the state push shows in the weights
    return er, ec, ev, rows, g, want_w, want_s


def test_ftrl_push_after_unwaited_state_push_host(gpu):
    """A message-sized push into the state shard, staged and not waited for, then the host FTRL push: the
    step reads the state after that push."""
    cols = 9
    er, ec, ev, rows, g, want_w, want_s = _ordering_input(cols)
    w, s = pair(gpu, cols, "double")
    with w, s:
        ticket = s.push_async(er, ec, ev)
        assert w.updateRowsFtrl(s, rows, g, *K)
        q = np.arange(START, START + SIZE, dtype=np.int64)
        got_s, got_w = s.getRows(q), w.getRows(q)
        s.wait(ticket)
        assert_bits(np.asarray(got_s), want_s, "state")
        assert_bits(np.asarray(got_w), want_w, "weights")


def test_ftrl_push_after_state_push_device(gpu):
    """A device element push into the state shard on a second stream; the FTRL push on the current stream
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
        w.updateRowsFtrl(s, dev[3], dev[4], *K, sync=False)
        w.sync(w._stream_of(dev[3]))
        s.sync(side.cuda_stream)
        s.sync(s._stream_of(dev[3]))  # the stream of the last call that marked it
        assert_bits(s.to_numpy(), want_s, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


def test_ftrl_push_then_pull_on_one_stream(gpu):
    """Two FTRL pushes with sync=False and two row pulls on one stream, one sync per shard at the end."""
    import torch
    cols = 9
    rng = np.random.default_rng(21)
    d = torch.device("cuda", gpu)
    r1, g1 = rng.integers(START, START + 30, 300).astype(np.int64), ftrl_grads("float64", 300, cols, "stream1")
    r2, g2 = rng.integers(START + 15, START + 45, 400).astype(np.int64), ftrl_grads("float64", 400, cols, "stream2")
    q = np.arange(START, START + 45, dtype=np.int64)
    want_w, want_s = replay_ftrl(np.zeros((SIZE, cols)), np.zeros((SIZE, 2 * cols)), r1 - START, g1, *K)
    want_w, want_s = replay_ftrl(want_w, want_s, r2 - START, g2, *K)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    w, s = pair(gpu, cols, "double")
    with w, s:
        dev = [t(a) for a in (r1, g1, r2, g2, q)]
        w.updateRowsFtrl(s, dev[0], dev[1], *K, sync=False)
        w.updateRowsFtrl(s, dev[2], dev[3], *K, sync=False)
        out_w, out_s = w.getRows(dev[4], sync=False), s.getRows(dev[4], sync=False)
        w.sync(w._stream_of(dev[4]))
        s.sync(s._stream_of(dev[4]))
        assert_bits(out_w.cpu().numpy(), want_w[:45], "weights")
        assert_bits(out_s.cpu().numpy(), want_s[:45], "state")


# ---- launch count, client -----------------------------------------------------------------------------------
def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_ftrl_push_profiling_id(gpu):
    rows = np.arange(START, START + SIZE, dtype=np.int64)
    w, s = pair(gpu, 4, "double")
    ref = PartialMatrix(RangePartition(2, START, START + SIZE), 4, "double", gpu)  # a plain row push beside it
    with w, s, ref:
        for sh in (w, s, ref):
            assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        total = lambda sh: sum(_launches(sh, k) for k in range(N.GLINT_K_COUNT))  # noqa: E731
        assert (total(w), total(s), total(ref)) == (0, 0, 0)
        ref.updateRows(np.repeat(rows, 3), np.ones((3 * SIZE, 4)), deterministic=True)
        push(w, s, gpu, np.repeat(rows, 3), np.ones((3 * SIZE, 4)), "host")
        # the front end's launches are not timed, in either call: one fold launch each, under the row push's id
        assert _launches(w, N.GLINT_K_PUSH_ROWS) == _launches(ref, N.GLINT_K_PUSH_ROWS) == 1
        assert total(w) == total(ref) == 1 and total(s) == 0
        push(w, s, gpu, rows, np.ones((SIZE, 4)), "dev")
        assert _launches(w, N.GLINT_K_PUSH_ROWS) == 2 and total(w) == 2 and total(s) == 0
        push(w, s, gpu, rows[:0], np.ones((0, 4)), "host")  # an empty call launches nothing
        push(w, s, gpu, rows[:0], np.ones((0, 4)), "dev")
        assert total(w) == 2 and total(s) == 0


@pytest.mark.parametrize("kind", ["range", "cyclic"])
def test_ftrl_push_client(gpu, kind):
    """Three partitions; the first push names rows of partitions 0 and 2 only, the others all three. The
    tables are compared with the replay as a whole and partition by partition; a sparse pull of the trained
    rows is the sparse pull of the replay's weights."""
    rng = np.random.default_rng(8)
    R, cols = 90, 7
    make = RangePartitioner.apply if kind == "range" else CyclicPartitioner.apply
    c = Client([gpu] * 3)
    m = c.matrix(R, cols, "double", createPartitioner=make)
    st = c.matrix(R, 2 * cols, "double", createPartitioner=make)
    other = c.matrix(R, cols, "double", createPartitioner=make)
    wide = c.matrix(R, 2 * cols + 1, "double", createPartitioner=make)
    flt = c.matrix(R, 2 * cols, "float", createPartitioner=make)
    try:
        assert m.nrOfPartitions == 3
        every = np.arange(R, dtype=np.int64)
        owner = m.partitioner.partition_indices(every)
        rows = rng.integers(0, R, 400).astype(np.int64)
        for bad in (other, wide, flt, st.shards[0], None):
            with pytest.raises(ValueError):
                m.pushFtrl(bad, rows, np.zeros((400, cols)), ALPHA)
        with pytest.raises(ValueError):
            m.pushFtrl(st, rows, np.zeros((400, cols + 1)), ALPHA)
        want_w, want_s = np.zeros((R, cols)), np.zeros((R, 2 * cols))
        k = (ALPHA, BETA, 2000.0, L2)  # gradients over nine decades: an l1 that zeroes about 0.4 of the table
        for step in range(3):
            r = rows[owner[rows] != 1] if step == 0 else rows  # partition 1 is not named by the first push
            assert set(owner[r].tolist()) == ({0, 2} if step == 0 else {0, 1, 2})
            g = ftrl_grads("float64", r.size, cols, f"client{step}")
            assert m.pushFtrl(st, r, g, *k)
            want_w, want_s = replay_ftrl(want_w, want_s, r, g, *k)
            if step == 0:
                assert not m.shards[1].to_numpy().any() and not st.shards[1].to_numpy().any()
        assert m.pushFtrl(st, rows[:0], np.zeros((0, cols)), *k)  # an empty push
        assert_bits(m.pull(every), want_w, "weights")
        assert_bits(st.pull(every), want_s, "state")
        for p, part in enumerate(m.partitioner.all()):
            keys = every[owner == p]
            local = np.array([part.globalToLocal(int(x)) for x in keys])
            assert_bits(m.shards[p].to_numpy()[local], want_w[keys], f"weights of partition {p}")
            assert_bits(st.shards[p].to_numpy()[local], want_s[keys], f"state of partition {p}")
        zeros = int((want_w == 0).sum())
        assert 0.1 * want_w.size < zeros < 0.9 * want_w.size
        other.pushRows(every, want_w)
        got, want = m.pullSparse(every), other.pullSparse(every)
        _same_triple(got, want)
        assert int(np.asarray(got[0])[-1]) == want_w.size - zeros
    finally:
        for x in (m, st, other, wide, flt):
            x.destroy()
