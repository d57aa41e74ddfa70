"""Grouped row push (PartialMatrix.updateRowsGrouped, glint_mat_push_rows_grouped*) on the GPU.

The call is defined as the row push of the contribution rows ``values[group of i]`` (``weights[i] *
values[group of i]``, the product rounded on its own), so the expected values are group_cases.replay_grouped
-- the sequential loop in numpy -- and ``updateRows`` of those rows on a twin shard.

Bar: bit for bit for Int/Long everywhere, for host calls and for deterministic device calls; a row that
occurs once is bit-exact in every mode. Where the order of a repeated row's sum is free (the device default
and ``unordered``), Float/Double are held to test_gpu_axpy.check's bar, with the element the shard held
before the push counted as one of the sum's terms (the shards here start from a non-zero image)."""
import ctypes as C
import functools

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from axpy_cases import assert_bits, nofma_element
from group_cases import (bits, group_coef, group_contrib, group_of, group_records, group_values, replay_grouped)
from ieee_cases import write_image
from rowsum_cases import replay_groups
import test_gpu_axpy as A  # check: the bar of a sum whose order is free; read_image

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
START, SIZE = 1_000_003, 300
CYC = (2, 5, 1498)  # partition 2 of 5 over 1498 keys: 300 rows, key = 2 + 5 * local
PARTS = ["range", "cyclic"]
PAD = 777
# a single column, less than a slice, the scalar path, exactly one 16-B slice, a slice plus a part, several
COLS = [1, 6, 67, 128, 130, 515]
PATHS = ["host", "host_unordered", "dev", "dev_det", "dev_unordered"]
FREE = ("host_unordered", "dev", "dev_unordered")  # the order of a repeated row's sum is free


def npd_of(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def part_of(kind, size=SIZE):
    assert kind == "range" or size == SIZE
    return RangePartition(2, START, START + size) if kind == "range" else CyclicPartition(*CYC)


def keys_of(kind, local):
    local = np.asarray(local, np.int64)
    return START + local if kind == "range" else CYC[0] + CYC[1] * local


def dev_t(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", gpu))


def push(sh, gpu, rows, offsets, values, weights, path):
    kw = {"host": {}, "host_unordered": {"unordered": True}, "dev": {}, "dev_det": {"deterministic": True},
          "dev_unordered": {"unordered": True}}[path]
    if path.startswith("host"):
        assert sh.updateRowsGrouped(rows, offsets, values, weights, **kw)
    else:
        assert sh.updateRowsGrouped(dev_t(gpu, rows), dev_t(gpu, offsets), dev_t(gpu, values),
                                    None if weights is None else dev_t(gpu, weights), **kw)


def image(sh, gpu):
    """The shard's rows as they lie, and its pitch padding."""
    pitch = C.c_int64()
    assert N.load().glint_shard_pitch(sh.handle, C.byref(pitch)) == N.GLINT_OK
    raw = A.read_image(sh, gpu, sh.size, pitch.value)
    return raw[:, :sh.cols], raw[:, sh.cols:]


def shard(kind, cols, dtype, gpu, table, size=SIZE):
    sh = PartialMatrix(part_of(kind, size), cols, dtype, gpu)
    assert sh.size == size
    write_image(sh, gpu, np.array(table), npd_of(dtype)(PAD))
    return sh


def check_padding(pad, dtype):
    assert (pad == npd_of(dtype)(PAD)).all()  # neither read into a sum nor written


# ---- parity grid ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def case(dtype, cols, weighted):
    """(local rows, offsets, values, coef or None, table, the replay, sum |term| and terms per element);
    computed once and shared by the paths and partitions; read-only."""
    name = np.dtype(npd_of(dtype)).name
    local, offsets = group_records(SIZE)
    g = offsets.size - 1
    values = group_values(name, g, cols)
    coef = group_coef(name, local.size) if weighted else None
    table = group_values(name, SIZE, cols, "table")
    t = group_contrib(values, group_of(offsets, local.size), coef)
    want = replay_grouped(table, local, offsets, values, coef)
    mag = np.zeros((SIZE, cols), np.float64)
    terms = np.ones(SIZE, np.int64)  # the element the shard holds is the sum's first term
    np.add.at(terms, local, 1)
    if np.issubdtype(t.dtype, np.floating):
        mag += np.abs(table.astype(np.float64))
        np.add.at(mag, local, np.abs(t.astype(np.float64)))
        assert np.isfinite(want).all()
    for a in (want, mag, terms):
        a.setflags(write=False)
    return local, offsets, values, coef, table, want, mag, terms


def test_records_cover_the_shapes():
    local, offsets = group_records(SIZE)
    runs = np.bincount(local, minlength=SIZE)
    assert 650 <= local.size <= 750 and {1, 2, 9, 70, 300} <= set(runs.tolist())
    sizes = np.diff(offsets)
    assert sizes[0] == 0 and sizes[-1] == 0 and (sizes[1:-1] == 0).any() and (sizes == 1).any() and (sizes > 64).any()
    group = group_of(offsets, local.size)
    hot = int(np.argmax(runs))
    in_group = np.bincount(group[local == hot])
    assert (in_group > 1).any() and (in_group > 0).sum() > 1  # repeated inside a group and across groups


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", DT)
def test_grouped_push_parity(gpu, dtype, cols, path):
    for kind in PARTS:
        for weighted in (False, True):
            local, offsets, values, coef, table, want, mag, terms = case(dtype, cols, weighted)
            with shard(kind, cols, dtype, gpu, table) as sh:
                push(sh, gpu, keys_of(kind, local), offsets, values, coef, path)
                got, pad = image(sh, gpu)
            what = f"{kind} weighted={weighted}"
            check_padding(pad, dtype)
            if dtype in ("long", "int") or path not in FREE:
                assert_bits(got, want, what)
                continue
            once = terms <= 2  # untouched, or named by one record: bit-exact in every mode
            assert_bits(got[once], want[once], what)
            A.check(got, want, mag, terms, dtype, False)


# ---- identities ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "dev_det"])
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("float", 128), ("double", 130), ("long", 6)])
def test_grouped_push_identities(gpu, dtype, cols, path):
    local, offsets, values, coef, table, _, _, _ = case(dtype, cols, True)
    npd = npd_of(dtype)
    group = group_of(offsets, local.size)
    rows = keys_of("range", local)

    def row_push(sh, r, v):
        if path == "host":
            sh.updateRows(r, v)
        else:
            sh.updateRows(dev_t(gpu, r), dev_t(gpu, v), deterministic=True)

    for w in (None, coef):  # updateRows of the expanded rows on a twin shard
        with shard("range", cols, dtype, gpu, table) as a, shard("range", cols, dtype, gpu, table) as b:
            push(a, gpu, rows, offsets, values, w, path)
            row_push(b, rows, group_contrib(values, group, w))
            assert_bits(image(a, gpu)[0], image(b, gpu)[0])
    # weights all 1: the unweighted call (1 * v is v; the data holds no NaN)
    with shard("range", cols, dtype, gpu, table) as a, shard("range", cols, dtype, gpu, table) as b:
        push(a, gpu, rows, offsets, values, np.ones(local.size, npd), path)
        push(b, gpu, rows, offsets, values, None, path)
        np.testing.assert_array_equal(bits(image(a, gpu)[0]), bits(image(b, gpu)[0]))
    # g == n with groups of one: updateRows(rows, values)
    one = np.array(group_values(np.dtype(npd).name, local.size, cols, "one"))
    with shard("range", cols, dtype, gpu, table) as a, shard("range", cols, dtype, gpu, table) as b:
        push(a, gpu, rows, np.arange(local.size + 1, dtype=np.int64), one, None, path)
        row_push(b, rows, one)
        assert_bits(image(a, gpu)[0], image(b, gpu)[0])


# ---- no fused multiply-add -------------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("dtype,cols", [("double", 2), ("double", 67), ("float", 4), ("float", 67)])
def test_grouped_push_is_unfused(gpu, dtype, cols, path):
    """-b + a * a is exactly +0 with a rounded product and 2^-54 / 2^-24 fused: the vector is a group's
    value row and a the record's weight. On the 16-B path (cols 2 / 4) and on the scalar path (cols 67)."""
    npd = npd_of(dtype)
    c = cols - 1 if cols > 4 else 1
    elem, coef1, x, fused = nofma_element(npd, cols, c)
    table = np.zeros((SIZE, cols), npd)
    table[5] = elem
    with shard("range", cols, dtype, gpu, table) as sh:
        # two groups, the second empty; the middle record of a run of three carries a, the others 0
        w = np.array([0, coef1[0, 0], 0], npd)
        push(sh, gpu, keys_of("range", [5, 5, 5]), np.array([0, 3, 3], np.int64), np.concatenate([x, x]), w, path)
        got = image(sh, gpu)[0][5]
    assert bits(got)[c] == 0, f"{got[c]!r}: a fused product would leave {fused!r}"
    assert not got.any()


# ---- unweighted: the stored bits pass through -------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "dev", "dev_det"])
@pytest.mark.parametrize("dtype,cols", [("double", 6), ("double", 67), ("float", 12), ("float", 67)])
def test_grouped_push_passes_bits_through(gpu, dtype, cols, path):
    npd = npd_of(dtype)
    sub = npd(np.finfo(npd).smallest_subnormal * 5)
    table = np.zeros((SIZE, cols), npd)
    table[3] = -0.0
    values = np.zeros((3, cols), npd)
    values[0] = -0.0  # into the -0.0 row: stays -0.0 (a sum started from +0 would not)
    values[1] = sub   # into a +0 row, once: the subnormal is kept
    values[2] = sub   # into another row, three times: subnormal sums are kept
    local = np.array([3, 8, 9, 9, 9])
    offsets = np.array([0, 1, 2, 5], np.int64)
    want = replay_grouped(table, local, offsets, values)
    assert (bits(want[3]) == bits(npd(-0.0))).all() and want[9, 0] == 3 * sub != 0
    with shard("range", cols, dtype, gpu, table) as sh:
        push(sh, gpu, keys_of("range", local), offsets, values, None, path)
        got, pad = image(sh, gpu)
    np.testing.assert_array_equal(bits(got), bits(want))
    check_padding(pad, dtype)


# ---- device vals not 16-B aligned -------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype,cols", [("double", 128), ("float", 128), ("double", 130)])
def test_grouped_push_unaligned_values_give_the_same_bits(gpu, dtype, cols, weighted):
    import torch
    local, offsets, values, coef, table, want, _, _ = case(dtype, cols, weighted)
    d = torch.device("cuda", gpu)
    buf = torch.zeros(values.size + 8, dtype=getattr(torch, np.dtype(npd_of(dtype)).name), device=d)
    assert buf.data_ptr() % 16 == 0
    v = buf[1:1 + values.size]  # the same values one element into a buffer
    v.copy_(dev_t(gpu, values).view(-1))
    assert v.data_ptr() % 16 != 0 and v.is_contiguous()
    with shard("range", cols, dtype, gpu, table) as sh:
        sh.updateRowsGrouped(dev_t(gpu, keys_of("range", local)), dev_t(gpu, offsets), v.view(values.shape),
                             None if coef is None else dev_t(gpu, coef), deterministic=True)
        assert_bits(image(sh, gpu)[0], want)


# ---- device grp_ptr clamping --------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("long", 128)])
def test_grouped_push_device_offsets_are_clamped(gpu, dtype, cols, weighted):
    """Offsets that are non-decreasing after clamping to [0, n]: record i belongs to the group k with
    c[k] <= i < c[k+1], or to none -- then it is not applied and not reported."""
    local, _, _, coef, table, _, _, _ = case(dtype, cols, weighted)
    n = local.size
    values = group_values(np.dtype(npd_of(dtype)).name, 6, cols, "clamp")
    rows = dev_t(gpu, keys_of("range", local))
    for offsets in ([40, 100, 100, 300, 650],            # grp_ptr[0] > 0 and grp_ptr[g] < n: both ends uncovered
                    [-7, -1, 50, 400, n + 9, 2**40],     # below 0 and above n: as 0, 0, 50, 400, n, n
                    [-(2**62), 10, n, n + 1, 2**62],     # the ends of the type
                    [n + 5, n + 6],                      # nothing covered: one group, empty after clamping
                    [0, n]):                             # everything in one group
        offsets = np.array(offsets, np.int64)
        c = np.clip(offsets, 0, n)
        assert (np.diff(c) >= 0).all()
        group = np.full(n, -1, np.int64)
        for k in range(c.size - 1):
            group[c[k]:c[k + 1]] = k
        covered = np.flatnonzero(group >= 0)
        vals = values[:offsets.size - 1]
        t = group_contrib(vals, group[covered], None if coef is None else coef[covered])
        want = A.fold_rows(table, local[covered], t)
        with shard("range", cols, dtype, gpu, table) as sh:
            # (Long is exact in every mode: the default splits the run of 300, so a chunk may lose every record)
            assert sh.updateRowsGrouped(rows, dev_t(gpu, offsets), dev_t(gpu, vals),
                                        None if coef is None else dev_t(gpu, coef),
                                        deterministic=(dtype == "double"))  # raises nothing: not reported
            assert_bits(image(sh, gpu)[0], want, str(offsets))


# ---- errors -------------------------------------------------------------------------------------------------
def _error_input():
    local, offsets, values, coef, table, _, _, _ = case("long", 6, True)
    rows = np.array(keys_of("range", local))
    rows[7] = START - 1
    rows[60] = START + SIZE
    return local, rows, offsets, values, coef, table


def test_grouped_push_errors_host(gpu):
    _, rows, offsets, values, coef, table = _error_input()
    with shard("range", 6, "long", gpu, table) as sh:
        for w in (None, coef):
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                sh.updateRowsGrouped(rows, offsets, values, w)
            assert ei.value.record == 7  # the lowest
            np.testing.assert_array_equal(image(sh, gpu)[0], table)  # a rejected message applies nothing


def test_grouped_push_errors_device(gpu):
    local, rows, offsets, values, coef, table = _error_input()
    keep = np.ones(local.size, bool)
    keep[[7, 60]] = False
    t = group_contrib(values, group_of(offsets, local.size), coef)
    want = A.fold_rows(table, local[keep], t[keep])
    for det in (False, True):
        with shard("range", 6, "long", gpu, table) as sh:
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                sh.updateRowsGrouped(dev_t(gpu, rows), dev_t(gpu, offsets), dev_t(gpu, values), dev_t(gpu, coef),
                                     deterministic=det)
            assert ei.value.record == 7
            np.testing.assert_array_equal(image(sh, gpu)[0], want)  # the other records were applied


def test_grouped_push_argument_errors(gpu):
    lib = N.load()
    cols = 4
    r = np.array([START, START + 1, START], np.int64)
    o = np.array([0, 1, 3], np.int64)
    v = np.ones((2, cols))
    w = np.ones(3)
    rd, od, vd, wd = (dev_t(gpu, a) for a in (r, o, v, w))
    host = lib.glint_mat_push_rows_grouped
    devc = lambda *args: lib.glint_mat_push_rows_grouped_dev(*args, None)  # noqa: E731
    hp = (r.ctypes.data, o.ctypes.data, v.ctypes.data, w.ctypes.data)
    dp = (rd.data_ptr(), od.data_ptr(), vd.data_ptr(), wd.data_ptr())
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        assert host(vec.handle, hp[0], 3, hp[1], 2, hp[2], hp[3], 0) == N.GLINT_EINVAL
        assert devc(vec.handle, dp[0], 3, dp[1], 2, dp[2], dp[3], 0) == N.GLINT_EINVAL
    table = np.full((10, cols), 2.0)
    with shard("range", cols, "double", gpu, table, size=10) as sh:
        h = sh.handle
        for call, (pr, po, pv, pw) in ((host, hp), (devc, dp)):
            assert call(h, pr, 3, po, 2, pv, pw, N.GLINT_PUSH_VALIDATE) == N.GLINT_EINVAL
            assert call(h, pr, 3, po, 2, pv, pw, 8) == N.GLINT_EINVAL  # unknown flag bit
            assert call(h, pr, -1, po, 2, pv, pw, 0) == N.GLINT_EINVAL
            assert call(h, pr, (1 << 32) - 2048, po, 2, pv, pw, 0) == N.GLINT_EINVAL
            assert call(h, pr, 3, po, -1, pv, pw, 0) == N.GLINT_EINVAL
            assert call(h, pr, 3, po, 1 << 31, pv, pw, 0) == N.GLINT_EINVAL
            assert call(h, pr, 3, None, 2, pv, pw, 0) == N.GLINT_EINVAL
            assert call(h, None, 3, po, 2, pv, pw, 0) == N.GLINT_EINVAL
            assert call(h, pr, 3, po, 2, None, pw, 0) == N.GLINT_EINVAL
        # host only: a grp_ptr that breaks the rule, checked before anything is staged
        for bad in ([1, 1, 3], [0, 1, 2], [0, 1, 4], [3, 3, 0], [0, 5, 3], [0, -1, 3]):
            b = np.array(bad, np.int64)
            assert host(h, hp[0], 3, b.ctypes.data, 2, hp[2], hp[3], 0) == N.GLINT_EINVAL, bad
        sh.sync()
        np.testing.assert_array_equal(image(sh, gpu)[0], table)  # none of them changed the shard
        # n == 0 launches nothing
        z = np.zeros(1, np.int64)
        assert host(h, None, 0, z.ctypes.data, 0, None, None, 0) == N.GLINT_OK
        assert devc(h, None, 0, dev_t(gpu, z).data_ptr(), 0, None, None, 0) == N.GLINT_OK
        # the wrapper: shapes, and mixing host arrays and device tensors
        for args in ((r, o, np.ones((3, cols))), (r, o, np.ones((2, cols + 1))), (r, o, v, np.ones(2)),
                     (r, np.zeros(0, np.int64), np.zeros((0, cols)))):
            with pytest.raises(ValueError):
                sh.updateRowsGrouped(*args)
        for args in ((rd, o, vd), (rd, od, v), (rd, od, vd, w), (r, od, v), (r, o, v, wd)):
            with pytest.raises(TypeError):
                sh.updateRowsGrouped(*args)
        with pytest.raises(TypeError):
            sh.updateRowsGrouped(rd, od, vd.float())  # not the shard's type
        with pytest.raises(ValueError):
            sh.updateRowsGrouped(rd, od, vd, wd[:2].clone())
        np.testing.assert_array_equal(image(sh, gpu)[0], table)
        assert sh.updateRowsGrouped(r, o, v) and sh.updateRowsGrouped(rd, od, vd.view(-1), wd)
        want = table.copy()
        want[0] += 4
        want[1] += 2
        np.testing.assert_array_equal(image(sh, gpu)[0], want)


def test_grouped_push_refuses_a_slab_with_views_on_the_host(gpu):
    slab = PartialMatrix(RangePartition(0, 0, 128), 4, "double", gpu)
    view = PartialMatrix.view(slab, RangePartition(0, START, START + 64), 0)
    try:
        r, o, v = np.array([3], np.int64), np.array([0, 1], np.int64), np.ones((1, 4))
        with pytest.raises(ValueError):
            slab.updateRowsGrouped(r, o, v)
        assert view.updateRowsGrouped(r + START, o, v)  # the view itself is a shard like any other
        assert (view.getRows(r + START) == 1.0).all()
    finally:
        view.destroy()
        slab.destroy()


# ---- profiling ------------------------------------------------------------------------------------------------
def _counts(sh):
    out = []
    for kid in range(N.GLINT_K_COUNT):
        ms, cnt = C.c_double(), C.c_int64()
        assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
        out.append(cnt.value)
    return np.array(out)


@pytest.mark.parametrize("path", ["host", "dev", "dev_det"])
def test_grouped_push_profiling(gpu, path):
    local, offsets, values, coef, table, _, _, _ = case("double", 67, True)
    rows = keys_of("range", local)
    t = group_contrib(values, group_of(offsets, local.size), coef)
    with shard("range", 67, "double", gpu, table) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        c0 = _counts(sh)
        if path == "host":
            sh.updateRows(rows, t)
        else:
            sh.updateRows(dev_t(gpu, rows), dev_t(gpu, t), deterministic=(path == "dev_det"))
        c1 = _counts(sh)
        fold = np.zeros(N.GLINT_K_COUNT, np.int64)
        fold[N.GLINT_K_PUSH_ROWS] = 1
        front = c1 - c0 - fold  # what the row push records for its front end
        assert (front >= 0).all()
        for w in (None, coef):
            before = _counts(sh)
            push(sh, gpu, rows, offsets, values, w, path)
            np.testing.assert_array_equal(_counts(sh) - before, front + fold)  # the front end and one fold launch
        before = _counts(sh)
        z = np.zeros(0, np.int64)
        push(sh, gpu, z, np.zeros(3, np.int64), values[:2], None, path)  # n == 0 launches nothing
        np.testing.assert_array_equal(_counts(sh), before)


# ---- sequence -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("where", ["host", "dev"])
@pytest.mark.parametrize("dtype", ["double", "float"])
def test_grouped_push_sequence(gpu, dtype, where):
    """getRowsSum of the groups, updateRowsGrouped of a function of that answer, getRows: an embedding
    bag's forward pass, its backward pass and a read, against the numpy replay of the three steps."""
    cols = 67
    npd = npd_of(dtype)
    local, offsets, _, coef, table, _, _, _ = case(dtype, cols, True)
    rows = keys_of("cyclic", local)
    every = keys_of("cyclic", np.arange(SIZE))
    lr = npd(-0.125)  # a power of two: the product is exact, so numpy and torch agree on it
    sums = replay_groups(table, local, offsets)
    want = replay_grouped(table, local, offsets, np.multiply(sums, lr, dtype=npd), coef)
    with shard("cyclic", cols, dtype, gpu, table) as sh:
        if where == "host":
            s = sh.getRowsSum(rows, offsets)
            sh.updateRowsGrouped(rows, offsets, s * lr, coef)
            got = sh.getRows(every)
        else:
            r, o = dev_t(gpu, rows), dev_t(gpu, offsets)
            s = sh.getRowsSum(r, o, sync=False)
            sh.updateRowsGrouped(r, o, s * float(lr), dev_t(gpu, coef), deterministic=True, sync=False)
            out = sh.getRows(dev_t(gpu, every), sync=False)
            sh.sync(sh._stream_of(r))
            s, got = s.cpu().numpy(), out.cpu().numpy()
    assert_bits(np.asarray(s), sums)
    assert_bits(np.asarray(got).reshape(SIZE, cols), want)
