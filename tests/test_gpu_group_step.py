"""Grouped optimizer row pushes (updateRowsAdagrad / AdagradRowwise / Adam / Ftrl with ``offsets``,
glint_mat_push_rows_*_grouped*) against the replay of the expanded rows.

The call is deterministic on every path, so the bar is one: both shards equal group_step_cases.replay bit for
bit (a NaN by class), on the host and on the device path. The premises of the inputs are asserted from the
replays alone in test_group_step_cpu.py.
"""
import ctypes as C

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import (ArrayIndexOutOfBoundsException, Client, CyclicPartitioner, PartialMatrix, PartialVector,
                       RangePartition, RangePartitioner)
from adagrad_cases import NOFMA, assert_bits
from group_cases import bits, group_coef, group_contrib, group_of, group_records, group_values
from group_step_cases import OPT, SIZE, case, inputs, replay, start

pytestmark = pytest.mark.gpu
START = 1_000_003
PATHS = ["host", "dev"]
SLICED = ("adagrad", "adam", "ftrl")


def np_name(dtype):
    return np.dtype(glint_amd.shard.resolve_dtype(dtype)[1]).name


def pair(gpu, name, dtype, cols, w0=None, s0=None, size=SIZE):
    """(weights, state) over rows [START, START + size), holding w0 and s0 when given (0 + x is x)."""
    part, parts = RangePartition(2, START, START + size), OPT[name][5]
    w = PartialMatrix(part, cols, dtype, gpu)
    s = PartialMatrix(part, parts * cols, dtype, gpu) if parts else PartialVector(part, dtype, gpu)
    keys = np.arange(START, START + size, dtype=np.int64)
    if w0 is not None and w0.any():
        w.updateRows(keys, w0)
    if s0 is not None and s0.any():
        s.updateRows(keys, s0) if parts else s.update(keys, s0)
    return w, s


def push(name, w, s, gpu, local, offsets, values, coef, path, vals_dev=None, sync=True):
    args = [np.asarray(local) + START, values, np.asarray(offsets), coef]
    if path == "dev":
        import torch
        d = torch.device("cuda", gpu)
        args = [None if a is None else torch.from_numpy(np.array(a)).to(d) for a in args]
        if vals_dev is not None:
            args[1] = vals_dev
    return getattr(w, OPT[name][0])(s, args[0], args[1], *OPT[name][3], sync=sync, offsets=args[2], weights=args[3])


def check(w, s, want_w, want_s):
    assert_bits(s.to_numpy(), want_s, "state")
    assert_bits(w.to_numpy(), want_w, "weights")


# cols 3: less than a scalar slice; 67: two scalar slices, pitch padding; 128: the 16-B path. Row-wise also 259
# (five scalar strips: KEEP 0) and 1028 Float / 516 Double (five 16-B strips: KEEP 0)
GRID = [(n, dt, c) for n in SLICED for dt in ("double", "float") for c in (3, 67, 128)] + \
       [("rowwise", dt, c) for dt, wide in (("double", 516), ("float", 1028)) for c in (3, 67, 128, 259, wide)]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("name,dtype,cols", GRID)
def test_parity(gpu, name, dtype, cols, weighted, path):
    dn = np_name(dtype)
    w, s = pair(gpu, name, dtype, cols, *start(name, dn, cols))
    with w, s:
        for _ in range(2):  # the second push steps from the first one's state
            assert push(name, w, s, gpu, *inputs(dn, cols, weighted), path)
        check(w, s, *case(name, dn, cols, weighted))


@pytest.mark.parametrize("name", ["adam", "rowwise"])
def test_alignment_independence(gpu, name):
    """Value rows 16-B aligned (the 16-B loads at cols 128) and one element off (the scalar loads): one set of
    bits, the replay's."""
    import torch
    cols, d = 128, torch.device("cuda", gpu)
    local, offsets, values, coef = inputs("float64", cols, True)
    w0, s0 = start(name, "float64", cols)
    for off in (0, 1):
        buf = torch.zeros(values.size + 2, dtype=torch.float64, device=d)
        v = buf[off:off + values.size]
        v.copy_(torch.from_numpy(np.array(values)).to(d).view(-1))
        assert v.data_ptr() % 16 == 8 * off
        w, s = pair(gpu, name, "double", cols, w0, s0)
        with w, s:
            assert push(name, w, s, gpu, local, offsets, values, coef, "dev", vals_dev=v)
            check(w, s, *replay(name, w0, s0, local, offsets, values, coef))


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cols", [2, 67])
@pytest.mark.parametrize("dtype", ["double", "float"])
def test_weight_product_is_unfused(gpu, dtype, cols, path):
    """adagrad_cases.NOFMA: one row, two records in two groups, 1 * -b + a * a in the last column. With the
    product rounded before the add G is +0 and, eps being 1, the weight stays +0; fma(a, a, -b) is not 0."""
    npd = glint_amd.shard.resolve_dtype(dtype)[1]
    a, b, _ = NOFMA[npd]
    values = np.zeros((2, cols), npd)
    values[0, -1], values[1, -1] = -b, a
    local, offsets, coef = np.array([7, 7]), np.array([0, 1, 2]), np.array([1, a], npd)
    zero = np.zeros((SIZE, cols), npd)
    want_w, want_h = OPT["adagrad"][6](zero, zero, local, coef[:, None] * values, 0.05, 1.0)
    assert (bits(want_w) == 0).all() and (bits(want_h) == 0).all()
    w, s = pair(gpu, "adagrad", dtype, cols)
    with w, s:
        args = [local + START, values, offsets, coef]
        if path == "dev":
            import torch
            args = [torch.from_numpy(x).to(torch.device("cuda", gpu)) for x in args]
        assert w.updateRowsAdagrad(s, args[0], args[1], 0.05, 1.0, offsets=args[2], weights=args[3])
        check(w, s, want_w, want_h)


@pytest.mark.parametrize("name,cols", [(n, c) for n in OPT for c in (67, 128)] + [("rowwise", 1028)])
def test_uncovered_records(gpu, name, cols):
    """Device offsets that clamp to [0, 30, 30, 250, 400] over 700 records: records 400.. have no group. A row
    all of whose records are uncovered is not stepped -- neither shard's bits change --, the others take the
    replay's step over their covered records, and nothing is reported."""
    local = np.array(group_records(SIZE)[0])
    unused = np.setdiff1d(np.arange(SIZE), local)[0]
    local[650:660] = unused
    assert set(local[:400]) & set(local[400:]) and unused not in local[:400]
    offsets, cut = np.array([-7, 30, 30, 250, 400], np.int64), np.array([0, 30, 30, 250, 400], np.int64)
    values, coef = group_values("float32", 4, cols), group_coef("float32", 700)
    w0, s0 = start(name, "float32", cols)
    w, s = pair(gpu, name, "float", cols, w0, s0)
    with w, s:
        assert push(name, w, s, gpu, local, offsets, values, coef, "dev")
        check(w, s, *replay(name, w0, s0, local[:400], cut, values, coef[:400]))


def test_errors(gpu):
    """Host: a row outside the partition rejects the message with its record index, both shards unchanged.
    Device: that record is skipped, the others applied, the error raised at the sync."""
    name, cols = "adam", 6
    local, offsets, values, coef = inputs("float64", cols, True)
    local = np.array(local)
    local[7] = -1
    w0, s0 = start(name, "float64", cols)
    w, s = pair(gpu, name, "double", cols, w0, s0)
    with w, s:
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push(name, w, s, gpu, local, offsets, values, coef, "host")
        assert ei.value.record == 7
        check(w, s, w0, s0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push(name, w, s, gpu, local, offsets, values, coef, "dev")
        assert ei.value.record == 7
        s.sync()
        keep = np.arange(local.size) != 7
        contrib = group_contrib(values, group_of(offsets, local.size), coef)[keep]
        check(w, s, *OPT[name][6](w0, s0, local[keep], contrib, *OPT[name][3]))


@pytest.mark.parametrize("dev", [False, True], ids=PATHS)
@pytest.mark.parametrize("name", list(OPT))
def test_c_argument_checks(gpu, name, dev):
    import torch
    lib, d = N.load(), torch.device("cuda", gpu)
    _, _, symbol, _, kc, parts, _ = OPT[name]
    arrays = (np.array([START], np.int64), np.array([0, 1], np.int64), np.ones(4), np.ones(1))
    held = [torch.from_numpy(x).to(d) for x in arrays] if dev else arrays
    r, o, v, c = (x.data_ptr() if dev else x.ctypes.data for x in held)
    w, s = pair(gpu, name, "double", 4, size=10)
    odd = PartialMatrix(RangePartition(2, START, START + 10), 12, "double", gpu)  # no optimizer's state shape
    with w, s, odd:
        def call(a, b, n=1, rows=r, grp=o, g=1, vals=v, coef=c):
            tail = (None,) if dev else ()
            return getattr(lib, symbol + ("_dev" if dev else ""))(a, b, rows, n, grp, g, vals, coef, *kc, *tail)

        assert call(None, s.handle) == call(w.handle, None) == N.GLINT_EINVAL
        assert call(w.handle, w.handle) == N.GLINT_EINVAL  # state is weights
        assert call(w.handle, odd.handle) == N.GLINT_EINVAL  # the state's shape
        assert call(w.handle, s.handle, g=-1) == call(w.handle, s.handle, grp=None) == N.GLINT_EINVAL
        assert call(w.handle, s.handle, vals=None) == call(w.handle, s.handle, rows=None) == N.GLINT_EINVAL
        if not dev:  # a host grp_ptr is checked: non-decreasing from 0 to n
            bad = np.array([0, 2], np.int64)
            assert call(w.handle, s.handle, grp=bad.ctypes.data) == N.GLINT_EINVAL
        assert call(w.handle, s.handle, n=0, rows=None, g=0, vals=None, coef=None) == N.GLINT_OK
        assert not w.to_numpy().any() and not s.to_numpy().any()
        assert call(w.handle, s.handle, coef=None) == N.GLINT_OK  # coef may be NULL
        w.sync()
        assert w.to_numpy()[0].all() and not w.to_numpy()[1:].any()


def test_python_argument_checks(gpu):
    import torch
    r, o, v, c = np.array([START, START + 1]), np.array([0, 1, 2]), np.ones((2, 4)), np.ones(2)
    rd, od, vd = (torch.from_numpy(x).to(torch.device("cuda", gpu)) for x in (r, o, v))
    w, s = pair(gpu, "adagrad", "double", 4, size=10)
    with w, s:
        with pytest.raises(ValueError):
            w.updateRowsAdagrad(s, r, np.ones((2, 4)), 0.1, weights=c)  # weights without offsets
        for bad in (dict(grads=np.ones((3, 4))), dict(weights=np.ones(3)), dict(offsets=np.zeros(0, np.int64))):
            with pytest.raises(ValueError):
                w.updateRowsAdagrad(s, r, **{"grads": v, "lr": 0.1, "offsets": o, "weights": c, **bad})
        for mixed in ((rd, v, o), (r, vd, o), (r, v, od), (rd, vd, o)):
            with pytest.raises(TypeError):
                w.updateRowsAdagrad(s, mixed[0], mixed[1], 0.1, offsets=mixed[2])
        with pytest.raises(TypeError):
            w.updateRowsAdagrad(s, rd, vd, 0.1, offsets=od, weights=c)
        assert not w.to_numpy().any() and not s.to_numpy().any()


def _launches(sh):
    out = []
    for kid in range(N.GLINT_K_COUNT):
        ms, cnt = C.c_double(), C.c_int64()
        assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
        out.append(cnt.value)
    return out


@pytest.mark.parametrize("name", list(OPT))
def test_launch_count(gpu, name):
    local, offsets, values, coef = inputs("float64", 4, True)
    w, s = pair(gpu, name, "double", 4)
    with w, s:
        for sh in (w, s):
            assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        one = [int(k == N.GLINT_K_PUSH_ROWS) for k in range(N.GLINT_K_COUNT)]
        for i, path in enumerate(PATHS):  # the front end and the group ids are not counted: one fold launch
            push(name, w, s, gpu, local, offsets, values, coef, path)
            assert _launches(w) == [(i + 1) * x for x in one] and not any(_launches(s))
            push(name, w, s, gpu, local[:0], [0], values[:0], coef[:0], path)  # an empty call launches nothing
            assert _launches(w) == [(i + 1) * x for x in one] and not any(_launches(s))


@pytest.mark.parametrize("kind", ["range", "cyclic"])
@pytest.mark.parametrize("name", ["rowwise", "ftrl"])
def test_client(gpu, name, kind):
    """Three devices' worth of partitions, two models per server: each partition gets its own sub-groups and
    state shard; the whole table is the replay's."""
    _, method, _, k, _, parts, _ = OPT[name]
    cols = 67
    make = RangePartitioner.apply if kind == "range" else CyclicPartitioner.apply
    c = Client([gpu] * 3)
    m = c.matrix(SIZE, cols, "double", modelsPerServer=2, createPartitioner=make)
    st = c.matrix(SIZE, parts * cols, "double", modelsPerServer=2, createPartitioner=make) if parts \
        else c.vector(SIZE, "double", modelsPerServer=2, createPartitioner=make)
    try:
        assert m.nrOfPartitions == 6
        local, offsets, values, coef = inputs("float64", cols, True)
        with pytest.raises(ValueError):
            getattr(m, method)(st, local, np.zeros((local.size, cols)), *k, weights=coef)  # weights, no offsets
        want = np.zeros((SIZE, cols)), np.zeros((SIZE, parts * cols) if parts else SIZE)
        for _ in range(2):
            assert getattr(m, method)(st, local, values, *k, offsets=offsets, weights=coef)
            want = replay(name, *want, local, offsets, values, coef)
        every = np.arange(SIZE, dtype=np.int64)
        assert_bits(m.pull(every), want[0], "weights")
        assert_bits(st.pull(every), want[1], "state")
    finally:
        m.destroy()
        st.destroy()
