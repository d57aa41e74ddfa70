"""Narrow-format row transport (PartialMatrix.getRowsAs / updateRowsAs, glint_mat_pull_rows_as*,
glint_mat_push_rows_as*) on the GPU.

A pull is defined as the narrowing of what getRows returns and a push as updateRows of the widened rows, so
the expected values are numpy's conversions (wire_cases.ref_narrow / ref_widen), getRows, and updateRows on a
twin shard.

Bar: a pull is bit for bit everywhere (a NaN by class). A push is bit for bit for host calls and deterministic
device calls, and a row that occurs once is bit-exact in every mode; where the order of a repeated row's sum
is free (``unordered`` and the device default) the sums are held to test_gpu_axpy.check's bar, with the
element the shard held before the push counted as one of the sum's terms."""
import ctypes as C
import functools

import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import (ArrayIndexOutOfBoundsException, BigMatrix, CyclicPartition, CyclicPartitioner, PartialMatrix,
                       PartialVector, RangePartition, RangePartitioner)
from axpy_cases import assert_bits, fold_rows
from ieee_cases import edge_image, write_image
from wire_cases import (NPV, NPW, PAIRS, assert_wire_bits, bits, from_dev, narrow_set, padded, ref_narrow, ref_widen,
                        to_dev, torch_wire, widen_all)
import test_gpu_axpy as A  # check: the bar of a sum whose order is free; read_image

pytestmark = pytest.mark.gpu
START, SIZE = 1_000_003, 300
CYC = (2, 5, 1498)  # partition 2 of 5 over 1498 keys: 300 rows, key = 2 + 5 * local
PARTS = ["range", "cyclic"]
PAD = 777
# one column; a 16-B shard row whose wire row is 8 B (Float); the element path; exactly one 16-B wire chunk
# (Float); the element path past a slice; full slices; a slice and a part; the element path over several slices
COLS = [1, 4, 6, 8, 67, 128, 136, 515]
PATHS = ["host", "host_unordered", "dev", "dev_det", "dev_unordered"]
FREE = ("host_unordered", "dev", "dev_unordered")  # the order of a repeated row's sum is free
MAX_ROWS = 1100  # the largest shard a test here builds


def part_of(kind, size=SIZE):
    assert kind == "range" or size == SIZE
    return RangePartition(2, START, START + size) if kind == "range" else CyclicPartition(*CYC)


def keys_of(kind, local):
    local = np.asarray(local, np.int64)
    return START + local if kind == "range" else CYC[0] + CYC[1] * local


def dev_t(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", gpu))


def image(sh, gpu):
    """The shard's rows as they lie, and its pitch padding."""
    pitch = C.c_int64()
    assert N.load().glint_shard_pitch(sh.handle, C.byref(pitch)) == N.GLINT_OK
    raw = A.read_image(sh, gpu, sh.size, pitch.value)
    return raw[:, :sh.cols], raw[:, sh.cols:]


def shard(kind, cols, dtype, gpu, table, size=SIZE):
    sh = PartialMatrix(part_of(kind, size), cols, dtype, gpu)
    assert sh.size == size == table.shape[0]
    write_image(sh, gpu, np.array(table), NPV[dtype](PAD))
    return sh


def check_padding(pad, dtype):
    assert (pad == NPV[dtype](PAD)).all()  # neither read nor written


def offset_buffer(gpu, wire, elems, offset):
    """(buffer, the `elems` elements that start `offset` elements into it): the buffer 16-B aligned and filled
    with a sentinel, 16 elements longer than offset + elems."""
    import torch
    raw = {2: torch.int16, 4: torch.int32}[np.dtype(NPW[wire]).itemsize]
    buf = torch.full((offset + elems + 16,), 0x5A5A, dtype=raw, device=torch.device("cuda", gpu)).view(torch_wire(wire))
    assert buf.data_ptr() % 16 == 0
    return buf, buf[offset:offset + elems]


def sentinel_intact(buf, wire, offset, elems):
    raw = from_dev(buf, wire)
    rest = np.concatenate([bits(raw[:offset]), bits(raw[offset + elems:])])
    return (rest == 0x5A5A).all()


def pull(sh, gpu, rows, wire, where, offset=0):
    """getRowsAs through the host call or the device call, as the wire host array; on the device into a buffer
    with a sentinel around the answer, which must stay intact."""
    rows = np.asarray(rows, np.int64)
    if where == "host":
        return sh.getRowsAs(rows, wire)
    elems = rows.size * sh.cols
    buf, out = offset_buffer(gpu, wire, elems, offset)
    assert out.data_ptr() % 16 == (offset * out.element_size()) % 16
    got = sh.getRowsAs(dev_t(gpu, rows), wire, out=out.view(rows.size, sh.cols))
    assert got.data_ptr() == out.data_ptr()
    assert sentinel_intact(buf, wire, offset, elems), "written outside n * cols * sizeof W bytes"
    return from_dev(out, wire).reshape(rows.size, sh.cols)


def push(sh, gpu, rows, vals, wire, path, offset=0):
    kw = {"host": {}, "host_unordered": {"unordered": True}, "dev": {}, "dev_det": {"deterministic": True},
          "dev_unordered": {"unordered": True}}[path]
    if path.startswith("host"):
        assert sh.updateRowsAs(rows, vals, wire, **kw)
        return
    v = to_dev(gpu, vals, wire)
    if offset:
        buf, at = offset_buffer(gpu, wire, v.numel(), offset)
        at.copy_(v.view(-1))
        assert at.data_ptr() % 16 != 0 and at.is_contiguous()
        v = at
    assert sh.updateRowsAs(dev_t(gpu, rows), v, wire, **kw)


def row_push(sh, gpu, rows, vals, path):
    """updateRows of rows in the shard's type, on the same path."""
    kw = {"host": {}, "host_unordered": {"unordered": True}, "dev": {}, "dev_det": {"deterministic": True},
          "dev_unordered": {"unordered": True}}[path]
    if path.startswith("host"):
        assert sh.updateRows(rows, vals, **kw)
    else:
        assert sh.updateRows(dev_t(gpu, rows), dev_t(gpu, vals), **kw)


# ---- 1. narrowing is the contract's ---------------------------------------------------------------------------
@pytest.mark.parametrize("cols", [136, 515])  # the 16-B path and the element path, for Float and for Double
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_pull_narrows_as_the_contract(gpu, dtype, wire, cols):
    """narrow_set -- every tie between neighbouring W values with the values around it, the subnormal range, the
    overflow threshold -- written into shards of at most 1100 rows and pulled whole, host and device."""
    x = padded(narrow_set(wire), cols)
    for at in range(0, x.shape[0], MAX_ROWS):
        part = x[at:at + MAX_ROWS]
        want = ref_narrow(part, wire)
        size = part.shape[0]
        local = np.arange(size)
        with shard("range", cols, dtype, gpu, part, size=size) as sh:
            for where in ("host", "dev"):
                assert_wire_bits(pull(sh, gpu, keys_of("range", local), wire, where), want, wire, f"{where} rows {at}+")
            np.testing.assert_array_equal(bits(image(sh, gpu)[0]), bits(part))  # a pull writes nothing


# ---- 2. widening is exact for every pattern -------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "dev", "dev_det"])
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_push_widens_every_pattern_exactly(gpu, dtype, wire, path):
    """Every pattern of the wire type (F32: wire_cases' 6144) pushed once into a shard filled with -0.0, where
    -0 + x keeps every x, the sign of a zero included: the shard's image is numpy's widening."""
    w = widen_all(wire)
    w = w.reshape(256, -1)  # 256 x 256, or 256 x 24: one record per row
    rows, cols = w.shape
    npv = NPV[dtype]
    want = ref_widen(w, wire)
    assert (bits(np.add(npv(-0.0), want[~np.isnan(want)], dtype=npv)) == bits(want[~np.isnan(want)])).all()
    for order in (np.arange(rows), np.random.default_rng(3).permutation(rows)):  # record i: row order[i]
        with PartialMatrix(RangePartition(0, START, START + rows), cols, dtype, gpu) as sh:
            write_image(sh, gpu, np.zeros((rows, cols), npv), npv(PAD))
            assert sh.fill(-0.0)
            before, _ = image(sh, gpu)
            assert (bits(before) == bits(npv(-0.0))).all()
            push(sh, gpu, keys_of("range", order), w[order], wire, path)
            got, pad = image(sh, gpu)
        assert_bits(got, want, path)
        check_padding(pad, dtype)


# ---- 3. pull equals narrow(getRows) ---------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def requests(n):
    """n local rows of the 300, shuffled, with repeats (n = 700 names every row at least once)."""
    rng = np.random.default_rng(100 + n)
    r = rng.integers(0, SIZE, n)
    if n >= 3:
        r[n // 2] = r[0]  # a row requested twice
    if n >= SIZE:
        r[:SIZE] = rng.permutation(SIZE)
    r = rng.permutation(r)
    r.setflags(write=False)
    return r


@pytest.mark.parametrize("kind", PARTS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_pull_equals_narrowed_get_rows(gpu, dtype, wire, cols, kind):
    table = edge_image(dtype, SIZE, cols)  # -0.0, NaNs, infinities, subnormals, +/-MAX among ordinary values
    with shard(kind, cols, dtype, gpu, table) as sh:
        for n in (1, 63, 64, 65, 700):
            local = requests(n)
            rows = keys_of(kind, local)
            wide = sh.getRows(rows)
            np.testing.assert_array_equal(bits(wide), bits(table[local]))
            want = ref_narrow(wide, wire)
            assert_wire_bits(pull(sh, gpu, rows, wire, "host"), want, wire, f"host n={n}")
            assert_wire_bits(pull(sh, gpu, rows, wire, "dev"), want, wire, f"dev n={n}")
            assert_wire_bits(pull(sh, gpu, rows, wire, "dev", offset=1), want, wire, f"dev, out one element off, n={n}")
        got, pad = image(sh, gpu)
    np.testing.assert_array_equal(bits(got), bits(table))
    check_padding(pad, dtype)


# ---- 4. push equals updateRows of the widened rows ------------------------------------------------------------
LISTS = ["distinct", "hot", "zipf"]


@functools.lru_cache(maxsize=None)
def records(name):
    """Local rows of a push. distinct: 200 rows once each. hot: three rows hit 65, 129 and 300 times (past one
    64-record batch, past the 128-record split, several chunks) among 150 other records, shuffled. zipf: 700
    records, row r drawn with weight 1 / (r + 1)."""
    rng = np.random.default_rng({"distinct": 1, "hot": 2, "zipf": 3}[name])
    if name == "distinct":
        r = rng.permutation(SIZE)[:200]
    elif name == "hot":
        a, b, c = rng.permutation(SIZE)[:3]
        r = rng.permutation(np.concatenate([np.full(65, a), np.full(129, b), np.full(300, c),
                                            rng.integers(0, SIZE, 150)]))
    else:
        p = 1.0 / (np.arange(SIZE) + 1.0)
        r = rng.choice(SIZE, 700, p=p / p.sum())
    r = r.astype(np.int64)
    r.setflags(write=False)
    return r


@functools.lru_cache(maxsize=None)
def push_case(dtype, wire, cols, name):
    """(local rows, wire values, table, the replay in list order, sum |term| and terms per row); computed once,
    shared by the paths and partitions; read-only. The values span six decades and are finite in every wire
    type; the table is non-zero, so the shard's element is a term of every sum."""
    npv = NPV[dtype]
    local = records(name)
    rng = np.random.default_rng([len(name), cols, PAIRS.index((dtype, wire))])
    n = local.size
    vals = ref_narrow((rng.standard_normal((n, cols)) * 10.0 ** rng.integers(-3, 3, (n, cols))).astype(npv), wire)
    table = (rng.standard_normal((SIZE, cols)) * 10.0 ** rng.integers(-3, 3, (SIZE, cols))).astype(npv)
    wide = ref_widen(vals, wire)
    assert np.isfinite(wide).all()
    want = fold_rows(table, local, wide)
    mag = np.abs(table.astype(np.float64))
    np.add.at(mag, local, np.abs(wide.astype(np.float64)))
    terms = np.ones(SIZE, np.int64)  # the element the shard holds is the sum's first term
    np.add.at(terms, local, 1)
    assert np.isfinite(want).all()
    for a in (vals, table, wide, want, mag, terms):
        a.setflags(write=False)
    return local, vals, table, wide, want, mag, terms


def test_records_cover_the_shapes():
    assert np.bincount(records("distinct")).max() == 1
    runs = np.bincount(records("hot"), minlength=SIZE)
    count = lambda lo, hi: int(((runs >= lo) & (runs < hi)).sum())  # noqa: E731
    assert count(65, 75) == 1 and count(129, 140) == 1 and count(300, 310) == 1
    runs = np.bincount(records("zipf"), minlength=SIZE)
    assert runs.max() > 64 and (runs == 1).any() and (runs == 0).any()


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_push_equals_row_push_of_widened_rows(gpu, dtype, wire, cols, path):
    for kind in PARTS:
        for name in LISTS:
            local, vals, table, wide, want, mag, terms = push_case(dtype, wire, cols, name)
            rows = keys_of(kind, local)
            with shard(kind, cols, dtype, gpu, table) as a, shard(kind, cols, dtype, gpu, table) as b:
                push(a, gpu, rows, vals, wire, path)
                row_push(b, gpu, rows, wide, path)
                got, pad = image(a, gpu)
                twin, _ = image(b, gpu)
            what = f"{kind} {name}"
            check_padding(pad, dtype)
            once = terms <= 2  # untouched, or named by one record: bit-exact in every mode
            assert (~once).any() or name == "distinct"
            assert_bits(got[once], want[once], what)
            assert_bits(got[terms == 1], table[terms == 1], what)  # rows the push does not name keep their bits
            if path not in FREE:
                assert_bits(got, twin, what)
                assert_bits(got, want, what)
            else:
                A.check(got, want, mag, terms, dtype, False)
                A.check(twin, want, mag, terms, dtype, False)


@pytest.mark.parametrize("cols", [4, 8, 128, 136, 515])
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_push_unaligned_values_give_the_same_bits(gpu, dtype, wire, cols):
    local, vals, table, _, want, _, _ = push_case(dtype, wire, cols, "hot")
    with shard("range", cols, dtype, gpu, table) as sh:
        push(sh, gpu, keys_of("range", local), vals, wire, "dev_det", offset=1)
        got, pad = image(sh, gpu)
    assert_bits(got, want)
    check_padding(pad, dtype)


# ---- 5. errors ------------------------------------------------------------------------------------------------
def test_argument_errors(gpu):
    lib = N.load()
    cols = 4
    r = np.array([START, START + 1, START], np.int64)
    rd = dev_t(gpu, r)
    pull_h = lambda h, pr, po, n, w: lib.glint_mat_pull_rows_as(h, pr, po, n, w)  # noqa: E731
    pull_d = lambda h, pr, po, n, w: lib.glint_mat_pull_rows_as_dev(h, pr, po, n, w, None)  # noqa: E731
    push_h = lambda h, pr, pv, n, w, f: lib.glint_mat_push_rows_as(h, pr, pv, n, w, f)  # noqa: E731
    push_d = lambda h, pr, pv, n, w, f: lib.glint_mat_push_rows_as_dev(h, pr, pv, n, w, f, None)  # noqa: E731
    buf_h = np.zeros(3 * cols, np.float64)
    buf_d = dev_t(gpu, buf_h)
    hp, dp = (r.ctypes.data, buf_h.ctypes.data), (rd.data_ptr(), buf_d.data_ptr())
    calls = ((pull_h, push_h, hp), (pull_d, push_d, dp))
    F16, BF16, F32 = N.GLINT_WIRE_F16, N.GLINT_WIRE_BF16, N.GLINT_WIRE_F32
    with PartialVector(RangePartition(0, START, START + 10), "float", gpu) as vec:  # a vector shard
        for pl, ps, (pr, pb) in calls:
            assert pl(vec.handle, pr, pb, 3, F16) == N.GLINT_EINVAL
            assert ps(vec.handle, pr, pb, 3, F16, 0) == N.GLINT_EINVAL
    unsupported = {"int": (F16, BF16, F32), "long": (F16, BF16, F32), "float": (F32, -1, 3), "double": (F16, BF16, 3)}
    for dtype, wires in unsupported.items():
        table = np.full((10, cols), 2, {"int": np.int32, "long": np.int64, **NPV}[dtype])
        with PartialMatrix(RangePartition(0, START, START + 10), cols, dtype, gpu) as sh:
            assert sh.update(np.repeat(r[:2], cols), np.tile(np.arange(cols, dtype=np.int32), 2), table[:2].reshape(-1))
            before = sh.to_numpy()
            for w in wires:
                for pl, ps, (pr, pb) in calls:
                    assert pl(sh.handle, pr, pb, 3, w) == N.GLINT_EINVAL, (dtype, w)
                    assert ps(sh.handle, pr, pb, 3, w, 0) == N.GLINT_EINVAL, (dtype, w)
                    assert pl(sh.handle, pr, pb, 0, w) == N.GLINT_EINVAL  # also with nothing to do
            sh.sync()
            np.testing.assert_array_equal(sh.to_numpy(), before)
    table = np.full((10, cols), 2.0, np.float32)
    with shard("range", cols, "float", gpu, table, size=10) as sh:
        h = sh.handle
        for pl, ps, (pr, pb) in calls:
            for w in (F16, BF16):
                assert pl(h, pr, pb, -1, w) == N.GLINT_EINVAL
                assert pl(h, pr, pb, 1 << 31, w) == N.GLINT_EINVAL
                assert pl(h, None, pb, 3, w) == N.GLINT_EINVAL
                assert pl(h, pr, None, 3, w) == N.GLINT_EINVAL
                assert ps(h, pr, pb, -1, w, 0) == N.GLINT_EINVAL
                assert ps(h, pr, pb, (1 << 32) - 2048, w, 0) == N.GLINT_EINVAL
                assert ps(h, None, pb, 3, w, 0) == N.GLINT_EINVAL
                assert ps(h, pr, None, 3, w, 0) == N.GLINT_EINVAL
                assert ps(h, pr, pb, 3, w, N.GLINT_PUSH_VALIDATE) == N.GLINT_EINVAL
                assert ps(h, pr, pb, 3, w, 8) == N.GLINT_EINVAL  # unknown flag bit
                assert pl(h, None, None, 0, w) == N.GLINT_OK      # n == 0 launches nothing
                assert ps(h, None, None, 0, w, 0) == N.GLINT_OK
        sh.sync()
        np.testing.assert_array_equal(image(sh, gpu)[0], table)  # none of them changed the shard
        # the wrapper: a values dtype that does not match the wire type, shapes, mixing host and device
        v16 = np.ones((3, cols), np.float16)
        for vals, wire in ((v16, "bfloat16"), (v16.astype(np.float32), "float16"), (v16.view(np.uint16), "float16"),
                           (v16.astype(np.float64), "float16"), (np.ones((2, cols), np.float16), "float16"),
                           (np.ones((3, cols + 1), np.float16), "float16"), (v16, "half")):
            with pytest.raises(ValueError):
                sh.updateRowsAs(r, vals, wire)
        with pytest.raises(ValueError):
            sh.updateRowsAs(rd, to_dev(gpu, v16, "float16"), "bfloat16")
        with pytest.raises(ValueError):
            sh.updateRowsAs(rd, dev_t(gpu, v16.astype(np.float32)), "float16")
        with pytest.raises(ValueError):
            sh.updateRowsAs(r, v16.astype(np.float32), "float32")  # a pair the library refuses
        with pytest.raises(ValueError):
            sh.getRowsAs(r, "float32")
        for args in ((rd, v16, "float16"), (r, to_dev(gpu, v16, "float16"), "float16")):
            with pytest.raises(TypeError):
                sh.updateRowsAs(*args)
        with pytest.raises(ValueError):
            sh.getRowsAs(r, "float16", out=np.zeros((3, cols), np.float32))
        with pytest.raises(ValueError):
            sh.getRowsAs(r, "float16", out=np.zeros((2, cols), np.float16))
        np.testing.assert_array_equal(image(sh, gpu)[0], table)
        assert sh.updateRowsAs(r, v16, "float16")
        assert sh.updateRowsAs(rd, to_dev(gpu, v16.reshape(-1), "float16"), "float16")
        want = table.copy()
        want[0] += 4
        want[1] += 2
        np.testing.assert_array_equal(image(sh, gpu)[0], want)
        assert (sh.getRowsAs(r[:2], "float16") == np.array([[6.0] * cols, [4.0] * cols], np.float16)).all()


def test_a_slab_with_views_is_refused_on_the_host(gpu):
    slab = PartialMatrix(RangePartition(0, 0, 128), 4, "float", gpu)
    view = PartialMatrix.view(slab, RangePartition(0, START, START + 64), 0)
    try:
        r, v = np.array([3], np.int64), np.ones((1, 4), np.float16)
        with pytest.raises(ValueError):
            slab.updateRowsAs(r, v, "float16")
        with pytest.raises(ValueError):
            slab.getRowsAs(r, "float16")
        assert view.updateRowsAs(r + START, v, "float16")  # the view itself is a shard like any other
        assert (view.getRowsAs(r + START, "float16") == np.float16(1.0)).all()
        assert (from_dev(slab.getRowsAs(dev_t(gpu, r), "bfloat16"), "bfloat16") == 0x3F80).all()  # device calls pass
    finally:
        view.destroy()
        slab.destroy()


ERROR_CASES = [("float", "float16", 8), ("float", "bfloat16", 67), ("double", "float32", 6)]


def _error_input(dtype, wire, cols):
    local, vals, table, wide, _, _, _ = push_case(dtype, wire, cols, "zipf")
    rows = np.array(keys_of("range", local))
    rows[7] = START - 1
    rows[60] = START + SIZE
    return local, rows, vals, wide, table


@pytest.mark.parametrize("dtype,wire,cols", ERROR_CASES)
def test_out_of_range_rows_host(gpu, dtype, wire, cols):
    _, rows, vals, _, table = _error_input(dtype, wire, cols)
    with shard("range", cols, dtype, gpu, table) as sh:
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.updateRowsAs(rows, vals, wire)
        assert ei.value.record == 7  # the lowest
        out = np.full((rows.size, cols), 7, NPW[wire])
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.getRowsAs(rows, wire, out=out)
        assert ei.value.record == 7
        assert (out == 7).all()  # out untouched
        np.testing.assert_array_equal(bits(image(sh, gpu)[0]), bits(table))  # a rejected message applies nothing


@pytest.mark.parametrize("dtype,wire,cols", ERROR_CASES)
def test_out_of_range_rows_device(gpu, dtype, wire, cols):
    local, rows, vals, wide, table = _error_input(dtype, wire, cols)
    keep = np.ones(local.size, bool)
    keep[[7, 60]] = False
    with shard("range", cols, dtype, gpu, table) as sh:
        buf, out = offset_buffer(gpu, wire, rows.size * cols, 0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.getRowsAs(dev_t(gpu, rows), wire, out=out.view(rows.size, cols))
        assert ei.value.record == 7
        got = from_dev(out, wire).reshape(rows.size, cols)
        assert (bits(got[~keep]) == 0).all()  # answered with zero bits
        assert_wire_bits(got[keep], ref_narrow(table[local[keep]], wire), wire)  # the other rows are served
        assert sentinel_intact(buf, wire, 0, rows.size * cols)
    want = fold_rows(table, local[keep], wide[keep])
    mag = np.abs(table.astype(np.float64))
    np.add.at(mag, local[keep], np.abs(wide[keep].astype(np.float64)))
    terms = np.ones(SIZE, np.int64)
    np.add.at(terms, local[keep], 1)
    for det in (False, True):
        with shard("range", cols, dtype, gpu, table) as sh:
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                sh.updateRowsAs(dev_t(gpu, rows), to_dev(gpu, vals, wire), wire, deterministic=det)
            assert ei.value.record == 7
            got = image(sh, gpu)[0]
            if det:
                assert_bits(got, want)  # the other records were applied
            else:
                assert_bits(got[terms <= 2], want[terms <= 2])
                A.check(got, want, mag, terms, dtype, False)


# ---- 6. launch accounting -------------------------------------------------------------------------------------
def _counts(sh):
    out = []
    for kid in range(N.GLINT_K_COUNT):
        ms, cnt = C.c_double(), C.c_int64()
        assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
        out.append(cnt.value)
    return np.array(out)


@pytest.mark.parametrize("path", ["host", "dev", "dev_det"])
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_launch_accounting(gpu, dtype, wire, path):
    cols = 67
    local, vals, table, wide, _, _, _ = push_case(dtype, wire, cols, "hot")
    rows = keys_of("range", local)
    where = "host" if path == "host" else "dev"
    with shard("range", cols, dtype, gpu, table) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        one = lambda kid: np.eye(N.GLINT_K_COUNT, dtype=np.int64)[kid]  # noqa: E731
        c0 = _counts(sh)
        row_push(sh, gpu, rows, wide, path)
        front = _counts(sh) - c0 - one(N.GLINT_K_PUSH_ROWS)  # what the row push records for its front end
        assert (front >= 0).all()
        before = _counts(sh)
        push(sh, gpu, rows, vals, wire, path)
        np.testing.assert_array_equal(_counts(sh) - before, front + one(N.GLINT_K_PUSH_ROWS))
        before = _counts(sh)
        pull(sh, gpu, rows, wire, where)
        np.testing.assert_array_equal(_counts(sh) - before, one(N.GLINT_K_MAT_PULL_ROWS))  # one launch, none elsewhere
        before = _counts(sh)
        z = np.zeros(0, np.int64)
        if where == "host":
            assert sh.getRowsAs(z, wire).shape == (0, cols) and sh.updateRowsAs(z, np.zeros((0, cols), NPW[wire]), wire)
        else:
            assert sh.getRowsAs(dev_t(gpu, z), wire).shape == (0, cols)
            assert sh.updateRowsAs(dev_t(gpu, z), to_dev(gpu, np.zeros((0, cols), NPW[wire]), wire), wire)
        np.testing.assert_array_equal(_counts(sh), before)  # n == 0 launches nothing


# ---- 7. sequence ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,wire,cols",
                         [("float", "float16", 128), ("float", "bfloat16", 67), ("double", "float32", 136)])
def test_calls_in_sequence(gpu, dtype, wire, cols):
    """A device updateRowsAs (not waited for), a host getRowsAs, a host updateRows, on one shard in that order,
    against the numpy replay of the three steps."""
    local, vals, table, wide, want1, _, _ = push_case(dtype, wire, cols, "hot")
    rows = keys_of("cyclic", local)
    every = keys_of("cyclic", np.arange(SIZE))
    more = np.array(table[::-1])
    with shard("cyclic", cols, dtype, gpu, table) as sh:
        assert sh.updateRowsAs(dev_t(gpu, rows), to_dev(gpu, vals, wire), wire, deterministic=True, sync=False)
        narrow = sh.getRowsAs(every, wire)
        assert sh.updateRows(every, more)
        got, pad = image(sh, gpu)
        sh.sync()
    assert_wire_bits(narrow, ref_narrow(want1, wire), wire)
    assert_bits(got, np.add(want1, more, dtype=NPV[dtype]))
    check_padding(pad, dtype)


# ---- 8. BigMatrix over 3 partitions on one GPU ----------------------------------------------------------------
@pytest.mark.parametrize("make", [RangePartitioner.apply, CyclicPartitioner.apply])
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_big_matrix_equals_one_shard(gpu, dtype, wire, make):
    cols = 67
    local, vals, table, wide, want, _, _ = push_case(dtype, wire, cols, "zipf")
    partitioner = make(3, SIZE)
    shards = [PartialMatrix(p, cols, dtype, gpu) for p in partitioner.all()]
    M = BigMatrix(partitioner, shards, SIZE, cols)
    one = PartialMatrix(RangePartition(0, 0, SIZE), cols, dtype, gpu)
    try:
        every = np.arange(SIZE, dtype=np.int64)
        assert M.pushRows(every, table) and one.updateRows(every, table)
        assert M.pushRowsAs(local, vals, wire) and one.updateRowsAs(local, vals, wire)
        assert_bits(M.pull(every), want)
        assert_bits(one.getRows(every), want)
        ask = requests(700).astype(np.int64)
        got = M.pullRowsAs(ask, wire)
        assert_wire_bits(got, one.getRowsAs(ask, wire), wire)
        assert_wire_bits(got, ref_narrow(want[ask], wire), wire)
    finally:
        M.destroy()
        one.destroy()
