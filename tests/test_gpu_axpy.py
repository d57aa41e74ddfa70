"""Row axpy push (PartialMatrix.updateRowsAxpy, glint_mat_push_rows_axpy*) against the oracle.

The call is defined as the row push of the contribution rows t_i = ((coef[i][0] * x[0]) + (coef[i][1] *
x[1])) + ..., so the oracle is given the expanded triplets of axpy_cases.replay_contrib.

Bar: bit-exact for Int/Long everywhere, for every host-array and every deterministic push, and for the
device default whenever no row repeats inside a push. Device default with repeated rows: Double within
1e-9 of the element's sum |t| (tests/test_gpu_rows.py's bar); Float within the format's own bound: any
order of N float additions is within (N - 1) * 2^-24 * sum |t| of the exact sum, so two orders differ by
at most twice that (N: the element's number of terms over the two pushes).
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, Client, PartialMatrix, PartialVector, RangePartition
from oracle import oracle as O
from axpy_cases import assert_bits, axpy_inputs, bits, fold_rows, nofma_element, nofma_inner, replay_contrib
from ieee_cases import write_image
import test_gpu_rows as R  # the sort ladder's case builders

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
START, SIZE = 1_000_003, 1500
QMAX = N.GLINT_AXPY_MAX_VECTORS
PATTERNS = ["sorted_once", "permutation", "duplicates", "one_row", "single", "empty"]
REPEATS = ("duplicates", "one_row")
PATHS = ["host", "dev", "dev_det"]


def npd_of(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def make_rows(rng, pattern):
    if pattern == "sorted_once":
        return np.arange(START, START + SIZE, dtype=np.int64)
    if pattern == "permutation":
        return rng.permutation(SIZE).astype(np.int64) + START
    if pattern == "duplicates":
        return rng.choice(rng.choice(SIZE, 40, replace=False), 3000).astype(np.int64) + START
    if pattern == "one_row":  # crosses the sort's 2048-key tile, the 64-id batch and the split length
        return np.full(2100, START + 777, np.int64)
    if pattern == "single":
        return np.array([START + 17], np.int64)
    return np.zeros(0, np.int64)


def oracle_apply(ref, rows, values, cols):
    """The expansion that defines a row push."""
    n = rows.size
    bad = ref.update(np.repeat(rows, cols), np.tile(np.arange(cols, dtype=np.int32), n), values.reshape(-1))
    assert bad == -1


@functools.lru_cache(maxsize=None)
def case(dtype, cols, q, pattern):
    """(rows, coef, x, the oracle's shard after the push applied twice, sum |t| per element, terms per
    element): computed once and shared by the three paths; read-only."""
    rng = np.random.default_rng(zlib.crc32(f"axpy/{dtype}/{cols}/{q}/{pattern}".encode()))
    rows = make_rows(rng, pattern)
    coef, x = axpy_inputs(np.dtype(npd_of(dtype)).name, rows.size, q, cols)
    t = replay_contrib(coef, x)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE[dtype])
    for _ in range(2):
        oracle_apply(ref, rows, t, cols)
    mag = np.zeros((SIZE, cols), np.float64)
    terms = np.zeros(SIZE, np.int64)
    np.add.at(terms, rows - START, 2)
    if np.issubdtype(t.dtype, np.floating):
        with np.errstate(invalid="ignore", over="ignore"):
            np.add.at(mag, rows - START, 2.0 * np.abs(t.astype(np.float64)))
    for a in (rows, ref.data, mag, terms):
        a.setflags(write=False)
    return rows, coef, x, ref.data, mag, terms


def push(sh, gpu, rows, coef, x, path):
    if path == "host":
        assert sh.updateRowsAxpy(rows, coef, x)
        return
    import torch
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    assert sh.updateRowsAxpy(t(rows), t(coef), t(x), deterministic=(path == "dev_det"))


def check(got, ref, mag, terms, dtype, exact):
    if exact:
        np.testing.assert_array_equal(got, ref)
        return
    err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
    if dtype == "double":
        bound = 1e-9 * mag
    else:
        bound = 2.0 * np.maximum(terms - 1, 0)[:, None] * 2.0 ** -24 * mag
    assert not (err > bound).any(), f"max excess {np.max(err - bound)}"


# every instance: q 1 / 2..4 / blocked (5: one partial tile; max: full tiles), the 16-B slice (cols 128), the
# scalar slice (3, 67: less than and more than one slice), over the runs that repeat
CORE = {(dt, c, q, pat) for dt in DT for c in (3, 67, 128) for q in (1, 4, 5, QMAX) for pat in REPEATS}
# the other patterns, sizes and q = 2 on a thinner grid
WIDE = {(dt, c, q, pat) for dt, c, q in (("double", 1, 2), ("float", 513, 5), ("long", 513, 4), ("int", 1, 1),
                                         ("double", 130, 2), ("double", 513, 1), ("double", 67, 5),
                                         ("float", 128, 4), ("int", 3, QMAX), ("long", 128, 2))
        for pat in PATTERNS}
GRID = sorted(CORE | WIDE)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("dtype,cols,q,pattern", GRID)
def test_axpy_push_parity(gpu, dtype, cols, q, pattern, path):
    rows, coef, x, ref, mag, terms = case(dtype, cols, q, pattern)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        for _ in range(2):  # the second push accumulates onto non-zero state
            push(sh, gpu, rows, coef, x, path)
        got = sh.to_numpy()
    exact = dtype in ("long", "int") or path != "dev" or pattern not in REPEATS
    check(got, ref, mag, terms, dtype, exact)


@pytest.mark.parametrize("path", ["host", "dev_det"])
@pytest.mark.parametrize("dtype,cols,q", [("double", 67, 5), ("float", 128, 4), ("double", 128, 1)])
def test_axpy_equals_row_push_of_the_replay(gpu, dtype, cols, q, path):
    import torch
    rows, coef, x, _, _, _ = case(dtype, cols, q, "duplicates")
    t = replay_contrib(coef, x)
    d = torch.device("cuda", gpu)
    part = RangePartition(2, START, START + SIZE)
    with PartialMatrix(part, cols, dtype, gpu) as a, PartialMatrix(part, cols, dtype, gpu) as b:
        for _ in range(2):
            push(a, gpu, rows, coef, x, path)
            if path == "host":
                b.updateRows(rows, t)
            else:
                b.updateRows(torch.from_numpy(np.array(rows)).to(d), torch.from_numpy(t).to(d), deterministic=True)
        assert_bits(a.to_numpy(), b.to_numpy())


# ---- the sort's geometry ------------------------------------------------------------------------------
@pytest.mark.parametrize("q", [1, 5])
@pytest.mark.parametrize("size", R.SORT_SIZES[:-1])
def test_axpy_push_sort_passes(gpu, size, q):
    """The row push's ladder of shard sizes (test_gpu_rows.sort_rows: one to three passes of the shared
    sort, either buffer pair, the runs of RUNS): the axpy fold reads the sorted rows from whichever buffer
    the sort ended in. Long on every path, Double with deterministic=True; three pushes onto one shard,
    two records outside on the device paths. Expected: fold_rows over the replayed contributions."""
    import torch
    d = torch.device("cuda", gpu)
    t = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    cols = R.sort_cols(size)
    for dtype, path in (("long", "host"), ("long", "dev"), ("long", "dev_det"), ("double", "dev_det")):
        npd = npd_of(dtype)
        rng = np.random.default_rng(zlib.crc32(f"axpy/sort/{size}/{q}/{dtype}/{path}".encode()))
        want = np.zeros((size, cols), npd)
        with PartialMatrix(RangePartition(2, START, START + size), cols, dtype, gpu) as sh:
            for n in R.SORT_N:
                local, _, _ = R.sort_rows(rng, size, n, path != "host")
                coef, x = axpy_inputs(np.dtype(npd).name, n, q, cols, f"sort/{size}/{path}")
                inside = (local >= 0) & (local < size)
                want = fold_rows(want, local[inside], replay_contrib(coef[inside], x))
                if path == "host":
                    assert sh.updateRowsAxpy(local + START, coef, x)
                    continue
                with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                    sh.updateRowsAxpy(t(local + START), t(coef), t(x), deterministic=(path == "dev_det"))
                assert ei.value.record == int(np.flatnonzero(~inside)[0])
            assert_bits(sh.to_numpy(), want)


# ---- no fused multiply-add ---------------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("run", [1, 3])
@pytest.mark.parametrize("dtype,cols", [("double", 2), ("double", 67), ("float", 4), ("float", 67)])
def test_axpy_is_unfused(gpu, dtype, cols, run, path):
    """-b + a * a is exactly +0 with a rounded product and 2^-54 / 2^-24 fused; (1 * -b) + (a * a)
    likewise. As a single record, and as the middle record of a run of three for one row (the others
    with zero coefficients)."""
    npd = npd_of(dtype)
    c = cols - 1 if cols > 4 else 1  # columns 66 (the second slice of the scalar path), 1
    row = np.full(run, START + 5, np.int64)
    mid = run // 2
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        elem, coef1, x, fused = nofma_element(npd, cols, c)
        coef = np.zeros((run, 1), npd)
        coef[mid] = coef1[0]
        sh.updateRows(row[:1], elem[None])  # the element: -b
        assert sh.to_numpy()[5, c] == elem[c] != 0
        push(sh, gpu, row, coef, x, path)
        got = sh.to_numpy()[5]
        assert bits(got)[c] == 0, f"{got[c]!r}: a fused product would leave {fused!r}"
        assert not got.any()
        coef2, x2, fused = nofma_inner(npd, cols, c)
        coef = np.zeros((run, 2), npd)
        coef[mid] = coef2[0]
        push(sh, gpu, row, coef, x2, path)
        got = sh.to_numpy()[5]
        assert bits(got)[c] == 0, f"{got[c]!r}: a fused product would leave {fused!r}"


# ---- the bits do not depend on the alignment of x or coef ---------------------------------------------
@pytest.mark.parametrize("q", [4, 5])
def test_axpy_path_independence(gpu, q):
    import torch
    cols = 128
    rows, coef, x, ref, _, _ = case("double", cols, q, "duplicates")
    d = torch.device("cuda", gpu)
    t_rows = torch.from_numpy(np.array(rows)).to(d)

    def shifted(a):  # the same values one element into a buffer: 8-B aligned only
        buf = torch.zeros(a.size + 3, dtype=torch.float64, device=d)
        v = buf[1:1 + a.size]
        v.copy_(torch.from_numpy(np.array(a)).to(d).view(-1))
        assert v.data_ptr() % 16 == 8 and v.is_contiguous()
        return v.view(a.shape)

    aligned = lambda a: torch.from_numpy(np.array(a)).to(d)  # noqa: E731
    for cx, cc in ((shifted, aligned), (aligned, shifted), (shifted, shifted)):
        with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "double", gpu) as sh:
            tx, tc = cx(x), cc(coef)
            for _ in range(2):
                sh.updateRowsAxpy(t_rows, tc, tx, deterministic=True)
            np.testing.assert_array_equal(sh.to_numpy(), ref)


# ---- IEEE edges -----------------------------------------------------------------------------------------
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
def test_axpy_ieee_edges(gpu, dtype, cols, path):
    """Subnormal products kept, inf * 0 is NaN, a -0.0 product, and the pitch padding neither read nor
    written; each against the replay, a NaN by class."""
    npd = npd_of(dtype)
    small = (2.0 ** -540, 2.0 ** -520) if dtype == "double" else (2.0 ** -70, 2.0 ** -70)
    x = np.zeros((2, cols), npd)
    x[0, :] = small[1]   # times small[0]: a subnormal product
    x[1, 0] = np.inf     # times 0: NaN
    x[1, 1] = 0.0        # times -1: -0.0
    x[1, 2:] = 1.0
    coef = np.array([[small[0], 0.0], [small[0], -1.0], [3.0, 0.0], [0.0, -0.0], [small[0], small[0]]], npd)
    rows = np.array([START, START + 1, START + 1, START + 2, START + 2], np.int64)
    t = replay_contrib(coef, x)
    assert t[0, 1] != 0 and abs(t[0, 1]) < np.finfo(npd).tiny and np.isnan(t[0, 0])  # the premises
    assert bits(np.multiply(coef[1, 1], x[1, 1], dtype=npd)) == bits(npd(-0.0))
    img = np.zeros((3, cols), npd)
    img[2] = -0.0
    exp = img.copy()
    with np.errstate(invalid="ignore", under="ignore"):
        for i, r in enumerate(rows - START):
            exp[r] = exp[r] + t[i]
    pad = npd(777.0)
    with PartialMatrix(RangePartition(2, START, START + 3), cols, dtype, gpu) as sh:
        write_image(sh, gpu, img, pad)
        push(sh, gpu, rows, coef, x, path)
        pitch = C.c_int64()
        assert N.load().glint_shard_pitch(sh.handle, C.byref(pitch)) == N.GLINT_OK
        raw = read_image(sh, gpu, 3, pitch.value)
        assert_bits(raw[:, :cols], exp)
        assert (pitch.value > cols) == (cols == 67)  # only a row that is no multiple of 16 B is padded
        assert (raw[:, cols:] == pad).all()  # neither read (no NaN, no sum) nor written


# ---- skew -------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def skew_case(dtype):
    """20 000 records over 3 rows plus 500 rows once each, shuffled: runs far past the split length."""
    cols, q = 64, 2
    rng = np.random.default_rng(77)
    picks = rng.choice(SIZE, 503, replace=False)
    rows = np.concatenate([rng.choice(picks[:3], 20_000), picks[3:]]).astype(np.int64) + START
    rng.shuffle(rows)
    npd = npd_of(dtype)
    if dtype == "double":
        coef, x = rng.uniform(-1, 1, (rows.size, q)), rng.uniform(-1, 1, (q, cols))
    else:
        info = np.iinfo(npd)
        coef = rng.integers(info.min, info.max, (rows.size, q), dtype=npd, endpoint=True)
        x = rng.integers(info.min, info.max, (q, cols), dtype=npd, endpoint=True)
    t = replay_contrib(coef, x)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE[dtype])
    for _ in range(2):
        oracle_apply(ref, rows, t, cols)
    mag = np.zeros((SIZE, cols), np.float64)
    if dtype == "double":
        np.add.at(mag, rows - START, 2.0 * np.abs(t))
    return cols, rows, coef, x, ref.data, mag


@pytest.mark.parametrize("dtype,det", [("long", False), ("double", False), ("double", True)])
def test_axpy_push_skew(gpu, dtype, det):
    """Long: a lost or doubled chunk of a split run cannot pass. Double default: within 1e-9 of sum |t|
    (the oracle's own sequential sum of ~6 700 terms is within 6 700 x 2^-53 ~ 7e-13 of exact). Double
    deterministic: nothing is split, bit-exact."""
    import torch
    cols, rows, coef, x, ref, mag = skew_case(dtype)
    assert rows.size == 20_500
    d = torch.device("cuda", gpu)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        r, c, v = torch.from_numpy(rows).to(d), torch.from_numpy(coef).to(d), torch.from_numpy(x).to(d)
        for _ in range(2):
            sh.updateRowsAxpy(r, c, v, deterministic=det)
        check(sh.to_numpy(), ref, mag, None, dtype, dtype == "long" or det)


# ---- errors and arguments -------------------------------------------------------------------------------
def _error_input(rng):
    cols, q = 6, 3
    rows = rng.integers(START, START + SIZE, 100).astype(np.int64)
    rows[7] = START - 1
    rows[60] = START + SIZE
    coef = rng.integers(-10**6, 10**6, (100, q)).astype(np.int64)
    x = rng.integers(-10**6, 10**6, (q, cols)).astype(np.int64)
    return cols, rows, coef, x


def test_axpy_push_errors_device(gpu):
    import torch
    cols, rows, coef, x = _error_input(np.random.default_rng(3))
    d = torch.device("cuda", gpu)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["long"])
    keep = np.ones(100, bool)
    keep[[7, 60]] = False
    oracle_apply(ref, rows[keep], replay_contrib(coef[keep], x), cols)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.updateRowsAxpy(torch.from_numpy(rows).to(d), torch.from_numpy(coef).to(d), torch.from_numpy(x).to(d))
        assert ei.value.record == 7
        np.testing.assert_array_equal(sh.to_numpy(), ref.data)  # the other 98 rows were applied


def test_axpy_push_errors_host(gpu):
    cols, rows, coef, x = _error_input(np.random.default_rng(3))
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        ok = np.arange(START, START + 50, dtype=np.int64)
        sh.updateRowsAxpy(ok, np.full(50, 9, np.int64), np.ones(cols, np.int64))
        before = sh.to_numpy().copy()
        assert (before[:50] == 9).all()
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.updateRowsAxpy(rows, coef, x)
        assert ei.value.record == 7
        np.testing.assert_array_equal(sh.to_numpy(), before)  # a rejected message applies nothing


def test_axpy_push_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    c = np.ones(2, np.float64)
    x = np.ones(8, np.float64)
    rd, cd, xd = torch.from_numpy(r).to(d), torch.from_numpy(c).to(d), torch.from_numpy(x).to(d)
    host = lib.glint_mat_push_rows_axpy
    devc = lambda *args: lib.glint_mat_push_rows_axpy_dev(*args, None)  # noqa: E731
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        assert host(vec.handle, r.ctypes.data, 1, c.ctypes.data, x.ctypes.data, 2, 0) == N.GLINT_EINVAL
        assert devc(vec.handle, rd.data_ptr(), 1, cd.data_ptr(), xd.data_ptr(), 2, 0) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        h = sh.handle
        for call, (pr, pc, px) in ((host, (r.ctypes.data, c.ctypes.data, x.ctypes.data)),
                                   (devc, (rd.data_ptr(), cd.data_ptr(), xd.data_ptr()))):
            assert call(h, pr, 1, pc, px, 2, N.GLINT_PUSH_VALIDATE) == N.GLINT_EINVAL
            assert call(h, pr, 1, pc, px, 2, 8) == N.GLINT_EINVAL  # unknown flag bit
            assert call(h, pr, -1, pc, px, 2, 0) == N.GLINT_EINVAL
            assert call(h, pr, (1 << 32) - 2048, pc, px, 2, 0) == N.GLINT_EINVAL
            assert call(h, pr, 1, pc, px, 0, 0) == N.GLINT_EINVAL
            assert call(h, pr, 1, pc, px, QMAX + 1, 0) == N.GLINT_EINVAL
            assert call(h, None, 1, pc, px, 2, 0) == N.GLINT_EINVAL
            assert call(h, pr, 1, None, px, 2, 0) == N.GLINT_EINVAL
            assert call(h, pr, 1, pc, None, 2, 0) == N.GLINT_EINVAL
            assert call(h, None, 0, None, None, 2, 0) == N.GLINT_OK
        assert not sh.to_numpy().any()
        for bad_c, bad_x in ((c[:1], x[:7]), (c[:1], x.reshape(2, 4)), (np.ones((1, 3)), x.reshape(2, 4)),
                             (c.reshape(2, 1), x[:4]), (np.ones((1, QMAX + 1)), np.ones((QMAX + 1, 4))),
                             (np.ones((1, 0)), np.ones((0, 4)))):
            with pytest.raises(ValueError):  # a shape mismatch: no call is made
                sh.updateRowsAxpy(r, bad_c, bad_x)
        with pytest.raises(ValueError):
            sh.updateRowsAxpy(rd, cd, xd.view(2, 4))  # coef (2,) is not (1, 2)
        with pytest.raises(TypeError):
            sh.updateRowsAxpy(rd, cd.view(1, 2), x.reshape(2, 4))  # x on the host
        with pytest.raises(TypeError):
            sh.updateRowsAxpy(rd, cd.view(1, 2).to(torch.float32), xd.view(2, 4))
        assert not sh.to_numpy().any()
        assert sh.updateRowsAxpy(r, c.reshape(1, 2), x.reshape(2, 4))
        assert sh.updateRowsAxpy(rd, cd.view(1, 2), xd.view(2, 4))
        assert sh.updateRowsAxpy(r, c[:1], x[:4]) and sh.updateRowsAxpy(rd, cd[:1].view(1, 1), xd[:4])
        np.testing.assert_array_equal(sh.to_numpy()[0], np.full(4, 6.0))


# ---- launch count, stream order, client -------------------------------------------------------------------
def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_axpy_push_profiling_id(gpu):
    import torch
    d = torch.device("cuda", gpu)
    rows = np.arange(START, START + 100, dtype=np.int64)
    with PartialMatrix(RangePartition(2, START, START + SIZE), 4, "double", gpu) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        sh.update(rows, np.zeros(100, np.int32), np.ones(100))
        sh.updateRows(rows, np.ones((100, 4)))
        assert _launches(sh, N.GLINT_K_PUSH_ROWS_AXPY) == 0  # neither is an axpy push
        sh.updateRowsAxpy(rows, np.ones(100), np.ones(4))
        assert _launches(sh, N.GLINT_K_PUSH_ROWS_AXPY) == 1  # one call, one launch under the id
        before = _launches(sh, N.GLINT_K_PUSH_ROWS)
        t = lambda a: torch.from_numpy(a).to(d)  # noqa: E731
        sh.updateRowsAxpy(t(rows), t(np.ones((100, 5))), t(np.ones((5, 4))))
        sh.updateRowsAxpy(t(np.repeat(rows, 30)), t(np.ones((3000, 2))), t(np.ones((2, 4))), deterministic=True)
        assert _launches(sh, N.GLINT_K_PUSH_ROWS_AXPY) == 3
        sh.updateRowsAxpy(rows[:0], np.ones((0, 2)), np.ones((2, 4)))  # an empty call launches nothing
        assert _launches(sh, N.GLINT_K_PUSH_ROWS_AXPY) == 3 and _launches(sh, N.GLINT_K_PUSH_ROWS) == before
        want = np.full((100, 4), 1.0 + 1 + 5 + 60)  # the row push and the three axpy pushes
        want[:, 0] += 1  # the element push
        np.testing.assert_array_equal(sh.to_numpy()[:100], want)
        assert _launches(sh, N.GLINT_K_PUSH_ROWS) == before


def test_axpy_push_stream_order(gpu):
    """An axpy push, an element push, an axpy push and a row pull on one stream, one sync at the end."""
    import torch
    cols = 9
    rng = np.random.default_rng(21)
    d = torch.device("cuda", gpu)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["long"])
    big = lambda *shape: rng.integers(-2**62, 2**62, shape).astype(np.int64)  # noqa: E731
    r1, c1, x1 = rng.integers(START, START + 200, 700).astype(np.int64), big(700, 3), big(3, cols)
    er = rng.integers(START, START + 200, 1000).astype(np.int64)  # the same rows, by element
    ec = rng.integers(0, cols, 1000).astype(np.int32)
    ev = big(1000)
    r2, c2, x2 = rng.integers(START + 100, START + 300, 900).astype(np.int64), big(900, 6), big(6, cols)
    q = np.arange(START, START + 300, dtype=np.int64)
    t = lambda a: torch.from_numpy(a).to(d)  # noqa: E731
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        dev = [t(a) for a in (r1, c1, x1, er, ec, ev, r2, c2, x2, q)]
        sh.updateRowsAxpy(dev[0], dev[1], dev[2], sync=False)
        sh.update(dev[3], dev[4], dev[5], sync=False)
        sh.updateRowsAxpy(dev[6], dev[7], dev[8], sync=False)
        out = sh.getRows(dev[9], sync=False)
        sh.sync(sh._stream_of(dev[9]))
        oracle_apply(ref, r1, replay_contrib(c1, x1), cols)
        assert ref.update(er, ec, ev) == -1
        oracle_apply(ref, r2, replay_contrib(c2, x2), cols)
        np.testing.assert_array_equal(out.cpu().numpy(), ref.data[:300])


def test_axpy_push_client(gpu):
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 1000, 5000).astype(np.int64)
    coef = rng.integers(-10**6, 10**6, (5000, 3)).astype(np.int64)
    x = rng.integers(-10**6, 10**6, (3, 7)).astype(np.int64)
    m = Client([gpu] * 3).matrix(1000, 7, "long", modelsPerServer=2)
    assert m.nrOfPartitions == 6
    m.pushAxpy(rows, coef, x)
    want = np.zeros((1000, 7), np.int64)
    np.add.at(want, rows, coef @ x)
    np.testing.assert_array_equal(m.pull(np.arange(1000)), want)
    m.destroy()
