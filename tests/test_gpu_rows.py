"""Whole-row matrix push (PartialMatrix.updateRows, glint_mat_push_rows*) against the oracle.

The reference has no row-push message; its semantics are PartialMatrix.update (PartialMatrix.scala:74-83)
applied to the expanded triplets (rows[i], c, values[i][c]), i in order and c in [0, cols) inside each
i -- which is what the oracle is given here.

Bar: bit-exact for Int/Long everywhere, for every host-array and every deterministic push, and for the
device default whenever no row repeats inside a push. Device default with repeated rows: Double within
1e-9 of the element's sum |v| (tests/test_gpu_wide.py's bar); Float rtol 1e-4 / atol 2e-3 at up to 400
values per element (tests/test_gpu_parity.py's bar). The one Float case with more values per element
(`one_row`: 2 x 2100) is held to the format's own bound instead: any order of N float additions is
within (N - 1) * 2^-24 * sum |v| of the exact sum, so two orders differ by at most twice that.
"""
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, Client, CyclicPartition, PartialMatrix, PartialVector, \
    RangePartition
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
START, SIZE = 1_000_003, 1500
PATTERNS = ["sorted_once", "permutation", "duplicates", "one_row", "single", "empty"]
REPEATS = ("duplicates", "one_row")
PATHS = ["host", "dev", "dev_det"]


def rand_vals(rng, dtype, n):
    npd = glint_amd.shard.resolve_dtype(dtype)[1]
    if np.issubdtype(npd, np.floating):
        return rng.uniform(-1, 1, n).astype(npd)
    info = np.iinfo(npd)
    return rng.integers(info.min, info.max, n, dtype=npd, endpoint=True)


def make_rows(rng, pattern):
    if pattern == "sorted_once":
        return np.arange(START, START + SIZE, dtype=np.int64)
    if pattern == "permutation":
        return rng.permutation(SIZE).astype(np.int64) + START
    if pattern == "duplicates":
        return rng.choice(rng.choice(SIZE, 40, replace=False), 3000).astype(np.int64) + START
    if pattern == "one_row":  # crosses the sort's 2048-key tile; a long run
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
def case(dtype, cols, pattern):
    """(rows, values, the oracle's shard after the push applied twice, sum |v| per element): computed
    once and shared by the three paths; read-only."""
    rng = np.random.default_rng(zlib.crc32(f"rows/{dtype}/{cols}/{pattern}".encode()))
    rows = make_rows(rng, pattern)
    values = rand_vals(rng, dtype, rows.size * cols).reshape(rows.size, cols)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE[dtype])
    for _ in range(2):
        oracle_apply(ref, rows, values, cols)
    mag = np.zeros((SIZE, cols), np.float64)
    if np.issubdtype(values.dtype, np.floating):
        np.add.at(mag, rows - START, 2.0 * np.abs(values.astype(np.float64)))
    for a in (rows, values, ref.data, mag):
        a.setflags(write=False)
    return rows, values, ref.data, mag


# ---- the sort's geometry and the run shapes, constructed ---------------------------------------------
# rows_front sorts (local row, record index) in ceil(end_bit / 8) passes, end_bit from the sentinel
# `size`, and the result lies in the second buffer pair when that count is odd. SORT_SIZES are the sizes
# at which the count, the buffer, or the sentinel's top bit changes: one pass up to 255 rows, two from 256
# (the sentinel 256 needs bit 8, no valid row does), three from 65 536, four at 2^24 + 1.
# Run lengths around the fold's depth of 8, its batch of 64 record indices, kRowsChunk = 128 and twice that.
RUNS = (1, 2, 3, 7, 8, 9, 63, 64, 65, 127, 128, 129, 255, 256, 257)
SORT_SIZES = [1, 2, 255, 256, 257, 65_535, 65_536, 65_537, (1 << 24) + 1]
SORT_N = (2047, 2048, 2049)  # records of the three pushes onto one shard: around the sort's 2048-key tile
SORT_PASSES = {1: 1, 2: 1, 255: 1, 256: 2, 257: 2, 65_535: 2, 65_536: 3, 65_537: 3, (1 << 24) + 1: 4}


def sort_passes(size):
    """The passes rows_front's sort makes for a shard of `size` rows."""
    end_bit = 1
    while end_bit < 32 and (1 << end_bit) <= size:
        end_bit += 1
    return (end_bit + 7) // 8


def sort_cols(size):
    return 1 if size > 1 << 20 else 3


def sort_rows(rng, size, n, bad):
    """(local rows of one push of n records, the rows that own a run, the runs' lengths). A shard of at
    least 15 rows: runs of RUNS on distinct rows, the first and the last row among them, and fillers on
    other rows -- each once where the shard has rows enough -- shuffled; the record pushed last is the
    last record of the largest row, so it is the last valid record of the sorted list, where the sentinel
    block begins. Fewer rows: every record on the rows there are. `bad`: two more records, local -1 and
    `size`."""
    nb = 2 if bad else 0
    owners, lengths = np.zeros(0, np.int64), np.zeros(0, np.int64)
    if size < len(RUNS):
        local = rng.integers(0, size, n - nb)
    else:
        owners = np.concatenate([[0, size - 1], 1 + rng.choice(size - 2, len(RUNS) - 2, replace=False)]).astype(np.int64)
        lengths = rng.permutation(RUNS)
        fill = n - nb - sum(RUNS)
        if size >= 1 << 15:
            cand = np.setdiff1d(rng.integers(0, size, 4 * fill), owners)
            fillers = rng.permutation(cand)[:fill]
            assert fillers.size == fill
        else:
            fillers = rng.choice(np.setdiff1d(np.arange(size), owners), fill)
        local = np.concatenate([np.repeat(owners, lengths), fillers])
    if bad:
        local = np.concatenate([local, [-1, size]])
    local = local.astype(np.int64)
    rng.shuffle(local)
    if owners.size:
        j = np.flatnonzero(local == size - 1)[-1]
        local[[j, n - 1]] = local[[n - 1, j]]
    assert local.size == n
    return local, owners, lengths


def sort_values(rng, dtype, shape):
    """Long: anywhere in the type, so a lost, doubled or misplaced record cannot cancel. Double: mixed
    magnitudes, 10 ** U(-6, 6) with a sign, so the order of a sum shows."""
    if dtype == "long":
        return rng.integers(-2**63, 2**63 - 1, shape, dtype=np.int64, endpoint=True)
    return rng.choice((-1.0, 1.0), shape) * 10.0 ** rng.uniform(-6, 6, shape)


def run_shows_order(terms):
    """The reversed and the pairwise fold of a run each differ from the sequential one in some column."""
    from rowsum_cases import replay, replay_pairwise, replay_reversed
    seq = replay(terms)
    return bool((seq != replay_reversed(terms)).any() and (seq != replay_pairwise(terms)).any())


def order_shows(local, values):
    """run_shows_order for every run of at least 8 records."""
    rows, counts = np.unique(local, return_counts=True)
    return all(run_shows_order(values[local == r]) for r in rows[counts >= 8])


def sort_case(size, dtype, bad, what="rows"):
    """([(rows, values, lowest index outside or None, local rows)] for the three pushes, the table after
    them: np.add.at over the records inside, in push order). Double: the values of a run of at least 8
    records are drawn again until run_shows_order holds for it, so a fold in another order cannot pass."""
    cols = sort_cols(size)
    rng = np.random.default_rng(zlib.crc32(f"{what}/sort/{size}/{dtype}/{bad}".encode()))
    pushes = []
    for n in SORT_N:
        local, _, _ = sort_rows(rng, size, n, bad)
        values = sort_values(rng, dtype, (n, cols))
        inside = (local >= 0) & (local < size)
        if dtype == "double":
            rows, counts = np.unique(local[inside], return_counts=True)
            for r in rows[counts >= 8]:
                at = np.flatnonzero(local == r)
                for _ in range(200):
                    if run_shows_order(values[at]):
                        break
                    values[at] = sort_values(rng, dtype, (at.size, cols))
                else:
                    raise AssertionError("no draw shows the order")
            assert order_shows(local[inside], values[inside])
        if size >= len(RUNS):  # the sorted list's last valid record is the one pushed last
            assert local[n - 1] == size - 1 == local[inside].max()
        low = int(np.flatnonzero(~inside)[0]) if bad else None
        pushes.append((local + START, values, low, local))
    want = np.zeros((size, cols), values.dtype)
    for _, values, _, local in pushes:
        inside = (local >= 0) & (local < size)
        np.add.at(want, local[inside], values[inside])
    return pushes, want


def same_bits(got, want):
    assert got.dtype == want.dtype and got.shape == want.shape
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))


def push(sh, gpu, rows, values, path):
    if path == "host":
        assert sh.updateRows(rows, values)
        return
    import torch
    d = torch.device("cuda", gpu)
    r = torch.from_numpy(np.array(rows)).to(d)
    v = torch.from_numpy(np.array(values)).to(d)
    assert sh.updateRows(r, v, deterministic=(path == "dev_det"))


def check(got, ref, mag, dtype, exact, per_element):
    if exact:
        np.testing.assert_array_equal(got, ref)
    elif dtype == "double":
        err = np.abs(got - ref)
        assert not (err > 1e-9 * mag).any(), f"max excess {np.max(err - 1e-9 * mag)}"
    elif per_element <= 400:
        np.testing.assert_allclose(got, ref, rtol=1e-4, atol=2e-3)
    else:
        err = np.abs(got.astype(np.float64) - ref.astype(np.float64))
        bound = 2.0 * (per_element - 1) * 2.0 ** -24 * mag
        assert not (err > bound).any(), f"max excess {np.max(err - bound)}"


GRID = [(dt, c) for dt in DT for c in (1, 3, 128, 513)] + [("double", 130)]


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("dtype,cols", GRID)
def test_row_push_parity(gpu, dtype, cols, pattern, path):
    rows, values, ref, mag = case(dtype, cols, pattern)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        for _ in range(2):  # the second push accumulates onto non-zero state
            push(sh, gpu, rows, values, path)
        got = sh.to_numpy()
    exact = dtype in ("long", "int") or path != "dev" or pattern not in REPEATS
    per_element = 2 * (rows.size if pattern == "one_row" else 75)
    check(got, ref, mag, dtype, exact, per_element)


def test_row_push_cyclic(gpu):
    import torch
    part = CyclicPartition(1, 3, 4000)
    cols = 5
    rng = np.random.default_rng(11)
    size = len(range(1, 4000, 3))
    rows = (rng.integers(0, size, 2500) * 3 + 1).astype(np.int64)  # keys = 1 (mod 3), with repeats
    assert np.unique(rows).size < rows.size
    values = rand_vals(rng, "double", rows.size * cols).reshape(-1, cols)
    ref = O.OracleMatrix(O.part_cyclic(1, 3, 4000), cols, O.CODE["double"])
    d = torch.device("cuda", gpu)
    with PartialMatrix(part, cols, "double", gpu) as sh:
        assert sh.size == size
        for _ in range(2):
            sh.updateRows(torch.from_numpy(rows).to(d), torch.from_numpy(values).to(d), deterministic=True)
            oracle_apply(ref, rows, values, cols)
        np.testing.assert_array_equal(sh.to_numpy(), ref.data)


def _error_input(rng):
    cols = 6
    rows = rng.integers(START, START + SIZE, 100).astype(np.int64)
    rows[7] = START - 1
    rows[60] = START + SIZE
    values = rand_vals(rng, "long", 100 * cols).reshape(100, cols)
    return cols, rows, values


def test_row_push_errors_device(gpu):
    import torch
    cols, rows, values = _error_input(np.random.default_rng(3))
    d = torch.device("cuda", gpu)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["long"])
    keep = np.ones(100, bool)
    keep[[7, 60]] = False
    oracle_apply(ref, rows[keep], values[keep], cols)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.updateRows(torch.from_numpy(rows).to(d), torch.from_numpy(values).to(d))
        assert ei.value.record == 7
        np.testing.assert_array_equal(sh.to_numpy(), ref.data)  # the other 98 rows were applied


def test_row_push_errors_host(gpu):
    cols, rows, values = _error_input(np.random.default_rng(3))
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        ok = np.arange(START, START + 50, dtype=np.int64)
        sh.updateRows(ok, np.full((50, cols), 9, np.int64))
        before = sh.to_numpy().copy()
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.updateRows(rows, values)
        assert ei.value.record == 7
        np.testing.assert_array_equal(sh.to_numpy(), before)  # a rejected message applies nothing


def test_row_push_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    v = np.ones(4, np.float64)
    rd, vd = torch.from_numpy(r).to(d), torch.from_numpy(v).to(d)
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        assert lib.glint_mat_push_rows(vec.handle, r.ctypes.data, v.ctypes.data, 1, 0) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows_dev(vec.handle, rd.data_ptr(), vd.data_ptr(), 1, 0, None) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        h = sh.handle
        assert lib.glint_mat_push_rows(h, r.ctypes.data, v.ctypes.data, 1, N.GLINT_PUSH_VALIDATE) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows_dev(h, rd.data_ptr(), vd.data_ptr(), 1, N.GLINT_PUSH_VALIDATE,
                                           None) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows(h, r.ctypes.data, v.ctypes.data, 1, 8) == N.GLINT_EINVAL  # unknown flag bit
        assert lib.glint_mat_push_rows(h, r.ctypes.data, v.ctypes.data, -1, 0) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows(h, None, v.ctypes.data, 1, 0) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows_dev(h, rd.data_ptr(), None, 1, 0, None) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows(h, r.ctypes.data, v.ctypes.data, (1 << 32) - 2048, 0) == N.GLINT_EINVAL
        assert lib.glint_mat_push_rows(h, None, None, 0, 0) == N.GLINT_OK
        with pytest.raises(ValueError):  # values one element short: no call is made
            sh.updateRows(r, v[:3])
        with pytest.raises(ValueError):
            sh.updateRows(rd, vd[:3])
        assert not sh.to_numpy().any()
        assert sh.updateRows(r, v) and sh.updateRows(rd, vd.view(1, 4))
        np.testing.assert_array_equal(sh.to_numpy()[0], np.full(4, 2.0))


def test_row_push_unaligned_values(gpu):
    """values starting one element into a buffer: 8-B aligned only, the fold takes the scalar slice."""
    import torch
    cols = 128
    rows, values, _, _ = case("double", cols, "duplicates")
    d = torch.device("cuda", gpu)
    n = rows.size
    buf = torch.zeros(n * cols + 3, dtype=torch.float64, device=d)
    v = buf[1:1 + n * cols]
    v.copy_(torch.from_numpy(np.array(values)).to(d).view(-1))
    assert v.data_ptr() % 16 == 8 and v.is_contiguous()
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["double"])
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "double", gpu) as sh:
        for _ in range(2):
            sh.updateRows(torch.from_numpy(np.array(rows)).to(d), v, deterministic=True)
            oracle_apply(ref, rows, values, cols)
        np.testing.assert_array_equal(sh.to_numpy(), ref.data)


@functools.lru_cache(maxsize=None)
def skew_case(dtype):
    """20 000 records over 3 rows plus 500 rows once each, shuffled: runs far past the split length."""
    cols = 64
    rng = np.random.default_rng(77)
    picks = rng.choice(SIZE, 503, replace=False)
    rows = np.concatenate([rng.choice(picks[:3], 20_000), picks[3:]]).astype(np.int64) + START
    rng.shuffle(rows)
    values = rand_vals(rng, dtype, rows.size * cols).reshape(-1, cols)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE[dtype])
    for _ in range(2):
        oracle_apply(ref, rows, values, cols)
    mag = np.zeros((SIZE, cols), np.float64)
    if dtype == "double":
        np.add.at(mag, rows - START, 2.0 * np.abs(values))
    return cols, rows, values, ref.data, mag


@pytest.mark.parametrize("dtype,det", [("long", False), ("double", False), ("double", True)])
def test_row_push_skew(gpu, dtype, det):
    """Long: a lost or doubled chunk of a split run cannot pass. Double default: within 1e-9 of sum |v|
    (the oracle's own sequential sum of ~6 700 terms is within 6 700 x 2^-53 ~ 7e-13 of exact, three
    orders of magnitude inside the bar). Double deterministic: nothing is split, bit-exact."""
    import torch
    cols, rows, values, ref, mag = skew_case(dtype)
    assert rows.size == 20_500
    d = torch.device("cuda", gpu)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        r, v = torch.from_numpy(rows).to(d), torch.from_numpy(values).to(d)
        for _ in range(2):
            sh.updateRows(r, v, deterministic=det)
        check(sh.to_numpy(), ref, mag, dtype, dtype == "long" or det, 0)


def test_row_push_stream_order(gpu):
    """Row pushes, an element push and a row pull on one stream, one sync at the end."""
    import torch
    cols = 9
    rng = np.random.default_rng(21)
    d = torch.device("cuda", gpu)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["long"])
    r1 = rng.integers(START, START + 200, 700).astype(np.int64)
    v1 = rand_vals(rng, "long", 700 * cols).reshape(-1, cols)
    er = rng.integers(START, START + 200, 1000).astype(np.int64)  # the same rows, by element
    ec = rng.integers(0, cols, 1000).astype(np.int32)
    ev = rand_vals(rng, "long", 1000)
    r2 = rng.integers(START + 100, START + 300, 900).astype(np.int64)
    v2 = rand_vals(rng, "long", 900 * cols).reshape(-1, cols)
    q = np.arange(START, START + 300, dtype=np.int64)
    t = lambda a: torch.from_numpy(a).to(d)  # noqa: E731
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        tr1, tv1, ter, tec, tev, tr2, tv2, tq = t(r1), t(v1), t(er), t(ec), t(ev), t(r2), t(v2), t(q)
        sh.updateRows(tr1, tv1, sync=False)
        sh.update(ter, tec, tev, sync=False)
        sh.updateRows(tr2, tv2, sync=False)
        out = sh.getRows(tq, sync=False)
        sh.sync(sh._stream_of(tq))
        oracle_apply(ref, r1, v1, cols)
        assert ref.update(er, ec, ev) == -1
        oracle_apply(ref, r2, v2, cols)
        np.testing.assert_array_equal(out.cpu().numpy(), ref.data[:300])


def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_row_push_profiling_id(gpu):
    rows = np.arange(START, START + 100, dtype=np.int64)
    with PartialMatrix(RangePartition(2, START, START + SIZE), 4, "double", gpu) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        sh.update(rows, np.zeros(100, np.int32), np.ones(100))
        assert _launches(sh, N.GLINT_K_PUSH_ROWS) == 0  # an element push is not a row push
        sh.updateRows(rows, np.ones((100, 4)))
        assert _launches(sh, N.GLINT_K_PUSH_ROWS) > 0


def test_row_push_past_4gib(gpu):
    """n x cols x 4 B just over 2^32: every offset into the values is 64-bit. Sums of small integers
    are exact in any order, so the default mode (these runs of 257 are split) must match exactly."""
    import torch
    d = torch.device("cuda", gpu)
    R, cols = 4096, 1024
    n = (1 << 20) + 4096
    assert n * cols * 4 > 1 << 32 and n == 257 * R
    rows = torch.arange(n, dtype=torch.int64, device=d) % R
    values = (torch.arange(n * cols, dtype=torch.int32, device=d) % 7 - 3).to(torch.float32)
    want = values.view(257, R, cols).sum(0)
    with PartialMatrix(RangePartition(0, 0, R), cols, "float", gpu) as sh:
        sh.updateRows(rows, values.view(n, cols))
        got = sh.getRows(torch.arange(R, dtype=torch.int64, device=d))
        assert torch.equal(got, want)


@pytest.mark.parametrize("path", PATHS)
@pytest.mark.parametrize("size", SORT_SIZES)
def test_row_push_sort_passes(gpu, size, path):
    """One to four passes of the sort, either buffer pair, 2^k-row shards whose sentinel alone has the top
    bit; runs of RUNS with the first and the last row among their owners; three pushes of 2047, 2048 and
    2049 records onto one shard. Long everywhere; Double, bit for bit, on the two paths that keep the
    order. On the device paths two records lie outside (START - 1 and START + size): skipped, the lower
    index reported."""
    import torch
    d = torch.device("cuda", gpu)
    assert sort_passes(size) == SORT_PASSES[size]
    for dtype in ("long",) + (("double",) if path != "dev" else ()):
        pushes, want = sort_case(size, dtype, path != "host")
        with PartialMatrix(RangePartition(2, START, START + size), sort_cols(size), dtype, gpu) as sh:
            for rows, values, low, _ in pushes:
                if path == "host":
                    assert sh.updateRows(rows, values)
                    continue
                with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                    sh.updateRows(torch.from_numpy(rows).to(d), torch.from_numpy(values).to(d),
                                  deterministic=(path == "dev_det"))
                assert ei.value.record == low
            same_bits(sh.to_numpy(), want)


@pytest.mark.parametrize("n", [1024 * 2048 + 1, 4096 * 2048 + 1])
def test_row_push_many_tiles(gpu, n):
    """1025 tiles: the second trip of the digit totals' loop; 4097 tiles: the second trip of the offsets'
    scan, with its carry. Long, one column, 65 537 rows (three passes), one push per mode."""
    import torch
    d = torch.device("cuda", gpu)
    size = 65_537
    rng = np.random.default_rng(n)
    local = rng.integers(0, size, n)
    values = rng.integers(-2**63, 2**63 - 1, n, dtype=np.int64, endpoint=True)
    want = np.zeros(size, np.int64)
    np.add.at(want, local, values)
    rows, vals = torch.from_numpy(local + START).to(d), torch.from_numpy(values).to(d)
    for det in (False, True):
        with PartialMatrix(RangePartition(2, START, START + size), 1, "long", gpu) as sh:
            assert sh.updateRows(rows, vals, deterministic=det)
            np.testing.assert_array_equal(sh.to_numpy()[:, 0], want)


def test_row_push_client(gpu):
    rng = np.random.default_rng(8)
    rows = rng.integers(0, 1000, 5000).astype(np.int64)
    values = rng.integers(-10**12, 10**12, (5000, 7)).astype(np.int64)
    m = Client([gpu] * 3).matrix(1000, 7, "long", modelsPerServer=2)
    assert m.nrOfPartitions == 6
    m.pushRows(rows, values)
    want = np.zeros((1000, 7), np.int64)
    np.add.at(want, rows, values)
    np.testing.assert_array_equal(m.pull(np.arange(1000)), want)
    m.destroy()
