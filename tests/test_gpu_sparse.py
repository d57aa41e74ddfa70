"""Sparse row pull (PartialMatrix.getRowsSparse, glint_mat_pull_rows_sparse*) against the oracle.

The expected answer is always OracleMatrix.get_rows(rows) turned into CSR with numpy: the `!= 0` mask
(-0.0 dropped, NaN kept), row-major. Everything is compared bit for bit, values through an integer
view so that NaN compares. The three paths -- host arrays, device tensors sized by a count
(cap=None), device tensors with a given cap -- must all give that answer.
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
from glint_amd.shard import check as check_rc
from ieee_cases import write_image
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
START, SIZE = 1_000_003, 1500
COLS = [1, 3, 64, 65, 130, 512]
# pushed with update(), so the oracle holds the same data; "raw" is written into the shard's memory
# as an image instead (update cannot produce -0.0 from a zeroed shard: +0.0 + -0.0 = +0.0)
FILLS = ["zero", "full", "random5", "col0", "last_col", "one_row", "raw"]
REQUESTS = ["all", "permutation", "draws", "one", "empty"]
SENTINEL = 0x5A


def np_dtype(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def nonzero_vals(rng, dtype, n):
    npd = np_dtype(dtype)
    if np.issubdtype(npd, np.floating):
        v = rng.uniform(-1, 1, n).astype(npd)
    else:
        info = np.iinfo(npd)
        v = rng.integers(info.min, info.max, n, dtype=npd, endpoint=True)
    v[v == 0] = 1
    return v


def fill_mask(rng, fill, cols):
    m = np.zeros((SIZE, cols), bool)
    if fill == "full":
        m[:] = True
    elif fill in ("random5", "raw"):
        m = rng.random((SIZE, cols)) < 0.05
    elif fill == "col0":
        m[:, 0] = True
    elif fill == "last_col":
        m[:, cols - 1] = True
    elif fill == "one_row":
        m[777] = True
    return m


@functools.lru_cache(maxsize=None)
def image(dtype, cols, fill):
    """The shard's (SIZE, cols) content for a fill; read-only, shared by every test that uses it."""
    rng = np.random.default_rng(zlib.crc32(f"sparse/{dtype}/{cols}/{fill}".encode()))
    npd = np_dtype(dtype)
    m = fill_mask(rng, fill, cols)
    img = np.zeros((SIZE, cols), npd)
    img[m] = nonzero_vals(rng, dtype, int(m.sum()))
    if fill == "raw" and np.issubdtype(npd, np.floating):
        # -0.0 (dropped), NaNs with different payloads and signs (kept, bits unchanged), a subnormal (kept)
        if npd == np.float32:
            special = np.array([0x80000000, 0x7FC00001, 0xFFC00001, 0x7FC00000, 0x00000001, 0x80000000],
                               np.uint32).view(np.float32)
        else:
            special = np.array([0x8000000000000000, 0x7FF8000000000123, 0xFFF8000000000123, 0x7FF8000000000000,
                                0x0000000000000001, 0x8000000000000000], np.uint64).view(np.float64)
        pick = rng.random((SIZE, cols)) < 0.05
        img[pick] = special[rng.integers(0, special.size, int(pick.sum()))]
        img[5, 0], img[6, cols - 1] = special[0], special[1]
    img.setflags(write=False)
    return img


def load_shard(sh, ref, gpu, img, fill):
    """Shard and oracle to the image: by update() of its non-zero elements, or ("raw") as memory."""
    if fill == "raw":
        write_image(sh, gpu, img, 1)
        ref.data[...] = img
        return
    r, c = np.nonzero(img)
    if r.size:
        rows, cols, vals = (r + START).astype(np.int64), c.astype(np.int32), img[r, c]
        assert sh.update(rows, cols, vals)
        assert ref.update(rows, cols, vals) == -1


def make_rows(rng, request, size=SIZE, start=START):
    if request == "all":
        return np.arange(start, start + size, dtype=np.int64)
    if request == "permutation":
        return rng.permutation(size).astype(np.int64) + start
    if request == "draws":
        return rng.choice(rng.choice(size, 40, replace=False), 3000).astype(np.int64) + start
    if request == "one":
        return np.array([start + min(777, size - 1)], np.int64)
    return np.zeros(0, np.int64)


def to_csr(dense):
    mask = dense != 0
    indptr = np.zeros(dense.shape[0] + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(mask)[1].astype(np.int32), dense[mask]


def expected(ref, rows):
    dense, bad = ref.get_rows(rows)
    assert bad == -1
    return to_csr(dense)


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)


def host_triple(t):
    return tuple(x.cpu().numpy() if hasattr(x, "cpu") else x for x in t)


def assert_same(got, exp, what=""):
    gp, gc, gv = host_triple(got)
    ep, ec, ev = exp
    assert gp.dtype == np.int64 and gc.dtype == np.int32 and gv.dtype == ev.dtype, what
    np.testing.assert_array_equal(gp, ep, err_msg=what)
    np.testing.assert_array_equal(gc, ec, err_msg=what)
    np.testing.assert_array_equal(bits(gv), bits(ev), err_msg=what)


def pull_paths(sh, gpu, rows, exp):
    """host, device exact, device with a cap (a little more than needed): all the expected triple."""
    import torch
    nnz = int(exp[0][-1])
    assert_same(sh.getRowsSparse(rows), exp, "host")
    t = torch.from_numpy(np.array(rows)).to(torch.device("cuda", gpu))
    got = sh.getRowsSparse(t)
    assert got[1].numel() == nnz and got[2].numel() == nnz
    assert_same(got, exp, "device exact")
    ip, c, v = sh.getRowsSparse(t, cap=nnz + 7)
    assert c.numel() == nnz + 7 and int(ip[-1]) == nnz
    assert_same((ip, c[:nnz], v[:nnz]), exp, "device cap")


@pytest.mark.parametrize("fill", FILLS)
@pytest.mark.parametrize("cols", COLS)
@pytest.mark.parametrize("dtype", DT)
def test_sparse_pull_parity(gpu, dtype, cols, fill):
    img = image(dtype, cols, fill)
    rng = np.random.default_rng(zlib.crc32(f"req/{dtype}/{cols}/{fill}".encode()))
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE[dtype])
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        load_shard(sh, ref, gpu, img, fill)
        for request in REQUESTS:
            rows = make_rows(rng, request)
            exp = expected(ref, rows)
            pull_paths(sh, gpu, rows, exp)
            if request == "all":  # the triple scattered into zeros is getRows (a dropped -0.0 comes back +0.0)
                ip, c, v = sh.getRowsSparse(rows)
                dense = np.zeros((rows.size, cols), img.dtype)
                dense[np.repeat(np.arange(rows.size), np.diff(ip)), c] = v
                full = sh.getRows(rows)
                np.testing.assert_array_equal(bits(dense), bits(np.where(full == 0, np.zeros_like(full), full)))


def test_sparse_pull_keeps_bits_and_drops_negative_zero(gpu):
    """What the raw fill is for, stated directly: no -0.0 among the values, every NaN of the requested
    rows among them with its payload and sign."""
    img = image("float", 65, "raw")
    with PartialMatrix(RangePartition(2, START, START + SIZE), 65, "float", gpu) as sh:
        write_image(sh, gpu, img, 1)
        ip, c, v = sh.getRowsSparse(np.arange(START, START + SIZE, dtype=np.int64))
    assert (bits(img) == 0x80000000).sum() > 100 and not (bits(v) == 0x80000000).any()
    nan_bits = np.sort(bits(img)[np.isnan(img)])
    assert nan_bits.size > 100 and np.unique(nan_bits).size >= 3
    np.testing.assert_array_equal(np.sort(bits(v)[np.isnan(v)]), nan_bits)
    assert ip[-1] == (img != 0).sum()


def _raw_call(sh, gpu, rows, cap, size, path, null_outputs=False):
    """One C ABI call with sentinel-filled outputs of `size` entries; returns (rc, row_ptr, cols, vals, nnz)."""
    lib = N.load()
    n = rows.size
    if path == "host":
        rp = np.full(n + 1, -1, np.int64)
        oc = np.full(size, -1, np.int32)
        ov = np.zeros(size, sh.np_dtype)
        ov.view(np.uint8)[:] = SENTINEL
        nnz = C.c_int64(-1)
        rc = lib.glint_mat_pull_rows_sparse(sh.handle, rows.ctypes.data, n, rp.ctypes.data,
                                            None if null_outputs else oc.ctypes.data,
                                            None if null_outputs else ov.ctypes.data, cap, C.byref(nnz))
        return rc, rp, oc, ov, nnz.value
    import torch
    d = torch.device("cuda", gpu)
    t = torch.from_numpy(np.array(rows)).to(d)
    rp = torch.full((n + 1,), -1, dtype=torch.int64, device=d)
    oc = torch.full((size,), -1, dtype=torch.int32, device=d)
    ov = torch.full((size * np.dtype(sh.np_dtype).itemsize,), SENTINEL, dtype=torch.uint8, device=d)
    st = torch.cuda.current_stream(d).cuda_stream
    rc = lib.glint_mat_pull_rows_sparse_dev(sh.handle, t.data_ptr(), n, rp.data_ptr(),
                                            None if null_outputs else oc.data_ptr(),
                                            None if null_outputs else ov.data_ptr(), cap, st)
    torch.cuda.synchronize(d)
    rp = rp.cpu().numpy()
    return rc, rp, oc.cpu().numpy(), ov.cpu().numpy().view(sh.np_dtype), int(rp[-1])


def _sentinel_vals(npd, k):
    v = np.zeros(k, npd)
    v.view(np.uint8)[:] = SENTINEL
    return v


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("dtype,cols", [("double", 130), ("int", 65), ("float", 512), ("long", 3)])
def test_sparse_pull_capacity(gpu, dtype, cols, path):
    """As snprintf: row_ptr complete whatever the capacity, entries stored only below cap, nothing
    touched from cap on."""
    fill = "full" if cols == 3 else "random5"
    img = image(dtype, cols, fill)
    rng = np.random.default_rng(9)
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE[dtype])
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, dtype, gpu) as sh:
        load_shard(sh, ref, gpu, img, fill)
        rows = make_rows(rng, "draws")
        e_ptr, e_cols, e_vals = expected(ref, rows)
        nnz = int(e_ptr[-1])
        counts = np.diff(e_ptr)
        i = int(np.argmax(counts >= 2))  # a request with at least two entries: cap falls between them
        assert counts[i] >= 2 and nnz > 16
        mid_row = int(e_ptr[i]) + 1
        size = nnz + 16
        for cap, null_outputs in [(0, True), (0, False), (1, False), (mid_row, False), (nnz - 1, False),
                                  (nnz, False), (nnz + 9, False)]:
            rc, rp, oc, ov, total = _raw_call(sh, gpu, rows, cap, size, path, null_outputs)
            assert rc == N.GLINT_OK and total == nnz, (cap, rc, total)
            np.testing.assert_array_equal(rp, e_ptr)
            k = min(cap, nnz)
            np.testing.assert_array_equal(oc[:k], e_cols[:k])
            np.testing.assert_array_equal(bits(ov[:k]), bits(e_vals[:k]))
            assert (oc[k:] == -1).all(), cap
            np.testing.assert_array_equal(bits(ov[k:]), bits(_sentinel_vals(sh.np_dtype, size - k)))
        if path == "host":  # the Python wrapper with a cap: exact-size arrays, or cut at cap
            ip, c, v = sh.getRowsSparse(rows, cap=nnz + 9)
            assert_same((ip, c, v), (e_ptr, e_cols, e_vals))
            ip, c, v = sh.getRowsSparse(rows, cap=mid_row)
            assert_same((ip, c, v), (e_ptr, e_cols[:mid_row], e_vals[:mid_row]))


def test_sparse_pull_errors_host(gpu):
    cols = 6
    img = image("long", cols, "full")
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["long"])
    rows = np.random.default_rng(3).integers(START, START + SIZE, 100).astype(np.int64)
    rows[7], rows[60] = START - 1, START + SIZE
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        load_shard(sh, ref, gpu, img, "full")
        rc, rp, oc, ov, total = _raw_call(sh, gpu, rows, 1000, 1000, "host")
        assert rc == N.GLINT_EOUTOFRANGE
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            check_rc(rc, sh.handle)
        assert ei.value.record == 7
        assert (rp == -1).all() and (oc == -1).all() and total == -1  # nothing written
        np.testing.assert_array_equal(bits(ov), bits(_sentinel_vals(np.int64, 1000)))
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            sh.getRowsSparse(rows)
        assert ei.value.record == 7
        good = rows[:7]
        assert_same(sh.getRowsSparse(good), expected(ref, good))  # the shard answers the next pull


def test_sparse_pull_errors_device(gpu):
    import torch
    cols = 6
    img = image("long", cols, "full")
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), cols, O.CODE["long"])
    rows = np.random.default_rng(3).integers(START, START + SIZE, 100).astype(np.int64)
    rows[7], rows[60] = START - 1, START + SIZE
    stand_in = rows.copy()
    stand_in[[7, 60]] = START
    d = torch.device("cuda", gpu)
    with PartialMatrix(RangePartition(2, START, START + SIZE), cols, "long", gpu) as sh:
        load_shard(sh, ref, gpu, img, "full")
        dense, bad = ref.get_rows(stand_in)
        assert bad == -1
        dense[[7, 60]] = 0  # a row outside the partition has no entries; the others are answered
        exp = to_csr(dense)
        t = torch.from_numpy(rows).to(d)
        for cap in (None, int(exp[0][-1])):
            got = sh.getRowsSparse(t, cap=cap, sync=False)
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                sh.sync(sh._stream_of(t))
            assert ei.value.record == 7
            assert_same(got, exp)
        sh.sync(sh._stream_of(t))  # the error state was cleared


def test_sparse_pull_argument_errors(gpu):
    import torch
    lib = N.load()
    d = torch.device("cuda", gpu)
    r = np.array([START], np.int64)
    rp = np.zeros(2, np.int64)
    oc = np.zeros(4, np.int32)
    ov = np.zeros(4, np.float64)
    rd, rpd, ocd, ovd = (torch.from_numpy(a).to(d) for a in (r, rp, oc, ov))
    host = lambda h, rows, n, p, c, v, cap: lib.glint_mat_pull_rows_sparse(h, rows, n, p, c, v, cap, None)  # noqa: E731
    dev = lambda h, rows, n, p, c, v, cap: lib.glint_mat_pull_rows_sparse_dev(h, rows, n, p, c, v, cap, None)  # noqa: E731
    with PartialVector(RangePartition(0, START, START + 10), "double", gpu) as vec:
        assert host(vec.handle, r.ctypes.data, 1, rp.ctypes.data, oc.ctypes.data, ov.ctypes.data, 4) == N.GLINT_EINVAL
        assert dev(vec.handle, rd.data_ptr(), 1, rpd.data_ptr(), ocd.data_ptr(), ovd.data_ptr(), 4) == N.GLINT_EINVAL
    with PartialMatrix(RangePartition(0, START, START + 10), 4, "double", gpu) as sh:
        h = sh.handle
        sh.update(r, np.array([2], np.int32), np.array([3.5]))
        for call, a in ((host, (r.ctypes.data, rp.ctypes.data, oc.ctypes.data, ov.ctypes.data)),
                        (dev, (rd.data_ptr(), rpd.data_ptr(), ocd.data_ptr(), ovd.data_ptr()))):
            rows_p, ptr_p, cols_p, vals_p = a
            assert call(h, rows_p, -1, ptr_p, cols_p, vals_p, 4) == N.GLINT_EINVAL
            assert call(h, rows_p, 1 << 31, ptr_p, cols_p, vals_p, 4) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, ptr_p, cols_p, vals_p, -1) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, None, cols_p, vals_p, 4) == N.GLINT_EINVAL
            assert call(h, None, 1, ptr_p, cols_p, vals_p, 4) == N.GLINT_EINVAL
            assert call(h, rows_p, 1, ptr_p, None, vals_p, 4) == N.GLINT_EINVAL  # NULL outputs only with cap == 0
            assert call(h, rows_p, 1, ptr_p, cols_p, None, 4) == N.GLINT_EINVAL
        # n == 0 still writes row_ptr[0] = 0 (rows may be NULL)
        p0 = np.full(1, -1, np.int64)
        nnz = C.c_int64(-1)
        assert lib.glint_mat_pull_rows_sparse(h, None, 0, p0.ctypes.data, None, None, 0, C.byref(nnz)) == N.GLINT_OK
        assert p0[0] == 0 and nnz.value == 0
        p0d = torch.full((1,), -1, dtype=torch.int64, device=d)
        assert dev(h, None, 0, p0d.data_ptr(), None, None, 0) == N.GLINT_OK
        torch.cuda.synchronize(d)
        assert int(p0d[0]) == 0
        with pytest.raises(TypeError):  # rows of the wrong dtype: no call is made
            sh.getRowsSparse(rd.to(torch.int32))
        ip, c, v = sh.getRowsSparse(r)
        assert ip.tolist() == [0, 1] and c.tolist() == [2] and v.tolist() == [3.5]


def test_sparse_pull_cyclic(gpu):
    part = CyclicPartition(1, 3, 4000)
    cols = 65
    size = len(range(1, 4000, 3))
    rng = np.random.default_rng(11)
    ref = O.OracleMatrix(O.part_cyclic(1, 3, 4000), cols, O.CODE["long"])
    n = 6000
    ur = (rng.integers(0, size, n) * 3 + 1).astype(np.int64)
    uc = rng.integers(0, cols, n).astype(np.int32)
    uv = nonzero_vals(rng, "long", n)
    with PartialMatrix(part, cols, "long", gpu) as sh:
        assert sh.size == size
        assert sh.update(ur, uc, uv) and ref.update(ur, uc, uv) == -1
        rows = (rng.integers(0, size, 2500) * 3 + 1).astype(np.int64)  # keys = 1 (mod 3), with repeats
        pull_paths(sh, gpu, rows, expected(ref, rows))


def test_sparse_pull_slab_view(gpu):
    """A view inside a slab: its rows start 32 rows into the slab's allocation (66-element pitch:
    views start every 16 rows); the slab's other rows are non-zero and must not show up."""
    import torch
    cols, vrows = 65, 48
    rng = np.random.default_rng(12)
    d = torch.device("cuda", gpu)
    slab = PartialMatrix(RangePartition(0, 0, 96), cols, "long", gpu)
    sr = torch.arange(96, dtype=torch.int64, device=d).repeat_interleave(cols)
    sc = torch.arange(cols, dtype=torch.int32, device=d).repeat(96)
    slab.update(sr, sc, torch.full((96 * cols,), 9, dtype=torch.int64, device=d))  # every slab element 9
    view = PartialMatrix.view(slab, RangePartition(1, START, START + vrows), 32)
    try:
        ref = O.OracleMatrix(O.part_range(START, START + vrows), cols, O.CODE["long"])
        ref.data[...] = 9
        n = 1500
        ur = rng.integers(START, START + vrows, n).astype(np.int64)
        uc = rng.integers(0, cols, n).astype(np.int32)
        uv = np.where(rng.random(n) < 0.5, -9, nonzero_vals(rng, "long", n)).astype(np.int64)  # -9: back to zero
        assert view.update(ur, uc, uv) and ref.update(ur, uc, uv) == -1
        assert (ref.data == 0).sum() > 100
        for request in ("all", "draws"):
            rows = make_rows(rng, request, vrows, START) if request == "all" else \
                rng.integers(START, START + vrows, 700).astype(np.int64)
            pull_paths(view, gpu, rows, expected(ref, rows))
    finally:
        view.destroy()
        slab.destroy()


SCAN_TILE = N.GLINT_SPARSE_SCAN_TILE  # counts one scan workgroup covers (include/glint_gpu.h)


@pytest.mark.parametrize("n", [SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 5, SCAN_TILE * SCAN_TILE - 1,
                               SCAN_TILE * SCAN_TILE + 3])
def test_sparse_pull_multi_level_scan(gpu, n):
    """The prefix runs over n + 1 counts: one workgroup up to SCAN_TILE of them, two levels up to
    SCAN_TILE^2, three beyond (the second level then exceeds one workgroup too)."""
    import torch
    img = image("int", 1, "random5")
    dense_img = np.where(np.arange(SIZE)[:, None] % 3 == 0, img, 1).astype(np.int32)  # ~2/3 non-zero
    ref = O.OracleMatrix(O.part_range(START, START + SIZE), 1, O.CODE["int"])
    rng = np.random.default_rng(n)
    rows = rng.integers(START, START + SIZE, n).astype(np.int64)
    with PartialMatrix(RangePartition(2, START, START + SIZE), 1, "int", gpu) as sh:
        load_shard(sh, ref, gpu, dense_img, "update")
        exp = expected(ref, rows)
        assert 0 < exp[0][-1] < n
        assert_same(sh.getRowsSparse(torch.from_numpy(rows).to(torch.device("cuda", gpu))), exp, "device")
        assert_same(sh.getRowsSparse(rows), exp, "host")


def test_sparse_pull_past_2_31(gpu):
    """4 rows x 2^20 columns, every element non-zero, 2049 requests: row_ptr[i] = i * 2^20 exactly, so
    row_ptr[n] > 2^31 -- positions are 64-bit. cap = 1000: the first 1000 entries, nothing more."""
    import torch
    R, cols, n, cap = 4, 1 << 20, 2049, 1000
    d = torch.device("cuda", gpu)
    ref = O.OracleMatrix(O.part_range(0, R), cols, O.CODE["int"])
    ur = np.repeat(np.arange(R, dtype=np.int64), cols)
    uc = np.tile(np.arange(cols, dtype=np.int32), R)
    uv = (np.arange(R * cols, dtype=np.int64) % 1000 + 1).astype(np.int32)
    assert ref.update(ur, uc, uv) == -1
    rows = (np.arange(n, dtype=np.int64) * 3 + 2) % R
    first, bad = ref.get_rows(rows[:1])
    assert bad == -1 and (first != 0).all()
    with PartialMatrix(RangePartition(0, 0, R), cols, "int", gpu) as sh:
        assert sh.update(torch.from_numpy(ur).to(d), torch.from_numpy(uc).to(d), torch.from_numpy(uv).to(d))
        ip, c, v = sh.getRowsSparse(torch.from_numpy(rows).to(d), cap=cap)
        np.testing.assert_array_equal(ip.cpu().numpy(), np.arange(n + 1, dtype=np.int64) << 20)
        assert int(ip[-1]) > 1 << 31
        np.testing.assert_array_equal(c.cpu().numpy(), np.arange(cap, dtype=np.int32))
        np.testing.assert_array_equal(v.cpu().numpy(), first[0, :cap])


def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def test_sparse_pull_profiling_id(gpu):
    rows = np.arange(START, START + 100, dtype=np.int64)
    with PartialMatrix(RangePartition(2, START, START + SIZE), 4, "double", gpu) as sh:
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        sh.update(rows, np.zeros(100, np.int32), np.ones(100))
        sh.getRows(rows)
        assert _launches(sh, N.GLINT_K_PULL_ROWS_SPARSE) == 0  # a dense row pull is not a sparse one
        ip, c, v = sh.getRowsSparse(rows)
        assert ip[-1] == 100 and _launches(sh, N.GLINT_K_PULL_ROWS_SPARSE) >= 1


def test_sparse_pull_client(gpu):
    rng = np.random.default_rng(8)
    table = rng.integers(-10**12, 10**12, (1000, 7)).astype(np.int64) * (rng.random((1000, 7)) < 0.3)
    m = Client([gpu] * 3).matrix(1000, 7, "long", modelsPerServer=2)
    assert m.nrOfPartitions == 6
    m.pushRows(np.arange(1000, dtype=np.int64), table)
    rows = rng.integers(0, 1000, 5000).astype(np.int64)
    got = m.pullSparse(rows)
    assert_same(got, to_csr(m.pull(rows)))
    assert_same(got, to_csr(table[rows]))
    m.destroy()
