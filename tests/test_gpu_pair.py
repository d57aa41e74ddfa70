"""Row-pair dot pull and row-pair axpy push (PartialMatrix.getPairsDot / updatePairsAxpy,
glint_mat_pull_pairs_dot*, glint_mat_push_pairs_axpy*) on the GPU.

Pair dot: bit for bit against pair_cases.replay_pair_dot, the row dot pull's replay with the second shard's
stored row as the vector. Pair axpy: against updateRows of the replayed contributions on a twin shard --
bit for bit for host arrays and deterministic device pushes and for Int/Long on every path; the device
default and `unordered` within test_gpu_axpy.check's bar (Double 1e-9 of the element's sum of magnitudes,
Float the format's own bound for that many terms). Every shard image is written with a non-zero pitch
padding, so a kernel that read the padding would count it."""
import contextlib
import ctypes as C
import functools
import zlib

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import (ArrayIndexOutOfBoundsException, Client, CyclicPartition, PartialMatrix, PartialVector,
                       RangePartition, RangePartitioner)
from axpy_cases import assert_bits, nofma_element
from dot_cases import NOFMA_PLACES, assert_dot_bits, nofma_case
from ieee_cases import GRIDS, special, write_image
from pair_cases import bits, pair_coef, pair_contrib, pair_values, replay_pair_axpy, replay_pair_dot
from test_gpu_axpy import check, read_image

pytestmark = pytest.mark.gpu
DT = ["double", "float", "long", "int"]
SA, NA = 1_000_003, 300        # a: a range shard with a non-zero start
SB, NB = 77_000, 211           # b: another start and size
CYC = (1, 3, 700)              # b cyclic: index, parts, keys -> 233 rows
PAD = 777
WIDTHS = [1, 6, 67, 128, 130, 515]
PARTS = ["range", "cyclic", "same", "views"]
AXPY_PARTS = ["range", "cyclic", "both_cyclic", "views_apart"]
AXPY_PATHS = ["host", "host_unordered", "dev", "dev_det", "dev_unordered"]


def npd_of(dtype):
    return glint_amd.shard.resolve_dtype(dtype)[1]


def keys_of(part, local):
    local = np.asarray(local, np.int64)
    if isinstance(part, RangePartition):
        return local + part.start
    return local * part.numberOfPartitions + part.index


def dev_t(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", gpu))


@contextlib.contextmanager
def two_shards(gpu, dtype, cols, parts, what="t"):
    """(a, A, b, B): two shards and their images, written as they lie with the pitch padding set to PAD.
    `same`: b is a. `views` / `views_apart`: both are views of one 512-row slab, rows [0, 300) and
    [128, 339) / [320, 512)."""
    name = np.dtype(npd_of(dtype)).name
    made = []
    try:
        if parts in ("views", "views_apart"):
            off_b, nb = (128, NB) if parts == "views" else (320, 192)
            slab = PartialMatrix(RangePartition(0, 0, 512), cols, dtype, gpu)
            made.append(slab)
            S = pair_values(name, 512, cols, what + "/slab")
            write_image(slab, gpu, S, PAD)
            a = PartialMatrix.view(slab, RangePartition(0, SA, SA + NA), 0)
            made.insert(0, a)
            b = PartialMatrix.view(slab, RangePartition(1, SB, SB + nb), off_b)
            made.insert(0, b)
            yield a, S[:NA], b, S[off_b:off_b + nb]
            return
        pa = CyclicPartition(2, 5, 1498) if parts == "both_cyclic" else RangePartition(2, SA, SA + NA)
        a = PartialMatrix(pa, cols, dtype, gpu)
        made.append(a)
        A = pair_values(name, a.size, cols, what + "/a")
        write_image(a, gpu, A, PAD)
        if parts == "same":
            yield a, A, a, A
            return
        pb = CyclicPartition(*CYC) if parts in ("cyclic", "both_cyclic") else RangePartition(1, SB, SB + NB)
        b = PartialMatrix(pb, cols, dtype, gpu)
        made.append(b)
        B = pair_values(name, b.size, cols, what + "/b")
        write_image(b, gpu, B, PAD)
        yield a, A, b, B
    finally:
        for sh in made:  # views before their slab
            sh.destroy()


@functools.lru_cache(maxsize=None)
def pair_rows(na, nb, n, seed):
    """Local rows of n pairs: every row of a at least once when n allows, rows of b with repeats and in
    random order; read-only, shared."""
    rng = np.random.default_rng(zlib.crc32(f"pairs/{na}/{nb}/{n}/{seed}".encode()))
    la = np.concatenate([rng.permutation(na)[:min(na, n // 2)], rng.integers(0, na, n - min(na, n // 2))])
    lb = rng.choice(rng.choice(nb, max(1, nb // 2), replace=False), n)
    for x in (la, lb):
        x.setflags(write=False)
    return la, lb


def pairs_dot(a, b, ra, rb, path, gpu, out=None):
    if path == "host":
        return a.getPairsDot(b, ra, rb, out=out)
    return a.getPairsDot(b, dev_t(gpu, ra), dev_t(gpu, rb), out=out).cpu().numpy()


# ---- pair dot: bit for bit against the replay -----------------------------------------------------------
# a single column, less than a strip, the scalar path, exactly one 16-B strip, one strip plus a part, past
# eight strips on the scalar path (515) and on the 16-B path (Double 1154, Float 2308). The kernel keeps
# eight strips of each row in flight, not more.
DOT_GRID = sorted({(dt, c, "range") for dt in DT for c in WIDTHS} | {("double", 1154, "range"), ("float", 2308, "range")}
                  | {(dt, c, p) for dt in ("double", "int") for c in (67, 128) for p in PARTS})


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("dtype,cols,parts", DOT_GRID)
def test_pair_dot_parity(gpu, dtype, cols, parts, path):
    with two_shards(gpu, dtype, cols, parts) as (a, A, b, B):
        la, lb = pair_rows(A.shape[0], B.shape[0], 500, "dot")
        got = pairs_dot(a, b, keys_of(a.partition, la), keys_of(b.partition, lb), path, gpu)
        assert_dot_bits(got, replay_pair_dot(A[la], B[lb]), f"{dtype}/{cols}/{parts}/{path}")


# ---- pair dot: identities ----------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("float", 128), ("long", 130)])
def test_pair_dot_equals_the_row_dot_pull_of_the_stored_row(gpu, dtype, cols):
    with two_shards(gpu, dtype, cols, "cyclic") as (a, A, b, B):
        la, lb = pair_rows(A.shape[0], B.shape[0], 50, "identity")
        ra, rb = keys_of(a.partition, la), keys_of(b.partition, lb)
        got = a.getPairsDot(b, ra, rb)
        for i in range(50):
            x = b.getRows(rb[i:i + 1])[0]
            assert bits(a.getRowsDot(ra[i:i + 1], x=x))[0] == bits(got)[i], i


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("float", 2308)])
def test_pair_dot_commutes(gpu, dtype, cols, path):
    """(a, b, ra, rb) against (b, a, rb, ra): IEEE multiplication commutes, the order of the sum is the
    same. The data holds no NaN."""
    with two_shards(gpu, dtype, cols, "range") as (a, A, b, B):
        la, lb = pair_rows(A.shape[0], B.shape[0], 300, "commute")
        ra, rb = keys_of(a.partition, la), keys_of(b.partition, lb)
        one, two = pairs_dot(a, b, ra, rb, path, gpu), pairs_dot(b, a, rb, ra, path, gpu)
        assert not np.isnan(one).any()
        np.testing.assert_array_equal(bits(one), bits(two))


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("dtype,cols", [("double", 130), ("float", 128), ("int", 67)])
def test_pair_dot_of_a_shard_with_itself(gpu, dtype, cols, path):
    with two_shards(gpu, dtype, cols, "same") as (a, A, b, _):
        assert b is a
        ra = keys_of(a.partition, pair_rows(NA, NA, 200, "self")[0])
        got = pairs_dot(a, a, ra, ra, path, gpu)
        np.testing.assert_array_equal(bits(got), bits(a.getRowsDot(ra)))  # x=None: the self-dot


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("dtype,cols,c0,c1", [(dt, *place) for dt, npd in (("double", np.float64), ("float", np.float32))
                                              for place in NOFMA_PLACES[npd]])
def test_pair_dot_is_unfused(gpu, dtype, cols, c0, c1, path):
    """dot_cases.nofma_case with its vector stored as b's row: -b * 1 + a * a is exactly 0 with rounded
    products; a fused product would leave 2^-54 / 2^-24. On the 16-B and on the scalar strip path."""
    npd = npd_of(dtype)
    row, x, fused = nofma_case(npd, cols, c0, c1)
    with PartialMatrix(RangePartition(0, SA, SA + 8), cols, dtype, gpu) as a, \
            PartialMatrix(RangePartition(0, SB, SB + 8), cols, dtype, gpu) as b:
        A, B = np.zeros((8, cols), npd), np.zeros((8, cols), npd)
        A[3], B[6] = row, x
        write_image(a, gpu, A, PAD)
        write_image(b, gpu, B, PAD)
        got = pairs_dot(a, b, np.array([SA + 3]), np.array([SB + 6]), path, gpu)
        assert bits(got)[0] == 0, f"{got[0]!r}: a fused product would leave {fused!r}"


# ---- pair dot: errors ---------------------------------------------------------------------------------------
def test_pair_dot_errors_host(gpu):
    with two_shards(gpu, "double", 6, "range") as (a, A, b, B):
        la, lb = pair_rows(NA, NB, 100, "err")
        ra, rb = np.array(keys_of(a.partition, la)), np.array(keys_of(b.partition, lb))
        ra[40], rb[17], rb[80] = SA + NA, SB - 1, SB + NB  # a bad row of a, an earlier and a later bad row of b
        out = np.full(100, 12345.0)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            a.getPairsDot(b, ra, rb, out=out)
        assert ei.value.record == 17
        assert (out == 12345.0).all()  # nothing written
        rb[17] = SB
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            a.getPairsDot(b, ra, rb, out=out)
        assert ei.value.record == 40 and (out == 12345.0).all()
        ra[40] = SA
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            a.getPairsDot(b, ra, rb, out=out)
        assert ei.value.record == 80 and (out == 12345.0).all()


def test_pair_dot_errors_device(gpu):
    import torch
    with two_shards(gpu, "long", 67, "cyclic") as (a, A, b, B):
        la, lb = pair_rows(A.shape[0], B.shape[0], 100, "err")
        ra, rb = np.array(keys_of(a.partition, la)), np.array(keys_of(b.partition, lb))
        ra[40], rb[17], rb[80] = SA - 1, CYC[0] + CYC[1] * B.shape[0], CYC[0] - CYC[1]
        bad = np.zeros(100, bool)
        bad[[17, 40, 80]] = True
        out = torch.full((100,), 99, dtype=torch.int64, device=torch.device("cuda", gpu))
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            a.getPairsDot(b, dev_t(gpu, ra), dev_t(gpu, rb), out=out)
        assert ei.value.record == 17  # the lowest index, at a's sync
        got = out.cpu().numpy()
        assert (got[bad] == 0).all()  # bad pairs answer 0
        np.testing.assert_array_equal(got[~bad], replay_pair_dot(A[la[~bad]], B[lb[~bad]]))
        b.sync()  # nothing is reported on b


def test_pair_dot_argument_errors(gpu):
    lib = N.load()
    r = np.array([SA], np.int64)
    o = np.array([SB], np.int64)
    out = np.full(1, 5.0)
    rd, od, outd = dev_t(gpu, r), dev_t(gpu, o), dev_t(gpu, out)
    host = lib.glint_mat_pull_pairs_dot
    devc = lambda *args: lib.glint_mat_pull_pairs_dot_dev(*args, None)  # noqa: E731
    with PartialMatrix(RangePartition(0, SA, SA + 10), 4, "double", gpu) as a, \
            PartialMatrix(RangePartition(0, SB, SB + 10), 4, "double", gpu) as b, \
            PartialMatrix(RangePartition(0, SB, SB + 10), 5, "double", gpu) as wide, \
            PartialMatrix(RangePartition(0, SB, SB + 10), 4, "float", gpu) as flt, \
            PartialVector(RangePartition(0, SB, SB + 10), "double", gpu) as vec:
        for call, (pr, po, pout) in ((host, (r.ctypes.data, o.ctypes.data, out.ctypes.data)),
                                     (devc, (rd.data_ptr(), od.data_ptr(), outd.data_ptr()))):
            for x, y in ((None, b.handle), (a.handle, None), (vec.handle, b.handle), (a.handle, vec.handle),
                         (a.handle, wide.handle), (a.handle, flt.handle)):
                assert call(x, y, pr, po, 1, pout) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, po, -1, pout) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, po, 1 << 31, pout) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, None, po, 1, pout) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, None, 1, pout) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, po, 1, None) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, None, None, 0, None) == N.GLINT_OK  # n == 0 writes nothing
            assert call(a.handle, b.handle, pr, po, 1, pout) == N.GLINT_OK
        a.sync()
        assert out[0] == 0.0 and outd.cpu().numpy()[0] == 0.0
        if lib.glint_device_count() > 1:
            with PartialMatrix(RangePartition(0, SB, SB + 10), 4, "double", (gpu + 1) % lib.glint_device_count()) as far:
                assert host(a.handle, far.handle, r.ctypes.data, o.ctypes.data, 1, out.ctypes.data) == N.GLINT_EINVAL
        for args in ((wide, r, o), (flt, r, o), (vec, r, o), (b, r, np.array([SB, SB]))):
            with pytest.raises((ValueError, TypeError)):  # the wrapper refuses before any call
                a.getPairsDot(*args)
        with pytest.raises(TypeError):
            a.getPairsDot(b, rd, o)  # mixing device tensors and host arrays
    # a slab that has views: the device call refuses it for either shard (the host call as every host call)
    slab = PartialMatrix(RangePartition(0, 0, 128), 4, "double", gpu)
    view = PartialMatrix.view(slab, RangePartition(0, SA, SA + 64), 0)
    try:
        with PartialMatrix(RangePartition(0, SB, SB + 10), 4, "double", gpu) as b:
            zero = dev_t(gpu, np.array([0], np.int64))
            for x, y, px, py in ((slab, b, zero, od), (b, slab, od, zero)):
                assert lib.glint_mat_pull_pairs_dot_dev(x.handle, y.handle, px.data_ptr(), py.data_ptr(), 1,
                                                        outd.data_ptr(), None) == N.GLINT_EINVAL
            assert view.getPairsDot(b, rd, od).cpu().numpy()[0] == 0.0  # the view itself is a shard like any other
    finally:
        view.destroy()
        slab.destroy()


# ---- pair axpy: against updateRows of the replayed contributions -------------------------------------------
RUNS = (1, 2, 63, 64, 65, 129, 300)  # the 64-id batch, a remainder of the load depth, the kRowsChunk split


@functools.lru_cache(maxsize=None)
def axpy_rows(nd, ns, seed, runs=RUNS):
    """Local (dst, src) rows: one destination row per run length of RUNS, each with that many records, and
    200 records on random rows, shuffled; sources with repeats. Read-only, shared."""
    rng = np.random.default_rng(zlib.crc32(f"pairs/axpy/{nd}/{ns}/{seed}".encode()))
    heads = rng.choice(nd, len(runs), replace=False)
    ld = np.concatenate([np.repeat(heads, runs), rng.integers(0, nd, 200)])
    rng.shuffle(ld)
    ls = rng.choice(rng.choice(ns, max(1, ns // 2), replace=False), ld.size)
    for x in (ld, ls):
        x.setflags(write=False)
    return ld, ls


def push_pairs(dst, src, rd, rs, coef, path, gpu):
    kw = dict(unordered=path.endswith("unordered"), deterministic=path.endswith("det"))
    if path.startswith("host"):
        assert dst.updatePairsAxpy(src, rd, rs, coef, **kw)
    else:
        assert dst.updatePairsAxpy(src, dev_t(gpu, rd), dev_t(gpu, rs), dev_t(gpu, coef), **kw)


def check_axpy(gpu, dtype, dst, D, ld, contrib, path, twin_part):
    """dst's content against updateRows of the contributions onto a twin shard that starts from the same
    image: bit for bit where the order is kept (and for Int/Long), else within test_gpu_axpy.check's bar."""
    cols = D.shape[1]
    with PartialMatrix(twin_part, cols, dtype, gpu) as twin:
        write_image(twin, gpu, D, PAD)
        twin.updateRows(keys_of(twin_part, ld), contrib)
        want = twin.to_numpy()
    got = dst.to_numpy()
    if dtype in ("long", "int") or path in ("host", "dev_det"):
        assert_bits(got, want, path)
        return
    mag = np.abs(D.astype(np.float64))
    terms = np.ones(D.shape[0], np.int64)
    np.add.at(terms, ld, 1)
    with np.errstate(invalid="ignore", over="ignore"):
        np.add.at(mag, ld, np.abs(contrib.astype(np.float64)))
    check(got, want, mag, terms, dtype, False)


@pytest.mark.parametrize("path", AXPY_PATHS)
@pytest.mark.parametrize("dtype,cols", [(dt, c) for dt in DT for c in WIDTHS])
def test_pair_axpy_parity(gpu, dtype, cols, path):
    with two_shards(gpu, dtype, cols, "range", "axpy") as (dst, D, src, S):
        ld, ls = axpy_rows(NA, NB, "parity")
        coef = pair_coef(np.dtype(npd_of(dtype)).name, ld.size)
        push_pairs(dst, src, keys_of(dst.partition, ld), keys_of(src.partition, ls), coef, path, gpu)
        check_axpy(gpu, dtype, dst, D, ld, pair_contrib(coef, S[ls]), path, dst.partition)
        assert_bits(src.to_numpy(), S)  # the source is only read


@pytest.mark.parametrize("path", ["host", "dev", "dev_det"])
@pytest.mark.parametrize("dtype,cols,parts", [(dt, c, p) for dt in ("double", "long") for c in (67, 128)
                                              for p in AXPY_PARTS[1:]])
def test_pair_axpy_partitions(gpu, dtype, cols, parts, path):
    with two_shards(gpu, dtype, cols, parts, "axpy") as (dst, D, src, S):
        ld, ls = axpy_rows(D.shape[0], S.shape[0], parts)
        coef = pair_coef(np.dtype(npd_of(dtype)).name, ld.size)
        push_pairs(dst, src, keys_of(dst.partition, ld), keys_of(src.partition, ls), coef, path, gpu)
        twin = dst.partition if parts != "views_apart" else RangePartition(0, SA, SA + NA)
        check_axpy(gpu, dtype, dst, D, ld, pair_contrib(coef, S[ls]), path, twin)
        assert_bits(src.to_numpy(), S)


@pytest.mark.parametrize("size", [255, 256, 257, 65_537])
def test_pair_axpy_sort_passes(gpu, size):
    """Destination shards whose sentinel key needs one, two and three passes of the unchanged front end's
    sort, at cols = 4: records over the whole shard, its last row included. Long on the device default,
    Double in host order and with deterministic=True."""
    cols = 4
    for dtype, path in (("long", "dev"), ("double", "host"), ("double", "dev_det")):
        name = np.dtype(npd_of(dtype)).name
        rng = np.random.default_rng(zlib.crc32(f"pairs/sort/{size}/{dtype}/{path}".encode()))
        part = RangePartition(2, SA, SA + size)
        D, S = pair_values(name, size, cols, "sort/d"), pair_values(name, NB, cols, "sort/s")
        ld = np.concatenate([rng.integers(0, size, 3000), [size - 1, 0, size - 1]])
        ls = rng.integers(0, NB, ld.size)
        coef = pair_coef(name, ld.size, "sort")
        with PartialMatrix(part, cols, dtype, gpu) as dst, PartialMatrix(RangePartition(1, SB, SB + NB), cols, dtype,
                                                                        gpu) as src:
            write_image(dst, gpu, D, PAD)
            write_image(src, gpu, S, PAD)
            push_pairs(dst, src, ld + SA, ls + SB, coef, path, gpu)
            assert_bits(dst.to_numpy(), replay_pair_axpy(D, ld, coef, S[ls]), f"{size}/{dtype}/{path}")


# ---- pair axpy: arithmetic and aliasing ---------------------------------------------------------------------
@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("run", [1, 3])
@pytest.mark.parametrize("dtype,cols", [("double", 2), ("double", 67), ("float", 4), ("float", 67)])
def test_pair_axpy_is_unfused(gpu, dtype, cols, run, path):
    """axpy_cases.nofma_element with its vector stored as the source row: dst = -b plus coef * src = a * a
    is exactly +0 with a rounded product and 2^-54 / 2^-24 fused. As a single record, and as the middle
    record of a run of three for one row (the others with zero coefficients); 16-B and scalar slices."""
    npd = npd_of(dtype)
    c = cols - 1 if cols > 4 else 1
    elem, coef1, x, fused = nofma_element(npd, cols, c)
    with PartialMatrix(RangePartition(0, SA, SA + 8), cols, dtype, gpu) as dst, \
            PartialMatrix(RangePartition(0, SB, SB + 8), cols, dtype, gpu) as src:
        D, S = np.zeros((8, cols), npd), np.zeros((8, cols), npd)
        D[5], S[2] = elem, x[0]
        write_image(dst, gpu, D, PAD)
        write_image(src, gpu, S, PAD)
        coef = np.zeros(run, npd)
        coef[run // 2] = coef1[0, 0]
        push_pairs(dst, src, np.full(run, SA + 5, np.int64), np.full(run, SB + 2, np.int64), coef, path, gpu)
        got = dst.to_numpy()
        assert bits(got)[5, c] == 0, f"{got[5, c]!r}: a fused product would leave {fused!r}"
        assert not got.any()


@pytest.mark.parametrize("path", ["host", "dev_det", "dev"])
def test_pair_axpy_many_records_share_one_source_row(gpu, path):
    with two_shards(gpu, "long", 130, "range", "axpy") as (dst, D, src, S):
        ld = axpy_rows(NA, NB, "one_src")[0]
        ls = np.full(ld.size, 7, np.int64)
        coef = pair_coef("int64", ld.size)
        push_pairs(dst, src, ld + SA, ls + SB, coef, path, gpu)
        np.testing.assert_array_equal(dst.to_numpy(), replay_pair_axpy(D, ld, coef, S[ls]))


def test_pair_axpy_source_must_not_share_memory(gpu):
    lib = N.load()
    r = np.array([SA], np.int64)
    c = np.ones(1)
    rd, cd = dev_t(gpu, r), dev_t(gpu, c)
    with two_shards(gpu, "double", 4, "views") as (a, A, b, _):       # rows [0, 300) and [128, 339) of one slab
        o = np.array([SB], np.int64)
        od = dev_t(gpu, o)
        for dst, src, pd, ps in ((a, a, r, r), (a, b, r, o), (b, a, o, r)):
            assert lib.glint_mat_push_pairs_axpy(dst.handle, src.handle, pd.ctypes.data, ps.ctypes.data,
                                                 c.ctypes.data, 1, 0) == N.GLINT_EINVAL
        assert lib.glint_mat_push_pairs_axpy_dev(a.handle, a.handle, rd.data_ptr(), rd.data_ptr(), cd.data_ptr(), 1, 0,
                                                 None) == N.GLINT_EINVAL
        assert lib.glint_mat_push_pairs_axpy_dev(a.handle, b.handle, rd.data_ptr(), od.data_ptr(), cd.data_ptr(), 1, 0,
                                                 None) == N.GLINT_EINVAL
        with pytest.raises(ValueError):
            a.updatePairsAxpy(b, r, o, c)
        assert_bits(a.to_numpy(), A)


def test_pair_axpy_argument_errors(gpu):
    lib = N.load()
    r, o, c = np.array([SA], np.int64), np.array([SB], np.int64), np.full(1, 2.0)
    rd, od, cd = dev_t(gpu, r), dev_t(gpu, o), dev_t(gpu, c)
    host = lib.glint_mat_push_pairs_axpy
    devc = lambda *args: lib.glint_mat_push_pairs_axpy_dev(*args, None)  # noqa: E731
    with PartialMatrix(RangePartition(0, SA, SA + 10), 4, "double", gpu) as a, \
            PartialMatrix(RangePartition(0, SB, SB + 10), 4, "double", gpu) as b, \
            PartialMatrix(RangePartition(0, SB, SB + 10), 5, "double", gpu) as wide, \
            PartialMatrix(RangePartition(0, SB, SB + 10), 4, "float", gpu) as flt, \
            PartialVector(RangePartition(0, SB, SB + 10), "double", gpu) as vec:
        b.updateRows(o, np.ones((1, 4)))
        for call, (pr, po, pc) in ((host, (r.ctypes.data, o.ctypes.data, c.ctypes.data)),
                                   (devc, (rd.data_ptr(), od.data_ptr(), cd.data_ptr()))):
            for x, y in ((None, b.handle), (a.handle, None), (vec.handle, b.handle), (a.handle, vec.handle),
                         (a.handle, wide.handle), (a.handle, flt.handle)):
                assert call(x, y, pr, po, pc, 1, 0) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, po, pc, 1, N.GLINT_PUSH_VALIDATE) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, po, pc, 1, 8) == N.GLINT_EINVAL  # unknown flag bit
            assert call(a.handle, b.handle, pr, po, pc, -1, 0) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, po, pc, (1 << 32) - 2048, 0) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, None, po, pc, 1, 0) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, None, pc, 1, 0) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, pr, po, None, 1, 0) == N.GLINT_EINVAL
            assert call(a.handle, b.handle, None, None, None, 0, 0) == N.GLINT_OK
        assert not a.to_numpy().any()
        for args in ((wide, r, o, c), (flt, r, o, c), (vec, r, o, c), (b, r, np.array([SB, SB]), c),
                     (b, r, o, np.ones(2))):
            with pytest.raises((ValueError, TypeError)):
                a.updatePairsAxpy(*args)
        with pytest.raises(TypeError):
            a.updatePairsAxpy(b, rd, od, c)  # coef on the host
        assert a.updatePairsAxpy(b, r, o, c) and a.updatePairsAxpy(b, rd, od, cd)
        np.testing.assert_array_equal(a.to_numpy()[0], np.full(4, 4.0))


# ---- pair axpy: errors --------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("float", 6)])
def test_pair_axpy_errors_host(gpu, dtype, cols):
    """A bad pair of either kind: nothing is applied -- the whole image, pitch padding included, keeps its
    bits in both shards."""
    with two_shards(gpu, dtype, cols, "range", "axpy") as (dst, D, src, S):
        ld, ls = axpy_rows(NA, NB, "err")
        rd, rs = np.array(ld + SA), np.array(ls + SB)
        coef = pair_coef(np.dtype(npd_of(dtype)).name, ld.size)
        pitch = C.c_int64()
        assert N.load().glint_shard_pitch(dst.handle, C.byref(pitch)) == N.GLINT_OK
        before = read_image(dst, gpu, NA, pitch.value)
        for (i_d, i_s), first in (((400, 90), 90), ((90, 400), 90), ((55, None), 55), ((None, 7), 7)):
            bd, bs = np.array(rd), np.array(rs)
            if i_d is not None:
                bd[i_d] = SA + NA
            if i_s is not None:
                bs[i_s] = SB - 1
            with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
                dst.updatePairsAxpy(src, bd, bs, coef)
            assert ei.value.record == first  # the lowest index over both arrays
            np.testing.assert_array_equal(bits(read_image(dst, gpu, NA, pitch.value)), bits(before))
        assert (before[:, cols:] == PAD).all()
        assert_bits(src.to_numpy(), S)


@pytest.mark.parametrize("path", ["dev", "dev_det", "dev_unordered"])
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("float", 128)])
def test_pair_axpy_errors_device(gpu, dtype, cols, path):
    """A record with either row outside contributes nothing -- not +0: two destination rows seeded with
    -0.0 whose every record names a bad source row (a run of 300, which the default path splits into
    chunks, and a run of 2) keep their bits -- the lowest index is reported at dst's sync, and the other
    records are applied."""
    npd = npd_of(dtype)
    with two_shards(gpu, dtype, cols, "range", "axpy") as (dst, D, src, S):
        ld, ls = axpy_rows(NA, NB, "parity")
        count = np.bincount(ld, minlength=NA)
        all_bad = sorted({int(np.flatnonzero(count >= 300)[0]), int(np.flatnonzero(count == 2)[0])})
        assert len(all_bad) == 2
        D = np.array(D)
        D[all_bad] = npd(-0.0)
        write_image(dst, gpu, D, PAD)
        rd, rs = np.array(ld + SA), np.array(ls + SB)
        bad = np.isin(ld, all_bad)
        rs[bad] = np.where(np.arange(bad.sum()) % 2 == 0, SB - 1, SB + NB)
        lone = np.flatnonzero(~bad)[[3, 50]]
        rs[lone[0]] = SB + NB + 5   # a bad source inside a run that also has good records
        rd[lone[1]] = SA - 1        # a bad destination
        bad[lone] = True
        coef = pair_coef(np.dtype(npd).name, ld.size)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push_pairs(dst, src, rd, rs, coef, path, gpu)
        assert ei.value.record == int(np.flatnonzero(bad)[0])
        got = dst.to_numpy()
        assert (bits(got[all_bad]) == bits(npd(-0.0))).all()  # as if the records were absent
        keep = ~bad
        check_axpy(gpu, dtype, dst, D, ld[keep], pair_contrib(coef[keep], S[ls[keep]]), path, dst.partition)
        src.sync()  # nothing is reported on src


# ---- IEEE edges ---------------------------------------------------------------------------------------------
def edge_tables(dtype, cols):
    """Two small tables over ieee_cases' values: infinities, NaNs with payloads, +/-max, subnormals and
    values whose products are subnormal, zeros of both signs, among ordinary values."""
    npd = npd_of(dtype)
    sub = np.ldexp(1.0, GRIDS[dtype]["subnormal"] + 3)
    small = (2.0 ** -540, 2.0 ** -520) if dtype == "double" else (2.0 ** -70, 2.0 ** -70)
    vals = [special(v, dtype) for v in ("+inf", "-inf", "nan", "-nan", "+max", "-max")] + \
           [npd(v) for v in (0.0, -0.0, sub, -sub, small[0], small[1], 1.0, -1.0, 3.0, 0.5)]
    rng = np.random.default_rng(zlib.crc32(f"pairs/edges/{dtype}/{cols}".encode()))
    A = np.array(vals, npd)[rng.integers(0, len(vals), (16, cols))]
    B = np.array(vals, npd)[rng.integers(0, len(vals), (16, cols))]
    A[0, 0], B[0, 0] = np.inf, 0.0            # inf * 0
    A[1], B[1] = small[0], small[1]           # every product subnormal
    A[2], B[2] = -0.0, 1.0                    # -0 products
    return A, B, small


@pytest.mark.parametrize("path", ["host", "dev"])
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("double", 6), ("float", 67), ("float", 12)])
def test_pair_dot_ieee_edges(gpu, dtype, cols, path):
    A, B, _ = edge_tables(dtype, cols)
    with PartialMatrix(RangePartition(0, SA, SA + 16), cols, dtype, gpu) as a, \
            PartialMatrix(RangePartition(0, SB, SB + 16), cols, dtype, gpu) as b:
        write_image(a, gpu, A, PAD)
        write_image(b, gpu, B, PAD)
        la = np.repeat(np.arange(16), 16)
        lb = np.tile(np.arange(16), 16)
        exp = replay_pair_dot(A[la], B[lb])
        assert np.isnan(exp[0]) and exp[17] != 0 and abs(exp[17]) < np.finfo(A.dtype).tiny  # the premises
        assert_dot_bits(pairs_dot(a, b, la + SA, lb + SB, path, gpu), exp)


@pytest.mark.parametrize("path", ["host", "dev", "dev_det"])
@pytest.mark.parametrize("dtype,cols", [("double", 67), ("double", 6), ("float", 67), ("float", 12)])
def test_pair_axpy_ieee_edges(gpu, dtype, cols, path):
    """Subnormal products kept, inf * 0 is NaN, -0.0 products onto a -0.0 element, and the pitch padding
    neither read nor written; each against the replay, a NaN by class. No destination row repeats, so the
    device default is in order too."""
    npd = npd_of(dtype)
    S, D, small = edge_tables(dtype, cols)
    D = np.where(np.isnan(D) | np.isinf(D), npd(2.0), D).astype(npd)
    D[2] = -0.0
    ld = np.arange(16)
    ls = np.array([0, 1, 2] + list(range(3, 16)))
    coef = np.array([0.0, small[1], 1.0, -0.0, 2.0, small[0], -1.0, 0.5] * 2, npd)
    exp = replay_pair_axpy(D, ld, coef, S[ls])
    assert np.isnan(exp[0, 0]) and (bits(exp[2]) == bits(npd(-0.0))).all()  # inf * 0; -0 + (1 * -0)
    t = pair_contrib(coef, S[ls])
    assert t[1, 0] != 0 and abs(t[1, 0]) < np.finfo(npd).tiny
    with PartialMatrix(RangePartition(0, SA, SA + 16), cols, dtype, gpu) as dst, \
            PartialMatrix(RangePartition(0, SB, SB + 16), cols, dtype, gpu) as src:
        write_image(dst, gpu, D, PAD)
        write_image(src, gpu, S, PAD)
        push_pairs(dst, src, ld + SA, ls + SB, coef, path, gpu)
        pitch = C.c_int64()
        assert N.load().glint_shard_pitch(dst.handle, C.byref(pitch)) == N.GLINT_OK
        raw = read_image(dst, gpu, 16, pitch.value)
        assert_bits(raw[:, :cols], exp)
        assert (raw[:, cols:] == PAD).all()  # neither read (no NaN, no sum) nor written


# ---- profiling ----------------------------------------------------------------------------------------------
def launches(sh):
    out = []
    for kid in range(N.GLINT_K_COUNT):
        ms, cnt = C.c_double(), C.c_int64()
        assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
        out.append(cnt.value)
    return out


@pytest.mark.parametrize("dev", [False, True])
def test_pair_calls_profiling(gpu, dev):
    with two_shards(gpu, "double", 6, "range") as (a, A, b, B), \
            PartialMatrix(RangePartition(2, SA, SA + NA), 6, "double", gpu) as twin:
        for sh in (a, b, twin):
            assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        ld, ls = axpy_rows(NA, NB, "parity")
        rd, rs, coef = ld + SA, ls + SB, pair_coef("float64", ld.size)
        conv = (lambda x: dev_t(gpu, x)) if dev else (lambda x: x)  # noqa: E731
        a.getPairsDot(b, conv(rd), conv(rs))
        want = [0] * N.GLINT_K_COUNT
        want[N.GLINT_K_PULL_ROWS_DOT] = 1
        assert launches(a) == want            # one launch under the dot pull's id on a
        assert launches(b) == [0] * N.GLINT_K_COUNT  # nothing of any kind on b
        assert N.load().glint_prof_reset(a.handle) == N.GLINT_OK
        a.updatePairsAxpy(b, conv(rd), conv(rs), conv(coef))
        twin.updateRowsAxpy(conv(rd), conv(coef), conv(np.ones(6)))
        got = launches(a)
        assert got == launches(twin) and got[N.GLINT_K_PUSH_ROWS_AXPY] == 1  # as the row axpy push counts
        assert launches(b) == [0] * N.GLINT_K_COUNT
        a.updatePairsAxpy(b, conv(rd[:0]), conv(rs[:0]), conv(coef[:0]))  # an empty call launches nothing
        a.getPairsDot(b, conv(rd[:0]), conv(rs[:0]))
        assert launches(a) == got


# ---- stream order -------------------------------------------------------------------------------------------
def test_pair_axpy_then_pair_dot_on_one_stream(gpu):
    """A device pair axpy, then a device pair dot that reads the destination, no sync in between."""
    with two_shards(gpu, "long", 67, "cyclic", "stream") as (dst, D, src, S):
        ld, ls = axpy_rows(NA, S.shape[0], "stream")
        rd, rs = dev_t(gpu, ld + SA), dev_t(gpu, keys_of(src.partition, ls))
        coef = pair_coef("int64", ld.size)
        dst.updatePairsAxpy(src, rd, rs, dev_t(gpu, coef), sync=False)
        out = dst.getPairsDot(src, rd, rs, sync=False)
        dst.sync(dst._stream_of(rd))
        after = replay_pair_axpy(D, ld, coef, S[ls])
        assert (after != D).any()
        np.testing.assert_array_equal(out.cpu().numpy(), replay_pair_dot(after[ld], S[ls]))


# ---- client -------------------------------------------------------------------------------------------------
def test_pair_calls_client(gpu):
    cols = 67
    c = Client([gpu])
    A = c.matrix(1000, cols, "double", modelsPerServer=3)
    B = c.matrix(611, cols, "double", modelsPerServer=3)
    assert A.nrOfPartitions == 3 and B.nrOfPartitions == 3
    TA, TB = pair_values("float64", 1000, cols, "client/a"), pair_values("float64", 611, cols, "client/b")
    A.pushRows(np.arange(1000), TA)
    B.pushRows(np.arange(611), TB)
    rng = np.random.default_rng(12)
    ra, rb = rng.integers(0, 1000, 3000).astype(np.int64), rng.integers(0, 611, 3000).astype(np.int64)
    assert_dot_bits(A.pullPairDot(B, ra, rb), replay_pair_dot(TA[ra], TB[rb]))
    coef = pair_coef("float64", 3000, "client")
    assert A.pushPairAxpy(B, ra, rb, coef)
    own = RangePartitioner.apply(3, 1000).partition_indices(ra)
    oth = RangePartitioner.apply(3, 611).partition_indices(rb)
    order = np.lexsort((np.arange(3000), oth, own))  # the documented bucket order
    assert_bits(A.pull(np.arange(1000)), replay_pair_axpy(TA, ra, coef, TB[rb], order=order))
    assert_bits(B.pull(np.arange(611)), TB)
    with pytest.raises(ValueError):
        A.pushPairAxpy(A, ra, ra, coef)
    assert_dot_bits(A.pullPairDot(A, ra[:100], ra[100:200]),
                    replay_pair_dot(A.pull(ra[:100]), A.pull(ra[100:200])))
    A.destroy()
    B.destroy()
