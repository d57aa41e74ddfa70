"""Every push and pull path at IEEE-754 edge values: subnormals, signed zeros, infinities, NaNs and
values near the overflow limit (cases from tests/ieee_cases.py; tests/test_ieee_cpu.py holds the same
cases against the oracle alone).

Everything is compared bit for bit through an integer view. The unordered paths can be held to that
because the exact-grid cases have one result in every summation order (ieee_cases' docstring); the
non-finite cases compare the class of the chosen elements (NaN payloads are not promised) and the bits
of everything else -- the other half of a chosen element's pair, its neighbours across a slab
boundary, the next column. Where a path has a profiling id the test asserts from glint_prof_read that
this path ran.
"""
import ctypes as C

import numpy as np
import pytest

import ieee_cases as I
from glint_amd import _native as N
from glint_amd import PartialMatrix, PartialVector, RangePartition
from oracle import oracle as O

pytestmark = pytest.mark.gpu
DT = ["float", "double"]
CASES = ["subnormal", "crossing", "unit", "top", "nonfinite"]
START = 1_000_003  # the shards' first global key


def launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def profiled(sh):
    assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
    return sh


def dev(gpu, a):
    import torch
    return torch.from_numpy(np.array(a)).to(torch.device("cuda", gpu))


def pushes_of(case, shape, dtype):
    """([(keys, vals), ...], expect per push, class map or None): an exact grid pushed twice, or the
    non-finite push followed by one of ordinary values."""
    if case == "nonfinite":
        nf = I.nonfinite_case(shape, dtype)
        return nf.pushes, nf.expect, nf.cls
    keys, vals, expect = I.grid_case(shape, dtype, case)
    return [(keys, vals)] * 2, expect, None


def vector_shard(shape, dtype, gpu):
    size = I.SHAPES[shape][2]
    return profiled(PartialVector(RangePartition(1, START, START + size), dtype, gpu))


def run(sh, case, shape, dtype, push):
    """push(keys, vals) for each push of the case, the shard compared after each; returns the count."""
    pushes, expect, cls = pushes_of(case, shape, dtype)
    for p, (keys, vals) in enumerate(pushes):
        push(keys + START, vals)
        I.assert_matches(sh.to_numpy(), expect[p], cls, f"{shape}/{dtype}/{case} push {p + 1}")
    return len(pushes)


# ---- unordered and default device paths -------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", ["dense", "dense_odd_start"])
def test_dense_apply(gpu, shape, dtype, case):
    """Increasing unique keys, 9001 / 9000 device records (above kSmallPushMax = 4096, 16-byte aligned
    tensors): push_check finds no break and push_apply's paired read-modify-write takes every record.
    ``dense_odd_start`` begins at local element 1, so every record pair straddles two element pairs."""
    with vector_shard(shape, dtype, gpu) as sh:
        n = run(sh, case, shape, dtype, lambda k, v: sh.update(dev(gpu, k), dev(gpu, v)))
        assert launches(sh, N.GLINT_K_PUSH_APPLY) == n
        assert launches(sh, N.GLINT_K_PUSH_BINNED) == 0 and launches(sh, N.GLINT_K_PUSH_ORDERED) == 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
def test_dense_keys_from_unaligned_pointers(gpu, dtype, case):
    """The dense push from ``keys[1:]`` / ``vals[1:]`` of 16-byte aligned tensors. launch_push's
    ``vec_ok`` (keys 16-byte, values pair aligned) is false then, and the dispatch sends every record
    to the LDS-hash scatter instead of the dense apply: one scatter launch per push, no apply."""
    import torch
    with vector_shard("dense_odd_start", dtype, gpu) as sh:
        def push(k, v):
            kb, vb = torch.empty(k.size + 1, dtype=torch.int64, device=f"cuda:{gpu}"), dev(gpu, np.append(v[:1], v))
            kb[1:] = dev(gpu, k)
            assert kb[1:].data_ptr() % 16 == 8
            sh.update(kb[1:], vb[1:])
        n = run(sh, case, "dense_odd_start", dtype, push)
        assert launches(sh, N.GLINT_K_PUSH_SCATTER) == n and launches(sh, N.GLINT_K_PUSH_APPLY) == 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", ["dups1000", "dups4096"])
def test_one_launch_scatter(gpu, shape, dtype, case):
    """Device tensors of at most kSmallPushMax = 4096 records, duplicates on 64 keys: the scatter alone
    (LDS partial sums, one global atomic per distinct element and workgroup)."""
    with vector_shard(shape, dtype, gpu) as sh:
        n = run(sh, case, shape, dtype, lambda k, v: sh.update(dev(gpu, k), dev(gpu, v)))
        assert launches(sh, N.GLINT_K_PUSH_SCATTER) == n
        assert launches(sh, N.GLINT_K_PUSH_APPLY) == 0 and launches(sh, N.GLINT_K_PUSH_BINNED) == 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
def test_check_apply_and_scatter_tail(gpu, dtype, case):
    """An increasing prefix of 10 000 records, then 10 000 unordered ones, no hint, a fresh shard: the
    apply takes the records before the break and the scatter the tail (20 000 records are below
    kBinMin = 2^20, so the adaptive switch never bins it)."""
    with vector_shard("prefix_tail", dtype, gpu) as sh:
        n = run(sh, case, "prefix_tail", dtype, lambda k, v: sh.update(dev(gpu, k), dev(gpu, v)))
        assert launches(sh, N.GLINT_K_PUSH_APPLY) == n and launches(sh, N.GLINT_K_PUSH_SCATTER) == n
        assert launches(sh, N.GLINT_K_PUSH_BINNED) == 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("binned", ["default", "0"])
def test_host_unordered(gpu, monkeypatch, binned, dtype, case):
    """Host arrays with ``unordered=True``, 5000 records (more than kBatchMax = 4096, so the push is
    staged and launched on its own, not through the ring's ordered fold). The unordered flag sends a
    staged push to the binned pipeline (launch_push: ``binned && unordered``); with GLINT_BINNED=0 the
    same call is check + apply + scatter."""
    if binned == "0":
        monkeypatch.setenv("GLINT_BINNED", "0")
    else:
        monkeypatch.delenv("GLINT_BINNED", raising=False)
    N.reload_env()
    with vector_shard("uniform5000", dtype, gpu) as sh:
        n = run(sh, case, "uniform5000", dtype, lambda k, v: sh.update(k, v, unordered=True))
        assert launches(sh, N.GLINT_K_PUSH_ORDERED) == 0
        if binned == "0":
            assert launches(sh, N.GLINT_K_PUSH_SCATTER) == n and launches(sh, N.GLINT_K_PUSH_BINNED) == 0
        else:
            assert launches(sh, N.GLINT_K_PUSH_BINNED) == n and launches(sh, N.GLINT_K_PUSH_SCATTER) == 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("front", ["dedup", "hot", "prep"])
def test_binned_fronts(gpu, monkeypatch, front, dtype, case):
    """The binned pipeline with each front end forced, on 20 485 elements (five slabs and an odd
    partial one): 150 000 uniform records, 100 000 on one key (split items, flushed by global atomics)
    and 60 000 on 300 keys of one slab (the hot-slab split)."""
    monkeypatch.setenv("GLINT_BIN_FRONT", front)
    monkeypatch.delenv("GLINT_BINNED", raising=False)
    N.reload_env()
    with vector_shard("binned", dtype, gpu) as sh:
        n = run(sh, case, "binned", dtype, lambda k, v: sh.update(dev(gpu, k), dev(gpu, v), unordered=True))
        assert launches(sh, N.GLINT_K_PUSH_BINNED) == n
        assert launches(sh, N.GLINT_K_PUSH_SCATTER) == 0 and launches(sh, N.GLINT_K_PUSH_APPLY) == 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("front", ["dedup", "hot", "prep"])
@pytest.mark.parametrize("shape", ["binned_mat3", "binned_mat64"])
def test_binned_fronts_matrix(gpu, monkeypatch, shape, front, dtype, case):
    """The same records as (row, column) triplets of a 6827 x 3 and a 321 x 64 matrix; the chosen
    elements include column 0 and the last column."""
    monkeypatch.setenv("GLINT_BIN_FRONT", front)
    monkeypatch.delenv("GLINT_BINNED", raising=False)
    N.reload_env()
    _, _, elems, _, cols = I.SHAPES[shape]
    with profiled(PartialMatrix(RangePartition(1, START, START + elems // cols), cols, dtype, gpu)) as sh:
        def push(k, v):  # (k arrives rebased by START: flat cell -> row + START, column)
            k = k - START
            sh.update(dev(gpu, k // cols + START), dev(gpu, (k % cols).astype(np.int32)), dev(gpu, v), unordered=True)
        n = run(sh, case, shape, dtype, push)
        assert launches(sh, N.GLINT_K_PUSH_BINNED) == n and launches(sh, N.GLINT_K_PUSH_SCATTER) == 0


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
def test_set_push(gpu, dtype, case):
    """glint_vec_push_dev_shards over three shards whose ranges are given out of order; the 30 000
    records cross all three. The set's scatter adds every record with one global atomic; its launches
    are accounted to the shard with the lowest range."""
    import torch
    size = I.SHAPES["uniform30000"][2]
    ranges = [(6000, size), (0, 2500), (2500, 6000)]
    shards = [PartialVector(RangePartition(i, START + a, START + b), dtype, gpu) for i, (a, b) in enumerate(ranges)]
    for sh in shards:
        profiled(sh)
    d = torch.device("cuda", gpu)
    gate = torch.full((1,), 7, dtype=torch.int64, device=d)
    hs = (C.c_void_p * 3)(*[s.handle for s in shards])
    st = torch.cuda.current_stream(d).cuda_stream
    pushes, expect, cls = pushes_of(case, "uniform30000", dtype)
    try:
        for p, (keys, vals) in enumerate(pushes):
            kt, vt = dev(gpu, keys + START), dev(gpu, vals)
            assert N.load().glint_vec_push_dev_shards(hs, 3, kt.data_ptr(), vt.data_ptr(), kt.numel(),
                                                      gate.data_ptr(), st) == N.GLINT_OK
            shards[0].sync(st)
            assert int(gate.item()) == 0
            got = np.empty(size, I.NPD[dtype])
            for sh, (a, b) in zip(shards, ranges):
                got[a:b] = sh.to_numpy()
            I.assert_matches(got, expect[p], cls, f"set/{dtype}/{case} push {p + 1}")
        assert [launches(sh, N.GLINT_K_PUSH_SCATTER) for sh in shards] == [0, len(pushes), 0]
    finally:
        for sh in shards:
            sh.destroy()


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", ["rows3", "rows64"])
def test_row_push_device_default(gpu, shape, dtype, case):
    """updateRows with device tensors, no flag: one row gets 300 contributions (a run longer than
    kRowsChunk = 128 is split into chunks that add with global atomics), the others one or two.
    3 columns are scalar slices, 64 columns 16-byte slices."""
    _, _, rows, cols, _ = I.SHAPES[shape]
    with profiled(PartialMatrix(RangePartition(1, START, START + rows), cols, dtype, gpu)) as sh:
        n = run(sh, case, shape, dtype, lambda k, v: sh.updateRows(dev(gpu, k), dev(gpu, v)))
        assert launches(sh, N.GLINT_K_PUSH_ROWS) == n


# ---- ordered paths ------------------------------------------------------------------------------------
def ordered_shard(shape, dtype, gpu):
    """The shard of an ordered case with its start image (-0.0 under two vectors) written as memory."""
    spec = I.ORDERED_SHAPES[shape]
    case = I.ordered_shape(shape, dtype)
    cols = spec.get("cols", 0)
    if cols:
        rows = case.init.size // cols
        sh = PartialMatrix(RangePartition(1, START, START + rows), cols, dtype, gpu)
    else:
        rows, cols = case.init.size, 1
        sh = PartialVector(RangePartition(1, START, START + rows), dtype, gpu)
    I.write_image(sh, gpu, case.init.reshape(rows, cols), 1)
    return profiled(sh), case


def check_ordered(sh, case, what):
    I.assert_matches(sh.to_numpy(), case.expect, case.cls, what)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("path,shape", [
    ("host", "msg1000"), ("host", "fold4097"), ("host_det", "msg1000"), ("host_det", "fold4097"),
    ("wire", "msg1000"), ("async", "msg1000"), ("async3", "msg1000"), ("dev_det", "fold4097")])
def test_ordered_fold(gpu, path, shape, dtype):
    """The ordered vectors, a non-finite set and subnormal traffic through every entry that promises
    the message order and runs the ordered fold: host update (the ring below kBatchMax = 4096 records,
    a staged launch above), the wire image, push_async as one message and as three consecutive ones
    that coalesce into one launch, and a deterministic device push of 4097 records (kOrdCap = 4096:
    more than one LDS list)."""
    sh, case = ordered_shard(shape, dtype, gpu)
    with sh:
        keys, vals = case.keys + START, case.vals
        want_launches = 1
        if path in ("host", "host_det"):
            sh.update(keys, vals, deterministic=path == "host_det")
        elif path == "wire":
            assert sh.push_wire(O.encode_push_vector(O.CODE[dtype], 11, keys, vals)) == 11
        elif path == "async":
            sh.wait(sh.push_async(keys, vals))
        elif path == "async3":
            for part in np.array_split(np.arange(keys.size), 3):
                t = sh.push_async(keys[part], vals[part])
            sh.wait(t)
        else:
            sh.update(dev(gpu, keys), dev(gpu, vals), deterministic=True)
        assert launches(sh, N.GLINT_K_PUSH_ORDERED) == want_launches
        check_ordered(sh, case, f"{path}/{shape}/{dtype}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", ["sort131073", "sort524289"])
def test_ordered_sort_tail(gpu, shape, dtype):
    """Deterministic device pushes above kOrderedMax = 2^17 records take the stable sort and the
    chain folds. 131 073 records with a 70 000-record chain on one key: the chain is one long run.
    det_tail_k splits hot chains off only from 8 * kHotMinRecords = 2^19 records on, so the split is
    reached by the second shape: 524 289 records with an 80 000-record chain (2500 of the 16 384
    samples, above the threshold of 2047 that stands for kHotMinRecords = 2^16 records)."""
    sh, case = ordered_shard(shape, dtype, gpu)
    with sh:
        sh.update(dev(gpu, case.keys + START), dev(gpu, case.vals), deterministic=True)
        assert launches(sh, N.GLINT_K_PUSH_ORDERED) == 0 and launches(sh, N.GLINT_K_PUSH_BINNED) == 0
        check_ordered(sh, case, f"{shape}/{dtype}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", ["rows3", "rows64"])
@pytest.mark.parametrize("path", ["host", "dev_det"])
def test_ordered_row_push(gpu, path, shape, dtype):
    """updateRows from host arrays (message order by default) and from device tensors with
    ``deterministic=True``; one row gets 300 records, which stay one run here."""
    sh, case = ordered_shard(shape, dtype, gpu)
    with sh:
        if path == "host":
            sh.updateRows(case.keys + START, case.vals)
        else:
            sh.updateRows(dev(gpu, case.keys + START), dev(gpu, case.vals), deterministic=True)
        assert launches(sh, N.GLINT_K_PUSH_ROWS) == 1
        check_ordered(sh, case, f"{path}/{shape}/{dtype}")


@pytest.mark.parametrize("dtype", DT)
def test_ordered_matrix_triplets_from_host(gpu, dtype):
    sh, case = ordered_shard("mat3", dtype, gpu)
    with sh:
        sh.update(case.keys // 3 + START, (case.keys % 3).astype(np.int32), case.vals)
        assert launches(sh, N.GLINT_K_PUSH_ORDERED) == 1
        check_ordered(sh, case, f"mat3/{dtype}")


# ---- elements no record addresses -------------------------------------------------------------------------
def _push_fn(sh, gpu, how):
    if how == "dev":
        return lambda k, v: sh.update(dev(gpu, k), dev(gpu, v))
    if how == "dev_unordered":
        return lambda k, v: sh.update(dev(gpu, k), dev(gpu, v), unordered=True)
    if how == "dev_det":
        return lambda k, v: sh.update(dev(gpu, k), dev(gpu, v), deterministic=True)
    if how == "host":
        return lambda k, v: sh.update(k, v)
    assert how == "host_unordered"
    return lambda k, v: sh.update(k, v, unordered=True)


UNTOUCHED_VECTOR = [  # (shape, how it is pushed, GLINT_BIN_FRONT, the profiling id that must count the push)
    ("dense", "dev", None, N.GLINT_K_PUSH_APPLY), ("dups1000", "dev", None, N.GLINT_K_PUSH_SCATTER),
    ("prefix_tail", "dev", None, N.GLINT_K_PUSH_SCATTER), ("uniform5000", "host_unordered", None, N.GLINT_K_PUSH_BINNED),
    ("binned", "dev_unordered", "dedup", N.GLINT_K_PUSH_BINNED), ("binned", "dev_unordered", "hot", N.GLINT_K_PUSH_BINNED),
    ("binned", "dev_unordered", "prep", N.GLINT_K_PUSH_BINNED), ("uniform1000", "host", None, N.GLINT_K_PUSH_ORDERED),
    ("uniform4097", "dev_det", None, N.GLINT_K_PUSH_ORDERED), ("uniform131073", "dev_det", None, N.GLINT_K_PUSH_CHECK)]


def check_untouched(sh, img, untouched, what):
    got = np.asarray(sh.to_numpy()).reshape(-1)
    bad = np.flatnonzero((I.bits(got) != I.bits(img.reshape(-1))) & untouched)
    assert bad.size == 0, f"{what}: {bad.size} untouched elements changed, first at {bad[:6]}: {got[bad[:6]]!r}"
    assert (I.bits(got) != I.bits(img.reshape(-1))).any(), "the push applied nothing"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape,how,front,kid", UNTOUCHED_VECTOR)
def test_untouched_vector_elements_keep_their_bits(gpu, monkeypatch, shape, how, front, kid, dtype):
    """A shard full of edge values; the records fall on every fourth key only. Every other element --
    the second half of each touched pair, the lines and slabs a write-back sweeps -- must hold the bits
    it held: no ``d + 0`` (it turns -0.0 into +0.0 and quiets a signalling NaN), no neighbour's sum."""
    if front:
        monkeypatch.setenv("GLINT_BIN_FRONT", front)
    monkeypatch.delenv("GLINT_BINNED", raising=False)
    N.reload_env()
    keys, vals, img, untouched = I.untouched_case(shape, dtype)
    with profiled(PartialVector(RangePartition(1, START, START + img.shape[0]), dtype, gpu)) as sh:
        I.write_image(sh, gpu, img, 1)
        _push_fn(sh, gpu, how)(keys + START, vals)
        assert launches(sh, kid) == 1
        check_untouched(sh, img, untouched, f"{shape}/{how}/{front}/{dtype}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("front", ["dedup", "hot", "prep"])
@pytest.mark.parametrize("shape", ["binned_mat3", "binned_mat64"])
def test_untouched_matrix_cells_keep_their_bits(gpu, monkeypatch, shape, front, dtype):
    monkeypatch.setenv("GLINT_BIN_FRONT", front)
    monkeypatch.delenv("GLINT_BINNED", raising=False)
    N.reload_env()
    cols = I.UNTOUCHED_SHAPES[shape][4]
    keys, vals, img, untouched = I.untouched_case(shape, dtype)
    img = img.reshape(-1, cols)
    with profiled(PartialMatrix(RangePartition(1, START, START + img.shape[0]), cols, dtype, gpu)) as sh:
        I.write_image(sh, gpu, img, 1)
        sh.update(dev(gpu, keys // cols + START), dev(gpu, (keys % cols).astype(np.int32)), dev(gpu, vals), unordered=True)
        assert launches(sh, N.GLINT_K_PUSH_BINNED) == 1
        check_untouched(sh, img, untouched, f"{shape}/{front}/{dtype}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", ["rows3", "rows64"])
@pytest.mark.parametrize("path", ["host", "dev", "dev_det"])
def test_untouched_rows_keep_their_bits(gpu, path, shape, dtype):
    keys, vals, img, untouched = I.untouched_case(shape, dtype)
    with profiled(PartialMatrix(RangePartition(1, START, START + img.shape[0]), img.shape[1], dtype, gpu)) as sh:
        I.write_image(sh, gpu, img, 1)
        if path == "host":
            sh.updateRows(keys + START, vals)
        else:
            sh.updateRows(dev(gpu, keys + START), dev(gpu, vals), deterministic=path == "dev_det")
        assert launches(sh, N.GLINT_K_PUSH_ROWS) == 1
        check_untouched(sh, img, untouched, f"{shape}/{path}/{dtype}")


@pytest.mark.parametrize("dtype", DT)
def test_untouched_elements_of_a_set_push_keep_their_bits(gpu, dtype):
    import torch
    keys, vals, img, untouched = I.untouched_case("uniform30000", dtype)
    size = img.shape[0]
    ranges = [(6000, size), (0, 2500), (2500, 6000)]
    shards = [PartialVector(RangePartition(i, START + a, START + b), dtype, gpu) for i, (a, b) in enumerate(ranges)]
    d = torch.device("cuda", gpu)
    gate = torch.full((1,), 7, dtype=torch.int64, device=d)
    hs = (C.c_void_p * 3)(*[s.handle for s in shards])
    st = torch.cuda.current_stream(d).cuda_stream
    try:
        for sh, (a, b) in zip(shards, ranges):
            I.write_image(sh, gpu, img[a:b], 1)
        kt, vt = dev(gpu, keys + START), dev(gpu, vals)
        assert N.load().glint_vec_push_dev_shards(hs, 3, kt.data_ptr(), vt.data_ptr(), kt.numel(), gate.data_ptr(),
                                                  st) == N.GLINT_OK
        shards[0].sync(st)
        assert int(gate.item()) == 0
        got = np.empty(size, I.NPD[dtype])
        for sh, (a, b) in zip(shards, ranges):
            got[a:b] = sh.to_numpy()
        bad = np.flatnonzero((I.bits(got) != I.bits(img[:, 0])) & untouched)
        assert bad.size == 0, f"{bad.size} untouched elements changed, first at {bad[:6]}: {got[bad[:6]]!r}"
    finally:
        for sh in shards:
            sh.destroy()


# ---- pulls ----------------------------------------------------------------------------------------------
ROWS = 4099  # rows (vector: elements) of the pulled shards


def pull_keys(n, rows):
    """n local rows: the image's first rows (its edge values), then random ones with repeats."""
    rng = I.rng_for("pull", n, rows)
    return np.concatenate([np.arange(min(n, 15)), rng.integers(0, rows, max(0, n - 15))]).astype(np.int64)


def same_bits(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    assert np.array_equal(I.bits(got), I.bits(want)), what


@pytest.mark.parametrize("n", [1, 4096, 4097])
@pytest.mark.parametrize("dtype", DT)
def test_vector_pulls_move_the_bits(gpu, dtype, n):
    """Every vector pull answers with the stored bits: -0.0, NaN payloads and signs (a signalling NaN
    too), infinities, subnormals. 4096 records is the ring's bound (GLINT_ZERO_COPY_MAX): 4097 takes
    the staged gather."""
    img = I.edge_image(dtype, ROWS, 1)
    keys = pull_keys(n, ROWS)
    want = img[keys, 0]
    with PartialVector(RangePartition(1, START, START + ROWS), dtype, gpu) as sh:
        I.write_image(sh, gpu, img, 1)
        same_bits(sh.get(keys + START), want, "get, host arrays")
        same_bits(sh.get(dev(gpu, keys + START)).cpu().numpy(), want, "get, device tensors")
        t, out = sh.pull_async(keys + START)
        sh.wait(t)
        same_bits(out, want, "pull_async")
        resp = O.decode_response(sh.pull_wire(O.encode_pull_vector(keys + START)))
        assert resp["code"] == O.CODE[dtype]
        same_bits(resp["values"], want, "pull_wire")
        same_bits(sh.to_numpy(), img[:, 0], "to_numpy")


@pytest.mark.parametrize("n", [1, 4096, 4097])
@pytest.mark.parametrize("cols", [3, 64])
@pytest.mark.parametrize("dtype", DT)
def test_matrix_pulls_move_the_bits(gpu, dtype, cols, n):
    """Element pulls, row pulls (3 columns: scalar copies; 64: 16-byte ones) and their ring forms; the
    pitch padding holds a non-zero value that no answer may show."""
    img = I.edge_image(dtype, ROWS, cols)
    rows = pull_keys(n, ROWS)
    cl = I.rng_for("pull/cols", n, cols).integers(0, cols, n).astype(np.int32)
    cl[:min(n, 15)] = np.arange(min(n, 15)) % cols
    with PartialMatrix(RangePartition(1, START, START + ROWS), cols, dtype, gpu) as sh:
        I.write_image(sh, gpu, img, 1)
        same_bits(sh.get(rows + START, cl), img[rows, cl], "get, host arrays")
        same_bits(sh.get(dev(gpu, rows + START), dev(gpu, cl)).cpu().numpy(), img[rows, cl], "get, device tensors")
        t, out = sh.pull_async(rows + START, cl)
        sh.wait(t)
        same_bits(out, img[rows, cl], "pull_async")
        resp = O.decode_response(sh.pull_wire(O.encode_pull_matrix(rows + START, cl)))
        same_bits(resp["values"], img[rows, cl], "pull_wire")
        same_bits(sh.getRows(rows + START), img[rows], "getRows, host arrays")
        same_bits(sh.getRows(dev(gpu, rows + START)).cpu().numpy(), img[rows], "getRows, device tensors")
        t, out = sh.pull_async(rows + START, rows=True)
        sh.wait(t)
        same_bits(out, img[rows], "pull_async(rows=True)")
        resp = O.decode_response(sh.pull_wire(O.encode_pull_matrix_rows(rows + START)))
        same_bits(resp["values"], img[rows].reshape(-1), "pull_wire, rows")
        same_bits(sh.to_numpy(), img, "to_numpy")
