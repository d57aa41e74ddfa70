"""Narrow-format row transport, the parts that need no GPU: the ABI's symbols, NULL-shard checks and the
supported pairs, the contract header (through tests/c/wire_probe.cpp) against numpy bit for bit, the numpy
restatements glint_amd.to_bfloat16 / from_bfloat16, and BigMatrix.pullRowsAs / pushRowsAs' bucketing over fake
shards."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartitioner, IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix
from axpy_cases import fold_rows
from wire_cases import (NPV, NPW, PAIRS, assert_wire_bits, bf16_narrow, bf16_widen, bits, from_bits, narrow_set,
                        ref_narrow, ref_widen, widen_all)

ROOT = Path(__file__).resolve().parent.parent
SFX = {"float": "f32", "double": "f64", "float16": "f16", "bfloat16": "bf16", "float32": "f32"}


# ---- ABI -------------------------------------------------------------------------------------------------
def test_abi():
    lib = N.load()
    for name in ("glint_mat_pull_rows_as", "glint_mat_push_rows_as", "glint_mat_pull_rows_as_dev",
                 "glint_mat_push_rows_as_dev", "glint_wire_supported"):
        assert callable(getattr(lib, name)) and name in N.SIGNATURES
    assert lib.glint_version() > 1200
    assert N.GLINT_K_COUNT == 13  # no new kernel id
    assert (N.GLINT_WIRE_F16, N.GLINT_WIRE_BF16, N.GLINT_WIRE_F32) == (0, 1, 2)
    assert lib.glint_mat_pull_rows_as(None, None, None, 0, N.GLINT_WIRE_F16) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_as(None, None, None, 0, N.GLINT_WIRE_F16, 0) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_as_dev(None, None, None, 0, N.GLINT_WIRE_F16, None) == N.GLINT_EINVAL
    assert lib.glint_mat_push_rows_as_dev(None, None, None, 0, N.GLINT_WIRE_F16, 0, None) == N.GLINT_EINVAL


def test_supported_pairs():
    lib = N.load()
    yes = {(N.GLINT_F32, N.GLINT_WIRE_F16), (N.GLINT_F32, N.GLINT_WIRE_BF16), (N.GLINT_F64, N.GLINT_WIRE_F32)}
    for dt in (N.GLINT_I32, N.GLINT_I64, N.GLINT_F32, N.GLINT_F64):
        for w in (N.GLINT_WIRE_F16, N.GLINT_WIRE_BF16, N.GLINT_WIRE_F32):
            assert lib.glint_wire_supported(dt, w) == int((dt, w) in yes), (dt, w)
    for dt, w in ((-1, 0), (4, 0), (N.GLINT_F32, -1), (N.GLINT_F32, 3), (N.GLINT_F64, 7)):  # never fails
        assert lib.glint_wire_supported(dt, w) == 0


def test_methods_are_public():
    for obj, names in ((glint_amd.PartialMatrix, ("getRowsAs", "updateRowsAs")),
                       (glint_amd.BigMatrix, ("pullRowsAs", "pushRowsAs")),
                       (glint_amd, ("to_bfloat16", "from_bfloat16"))):
        for name in names:
            assert callable(getattr(obj, name))


# ---- the contract header against numpy -----------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("_glint_build", ROOT / "glint_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = C.CDLL(str(mod.build_wire_probe()))
    for name in ("wire_narrow_f32_f16", "wire_narrow_f32_bf16", "wire_narrow_f64_f32", "wire_widen_f16_f32",
                 "wire_widen_bf16_f32", "wire_widen_f32_f64"):
        fn = getattr(lib, name)
        fn.argtypes, fn.restype = [C.c_void_p, C.c_int64, C.c_void_p], None
    lib.wire_probe_supported.argtypes = lib.wire_probe_size.argtypes = [C.c_int] * 2
    lib.wire_probe_size.argtypes = [C.c_int]
    return lib


def probe_narrow(probe, x, dtype, wire):
    x = np.ascontiguousarray(x, NPV[dtype])
    out = np.empty(x.shape, NPW[wire])
    getattr(probe, f"wire_narrow_{SFX[dtype]}_{SFX[wire]}")(x.ctypes.data, x.size, out.ctypes.data)
    return out


def probe_widen(probe, w, dtype, wire):
    w = np.ascontiguousarray(w, NPW[wire])
    out = np.empty(w.shape, NPV[dtype])
    getattr(probe, f"wire_widen_{SFX[wire]}_{SFX[dtype]}")(w.ctypes.data, w.size, out.ctypes.data)
    return out


def assert_v_bits(got, exp, what=""):
    nan = np.isnan(exp)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    np.testing.assert_array_equal(np.where(nan, 0, bits(got)), np.where(nan, 0, bits(exp)), err_msg=what)


def test_header_pairs_and_sizes(probe):
    lib = N.load()
    for dt in range(-1, 6):
        for w in range(-1, 5):
            assert probe.wire_probe_supported(dt, w) == lib.glint_wire_supported(dt, w)
    assert [probe.wire_probe_size(w) for w in (-1, 0, 1, 2, 3)] == [0, 2, 2, 4, 0]


@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_header_widening_is_numpys(probe, dtype, wire):
    w = widen_all(wire)
    assert w.size == (6144 if wire == "float32" else 65536)
    got, exp = probe_widen(probe, w, dtype, wire), ref_widen(w, wire)
    assert_v_bits(got, exp, wire)
    fin = ~np.isnan(exp)
    # exact: narrowing the widened value gives the pattern back (NaNs apart)
    back = probe_narrow(probe, got, dtype, wire)
    np.testing.assert_array_equal(bits(back)[fin], bits(w)[fin])


@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_header_narrowing_is_numpys(probe, dtype, wire):
    x = narrow_set(wire)
    assert x.dtype == NPV[dtype] and x.size > (250_000 if wire != "float32" else 60_000)
    exp = ref_narrow(x, wire)
    assert_wire_bits(probe_narrow(probe, x, dtype, wire), exp, wire)
    # what the set is made for: a tie goes to even, its two neighbours go apart, and the top rounds to infinity
    m = (x.size // 2 - 8) // 4  # a, mid, below, above: m values each, then the extras, then the negatives
    a, mid, below, above = (bits(exp[k * m:(k + 1) * m]).astype(np.int64) for k in range(4))
    assert (below == a).all() and (above == a + 1).all()
    assert (mid == a + (a & 1)).all()
    assert np.isinf(ref_widen(exp[m:2 * m][-1:], wire)).all() and not np.isinf(ref_widen(exp[:m][-1:], wire)).any()
    assert mid[0] == 0 and above[0] == 1  # half the smallest subnormal: zero; just above it: the subnormal is kept


# ---- to_bfloat16 / from_bfloat16 -------------------------------------------------------------------------------
def test_bfloat16_known_answers():
    f = lambda *u: from_bits(np.array(u, np.uint32), np.float32)  # noqa: E731
    t = glint_amd.to_bfloat16
    assert t(np.array([1.0], np.float32)).tolist() == [0x3F80]
    assert t(f(0x3F808000, 0x3F818000)).tolist() == [0x3F80, 0x3F82]      # ties: to even, down and up
    assert t(f(0x3F808001, 0x3F817FFF)).tolist() == [0x3F81, 0x3F81]      # just past / just short of a tie
    assert t(f(0x7F7FFFFF, 0xFF7FFFFF)).tolist() == [0x7F80, 0xFF80]      # the largest float rounds to infinity
    assert t(f(0x7F800000, 0xFF800000, 0x80000000, 0)).tolist() == [0x7F80, 0xFF80, 0x8000, 0]
    assert t(f(0x00000001, 0x00008000, 0x00008001, 0x00018000)).tolist() == [0, 0, 1, 2]  # subnormals, the tie to zero
    nan = t(f(0x7FC00001, 0xFFFFFFFF, 0x7F800001))
    assert ((nan & 0x7F80) == 0x7F80).all() and ((nan & 0x7F) != 0).all()
    assert t(np.zeros((3, 5), np.float32)).shape == (3, 5) and t(np.zeros(2, np.float32)).dtype == np.uint16
    g = glint_amd.from_bfloat16
    assert bits(g(np.array([0x3F80, 0x8000, 0x0001, 0x7F80], np.uint16))).tolist() == [0x3F800000, 0x80000000, 0x10000,
                                                                                      0x7F800000]
    assert g(np.zeros(4, np.uint16)).dtype == np.float32
    for bad in (np.zeros(2, np.float64), np.zeros(2, np.float16)):
        with pytest.raises(TypeError):
            t(bad)
    with pytest.raises(TypeError):
        g(np.zeros(2, np.int16))


def test_bfloat16_equals_the_reference_everywhere():
    x = narrow_set("bfloat16")
    assert_wire_bits(glint_amd.to_bfloat16(x), bf16_narrow(x), "bfloat16")
    w = widen_all("bfloat16")
    got, exp = glint_amd.from_bfloat16(w), bf16_widen(w)
    np.testing.assert_array_equal(bits(got), bits(exp))  # the pattern is the float's upper half, NaNs included
    fin = ~np.isnan(exp)
    np.testing.assert_array_equal(glint_amd.to_bfloat16(got)[fin], w[fin])  # a round trip


# ---- BigMatrix.pullRowsAs / pushRowsAs over fake shards ----------------------------------------------------------
class FakeShard:
    """A slice of a numpy table behind PartialMatrix.getRowsAs / updateRowsAs, by the references; records its
    calls."""

    def __init__(self, table, part, log, name):
        self.table, self.part, self.log, self.name = table, part, log, name
        self.np_dtype = table.dtype.type

    def _local(self, rows):
        loc = np.array([self.part.globalToLocal(int(r)) for r in rows], np.int64)
        assert ((loc >= 0) & (loc < self.table.shape[0])).all()
        return loc

    def getRowsAs(self, rows, wire, out=None, sync=True):
        self.log.append((self.name, "pull", np.array(rows), wire))
        return ref_narrow(self.table[self._local(rows)], wire)

    def updateRowsAs(self, rows, values, wire, deterministic=False, sync=True, unordered=False):
        self.log.append((self.name, "push", np.array(rows), wire, np.array(values), deterministic))
        self.table[:] = fold_rows(self.table, self._local(rows), ref_widen(np.asarray(values), wire))
        return True


def _model(partitioner, nrows, log, cols=7, dtype=np.float32, seed=1):
    rng = np.random.default_rng(seed)
    full = (rng.standard_normal((nrows, cols)) * 10.0 ** rng.integers(-3, 4, (nrows, cols))).astype(dtype)
    shards, keys_of = [], []
    for i, p in enumerate(partitioner.all()):
        keys = np.array([k for k in range(nrows) if p.contains(k)], np.int64)
        assert all(p.globalToLocal(int(k)) == j for j, k in enumerate(keys))
        shards.append(FakeShard(np.array(full[keys]), p, log, i))
        keys_of.append(keys)
    return full, shards, keys_of, BigMatrix(partitioner, shards, nrows, cols)


def _whole(shards, keys_of, nrows):
    out = np.empty((nrows, shards[0].table.shape[1]), shards[0].table.dtype)
    for s, keys in zip(shards, keys_of):
        out[keys] = s.table
    return out


@pytest.mark.parametrize("make", [RangePartitioner.apply, CyclicPartitioner.apply])
@pytest.mark.parametrize("dtype,wire", PAIRS)
def test_big_matrix_buckets_by_partition(make, dtype, wire):
    log = []
    nrows, cols, n = 300, 7, 400
    full, shards, keys_of, M = _model(make(3, nrows), nrows, log, cols, NPV[dtype])
    rng = np.random.default_rng(11)
    rows = rng.integers(0, nrows, n).astype(np.int64)
    rows[10:20] = rows[10]  # a repeated row
    own = M.partitioner.partition_indices(rows)
    # pull: the caller's order restored, the bits the shards'
    got = M.pullRowsAs(rows, wire)
    assert got.dtype == NPW[wire] and got.shape == (n, cols)
    assert_wire_bits(got, ref_narrow(full[rows], wire), wire)
    assert [(c[0], c[1], c[3]) for c in log] == [(p, "pull", wire) for p in range(3)]
    for c in log:
        np.testing.assert_array_equal(c[2], rows[own == c[0]])  # its own rows only, in the caller's order
    # push: every record reaches its partition, in the caller's order, in the wire type
    log.clear()
    wide = (rng.standard_normal((n, cols)) * 10.0 ** rng.integers(-3, 4, (n, cols))).astype(NPV[dtype])
    vals = ref_narrow(wide, wire)
    assert M.pushRowsAs(rows, vals, wire, deterministic=True)
    want = fold_rows(full, rows, ref_widen(vals, wire))
    np.testing.assert_array_equal(bits(_whole(shards, keys_of, nrows)), bits(want))
    assert [(c[0], c[1], c[3], c[5]) for c in log] == [(p, "push", wire, True) for p in range(3)]
    for c in log:
        np.testing.assert_array_equal(c[2], rows[own == c[0]])
        assert c[4].dtype == NPW[wire]
        np.testing.assert_array_equal(bits(c[4]), bits(vals[own == c[0]]))
    # flat values are taken too
    log.clear()
    assert M.pushRowsAs(rows[:5], vals[:5].reshape(-1), wire)
    assert sum(c[2].size for c in log) == 5


def test_big_matrix_skips_empty_partitions_and_empty_calls():
    log = []
    _, _, _, M = _model(RangePartitioner.apply(3, 300), 300, log)
    rows = np.array([250, 3, 299, 0], np.int64)  # nothing from partition 1
    M.pushRowsAs(rows, np.ones((4, 7), np.float16), "float16")
    assert [c[0] for c in log] == [0, 2]
    np.testing.assert_array_equal(log[0][2], [3, 0])
    np.testing.assert_array_equal(log[1][2], [250, 299])
    log.clear()
    assert M.pullRowsAs(rows, "bfloat16").shape == (4, 7)
    assert [c[0] for c in log] == [0, 2]
    log.clear()
    assert M.pushRowsAs(np.zeros(0, np.int64), np.zeros((0, 7), np.float16), "float16")
    assert M.pullRowsAs(np.zeros(0, np.int64), "float16").shape == (0, 7)
    assert not log


def test_big_matrix_rejects_before_any_shard_is_called():
    log = []
    _, _, _, M = _model(RangePartitioner.apply(3, 300), 300, log)
    vals = np.ones((3, 7), np.float16)
    for bad_rows in (np.array([3, 300, 7], np.int64), np.array([-1, 3, 7], np.int64)):
        with pytest.raises(IndexOutOfBoundsException):
            M.pushRowsAs(bad_rows, vals, "float16")
        with pytest.raises(IndexOutOfBoundsException):
            M.pullRowsAs(bad_rows, "float16")
    rows = np.array([3, 299, 7], np.int64)
    for v, wire in ((vals, "bfloat16"), (vals.astype(np.float32), "float16"), (vals.astype(np.uint16), "float16"),
                    (vals, "float32"), (vals.astype(np.float64), "float32"), (vals.tolist(), "float16")):
        with pytest.raises(ValueError):
            M.pushRowsAs(rows, v, wire)  # the values' dtype does not match the wire type
    with pytest.raises(ValueError):
        M.pushRowsAs(rows, np.ones((3, 8), np.float16), "float16")  # other cols
    with pytest.raises(ValueError):
        M.pushRowsAs(rows, np.ones((2, 7), np.float16), "float16")  # one row short
    for wire in ("half", "float64", None, 0):
        with pytest.raises(ValueError):
            M.pushRowsAs(rows, vals, wire)
        with pytest.raises(ValueError):
            M.pullRowsAs(rows, wire)
    assert not log
