"""The Python layer's argument handling, pinned without a GPU or the native library: shards built by hand
over a stub ``lib`` that records every ``glint_*`` call. For each public method's host-array path the recorded
symbol, every count, flag and scalar and the pointers' positions (which array stands where, which are NULL)
are literals here; every reject that happens before a C call is pinned by class and full message, and by
which fault is reported when there are two. The device-tensor branches need torch tensors on a GPU and are
covered by the ``gpu`` suite. Last, the client's bucket iterator over a partitioner."""
import ctypes as C
import re

import numpy as np
import pytest

from glint_amd import client as CL
from glint_amd import shard as S
from glint_amd.errors import ArrayIndexOutOfBoundsException, GlintDeviceError, IndexOutOfBoundsException
from glint_amd.partitioning import CyclicPartition, RangePartition, RangePartitioner
from glint_amd.shard import PartialMatrix, PartialVector

F32 = np.float32
P = object()  # in an expected call: a pointer that is not NULL, whatever it points to


class StubLib:
    """Every ``glint_*`` attribute is a function that records (symbol, args) and returns ``rc``; with ``bad``
    it also stores that record index through its last argument, as glint_shard_sync / _wait do."""

    def __init__(self, rc=0, bad=None):
        self.calls, self.rc, self.bad = [], rc, bad

    def __getattr__(self, name):
        if not name.startswith("glint_"):
            raise AttributeError(name)

        def call(*args):
            self.calls.append((name, args))
            if self.bad is not None:
                args[-1]._obj.value = self.bad
            return self.rc
        return call


def _shard(cls, cols, partition=None, code=2, npd=F32):
    """A shard of 8 rows (keys 16..23 by default) put together as _Shard.view does, over a StubLib."""
    sh = cls.__new__(cls)
    sh.lib, sh._h = StubLib(), C.c_void_p(0x1000 + cols)
    sh.code, sh.np_dtype, sh.device = code, npd, 0
    sh.partition, sh.size, sh.cols = partition or RangePartition(1, 16, 24), 8, cols
    if cols:
        sh.rows = 8
    return sh


def matrix(cols=4, **kw):
    return _shard(PartialMatrix, cols, **kw)


def vector(**kw):
    return _shard(PartialVector, 0, **kw)


def called(sh, symbol, *want):
    """The one C call ``sh`` made since the last look. ``want`` per argument: None -- NULL; P -- any other
    pointer; an array -- that array's own buffer; a shard -- its handle; else a count, flag or scalar of that
    very type and value."""
    (name, args), = sh.lib.calls
    sh.lib.calls.clear()
    assert name == symbol
    assert len(args) == len(want), args
    for i, (a, w) in enumerate(zip(args, want)):
        if w is None:
            assert a is None, (i, a)
        elif w is P:
            assert a is not None and a != 0, (i, a)
        elif isinstance(w, np.ndarray):
            assert a == w.ctypes.data, (i, a)
        elif isinstance(w, S._Shard):
            assert a is w._h, (i, a)
        else:
            assert type(a) is type(w) and a == w, (i, a, w)


def rejects(sh, cls, message, call, *a, **kw):
    """``call`` raises exactly ``cls`` with exactly ``message``, and before any C call."""
    with pytest.raises(cls, match="^" + re.escape(message) + "$") as e:
        call(*a, **kw)
    assert e.type is cls
    assert not sh.lib.calls


class Dev:
    """What _is_torch_cuda takes for a device tensor."""
    __module__ = "torch.standin"
    is_cuda = True


ROWS = np.array([17, 20, 17], np.int64)      # 3 records, one row twice
COLS = np.array([0, 3, 1], np.int32)
VALS = np.arange(3, dtype=F32)
GRADS = np.arange(12, dtype=F32).reshape(3, 4)
OFFS = np.array([0, 3, 3], np.int64)         # 2 groups, the second empty
GVALS = np.arange(8, dtype=F32).reshape(2, 4)
WEIGHTS = np.array([0.5, 2.0, -1.0], F32)
X1 = np.arange(4, dtype=F32)                 # q = 1
X2 = np.arange(8, dtype=F32).reshape(2, 4)   # q = 2
NOROWS = np.zeros(0, np.int64)


def test_stand_in_is_a_device_tensor_to_the_shard():
    assert S._is_torch_cuda(Dev()) and not S._is_torch_cuda(ROWS) and not S._is_torch_cuda(None)


# ---- host-path call pins ------------------------------------------------------------------------------------

def test_vector_update_and_get():
    v = vector()
    assert v.update(ROWS, VALS) is True
    called(v, "glint_vec_push", v, ROWS, VALS, 3, 0)
    v.update(ROWS, VALS, deterministic=True)
    called(v, "glint_vec_push", v, ROWS, VALS, 3, 1)
    v.update(ROWS, VALS, unordered=True, validate=True)
    called(v, "glint_vec_push", v, ROWS, VALS, 3, 6)
    res = v.get(ROWS)
    assert res.dtype == F32 and res.shape == (3,)
    called(v, "glint_vec_pull", v, ROWS, res, 3)
    out = np.empty(3, F32)
    assert v.get(ROWS, out=out) is out
    called(v, "glint_vec_pull", v, ROWS, out, 3)


def test_matrix_update_get_and_get_rows():
    m = matrix()
    assert m.update(ROWS, COLS, VALS, deterministic=True, unordered=True) is True
    called(m, "glint_mat_push", m, ROWS, COLS, VALS, 3, 3)
    m.update(ROWS, COLS, VALS, validate=True)
    called(m, "glint_mat_push", m, ROWS, COLS, VALS, 3, 4)
    res = m.get(ROWS, COLS)
    assert res.dtype == F32 and res.shape == (3,)
    called(m, "glint_mat_pull", m, ROWS, COLS, res, 3)
    res = m.getRows(ROWS)
    assert res.dtype == F32 and res.shape == (3, 4)
    called(m, "glint_mat_pull_rows", m, ROWS, res, 3)
    out = np.empty((3, 4), F32)
    assert m.getRows(ROWS, out=out) is out
    called(m, "glint_mat_pull_rows", m, ROWS, out, 3)


def test_update_rows_and_its_wire_variant():
    m = matrix()
    assert m.updateRows(ROWS, GRADS) is True
    called(m, "glint_mat_push_rows", m, ROWS, GRADS, 3, 0)
    m.updateRows(ROWS, GRADS.reshape(-1), deterministic=True)  # flat values
    called(m, "glint_mat_push_rows", m, ROWS, GRADS, 3, 1)
    m.updateRows(NOROWS, np.zeros((0, 4), F32), unordered=True)
    called(m, "glint_mat_push_rows", m, P, P, 0, 2)
    for wire, code, npd in (("float16", 0, np.float16), ("bfloat16", 1, np.uint16), ("float32", 2, np.float32)):
        v = np.arange(12).astype(npd).reshape(3, 4)
        assert m.updateRowsAs(ROWS, v, wire) is True
        called(m, "glint_mat_push_rows_as", m, ROWS, v, 3, code, 0)
        m.updateRowsAs(ROWS, v.reshape(-1), wire, deterministic=True, unordered=True)
        called(m, "glint_mat_push_rows_as", m, ROWS, v, 3, code, 3)


def test_get_rows_as():
    m = matrix()
    for wire, code, npd in (("float16", 0, np.float16), ("bfloat16", 1, np.uint16), ("float32", 2, np.float32)):
        res = m.getRowsAs(ROWS, wire)
        assert res.dtype == npd and res.shape == (3, 4)
        called(m, "glint_mat_pull_rows_as", m, ROWS, res, 3, code)
        out = np.empty((3, 4), npd)
        assert m.getRowsAs(ROWS, wire, out=out) is out
        called(m, "glint_mat_pull_rows_as", m, ROWS, out, 3, code)


def test_update_rows_axpy():
    m = matrix()
    coef = np.array([1, 2, 3], F32)
    assert m.updateRowsAxpy(ROWS, coef, X1) is True  # q == 1 takes (n,) coefficients
    called(m, "glint_mat_push_rows_axpy", m, ROWS, 3, coef, X1, 1, 0)
    m.updateRowsAxpy(ROWS, coef.reshape(3, 1), X1.reshape(1, 4), deterministic=True)
    called(m, "glint_mat_push_rows_axpy", m, ROWS, 3, coef, X1, 1, 1)
    coef2 = np.arange(6, dtype=F32).reshape(3, 2)
    m.updateRowsAxpy(ROWS, coef2, X2, unordered=True)
    called(m, "glint_mat_push_rows_axpy", m, ROWS, 3, coef2, X2, 2, 2)


def test_update_rows_grouped():
    m = matrix()
    assert m.updateRowsGrouped(ROWS, OFFS, GVALS) is True
    called(m, "glint_mat_push_rows_grouped", m, ROWS, 3, OFFS, 2, GVALS, None, 0)
    m.updateRowsGrouped(ROWS, OFFS, GVALS.reshape(-1), WEIGHTS, deterministic=True)
    called(m, "glint_mat_push_rows_grouped", m, ROWS, 3, OFFS, 2, GVALS, WEIGHTS, 1)
    none = np.zeros(1, np.int64)  # g == 0: no value row, NULL
    m.updateRowsGrouped(NOROWS, none, np.zeros((0, 4), F32), unordered=True)
    called(m, "glint_mat_push_rows_grouped", m, P, 0, none, 0, None, None, 2)


def test_optimizer_pushes():
    m, st, st2, sv = matrix(), matrix(), matrix(8), vector()
    assert m.updateRowsAdagrad(st, ROWS, GRADS, 0.5) is True
    called(m, "glint_mat_push_rows_adagrad", m, st, ROWS, GRADS, 3, 0.5, 1e-10)
    m.updateRowsAdagrad(st, ROWS, GRADS.reshape(-1), 1, eps=0)  # scalars become floats
    called(m, "glint_mat_push_rows_adagrad", m, st, ROWS, GRADS, 3, 1.0, 0.0)
    assert m.updateRowsAdagradRowwise(sv, ROWS, GRADS, 0.25) is True
    called(m, "glint_mat_push_rows_adagrad_rowwise", m, sv, ROWS, GRADS, 3, 0.25, 1e-10)
    m.updateRowsAdagradRowwise(sv, ROWS, GRADS, np.float32(2), 0.125)
    called(m, "glint_mat_push_rows_adagrad_rowwise", m, sv, ROWS, GRADS, 3, 2.0, 0.125)
    assert m.updateRowsAdam(st2, ROWS, GRADS, 0.5, 7) is True
    called(m, "glint_mat_push_rows_adam", m, st2, ROWS, GRADS, 3, 0.5, 0.9, 0.999, 1e-8, 7)
    m.updateRowsAdam(st2, ROWS, GRADS, 1, np.int64(2), beta1=0.5, beta2=0.75, eps=0)
    called(m, "glint_mat_push_rows_adam", m, st2, ROWS, GRADS, 3, 1.0, 0.5, 0.75, 0.0, 2)
    assert m.updateRowsFtrl(st2, ROWS, GRADS, 0.5) is True
    called(m, "glint_mat_push_rows_ftrl", m, st2, ROWS, GRADS, 3, 0.5, 1.0, 0.0, 0.0)
    m.updateRowsFtrl(st2, ROWS, GRADS, 2, beta=3, l1=0.25, l2=0.125)
    called(m, "glint_mat_push_rows_ftrl", m, st2, ROWS, GRADS, 3, 2.0, 3.0, 0.25, 0.125)
    for sh in (st, st2, sv):
        assert not sh.lib.calls  # every call goes through the weights shard's library


def test_get_rows_sparse():
    m = matrix()
    indptr, cols, vals = m.getRowsSparse(ROWS)  # the stub counts no entry: the count-only call is the only one
    called(m, "glint_mat_pull_rows_sparse", m, ROWS, 3, indptr, None, None, 0, P)
    assert (indptr.dtype, indptr.shape) == (np.int64, (4,))
    assert (cols.dtype, cols.shape, vals.dtype, vals.shape) == (np.int32, (0,), F32, (0,))
    indptr, cols, vals = m.getRowsSparse(ROWS, cap=5)
    called(m, "glint_mat_pull_rows_sparse", m, ROWS, 3, indptr, P, P, 5, P)
    assert (cols.dtype, cols.shape, vals.dtype, vals.shape) == (np.int32, (0,), F32, (0,))
    indptr, cols, vals = m.getRowsSparse(ROWS, cap=0)
    called(m, "glint_mat_pull_rows_sparse", m, ROWS, 3, indptr, None, None, 0, P)


def test_get_rows_sum():
    m = matrix()
    res = m.getRowsSum(ROWS, OFFS)
    assert res.dtype == F32 and res.shape == (2, 4)
    called(m, "glint_mat_pull_rows_sum", m, ROWS, 3, OFFS, 2, res)
    out = np.empty((2, 4), F32)
    assert m.getRowsSum(ROWS, OFFS, out, weights=WEIGHTS) is out
    called(m, "glint_mat_pull_rows_wsum", m, ROWS, 3, OFFS, 2, WEIGHTS, out)
    offs = np.zeros(2, np.int64)  # no record: the weights pointer is NULL
    res = m.getRowsSum(NOROWS, offs, weights=np.zeros(0, F32))
    assert res.shape == (1, 4)
    called(m, "glint_mat_pull_rows_wsum", m, P, 0, offs, 1, None, res)


def test_get_rows_group_dot():
    m = matrix()
    res = m.getRowsGroupDot(ROWS, OFFS, GVALS)
    assert res.dtype == F32 and res.shape == (3,)
    called(m, "glint_mat_pull_rows_gdot", m, ROWS, 3, OFFS, 2, GVALS, res)
    out = np.empty(3, F32)
    assert m.getRowsGroupDot(ROWS, OFFS, GVALS.reshape(-1), out=out) is out  # flat x
    called(m, "glint_mat_pull_rows_gdot", m, ROWS, 3, OFFS, 2, GVALS, out)
    none = np.zeros(1, np.int64)  # g == 0: no vector, NULL
    res = m.getRowsGroupDot(NOROWS, none, np.zeros((0, 4), F32))
    assert res.shape == (0,)
    called(m, "glint_mat_pull_rows_gdot", m, P, 0, none, 0, None, P)


def test_get_rows_dot():
    m = matrix()
    res = m.getRowsDot(ROWS)
    assert res.dtype == F32 and res.shape == (3,)
    called(m, "glint_mat_pull_rows_dot", m, ROWS, 3, None, 1, res)
    res = m.getRowsDot(ROWS, X1)
    assert res.shape == (3,)
    called(m, "glint_mat_pull_rows_dot", m, ROWS, 3, X1, 1, res)
    res = m.getRowsDot(ROWS, X1.reshape(1, 4))
    assert res.shape == (3, 1)
    called(m, "glint_mat_pull_rows_dot", m, ROWS, 3, X1, 1, res)
    out = np.empty((3, 2), F32)
    assert m.getRowsDot(ROWS, X2, out=out) is out
    called(m, "glint_mat_pull_rows_dot", m, ROWS, 3, X2, 2, out)


def test_pair_calls():
    m, other = matrix(), matrix(partition=RangePartition(0, 0, 8))
    orows = np.array([0, 7, 3], np.int64)
    res = m.getPairsDot(other, ROWS, orows)
    assert res.dtype == F32 and res.shape == (3,)
    called(m, "glint_mat_pull_pairs_dot", m, other, ROWS, orows, 3, res)
    out = np.empty(3, F32)
    assert m.getPairsDot(m, ROWS, ROWS, out=out) is out  # with itself
    called(m, "glint_mat_pull_pairs_dot", m, m, ROWS, ROWS, 3, out)
    assert m.updatePairsAxpy(other, ROWS, orows, WEIGHTS) is True
    called(m, "glint_mat_push_pairs_axpy", m, other, ROWS, orows, WEIGHTS, 3, 0)
    m.updatePairsAxpy(other, ROWS, orows, WEIGHTS, deterministic=True, unordered=True)
    called(m, "glint_mat_push_pairs_axpy", m, other, ROWS, orows, WEIGHTS, 3, 3)
    assert not other.lib.calls


def test_get_top_k():
    m = matrix()
    rows, vals = m.getTopK(X1, 3)
    assert (rows.dtype, rows.shape, vals.dtype, vals.shape) == (np.int64, (3,), F32, (3,))
    called(m, "glint_mat_pull_topk", m, X1, 1, 3, rows, vals)
    rows, vals = m.getTopK(X2, np.int64(5))  # k becomes an int
    assert (rows.dtype, rows.shape, vals.dtype, vals.shape) == (np.int64, (2, 5), F32, (2, 5))
    called(m, "glint_mat_pull_topk", m, X2, 2, 5, rows, vals)


@pytest.mark.parametrize("make", [vector, matrix])
def test_shard_calls(make):
    sh = make()
    sh.zero()
    called(sh, "glint_shard_zero", sh)
    assert sh.fill(1.5) is True
    called(sh, "glint_shard_fill", sh, None, 0, P)
    sh.fill(1.5, rows=ROWS)
    called(sh, "glint_shard_fill", sh, ROWS, 3, P)
    sh.fill(1.5, rows=NOROWS)  # names nothing: never the NULL that names every row
    called(sh, "glint_shard_fill", sh, P, 0, P)
    assert sh.initUniform(7, -1, 1) is True
    called(sh, "glint_shard_init_uniform", sh, None, 0, 7, -1.0, 1.0)
    sh.initUniform((1 << 64) - 1, 0.5, 0.75, rows=ROWS)
    called(sh, "glint_shard_init_uniform", sh, ROWS, 3, (1 << 64) - 1, 0.5, 0.75)
    sh.initUniform(0, 0.5, 0.75, rows=NOROWS)
    called(sh, "glint_shard_init_uniform", sh, P, 0, 0, 0.5, 0.75)
    assert sh.data_ptr() == 0  # (the stub stores no address)
    called(sh, "glint_shard_data", sh, P)
    sh.sync()
    called(sh, "glint_shard_sync", sh, None, P)
    sh.sync(0x55)
    called(sh, "glint_shard_sync", sh, 0x55, P)
    sh.wait(9)
    called(sh, "glint_shard_wait", sh, 9, P)
    h = sh._h
    sh.destroy()
    assert sh.lib.calls == [("glint_shard_destroy", (h,))]
    sh.destroy()  # once
    assert len(sh.lib.calls) == 1
    sh.lib.calls.clear()
    rejects(sh, ValueError, "shard already destroyed", sh.zero)


def test_to_numpy_names_every_key_of_the_partition():
    for part, keys in ((RangePartition(1, 16, 24), [16, 17, 18, 19, 20, 21, 22, 23]),
                       (CyclicPartition(1, 3, 24), [1, 4, 7, 10, 13, 16, 19, 22])):
        v, m = vector(partition=part), matrix(partition=part)
        v.get = m.getRows = lambda k: k  # what to_numpy pulls
        for got in (v.to_numpy(), m.to_numpy()):
            assert got.dtype == np.int64 and got.tolist() == keys
        assert not v.lib.calls and not m.lib.calls


def test_out_of_range_status_becomes_the_exception():
    for name, args in (("sync", ()), ("wait", (3,))):
        sh = matrix()
        sh.lib = StubLib(rc=1, bad=5)
        with pytest.raises(ArrayIndexOutOfBoundsException, match="^record 5 is outside the partition$") as e:
            getattr(sh, name)(*args)
        assert e.value.record == 5
        assert [c[0] for c in sh.lib.calls] == ["glint_shard_" + name]  # the record came with the status
    with pytest.raises(ArrayIndexOutOfBoundsException, match="^record -1 is outside the partition$") as e:
        S.check(1)
    assert e.value.record == -1
    S.check(0)
    for rc, cls in ((2, GlintDeviceError), (3, ValueError), (4, MemoryError)):
        with pytest.raises(cls) as e:
            S.check(rc)
        assert e.type is cls


# ---- rejects before any C call ------------------------------------------------------------------------------

OPTIMIZERS = [("updateRowsAdagrad", "PartialMatrix", (0.5,)), ("updateRowsAdagradRowwise", "PartialVector", (0.5,)),
              ("updateRowsAdam", "PartialMatrix", (0.5, 1)), ("updateRowsFtrl", "PartialMatrix", (0.5,))]


@pytest.mark.parametrize("method,state_cls,scalars", OPTIMIZERS)
def test_optimizer_push_rejects(method, state_cls, scalars):
    m, ints = matrix(), matrix(code=0, npd=np.int32)
    good = vector() if state_cls == "PartialVector" else matrix(8)
    wrong = matrix() if state_cls == "PartialVector" else vector()
    short = GRADS.reshape(-1)[:11]
    for state in (wrong, None, m.handle):
        rejects(m, TypeError, f"state: expected a {state_cls}", getattr(m, method), state, ROWS, GRADS, *scalars)
    needs = f"{method} needs a Float or Double shard, not int32"
    rejects(ints, TypeError, needs, getattr(ints, method), good, ROWS, GRADS.astype(np.int32), *scalars)
    mixing = "rows and grads: mixing host arrays and device tensors"
    rejects(m, TypeError, mixing, getattr(m, method), good, ROWS, Dev(), *scalars)
    rejects(m, TypeError, mixing, getattr(m, method), good, Dev(), GRADS, *scalars)
    size = "grads: 11 elements, expected 3 rows x 4 columns"
    rejects(m, ValueError, size, getattr(m, method), good, ROWS, short, *scalars)
    rejects(m, ValueError, "grads: 12 elements, expected 2 rows x 4 columns", getattr(m, method), good, ROWS[:2],
            GRADS, *scalars)
    # two faults: the state's class before the shard's type, that before the mixing, that before the size
    rejects(ints, TypeError, f"state: expected a {state_cls}", getattr(ints, method), wrong, ROWS, Dev(), *scalars)
    rejects(ints, TypeError, needs, getattr(ints, method), good, ROWS, Dev(), *scalars)
    assert not good.lib.calls and not wrong.lib.calls


def test_update_and_get_rejects():
    v, m = vector(), matrix()
    rejects(v, ValueError, "keys and values differ in length", v.update, ROWS, VALS[:2])
    rejects(m, ValueError, "rows, cols and values differ in length", m.update, ROWS, COLS, VALS[:2])
    rejects(m, ValueError, "rows, cols and values differ in length", m.update, ROWS, COLS[:2], VALS)
    rejects(m, ValueError, "rows and cols differ in length", m.get, ROWS, COLS[:2])
    rejects(m, ValueError, "values: 11 elements, expected 3 rows x 4 columns", m.updateRows, ROWS,
            GRADS.reshape(-1)[:11])
    rejects(m, ValueError, "values: 12 elements, expected 2 rows x 4 columns", m.updateRows, ROWS[:2], GRADS)


def _bad_outs(shape, npd=F32):
    """Arrays that no host result buffer of ``shape`` and ``npd`` may be."""
    ro = np.empty(shape, npd)
    ro.flags.writeable = False
    wide = np.empty(shape[:-1] + (2 * shape[-1],), npd)
    return [np.empty(shape, np.float64 if npd != np.float64 else F32), np.empty(shape + (1,), npd), ro,
            wide[..., ::2], np.empty(shape, npd).tolist()]


def test_out_rejects():
    v, m = vector(), matrix()
    for out in _bad_outs((3,)):
        message = "out must be a writable C-contiguous float32 array of shape (3,)"
        rejects(v, ValueError, message, v.get, ROWS, out=out)
        rejects(m, ValueError, message, m.get, ROWS, COLS, out=out)
        rejects(m, ValueError, message, m.getRowsDot, ROWS, out=out)
        rejects(m, ValueError, message, m.getRowsGroupDot, ROWS, OFFS, GVALS, out=out)
        rejects(m, ValueError, message, m.getPairsDot, m, ROWS, ROWS, out=out)
    for out in _bad_outs((3, 4)):
        rejects(m, ValueError, "out must be a writable C-contiguous float32 array of shape (3, 4)", m.getRows, ROWS,
                out=out)
    for out in _bad_outs((3, 2)):
        rejects(m, ValueError, "out must be a writable C-contiguous float32 array of shape (3, 2)", m.getRowsDot,
                ROWS, X2, out=out)
    for out in _bad_outs((2, 4)):
        rejects(m, ValueError, "out must be a writable C-contiguous float32 array of shape (2, 4)", m.getRowsSum,
                ROWS, OFFS, out)
    for wire, name, npd in (("float16", "float16", np.float16), ("bfloat16", "uint16", np.uint16),
                            ("float32", "float32", np.float32)):
        for out in _bad_outs((3, 4), npd):
            rejects(m, ValueError, f"out must be a writable C-contiguous {name} array of shape (3, 4)", m.getRowsAs,
                    ROWS, wire, out=out)


def test_wire_rejects():
    m = matrix()
    h = GRADS.astype(np.float16)
    for wire in ("float64", "half", "Float16", 0, None):
        message = f"unsupported wire type {wire!r} ('float16', 'bfloat16' or 'float32')"
        rejects(m, ValueError, message, m.updateRowsAs, ROWS, h, wire)
        rejects(m, ValueError, message, m.getRowsAs, ROWS, wire)
        rejects(m, ValueError, message, m.updateRowsAs, ROWS, GRADS[:2], wire)  # before the dtype and the size
        rejects(m, ValueError, message, m.getRowsAs, ROWS, wire, out=np.empty(3))  # before the out array
    rejects(m, ValueError, "values: dtype float32, expected float16 for wire type 'float16'", m.updateRowsAs, ROWS,
            GRADS, "float16")
    rejects(m, ValueError, "values: dtype float16, expected uint16 for wire type 'bfloat16'", m.updateRowsAs, ROWS,
            h, "bfloat16")
    rejects(m, ValueError, "values: dtype float64, expected float32 for wire type 'float32'", m.updateRowsAs, ROWS,
            GRADS.astype(np.float64), "float32")
    rejects(m, ValueError, "values: dtype float32, expected float16 for wire type 'float16'", m.updateRowsAs, ROWS,
            GRADS[:2], "float16")  # the dtype before the size
    rejects(m, ValueError, "values: dtype int64, expected float16 for wire type 'float16'", m.updateRowsAs, ROWS,
            list(range(12)), "float16")  # nothing is converted
    rejects(m, ValueError, "values: 8 elements, expected 3 rows x 4 columns", m.updateRowsAs, ROWS, h[:2], "float16")
    rejects(m, TypeError, "values: a device tensor with host rows (mixing host arrays and device tensors)",
            m.updateRowsAs, ROWS, Dev(), "float16")


def test_axpy_rejects():
    m = matrix()
    coef = np.ones(3, F32)
    xmsg = "x: shape {}, expected (4,) or (q, 4) with 1 <= q <= 64"
    for x in (np.ones(3, F32), np.ones((2, 3), F32), np.ones((0, 4), F32), np.ones((65, 4), F32),
              np.ones((1, 1, 4), F32)):
        rejects(m, ValueError, xmsg.format(x.shape), m.updateRowsAxpy, ROWS, coef, x)
    rejects(m, ValueError, "coef: shape (2,), expected (3, 1) or (3,)", m.updateRowsAxpy, ROWS, coef[:2], X1)
    rejects(m, ValueError, "coef: shape (3, 2), expected (3, 1) or (3,)", m.updateRowsAxpy, ROWS, np.ones((3, 2), F32),
            X1)
    rejects(m, ValueError, "coef: shape (3,), expected (3, 2)", m.updateRowsAxpy, ROWS, coef, X2)
    rejects(m, ValueError, "coef: shape (2, 3), expected (3, 2)", m.updateRowsAxpy, ROWS, np.ones((2, 3), F32), X2)
    rejects(m, ValueError, xmsg.format((3,)), m.updateRowsAxpy, ROWS, coef[:2], np.ones(3, F32))  # x before coef


def test_grouped_push_rejects():
    m = matrix()
    for name, args in (("offsets", (Dev(), GVALS)), ("values", (OFFS, Dev())), ("weights", (OFFS, GVALS, Dev()))):
        rejects(m, TypeError, f"rows and {name}: mixing host arrays and device tensors", m.updateRowsGrouped, ROWS,
                *args)
    rejects(m, TypeError, "rows and offsets: mixing host arrays and device tensors", m.updateRowsGrouped, Dev(),
            OFFS, Dev())
    rejects(m, TypeError, "rows and offsets: mixing host arrays and device tensors", m.updateRowsGrouped, ROWS,
            Dev(), Dev(), Dev())  # the first such argument
    none = np.zeros(0, np.int64)
    rejects(m, ValueError, "offsets needs g + 1 entries", m.updateRowsGrouped, ROWS, none, GVALS)
    rejects(m, ValueError, "offsets needs g + 1 entries", m.updateRowsGrouped, ROWS, none, GVALS[:1], WEIGHTS[:2])
    rejects(m, ValueError, "values: 7 elements, expected 2 groups x 4 columns", m.updateRowsGrouped, ROWS, OFFS,
            GVALS.reshape(-1)[:7])
    rejects(m, ValueError, "values: 8 elements, expected 0 groups x 4 columns", m.updateRowsGrouped, ROWS, OFFS[:1],
            GVALS)
    rejects(m, ValueError, "weights: 2 values, expected 3", m.updateRowsGrouped, ROWS, OFFS, GVALS, WEIGHTS[:2])
    rejects(m, ValueError, "values: 4 elements, expected 2 groups x 4 columns", m.updateRowsGrouped, ROWS, OFFS,
            GVALS[:1], WEIGHTS[:2])  # the values before the weights


def test_rows_sum_rejects():
    m = matrix()
    mixing = "rows, offsets and weights: mixing host arrays and device tensors"
    rejects(m, TypeError, mixing, m.getRowsSum, ROWS, Dev())
    rejects(m, TypeError, mixing, m.getRowsSum, ROWS, OFFS, weights=Dev())
    none = np.zeros(0, np.int64)
    rejects(m, ValueError, "offsets needs g + 1 entries", m.getRowsSum, ROWS, none)
    rejects(m, ValueError, "offsets needs g + 1 entries", m.getRowsSum, ROWS, none, weights=WEIGHTS.astype(np.float64))
    rejects(m, TypeError, "weights: expected float32, not float64", m.getRowsSum, ROWS, OFFS,
            weights=WEIGHTS.astype(np.float64))
    rejects(m, TypeError, "weights: expected float32, not int64", m.getRowsSum, ROWS, OFFS,
            weights=np.ones(2, np.int64))  # the dtype before the size
    rejects(m, ValueError, "weights: 2 values, expected 3", m.getRowsSum, ROWS, OFFS, weights=WEIGHTS[:2])
    rejects(m, ValueError, "weights: 2 values, expected 3", m.getRowsSum, ROWS, OFFS, np.empty(3),
            weights=WEIGHTS[:2])  # the weights before the out array
    rejects(m, ValueError, "weights: 4 values, expected 3", m.getRowsSum, ROWS, OFFS, weights=[1.0, 2.0, 3.0, 4.0])


def test_group_dot_rejects():
    m = matrix()
    mixing = "rows, offsets and x: mixing host arrays and device tensors"
    rejects(m, TypeError, mixing, m.getRowsGroupDot, ROWS, Dev(), GVALS)
    rejects(m, TypeError, mixing, m.getRowsGroupDot, ROWS, OFFS, Dev())
    none = np.zeros(0, np.int64)
    rejects(m, ValueError, "offsets needs g + 1 entries", m.getRowsGroupDot, ROWS, none, GVALS)
    rejects(m, ValueError, "offsets needs g + 1 entries", m.getRowsGroupDot, ROWS, none, GVALS.astype(np.float64))
    rejects(m, TypeError, "x: expected float32, not float64", m.getRowsGroupDot, ROWS, OFFS, GVALS.astype(np.float64))
    rejects(m, TypeError, "x: expected float32, not float64", m.getRowsGroupDot, ROWS, OFFS,
            np.ones((2, 3)))  # the dtype before the shape
    for x in (np.ones((2, 3), F32), np.ones(7, F32), np.ones((1, 4), F32), np.ones((4, 2), F32), np.ones((1, 8), F32)):
        rejects(m, ValueError, f"x: shape {x.shape}, expected (2, 4) or (8,)", m.getRowsGroupDot, ROWS, OFFS, x)
    rejects(m, ValueError, "x: shape (2, 3), expected (2, 4) or (8,)", m.getRowsGroupDot, ROWS, OFFS,
            np.ones((2, 3), F32), out=np.empty(2))  # x before the out array


def test_dot_and_top_k_rejects():
    m = matrix()
    dmsg = "x: shape {}, expected (4,) or (q, 4) with 1 <= q <= 1024"
    tmsg = "x: shape {}, expected (4,) or (q, 4) with 1 <= q <= 64"
    for x in (np.ones(3, F32), np.ones((2, 3), F32), np.ones((0, 4), F32), np.ones((1, 1, 4), F32)):
        rejects(m, ValueError, dmsg.format(x.shape), m.getRowsDot, ROWS, x)
        rejects(m, ValueError, tmsg.format(x.shape), m.getTopK, x, 3)
    rejects(m, ValueError, dmsg.format((1025, 4)), m.getRowsDot, ROWS, np.ones((1025, 4), F32))
    rejects(m, ValueError, tmsg.format((65, 4)), m.getTopK, np.ones((65, 4), F32), 3)
    rejects(m, ValueError, dmsg.format((3,)), m.getRowsDot, ROWS, np.ones(3, F32), out=np.empty(2))  # x before out
    rejects(m, ValueError, "k: 0, expected 1 <= k <= 1024", m.getTopK, X1, 0)
    rejects(m, ValueError, "k: -3, expected 1 <= k <= 1024", m.getTopK, X1, -3)
    rejects(m, ValueError, "k: 1025, expected 1 <= k <= 1024", m.getTopK, X1, 1025)
    rejects(m, ValueError, "k: 0, expected 1 <= k <= 1024", m.getTopK, np.ones(3, F32), 0)  # k before x
    rejects(m, ValueError, "k: 0, expected 1 <= k <= 1024", m.getTopK, Dev(), 0)


def test_pair_rejects():
    m, five, dbl = matrix(), matrix(5), matrix(code=3, npd=np.float64)
    far = matrix()
    far.device = 1
    for method, name, rest in ((m.getPairsDot, "other", ()), (m.updatePairsAxpy, "src", (WEIGHTS,))):
        for other in (vector(), None):
            rejects(m, TypeError, f"{name}: expected a PartialMatrix", method, other, ROWS, ROWS, *rest)
        for other, what in ((five, "(float32, cuda:0, 5)"), (dbl, "(float64, cuda:0, 4)"),
                            (far, "(float32, cuda:1, 4)")):
            rejects(m, ValueError, f"{name}: expected a shard of this one's type, device and cols (float32, cuda:0, 4), "
                    f"not {what}", method, other, ROWS, ROWS, *rest)
        rejects(m, ValueError, f"{name}: expected a shard of this one's type, device and cols (float32, cuda:0, 4), "
                "not (float32, cuda:0, 5)", method, five, ROWS, Dev(), *rest)  # the shard before the mixing
    rejects(m, TypeError, "rows and other_rows: mixing host arrays and device tensors", m.getPairsDot, m, ROWS, Dev())
    rejects(m, ValueError, "other_rows: 2 rows, expected 3", m.getPairsDot, m, ROWS, ROWS[:2])
    rejects(m, ValueError, "other_rows: 2 rows, expected 3", m.getPairsDot, m, ROWS, ROWS[:2], out=np.empty(2))
    mixing = "rows, src_rows and coef: mixing host arrays and device tensors"
    rejects(m, TypeError, mixing, m.updatePairsAxpy, matrix(), ROWS, Dev(), WEIGHTS)
    rejects(m, TypeError, mixing, m.updatePairsAxpy, matrix(), ROWS, ROWS, Dev())
    rejects(m, ValueError, "src_rows: 2 rows and coef: 3 values, expected 3 of each", m.updatePairsAxpy, matrix(),
            ROWS, ROWS[:2], WEIGHTS)
    rejects(m, ValueError, "src_rows: 3 rows and coef: 2 values, expected 3 of each", m.updatePairsAxpy, matrix(),
            ROWS, ROWS, WEIGHTS[:2])


def test_sparse_seed_and_dtype_rejects():
    m = matrix()
    rejects(m, ValueError, "cap must be >= 0", m.getRowsSparse, ROWS, cap=-1)
    for seed in (-1, 1 << 64):
        rejects(m, ValueError, "seed: expected an unsigned 64-bit integer", m.initUniform, seed, 0.0, 1.0)
        rejects(m, ValueError, "seed: expected an unsigned 64-bit integer", m.initUniform, seed, 0.0, 1.0, rows=ROWS)
    with pytest.raises(ValueError, match=re.escape("unsupported value type 'half' (Int, Long, Float or Double)")):
        S.resolve_dtype("half")


# ---- the client's bucket iterator ---------------------------------------------------------------------------

class _Model:
    def __init__(self, parts, keys):
        self.partitioner = RangePartitioner.apply(parts, keys)
        self.shards = [object() for _ in range(parts)]


def test_bucket_iterator_skips_empty_partitions_and_keeps_the_callers_order():
    model = _Model(3, 9)  # keys [0, 3), [3, 6), [6, 9)
    keys = np.array([7, 0, 8, 2, 7, 1], np.int64)  # nothing for the middle partition
    got = [(p, sh, idx.tolist()) for p, sh, idx in CL._buckets(model, keys)]
    assert got == [(0, model.shards[0], [1, 3, 5]), (2, model.shards[2], [0, 2, 4])]
    assert [(p, idx.tolist()) for p, _, idx in CL._buckets(model, np.array([4, 4], np.int64))] == [(1, [0, 1])]
    assert list(CL._buckets(model, np.zeros(0, np.int64))) == []


def test_bucket_iterator_validates_every_key_before_the_first_bucket():
    model = _Model(3, 9)
    for keys in ([0, 4, 9], [0, 4, -1]):
        got = []
        with pytest.raises(IndexOutOfBoundsException):
            for item in CL._buckets(model, np.array(keys, np.int64)):
                got.append(item)
        assert got == []
