"""The binned unordered push (glint_bin.hip) on inputs constructed to reach its data-dependent branches
(tests/bin_cases.py: bin_fsort's slow gather, the plan's wave emit / walk / staging-tile limits with the
plan fused and launched, units closed at the run cap, bin_apply2's write-back variants at their
thresholds, bin_scan's items ending on run boundaries), against the oracle.

Under GLINT_BIN_FRONT=prep the host model is exact, and each test first re-evaluates the case's
predicates for this device's CU count: a device on which a case does not reach its branches fails the
test (it is never skipped). The same keys are also pushed through the hot and dedup front ends and with
no front end forced; there the model is not claimed, except for case A's hot variant, whose thin records
are cold and keep their chunks.

Long (Int for case D's 2^28-element shard) is compared bit for bit; Double within 1e-9 of each
element's sum of magnitudes, the bar of test_binned_stream_of_batches; Float bit for bit on the variant
of case E with one record per element per push."""
import ctypes as C

import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import PartialMatrix, PartialVector, RangePartition
from oracle import oracle as O

import bin_cases as B

pytestmark = pytest.mark.gpu

FRONT_NAMES = ("prep", "hot", "dedup", "auto")
# (case, dtype): every front end of each, the case outermost so that its keys and reference are built once
RUNS = [("A", "long"), ("A", "double"), ("B", "long"), ("B", "double"), ("C", "long"), ("D_small", "int"),
        ("D_large", "int"), ("E", "long"), ("E", "double"), ("E_mat", "long"), ("E_mat", "double"),
        ("E_unique", "float"), ("E_unique_mat", "float")]
PARAMS = [(case, dtype, front) for case, dtype in RUNS for front in FRONT_NAMES]

_ref = {}


def _cus(gpu):
    import torch
    return int(torch.cuda.get_device_properties(gpu).multi_processor_count)


def _launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


def _reference(c, dtype, vals):
    """The oracle's shard after the two pushes, and each element's sum of magnitudes (Double); kept for
    the case's other front ends."""
    key = (c.name, dtype)
    if key not in _ref:
        _ref.clear()
        code = O.CODE[dtype]
        if c.cols:
            ref = O.OracleMatrix(O.part_range(0, -(-c.elems // (c.cols + 1))), c.cols, code)
        else:
            ref = O.OracleVector(O.part_range(0, c.elems), code)
        for _ in range(2):
            assert ref.update(*B.keys(c), vals) == -1
        mag = None
        if dtype == "double":
            mag = 2 * np.bincount(c.addr, np.abs(vals), minlength=c.elems)
            if c.cols:
                mag = mag.reshape(-1, c.cols + 1)[:, :c.cols]
        _ref[key] = (ref.data, mag)
    return _ref[key]


@pytest.mark.parametrize("case,dtype,front", PARAMS, ids=["-".join(p) for p in PARAMS])
def test_binned_constructed(gpu, monkeypatch, case, dtype, front):
    cus = _cus(gpu)
    # case A under the hot front end: the variant built for its chunks of 4096, with the model claimed
    name = "A_hot" if (case, front) == ("A", "hot") else "A_prep" if case == "A" else case
    c = B.build(name, cus)
    if front == "prep" or name == "A_hot":
        res = c.checks(c.m)
        failed = sorted(k for k, v in res.items() if not v)
        if failed or cus not in B.SUPPORTED_CUS[name]:
            pytest.fail(f"case {name} does not reach its branches on {cus} CUs: {failed}")
    if front != "auto":
        monkeypatch.setenv("GLINT_BIN_FRONT", front)
    else:
        monkeypatch.delenv("GLINT_BIN_FRONT", raising=False)
    N.reload_env()
    vals = B.values(c, dtype)
    want, mag = _reference(c, dtype, vals)
    if c.cols:
        sh = PartialMatrix(RangePartition(0, 0, -(-c.elems // (c.cols + 1))), c.cols, dtype, gpu)
    else:
        sh = PartialVector(RangePartition(0, 0, c.elems), dtype, gpu)
    with sh:
        N.load().glint_prof_enable(sh.handle, 1)
        for _ in range(2):
            sh.update(*B.keys(c), vals, unordered=True)
        assert _launches(sh, N.GLINT_K_PUSH_BINNED) == 2
        got = sh.to_numpy()
    assert got.shape == want.shape and got.dtype == want.dtype
    if dtype == "double":
        bad = np.abs(got - want) > 1e-9 * mag
    else:
        bad = got != want
    if bad.any():
        where = np.flatnonzero(bad.reshape(-1))
        if c.cols:
            where = (where // c.cols) * (c.cols + 1) + where % c.cols
        slabs = np.unique(where >> B.K_SLAB_BITS)
        fb, nf = c.L["fb"], c.L["nf"]
        pytest.fail(f"{where.size} elements differ, the first at address {int(where[0])}; (bucket, slab) of the "
                    f"first wrong slabs under the plain front end's geometry: "
                    f"{[(int(s) >> fb, int(s) & (nf - 1)) for s in slabs[:16]]}")
