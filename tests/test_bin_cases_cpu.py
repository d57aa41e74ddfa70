"""tests/bin_cases.py on a CPU: its restatement of bin_layout equals the real headers' (through
tests/c/plan_probe.cpp), every case's predicates hold under the host model at the CU counts the case
supports (and, explicitly, not at the others), and the expected sums do not hang on one implementation:
the oracle's result equals numpy's add.at on int64."""
import ctypes
import importlib.util
import itertools
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent
import bin_cases as B
from oracle import oracle as O

CUS = (64, 256, 304)


@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("_glint_build", ROOT / "glint_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(str(mod.build_plan_probe()))


def probe_layout(probe, *args):
    inp = (ctypes.c_int64 * 6)(*args)
    out = (ctypes.c_int64 * len(B.LAYOUT_WORDS))()
    probe.plan_layout(inp, out)
    return dict(zip(B.LAYOUT_WORDS, out))


@pytest.fixture(scope="module", params=list(B.CASES))
def name(request):
    """(module scope: pytest runs the tests case by case, so each case is built once)"""
    B.shape(request.param)
    return request.param


def test_shapes_known(name):
    assert B.shape(name)[1] > 0


def test_layout_restatement_equals_the_headers(probe):
    shapes = {B.shape(name)[:2] for name in B.CASES}
    shapes |= set(itertools.product((1, 4096, 4097, 1 << 20, 1 << 28, (1 << 32) - 2), (1, 4095, 4096, 1 << 20, 1 << 26)))
    checked = 0
    for (elems, n), cus, front, acc, occ in itertools.product(sorted(shapes), CUS, (0, 1, 2), (4, 8), (1, 2)):
        got = B.layout(elems, n, cus, front, acc, occ)
        want = probe_layout(probe, elems, n, cus, front, acc, occ)
        assert {k: got[k] for k in B.LAYOUT_WORDS} == want, (elems, n, cus, front, acc, occ)
        checked += 1
    assert checked >= 3 * 3 * len(B.CASES)


def test_every_case_supports_256_cus():
    assert set(B.SUPPORTED_CUS) == set(B.CASES)
    assert all(256 in s and s <= set(CUS) for s in B.SUPPORTED_CUS.values())


def test_predicates_hold_under_the_model(name):
    """At every supported CU count each declared predicate holds; at an unsupported one the case says so
    itself: some predicate is false there (no silent pass either way)."""
    for cus in CUS:
        c = B.build(name, cus)
        assert c.L == B.layout(c.elems, c.n, cus, c.front)
        res = c.checks(c.m)
        assert res and all(isinstance(v, (bool, np.bool_)) for v in res.values()), res
        failed = sorted(k for k, v in res.items() if not v)
        if cus in B.SUPPORTED_CUS[name]:
            assert not failed, (name, cus, failed)
        else:
            assert failed, (name, cus, "listed as unsupported, but every predicate holds")


def test_model_bounds_hold_for_an_order_inside_the_runs(name):
    """The model's bounds against a direct count: records stably sorted by (bucket, chunk) are one order
    the device may produce; each (item, slab) count of that order lies within [lo, hi], and the chunk
    windows are those of the items' first and last records."""
    c = B.build(name, 256)
    m, L = c.m, c.L
    slab = c.addr >> B.K_SLAB_BITS
    bucket = slab >> L["fb"]
    chunk = np.arange(c.n) // L["kchunk"]
    order = np.lexsort((chunk, bucket))
    start = np.concatenate(([0], np.cumsum(m.T)[:-1]))
    v = np.arange(c.n) - start[bucket[order]]
    it = m.Ib[bucket[order]] + v // L["item"]
    cnt = np.bincount(it * L["nf"] + (slab[order] & (L["nf"] - 1)), minlength=m.lo.size).reshape(m.lo.shape)
    assert (m.lo <= cnt).all() and (cnt <= m.hi).all()
    assert (m.lo.sum(axis=0) <= m.hi.sum(axis=0)).all() and (m.hi >= m.lo).all()
    has = np.bincount(it, minlength=m.lo.shape[0]) > 0
    first = np.full(m.lo.shape[0], c.n, np.int64)
    last = np.zeros(m.lo.shape[0], np.int64)
    np.minimum.at(first, it, chunk[order])
    np.maximum.at(last, it, chunk[order])
    assert (m.cwx[has] == first[has]).all() and (m.cwy[has] == last[has]).all()
    assert (m.J == np.maximum(1, -(-m.T // L["item"]))).all() and int(m.T.sum()) == c.n


def test_oracle_equals_add_at(name):
    c = B.build(name, 256)
    dtype = "int" if name.startswith("D") else "long"
    vals = B.values(c, dtype)
    u, inv = np.unique(c.addr, return_inverse=True)
    want = np.zeros(u.size, np.int64)
    np.add.at(want, inv, vals.astype(np.int64))
    want = want.astype(B.NP_DTYPE[dtype])  # (Int sums wrap)
    if c.cols:
        rows = -(-c.elems // (c.cols + 1))
        ref = O.OracleMatrix(O.part_range(0, rows), c.cols, O.CODE[dtype])
        assert ref.update(*B.keys(c), vals) == -1
        got = ref.data[u // (c.cols + 1), u % (c.cols + 1)]
    else:
        ref = O.OracleVector(O.part_range(0, c.elems), O.CODE[dtype])
        assert ref.update(*B.keys(c), vals) == -1
        got = ref.data[u]
    np.testing.assert_array_equal(got, want)
    assert np.count_nonzero(ref.data) == np.count_nonzero(want)
