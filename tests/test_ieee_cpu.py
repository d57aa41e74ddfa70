"""The IEEE edge-value cases (tests/ieee_cases.py) against the oracle alone -- no GPU.

tests/test_gpu_ieee.py compares the device with the cases' own expectations, bit for bit and in any
summation order. That is only sound if the reference itself stays within the condition: here the
oracle's sequential loop must give the builder's expected bits for every case, and must give them again
for a random permutation of the records.
"""
import numpy as np
import pytest

import ieee_cases as I
from oracle import oracle as O

DT = ["float", "double"]
GRID_NAMES = ["subnormal", "crossing", "unit", "top"]


def oracle_push(ref, keys, vals, perm=None):
    k, v = I.flat_records(keys, vals)
    if perm is not None:
        k, v = k[perm], v[perm]
    assert ref.update(k, v) == -1


def elements(shape):
    _, _, size, width, _ = I.SHAPES[shape]
    return size * width


@pytest.mark.parametrize("grid", GRID_NAMES)
@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", list(I.SHAPES))
def test_exact_grid_is_order_free(shape, dtype, grid):
    keys, vals, expect = I.grid_case(shape, dtype, grid)
    rng = I.rng_for("cpu/perm", shape, dtype, grid)
    straight = O.OracleVector(O.part_range(0, elements(shape)), O.CODE[dtype])
    mixed = O.OracleVector(O.part_range(0, elements(shape)), O.CODE[dtype])
    for p in range(2):
        oracle_push(straight, keys, vals)
        oracle_push(mixed, keys, vals, rng.permutation(vals.size))
        I.assert_matches(straight.data, expect[p], what=f"push {p + 1}")
        I.assert_matches(mixed.data, expect[p], what=f"permuted push {p + 1}")


@pytest.mark.parametrize("dtype", DT)
def test_grids_cover_the_subnormal_range(dtype):
    """On the shape with a hot key: the subnormal grid never leaves the subnormal range, the crossing
    grid sums subnormal addends to normal numbers, the top grid sits within 2^-100 of the limit."""
    tiny, big = np.finfo(I.NPD[dtype]).tiny, np.finfo(I.NPD[dtype]).max
    _, vals, expect = I.grid_case("binned", dtype, "subnormal")
    assert np.abs(expect).max() < tiny and np.count_nonzero(expect) > expect.size // 2
    for shape in I.SHAPES:
        _, vals, expect = I.grid_case(shape, dtype, "crossing")
        assert np.abs(vals).max() < tiny, "every addend is subnormal"
        assert (np.abs(expect[1]) >= tiny).any(), f"{shape}: no sum became normal"
        assert ((expect[1] != 0) & (np.abs(expect[1]) < tiny)).any(), f"{shape}: no sum stayed subnormal"
    _, vals, expect = I.grid_case("binned", dtype, "top")
    assert np.abs(expect).max() > big * 2.0 ** -100 and np.isfinite(expect).all()


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", list(I.SHAPES))
def test_nonfinite_classes_are_order_free(shape, dtype):
    case = I.nonfinite_case(shape, dtype)
    rng = I.rng_for("cpu/perm/nf", shape, dtype)
    straight = O.OracleVector(O.part_range(0, elements(shape)), O.CODE[dtype])
    mixed = O.OracleVector(O.part_range(0, elements(shape)), O.CODE[dtype])
    for p, (keys, vals) in enumerate(case.pushes):
        oracle_push(straight, keys, vals)
        # (a pattern with one record per key stays one: the dense apply's shape)
        oracle_push(mixed, keys, vals, rng.permutation(vals.size))
        I.assert_matches(straight.data, case.expect[p], case.cls, f"push {p + 1}")
        I.assert_matches(mixed.data, case.expect[p], case.cls, f"permuted push {p + 1}")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", list(I.SHAPES))
def test_nonfinite_chosen_elements(shape, dtype):
    """The required elements are chosen, every class occurs, and every neighbour of a chosen element
    (the other half of its pair included) is an exact, finite one."""
    pattern, _, size, width, cols = I.SHAPES[shape]
    case = I.nonfinite_case(shape, dtype)
    elems = size * width
    chosen = np.flatnonzero(case.cls)
    assert 24 <= chosen.size <= 48
    must = [elems - 1, 21] + ([] if shape == "dense_odd_start" else [0]) + [10]
    must += [e for e in (4095, 8192) if e < elems - 8] + ([5 * cols, 8 * cols - 1] if cols else [])
    assert set(must) <= set(chosen.tolist())
    assert cols or elems % 2 == 1
    assert set(case.cls[chosen].tolist()) == {I.PINF, I.NINF, I.NAN}
    assert (np.diff(chosen) > 1).all()
    for p in range(2):
        assert np.isfinite(case.expect[p][case.cls == I.EXACT]).all()


def test_nonfinite_recipes_match_the_issue_table():
    """inf + 1, inf - inf, NaN + 1, 3 x MAX, -inf - 5 through the oracle, each on its own key."""
    for dtype in DT:
        npd = I.NPD[dtype]
        rows = [(["+inf", 1.0], I.PINF), (["+inf", "-inf"], I.NAN), (["nan", 1.0], I.NAN),
                (["+max", "+max", "+max"], I.PINF), (["-inf", -5.0], I.NINF)]
        ref = O.OracleVector(O.part_range(0, len(rows)), O.CODE[dtype])
        for i, (addends, _) in enumerate(rows):
            for a in addends:
                assert ref.update(np.array([i], np.int64), np.array([I.special(a, dtype)], npd)) == -1
        assert I.classify(ref.data).tolist() == [c for _, c in rows]


@pytest.mark.parametrize("dtype", DT)
def test_ordered_vectors_tell_the_folds_apart(dtype):
    """Each alternative to the sequential fold in V changes at least one vector's bits: summing the
    addends first, and accumulating in a wider type that is rounded to V once (Float: double; Double:
    the platform's long double where it is wider)."""
    vecs = I.ordered_vectors(dtype)
    seq = np.array([I.sequential(d, a, dtype) for d, a in vecs])
    want = {"float": [np.inf, np.finfo(np.float32).max, -np.inf, -0.0, 0.0],
            "double": [np.inf, np.finfo(np.float64).max, -np.inf, -0.0, 0.0]}[dtype]
    assert I.bits(seq).tolist() == I.bits(np.array(want, I.NPD[dtype])).tolist()
    pre = np.array([I.presummed(d, a, dtype) for d, a in vecs])
    assert (I.bits(pre) != I.bits(seq)).any()
    wider = np.float64 if dtype == "float" else np.longdouble
    if np.finfo(wider).max > np.finfo(I.NPD[dtype]).max:
        wide = np.array([I.sequential(d, a, dtype, acc_type=wider) for d, a in vecs])
        assert (I.bits(wide) != I.bits(seq)).any()
    else:
        assert dtype == "double"


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("shape", list(I.ORDERED_SHAPES))
def test_ordered_cases_against_the_oracle(shape, dtype):
    case = I.ordered_shape(shape, dtype)
    ref = O.OracleVector(O.part_range(0, case.init.size), O.CODE[dtype])
    ref.data[:] = case.init
    oracle_push(ref, case.keys, case.vals)
    I.assert_matches(ref.data, case.expect, case.cls, shape)
    w = 1 if case.vals.ndim == 1 else case.vals.shape[1]
    velems = I.vector_elems(w)
    assert (case.cls[velems] == I.EXACT).all()
    want = [I.sequential(d, a, dtype) for d, a in I.ordered_vectors(dtype)]
    assert I.bits(case.expect[velems]).tolist() == I.bits(np.array(want, I.NPD[dtype])).tolist()
    assert {0, case.init.size - 1} <= set(np.flatnonzero(case.cls).tolist())
    # three consecutive messages are the same sequence
    ref3 = O.OracleVector(O.part_range(0, case.init.size), O.CODE[dtype])
    ref3.data[:] = case.init
    for part in np.array_split(np.arange(case.keys.size), 3):
        oracle_push(ref3, case.keys[part], case.vals[part])
    I.assert_matches(ref3.data, case.expect, case.cls, shape)


def test_edge_image_holds_every_edge_value():
    for dtype in DT:
        npd = I.NPD[dtype]
        fi = np.finfo(npd)
        for rows, cols in ((1, 1), (4099, 1), (4097, 3), (4097, 64)):
            img = I.edge_image(dtype, rows, cols)
            if img.size < 15:
                continue
            flat = img.reshape(-1)
            b = I.bits(flat)
            assert (b == I.bits(np.array([-0.0], npd))[0]).any()
            nan_bits = np.unique(b[np.isnan(flat)])
            assert nan_bits.size >= 5 and np.signbit(flat[np.isnan(flat)]).any()
            for v in (np.inf, -np.inf, fi.smallest_subnormal, fi.tiny, fi.max, -fi.max,
                      np.nextafter(fi.tiny, npd(0))):
                assert (flat == npd(v)).any(), v
