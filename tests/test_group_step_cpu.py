"""Grouped optimizer row pushes, the parts that need no GPU: the ABI's symbols, and the premises the GPU
tests rest on -- asserted from the replays alone, on the inputs test_gpu_group_step.py pushes."""
import numpy as np
import pytest

from glint_amd import _native as N
from group_cases import bits, group_contrib, group_of
from group_step_cases import OPT, case, inputs, replay, start


def test_abi():
    lib = N.load()
    for _, _, symbol, _, kc, _, _ in OPT.values():
        nulls = (None, None, None, 0, None, 0, None, None) + kc
        assert getattr(lib, symbol)(*nulls) == N.GLINT_EINVAL
        assert getattr(lib, symbol + "_dev")(*nulls, None) == N.GLINT_EINVAL
    assert lib.glint_version() > 1800
    assert N.GLINT_K_COUNT == 13 and N.GLINT_K_PUSH_ROWS == 8  # no new kernel id


@pytest.mark.parametrize("dtype_name", ["float64", "float32"])
@pytest.mark.parametrize("cols", [3, 67, 128])
@pytest.mark.parametrize("name", list(OPT))
def test_premises(name, cols, dtype_name):
    """Every expected table is finite; the order of a row's records shows in the bits (from 67 columns on);
    the weighted contributions are not the unweighted ones."""
    for weighted in (False, True):
        w, s = case(name, dtype_name, cols, weighted)
        assert np.isfinite(w).all() and np.isfinite(s).all()
    local, offsets, values, coef = inputs(dtype_name, cols, True)
    w0, s0 = start(name, dtype_name, cols)
    if cols >= 67:
        fwd = replay(name, w0, s0, local, offsets, values, coef)
        rev = replay(name, w0, s0, local, offsets, values, coef, order=np.arange(local.size)[::-1])
        # the rows with runs of 300, 70 and 9 records at least (a run of two commutes)
        assert (bits(fwd[0]) != bits(rev[0])).any(axis=1).sum() >= 3
    group = group_of(offsets, local.size)
    assert (bits(group_contrib(values, group, coef)) != bits(group_contrib(values, group))).mean() > 0.9
