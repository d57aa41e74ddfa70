"""Shard operations in sequence on one PartialMatrix, against the host model of tests/sequence_cases.py.

Each single-operation file builds a fresh shard; here forty to seventy calls share one, so that what a
call leaves behind -- the grow-only scratch and its reallocation in mid-stream, the alternating control
slots, the latched hints, the ordering between host-pointer and device-resident calls, the ring's open
batch, the two error states -- meets the next call. Every pull is compared bit for bit (a NaN by class)
with the model as it stood at that step, every sync with the error the model expects there, and
to_numpy() with the model at the end. tests/test_sequence_cpu.py checks, for every parameter set used
here, the conditions the generator builds in, the model against the oracle, and that the runner fails
at the right step for broken shards."""
import numpy as np
import pytest

from glint_amd import ArrayIndexOutOfBoundsException, PartialMatrix, RangePartition
import glint_amd._native as N
from axpy_cases import assert_bits
import sequence_cases as S

pytestmark = pytest.mark.gpu
GEOMETRY_IDS = [f"{r}x{c}" for r, c in S.GEOMETRIES]


def run_sequences(gpu, geometry, dtype, regime):
    import torch
    d = torch.device("cuda", gpu)
    for seed in S.SEEDS:
        seq = S.sequence(*geometry, dtype, regime, seed)
        with PartialMatrix(RangePartition(2, S.START, S.START + seq.size), seq.cols, dtype, gpu) as sh:
            S.run(sh, seq, d, ArrayIndexOutOfBoundsException)


@pytest.mark.parametrize("dtype", ["double", "float", "long", "int"])
@pytest.mark.parametrize("geometry", S.GEOMETRIES, ids=GEOMETRY_IDS)
def test_sequence_grid(gpu, geometry, dtype):
    run_sequences(gpu, geometry, dtype, "grid")


@pytest.mark.parametrize("dtype", ["double", "float"])
@pytest.mark.parametrize("geometry", S.GEOMETRIES, ids=GEOMETRY_IDS)
def test_sequence_strict(gpu, geometry, dtype):
    run_sequences(gpu, geometry, dtype, "strict")


@pytest.fixture
def pageable_staging(monkeypatch):
    """GLINT_PINNED_STAGE_MAX=0 for the test (test_gpu_validation.test_pinned_stage_max_knob's knob), and
    the default again for the tests after it."""
    monkeypatch.setenv("GLINT_PINNED_STAGE_MAX", "0")
    N.reload_env()
    yield
    monkeypatch.undo()
    N.reload_env()


@pytest.mark.parametrize("dtype,regime", [("float", "strict"), ("long", "grid")])
def test_sequence_pageable_staging(gpu, pageable_staging, dtype, regime):
    """The sequences with every host-pointer call staged from pageable memory, one copy per section, and
    answered straight into the caller's arrays: the branch that only messages above the 2 MiB default
    take."""
    run_sequences(gpu, S.GEOMETRIES[1], dtype, regime)


def test_sequence_on_a_side_stream(gpu):
    """The same sequence and answers with every device-resident call, and every sync, on a stream of the
    caller's own."""
    import torch
    d = torch.device("cuda", gpu)
    seq = S.sequence(*S.GEOMETRIES[1], "double", "grid", 0)
    side = torch.cuda.Stream(d)
    with PartialMatrix(RangePartition(2, S.START, S.START + seq.size), seq.cols, "double", gpu) as sh:
        with torch.cuda.stream(side):
            S.run(sh, seq, d, ArrayIndexOutOfBoundsException)
        side.synchronize()


def test_sequence_on_slab_views(gpu):
    """Four 16-row views of a 17-column Double slab (test_gpu_slab.test_matrix_views' layout): the row
    family on views, two neighbouring views taking their steps in turn. The slab's getRows over all 64
    rows is then the four models side by side, the rows no step touched still zero."""
    import torch
    d = torch.device("cuda", gpu)
    slab = PartialMatrix(RangePartition(0, 0, 64), 17, "double", gpu)
    views = [PartialMatrix.view(slab, RangePartition(j, 16 * j, 16 * (j + 1)), 16 * j) for j in range(4)]
    seqs = [S.sequence(16, 17, "double", "grid", j, start=16 * j, short=True) for j in range(4)]
    try:
        for a, b in ((0, 1), (2, 3)):
            ra = S.Runner(views[a], seqs[a], d, ArrayIndexOutOfBoundsException)
            rb = S.Runner(views[b], seqs[b], d, ArrayIndexOutOfBoundsException)
            assert len(seqs[a].steps) == len(seqs[b].steps)
            for _ in seqs[a].steps:
                ra.step()
                rb.step()
            ra.finish()
            rb.finish()
        got = slab.getRows(torch.arange(0, 64, device=d)).cpu().numpy()
        assert_bits(got, np.vstack([s.final for s in seqs]), "the slab")
        assert all((~s.final.any(axis=1)).sum() >= 4 for s in seqs)  # rows that no step touched
    finally:
        for v in views:
            v.destroy()
        slab.destroy()
