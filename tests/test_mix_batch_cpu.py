"""Batched row mix pull without a GPU: the ABI's symbols, constants and NULL-shard check, and
BigMatrix.pullMixBatch's fan-out and combine over fake shards."""
from pathlib import Path

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix


def test_symbols_constants_and_version():
    lib = N.load()
    assert callable(lib.glint_mat_pull_rows_mix_batch) and callable(lib.glint_mat_pull_rows_mix_batch_dev)
    text = (Path(__file__).resolve().parent.parent / "include" / "glint_gpu.h").read_text()
    for name in ("GLINT_MIX_BATCH_MAX_VECTORS", "GLINT_MIX_BATCH_CHUNK", "GLINT_MIX_BATCH_MAX_CHUNKS"):
        assert f"#define {name} {getattr(N, name)}\n" in text
    assert N.GLINT_MIX_BATCH_MAX_VECTORS == N.GLINT_DOT_MAX_QUERIES and N.GLINT_MIX_BATCH_MAX_CHUNKS == 64
    assert N.GLINT_MIX_BATCH_CHUNK % 32 == 0 and N.GLINT_MIX_BATCH_CHUNK & (N.GLINT_MIX_BATCH_CHUNK - 1) == 0
    assert N.GLINT_K_COUNT == 13
    assert lib.glint_version() > 2200  # glint_version() at the parent of the batched row mix pull
    assert callable(glint_amd.PartialMatrix.getRowsMixBatch) and callable(glint_amd.BigMatrix.pullMixBatch)
    rows, coef, out = np.zeros(1, np.int64), np.zeros(1), np.zeros(4)  # a NULL shard
    args = (None, rows.ctypes.data, 1, coef.ctypes.data, 1, out.ctypes.data)
    assert lib.glint_mat_pull_rows_mix_batch(*args) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_rows_mix_batch_dev(*args, None) == N.GLINT_EINVAL


class FakeShard:
    """Answers getRowsMixBatch from the whole integer-valued table (exact sums) for the rows it owns, and
    keeps what each call was handed."""
    def __init__(self, table, owned):
        self.table, self.owned, self.calls, self.np_dtype = table, set(owned.tolist()), [], table.dtype.type

    def getRowsMixBatch(self, rows, coef):
        self.calls.append((rows.copy(), coef.copy()))
        assert set(rows.tolist()) <= self.owned
        return coef.T @ self.table[rows]


@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("parts", [1, 3, 7])
def test_pull_mix_batch_sends_each_partition_its_own_lines(parts, cyclic):
    rng = np.random.default_rng(29)
    table = rng.integers(-2, 3, (60, 5)).astype(np.float64)
    partitioner = (CyclicPartitioner if cyclic else RangePartitioner).apply(parts, 60)
    owner = partitioner.partition_indices(np.arange(60, dtype=np.int64))
    shards = [FakeShard(table, np.flatnonzero(owner == p)) for p in range(parts)]
    m = BigMatrix(partitioner, shards, 60, 5)
    rows = rng.permutation(np.concatenate([np.arange(60), rng.integers(0, 60, 30)]))  # shuffled, with repeats
    coef = rng.integers(-2, 3, (rows.size, 70)).astype(np.float64)
    np.testing.assert_array_equal(m.pullMixBatch(rows, coef), coef.T @ table[rows])
    for p, sh in enumerate(shards):  # one call each: its own records and their lines, in the caller's order
        [(r, c)], mine = sh.calls, owner[rows] == p
        np.testing.assert_array_equal(r, rows[mine])
        np.testing.assert_array_equal(c, coef[mine])
    few = np.flatnonzero(owner == parts - 1)[[2, 0, 2]]  # rows of the last partition only
    ans = m.pullMixBatch(few, coef[:3, 4])  # coef of shape (n,) answers (cols,)
    np.testing.assert_array_equal(ans, coef[:3, 4] @ table[few])
    assert [len(sh.calls) for sh in shards] == [1] * (parts - 1) + [2]  # none for a partition that owns none
    with pytest.raises(ValueError):
        m.pullMixBatch(few, coef[:2])
