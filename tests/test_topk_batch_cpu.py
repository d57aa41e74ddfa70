"""Batched top-k row pull without a GPU: the ABI's symbols, constants and NULL-shard check, and
BigMatrix.pullTopKBatch's merge over fake shards."""
from pathlib import Path

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix
from topk_cases import global_rows, topk_of_score_table


def test_symbols_constants_and_version():
    lib = N.load()
    assert callable(lib.glint_mat_pull_topk_batch) and callable(lib.glint_mat_pull_topk_batch_dev)
    text = (Path(__file__).resolve().parent.parent / "include" / "glint_gpu.h").read_text()
    assert f"#define GLINT_TOPK_BATCH_MAX_QUERIES {N.GLINT_TOPK_BATCH_MAX_QUERIES}\n" in text
    assert f"#define GLINT_TOPK_BATCH_ROWS {N.GLINT_TOPK_BATCH_ROWS}\n" in text
    assert N.GLINT_TOPK_BATCH_MAX_QUERIES == 1024 and N.GLINT_TOPK_MAX_QUERIES == 64 and N.GLINT_K_COUNT == 13
    assert lib.glint_version() > 1900  # glint_version() at the parent of the batched top-k pull
    assert callable(glint_amd.PartialMatrix.getTopKBatch) and callable(glint_amd.BigMatrix.pullTopKBatch)
    x, rows, vals = np.zeros(4), np.zeros(1, np.int64), np.zeros(1)  # a NULL shard
    args = (None, x.ctypes.data, 1, 1, rows.ctypes.data, vals.ctypes.data)
    assert lib.glint_mat_pull_topk_batch(*args) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_topk_batch_dev(*args, None) == N.GLINT_EINVAL


class FakeShard:
    """Answers getTopKBatch from its slice of an integer-valued table (exact scores), and counts the calls."""
    def __init__(self, table, rows):
        self.table, self.rows, self.calls, self.np_dtype = table, rows, 0, table.dtype.type

    def getTopKBatch(self, x, k):
        self.calls += 1
        return topk_of_score_table(self.table @ x.T, self.rows, k)


@pytest.mark.parametrize("cyclic", [False, True])
@pytest.mark.parametrize("parts", [1, 3, 7])
def test_pull_topk_batch_equals_the_whole_table(parts, cyclic):
    rng = np.random.default_rng(19)
    table = rng.integers(-2, 3, (60, 5)).astype(np.float64)  # full of ties, also across partition borders
    x = rng.integers(-2, 3, (70, 5)).astype(np.float64)
    if cyclic:
        partitioner = CyclicPartitioner.apply(parts, 60)
        shards = [FakeShard(table[i::parts], global_rows(len(table[i::parts]), cyclic=(i, parts))) for i in range(parts)]
    else:
        partitioner = RangePartitioner.apply(parts, 60)
        shards = [FakeShard(table[p.start:p.end], global_rows(p.end - p.start, p.start)) for p in partitioner.all()]
    m = BigMatrix(partitioner, shards, 60, 5)
    for n, k in enumerate((1, 9, 64)):  # 64 exceeds the matrix: the -1 fill
        exp = topk_of_score_table(table @ x.T, global_rows(60), k)
        rows, vals = m.pullTopKBatch(x, k)
        np.testing.assert_array_equal(rows, exp[0])
        np.testing.assert_array_equal(vals, exp[1])
        assert [sh.calls for sh in shards] == [n + 1] * parts  # exactly one getTopKBatch each
    np.testing.assert_array_equal(m.pullTopKBatch(x[4], 9)[0], topk_of_score_table(table @ x.T, global_rows(60), 9)[0][4])
