"""Top-k row pull, the parts that need no GPU: the ABI's symbols, constants and NULL-shard checks, the
order the GPU tests take their expected values from (topk_cases), the level plan's invariants
(glint_topk_plan.h through tests/c/topk_probe.cpp) and BigMatrix.pullTopK's merge over fake shards."""
import ctypes
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartitioner, RangePartitioner
from glint_amd.client import BigMatrix, topk_rank_key
from dot_cases import bits, replay_dot
from topk_cases import assert_topk_bits, expected_topk, rank_key, rank_key_fast, topk_of_scores

ROOT = Path(__file__).resolve().parent.parent
# glint_version() at the parent of the top-k pull ("Top-k pull")
PARENT_VERSION = 600
T = N.GLINT_TOPK_TILE


def test_symbols_constants_and_version():
    lib = N.load()
    assert callable(lib.glint_mat_pull_topk) and callable(lib.glint_mat_pull_topk_dev)
    assert lib.glint_version() > PARENT_VERSION
    assert N.GLINT_K_COUNT == 13 and N.GLINT_K_PULL_ROWS_DOT == 11  # no new kernel id
    assert (N.GLINT_TOPK_MAX_K, N.GLINT_TOPK_MAX_QUERIES, N.GLINT_TOPK_TILE) == (1024, 64, 4096)
    text = (ROOT / "include" / "glint_gpu.h").read_text()
    for name in ("GLINT_TOPK_MAX_K 1024", "GLINT_TOPK_MAX_QUERIES 64", "GLINT_TOPK_TILE 4096"):
        assert f"#define {name}" in text
    assert callable(glint_amd.PartialMatrix.getTopK) and callable(glint_amd.BigMatrix.pullTopK)


def test_null_shard_is_einval():
    lib = N.load()
    x = np.zeros(4)
    rows, vals = np.zeros(1, np.int64), np.zeros(1)
    assert lib.glint_mat_pull_topk(None, x.ctypes.data, 1, 1, rows.ctypes.data, vals.ctypes.data) == N.GLINT_EINVAL
    assert lib.glint_mat_pull_topk_dev(None, x.ctypes.data, 1, 1, rows.ctypes.data, vals.ctypes.data,
                                       None) == N.GLINT_EINVAL
    assert lib.glint_prof_read_launches(None, N.GLINT_K_PULL_ROWS_DOT, None, 0, None) == N.GLINT_EINVAL


# ---- the order -----------------------------------------------------------------------------------
@pytest.mark.parametrize("npd", [np.float64, np.float32])
def test_rank_key_known_answers_float(npd):
    fi = np.finfo(npd)
    sub = npd(fi.smallest_subnormal)
    ladder = np.array([np.nan, -np.inf, -fi.max, -1.0, -sub, 0.0, sub, 1.0, fi.max, np.inf], npd)
    key = rank_key(ladder)
    assert (np.diff(key.astype(object)) > 0).all()  # NaN below -inf, then the numeric order
    assert rank_key(np.array([-0.0], npd))[0] == rank_key(np.array([0.0], npd))[0]  # -0 ties +0
    nans = np.array([np.nan, -np.nan, np.inf - np.inf], npd)
    nans = np.concatenate([nans, (bits(np.array([np.nan], npd)) | 5).view(npd)])  # another payload
    assert np.isnan(nans).all() and len(set(rank_key(nans).tolist())) == 1  # all NaNs rank equal
    np.testing.assert_array_equal(rank_key_fast(ladder), key)
    np.testing.assert_array_equal(rank_key_fast(nans), rank_key(nans))
    np.testing.assert_array_equal(topk_rank_key(ladder), key)  # the client's merge uses the same order
    np.testing.assert_array_equal(topk_rank_key(np.array([-0.0, 0.0], npd)), rank_key(np.array([0.0, 0.0], npd)))
    rng = np.random.default_rng(5)
    with np.errstate(over="ignore"):  # Float: some overflow to inf, some fall to subnormals and zero
        v = (rng.standard_normal(500) * 10.0 ** rng.integers(-40, 40, 500)).astype(npd)
    np.testing.assert_array_equal(rank_key_fast(v), rank_key(v))
    np.testing.assert_array_equal(topk_rank_key(v), rank_key(v))


@pytest.mark.parametrize("npd", [np.int64, np.int32])
def test_rank_key_known_answers_int(npd):
    ii = np.iinfo(npd)
    ladder = np.array([ii.min, ii.min + 1, -1, 0, 1, ii.max - 1, ii.max], npd)
    key = rank_key(ladder)
    assert (np.diff(key.astype(object)) > 0).all()
    np.testing.assert_array_equal(rank_key_fast(ladder), key)
    np.testing.assert_array_equal(topk_rank_key(ladder), key)


def test_ties_are_resolved_by_row_and_nans_come_last():
    scores = np.array([1.0, np.nan, 3.0, -0.0, 3.0, 0.0, -np.inf, np.nan, 3.0])
    rows = np.arange(100, 109, dtype=np.int64)
    r, v = topk_of_scores(scores, rows, 9)
    assert r.tolist() == [102, 104, 108, 100, 103, 105, 106, 101, 107]
    assert bits(v[4:6]).tolist() == bits(np.array([-0.0, 0.0])).tolist()  # a zero keeps its own bits
    r, v = topk_of_scores(scores, rows, 2)
    assert r.tolist() == [102, 104]  # the tie is cut by row
    r, v = topk_of_scores(scores[:3], rows[:3], 5)
    assert r.tolist() == [102, 100, 101, -1, -1] and bits(v[3:]).tolist() == [0, 0]


# ---- the level plan --------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("_glint_build", ROOT / "glint_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(str(mod.build_topk_probe()))
    lib.topk_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.topk_plan_of.restype = ctypes.c_int
    lib.topk_plan_of.argtypes = [ctypes.c_int64] * 4 + [ctypes.POINTER(ctypes.c_uint64), ctypes.POINTER(ctypes.c_int64)]
    lib.topk_tile_of.argtypes = [ctypes.c_int64] * 3 + [ctypes.POINTER(ctypes.c_int64)]
    return lib


def plan(probe, size, q, k, vsize):
    c = (ctypes.c_int64 * 4)()
    probe.topk_constants(c)
    head = (ctypes.c_uint64 * 2)()
    words = (ctypes.c_int64 * (7 * c[3]))()
    n = probe.topk_plan_of(size, q, k, vsize, head, words)
    names = ("n_in", "tiles", "n_out", "in_key", "in_row", "out_key", "out_row")
    return int(head[0]), int(head[1]), [dict(zip(names, words[7 * l:7 * l + 7])) for l in range(n)]


def tile(probe, n, t, k):
    out = (ctypes.c_int64 * 2)()
    probe.topk_tile_of(n, t, k, out)
    return int(out[0]), int(out[1])


PLAN_SIZES = sorted({s for m in range(1, 7) for s in (m * T - 1, m * T, m * T + 1)} | {1, 2**20, 2**31 - 1})


def test_plan_constants(probe):
    c = (ctypes.c_int64 * 4)()
    probe.topk_constants(c)
    assert list(c)[:3] == [T, N.GLINT_TOPK_MAX_K, N.GLINT_TOPK_MAX_QUERIES]


@pytest.mark.parametrize("q", [1, 64])
@pytest.mark.parametrize("k", [1, 2, 37, 1023, 1024])
def test_plan_invariants(probe, k, q):
    for size in PLAN_SIZES:
        for vsize in (4, 8):
            scores_bytes, total, levels = plan(probe, size, q, k, vsize)
            assert levels, (size, k, q)  # it terminates, within the level bound
            assert scores_bytes == q * size * vsize
            # level 0 covers each row once: tiles of T rows, the last one the remainder
            l0 = levels[0]
            assert l0["n_in"] == size and l0["tiles"] == -(-size // T)
            ends = [0, 1, l0["tiles"] // 2, l0["tiles"] - 2, l0["tiles"] - 1, l0["tiles"]]
            for t in {e for e in ends if 0 <= e <= l0["tiles"]}:
                cnt, _ = tile(probe, size, t, k)
                assert cnt == max(0, min(T, size - t * T))
            assert (l0["tiles"] - 1) * T + tile(probe, size, l0["tiles"] - 1, k)[0] == size
            assert tile(probe, size, l0["tiles"], k) == (0, 0)  # nothing past the last tile
            buffers = [(0, scores_bytes)]
            for i, lv in enumerate(levels):
                last = i == len(levels) - 1
                assert lv["tiles"] == max(1, -(-lv["n_in"] // T))
                # a tile emits min(k, count): k for every full tile, so tile t's pairs start at t * k
                full, (cnt, emits) = lv["tiles"] - 1, tile(probe, lv["n_in"], lv["tiles"] - 1, k)
                assert cnt == lv["n_in"] - full * T and 1 <= cnt <= T and emits == min(k, cnt)
                if full:
                    assert tile(probe, lv["n_in"], 0, k) == (T, k) and tile(probe, lv["n_in"], full - 1, k) == (T, k)
                assert lv["n_out"] == full * k + emits
                assert (lv["tiles"] == 1) == last  # the last level, and only it, has one tile per query
                if i > 0:  # a level selects from what the level before emitted
                    prev = levels[i - 1]
                    assert lv["n_in"] == prev["n_out"] and lv["n_in"] < prev["n_in"]
                    assert (lv["in_key"], lv["in_row"]) == (prev["out_key"], prev["out_row"])
                    if k == 1024:
                        assert lv["n_in"] * 4 <= prev["n_in"] + 4 * k  # a level shrinks its input 4x
                if not last:
                    buffers.append((lv["out_key"], q * lv["n_out"] * vsize))
                    buffers.append((lv["out_row"], q * lv["n_out"] * 4))
            # no buffer overlaps another, and all lie inside the scratch
            buffers.sort()
            for (a, na), (b, _) in zip(buffers, buffers[1:]):
                assert a + na <= b, (size, k, q, buffers)
            assert buffers[-1][0] + buffers[-1][1] <= total
            assert all(off % 256 == 0 for off, _ in buffers)


def test_plan_refuses_what_the_call_refuses(probe):
    for size, q, k, vsize in ((-1, 1, 1, 8), (2**31, 1, 1, 8), (10, 0, 1, 8), (10, 65, 1, 8), (10, 1, 0, 8),
                              (10, 1, 1025, 8), (10, 1, 1, 2)):
        assert plan(probe, size, q, k, vsize)[2] == []
    _, total, levels = plan(probe, 0, 3, 7, 4)  # an empty shard: one tile that emits nothing
    assert total == 0 and len(levels) == 1 and levels[0]["n_out"] == 0


def test_plan_level_counts(probe):
    assert len(plan(probe, T, 1, 1024, 8)[2]) == 1
    assert len(plan(probe, T + 1, 1, 1024, 8)[2]) == 2
    assert len(plan(probe, 4 * T + 1, 1, 1024, 8)[2]) == 3  # level 0 emits more than T candidates
    assert len(plan(probe, 5 * T + 3, 1, 1024, 8)[2]) == 3
    assert len(plan(probe, 2**31 - 1, 64, 1024, 8)[2]) == 11  # 2^31 -> 2^29 -> ... -> 2^13 -> 2048


# ---- BigMatrix.pullTopK over fake shards -----------------------------------------------------------
class FakeShard:
    """Answers getTopK from its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, first_row=0, cyclic=None):
        self.table, self.first_row, self.cyclic, self.calls = table, first_row, cyclic, []
        self.np_dtype = table.dtype.type

    def getTopK(self, x, k):
        self.calls.append((np.array(x), k))
        return expected_topk(self.table, x, k, self.first_row, self.cyclic)


def _range_model(table, parts):
    partitioner = RangePartitioner.apply(parts, table.shape[0])
    shards = [FakeShard(table[p.start:p.end], p.start) for p in partitioner.all()]
    return shards, BigMatrix(partitioner, shards, table.shape[0], table.shape[1])


def _cyclic_model(table, parts):
    partitioner = CyclicPartitioner.apply(parts, table.shape[0])
    shards = [FakeShard(table[i::parts], cyclic=(i, parts)) for i in range(parts)]
    return shards, BigMatrix(partitioner, shards, table.shape[0], table.shape[1])


def _tie_table():
    """60 rows of 4 small-integer columns: against x = ones, runs of equal scores all over the table."""
    rng = np.random.default_rng(17)
    return rng.integers(-1, 2, (60, 4)).astype(np.float64)


def test_pull_topk_equals_the_whole_table_and_ignores_the_partitioning():
    rng = np.random.default_rng(18)
    table = (rng.standard_normal((60, 7)) * 10.0 ** rng.integers(-4, 5, (60, 7)))
    x = rng.standard_normal((3, 7))
    for tab, xs in ((table, x), (_tie_table(), np.ones((2, 4)))):
        for k in (1, 5, 60):
            exp = expected_topk(tab, xs, k)
            for make in (_range_model, _cyclic_model):
                for parts in (1, 3, 7):
                    shards, m = make(tab, parts)
                    assert_topk_bits(m.pullTopK(xs, k), exp, f"k={k} parts={parts}")
                    assert all(len(sh.calls) == 1 and sh.calls[0][1] == k for sh in shards)  # one getTopK each
                    one = m.pullTopK(xs[1], k)
                    assert one[0].shape == (k,)
                    assert_topk_bits(one, (exp[0][1], exp[1][1]), "1-d x")


def test_pull_topk_tie_across_a_partition_border_goes_to_the_lower_row():
    table = np.zeros((9, 2))
    table[[2, 3, 7], 0] = 5.0  # rows 2 | 3 straddle the border of partitions 0 | 1 (3 rows each)
    shards, m = _range_model(table, 3)
    assert [sh.first_row for sh in shards] == [0, 3, 6]
    x = np.array([1.0, 0.0])
    for k, want in ((1, [2]), (2, [2, 3]), (4, [2, 3, 7, 0])):
        rows, vals = m.pullTopK(x, k)
        assert rows.tolist() == want
        assert_topk_bits((rows, vals), expected_topk(table, x, k))


def test_pull_topk_partitions_smaller_than_k_and_k_above_the_total():
    tab = _tie_table()[:20]
    x = np.ones(4)
    shards, m = _range_model(tab, 7)  # partitions of 2 or 3 rows
    assert max(sh.table.shape[0] for sh in shards) == 3
    exp = expected_topk(tab, x, 10)
    assert (exp[0] >= 0).all()
    assert_topk_bits(m.pullTopK(x, 10), exp, "partitions smaller than k")  # every shard answers with -1 fill
    rows, vals = m.pullTopK(x, 32)  # more than the matrix has
    assert_topk_bits((rows, vals), expected_topk(tab, x, 32))
    assert (rows[:20] >= 0).all() and rows[20:].tolist() == [-1] * 12 and bits(vals[20:]).tolist() == [0] * 12
    assert sorted(rows[:20].tolist()) == list(range(20))  # every row once
    with pytest.raises(ValueError):
        m.pullTopK(np.ones(5), 3)
    with pytest.raises(ValueError):
        m.pullTopK(x, 0)


def test_pull_topk_nan_scores_merge_last():
    table = np.ones((12, 2))
    table[[1, 6, 11], 0] = np.inf  # inf * 0 = NaN
    table[4, 1] = -np.inf
    x = np.array([0.0, 1.0])
    exp = expected_topk(table, x, 12)
    assert exp[0][-3:].tolist() == [1, 6, 11] and exp[0][-4] == 4 and np.isnan(replay_dot(table[[1]], x))[0]
    for parts in (1, 3, 7):
        _, m = _range_model(table, parts)
        assert_topk_bits(m.pullTopK(x, 12), exp, f"parts={parts}")
        assert_topk_bits(m.pullTopK(x, 9), expected_topk(table, x, 9), f"no NaN, parts={parts}")
