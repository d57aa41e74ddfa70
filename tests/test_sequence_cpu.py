"""Operation sequences, the parts that need no GPU: the conditions the generator guarantees, for every
parameter set tests/test_gpu_sequence.py uses; the model against the oracle; and the runner against a
numpy stand-in of the shard -- which must pass, and fail at the right step for three broken stand-ins."""
import re

import numpy as np
import pytest
import torch

from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException
from ieee_cases import LIMIT
from oracle import oracle as O
from axpy_cases import assert_bits, replay_contrib
import sequence_cases as S
import topk_cases

GRID = [(g, dt, "grid") for g in S.GEOMETRIES for dt in ("double", "float", "long", "int")]
STRICT = [(g, dt, "strict") for g in S.GEOMETRIES for dt in ("double", "float")]
CPU = torch.device("cpu")
PUSH_VARIANTS = {"grid": {"host", "dev", "dev_unordered", "dev_det", "async"}, "strict": {"host", "dev_det", "async"}}
ROW_VARIANTS = {"grid": {"host", "dev", "dev_det"}, "strict": {"host", "dev_det"}}


def test_constants_and_walks():
    assert S.TOPK_TILE == N.GLINT_TOPK_TILE
    edges = {(a, b) for w in S.WALKS for a, b in zip(w, w[1:])}
    assert len(edges) == 36 and all(len(w) == 19 for w in S.WALKS)
    assert S.rows_scratch_bytes(S.GROW_RECORDS) > S.SCRATCH_FLOOR


@pytest.mark.parametrize("dtype", ["double", "float", "long", "int"])
@pytest.mark.parametrize("cols", [1, 2, 3, 4, 67, 130, 256])
def test_table_scores_are_the_dot_replay(dtype, cols):
    """The model's scores on the lanes that own a column are topk_cases.scores_of bit for bit, and the
    model's top-k is topk_cases.expected_topk: zero rows, negative and zero x, NaN and -0 included."""
    npd = S.NPD[dtype]
    rng = np.random.default_rng(cols)
    m = S.Model(300, cols, npd, start=11)
    if dtype in ("double", "float"):
        m.table[:] = (rng.standard_normal((300, cols)) * 10.0 ** rng.integers(-4, 5, (300, cols))).astype(npd)
        m.table[rng.random((300, cols)) < 0.3] = 0
        m.table[5, 0], m.table[6, cols - 1], m.table[7] = np.nan, -0.0, -0.0
        x = rng.standard_normal((5, cols)).astype(npd)
        x[1], x[2, 0] = -np.abs(x[1]), 0
    else:
        info = np.iinfo(npd)
        m.table[:] = rng.integers(info.min, info.max, (300, cols), dtype=npd, endpoint=True)
        x = rng.integers(info.min, info.max, (5, cols), dtype=npd, endpoint=True)
    m.table[100:140] = 0
    assert_bits(S.table_scores(m.table, x), topk_cases.scores_of(m.table, x))
    for xs, k in ((x, 9), (x[3], 310)):
        got, exp = m.topk(xs, k), topk_cases.expected_topk(m.table, xs, k, first_row=11)
        topk_cases.assert_topk_bits(got, exp)


# ---- a numpy stand-in with PartialMatrix's method surface ---------------------------------------------
class StandIn:
    """The model behind the shard's methods; a torch (CPU) tensor argument marks a device-resident call,
    which notes a row outside the partition for the next sync where a host-pointer call raises."""

    def __init__(self, seq):
        self.m = S.Model(seq.size, seq.cols, S.NPD[seq.dtype], seq.start)
        self.size, self.cols, self.np_dtype = seq.size, seq.cols, S.NPD[seq.dtype]
        self.pending, self.last_scratch, self.last_call = None, None, None

    @staticmethod
    def dev(x):
        return isinstance(x, torch.Tensor)

    @staticmethod
    def a(x):
        return None if x is None else (x.numpy() if isinstance(x, torch.Tensor) else np.asarray(x))

    def out(self, dev, *arrays):
        res = tuple(torch.from_numpy(np.array(a)) if dev else np.array(a) for a in arrays)
        return res if len(res) > 1 else res[0]

    def note(self, dev, bad):
        if bad is not None:
            assert dev, "the sequences give host-pointer calls rows of the partition only"
            self.pending = bad if self.pending is None else self.pending

    def called(self, name, dev, scratch):
        self.last_call = (name, dev)
        if scratch:
            self.last_scratch = name

    def update(self, rows, cols, values, deterministic=False, sync=True, unordered=False):
        self.m.push(self.a(rows), self.a(cols), self.a(values))
        self.called("push", self.dev(rows), deterministic and self.dev(rows) and self.a(rows).size > S.ORDERED_MAX)
        return True

    def updateRows(self, rows, values, deterministic=False, sync=True, unordered=False):
        self.note(self.dev(rows), self.m.push_rows(self.a(rows), self.a(values)))
        self.called("rows", self.dev(rows), True)
        return True

    def updateRowsAxpy(self, rows, coef, x, deterministic=False, sync=True, unordered=False):
        self.note(self.dev(rows), self.m.push_axpy(self.a(rows), self.a(coef), self.a(x)))
        self.called("axpy", self.dev(rows), True)
        return True

    def get(self, rows, cols, out=None, sync=True):
        self.called("get", self.dev(rows), False)
        return self.out(self.dev(rows), self.m.get(self.a(rows), self.a(cols)))

    def getRows(self, rows, out=None, sync=True):
        res, bad = self.m.get_rows(self.a(rows))
        self.note(self.dev(rows), bad)
        self.called("getrows", self.dev(rows), False)
        return self.out(self.dev(rows), res)

    def getRowsSparse(self, rows, cap=None, sync=True):
        (ip, c, v), bad = self.m.sparse(self.a(rows))
        self.note(self.dev(rows), bad)
        self.called("sparse", self.dev(rows), True)
        if cap is not None:  # entries at positions >= cap are not stored: whatever the buffer held
            cc, vv = np.full(cap, -7, np.int32), np.full(cap, 77, v.dtype)
            cc[:min(cap, c.size)], vv[:min(cap, v.size)] = c[:cap], v[:cap]
            c, v = cc, vv
        return self.out(self.dev(rows), ip, c, v)

    def getRowsSum(self, rows, offsets, out=None, sync=True):
        res, bad = self.m.sum(self.a(rows), self.a(offsets))
        self.note(self.dev(rows), bad)
        self.called("sum", self.dev(rows), not self.dev(rows))
        return self.out(self.dev(rows), res)

    def getRowsDot(self, rows, x=None, out=None, sync=True):
        res, bad = self.m.dot(self.a(rows), self.a(x))
        self.note(self.dev(rows), bad)
        self.called("dot", self.dev(rows), not self.dev(rows))
        return self.out(self.dev(rows), res)

    def getTopK(self, x, k, sync=True):
        self.called("topk", self.dev(x), True)
        return self.out(self.dev(x), *self.m.topk(self.a(x), k))

    def push_async(self, rows, cols, values):
        self.update(rows, cols, values)
        return 0

    def pull_async(self, *arrays, rows=False, out=None):
        assert rows is True and len(arrays) == 1
        return 0, self.getRows(arrays[0])

    def wait(self, ticket):
        pass

    def sync(self, stream=None):
        bad, self.pending = self.pending, None
        if bad is not None:
            raise ArrayIndexOutOfBoundsException(f"record {bad} is outside the partition", bad)

    def to_numpy(self):
        return self.m.table.copy()


class DropsAfterTopK(StandIn):
    """Loses the last record of a row push whose scratch was last used by a top-k pull."""

    def updateRows(self, rows, values, **kw):
        if self.last_scratch == "topk":
            n = self.a(rows).size
            rows, values = self.a(rows)[:n - 1], self.a(values).reshape(n, -1)[:n - 1]
            self.m.push_rows(rows, values)
            self.called("rows", True, True)
            return True
        return super().updateRows(rows, values, **kw)


class StaleSparse(StandIn):
    """Answers a sparse pull from the table as it was before the unsynced push directly in front of it."""
    before = None

    def update(self, rows, cols, values, **kw):
        self.before = self.m.table.copy()
        return super().update(rows, cols, values, **kw)

    def getRowsSparse(self, rows, cap=None, sync=True):
        if self.last_call == ("push", True):
            now, self.m.table = self.m.table, self.before
            try:
                return super().getRowsSparse(rows, cap=cap, sync=sync)
            finally:
                self.m.table = now
        return super().getRowsSparse(rows, cap=cap, sync=sync)


class LateError(StandIn):
    """Reports a pending out-of-range error one sync late."""
    held = None

    def sync(self, stream=None):
        bad, self.held, self.pending = self.held, self.pending, None
        if bad is not None:
            raise ArrayIndexOutOfBoundsException(f"record {bad} is outside the partition", bad)


def run_on(cls, seq):
    sh = cls(seq)
    S.run(sh, seq, CPU, ArrayIndexOutOfBoundsException)
    return sh


# ---- the model against the oracle ------------------------------------------------------------------------
def oracle_table(seq):
    """Every push of the sequence expanded into triplets (test_gpu_rows.oracle_apply's expansion) and
    applied to the oracle in order; rows outside the partition left out, as a device-resident push skips
    them."""
    ref = O.OracleMatrix(O.part_range(seq.start, seq.start + seq.size), seq.cols, O.CODE[seq.dtype])
    cols = np.arange(seq.cols, dtype=np.int32)
    for s in seq.steps:
        a = s.args
        if s.op == "push":
            assert ref.update(a["rows"], a["cols"], a["vals"]) == -1
        elif s.op in ("rows", "axpy"):
            values = a["values"] if s.op == "rows" else replay_contrib(a["coef"], a["x"])
            ok = (a["rows"] >= seq.start) & (a["rows"] < seq.start + seq.size)
            assert (s.bad is None) == bool(ok.all())
            rows, values = a["rows"][ok], values.reshape(-1, seq.cols)[ok]
            assert ref.update(np.repeat(rows, seq.cols), np.tile(cols, rows.size), values.reshape(-1)) == -1
    return ref.data


# ---- the conditions ----------------------------------------------------------------------------------------
def check_conditions(seq, regime):
    steps = seq.steps
    fam = [s.op for s in steps]
    # counts and the end
    for f in S.FAMILIES:
        assert fam.count(f) >= 2, f
    assert fam.count("sync") >= 2 and fam.count("wait") >= 2
    variants = {f: {s.variant for s in steps if s.op == f} for f in S.FAMILIES}
    assert variants["push"] == PUSH_VARIANTS[regime]
    assert variants["rows"] == ROW_VARIANTS[regime] == variants["axpy"]
    assert variants["get"] == {"host", "dev"} and variants["getrows"] == {"host", "dev", "async"}
    assert variants["sparse"] == {"host", "dev", "dev_cap"}
    assert variants["sum"] == variants["topk"] == {"host", "dev"}
    assert {(s.variant, s.args["x"] is None) for s in steps if s.op == "dot"} == \
        {("host", True), ("host", False), ("dev", True), ("dev", False)}
    caps = [(s.args["cap"], int(s.expect[0][-1])) for s in steps if s.variant == "dev_cap"]
    assert any(c < nnz for c, nnz in caps) or len(caps) < 2
    assert 40 <= len(steps) <= 75
    assert steps[-2].op == "sync" and steps[-1].op == "getrows" and steps[-1].variant == "host"
    np.testing.assert_array_equal(steps[-1].args["rows"], np.arange(seq.start, seq.start + seq.size))
    assert_bits(steps[-1].expect, seq.final)
    # host/device alternation
    behind_dev = {b.op for a, b in zip(steps, steps[1:]) if a.dev and b.host}
    behind_host = {b.op for a, b in zip(steps, steps[1:]) if a.host and b.dev}
    assert behind_dev >= set(S.FAMILIES) and behind_host >= set(S.FAMILIES)
    # errors: one call at most per sync window, reported by that window's sync and no other
    windows, pending, outside = 0, None, set()
    for s in steps:
        if s.bad is not None:
            assert pending is None and s.dev and s.op in S.ERROR_FAMILIES
            bad_rows = s.args["rows"][(s.args["rows"] < seq.start) | (s.args["rows"] >= seq.start + seq.size)]
            assert set(bad_rows) == {seq.start - 1, seq.start + seq.size}
            assert s.bad == int(np.flatnonzero(np.isin(s.args["rows"], bad_rows))[0])
            pending, windows = s.bad, windows + 1
        elif s.op != "sync" and "rows" in s.args:
            assert ((s.args["rows"] >= seq.start) & (s.args["rows"] < seq.start + seq.size)).all()
        if s.op == "sync":
            assert s.expect == pending
            pending = None
    assert windows >= 2 and pending is None
    # the scratch grows in mid-stream: behind an unsynced device sparse or top-k pull, a row push that
    # needs more than the first allocation, which is all that any earlier user needed
    g = seq.growth
    assert steps[g - 1].op in ("sparse", "topk") and steps[g - 1].dev and steps[g].op == "rows" and steps[g].dev
    assert S.rows_scratch_bytes(steps[g].args["rows"].size) > S.SCRATCH_FLOOR
    for s in steps[:g]:
        kind = S.scratch_kind(s)
        assert kind in (None, "rows", "sparse") and s.args["rows"].size * 24 + 4096 < S.SCRATCH_FLOOR
    assert "sync" in fam[g + 1:g + 3] and steps[g - 1].expect is not None
    if seq.dtype == "float" and regime == "grid":
        assert np.abs(steps[g].args["values"]).max() <= 3
    # a deterministic element push with repeated keys that is too long for the one-launch fold
    for s in steps:
        if S.scratch_kind(s) == "det":
            key = s.args["rows"] * seq.cols + s.args["cols"]
            assert np.unique(key).size < key.size
    # the value caps (asserted step by step while generating; the largest sum met is kept)
    if regime == "grid" and seq.dtype in LIMIT:
        assert 0 < seq.mag_max <= LIMIT[seq.dtype]
        for s in steps:
            for name in ("vals", "values", "coef", "x"):
                v = s.args.get(name)
                if v is not None:
                    assert (v != 0).all() and (v == np.rint(v)).all()


@pytest.mark.parametrize("geometry,dtype,regime", GRID + STRICT, ids=lambda p: str(p).replace(" ", ""))
def test_sequence_conditions(geometry, dtype, regime):
    pairs = set()
    for seed in S.SEEDS:
        seq = S.sequence(*geometry, dtype, regime, seed)
        check_conditions(seq, regime)
        pairs |= S.scratch_pairs(seq.steps)
        assert_bits(oracle_table(seq), seq.final, seq.what)
        assert_bits(run_on(StandIn, seq).to_numpy(), seq.final)
    assert pairs >= {(a, b) for a in S.KINDS for b in S.KINDS}, sorted({(a, b) for a in S.KINDS for b in S.KINDS} - pairs)


def slab_sequences():
    """The sequences of test_gpu_sequence.test_sequence_on_slab_views: one per 16-row view."""
    return [S.sequence(16, 17, "double", "grid", j, start=16 * j, short=True) for j in range(4)]


def test_short_sequences():
    for seq in slab_sequences():
        fam = [s.op for s in seq.steps]
        assert set(fam) >= {"rows", "axpy", "sparse", "sum", "dot", "topk", "getrows", "sync"}
        assert sum(s.bad is not None for s in seq.steps) == 2 and 0 < seq.mag_max <= LIMIT["double"]
        assert any(s.op == "topk" and s.args["k"] > seq.size and (s.expect[0] == -1).any() for s in seq.steps)
        assert_bits(oracle_table(seq), seq.final, seq.what)
        run_on(StandIn, seq)


# ---- the runner fails where it should -------------------------------------------------------------------
def failing_step(cls, seq):
    with pytest.raises(AssertionError) as ei:
        run_on(cls, seq)
    msg = str(ei.value)
    assert seq.what in msg
    i = int(re.search(r" step (\d+): ", msg).group(1))
    assert seq.steps[i].describe() in msg
    return i


@pytest.mark.parametrize("dtype,regime", [("long", "grid"), ("float", "grid"), ("double", "strict")])
def test_runner_catches_broken_shards(dtype, regime):
    seqs = [S.sequence(255, 3, dtype, regime, seed) for seed in S.SEEDS]
    # 1. a row push that loses its last record behind a top-k pull: some later answer names it
    hit = 0
    for seq in seqs:
        users = [(i, S.scratch_kind(s)) for i, s in enumerate(seq.steps) if S.scratch_kind(s)]
        first = next((j for (_, a), (j, b) in zip(users, users[1:]) if (a, b) == ("topk", "rows")), None)
        if first is not None:
            hit += 1
            assert first < failing_step(DropsAfterTopK, seq) < len(seq.steps)
    assert hit
    for seq in seqs:
        # 2. a stale sparse pull: the pull itself is named
        stale = next(i for i, (a, b) in enumerate(zip(seq.steps, seq.steps[1:]), 1)
                     if a.op == "push" and a.dev and b.op == "sparse")
        assert failing_step(StaleSparse, seq) == stale
        # 3. an error reported one sync late: the sync that should have reported it is named
        late = next(i for i, s in enumerate(seq.steps) if s.op == "sync" and s.expect is not None)
        assert failing_step(LateError, seq) == late
