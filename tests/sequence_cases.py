"""Sequences of shard operations on one PartialMatrix: generator, host model and runner, shared by
test_sequence_cpu.py and test_gpu_sequence.py.

Nothing here calls the code under test to get an expected value. The model is a numpy table in the
shard's dtype, moved by the replays the single-operation tests already use (np.add.at -- unbuffered, in
index order, so the sequential loop --, axpy_cases.replay_contrib, rowsum_cases.replay_groups,
dot_cases.replay_dot / replay_self, topk_cases' order over the scores of `table_scores` -- expected_topk's
answer, test_sequence_cpu.py holds them equal -- and the `!= 0` CSR of test_gpu_sparse.py).
Every pull's answer is computed when its step is generated, from the table as it stands then.

A sequence is a pure function of (size, cols, dtype, regime, seed, start): a failure message carries
those, the step's index and its description, and `sequence(...)` rebuilds it.

Regimes. ``grid``: every push mode. Int/Long values lie anywhere in the type (sums wrap: exact in any
order). Float/Double values are non-zero integers, and the generator tracks per element the sum of the
magnitudes pushed so far; it asserts that this sum, every group sum's and every dot product's sum of
magnitudes stay within ieee_cases.LIMIT (2^24 / 2^53), so every partial sum in every order is exact and
a bit-for-bit comparison holds whatever order a kernel adds in (no zero input, so no -0 arises).
``strict``: Float/Double values of mixed magnitude, 10 ** U(-6, 6); only the order-preserving modes
(host-pointer calls of message size, device calls with deterministic=True); the model is the sequential
fold.

Layout of a full sequence (`Gen.full`):
  prologue   a host row push; an unsynced device element push; a device sparse pull of the rows it
             touched (a stale answer shows); directly behind it, unsynced, a device row push of
             GROW_RECORDS records, whose 24 B per record exceed the 1 MiB the scratch holds until then:
             the scratch is freed and reallocated with the sparse pull's launches in the stream; a sync;
             a host sparse pull (a scratch user outside the six kinds, kept out of the walk);
  walk       the scratch users of WALKS[seed % 2] -- the two halves of an Euler circuit through all 36
             ordered pairs of the six kinds -- with one filler that uses no scratch behind each;
  chain      for every family a device call, then the host call directly behind it, so that every family
             is a host-pointer call behind an unsynced device call and a device call behind a host call;
             in three sync windows, each with one device call that names START - 1 and START + size;
  epilogue   a sync, a full getRows; the runner ends with to_numpy().
"""
import zlib

import numpy as np

from axpy_cases import assert_bits, replay_contrib
from dot_cases import lane_width, replay_dot, replay_self
from ieee_cases import LIMIT
from rowsum_cases import replay_groups
from topk_cases import global_rows, topk_of_score_table, topk_of_scores

START = 1_000_003
TOPK_TILE = 4096         # GLINT_TOPK_TILE (test_sequence_cpu.py pins it to the binding's)
ORDERED_MAX = 1 << 17    # kOrderedMax (glint_push_plan.h): a longer deterministic Float/Double push sorts
SCRATCH_FLOOR = 1 << 20  # the scratch's first allocation (glint_host.h, grow)
GROW_RECORDS = 50_000    # x 24 B per record of a row push > SCRATCH_FLOOR
NPD = {"double": np.float64, "float": np.float32, "long": np.int64, "int": np.int32}
GEOMETRIES = [(255, 3), (256, 4), (TOPK_TILE + 1, 67), (65_537, 2)]
SEEDS = (0, 1)
KINDS = ("det", "rows", "axpy", "sparse", "topk", "hostred")  # the six kinds of scratch user
FAMILIES = ("push", "rows", "axpy", "get", "getrows", "sparse", "sum", "dot", "topk")
ERROR_FAMILIES = ("rows", "axpy", "getrows", "sparse", "sum", "dot")  # skipped / zeros, lowest index at the sync


def euler_circuit(k=len(KINDS)):
    """A closed walk over k nodes that takes every ordered pair (u, v), u == v included, exactly once."""
    adj = {u: list(range(k)) for u in range(k)}
    stack, out = [0], []
    while stack:
        u = stack[-1]
        if adj[u]:
            stack.append(adj[u].pop())
        else:
            out.append(stack.pop())
    return out[::-1]


_CIRCUIT = euler_circuit()
_HALF = (len(_CIRCUIT) - 1) // 2
WALKS = (_CIRCUIT[:_HALF + 1], _CIRCUIT[_HALF:])  # 19 nodes each; together every one of the 36 edges


def to_csr(dense):
    mask = dense != 0
    indptr = np.zeros(dense.shape[0] + 1, np.int64)
    np.cumsum(mask.sum(axis=1), out=indptr[1:])
    return indptr, np.nonzero(mask)[1].astype(np.int32), dense[mask]


def table_scores(table, x):
    """topk_cases.scores_of(table, x) -- dot_cases.replay_dot over every row -- computed on the lanes that
    own a column only, rounded up to a power of two P: (n, q) for x (q, cols). The same bits: a lane sum
    starts from +0, so it is never -0, the lanes without a column hold +0, and the butterfly's steps
    d >= P add to each of the first P lanes only such zeros, which changes no bit; the steps d < P are
    the butterfly over P lanes. 65 537 rows of two columns then cost 2 lanes, not 64
    (test_sequence_cpu.py pins the equality)."""
    table, x = np.asarray(table), np.asarray(x, dtype=table.dtype).reshape(-1, table.shape[1])
    dt, cols = table.dtype, table.shape[1]
    E = lane_width(dt, cols)
    P = 1
    while P < min(64, -(-cols // E)):
        P *= 2
    lane = np.arange(P)
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        prod = np.multiply(table[:, None, :], x[None, :, :], dtype=dt)
        acc = np.zeros(prod.shape[:-1] + (P,), dt)
        for s in range(0, cols, 64 * E):
            for e in range(E):
                c = s + lane * E + e
                k = int((c < cols).sum())
                acc[..., :k] = np.add(acc[..., :k], prod[..., c[:k]], dtype=dt)
        d = P // 2
        while d:
            acc = np.add(acc, acc[..., lane ^ d], dtype=dt)
            d //= 2
    return np.ascontiguousarray(acc[..., 0])


def rows_scratch_bytes(n):
    """What a row or axpy push of n records needs of the scratch (rows_front, glint_rows.hip)."""
    pad = lambda b: (b + 255) & ~255  # noqa: E731
    ntiles = (n + 2047) // 2048
    return 4 * pad(n * 4) + pad(n * 8) + 2 * pad(ntiles * 1024) + 1024 + 256


# ---- the model --------------------------------------------------------------------------------------------
class Model:
    """The shard as a numpy table (size, cols) in its dtype. A device-resident call skips a row outside
    the partition (a push) or answers it with zeros (a pull) and returns the lowest such index."""

    def __init__(self, size, cols, npd, start=START):
        self.size, self.cols, self.npd, self.start = int(size), int(cols), np.dtype(npd).type, int(start)
        self.table = np.zeros((self.size, self.cols), self.npd)

    def local(self, rows):
        l = np.asarray(rows, np.int64).reshape(-1) - self.start
        return l, (l >= 0) & (l < self.size)

    @staticmethod
    def lowest_bad(ok):
        bad = np.flatnonzero(~ok)
        return int(bad[0]) if bad.size else None

    def push(self, rows, cols, vals):
        l, ok = self.local(rows)
        assert ok.all()
        with np.errstate(over="ignore", invalid="ignore"):
            np.add.at(self.table, (l, np.asarray(cols, np.int64)), np.asarray(vals, self.npd))

    def push_rows(self, rows, values):
        l, ok = self.local(rows)
        values = np.asarray(values, self.npd).reshape(-1, self.cols)
        with np.errstate(over="ignore", invalid="ignore"):
            np.add.at(self.table, l[ok], values[ok])
        return self.lowest_bad(ok)

    def push_axpy(self, rows, coef, x):
        return self.push_rows(rows, replay_contrib(coef, np.asarray(x, self.npd)))

    def get(self, rows, cols):
        l, ok = self.local(rows)
        assert ok.all()
        return self.table[l, np.asarray(cols, np.int64)]

    def _extended(self, rows):
        """(the table with a row of zeros behind it, local rows with `size` for a row outside, lowest bad)."""
        l, ok = self.local(rows)
        ext = np.vstack([self.table, np.zeros((1, self.cols), self.npd)])
        return ext, np.where(ok, l, self.size), self.lowest_bad(ok)

    def get_rows(self, rows):
        ext, l, bad = self._extended(rows)
        return ext[l], bad

    def sparse(self, rows):
        dense, bad = self.get_rows(rows)
        return to_csr(dense), bad

    def sum(self, rows, offsets):
        ext, l, bad = self._extended(rows)
        return replay_groups(ext, l, np.asarray(offsets, np.int64)), bad

    def dot(self, rows, x=None):
        dense, bad = self.get_rows(rows)
        return (replay_self(dense) if x is None else replay_dot(dense, np.asarray(x, self.npd))), bad

    def topk(self, x, k):
        """topk_cases.expected_topk(table, x, k, first_row=start), with the scores from table_scores."""
        x = np.asarray(x, self.npd)
        sc = table_scores(self.table, x)
        rows = global_rows(self.size, self.start)
        return topk_of_scores(np.ascontiguousarray(sc[:, 0]), rows, k) if x.ndim == 1 else topk_of_score_table(sc, rows, k)


# ---- steps --------------------------------------------------------------------------------------------------
class Step:
    """One call. `variant`: host, dev, dev_unordered, dev_det, dev_cap or async; `expect` the answer of a
    pull, or of a sync the index it reports (None: no error); `bad` the lowest index outside the
    partition that this device-resident call names."""

    def __init__(self, op, variant="", args=None, expect=None, bad=None):
        self.op, self.variant, self.args, self.expect, self.bad = op, variant, args or {}, expect, bad

    @property
    def dev(self):
        return self.variant.startswith("dev")

    @property
    def host(self):
        return self.variant in ("host", "async")

    def describe(self):
        a = self.args
        parts = [f"{self.op}/{self.variant}" if self.variant else self.op]
        for key in ("rows", "x"):
            if a.get(key) is not None:
                parts.append(f"{key}{tuple(np.shape(a[key]))}")
        for key in ("k", "cap"):
            if a.get(key) is not None:
                parts.append(f"{key}={a[key]}")
        if self.op == "dot" and a.get("x") is None:
            parts.append("self")
        if self.bad is not None:
            parts.append(f"lowest row outside at {self.bad}")
        if self.op == "sync":
            parts.append(f"reports {self.expect}")
        return " ".join(parts)


def scratch_kind(step):
    """The kind of scratch user a step is: one of KINDS, "other" (the host sparse pull's answer), or None."""
    if step.op == "push":
        return "det" if step.variant == "dev_det" and step.args["rows"].size > ORDERED_MAX else None
    if step.op in ("rows", "axpy", "topk"):
        return step.op
    if step.op == "sparse":
        return "sparse" if step.dev else "other"
    if step.op in ("sum", "dot"):
        return "hostred" if step.host else None
    return None


def scratch_pairs(steps):
    """The ordered pairs of kinds that follow each other with no other scratch user between them."""
    users = [k for k in map(scratch_kind, steps) if k is not None]
    return {(a, b) for a, b in zip(users, users[1:]) if a != "other" and b != "other"}


class Sequence:
    def __init__(self, what, steps, final, size, cols, dtype, start, growth, mag_max):
        self.what, self.steps, self.final = what, steps, final
        self.size, self.cols, self.dtype, self.start = size, cols, dtype, start
        self.growth = growth    # index of the step that outgrows the scratch (None in a short sequence)
        self.mag_max = mag_max  # grid Float/Double: the largest sum of magnitudes met (else 0)


# ---- the generator ---------------------------------------------------------------------------------------
class Gen:
    def __init__(self, size, cols, dtype, regime, seed, start=START):
        assert regime in ("grid", "strict") and (regime == "grid" or dtype in ("double", "float"))
        self.size, self.cols, self.dtype, self.regime, self.seed, self.start = size, cols, dtype, regime, seed, start
        self.what = f"size={size} cols={cols} dtype={dtype} regime={regime} seed={seed} start={start}"
        self.rng = np.random.default_rng(zlib.crc32(f"sequence/{self.what}".encode()))
        self.npd = NPD[dtype]
        self.fp = np.issubdtype(self.npd, np.floating)
        self.m = Model(size, cols, self.npd, start)
        self.exact = self.fp and regime == "grid"
        self.mag = np.zeros((size, cols)) if self.exact else None  # per element: sum of |v| pushed so far
        self.limit = float(LIMIT[dtype]) if self.exact else None
        self.mag_max = 0.0
        self.steps, self.pending_bad, self.open_tickets, self.growth = [], None, 0, None
        self.hot = self.rng.choice(size, min(size, 48), replace=False)
        self.turn, self.only_hot = {}, False

    # -- helpers
    def cycle(self, name, options):
        i = self.turn.get(name, 0)
        self.turn[name] = i + 1
        return options[i % len(options)]

    def variant(self, v):
        """strict: only the order-preserving device mode."""
        return "dev_det" if self.regime == "strict" and v in ("dev", "dev_unordered") else v

    def values(self, shape, hi=3):
        rng = self.rng
        if not self.fp:
            info = np.iinfo(self.npd)
            return rng.integers(info.min, info.max, shape, dtype=self.npd, endpoint=True)
        if self.regime == "grid":  # non-zero integers
            return (rng.integers(1, hi + 1, shape) * rng.choice((-1, 1), shape)).astype(self.npd)
        return (rng.choice((-1.0, 1.0), shape) * 10.0 ** rng.uniform(-6, 6, shape)).astype(self.npd)

    def some_rows(self, n, uniform=False):
        """Global rows: uniform, or half of them from 48 hot rows (repeats at every size)."""
        n = int(n)
        l = self.rng.integers(0, self.size, n)
        if self.only_hot:
            l = self.rng.choice(self.hot, n)
        elif not uniform:
            l = np.where(self.rng.random(n) < 0.5, self.rng.choice(self.hot, n), l)
        return l.astype(np.int64) + self.start

    def bound(self, m):
        """grid Float/Double: a sum of magnitudes, which must stay within the format's exact integers."""
        m = float(np.max(m, initial=0.0))
        assert m <= self.limit, f"{self.what}: sum of magnitudes {m} above {self.limit}"
        self.mag_max = max(self.mag_max, m)

    def outside(self, rows):
        """Puts START - 1 and START + size at two places of `rows`; returns the lower index."""
        i, j = self.rng.choice(rows.size, 2, replace=False)
        rows[i], rows[j] = self.start - 1, self.start + self.size
        return int(min(i, j))

    def emit(self, op, variant, args, expect=None, bad=None):
        for a in args.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        if bad is not None:
            assert variant.startswith("dev") and op in ERROR_FAMILIES and self.pending_bad is None
            self.pending_bad = bad
        self.steps.append(Step(op, variant, args, expect, bad))

    def ext_mag(self, rows):
        l, ok = self.m.local(rows)
        return np.vstack([self.mag, np.zeros((1, self.cols))])[np.where(ok, l, self.size)]

    # -- operations
    def push(self, variant, n, hi=3, uniform=False):
        variant = self.variant(variant)
        rows = self.some_rows(n, uniform)
        cols = self.rng.integers(0, self.cols, rows.size).astype(np.int32)
        vals = self.values(rows.size, hi)
        self.m.push(rows, cols, vals)
        if self.exact:
            np.add.at(self.mag, (rows - self.start, cols.astype(np.int64)), np.abs(vals).astype(np.float64))
            self.bound(self.mag)
        if variant == "async":
            self.open_tickets += 1
        self.emit("push", variant, {"rows": rows, "cols": cols, "vals": vals})

    def rows(self, variant, n, hi=3, bad=False, uniform=False):
        variant = self.variant(variant)
        rows = self.some_rows(n, uniform)
        values = self.values((rows.size, self.cols), hi)
        low = self.outside(rows) if bad else None
        assert self.m.push_rows(rows, values) == low
        if self.exact:
            l, ok = self.m.local(rows)
            np.add.at(self.mag, l[ok], np.abs(values[ok]).astype(np.float64))
            self.bound(self.mag)
        self.emit("rows", variant, {"rows": rows, "values": values}, bad=low)

    def axpy(self, variant, n, q, bad=False):
        variant = self.variant(variant)
        rows = self.some_rows(n)
        coef, x = self.values((rows.size, q), 2), self.values((q, self.cols), 2)
        if q == 1 and self.cycle("axpy_flat", (True, False)):
            coef, x = coef.reshape(-1), x.reshape(-1)  # the (n,) / (cols,) form
        low = self.outside(rows) if bad else None
        assert self.m.push_axpy(rows, coef, x) == low
        if self.exact:
            l, ok = self.m.local(rows)
            t = np.abs(coef.reshape(rows.size, -1)).astype(np.float64) @ np.abs(x.reshape(-1, self.cols)).astype(np.float64)
            np.add.at(self.mag, l[ok], t[ok])
            self.bound(self.mag)
        self.emit("axpy", variant, {"rows": rows, "coef": coef, "x": x}, bad=low)

    def get(self, variant, n):
        rows = self.some_rows(n)
        cols = self.rng.integers(0, self.cols, rows.size).astype(np.int32)
        self.emit("get", variant, {"rows": rows, "cols": cols}, self.m.get(rows, cols))

    def getrows(self, variant, n=None, bad=False, rows=None):
        rows = self.some_rows(n) if rows is None else rows
        low = self.outside(rows) if bad else None
        exp, got_low = self.m.get_rows(rows)
        assert got_low == low
        if variant == "async":
            self.open_tickets += 1
        self.emit("getrows", variant, {"rows": rows}, exp, bad=low)

    def sparse(self, variant, n=None, bad=False, rows=None):
        rows = self.some_rows(n) if rows is None else rows
        low = self.outside(rows) if bad else None
        exp, got_low = self.m.sparse(rows)
        assert got_low == low
        args = {"rows": rows}
        if variant == "dev_cap":  # below the answer's size, or above it, in turn
            nnz = int(exp[0][-1])
            args["cap"] = max(1, nnz // 2) if self.cycle("cap", (True, False)) else nnz + 5
        self.emit("sparse", variant, args, exp, bad=low)

    def sum(self, variant, n, g, bad=False):
        rows = self.some_rows(n)
        offsets = np.concatenate([[0], np.sort(self.rng.integers(0, rows.size + 1, g - 1)), [rows.size]]).astype(np.int64)
        low = self.outside(rows) if bad else None
        exp, got_low = self.m.sum(rows, offsets)
        assert got_low == low
        if self.exact:
            gm = np.zeros((g, self.cols))
            np.add.at(gm, np.repeat(np.arange(g), np.diff(offsets)), self.ext_mag(rows))
            self.bound(gm)
        self.emit("sum", variant, {"rows": rows, "offsets": offsets}, exp, bad=low)

    def dot(self, variant, n, q, bad=False):
        """q: None the self-dot, 0 one vector as (cols,), else (q, cols)."""
        rows = self.some_rows(n)
        x = None if q is None else self.values(self.cols if q == 0 else (q, self.cols), 3)
        low = self.outside(rows) if bad else None
        exp, got_low = self.m.dot(rows, x)
        assert got_low == low
        if self.exact:
            em = self.ext_mag(rows)
            self.bound((em * em).sum(axis=1) if x is None else em @ np.abs(x.reshape(-1, self.cols)).astype(np.float64).T)
        self.emit("dot", variant, {"rows": rows, "x": x}, exp, bad=low)

    def topk(self, variant, q, k):
        x = self.values(self.cols if q == 0 else (q, self.cols), 3)
        if self.exact:
            self.bound(self.mag @ np.abs(x.reshape(-1, self.cols)).astype(np.float64).T)
        self.emit("topk", variant, {"x": x, "k": int(k)}, self.m.topk(x, k))

    def sync(self):
        self.emit("sync", "", {}, expect=self.pending_bad)
        self.pending_bad = None

    def wait(self):
        if self.open_tickets:
            self.emit("wait", "", {})
            self.open_tickets = 0

    def scratch_user(self, kind):
        n = min(600, 40 * self.size)
        if kind == "det":  # longer than the one-launch ordered fold takes: the sort tail, with repeated keys
            self.push("dev_det", ORDERED_MAX + 1 + int(self.rng.integers(0, 64)), hi=1, uniform=True)
            r, c = self.steps[-1].args["rows"], self.steps[-1].args["cols"]
            assert np.unique(r * self.cols + c).size < r.size
        elif kind == "rows":
            self.rows(self.cycle("rows", ("dev", "host", "dev_det")), n)
        elif kind == "axpy":
            self.axpy(self.cycle("axpy", ("dev_det", "dev", "host")), n, self.cycle("axpy_q", (3, 1, 5, 1)))
        elif kind == "sparse":
            self.sparse(self.cycle("sparse", ("dev", "dev_cap")), n // 2)
        elif kind == "topk":
            self.topk(self.cycle("topk", ("dev", "host")), self.cycle("topk_q", (5, 0, 3)), self.cycle("topk_k", (7, 70)))
        else:
            which = self.cycle("hostred", ("sum", "dot", "self"))
            if which == "sum":
                self.sum("host", n // 2, 9)
            else:
                self.dot("host", n // 2, 3 if which == "dot" else None)

    # -- plans
    def full(self):
        n = 600
        # prologue
        self.rows("host", 400)
        self.push("dev", 700)
        touched = np.unique(self.steps[-1].args["rows"])
        self.sparse(self.cycle("sparse", ("dev", "dev_cap") if self.seed % 2 == 0 else ("dev_cap", "dev")),
                    rows=np.concatenate([touched, self.some_rows(50)]))
        self.growth = len(self.steps)
        self.rows("dev", GROW_RECORDS, uniform=True)  # strict: dev_det
        self.sync()
        self.sparse("host", 300)
        # walk
        fillers = iter([
            lambda: self.push("host", 800), lambda: self.push("dev_unordered", 3000),
            lambda: self.push("async", 1000), lambda: self.get("dev", 500), self.wait,
            lambda: self.getrows("async", 100), lambda: self.dot("dev", 300, 2), self.wait,
            lambda: self.sum("dev", 300, 11), lambda: self.push("dev", 5000), lambda: self.getrows("dev", 200),
            lambda: self.dot("dev", 300, None), lambda: self.get("host", 500), lambda: self.push("dev_det", 2000),
            lambda: self.get("dev", 100),
        ])
        for j, kind in enumerate(WALKS[self.seed % 2]):
            self.scratch_user(KINDS[kind])
            f = next(fillers, None)
            if f is not None:
                f()
            if j % 5 == 4:
                self.sync()
        self.wait()
        # a walk holds each kind three times or so: the variants its turns did not reach
        have = {(s.op, s.variant, s.op == "dot" and s.args["x"] is None) for s in self.steps}
        for v in ("host", "dev", "dev_det"):
            if ("rows", self.variant(v), False) not in have:
                self.rows(v, n)
            if ("axpy", self.variant(v), False) not in have:
                self.axpy(v, n, 4)
        if ("sparse", "dev_cap", False) not in have:
            self.sparse("dev_cap", n // 2)
        if ("dot", "host", True) not in have:
            self.dot("host", n // 2, None)
        self.sync()
        self.chain(n)
        # epilogue
        self.sync()
        self.getrows("host", rows=np.arange(self.start, self.start + self.size, dtype=np.int64))
        return self.done()

    def chain(self, n):
        """Every family as a device call and, directly behind it, as a host-pointer call; three sync
        windows with one call each that names rows outside the partition."""
        windows = (("push", "rows", "axpy"), ("get", "getrows", "sparse"), ("sum", "dot", "topk"))
        for w, fams in enumerate(windows):
            if w:
                self.get("host", 50)  # the window's first device call stands directly behind a host call
            culprit = self.rng.choice([f for f in fams if f in ERROR_FAMILIES])
            for fam in fams:
                for variant in ("dev", "host"):
                    bad = variant == "dev" and fam == culprit
                    if fam == "push":
                        self.push(variant, n)
                    elif fam == "rows":
                        self.rows(variant, n, bad=bad)
                    elif fam == "axpy":
                        self.axpy(variant, n, 2, bad=bad)
                    elif fam == "get":
                        self.get(variant, n)
                    elif fam == "getrows":
                        self.getrows(variant, n // 2, bad=bad)
                    elif fam == "sparse":
                        self.sparse(variant, n // 2, bad=bad)
                    elif fam == "sum":
                        self.sum(variant, n // 2, 7, bad=bad)
                    elif fam == "dot":
                        self.dot(variant, n // 2, None if variant == "dev" else 0, bad=bad)
                    else:
                        self.topk(variant, 2, 5)
            if w < len(windows) - 1:
                self.sync()

    def short(self):
        """A dozen steps of the row family for a small shard (a slab's view)."""
        n = 4 * self.size
        self.hot, self.only_hot = self.hot[:max(1, self.size * 5 // 8)], True  # the other rows stay untouched
        self.rows("host", n)
        self.axpy("dev", n, 2)
        self.sparse("dev", n // 2)
        self.rows("dev_det", n, bad=True)
        self.sum("host", n, 5)
        self.sync()
        self.topk("dev", 2, self.size + 4)  # more than the view has rows: the -1 fill
        self.axpy("host", n, 1)
        self.dot("dev", n, 3)
        self.sum("dev", n, 4, bad=True)
        self.topk("host", 0, 3)
        self.rows("dev", n)
        self.dot("host", n, None)
        self.sync()
        self.getrows("dev", n)
        self.sync()
        return self.done()

    def done(self):
        assert self.pending_bad is None and not self.open_tickets
        final = self.m.table.copy()
        final.setflags(write=False)
        return Sequence(self.what, self.steps, final, self.size, self.cols, self.dtype, self.start, self.growth,
                        self.mag_max)


def sequence(size, cols, dtype, regime, seed, start=START, short=False):
    g = Gen(size, cols, dtype, regime, seed, start)
    return g.short() if short else g.full()


# ---- the runner ---------------------------------------------------------------------------------------------
def _np(a):
    return a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)


class Runner:
    """Drives a Sequence's steps against `sh`, anything with PartialMatrix's methods. Device-resident
    calls get tensors on `device` and sync=False; their answers are compared after the next sync step,
    and every tensor handed in or out stays alive until then. A failure names the sequence and the step."""

    def __init__(self, sh, seq, device, out_of_range):
        import torch
        self.torch, self.sh, self.seq, self.device, self.oor = torch, sh, seq, device, out_of_range
        self.stream = torch.cuda.current_stream(device).cuda_stream if device.type == "cuda" else None
        self.alive, self.unchecked, self.tickets, self.at = [], [], [], 0

    def t(self, a):
        if a is None:
            return None
        x = self.torch.from_numpy(np.array(a)).to(self.device)
        self.alive.append(x)
        return x

    def fail(self, i, msg):
        raise AssertionError(f"{self.seq.what} step {i}: {self.seq.steps[i].describe()}: {str(msg).strip()}")

    def compare(self, i, got, exp):
        try:
            if self.seq.steps[i].op == "sparse":
                (ip, c, v), (eip, ec, ev) = got, exp
                keep = min(int(eip[-1]), self.seq.steps[i].args.get("cap", int(eip[-1])))
                assert_bits(_np(ip), eip, "indptr")
                assert_bits(_np(c)[:keep], ec[:keep], "cols")
                assert_bits(_np(v)[:keep], ev[:keep], "values")
                assert self.seq.steps[i].args.get("cap") is not None or _np(c).size == keep == _np(v).size
            elif self.seq.steps[i].op == "topk":
                assert_bits(_np(got[0]), exp[0], "rows")
                assert_bits(_np(got[1]), exp[1], "values")
            else:
                assert_bits(_np(got), exp)
        except AssertionError as e:
            self.fail(i, e)

    def run(self):
        while self.at < len(self.seq.steps):
            self.step()
        self.finish()

    def step(self):
        i, s, sh, t = self.at, self.seq.steps[self.at], self.sh, self.t
        self.at += 1
        a, dev = s.args, s.dev
        later = lambda got: self.unchecked.append((i, got, s.expect))  # noqa: E731
        try:
            if s.op == "push":
                if s.variant == "async":
                    self.tickets.append((sh.push_async(a["rows"], a["cols"], a["vals"]), None, None))
                elif dev:
                    sh.update(t(a["rows"]), t(a["cols"]), t(a["vals"]), deterministic=s.variant == "dev_det",
                              unordered=s.variant == "dev_unordered", sync=False)
                else:
                    sh.update(a["rows"], a["cols"], a["vals"])
            elif s.op == "rows":
                if dev:
                    sh.updateRows(t(a["rows"]), t(a["values"]), deterministic=s.variant == "dev_det", sync=False)
                else:
                    sh.updateRows(a["rows"], a["values"])
            elif s.op == "axpy":
                if dev:
                    sh.updateRowsAxpy(t(a["rows"]), t(a["coef"]), t(a["x"]), deterministic=s.variant == "dev_det",
                                      sync=False)
                else:
                    sh.updateRowsAxpy(a["rows"], a["coef"], a["x"])
            elif s.op == "get":
                if dev:
                    later(sh.get(t(a["rows"]), t(a["cols"]), sync=False))
                else:
                    self.compare(i, sh.get(a["rows"], a["cols"]), s.expect)
            elif s.op == "getrows":
                if s.variant == "async":
                    ticket, out = sh.pull_async(a["rows"], rows=True)
                    self.tickets.append((ticket, i, out))
                elif dev:
                    later(sh.getRows(t(a["rows"]), sync=False))
                else:
                    self.compare(i, sh.getRows(a["rows"]), s.expect)
            elif s.op == "sparse":
                if dev:
                    later(sh.getRowsSparse(t(a["rows"]), cap=a.get("cap"), sync=False))
                else:
                    self.compare(i, sh.getRowsSparse(a["rows"]), s.expect)
            elif s.op == "sum":
                if dev:
                    later(sh.getRowsSum(t(a["rows"]), t(a["offsets"]), sync=False))
                else:
                    self.compare(i, sh.getRowsSum(a["rows"], a["offsets"]), s.expect)
            elif s.op == "dot":
                if dev:
                    later(sh.getRowsDot(t(a["rows"]), t(a["x"]), sync=False))
                else:
                    self.compare(i, sh.getRowsDot(a["rows"], a["x"]), s.expect)
            elif s.op == "topk":
                if dev:
                    later(sh.getTopK(t(a["x"]), a["k"], sync=False))
                else:
                    self.compare(i, sh.getTopK(a["x"], a["k"]), s.expect)
            elif s.op == "wait":
                for ticket, j, out in self.tickets:
                    sh.wait(ticket)
                    if j is not None:
                        self.compare(j, out, self.seq.steps[j].expect)
                self.tickets = []
            elif s.op == "sync":
                reported = None
                try:
                    sh.sync(self.stream)
                except self.oor as e:
                    reported = e.record
                if reported != s.expect:
                    self.fail(i, f"the sync reported {reported}, expected {s.expect}")
                for j, got, exp in self.unchecked:
                    self.compare(j, got, exp)
                self.unchecked, self.alive = [], []
            else:
                raise ValueError(s.op)
        except self.oor as e:
            self.fail(i, f"unexpected {type(e).__name__}: {e}")

    def finish(self):
        last = len(self.seq.steps) - 1
        assert self.at == last + 1 and not self.unchecked and not self.tickets
        try:
            assert_bits(self.sh.to_numpy(), self.seq.final, "to_numpy()")
        except AssertionError as e:
            self.fail(last, f"after the last step: {e}")


def run(sh, seq, device, out_of_range):
    Runner(sh, seq, device, out_of_range).run()
