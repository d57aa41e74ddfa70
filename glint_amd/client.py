"""In-process client over HBM shards: the exchange step in front of the shard kernels.

Mirrors the reference's client factory and asynchronous models, minus the Akka transport:

* ``Client.vector`` / ``Client.matrix`` -- glint.Client.vector/matrix/create
  (src/main/scala/glint/Client.scala:53-94, 105-196): P = min(keys, modelsPerServer x servers)
  partitions, partition i placed on "server" (here: GPU) i % servers.
* ``BigVector.push/pull`` -- AsyncBigVector.push/pull (AsyncBigVector.scala:49-121): records are
  bucketed by partition preserving their order inside each bucket (``mapPartitions``, :96-98),
  one shard call per partition, and pulled values scattered back to the caller's order (:61-79).
* ``BigMatrix.push/pull`` -- AsyncBigMatrix (AsyncBigMatrix.scala:53-170), including the row pull.
* ``BigMatrix.pushRows`` -- an extension with no AsyncBigMatrix counterpart: the row pull's write
  side, whole rows added without expanding them into (row, col, value) triplets.
* ``BigMatrix.pullRowsAs`` / ``BigMatrix.pushRowsAs`` -- extensions: the row pull and the row push with the
  rows crossing the link as float16 or bfloat16 (Float) or float32 (Double), rounded / widened on the shards
  (PartialMatrix.getRowsAs / updateRowsAs).
* ``BigMatrix.pushAxpy`` -- an extension: rows += coefficients times caller vectors, the contribution
  rows rebuilt on the shards (PartialMatrix.updateRowsAxpy) instead of sent.
* ``BigMatrix.pushAdagrad`` -- an extension: gradient rows summed per distinct row, then one Adagrad step
  of this matrix and of a second one that holds the accumulators, on the shards
  (PartialMatrix.updateRowsAdagrad).
* ``BigMatrix.pushAdagradRowwise`` -- an extension: row-wise Adagrad, one accumulator per row held in a
  ``BigVector`` with this matrix's partitioner (PartialMatrix.updateRowsAdagradRowwise).
* ``BigMatrix.pushAdam`` -- an extension: the same with one lazy Adam step, the second matrix holding both
  moments of a row side by side in ``2 * cols`` columns (PartialMatrix.updateRowsAdam).
* ``BigMatrix.pushFtrl`` -- an extension: the same with one FTRL-proximal step, the second matrix holding
  ``z`` and ``n`` of a row side by side; with ``l1 > 0`` most weights become exact zeros, which
  ``pullSparse`` then leaves out (PartialMatrix.updateRowsFtrl).
* ``BigMatrix.pullSum`` -- an extension: the sums of groups of rows, reduced on the shards
  (PartialMatrix.getRowsSum) and combined per group in partition-index order.
* ``BigMatrix.pullDot`` -- an extension: the dot products of rows with caller vectors (or with
  themselves), reduced over the columns on the shards (PartialMatrix.getRowsDot); a row lives in one
  partition, so the answers are only scattered back.
* ``BigMatrix.pullTopK`` -- an extension: the rows that score highest against caller vectors, selected on
  the shards (PartialMatrix.getTopK) and merged here, at most ``parts * k`` pairs per query.
* ``BigMatrix.pullPairDot`` / ``BigMatrix.pushPairAxpy`` -- extensions: the two halves of a two-table
  scoring step, rows of this matrix dotted with, or stepped by coefficients times, rows of a second
  matrix on the same devices (PartialMatrix.getPairsDot / updatePairsAxpy); pairs are bucketed by (own
  partition, other partition) and nothing of size ``cols`` leaves the devices.
* ``fill`` / ``initUniform`` of both models -- extensions: a constant, or a seeded uniform table whose
  bits do not depend on the layout, written on the shards (``fill`` / ``initUniform`` of the shards).

Out-of-range keys raise ``IndexOutOfBoundsException`` before any shard is touched, as the
reference's ``partitioner.partition`` does synchronously inside ``mapPartitions``.
"""
from __future__ import annotations

from typing import Callable, List, Optional, Sequence

import numpy as np

from .errors import ModelCreationException
from .partitioning import CyclicPartitioner, RangePartitioner
from .shard import PartialMatrix, PartialVector, resolve_dtype, resolve_wire


def bucket(owner: np.ndarray, nparts: int):
    """Stable grouping of record indices by owning partition (AsyncBigVector.scala:96-98).
    Returns (order, offsets): records of partition p are order[offsets[p]:offsets[p+1]], in the
    caller's order."""
    order = np.argsort(owner, kind="stable")
    counts = np.bincount(owner, minlength=nparts)
    offsets = np.zeros(nparts + 1, dtype=np.int64)
    np.cumsum(counts, out=offsets[1:])
    return order, offsets


def _buckets(model, keys) -> list:
    """The fan-out every call of both models makes: ``[(p, shard, idx)]`` for the non-empty partitions of
    ``keys`` (global keys) in ascending p, ``idx`` the positions of partition p's keys in the caller's order.
    The partitioner validates every key first, so a key outside the model raises before any shard is called."""
    order, off = bucket(model.partitioner.partition_indices(keys), len(model.shards))
    return [(p, sh, order[off[p]:off[p + 1]]) for p, sh in enumerate(model.shards) if off[p + 1] > off[p]]


def _same_partitioner(a, b) -> bool:
    """Whether two partitioners lay the same key space out the same way: one kind, the same partitions."""
    return type(a) is type(b) and [repr(p) for p in a.all()] == [repr(p) for p in b.all()]


_TWICE_COLS = "state: expected a matrix with this one's partitioner, rows and dtype and twice its cols"


def _init_fanout(model, rows, call) -> bool:
    """What ``fill`` and ``initUniform`` of both models do: ``rows`` None reaches every shard once,
    ``call(shard, None)``; else the rows (global keys) are validated by the partitioner before any shard is
    called, and each non-empty partition gets one ``call(shard, its rows)`` in the caller's order."""
    if rows is None:
        for sh in model.shards:
            call(sh, None)
        return True
    rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
    for _, sh, idx in _buckets(model, rows):
        call(sh, rows[idx])
    return True


class _InitMixin:
    def fill(self, value, rows=None) -> bool:
        """Every element of the named rows (vector: keys) = ``value``, written on the shards (an extension;
        ``PartialVector.fill`` / ``PartialMatrix.fill``): an Adagrad accumulator's initial value. ``rows``
        None: the whole model, one call per shard. Else global keys, validated before any shard is called
        and bucketed by partition as ``push``; one call per non-empty partition."""
        return _init_fanout(self, rows, lambda sh, r: sh.fill(value, rows=r))

    def initUniform(self, seed: int, lo: float, hi: float, rows=None) -> bool:
        """Seeded uniform init of the named rows in [lo, hi], generated on the shards (an extension;
        ``initUniform`` of the shards; Float and Double). An element's value depends on (seed, global row,
        column, lo, hi, dtype) only, so every shard gets the same seed and the model holds the same bits
        under any partitioner and any number of partitions. ``rows`` as for ``fill``."""
        return _init_fanout(self, rows, lambda sh, r: sh.initUniform(seed, lo, hi, rows=r))


class BigVector(_InitMixin):
    """AsyncBigVector over PartialVector shards (one per partition)."""

    def __init__(self, partitioner, shards: Sequence[PartialVector], size: int):
        self.partitioner = partitioner
        self.shards = list(shards)
        self.size = int(size)

    @property
    def nrOfPartitions(self) -> int:  # AsyncBigVector.scala:126-128
        return len(self.partitioner.all())

    def push(self, keys, values, deterministic: bool = False) -> bool:
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        values = np.ascontiguousarray(values, dtype=self.shards[0].np_dtype)
        for _, sh, idx in _buckets(self, keys):
            sh.update(keys[idx], values[idx], deterministic=deterministic)
        return True

    def pull(self, keys) -> np.ndarray:
        keys = np.ascontiguousarray(keys, dtype=np.int64)
        out = np.zeros(keys.shape, dtype=self.shards[0].np_dtype)
        for _, sh, idx in _buckets(self, keys):
            out[idx] = sh.get(keys[idx])
        return out

    def destroy(self) -> bool:
        for sh in self.shards:
            sh.destroy()
        return True


class BigMatrix(_InitMixin):
    """AsyncBigMatrix over PartialMatrix shards."""

    def __init__(self, partitioner, shards: Sequence[PartialMatrix], rows: int, cols: int):
        self.partitioner = partitioner
        self.shards = list(shards)
        self.rows = int(rows)
        self.cols = int(cols)

    @property
    def nrOfPartitions(self) -> int:
        return len(self.partitioner.all())

    def push(self, rows, cols, values, deterministic: bool = False) -> bool:
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        values = np.ascontiguousarray(values, dtype=self.shards[0].np_dtype)
        for _, sh, idx in _buckets(self, rows):
            sh.update(rows[idx], cols[idx], values[idx], deterministic=deterministic)
        return True

    # what the row calls below validate before any shard is called ----------------------------------------
    def _rows_values(self, rows, values, dtype, name: str = "values") -> tuple:
        """Flat int64 rows and their value rows ((n, cols) or flat, called ``name``) as an (n, cols) array."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        values = np.ascontiguousarray(values, dtype=dtype)
        if values.size != rows.size * self.cols:
            raise ValueError(f"{name}: {values.size} elements, expected {rows.size} rows x {self.cols} columns")
        return rows, values.reshape(rows.size, self.cols)

    @staticmethod
    def _offsets(rows: np.ndarray, offsets) -> tuple:
        """The offsets of a grouped call over flat ``rows`` as (flat int64 array, g)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if offsets.size < 1 or offsets[0] != 0 or offsets[-1] != rows.size or (np.diff(offsets) < 0).any():
            raise ValueError("offsets must be non-decreasing from 0 to len(rows)")
        return offsets, offsets.size - 1

    def _check_queries(self, x: np.ndarray) -> None:
        """Caller vectors: (cols,), or (q, cols) with q >= 1."""
        if x.shape != (self.cols,) and not (x.ndim == 2 and x.shape[1] == self.cols and x.shape[0] >= 1):
            raise ValueError(f"x: shape {x.shape}, expected ({self.cols},) or (q, {self.cols})")

    def pushRows(self, rows, values, deterministic: bool = False) -> bool:
        """Whole rows: row rows[i] += values[i] (an (n, cols) array, or flat), in the caller's order
        -- ``push`` of the triplets (rows[i], c, values[i][c]) without expanding them. Bucketed by
        partition as ``push``; one PartialMatrix.updateRows per non-empty partition."""
        rows, values = self._rows_values(rows, values, self.shards[0].np_dtype)
        for _, sh, idx in _buckets(self, rows):
            sh.updateRows(rows[idx], values[idx], deterministic=deterministic)
        return True

    def pushRowsAs(self, rows, values, wire: str, deterministic: bool = False) -> bool:
        """Narrow-format row push (an extension): ``pushRows`` of rows that arrive in the wire type ``wire``
        ('float16' or 'bfloat16' for a Float matrix, 'float32' for a Double one) and are widened on the
        shards, so half the bytes cross the link. ``values`` is an (n, cols) or flat numpy array of float16,
        of uint16 bfloat16 bit patterns (``to_bfloat16``) or of float32; another dtype raises ValueError.
        All rows are validated before any shard is called; bucketed by partition as ``pushRows``, one
        PartialMatrix.updateRowsAs per non-empty partition."""
        np_wire = resolve_wire(wire)[1]
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        values = np.asarray(values)
        if values.dtype != np_wire:
            raise ValueError(f"values: dtype {values.dtype}, expected {np.dtype(np_wire).name} for wire type {wire!r}")
        rows, values = self._rows_values(rows, values, np_wire)
        for _, sh, idx in _buckets(self, rows):
            sh.updateRowsAs(rows[idx], values[idx], wire, deterministic=deterministic)
        return True

    def pullRowsAs(self, rows, wire: str) -> np.ndarray:
        """Narrow-format row pull (an extension): ``pull(rows)`` rounded on the shards to the wire type
        ``wire``, as an (n, cols) array of float16, of uint16 bfloat16 bit patterns (``from_bfloat16``) or of
        float32, in the caller's order. A row lives in one partition, so the bits are the shard's. Bucketed
        by partition as ``pull``; one PartialMatrix.getRowsAs per non-empty partition."""
        np_wire = resolve_wire(wire)[1]
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        out = np.zeros((rows.size, self.cols), dtype=np_wire)
        for _, sh, idx in _buckets(self, rows):
            out[idx] = sh.getRowsAs(rows[idx], wire)
        return out

    def pushAxpy(self, rows, coef, x, deterministic: bool = False) -> bool:
        """Row axpy push (an extension): row rows[i] += sum over j of ``coef[i, j] * x[j]``, in the
        caller's order -- ``pushRows`` of those contribution rows without building or sending them. ``x``
        is (cols,) or (q, cols), ``coef`` (n,) (only with q == 1) or (n, q). Bucketed by partition as
        ``pushRows``; one PartialMatrix.updateRowsAxpy per non-empty partition, with its rows and
        coefficient rows in the caller's order and the same ``x``."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        dtype = self.shards[0].np_dtype
        x = np.ascontiguousarray(x, dtype=dtype)
        coef = np.ascontiguousarray(coef, dtype=dtype)
        self._check_queries(x)
        q = 1 if x.ndim == 1 else x.shape[0]
        if coef.shape != (rows.size, q) and not (q == 1 and coef.shape == (rows.size,)):
            raise ValueError(f"coef: shape {coef.shape}, expected ({rows.size}, {q})")
        for _, sh, idx in _buckets(self, rows):
            sh.updateRowsAxpy(rows[idx], coef[idx], x, deterministic=deterministic)
        return True

    def pushGroups(self, rows, offsets, values, weights=None, deterministic: bool = False) -> bool:
        """Grouped row push (an extension), the write side of ``pullSum``: ``offsets`` has g + 1 entries,
        non-decreasing from 0 to len(rows); every row of ``rows[offsets[k]:offsets[k+1]]`` += ``values[k]``
        -- times ``weights[i]`` for record i when ``weights`` (n,) is given -- in the caller's order.
        ``values`` is (g, cols) or flat. It is ``pushRows`` of the n expanded rows without building or
        sending them. ``offsets``, the shapes and -- by the partitioner -- every row are validated before
        any shard is called. Records are bucketed by partition as ``pushRows``; each non-empty partition
        gets one PartialMatrix.updateRowsGrouped over the sub-groups of its own rows, in the caller's
        order: only the groups that have a record in that partition are sent, their value rows compacted.
        A row lives in one partition, so a row's additions run in the caller's order under any
        partitioning.

        Bytes sent to a partition with n_p of the records in g_p of the groups: ``8 n_p + 8 (g_p + 1) +
        g_p * cols * itemsize``, plus ``n_p * itemsize`` with ``weights`` -- against ``8 n_p + n_p * cols *
        itemsize`` for ``pushRows`` of the expanded rows."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        offsets, g = self._offsets(rows, offsets)
        dtype = self.shards[0].np_dtype
        values = np.ascontiguousarray(values, dtype=dtype)
        if values.size != g * self.cols:
            raise ValueError(f"values: {values.size} elements, expected {g} groups x {self.cols} columns")
        values = values.reshape(g, self.cols)
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=dtype).reshape(-1)
            if weights.size != rows.size:
                raise ValueError(f"weights: {weights.size} values, expected {rows.size}")
        group = np.repeat(np.arange(g, dtype=np.int64), np.diff(offsets))  # the group of every record
        for _, sh, idx in _buckets(self, rows):  # idx in the caller's order, so its groups are non-decreasing
            counts = np.bincount(group[idx], minlength=g)
            has = np.flatnonzero(counts)  # the groups with a record here, ascending
            sub = np.zeros(has.size + 1, dtype=np.int64)
            np.cumsum(counts[has], out=sub[1:])
            sh.updateRowsGrouped(rows[idx], sub, values[has], None if weights is None else weights[idx],
                                 deterministic=deterministic)
        return True

    def pushAdagrad(self, state: "BigMatrix", rows, grads, lr: float, eps: float = 1e-10) -> bool:
        """Adagrad row push (an extension): this matrix holds the weights and ``state`` -- a BigMatrix
        with the same partitioner, rows, cols and dtype -- the accumulated squared gradients. ``grads`` is
        (n, cols) or flat. Per distinct row: its gradient rows are summed in the caller's order, then
        ``state += G * G`` and ``weights -= (lr * G) / (sqrt(state) + eps)`` on the shard that holds the
        row (PartialMatrix.updateRowsAdagrad). Bucketed by partition as ``pushRows``; one
        PartialMatrix.updateRowsAdagrad per non-empty partition, with its rows and gradient rows in the
        caller's order and that partition's state shard. A row lives in one partition, so the bits are the
        shard's."""
        return self._push_step(state, BigMatrix, 1, "state: expected a matrix with this one's partitioner, rows, "
                               "cols and dtype", rows, grads,
                               lambda sh, st, r, g: sh.updateRowsAdagrad(st, r, g, lr, eps))

    def _push_step(self, state, kind, state_cols_factor: int, message: str, rows, grads, call) -> bool:
        """What the optimizer row pushes share: ``state`` is a model of class ``kind`` laid out as this one --
        a BigVector of ``rows`` keys, or a BigMatrix of ``rows`` rows and ``state_cols_factor * cols`` columns,
        else ValueError(``message``) -- and each non-empty partition gets one ``call(shard, its state shard,
        its rows, their gradient rows)``, in the caller's order."""
        if not isinstance(state, kind):
            raise ValueError(f"state: expected a {kind.__name__}")
        dtype = self.shards[0].np_dtype
        if kind is BigVector:
            fits = state.size == self.rows
        else:
            fits = (state.rows, state.cols) == (self.rows, state_cols_factor * self.cols)
        if not fits or len(state.shards) != len(self.shards) \
                or np.dtype(state.shards[0].np_dtype) != np.dtype(dtype) \
                or not _same_partitioner(state.partitioner, self.partitioner):
            raise ValueError(message)
        rows, grads = self._rows_values(rows, grads, dtype, "grads")
        for p, sh, idx in _buckets(self, rows):
            call(sh, state.shards[p], rows[idx], grads[idx])
        return True

    def pushAdagradRowwise(self, state: "BigVector", rows, grads, lr: float, eps: float = 1e-10) -> bool:
        """Row-wise Adagrad row push (an extension): this matrix holds the weights and ``state`` -- a
        BigVector with the same partitioner, ``size == rows`` and dtype -- one accumulator per row (zeros
        to start with), so the optimizer state is ``1 / cols`` of the table. ``grads`` is (n, cols) or
        flat. Per distinct row: its gradient rows are summed in the caller's order, then ``state += mean(G
        * G)`` and ``weights -= (lr / (sqrt(state) + eps)) * G`` on the shard that holds the row
        (PartialMatrix.updateRowsAdagradRowwise). ``state``, the shapes and -- by the partitioner -- every
        row are validated before any shard is called. Bucketed by partition as ``pushRows``; one
        PartialMatrix.updateRowsAdagradRowwise per non-empty partition, with its rows and gradient rows in
        the caller's order and that partition's state shard. A row lives in one partition, so the bits are
        the shard's."""
        return self._push_step(state, BigVector, 0, "state: expected a vector with this matrix's partitioner, rows "
                               "and dtype", rows, grads,
                               lambda sh, st, r, g: sh.updateRowsAdagradRowwise(st, r, g, lr, eps))

    def pushAdam(self, state: "BigMatrix", rows, grads, lr: float, step: int, beta1: float = 0.9,
                 beta2: float = 0.999, eps: float = 1e-8) -> bool:
        """Adam row push (an extension): this matrix holds the weights and ``state`` -- a BigMatrix with
        the same partitioner, rows and dtype and ``2 * cols`` columns -- both moments of every row, ``m``
        in columns ``[0, cols)`` and ``v`` in ``[cols, 2 * cols)`` (zeros to start with). ``grads`` is
        (n, cols) or flat. Per distinct row: its gradient rows are summed in the caller's order, then one
        lazy Adam step with the caller's global ``step`` (from 1) is taken on the shard that holds the row
        (PartialMatrix.updateRowsAdam); rows that are not named keep their moments. ``state``, the shapes
        and -- by the partitioner -- every row are validated before any shard is called. Bucketed by
        partition as ``pushRows``; one PartialMatrix.updateRowsAdam per non-empty partition, with its rows
        and gradient rows in the caller's order and that partition's state shard. A row lives in one
        partition, so the bits are the shard's."""
        return self._push_step(state, BigMatrix, 2, _TWICE_COLS, rows, grads,
                               lambda sh, st, r, g: sh.updateRowsAdam(st, r, g, lr, step, beta1, beta2, eps))

    def pushFtrl(self, state: "BigMatrix", rows, grads, alpha: float, beta: float = 1.0, l1: float = 0.0,
                 l2: float = 0.0) -> bool:
        """FTRL-proximal row push (an extension): this matrix holds the weights and ``state`` -- a
        BigMatrix with the same partitioner, rows and dtype and ``2 * cols`` columns -- ``z`` in columns
        ``[0, cols)`` and ``n`` in ``[cols, 2 * cols)`` of every row (zeros to start with, beside zeroed
        weights). ``grads`` is (n, cols) or flat. Per distinct row: its gradient rows are summed in the
        caller's order, then one FTRL-proximal step is taken on the shard that holds the row
        (PartialMatrix.updateRowsFtrl); with ``l1 > 0`` a weight whose ``|z| <= l1`` becomes exactly +0, so
        ``pullSparse`` of trained rows moves their non-zeros only. ``state``, the shapes and -- by the
        partitioner -- every row are validated before any shard is called. Bucketed by partition as
        ``pushRows``; one PartialMatrix.updateRowsFtrl per non-empty partition, with its rows and gradient
        rows in the caller's order and that partition's state shard. A row lives in one partition, so the
        bits are the shard's."""
        return self._push_step(state, BigMatrix, 2, _TWICE_COLS, rows, grads,
                               lambda sh, st, r, g: sh.updateRowsFtrl(st, r, g, alpha, beta, l1, l2))

    def pull(self, rows, cols=None) -> np.ndarray:
        """pull(rows, cols): elements (AsyncBigMatrix.scala:96-130); pull(rows): whole rows as an
        (n, cols) array (AsyncBigMatrix.scala:53-86)."""
        rows = np.ascontiguousarray(rows, dtype=np.int64)
        buckets = _buckets(self, rows)
        if cols is None:
            out = np.zeros((rows.size, self.cols), dtype=self.shards[0].np_dtype)
            for _, sh, idx in buckets:
                out[idx] = sh.getRows(rows[idx])
            return out
        cols = np.ascontiguousarray(cols, dtype=np.int32)
        out = np.zeros(rows.shape, dtype=self.shards[0].np_dtype)
        for _, sh, idx in buckets:
            out[idx] = sh.get(rows[idx], cols[idx])
        return out

    def pullSparse(self, rows):
        """pull(rows) with only the non-zero elements (an extension): a CSR triple ``(indptr, cols,
        values)`` over the requested rows in the caller's order -- ``indptr`` n + 1 int64, request i's
        entries ``cols[indptr[i]:indptr[i+1]]`` (int32, ascending) with their ``values``. Bucketed by
        partition as ``pull``; one PartialMatrix.getRowsSparse per non-empty partition, and the partial
        triples merged without a Python loop over rows."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        n = rows.size
        counts = np.zeros(n, dtype=np.int64)  # entries per request, caller's order
        src0 = np.zeros(n, dtype=np.int64)    # where a request's entries start in the concatenated partials
        part_cols, part_vals, base = [], [], 0
        for _, sh, idx in _buckets(self, rows):
            ip, c, v = sh.getRowsSparse(rows[idx])
            ip = np.asarray(ip, dtype=np.int64)
            counts[idx] = np.diff(ip)
            src0[idx] = base + ip[:-1]
            part_cols.append(np.asarray(c, dtype=np.int32))
            part_vals.append(np.asarray(v, dtype=self.shards[0].np_dtype))
            base += int(ip[-1])
        indptr = np.zeros(n + 1, dtype=np.int64)
        np.cumsum(counts, out=indptr[1:])
        if not base:
            return indptr, np.zeros(0, np.int32), np.zeros(0, self.shards[0].np_dtype)
        # entry e of the answer belongs to request i = its row; it is entry e - indptr[i] of that request
        take = np.repeat(src0 - indptr[:-1], counts) + np.arange(base, dtype=np.int64)
        return indptr, np.concatenate(part_cols)[take], np.concatenate(part_vals)[take]

    def pullSum(self, rows, offsets, weights=None) -> np.ndarray:
        """The sums of groups of rows (an extension): ``offsets`` has g + 1 entries, non-decreasing from
        0 to len(rows); row k of the (g, cols) answer is the sum of ``rows[offsets[k]:offsets[k+1]]``, an
        empty group zeros. Bucketed by partition as ``pull``; each non-empty partition answers one
        PartialMatrix.getRowsSum over the sub-groups of its own rows, each in the caller's order. With
        ``weights`` (n,) record i's term is ``weights[i] * row``, the product rounded before it is added:
        the forward pass of a weighted bag, whose backward pass is ``pushGroups`` with the same weights;
        each partition is sent the weights of its own records, ``n_p * itemsize`` bytes more.

        Order of the additions: inside a partition strictly the caller's, left to right from the first
        row's stored bits; then, per group, the partials of the partitions that hold at least one of its
        rows are added in partition-index order, starting from the first such partial (not from zero).
        With one partition that is the strict caller order; with several it is partition-major, caller's
        order inside a partition. Deterministic either way; Int/Long wrap."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        offsets, g = self._offsets(rows, offsets)
        if weights is not None:
            weights = np.ascontiguousarray(weights, dtype=self.shards[0].np_dtype).reshape(-1)
            if weights.size != rows.size:
                raise ValueError(f"weights: {weights.size} values, expected {rows.size}")
        group = np.repeat(np.arange(g, dtype=np.int64), np.diff(offsets))  # the group of every record
        out = np.zeros((g, self.cols), dtype=self.shards[0].np_dtype)
        started = np.zeros(g, dtype=bool)  # groups that already hold a partition's partial
        for _, sh, idx in _buckets(self, rows):  # idx in the caller's order, so its groups are non-decreasing
            sub = np.zeros(g + 1, dtype=np.int64)
            np.cumsum(np.bincount(group[idx], minlength=g), out=sub[1:])
            if weights is None:
                part = sh.getRowsSum(rows[idx], sub)
            else:
                part = sh.getRowsSum(rows[idx], sub, weights=weights[idx])
            part = np.asarray(part, dtype=out.dtype)
            has = np.diff(sub) > 0
            first, more = has & ~started, has & started
            out[first] = part[first]
            out[more] = out[more] + part[more]
            started |= has
        return out

    def pullAverage(self, rows, offsets) -> np.ndarray:
        """pullSum over each group's length (1 for an empty group); Float/Double models."""
        return self.pullSum(rows, offsets) / np.maximum(np.diff(offsets), 1).astype(self.shards[0].np_dtype)[:, None]

    def pullDot(self, rows, x=None) -> np.ndarray:
        """The dot products of rows with caller vectors (an extension), reduced on the shards: ``x`` of
        shape (cols,) gives (n,), ``x`` of shape (q, cols) gives (n, q) with ``out[i, j] = dot(row
        rows[i], x[j])``, and ``x=None`` the (n,) squared norms. Bucketed by partition as ``pull``; one
        PartialMatrix.getRowsDot per non-empty partition, each with the same ``x``, and the answers
        scattered back to the caller's positions. A row lives in one partition, so nothing is combined
        here: the bits are the shard's."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        dtype = self.shards[0].np_dtype
        shape = (rows.size,)
        if x is not None:
            x = np.ascontiguousarray(x, dtype=dtype)
            self._check_queries(x)
            if x.ndim == 2:
                shape = (rows.size, x.shape[0])
        out = np.zeros(shape, dtype=dtype)
        for _, sh, idx in _buckets(self, rows):
            out[idx] = sh.getRowsDot(rows[idx], x)
        return out

    def pullGroupDot(self, rows, offsets, x) -> np.ndarray:
        """The dot product of every row with the one vector of its group (an extension), reduced on the
        shards: ``offsets`` is ``pullSum``'s, ``x`` is (g, cols) or flat, and the (n,) answer has
        ``out[i] = dot(row rows[i], x[k])`` with k the group of record i -- the gradient of
        ``pullSum(rows, offsets, weights)`` with respect to ``weights``. ``offsets``, the shapes and -- by
        the partitioner -- every row are validated before any shard is called. Records are bucketed by
        partition as ``pull``; each non-empty partition gets one PartialMatrix.getRowsGroupDot over the
        sub-groups of its own records, in the caller's order: only the groups that have a record in that
        partition are sent, their vectors compacted (``pushGroups``' construction), and the answers are
        scattered back to the caller's positions. A row lives in one partition, so nothing is combined
        here: the bits are the shard's under any partitioning.

        Bytes sent to a partition with n_p of the records in g_p of the groups: ``8 n_p + 8 (g_p + 1) +
        g_p * cols * itemsize``; bytes back: ``n_p * itemsize`` -- against ``n_p * cols * itemsize`` back
        for ``pull`` of the rows."""
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        offsets, g = self._offsets(rows, offsets)
        dtype = self.shards[0].np_dtype
        x = np.ascontiguousarray(x, dtype=dtype)
        if x.shape != (g, self.cols) and x.shape != (g * self.cols,):
            raise ValueError(f"x: shape {x.shape}, expected ({g}, {self.cols}) or ({g * self.cols},)")
        x = x.reshape(g, self.cols)
        group = np.repeat(np.arange(g, dtype=np.int64), np.diff(offsets))  # the group of every record
        out = np.zeros(rows.size, dtype=dtype)
        for _, sh, idx in _buckets(self, rows):  # idx in the caller's order, so its groups are non-decreasing
            counts = np.bincount(group[idx], minlength=g)
            has = np.flatnonzero(counts)  # the groups with a record here, ascending
            sub = np.zeros(has.size + 1, dtype=np.int64)
            np.cumsum(counts[has], out=sub[1:])
            out[idx] = sh.getRowsGroupDot(rows[idx], sub, x[has])
        return out

    def _pair_buckets(self, other: "BigMatrix", name: str, rows, other_rows):
        """What the row-pair calls do before any shard is called: ``other`` is a BigMatrix of this one's
        cols and dtype (its row count and partitioner are its own), both row arrays are validated by their
        own partitioner, and the pairs are bucketed by (own partition, other partition). Returns rows,
        other_rows and the non-empty buckets ``[(p, o, idx)]`` in ascending (p, o) order, ``idx`` the
        bucket's pair indices in the caller's order. A bucket whose two shards sit on different devices
        raises ValueError here."""
        if not isinstance(other, BigMatrix):
            raise ValueError(f"{name}: expected a BigMatrix")
        if other.cols != self.cols or np.dtype(other.shards[0].np_dtype) != np.dtype(self.shards[0].np_dtype):
            raise ValueError(f"{name}: expected a matrix with this one's cols and dtype")
        rows = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        other_rows = np.ascontiguousarray(other_rows, dtype=np.int64).reshape(-1)
        if other_rows.size != rows.size:
            raise ValueError(f"{name} rows: {other_rows.size}, expected {rows.size}")
        own = self.partitioner.partition_indices(rows)
        oth = other.partitioner.partition_indices(other_rows)
        nother = len(other.shards)
        order, off = bucket(own * nother + oth, len(self.shards) * nother)
        buckets = []
        for b in np.flatnonzero(np.diff(off)):
            p, o = divmod(int(b), nother)
            da, db = getattr(self.shards[p], "device", None), getattr(other.shards[o], "device", None)
            if da != db:
                raise ValueError(f"pairs of partition {p} (device {da}) with partition {o} of {name} (device {db}): "
                                 "the two shards of a pair must be on one device")
            buckets.append((p, o, order[off[b]:off[b + 1]]))
        return rows, other_rows, buckets

    def pullPairDot(self, other: "BigMatrix", rows, otherRows) -> np.ndarray:
        """Row-pair dot pull (an extension): ``out[i] = dot(row rows[i] of this matrix, row otherRows[i] of
        other)``, an (n,) array, reduced on the shards (PartialMatrix.getPairsDot): row ids go out and
        scores come back, nothing of size cols. ``other`` is a BigMatrix with this one's cols and dtype; its
        row count and partitioner may differ, and it may be this matrix. Both row arrays are validated
        before any shard is called. Pairs are bucketed by (own partition, other partition); each non-empty
        bucket gets one shard call, in ascending (own, other) order, with the caller's order inside a
        bucket, and the answers are scattered back to the caller's positions. A pair lives in one bucket,
        so nothing is combined here: the bits are the shard's. A bucket whose two shards are on different
        devices raises ValueError before any shard is called."""
        rows, other_rows, buckets = self._pair_buckets(other, "other", rows, otherRows)
        out = np.zeros(rows.size, dtype=self.shards[0].np_dtype)
        for p, o, idx in buckets:
            out[idx] = self.shards[p].getPairsDot(other.shards[o], rows[idx], other_rows[idx])
        return out

    def pushPairAxpy(self, src: "BigMatrix", rows, srcRows, coef, deterministic: bool = False) -> bool:
        """Row-pair axpy push (an extension): row rows[i] of this matrix += ``coef[i] *`` (row srcRows[i] of
        ``src``), the contribution rows built on the shards (PartialMatrix.updatePairsAxpy): row ids and
        coefficients go out, nothing of size cols. ``src`` is another BigMatrix with this one's cols and
        dtype; its row count and partitioner may differ. ``coef`` is (n,). Both row arrays are validated
        before any shard is called. Pairs are bucketed by (own partition, source partition); each non-empty
        bucket gets one shard call, in ascending (own, source) order, with the caller's order inside a
        bucket. A bucket whose two shards are on different devices raises ValueError before any shard is
        called.

        Order of a destination row's additions: buckets run in ascending source-partition index, with the
        caller's order inside a bucket -- source-partition-major. That equals the caller's order when
        ``src`` has one partition. Deterministic either way (as ``pullSum``'s partition-major rule);
        Int/Long wrap."""
        dtype = self.shards[0].np_dtype
        if src is self:
            raise ValueError("src: expected another matrix (the source must share no memory with this one)")
        rows, src_rows, buckets = self._pair_buckets(src, "src", rows, srcRows)
        coef = np.ascontiguousarray(coef, dtype=dtype).reshape(-1)
        if coef.size != rows.size:
            raise ValueError(f"coef: {coef.size} values, expected {rows.size}")
        for p, o, idx in buckets:
            self.shards[p].updatePairsAxpy(src.shards[o], rows[idx], src_rows[idx], coef[idx],
                                           deterministic=deterministic)
        return True

    def pullTopK(self, x, k: int):
        """The ``k`` rows of the matrix that score highest against caller vectors (an extension): ``x``
        of shape (cols,) gives ``(rows[k], vals[k])``, ``x`` of shape (q, cols) two (q, k) arrays. Every
        partition answers one PartialMatrix.getTopK with its own best ``k``; the -1 fill of partitions
        with fewer rows is dropped, and the at most ``parts * k`` pairs per query are merged here by the
        shards' order -- rank descending (every NaN below every number, -0 equal to +0), then global
        row ascending -- and the first ``k`` kept. A matrix of fewer than ``k`` rows fills the rest with
        row -1 and value 0. A score's bits depend on (type, cols) only and the order is total over
        (rank, row), so the answer does not depend on how the matrix is partitioned."""
        dtype = self.shards[0].np_dtype
        x = np.ascontiguousarray(x, dtype=dtype)
        self._check_queries(x)
        k = int(k)
        if k < 1:
            raise ValueError(f"k: {k}, expected k >= 1")
        x2 = x.reshape(-1, self.cols)
        parts = [sh.getTopK(x2, k) for sh in self.shards]
        rows = np.concatenate([np.asarray(r).reshape(x2.shape[0], k) for r, _ in parts], axis=1)
        vals = np.concatenate([np.asarray(v).reshape(x2.shape[0], k) for _, v in parts], axis=1)
        out_rows = np.full((x2.shape[0], k), -1, np.int64)
        out_vals = np.zeros((x2.shape[0], k), dtype)
        for j in range(x2.shape[0]):
            real = rows[j] >= 0
            r, v = rows[j][real], vals[j][real]
            best = np.lexsort((r, ~topk_rank_key(v)))[:k]  # the last key is the primary one
            out_rows[j, :best.size], out_vals[j, :best.size] = r[best], v[best]
        if x.ndim == 1:
            return out_rows[0], out_vals[0]
        return out_rows, out_vals

    def destroy(self) -> bool:
        for sh in self.shards:
            sh.destroy()
        return True


def topk_rank_key(vals: np.ndarray) -> np.ndarray:
    """Unsigned keys whose order is the top-k pull's rank (include/glint_gpu.h): Int/Long the value with
    its sign bit flipped; Float/Double the sign-flip key after -0 -> +0, with every NaN mapped to 0, below
    -inf's key."""
    vals = np.ascontiguousarray(vals)
    bits = 8 * vals.dtype.itemsize
    ut = np.dtype(f"uint{bits}").type
    sign = ut(1 << (bits - 1))
    if not np.issubdtype(vals.dtype, np.floating):
        return vals.view(ut) ^ sign
    u = np.where(vals == 0, ut(0), vals.view(ut))  # -0 -> +0
    key = np.where((u & sign) != 0, ~u, u | sign)
    return np.where(np.isnan(vals), ut(0), key).astype(ut)


class Client:
    """glint.Client's model factory with MI355X GPUs in the role of parameter servers."""

    def __init__(self, devices: Optional[Sequence[int]] = None):
        if devices is None:
            from . import _native as N
            devices = list(range(N.load().glint_device_count()))
        self.devices = list(devices)

    def _create(self, keys: int, modelsPerServer: int, createPartitioner: Callable, make_shard: Callable):
        # Client.create (Client.scala:53-94)
        if not self.devices:
            raise ModelCreationException("Cannot create a model without active parameter servers")
        nparts = int(min(keys, modelsPerServer * len(self.devices)))
        partitioner = createPartitioner(nparts, keys)
        shards = [make_shard(part, self.devices[i % len(self.devices)])
                  for i, part in enumerate(partitioner.all())]
        return partitioner, shards

    def vector(self, keys: int, dtype="double", modelsPerServer: int = 1,
               createPartitioner: Callable = RangePartitioner.apply) -> BigVector:
        resolve_dtype(dtype)  # ModelCreationException analogue for unsupported types: ValueError
        partitioner, shards = self._create(keys, modelsPerServer, createPartitioner,
                                           lambda part, dev: PartialVector(part, dtype, dev))
        return BigVector(partitioner, shards, keys)

    def matrix(self, rows: int, cols: int, dtype="double", modelsPerServer: int = 1,
               createPartitioner: Callable = RangePartitioner.apply) -> BigMatrix:
        resolve_dtype(dtype)
        partitioner, shards = self._create(rows, modelsPerServer, createPartitioner,
                                           lambda part, dev: PartialMatrix(part, cols, dtype, dev))
        return BigMatrix(partitioner, shards, rows, cols)

    def sampler(self, weights, firstKey: int = 0, device: Optional[int] = None):
        """A seeded weighted row sampler (glint_amd.sampler.Sampler; an extension) over integer ``weights``,
        entry i the weight of key ``firstKey + i``, on ``device`` or the client's first device."""
        from .sampler import Sampler
        if device is None:
            if not self.devices:
                raise ModelCreationException("Cannot create a sampler without active parameter servers")
            device = self.devices[0]
        return Sampler(weights, firstKey, device)


__all__ = ["Client", "BigVector", "BigMatrix", "bucket", "RangePartitioner", "CyclicPartitioner"]
