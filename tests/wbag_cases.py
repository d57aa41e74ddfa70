"""Expected values of the weighted row-sum pull and the grouped row-dot pull, shared by test_wbag_cpu.py
and test_gpu_wbag.py.

Nothing here calls the code under test. A weighted sum is the row-sum replay (rowsum_cases.replay: left to
right from the first term as it is) of the terms ``weights[i] * row``, one numpy multiply with every product
rounded on its own; a grouped dot is the row dot's replay (dot_cases.replay_dot) of record i's row against
the vector of its group (group_cases.group_of)."""
from fractions import Fraction

import numpy as np

from dot_cases import lane_width, reduce_products, replay_dot  # noqa: F401  (replay_dot: the per-record form)
from group_cases import group_of
from rowsum_cases import bits, replay  # noqa: F401  (bits re-exported for the tests)

# four rows of ones under these weights: the left-to-right sum is 1, the reversed and the pairwise sums 0
ORDER_WEIGHTS = {
    np.float64: np.array([1e16, 1.0, -1e16, 1.0], np.float64),
    np.float32: np.array([1e8, 1.0, -1e8, 1.0], np.float32),
}


def weighted_terms(table_rows, weights):
    """(n, cols): weights[i] * table_rows[i], each product rounded on its own; int dtypes wrap."""
    rows = np.asarray(table_rows)
    w = np.asarray(weights, dtype=rows.dtype).reshape(-1)
    assert rows.ndim == 2 and w.size == rows.shape[0]
    with np.errstate(over="ignore", invalid="ignore", under="ignore"):
        return np.multiply(w[:, None], rows, dtype=rows.dtype)


def replay_wsum(table_rows, weights):
    """((w0 * r0) + (w1 * r1)) + ... over the first axis, starting from the first product. Empty: zeros."""
    return replay(weighted_terms(table_rows, weights))


def replay_wgroups(table, local_rows, offsets, weights, bad=None):
    """(g, cols): group k = replay_wsum over its records. `bad` (n,) bool: records whose row lies outside the
    partition -- their term is +0 / 0 whatever the weight, and their entry of local_rows is not used."""
    table = np.asarray(table)
    local = np.asarray(local_rows, np.int64)
    terms = weighted_terms(table[np.where(bad, 0, local) if bad is not None else local], weights)
    if bad is not None:
        terms[np.asarray(bad, bool)] = 0
    g = len(offsets) - 1
    out = np.zeros((g, table.shape[1]), table.dtype)
    for k in range(g):
        out[k] = replay(terms[offsets[k]:max(offsets[k], offsets[k + 1])])
    return out


def replay_gdot(table, local_rows, group, x):
    """(n,): dot(table[local_rows[i]], x[group[i]]) in the row dot's order; group[i] < 0 (no group covers the
    record) answers zero."""
    table, x = np.asarray(table), np.asarray(x)
    local, group = np.asarray(local_rows, np.int64), np.asarray(group, np.int64)
    E = lane_width(table.dtype, table.shape[1])
    out = np.zeros(local.size, table.dtype)
    has = np.flatnonzero(group >= 0)
    if has.size:  # replay_dot(row, vector) for every record at once: the same products, the same reduction
        with np.errstate(over="ignore", invalid="ignore", under="ignore"):
            prod = np.multiply(table[local[has]], x[group[has]], dtype=table.dtype)
        out[has] = reduce_products(prod, E)
    return out


def replay_gdot_groups(table, local_rows, offsets, x):
    """replay_gdot with the groups of a well-formed offsets array."""
    return replay_gdot(table, local_rows, group_of(offsets, len(local_rows)), x)


def clamped_groups(offsets, n):
    """The group of every record under a device caller's malformed offsets, by the grouped push's rule:
    every value clamped to [0, n], then an upper-bound search for the first position p whose cut exceeds i;
    the group is p - 1, or -1 when p is 0 or past g (no group covers the record)."""
    cut = np.clip(np.asarray(offsets, np.int64), 0, n)
    g = cut.size - 1
    out = np.full(n, -1, np.int64)
    for i in range(n):
        lo, hi = 0, g + 1
        while lo < hi:  # the first position whose cut exceeds i
            mid = lo + (hi - lo) // 2
            if cut[mid] > i:
                hi = mid
            else:
                lo = mid + 1
        if 1 <= lo <= g:
            out[i] = lo - 1
    return out


# ---- known answers: a fused multiply-add shows ---------------------------------------------------
# w0 * r0 = -(1 + 2u) exactly; w1 * r1 = (1 + u)^2 = 1 + 2u + u^2 rounds to 1 + 2u (u^2 is a quarter of an
# ulp), so the sum of the rounded products is exactly 0, while a fused w1 * r1 + (w0 * r0) keeps the u^2:
# 2^-60 (Double, u = 2^-30), 2^-26 (Float, u = 2^-13).
NOFMA_W = {
    np.float64: (1.0, -(1.0 + 2.0 ** -29), 1.0 + 2.0 ** -30, 2.0 ** -60),
    np.float32: (np.float32(1.0), np.float32(-(1.0 + 2.0 ** -12)), np.float32(1.0 + 2.0 ** -13), 2.0 ** -26),
}


def nofma_wcase(npd):
    """(weights (2,), column values (2,), fused): the contract's sum is 0; `fused` is what a contraction of
    the second product into the add would give, computed exactly."""
    w0, r0, a, fused = NOFMA_W[npd]
    w, r = np.array([w0, a], npd), np.array([r0, a], npd)
    exact = Fraction(float(w[0])) * Fraction(float(r[0])) + Fraction(float(w[1])) * Fraction(float(r[1]))
    assert exact == Fraction(fused) and npd(float(exact)) == npd(fused)  # representable: the fused result
    return w, r, npd(fused)
