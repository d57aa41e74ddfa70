"""Expected values of the top-k row pull, shared by test_topk_cpu.py and test_gpu_topk.py.

Nothing here calls the code under test. Scores are the row dot pull's replay over the whole table
(dot_cases.replay_dot); the order is include/glint_gpu.h's: rank descending -- every NaN below every
number, all NaNs equal, -0 equal to +0, Int/Long by the signed value -- then global row ascending, taken
with a stable sort over the rows in ascending order."""
import numpy as np

from dot_cases import bits, replay_dot


def rank_key(vals):
    """Unsigned integers whose order is the rank of `vals`."""
    vals = np.ascontiguousarray(vals)
    nbits = 8 * vals.dtype.itemsize
    ut = np.dtype(f"uint{nbits}")
    top = 1 << (nbits - 1)
    out = np.empty(vals.shape, ut)
    flat_in, flat_out = vals.reshape(-1), out.reshape(-1)
    if np.issubdtype(vals.dtype, np.floating):
        raw = bits(flat_in)
        for i, v in enumerate(flat_in):
            if v != v:
                flat_out[i] = 0  # below -inf, whose key is the smallest of a number
            elif v == 0:
                flat_out[i] = top  # either zero
            elif v > 0:
                flat_out[i] = int(raw[i]) | top
            else:
                flat_out[i] = ~int(raw[i]) & ((1 << nbits) - 1)
    else:
        for i, v in enumerate(flat_in):
            flat_out[i] = int(v) + top
    return out


def rank_key_fast(vals):
    """rank_key, vectorised (the tables of the GPU tests have tens of thousands of rows);
    test_topk_cpu.py pins it to rank_key."""
    vals = np.ascontiguousarray(vals)
    nbits = 8 * vals.dtype.itemsize
    ut = np.dtype(f"uint{nbits}").type
    top = ut(1 << (nbits - 1))
    if not np.issubdtype(vals.dtype, np.floating):
        return bits(vals) ^ top
    raw = bits(vals)
    key = np.where(vals > 0, raw | top, ~raw)
    key = np.where(vals == 0, top, key)
    return np.where(np.isnan(vals), ut(0), key).astype(ut)


def global_rows(size, first_row=0, cyclic=None):
    """The global keys of local rows 0 .. size-1: first_row + local, or index + local * parts for
    cyclic = (index, parts)."""
    local = np.arange(size, dtype=np.int64)
    return local * cyclic[1] + cyclic[0] if cyclic else local + first_row


def scores_of(table, x):
    """replay_dot over the whole table, in blocks of rows: (n,) for x (cols,), (n, q) for (q, cols)."""
    table = np.asarray(table)
    x = np.asarray(x, dtype=table.dtype)
    if table.shape[0] == 0:
        return np.zeros((0,) + x.shape[:-1], table.dtype)
    step = max(1, (1 << 22) // max(1, table.shape[1] * (x.shape[0] if x.ndim == 2 else 1)))
    return np.concatenate([replay_dot(table[i:i + step], x) for i in range(0, table.shape[0], step)])


def topk_of_scores(scores, rows, k):
    """(rows[k], vals[k]) of one query: `scores` of the rows with global keys `rows`, ascending."""
    assert (np.diff(rows) > 0).all()
    inv = ~rank_key_fast(scores)  # ascending inv = descending rank
    order = np.argsort(inv, kind="stable")[:k]  # stable: equal ranks keep the ascending rows
    out_rows = np.full(k, -1, np.int64)
    out_vals = np.zeros(k, scores.dtype)
    out_rows[:order.size], out_vals[:order.size] = rows[order], scores[order]
    return out_rows, out_vals


def topk_of_score_table(sc, rows, k):
    """Two (q, k) arrays from the scores (n, q) of the rows with global keys `rows`."""
    per = [topk_of_scores(np.ascontiguousarray(sc[:, j]), rows, k) for j in range(sc.shape[1])]
    return np.stack([r for r, _ in per]), np.stack([v for _, v in per])


def expected_topk(table, x, k, first_row=0, cyclic=None):
    """x (cols,) -> (rows[k], vals[k]); x (q, cols) -> two (q, k) arrays."""
    table = np.asarray(table)
    x = np.asarray(x, dtype=table.dtype)
    rows = global_rows(table.shape[0], first_row, cyclic)
    sc = scores_of(table, x)
    if x.ndim == 1:
        return topk_of_scores(sc, rows, k)
    return topk_of_score_table(sc, rows, k)


def assert_topk_bits(got, exp, what=""):
    """Rows equal, scores bit for bit; a NaN is compared by class (payload and sign unspecified)."""
    g_rows, g_vals = (a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a) for a in got)
    e_rows, e_vals = exp
    assert g_rows.dtype == np.int64 and g_rows.shape == e_rows.shape, what
    assert g_vals.dtype == e_vals.dtype and g_vals.shape == e_vals.shape, what
    np.testing.assert_array_equal(g_rows, e_rows, err_msg=what)
    if np.issubdtype(e_vals.dtype, np.floating):
        nan = np.isnan(e_vals)
        np.testing.assert_array_equal(np.isnan(g_vals), nan, err_msg=what)
        g_vals, e_vals = np.where(nan, 0, g_vals), np.where(nan, 0, e_vals)
    np.testing.assert_array_equal(bits(g_vals), bits(e_vals), err_msg=what)
