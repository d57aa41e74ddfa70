"""Expected values of the grouped row-sum pull, shared by test_rowsum_cpu.py and test_gpu_rowsum.py.

Nothing here calls the code under test: sums are replayed with a Python loop of elementwise numpy adds
in the shard's dtype, left to right, starting from the first row itself (not from zero)."""
import numpy as np

# a column of four rows whose left-to-right sum is 1 while the reversed and the pairwise sums are 0
ORDER_VECTORS = {
    np.float64: np.array([1e16, 1.0, -1e16, 1.0], np.float64),
    np.float32: np.array([1e8, 1.0, -1e8, 1.0], np.float32),
}


def replay(terms):
    """((t0 + t1) + t2) + ... over the first axis, in terms' dtype; int dtypes wrap. Empty: zeros."""
    terms = np.asarray(terms)
    if terms.shape[0] == 0:
        return np.zeros(terms.shape[1:], terms.dtype)
    acc = terms[0].copy()
    with np.errstate(over="ignore", invalid="ignore"):
        for t in terms[1:]:
            acc = np.add(acc, t, dtype=terms.dtype)
    return acc


def replay_reversed(terms):
    return replay(np.asarray(terms)[::-1])


def replay_pairwise(terms):
    """Tree sum: halves summed pairwise, then added."""
    terms = np.asarray(terms)
    if terms.shape[0] <= 1:
        return replay(terms)
    h = terms.shape[0] // 2
    return np.add(replay_pairwise(terms[:h]), replay_pairwise(terms[h:]), dtype=terms.dtype)


def replay_groups(table, local_rows, offsets):
    """(g, cols): group k = replay(table[local_rows[offsets[k]:offsets[k+1]]])."""
    g = len(offsets) - 1
    out = np.zeros((g, table.shape[1]), table.dtype)
    for k in range(g):
        out[k] = replay(table[local_rows[offsets[k]:offsets[k + 1]]])
    return out


def bits(a):
    """Raw integer view, so that NaN and -0.0 compare by their bits."""
    a = np.ascontiguousarray(a)
    return a.view(np.uint32 if a.dtype.itemsize == 4 else np.uint64)
