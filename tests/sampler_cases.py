"""Expected draws of the row sampler, shared by test_sampler_cpu.py and test_gpu_sampler.py.

Nothing here calls the code under test. The generator is init_cases.py's numpy Philox4x32-10, the point of
an attempt is the exact 128-bit product taken with Python ints, and the search is ``bisect_right`` (one point)
or numpy's ``searchsorted(side="right")`` on uint64 (many points; the two are compared in the CPU file)
(include/glint_gpu.h, "Row sampler")."""
import bisect

import numpy as np

from init_cases import philox4x32_10

MAX_TRIES = 8
M64 = (1 << 64) - 1
W_MAX = (1 << 32) - 1


def cdf_of(weights):
    """Inclusive prefix sums as uint64 (the contract bounds the total below 2^63, so nothing wraps)."""
    w = np.asarray(weights)
    assert w.ndim == 1 and w.size >= 1 and (w >= 0).all() and (w <= W_MAX).all()
    assert w.size < 1 << 31  # so the total is below 2^31 * 2^32
    return np.cumsum(w.astype(np.uint64), dtype=np.uint64)


def words(seed, d, t, word3=1):
    """Philox output words (..., 4) of attempts t of draws d (arrays broadcast) under seed."""
    d = np.asarray(d, dtype=np.uint64)
    t = np.asarray(t, dtype=np.uint64)
    lo, hi = d & np.uint64(0xFFFFFFFF), d >> np.uint64(32)
    ctr = np.stack(np.broadcast_arrays(lo, hi, t, np.uint64(word3)), axis=-1)
    return philox4x32_10(ctr, np.array([seed & 0xFFFFFFFF, seed >> 32], np.uint64))


def points(seed, d, t, total):
    """x = floor(r * total / 2^64) of attempts t of draws d, as uint64; the product is a Python int."""
    o = words(seed, d, t).astype(np.uint64)
    r = o[..., 0] | (o[..., 1] << np.uint64(32))
    x = (r.astype(object) * int(total)) >> 64
    return np.asarray(x, dtype=object).astype(np.uint64)


def upper(cdf, x):
    """The smallest i with cdf[i] > x, one point."""
    return bisect.bisect_right(cdf, int(x)) if isinstance(cdf, list) else int(np.searchsorted(cdf, np.uint64(x), side="right"))


def counters(first, n):
    """first + i mod 2^64 for i < n, as uint64."""
    return ((np.arange(n, dtype=object) + int(first)) & M64).astype(np.uint64) if n else np.zeros(0, np.uint64)


def replay_draw(weights, first_key, seed, first, n, exclude=None, per=1, cdf=None):
    """The n global keys of a call (include/glint_gpu.h, "One draw")."""
    cdf = cdf_of(weights) if cdf is None else cdf
    m, total = cdf.size, int(cdf[-1])
    d = counters(first, n)
    idx = np.searchsorted(cdf, points(seed, d, 0, total), side="right").astype(np.int64)
    if exclude is not None and n:
        forb = np.asarray(exclude, dtype=np.int64)[np.arange(n) // per].astype(object) - int(first_key)
        forb = np.array([int(f) if 0 <= f < m else -1 for f in forb], np.int64)
        for i in np.nonzero(idx == forb)[0]:
            f, k = int(forb[i]), int(idx[i])
            for t in range(1, MAX_TRIES):
                if k != f:
                    break
                k = upper(cdf, points(seed, d[i], t, total))
            if k == f:
                k = upper(cdf, int(cdf[f]) % total)
            idx[i] = k
    return idx + np.int64(first_key)


# ---- weight tables -------------------------------------------------------------------------------------
def zipf_counts(m, rng_seed=3, top=1 << 20):
    """Counts ~ top / rank, at least 1, in a shuffled order (so the cdf's steps are of every size)."""
    w = np.maximum(top // np.arange(1, m + 1, dtype=np.int64), 1)
    return np.random.default_rng(rng_seed).permutation(w)


def table(m, pattern, coarse):
    """Weights of m entries. `coarse` is the library's coarse table size: the boundary a zero run is laid
    across is that of the coarse blocks (2^shift entries each, shift the least with coarse << shift >= m)."""
    rng = np.random.default_rng(m * 7 + len(pattern))
    shift = 0
    while (coarse << shift) < m:
        shift += 1
    if pattern == "ones":
        return np.ones(m, np.int64)
    if pattern == "zipf":
        return zipf_counts(m)
    if pattern == "max":
        return np.full(m, W_MAX, np.int64)
    w = rng.integers(1, 100, m).astype(np.int64)
    run = max(1, min(m // 3, 3 << shift))  # longer than a coarse block when m allows
    if pattern == "zeros_start":
        w[:run] = 0
    elif pattern == "zeros_end":
        w[m - run:] = 0
    elif pattern == "zeros_coarse":
        # across the boundaries between coarse blocks around the middle, from inside one block into another
        b = max(1, ((m // 2) >> shift) << shift)
        w[max(0, b - run // 2 - 1):min(m - 1, b + run // 2 + 1)] = 0
    else:
        raise ValueError(pattern)
    if not w.any():
        w[m - 1 if pattern != "zeros_end" else 0] = 5
    return w


# exclusion: (name, weights, first_key, exclude keys that the draws are made against)
BIG = 10 ** 12 % W_MAX
CONCENTRATED = np.array([0, BIG, 0, 1, 0], np.int64)       # nearly every attempt names entry 1
CONCENTRATED_LAST = np.array([0, 1, 0, BIG, 0], np.int64)  # ... entry 3, the last non-zero one
SINGLE = np.array([0, 0, 7, 0], np.int64)                  # one non-zero entry: a draw may equal forb
EXCLUSION = [
    ("concentrated_hot", CONCENTRATED, 100, 101),        # all tries hit -> the next non-zero entry (3)
    ("concentrated_wrap", CONCENTRATED_LAST, 100, 103),  # ... -> the fallback wraps round to entry 1
    ("concentrated_cold", CONCENTRATED, 100, 103),       # the excluded entry is (almost) never named
    ("single", SINGLE, -5, -3),                     # forb is the only entry: returned
    ("outside_low", CONCENTRATED, 100, 99),         # outside the key range: ignored
    ("outside_high", CONCENTRATED, 100, 105),
    ("outside_far", CONCENTRATED, 100, -(1 << 63)),
]

# the distribution check's table (the issue fixes it)
def dist_table():
    w = np.random.default_rng(1).integers(0, 50, 64)
    w[[0, 5, 6, 63]] = 0
    return w.astype(np.int64)
