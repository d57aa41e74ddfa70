"""Expected values of the row-wise Adagrad row push, shared by test_rowwise_cpu.py and test_gpu_rowwise.py.

Nothing here calls the code under test. A push is replayed by the contract of include/glint_gpu.h, in the
table's dtype: per distinct row a zero row plus its gradient rows in push order
(adagrad_cases.sum_gradients), ss = the row dot pull's self-dot of that sum (dot_cases.replay_self: the
lane layout, ascending columns per lane, the xor butterfly), then s = ss / C, h' = h + s, r = sqrt(h'),
d = r + eps, k = lr / d per row and p = k * G, w' = w - p per column, each one numpy ufunc call (rounded on
its own; numpy's sqrt and divide are IEEE correctly rounded and keep subnormals). The state is a vector:
one accumulator per row."""
import functools
import zlib
from fractions import Fraction

import numpy as np

from adagrad_cases import adagrad_inputs, assert_bits, bits, sum_gradients  # noqa: F401  (re-exported)
from dot_cases import lane_width, replay_self  # noqa: F401  (re-exported)

LANES = 64

_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def rowwise_terms(w, h, G, lr, eps, ss=None):
    """Every named value of the contract's steps 2 to 4 for a block of rows: w, G (m, cols), h (m,). `ss`
    overrides the contract-order sum of squares (the premises pass another order's)."""
    w, h, G = np.asarray(w), np.asarray(h), np.asarray(G)
    dt = w.dtype
    assert h.dtype == dt and G.dtype == dt and G.shape == w.shape and h.shape == w.shape[:1]
    lr, eps, C = dt.type(lr), dt.type(eps), dt.type(w.shape[1])  # each rounded once to the table's type
    with np.errstate(**_QUIET):
        if ss is None:
            ss = replay_self(G)
        s = np.divide(ss, C, dtype=dt)
        h2 = np.add(h, s, dtype=dt)
        r = np.sqrt(h2, dtype=dt)
        d = np.add(r, eps, dtype=dt)
        k = np.divide(lr, d, dtype=dt)
        p = np.multiply(k[:, None], G, dtype=dt)
        w2 = np.subtract(w, p, dtype=dt)
    return dict(ss=ss, s=s, h2=h2, r=r, d=d, k=k, p=p, w2=w2)


def rowwise_step(w, h, G, lr, eps):
    """(w', h') of a block of rows."""
    t = rowwise_terms(w, h, G, lr, eps)
    return t["w2"], t["h2"]


def replay_rowwise(w, h, local, grads, lr, eps):
    """(w', h') of the table w (size, cols) and the accumulators h (size,) after one push of gradient row i
    to row local[i]; rows the push does not name are copied."""
    w2, h2 = np.array(w), np.array(h)
    dt = w2.dtype
    assert h2.dtype == dt and h2.shape == w2.shape[:1]
    grads = np.asarray(grads, dtype=dt).reshape(len(local), w2.shape[1])
    sums = sum_gradients(local, grads, dt)
    if sums:
        named = np.fromiter(sums, np.int64, len(sums))  # the distinct rows: one step each, all at once
        w2[named], h2[named] = rowwise_step(w2[named], h2[named], np.stack(list(sums.values())), lr, eps)
    return w2, h2


# ---- exact arithmetic: known answers, and what a fused multiply-add would store ------------------------
def F(x):
    return Fraction(float(x))


def round_fraction(x, npd):
    """The rational x rounded once to the type, to nearest even; subnormals kept; no overflow expected
    (adam_cases.round_fraction's method)."""
    info = np.finfo(npd)
    if x == 0:
        return npd(0)
    a = abs(x)
    e = a.numerator.bit_length() - a.denominator.bit_length()
    if Fraction(2) ** e > a:
        e -= 1
    assert Fraction(2) ** e <= a < Fraction(2) ** (e + 1)
    e = max(e, int(info.minexp))
    quantum = Fraction(2) ** (e - int(info.nmant))
    k, rem = divmod(a / quantum, 1)
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2):
        k += 1
    val = float(k * quantum)  # exact: k has at most nmant + 2 bits
    assert val <= float(info.max)
    return npd(-val if x < 0 else val)


def round_sqrt(x, npd):
    """sqrt of the rational x > 0 rounded once to the type: the candidate from the type's own sqrt, proved
    by squaring the midpoints to its two neighbours."""
    c = np.sqrt(round_fraction(x, npd), dtype=npd)
    for _ in range(4):
        lo = (F(c) + F(np.nextafter(c, npd(0)))) / 2
        hi = (F(c) + F(np.nextafter(c, npd(np.inf)))) / 2
        if lo * lo > x:
            c = np.nextafter(c, npd(0))
        elif hi * hi < x:
            c = np.nextafter(c, npd(np.inf))
        else:
            assert lo * lo < x < hi * hi  # a tie would need a square root with one bit more than the type
            return npd(c)
    raise AssertionError("no rounding of the square root found")


def fused_ss(G):
    """ss of one row G with every lane's chain fused, acc = round(acc + exact G * G), and the butterfly as
    the contract has it: what contraction of dot_step would give."""
    G = np.asarray(G)
    npd = G.dtype.type
    cols = G.size
    E = lane_width(G.dtype, cols)
    acc = np.zeros(LANES, G.dtype)
    for c in range(cols):  # ascending c is ascending within every lane
        L = (c // E) % LANES
        acc[L] = round_fraction(F(acc[L]) + F(G[c]) * F(G[c]), npd)
    lane = np.arange(LANES)
    for d in (32, 16, 8, 4, 2, 1):
        acc = np.add(acc, acc[lane ^ d], dtype=G.dtype)
    return acc[0]


def fused_update(w, k, G):
    """fma(-k, G, w) for a row, computed exactly and rounded once."""
    npd = w.dtype.type
    return np.array([round_fraction(F(wi) - F(k) * F(gi), npd) for wi, gi in zip(w, G)], npd)


# ---- the premise inputs: what an order, a reciprocal or a fusion would show on -------------------------
@functools.lru_cache(maxsize=None)
def premise_rows(dtype_name, cols, what):
    """16 gradient rows over nine decades (adagrad_inputs under this file's own names); read-only, shared."""
    return adagrad_inputs(dtype_name, 16, cols, f"rowwise/{what}")


FUSED_SS_COLS = {"float32": 256, "float64": 128}  # one 16-B strip: a lane's chain has 4 / 2 products
LR, EPS = 0.05, 1e-6


@functools.lru_cache(maxsize=None)
def start_state(dtype_name, size, cols):
    """(w0, h0): random weights (size, cols) and |random| accumulators (size,); read-only, shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"rowwise/start/{dtype_name}/{size}/{cols}".encode()))
    w0 = rng.standard_normal((size, cols)).astype(npd)
    h0 = np.abs(rng.standard_normal(size)).astype(npd)
    w0.setflags(write=False)
    h0.setflags(write=False)
    return w0, h0


@functools.lru_cache(maxsize=None)
def cancel_inputs(dtype_name, cols=128, m=4):
    """(G, h0, w0) of m rows whose update cancels: G over five decades, k taken from the replay (LR, EPS, h0
    = |random|), w0 = (k * G)(1 + delta) with delta uniform in +-2^-10, so w - k * G keeps only what the
    product's rounding left. Read-only, shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"rowwise/cancel/{dtype_name}/{cols}".encode()))
    G = (rng.standard_normal((m, cols)) * 10.0 ** rng.integers(-2, 3, (m, cols))).astype(npd)
    G[G == 0] = 1
    h0 = np.abs(rng.standard_normal(m)).astype(npd)
    k = rowwise_terms(np.zeros_like(G), h0, G, LR, EPS)["k"]
    delta = rng.uniform(-2.0 ** -10, 2.0 ** -10, (m, cols))
    w0 = (k.astype(np.float64)[:, None] * G.astype(np.float64) * (1 + delta)).astype(npd)
    for a in (G, h0, w0):
        a.setflags(write=False)
    return G, h0, w0


def premise_pushes(dtype_name):
    """[(label, G, h0, w0)]: the inputs test_rowwise_cpu.py asserts its premises on, as pushes of m rows, every
    row once, with LR and EPS -- the order of ss (cols 67, 256), the division by C and the one division per
    row (cols 3, 67), the cancelling update and the lane chains that a fused add would change."""
    npd = np.dtype(dtype_name).type
    out = []
    for cols in (67, 256):
        G = premise_rows(dtype_name, cols, "order")
        out.append((f"order/{cols}", G, np.zeros(16, npd), start_state(dtype_name, 16, cols)[0]))
    for cols in (3, 67):
        G = premise_rows(dtype_name, cols, "divide")
        h0 = np.abs(premise_rows(dtype_name, cols, "divide-h")[:, 0])
        out.append((f"divide/{cols}", G, h0, start_state(dtype_name, 16, cols)[0]))
    G, h0, w0 = cancel_inputs(dtype_name)
    out.append(("cancel", G, h0, w0))
    cols = FUSED_SS_COLS[dtype_name]
    out.append(("fused-ss", premise_rows(dtype_name, cols, "fused"), np.zeros(16, npd),
                start_state(dtype_name, 16, cols)[0]))
    return out
