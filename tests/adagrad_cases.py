"""Expected values of the Adagrad row push, shared by test_adagrad_cpu.py and test_gpu_adagrad.py.

Nothing here calls the code under test. A push is replayed by the contract of include/glint_gpu.h, in the
table's dtype: per distinct row, a zero row plus its gradient rows in push order, then the seven operations
s = G * G, h' = h + s, r = sqrt(h'), d = r + eps, u = lr * G, p = u / d, w' = w - p, each one numpy ufunc
call (rounded on its own; numpy's sqrt and divide are IEEE correctly rounded and keep subnormals)."""
import functools
import zlib

import numpy as np

from axpy_cases import assert_bits  # noqa: F401  (re-exported for the tests)
from dot_cases import NOFMA, bits  # noqa: F401  (re-exported for the tests)

_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")


def sum_gradients(local, grads, dt, order=None):
    """{row: G}: a zero row plus the row's gradient rows, record by record in `order` (default: as given)."""
    G = {}
    with np.errstate(**_QUIET):
        for i in (range(len(local)) if order is None else order):
            l = int(local[i])
            G[l] = np.add(G.get(l, np.zeros(grads.shape[1], dt)), grads[i], dtype=dt)
    return G


def adagrad_step(w, h, G, lr, eps):
    """(w', h') of one row (or any broadcastable block): the seven operations, each one ufunc call."""
    dt = w.dtype
    lr, eps = dt.type(lr), dt.type(eps)  # rounded once to the table's type
    with np.errstate(**_QUIET):
        s = np.multiply(G, G, dtype=dt)
        h2 = np.add(h, s, dtype=dt)
        r = np.sqrt(h2, dtype=dt)
        d = np.add(r, eps, dtype=dt)
        u = np.multiply(lr, G, dtype=dt)
        p = np.divide(u, d, dtype=dt)
        w2 = np.subtract(w, p, dtype=dt)
    return w2, h2


def replay_adagrad(w, h, local, grads, lr, eps):
    """(w', h') of tables w, h (size, cols) after one push of gradient row i to row local[i]; rows the push
    does not name are copied."""
    w2, h2 = np.array(w), np.array(h)
    dt = w2.dtype
    assert h2.dtype == dt and h2.shape == w2.shape
    grads = np.asarray(grads, dtype=dt).reshape(len(local), w2.shape[1])
    sums = sum_gradients(local, grads, dt)
    if sums:
        named = np.fromiter(sums, np.int64, len(sums))  # the distinct rows: one step each, all at once
        w2[named], h2[named] = adagrad_step(w2[named], h2[named], np.stack(list(sums.values())), lr, eps)
    return w2, h2


# ---- the inputs that show the order -----------------------------------------------------------------
def order_inputs(npd):
    """600 records over 40 rows, cols = 67, gradient magnitudes over nine decades; (local, g, w0, h0, lr,
    eps)."""
    rng = np.random.default_rng(5)
    n, R, cols = 600, 40, 67
    local = rng.integers(0, R, n)
    g = (rng.standard_normal((n, cols)) * 10.0 ** rng.integers(-4, 5, (n, cols))).astype(npd)
    w0 = rng.standard_normal((R, cols)).astype(npd)
    h0 = np.abs(rng.standard_normal((R, cols))).astype(npd)
    return local, g, w0, h0, npd(0.05), npd(1e-6)


# ---- shared inputs of the GPU tests -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adagrad_inputs(dtype_name, n, cols, what="case"):
    """(n, cols) gradients over nine decades, so that the order of a sum shows; read-only, shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"adagrad/{what}/{dtype_name}/{n}/{cols}".encode()))
    g = (rng.standard_normal((n, cols)) * 10.0 ** rng.integers(-4, 5, (n, cols))).astype(npd)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def start_tables(dtype_name, size, cols):
    """(w0, h0): random weights and |random| accumulators of a shard; read-only, shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"adagrad/start/{dtype_name}/{size}/{cols}".encode()))
    w0 = rng.standard_normal((size, cols)).astype(npd)
    h0 = np.abs(rng.standard_normal((size, cols))).astype(npd)
    w0.setflags(write=False)
    h0.setflags(write=False)
    return w0, h0


@functools.lru_cache(maxsize=None)
def sweep_inputs(dtype_name, size, cols):
    """The rounding sweep's (h0, G, w0), every row named once: h spans the type's whole exponent range,
    subnormals and zero included; G spans +-(2^-60 .. 2^60) for double, +-(2^-20 .. 2^20) for float. Inside
    that span G * G is at least 2^-120 (2^-40), so neither h' nor p can be subnormal there; the first
    quarter of the rows therefore takes G below the span, near the square root of the smallest normal,
    against a subnormal h (even rows: G * G and h' subnormal) or a huge one (odd rows: p subnormal).
    Read-only, shared."""
    npd = np.dtype(dtype_name).type
    info = np.finfo(npd)
    rng = np.random.default_rng(zlib.crc32(f"adagrad/sweep/{dtype_name}/{size}/{cols}".encode()))
    shape = (size, cols)
    # exponents from below the smallest subnormal's to just under overflow
    lo_e, hi_e = info.minexp - info.nmant - 1, info.maxexp - 1
    mant = 1.0 + rng.random(shape)
    with np.errstate(under="ignore"):
        h = np.ldexp(mant, rng.integers(lo_e, hi_e, shape)).astype(npd)
    h[rng.random(shape) < 0.02] = 0
    ge = 60 if npd == np.float64 else 20
    G = (np.ldexp(1.0 + rng.random(shape), rng.integers(-ge, ge, shape)) * rng.choice([-1.0, 1.0], shape)).astype(npd)
    q = size // 4
    te = info.minexp // 2  # 2^te squared is the smallest normal
    G[:q] = (np.ldexp(1.0 + rng.random((q, cols)), rng.integers(te - 10, te, (q, cols)))
             * rng.choice([-1.0, 1.0], (q, cols))).astype(npd)
    with np.errstate(under="ignore"):
        h[0:q:2] = np.ldexp(mant[0:q:2], rng.integers(lo_e, info.minexp + 2, h[0:q:2].shape)).astype(npd)
    h[1:q:2] = np.ldexp(mant[1:q:2], rng.integers(info.maxexp - 8, info.maxexp - 1, h[1:q:2].shape)).astype(npd)
    w = rng.standard_normal(shape).astype(npd)
    w[::3] = 0  # weights that a subnormal p changes
    for a in (h, G, w):
        a.setflags(write=False)
    return h, G, w
