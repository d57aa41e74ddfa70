"""Expected values of the Adam row push, shared by test_adam_cpu.py and test_gpu_adam.py.

Nothing here calls the code under test. A push is replayed by the contract of include/glint_gpu.h, in the
table's dtype: the scalars settled in Python floats (doubles) and rounded once to the type; per distinct
row a zero row plus its gradient rows in push order (adagrad_cases.sum_gradients); then the fourteen
operations of the step, each one numpy ufunc call (rounded on its own; numpy's sqrt and divide are IEEE
correctly rounded and keep subnormals). The state table packs both moments: m in columns [0, cols), v in
[cols, 2 * cols)."""
import functools
import math
import zlib
from fractions import Fraction

import numpy as np

from adagrad_cases import adagrad_inputs, assert_bits, bits, order_inputs, sum_gradients  # noqa: F401  (re-exported)

_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")
BETA1, BETA2, EPS = 0.9, 0.999, 1e-8  # the defaults of updateRowsAdam / pushAdam


def adam_scalars(dt, lr, beta1, beta2, eps, step):
    """(b1, b2, a1, a2, alpha, rc2, eps) in the table's type: settled in double, each rounded once."""
    dt = np.dtype(dt)
    lr, beta1, beta2, eps = float(lr), float(beta1), float(beta2), float(eps)
    c1 = 1.0 - math.pow(beta1, float(step))
    c2 = 1.0 - math.pow(beta2, float(step))
    alpha = lr / c1
    rc2 = math.sqrt(c2)
    a1 = 1.0 - beta1
    a2 = 1.0 - beta2
    return tuple(dt.type(x) for x in (beta1, beta2, a1, a2, alpha, rc2, eps))


def adam_terms(w, m, v, G, scalars):
    """Every named value of the contract's step 2 for a block, as a dict; each operation one ufunc call."""
    dt = w.dtype
    b1, b2, a1, a2, alpha, rc2, eps = scalars
    assert all(type(x) is dt.type for x in scalars)
    with np.errstate(**_QUIET):
        t1 = np.multiply(b1, m, dtype=dt)
        t2 = np.multiply(a1, G, dtype=dt)
        m2 = np.add(t1, t2, dtype=dt)
        q = np.multiply(G, G, dtype=dt)
        t3 = np.multiply(b2, v, dtype=dt)
        t4 = np.multiply(a2, q, dtype=dt)
        v2 = np.add(t3, t4, dtype=dt)
        r = np.sqrt(v2, dtype=dt)
        s = np.divide(r, rc2, dtype=dt)
        d = np.add(s, eps, dtype=dt)
        u = np.multiply(alpha, m2, dtype=dt)
        p = np.divide(u, d, dtype=dt)
        w2 = np.subtract(w, p, dtype=dt)
    return dict(t1=t1, t2=t2, m2=m2, q=q, t3=t3, t4=t4, v2=v2, r=r, s=s, d=d, u=u, p=p, w2=w2)


def adam_step(w, m, v, G, scalars):
    """(w', m', v') of one row (or any broadcastable block)."""
    t = adam_terms(w, m, v, G, scalars)
    return t["w2"], t["m2"], t["v2"]


def replay_adam(w, state, local, grads, lr, step, beta1=BETA1, beta2=BETA2, eps=EPS):
    """(w', state') of tables w (size, cols) and state (size, 2 * cols) after one push of gradient row i to
    row local[i]; rows the push does not name are copied."""
    w2, s2 = np.array(w), np.array(state)
    dt = w2.dtype
    cols = w2.shape[1]
    assert s2.dtype == dt and s2.shape == (w2.shape[0], 2 * cols)
    grads = np.asarray(grads, dtype=dt).reshape(len(local), cols)
    sums = sum_gradients(local, grads, dt)
    if sums:
        named = np.fromiter(sums, np.int64, len(sums))  # the distinct rows: one step each, all at once
        k = adam_scalars(dt, lr, beta1, beta2, eps, step)
        w2[named], s2[named, :cols], s2[named, cols:] = adam_step(w2[named], s2[named, :cols], s2[named, cols:],
                                                                  np.stack(list(sums.values())), k)
    return w2, s2


# ---- exact arithmetic: what a fused multiply-add would store -------------------------------------------
def round_fraction(x, npd):
    """The rational x rounded once to the type, to nearest even; subnormals kept; no overflow expected."""
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
    n = a / quantum
    k = n.numerator // n.denominator
    rem = n - k
    if rem > Fraction(1, 2) or (rem == Fraction(1, 2) and k % 2):
        k += 1
    val = float(k * quantum)  # exact: k has at most nmant + 2 bits
    assert val <= float(info.max)
    return npd(-val if x < 0 else val)


def fused_states(m, v, G, scalars):
    """{name: (m', v')} with one of the four additions of the moments fused with one of its products:
    fma(b1, m, t2), fma(a1, G, t1), fma(b2, v, t4), fma(a2, q, t3), each computed exactly and rounded once."""
    npd = m.dtype.type
    b1, b2, a1, a2 = scalars[:4]
    t = adam_terms(np.zeros_like(m), m, v, G, scalars)
    F = lambda x: Fraction(float(x))  # noqa: E731
    fma = lambda a, x, y: np.array([round_fraction(F(a) * F(xi) + F(yi), npd)  # noqa: E731
                                    for xi, yi in zip(x.ravel(), y.ravel())], npd).reshape(x.shape)
    return {
        "fma(b1, m, t2)": (fma(b1, m, t["t2"]), t["v2"]),
        "fma(a1, G, t1)": (fma(a1, G, t["t1"]), t["v2"]),
        "fma(b2, v, t4)": (t["m2"], fma(b2, v, t["t4"])),
        "fma(a2, q, t3)": (t["m2"], fma(a2, t["q"], t["t3"])),
    }


@functools.lru_cache(maxsize=None)
def fusion_inputs(npd):
    """(G, m, v), 512 elements each, whose moment sums cancel: G over five decades, m = -(a1 * G) / b1 *
    (1 + delta) and v = -(a2 * G * G) / b2 * (1 + delta) with delta uniform in +-2^-10, so b1 * m + a1 * G
    and b2 * v + a2 * G * G keep only what the products' roundings left. The betas are the defaults at step
    1. A negative v is just bits here. Read-only, shared."""
    npd = np.dtype(npd).type
    rng = np.random.default_rng(zlib.crc32(f"adam/fusion/{np.dtype(npd).name}".encode()))
    n = 512
    b1, b2, a1, a2 = (float(x) for x in adam_scalars(npd, 0.05, BETA1, BETA2, EPS, 1)[:4])
    G = (rng.standard_normal(n) * 10.0 ** rng.integers(-2, 3, n)).astype(npd)
    G[G == 0] = 1
    Gd = G.astype(np.float64)
    delta = rng.uniform(-2.0 ** -10, 2.0 ** -10, (2, n))
    m = (-(a1 * Gd) / b1 * (1 + delta[0])).astype(npd)
    v = (-(a2 * Gd * Gd) / b2 * (1 + delta[1])).astype(npd)
    for a in (G, m, v):
        a.setflags(write=False)
    return G, m, v


# ---- shared inputs of the GPU tests -------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adam_start(dtype_name, size, cols):
    """(w0, state0): random weights, random first moments and |random| second moments; read-only, shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"adam/start/{dtype_name}/{size}/{cols}".encode()))
    w0 = rng.standard_normal((size, cols)).astype(npd)
    s0 = np.concatenate([rng.standard_normal((size, cols)), np.abs(rng.standard_normal((size, cols)))], 1).astype(npd)
    w0.setflags(write=False)
    s0.setflags(write=False)
    return w0, s0


def adam_grads(dtype_name, n, cols, what="case"):
    """(n, cols) gradients over nine decades, so that the order of a sum shows (adagrad_cases' builder under
    this file's own seeds); read-only, shared."""
    return adagrad_inputs(dtype_name, n, cols, f"adam/{what}")


@functools.lru_cache(maxsize=None)
def adam_sweep_inputs(dtype_name, size, cols):
    """The rounding sweep's (m0, v0, G, w0), every row named once, on adagrad_cases.sweep_inputs' plan: v
    spans the type's whole exponent range, subnormals and zero included; G spans +-(2^-60 .. 2^60) for
    double, +-(2^-20 .. 2^20) for float; m is standard normal. The first quarter of the rows takes G near
    the square root of the smallest normal and a subnormal m, against a subnormal v (even rows: a2 * G * G
    and v' subnormal) or a huge one (odd rows: u is tiny and d huge, p subnormal). Read-only, shared."""
    npd = np.dtype(dtype_name).type
    info = np.finfo(npd)
    rng = np.random.default_rng(zlib.crc32(f"adam/sweep/{dtype_name}/{size}/{cols}".encode()))
    shape = (size, cols)
    lo_e, hi_e = info.minexp - info.nmant - 1, info.maxexp - 1
    mant = 1.0 + rng.random(shape)
    with np.errstate(under="ignore"):
        v = np.ldexp(mant, rng.integers(lo_e, hi_e, shape)).astype(npd)
    v[rng.random(shape) < 0.02] = 0
    ge = 60 if npd == np.float64 else 20
    G = (np.ldexp(1.0 + rng.random(shape), rng.integers(-ge, ge, shape)) * rng.choice([-1.0, 1.0], shape)).astype(npd)
    m = rng.standard_normal(shape).astype(npd)
    q = size // 4
    te = info.minexp // 2  # 2^te squared is the smallest normal
    G[:q] = (np.ldexp(1.0 + rng.random((q, cols)), rng.integers(te - 10, te, (q, cols)))
             * rng.choice([-1.0, 1.0], (q, cols))).astype(npd)
    with np.errstate(under="ignore"):
        v[0:q:2] = np.ldexp(mant[0:q:2], rng.integers(lo_e, info.minexp + 2, v[0:q:2].shape)).astype(npd)
        m[:q] = (np.ldexp(mant[:q], rng.integers(info.minexp - info.nmant, info.minexp, (q, cols)))
                 * rng.choice([-1.0, 1.0], (q, cols))).astype(npd)
    v[1:q:2] = np.ldexp(mant[1:q:2], rng.integers(info.maxexp - 8, info.maxexp - 1, v[1:q:2].shape)).astype(npd)
    w = rng.standard_normal(shape).astype(npd)
    w[::3] = 0  # weights that a subnormal p changes
    for a in (m, v, G, w):
        a.setflags(write=False)
    return m, v, G, w


def sweep_premises(npd, m0, v0, G, w0, scalars):
    """Counts the rounding sweep relies on, from the replay alone: subnormal v', subnormal p, quotients s
    with s * rc2 != r and quotients p with p * d != u (a quotient that was rounded)."""
    t = adam_terms(w0, m0, v0, G, scalars)
    tiny = np.finfo(npd).tiny
    sub = lambda a: int(((a != 0) & (np.abs(a) < tiny)).sum())  # noqa: E731
    with np.errstate(**_QUIET):
        inexact_s = int((np.isfinite(t["s"]) & (np.multiply(t["s"], scalars[5], dtype=npd) != t["r"])).sum())
        inexact_p = int((np.isfinite(t["p"]) & np.isfinite(t["d"]) & (np.multiply(t["p"], t["d"], dtype=npd) != t["u"])).sum())
    return dict(sub_v=sub(t["v2"]), sub_p=sub(t["p"]), inexact_s=inexact_s, inexact_p=inexact_p)
