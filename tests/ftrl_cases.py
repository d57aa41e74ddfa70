"""Expected values of the FTRL-proximal row push, shared by test_ftrl_cpu.py and test_gpu_ftrl.py.

Nothing here calls the code under test. A push is replayed by the contract of include/glint_gpu.h, in the
table's dtype: the four scalars rounded once to the type; per distinct row a zero row plus its gradient rows
in push order (adagrad_cases.sum_gradients); then the operations of the step, each one numpy ufunc call
(rounded on its own; numpy's sqrt and divide are IEEE correctly rounded and keep subnormals). The state table
packs z in columns [0, cols) and n in [cols, 2 * cols).

`ftrl_terms(..., alt=NAME)` computes one of the forms the contract rules out (ALTS), for the premises: each
must be told from the contract by the inputs the GPU tests push."""
import functools
import zlib

import numpy as np

from adagrad_cases import adagrad_inputs, assert_bits, bits, sum_gradients  # noqa: F401  (re-exported)
from rowwise_cases import F, round_fraction, round_sqrt  # noqa: F401  (re-exported)

_QUIET = dict(over="ignore", invalid="ignore", under="ignore", divide="ignore")
ALPHA, BETA, L1, L2 = 0.05, 1.0, 0.3, 1e-4  # the scalars of the parity pushes

# the forms of the step that the contract rules out; the two about the whole push (the order of the sum, a
# step per record) are replay_ftrl's `order` and replay_ftrl_per_record
ALTS = ("ds * (1/alpha)", "b * (1/alpha)", "y * (1/d)", "q / (r1 + r0)", "fma(-sg, w, G)", "fma(G, G, n)")


def ftrl_scalars(dt, alpha, beta, l1, l2):
    """(alpha, beta, l1, l2) in the table's type, each rounded once."""
    dt = np.dtype(dt)
    return tuple(dt.type(float(x)) for x in (alpha, beta, l1, l2))


def _fma(a, x, y, npd):
    """round(a * x + y), computed exactly, element by element (small blocks only)."""
    a, x, y = np.broadcast_arrays(a, x, y)
    out = np.empty(x.shape, npd)
    for i in np.ndindex(x.shape):
        if not (np.isfinite(a[i]) and np.isfinite(x[i]) and np.isfinite(y[i])):
            with np.errstate(**_QUIET):
                out[i] = npd(a[i]) * npd(x[i]) + npd(y[i])
        else:
            out[i] = round_fraction(F(a[i]) * F(x[i]) + F(y[i]), npd)
    return out


def ftrl_terms(w, z, n, G, scalars, alt=None):
    """Every named value of the contract's step 2 for a block, as a dict; each operation one ufunc call.
    `alt` replaces one operation by a form the contract rules out (one of ALTS)."""
    w, z, n, G = (np.asarray(a) for a in (w, z, n, G))
    dt = w.dtype
    npd = dt.type
    alpha, beta, l1, l2 = scalars
    assert all(type(x) is npd for x in scalars) and alt in (None,) + ALTS
    with np.errstate(**_QUIET):
        q = np.multiply(G, G, dtype=dt)
        n2 = np.add(n, q, dtype=dt) if alt != "fma(G, G, n)" else _fma(G, G, n, npd)
        r0 = np.sqrt(n, dtype=dt)
        r1 = np.sqrt(n2, dtype=dt)
        if alt == "q / (r1 + r0)":
            ds = np.divide(q, np.add(r1, r0, dtype=dt), dtype=dt)
        else:
            ds = np.subtract(r1, r0, dtype=dt)
        if alt == "ds * (1/alpha)":
            sg = np.multiply(ds, np.divide(npd(1), alpha, dtype=dt), dtype=dt)
        else:
            sg = np.divide(ds, alpha, dtype=dt)
        if alt == "fma(-sg, w, G)":
            t = np.multiply(sg, w, dtype=dt)
            u = _fma(np.negative(sg), w, G, npd)
        else:
            t = np.multiply(sg, w, dtype=dt)
            u = np.subtract(G, t, dtype=dt)
        z2 = np.add(z, u, dtype=dt)
        a = np.abs(z2)
        s = np.copysign(l1, z2)
        y = np.subtract(z2, s, dtype=dt)
        b = np.add(beta, r1, dtype=dt)
        if alt == "b * (1/alpha)":
            c = np.multiply(b, np.divide(npd(1), alpha, dtype=dt), dtype=dt)
        else:
            c = np.divide(b, alpha, dtype=dt)
        d = np.add(c, l2, dtype=dt)
        if alt == "y * (1/d)":
            e = np.multiply(y, np.divide(npd(1), d, dtype=dt), dtype=dt)
        else:
            e = np.divide(y, d, dtype=dt)
        zero = np.less_equal(a, l1)  # false for a NaN z'
        w2 = np.where(zero, npd(0), np.negative(e)).astype(dt)
    return dict(q=q, n2=n2, r0=r0, r1=r1, ds=ds, sg=sg, t=t, u=u, z2=z2, a=a, s=s, y=y, b=b, c=c, d=d, e=e,
                zero=zero, w2=w2)


def ftrl_step(w, z, n, G, scalars, alt=None):
    """(w', z', n') of one row (or any broadcastable block)."""
    t = ftrl_terms(w, z, n, G, scalars, alt)
    return t["w2"], t["z2"], t["n2"]


def replay_ftrl(w, state, local, grads, alpha, beta=BETA, l1=0.0, l2=0.0, alt=None, order=None):
    """(w', state') of tables w (size, cols) and state (size, 2 * cols) after one push of gradient row i to
    row local[i]; rows the push does not name are copied. `order` sums the records in another order and
    `alt` takes another form of the step: the premises' alternatives, never the contract."""
    w2, s2 = np.array(w), np.array(state)
    dt = w2.dtype
    cols = w2.shape[1]
    assert s2.dtype == dt and s2.shape == (w2.shape[0], 2 * cols)
    grads = np.asarray(grads, dtype=dt).reshape(len(local), cols)
    sums = sum_gradients(local, grads, dt, order)
    if sums:
        named = np.fromiter(sums, np.int64, len(sums))  # the distinct rows: one step each, all at once
        k = ftrl_scalars(dt, alpha, beta, l1, l2)
        w2[named], s2[named, :cols], s2[named, cols:] = ftrl_step(w2[named], s2[named, :cols], s2[named, cols:],
                                                                  np.stack(list(sums.values())), k, alt)
    return w2, s2


def replay_ftrl_per_record(w, state, local, grads, alpha, beta=BETA, l1=0.0, l2=0.0):
    """What the contract rules out: one step per record, in push order, instead of one per distinct row."""
    w2, s2 = np.array(w), np.array(state)
    dt = w2.dtype
    cols = w2.shape[1]
    grads = np.asarray(grads, dtype=dt).reshape(len(local), cols)
    k = ftrl_scalars(dt, alpha, beta, l1, l2)
    for i, l in enumerate(local):
        w2[l], s2[l, :cols], s2[l, cols:] = ftrl_step(w2[l], s2[l, :cols], s2[l, cols:], grads[i], k)
    return w2, s2


# ---- shared inputs of the GPU tests -------------------------------------------------------------------
def _frozen(*arrays):
    for a in arrays:
        a.setflags(write=False)
    return arrays


@functools.lru_cache(maxsize=None)
def ftrl_start(dtype_name, size, cols):
    """(w0, state0): random weights, random z and |random| n; read-only, shared. The weights are no
    function of (z, n): the step reads them as they are."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"ftrl/start/{dtype_name}/{size}/{cols}".encode()))
    w0 = rng.standard_normal((size, cols)).astype(npd)
    s0 = np.concatenate([rng.standard_normal((size, cols)), np.abs(rng.standard_normal((size, cols)))], 1).astype(npd)
    return _frozen(w0, s0)


def ftrl_grads(dtype_name, n, cols, what="case"):
    """(n, cols) gradients over nine decades, so that the order of a sum shows (adagrad_cases' builder under
    this file's own seeds); read-only, shared."""
    return adagrad_inputs(dtype_name, n, cols, f"ftrl/{what}")


TH_L1, TH_L2 = 0.5, 0.25  # the threshold pushes' l1 (exact in both types, so that z = +-l1 is) and l2


@functools.lru_cache(maxsize=None)
def threshold_inputs(dtype_name, size, cols):
    """(w0, state0, local, grads) of the threshold push, with l1 = TH_L1: every row named, some twice. z and
    the gradients are of l1's size, so |z'| falls on both sides of it and z' takes both signs. Row 0 sits
    exactly on the threshold: z = +l1 in the even columns and -l1 in the odd ones, w = 0 and a gradient of
    zeros, so z' = z and |z'| == l1. Row 1 is the same with the gradient +-0 twice. Read-only, shared."""
    npd = np.dtype(dtype_name).type
    rng = np.random.default_rng(zlib.crc32(f"ftrl/threshold/{dtype_name}/{size}/{cols}".encode()))
    w0 = (0.1 * rng.standard_normal((size, cols))).astype(npd)
    z0 = (TH_L1 * rng.standard_normal((size, cols))).astype(npd)
    n0 = np.abs(rng.standard_normal((size, cols))).astype(npd)
    body = rng.permutation(np.concatenate([np.arange(2, size), rng.integers(2, size, size // 2)]))
    local = np.concatenate([[0, 1], body, [1]]).astype(np.int64)
    grads = (0.3 * TH_L1 * rng.standard_normal((local.size, cols))).astype(npd)
    for r in (0, 1):
        w0[r] = 0
        z0[r, 0::2], z0[r, 1::2] = TH_L1, -TH_L1
        grads[local == r] = 0
    grads[-1] = -0.0  # row 1's second record: +0 + -0 is +0
    assert local[0] == 0 and local[1] == 1 and local[-1] == 1
    return _frozen(w0, np.concatenate([z0, n0], 1), local, grads)


@functools.lru_cache(maxsize=None)
def fusion_inputs(npd):
    """(G, w, z, n), 512 elements each, whose sum G - sg * w cancels: G over five decades, n = G * G times a
    factor in [1/4, 4) (so that n + G * G rounds twice where a fused add rounds once), and w = G / sg * (1 +
    delta) with delta uniform in +-2^-10, sg being the contract's own (it does not depend on w), so G - sg *
    w keeps only what the product's rounding left. The scalars are ALPHA, BETA, L1, L2. Read-only, shared."""
    npd = np.dtype(npd).type
    rng = np.random.default_rng(zlib.crc32(f"ftrl/fusion/{np.dtype(npd).name}".encode()))
    size = 512
    G = (rng.standard_normal(size) * 10.0 ** rng.integers(-2, 3, size)).astype(npd)
    G[G == 0] = 1
    Gd = G.astype(np.float64)
    n = (Gd * Gd * rng.uniform(0.25, 4.0, size)).astype(npd)
    sg = ftrl_terms(np.zeros_like(G), np.zeros_like(G), n, G, ftrl_scalars(npd, ALPHA, BETA, L1, L2))["sg"]
    assert (sg > 0).all()
    w = (Gd / sg.astype(np.float64) * (1 + rng.uniform(-2.0 ** -10, 2.0 ** -10, size))).astype(npd)
    z = rng.standard_normal(size).astype(npd)
    return _frozen(G, w, z, n)


def sweep_scalars(npd, tiny_l1):
    """The rounding sweep's two settings: l1 = l2 = 0, or a tiny l1 (2^-5 of the square root of the smallest
    normal, inside the band of the first quarter's gradients: both sides of the threshold among the smallest
    z') with l2 = 2^-20. In doubles, as the call takes them."""
    tiny = float(np.ldexp(1.0, int(np.finfo(npd).minexp) // 2 - 5))
    return (ALPHA, BETA, tiny, 2.0 ** -20) if tiny_l1 else (ALPHA, BETA, 0.0, 0.0)


@functools.lru_cache(maxsize=None)
def ftrl_sweep_inputs(dtype_name, size, cols):
    """The rounding sweep's (w0, z0, n0, G), every row named once, on adagrad_cases.sweep_inputs' plan: n
    spans the type's whole exponent range, subnormals and zero included; G spans +-(2^-60 .. 2^60) for
    double, +-(2^-20 .. 2^20) for float; z is standard normal. The first quarter of the rows takes G near
    the square root of the smallest normal and a subnormal z, against a subnormal n (even rows: G * G and
    n' subnormal) or a huge one (odd rows: y is tiny and d huge, e subnormal). Read-only, shared."""
    npd = np.dtype(dtype_name).type
    info = np.finfo(npd)
    rng = np.random.default_rng(zlib.crc32(f"ftrl/sweep/{dtype_name}/{size}/{cols}".encode()))
    shape = (size, cols)
    lo_e, hi_e = info.minexp - info.nmant - 1, info.maxexp - 1
    mant = 1.0 + rng.random(shape)
    with np.errstate(under="ignore"):
        n = np.ldexp(mant, rng.integers(lo_e, hi_e, shape)).astype(npd)
    n[rng.random(shape) < 0.02] = 0
    ge = 60 if npd == np.float64 else 20
    G = (np.ldexp(1.0 + rng.random(shape), rng.integers(-ge, ge, shape)) * rng.choice([-1.0, 1.0], shape)).astype(npd)
    z = rng.standard_normal(shape).astype(npd)
    q = size // 4
    te = info.minexp // 2  # 2^te squared is the smallest normal
    G[:q] = (np.ldexp(1.0 + rng.random((q, cols)), rng.integers(te - 10, te, (q, cols)))
             * rng.choice([-1.0, 1.0], (q, cols))).astype(npd)
    with np.errstate(under="ignore"):
        n[0:q:2] = np.ldexp(mant[0:q:2], rng.integers(lo_e, info.minexp + 2, n[0:q:2].shape)).astype(npd)
        z[:q] = (np.ldexp(mant[:q], rng.integers(info.minexp - info.nmant, info.minexp, (q, cols)))
                 * rng.choice([-1.0, 1.0], (q, cols))).astype(npd)
    n[1:q:2] = np.ldexp(mant[1:q:2], rng.integers(info.maxexp - 8, info.maxexp - 1, n[1:q:2].shape)).astype(npd)
    w = rng.standard_normal(shape).astype(npd)
    w[::3] = 0
    return _frozen(w, z, n, G)


def sweep_premises(npd, w0, z0, n0, G, scalars):
    """Counts the rounding sweep relies on, from the replay alone: subnormal n', subnormal e, quotients sg
    with sg * alpha != ds and quotients e with e * d != y (a quotient that was rounded)."""
    t = ftrl_terms(w0, z0, n0, G, scalars)
    tiny = np.finfo(npd).tiny
    sub = lambda a: int(((a != 0) & (np.abs(a) < tiny)).sum())  # noqa: E731
    with np.errstate(**_QUIET):
        inexact_sg = int((np.isfinite(t["sg"]) & (np.multiply(t["sg"], scalars[0], dtype=npd) != t["ds"])).sum())
        inexact_e = int((np.isfinite(t["e"]) & np.isfinite(t["d"])
                         & (np.multiply(t["e"], t["d"], dtype=npd) != t["y"])).sum())
    return dict(sub_n=sub(t["n2"]), sub_e=sub(t["e"]), inexact_sg=inexact_sg, inexact_e=inexact_e)


# ---- what the GPU tests push, for the premises --------------------------------------------------------
SIZE = 48        # rows of the GPU tests' shards
SWEEP_COLS = 128


@functools.lru_cache(maxsize=None)
def duplicates_push(dtype_name, cols=67):
    """(w0, state0, local, grads) of the parity grid's `duplicates` pattern at `cols`: 300 records over 12 of
    the SIZE rows, gradients over nine decades."""
    rng = np.random.default_rng(zlib.crc32(f"ftrl/duplicates/{dtype_name}/{cols}".encode()))
    local = rng.choice(rng.choice(SIZE, 12, replace=False), 300).astype(np.int64)
    w0, s0 = ftrl_start(dtype_name, SIZE, cols)
    return w0, s0, _frozen(local)[0], ftrl_grads(dtype_name, 300, cols)
