"""Inputs and references of the narrow-format row transport, shared by test_wire_cpu.py and test_gpu_wire.py
(a plain helper module, pure numpy; torch only inside the two device helpers).

Nothing here calls the code under test. The references are numpy's own conversions -- ``astype(np.float16)``
for Float -> F16, ``astype(np.float32)`` for Double -> F32 and for both IEEE widenings -- and, because numpy
has no bfloat16, ``bf16_narrow`` / ``bf16_widen`` below: the rule of include/glint_gpu.h written out a second
time, independently of glint_amd.to_bfloat16 (test_wire_cpu.py holds the two to each other and to known
answers).

A pair is (shard dtype name, wire name). Host arrays of a wire type are np.float16, np.uint16 (bfloat16 bit
patterns) or np.float32."""
import functools

import numpy as np

PAIRS = [("float", "float16"), ("float", "bfloat16"), ("double", "float32")]
NPV = {"float": np.float32, "double": np.float64}                     # the shard side
NPW = {"float16": np.float16, "bfloat16": np.uint16, "float32": np.float32}  # the wire side, as host arrays
UINT = {2: np.uint16, 4: np.uint32, 8: np.uint64}
# (exponent bits, mantissa bits) of a wire type
FIELDS = {"float16": (5, 10), "bfloat16": (8, 7), "float32": (8, 23)}


def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype.itemsize])


def from_bits(u, npd):
    return np.ascontiguousarray(u).view(npd)


# ---- references ---------------------------------------------------------------------------------------------
def bf16_narrow(x):
    """float32 -> bfloat16 patterns: (u + 0x7FFF + ((u >> 16) & 1)) >> 16 on the bits; a NaN -> some NaN."""
    u = bits(np.asarray(x, np.float32)).astype(np.int64)
    r = (u + 0x7FFF + ((u >> 16) & 1)) >> 16
    nan = (u & 0x7FFFFFFF) > 0x7F800000
    return np.where(nan, 0x7FC0, r).astype(np.uint16)


def bf16_widen(b):
    return (np.asarray(b, np.uint16).astype(np.uint32) * np.uint32(65536)).view(np.float32)


def ref_narrow(x, wire):
    """V array -> the wire type's host array, numpy's rounding (BF16: the integer rule)."""
    x = np.asarray(x)
    assert x.dtype == (np.float64 if wire == "float32" else np.float32)
    if wire == "bfloat16":
        return bf16_narrow(x)
    with np.errstate(over="ignore", under="ignore", invalid="ignore"):
        return x.astype(NPW[wire])


def ref_widen(w, wire):
    """wire host array -> the equal V values (exact)."""
    w = np.asarray(w)
    assert w.dtype == NPW[wire]
    if wire == "bfloat16":
        return bf16_widen(w)
    with np.errstate(invalid="ignore"):
        return w.astype(np.float64 if wire == "float32" else np.float32)


def wire_isnan(w, wire):
    return np.isnan(ref_widen(w, wire))


def assert_wire_bits(got, exp, wire, what=""):
    """Bit for bit; a NaN is compared by class (axpy_cases.assert_bits's rule, on wire arrays)."""
    got, exp = np.asarray(got), np.asarray(exp)
    assert got.dtype == exp.dtype == NPW[wire] and got.shape == exp.shape, what
    nan = wire_isnan(exp, wire)
    np.testing.assert_array_equal(wire_isnan(got, wire), nan, err_msg=what)
    np.testing.assert_array_equal(np.where(nan, 0, bits(got)), np.where(nan, 0, bits(exp)), err_msg=what)


# ---- inputs -------------------------------------------------------------------------------------------------
def _f32_patterns():
    """Every exponent (0 .. 255) times the mantissas {0, 1, 0x400000, 0x7FFFFF} and 8 seeded random ones, in
    both signs: zeros, subnormals, every binade, infinities, quiet and signalling NaNs. 6144 patterns."""
    rng = np.random.default_rng(20_250_117)
    man = np.concatenate([np.array([0, 1, 0x400000, 0x7FFFFF], np.uint32),
                          rng.integers(2, 0x7FFFFF, 8, dtype=np.uint32)])
    exp = np.arange(256, dtype=np.uint32)
    mag = ((exp[:, None] << np.uint32(23)) | man[None, :]).reshape(-1)
    return np.concatenate([mag, mag | np.uint32(0x80000000)])


@functools.lru_cache(maxsize=None)
def widen_all(wire):
    """What a push is tried on, as a wire host array: all 65 536 patterns of F16 / BF16; for F32 the 6144
    patterns of _f32_patterns. Read-only."""
    if wire == "float32":
        out = from_bits(_f32_patterns(), np.float32)
    else:
        out = from_bits(np.arange(65536, dtype=np.uint16), NPW[wire])
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def narrow_set(wire):
    """What a pull is tried on, as a V array. For every non-negative finite W value a with successor b (the
    successor of the largest finite value is the next power of two): a, the midpoint (a + b) / 2 -- exact in V,
    a tie -- and the V neighbours just below and just above the midpoint, in both signs; plus V subnormals, V's
    largest finite value, +/-inf, +/-0 and a NaN. F16 and BF16: every such a (about 256 000 values). F32 has
    2^31 - 2^23 of them, so there a runs over the non-negative finite patterns of _f32_patterns -- every
    binade with its first, second, middle and last value and 8 random ones -- and over the 4096 values at
    each end of the subnormal range and below the largest finite value. Read-only."""
    E, M = FIELDS[wire]
    npv = np.float64 if wire == "float32" else np.float32
    uv = UINT[np.dtype(npv).itemsize]
    top = ((1 << E) - 1) << M  # the infinity's pattern: finite patterns lie below it
    if wire == "float32":
        p = _f32_patterns().astype(np.int64)
        a_bits = np.unique(np.concatenate([p[p < top], np.arange(0, 4096), np.arange(0x800000 - 4096, 0x800000 + 4096),
                                           np.arange(top - 4096, top)]))
    else:
        a_bits = np.arange(top, dtype=np.int64)
    wdt = NPW[wire]
    uw = UINT[np.dtype(wdt).itemsize]
    # a, b and the midpoint in double first (2^128, the successor of BF16's largest value, is no float)
    a = ref_widen(from_bits(a_bits.astype(uw), wdt), wire).astype(np.float64)
    b = np.empty_like(a)
    nxt = a_bits + 1
    fin = nxt < top
    b[fin] = ref_widen(from_bits(nxt[fin].astype(uw), wdt), wire)
    b[~fin] = 2.0 ** (1 << (E - 1))  # the next power of two past the largest finite value: 2^(emax + 1)
    mid64 = (a + b) / 2
    assert ((mid64 - a) == (b - mid64)).all() and (a < mid64).all() and (mid64 < b).all()  # exact in double
    mid = mid64.astype(npv)
    assert (mid.astype(np.float64) == mid64).all()  # ... and in V: a tie
    a = a.astype(npv)
    below = from_bits(bits(mid) - uv(1), npv)
    above = from_bits(bits(mid) + uv(1), npv)
    assert (a < below).all() and (below < mid).all() and (mid < above).all() and (above < b).all()
    fi = np.finfo(npv)
    sub = fi.smallest_subnormal
    extra = np.array([sub, sub * 3, fi.smallest_normal - sub, fi.smallest_normal, fi.max, np.inf, 0.0, np.nan], npv)
    pos = np.concatenate([a, mid, below, above, extra])
    out = np.concatenate([pos, -pos])
    out.setflags(write=False)
    return out


def padded(x, cols):
    """x as rows of `cols`, the last row filled up with zeros."""
    rows = -(-x.size // cols)
    out = np.zeros(rows * cols, x.dtype)
    out[:x.size] = x
    return out.reshape(rows, cols)


# ---- device tensors of a wire type (torch has no from_numpy for uint16 patterns of bfloat16) ------------------
def torch_wire(wire):
    import torch
    return getattr(torch, wire)


def to_dev(gpu, w, wire):
    """A wire host array as a device tensor of the wire's torch dtype, the same bits."""
    import torch
    w = np.ascontiguousarray(w)
    assert w.dtype == NPW[wire]
    raw = {2: np.int16, 4: np.int32}[w.dtype.itemsize]
    t = torch.from_numpy(w.view(raw).copy()).to(torch.device("cuda", gpu))
    return t.view(torch_wire(wire))


def from_dev(t, wire):
    """A device tensor of a wire type back as the wire host array, the same bits."""
    import torch
    raw = {2: torch.int16, 4: torch.int32}[t.element_size()]
    return t.contiguous().view(raw).cpu().numpy().view(NPW[wire])
