"""IEEE-754 edge-value cases for the push and pull paths (a plain helper module, pure numpy).

Every case is deterministic from a seed string. Three kinds:

* ``exact_grid`` -- every value is an integer multiple ``k * 2^exponent`` (|k| <= kmax) and, per
  element, the magnitudes of everything ever pushed sum to at most 2^24 (Float) / 2^53 (Double) units.
  Then every partial sum in every association is exactly representable -- also in a ``double``
  accumulator that is rounded to ``float`` once at the end -- so a correct push gives the expected bits
  whatever order it added in. The expectation comes from integer arithmetic, scaled once.
* ``nonfinite`` -- a few dozen chosen elements get, among ordinary exact-grid traffic everywhere,
  addends whose class (+inf, -inf, NaN) is the same in every order. Everything else stays bit-exact.
* ``ordered_case`` -- vectors whose result is defined by the sequential order only
  (``ordered_vectors``), each on its own element, mixed into exact-grid traffic and a non-finite set.

``GRIDS`` names the exponents: ``subnormal`` (every sum stays subnormal), ``crossing`` (every addend is
subnormal -- kmax * 2^exponent is below the smallest normal -- while a sum of 16 units is normal),
``unit`` and ``top`` (near the overflow limit).
"""
import ctypes as C
import functools
import zlib
from typing import NamedTuple

import numpy as np

NPD = {"float": np.float32, "double": np.float64}
UINT = {np.dtype(np.float32): np.uint32, np.dtype(np.float64): np.uint64}
LIMIT = {"float": 1 << 24, "double": 1 << 53}  # units an element's magnitudes may sum to
GRIDS = {"float": {"subnormal": -149, "crossing": -130, "unit": 0, "top": 100},
         "double": {"subnormal": -1074, "crossing": -1026, "unit": 0, "top": 960}}
KMAX = 8
EXACT, PINF, NINF, NAN = 0, 1, 2, 3  # class map entries

# what a chosen element receives -> its class in any order (finite traffic is added to all of them)
RECIPES = [(["+inf", 1.0], PINF), (["-inf", -5.0], NINF), (["+inf", "-inf"], NAN), (["nan"], NAN),
           (["+max", "+max", "+max"], PINF), (["-max", "-max", "-max"], NINF), (["-nan", 2.0], NAN)]
# ... when the path allows one record per element and push (increasing unique keys)
RECIPES_UNIQUE = [(["+inf"], PINF), (["-inf"], NINF), (["nan"], NAN), (["-nan"], NAN)]


def rng_for(*parts):
    return np.random.default_rng(zlib.crc32("/".join(str(p) for p in parts).encode()))


def special(name, dtype):
    """A named edge value (or a plain number) in the shard's type. The NaNs carry a payload."""
    npd = NPD[dtype]
    if not isinstance(name, str):
        return npd(name)
    f32 = npd == np.float32
    bits = {"nan": 0x7FC00001 if f32 else 0x7FF8000000000123, "-nan": 0xFFC00002 if f32 else 0xFFF8000000000456}
    if name in bits:
        return np.array([bits[name]], UINT[np.dtype(npd)]).view(npd)[0]
    sign = -1 if name[0] == "-" else 1
    return npd(sign * (np.inf if name[1:] == "inf" else np.finfo(npd).max))


def scale(k, exponent, dtype):
    """k * 2^exponent in the shard's type; asserts that every value is finite and exactly k units."""
    k = np.asarray(k, np.int64)
    v = np.ldexp(k.astype(np.float64), exponent).astype(NPD[dtype])
    assert np.abs(k).max(initial=0) <= 1 << 53 and np.isfinite(v).all()
    assert np.array_equal(np.ldexp(v.astype(np.float64), -exponent), k.astype(np.float64)), "not representable"
    return v


# ---- key patterns ----------------------------------------------------------------------------------
def pattern_keys(rng, pattern, n, size):
    """(ordered prefix, rest) of local keys. The rest may be permuted and mixed with further records."""
    none = np.zeros(0, np.int64)
    if isinstance(pattern, np.ndarray):
        return pattern.astype(np.int64), none
    if pattern == "dense":  # increasing unique keys that end at the shard's last element
        assert n <= size
        return np.arange(size - n, size, dtype=np.int64), none
    if pattern == "dups":  # duplicates on 64 keys
        hot = rng.choice(size, 64, replace=False)
        return none, rng.choice(hot, n).astype(np.int64)
    if pattern == "prefix_tail":  # an increasing prefix, then an unordered tail
        h = n // 2
        assert 2 * h <= size
        return np.arange(0, 2 * h, 2, dtype=np.int64), rng.integers(0, size, n - h)
    if pattern == "uniform":
        return none, rng.integers(0, size, n)
    if pattern == "binned":  # 15 : 10 : 6 -- uniform, one key, 300 keys of one slab (the hot-slab split)
        n_one, n_slab = n * 10 // 31, n * 6 // 31
        lo = 4096 if size >= 8192 else 0
        slab = lo + rng.choice(min(4096, size - lo), min(300, size - lo), replace=False)
        return none, np.concatenate([rng.integers(0, size, n - n_one - n_slab),
                                     np.full(n_one, rng.integers(0, size)), rng.choice(slab, n_slab)])
    if pattern == "rows":  # one row 300 times, every row once, some twice
        assert n >= 300 + size
        return none, np.concatenate([np.full(300, rng.integers(0, size)), rng.permutation(size),
                                     rng.choice(size, n - 300 - size, replace=n - 300 - size > size)])
    raise ValueError(pattern)


def _name(pattern):
    return pattern if isinstance(pattern, str) else f"keys{pattern.size}"


def _sums(keys, k, size, width):
    sums, mags = np.zeros((size, width), np.int64), np.zeros((size, width), np.int64)
    np.add.at(sums, keys, k)
    np.add.at(mags, keys, np.abs(k))
    return sums, mags


def _grid(dtype, exponent, keys_pattern, n, size, kmax, seed, width):
    rng = rng_for("grid", dtype, exponent, _name(keys_pattern), n, size, kmax, seed, width)
    prefix, rest = pattern_keys(rng, keys_pattern, n, size)
    keys = np.concatenate([prefix, rng.permutation(rest)]).astype(np.int64)
    k = rng.integers(-kmax, kmax + 1, (keys.size, width))
    return (keys, scale(k, exponent, dtype)) + _sums(keys, k, size, width)


def exact_grid(dtype, exponent, keys_pattern, n, size, kmax=KMAX, pushes=2, seed="", width=1):
    """``(keys, vals, expect)``: n records ``k * 2^exponent`` on local keys of a ``size``-element shard,
    and the exact content after 1 .. ``pushes`` pushes of them onto zeros, ``expect[p - 1]``.
    ``width`` > 1: a row push, ``vals`` is (n, width) and ``expect`` (pushes, size * width)."""
    keys, vals, sums, mags = _grid(dtype, exponent, keys_pattern, n, size, kmax, seed, width)
    assert mags.max(initial=0) * pushes <= LIMIT[dtype], "outside the exactness condition"
    expect = np.stack([scale(sums * p, exponent, dtype).reshape(-1) for p in range(1, pushes + 1)])
    return keys, (vals if width > 1 else vals.reshape(-1)), expect


# ---- non-finite ------------------------------------------------------------------------------------
def chosen_elements(rng, elems, cols=0, extra=24, avoid=()):
    """Flat element indices, no two adjacent: element 0, the last one, one even and one odd member of
    two aligned pairs, one element on each side of a 4096-element slab boundary (at different
    boundaries, so that both neighbours across the boundary stay finite), for a matrix one element in
    column 0 and one in the last column, and ``extra`` random ones."""
    must = [0, elems - 1, 10, 21]
    if elems > 4100:
        must.append(4095)
    if elems > 8200:
        must.append(8192)
    if cols:
        must += [5 * cols, 8 * cols - 1]
    taken = set(avoid)
    out = []
    for e in must + [int(e) for e in rng.permutation(elems)[:4 * extra + 64]]:
        if len(out) >= len(must) + extra:
            break
        if 0 <= e < elems and not ({e - 1, e, e + 1} & taken):
            out.append(e)
            taken.add(e)
    assert all(m in out for m in must), "shard too small for the required elements"
    return out


def _assemble(rng, dtype, exponent, prefix, rest, specials, size, width, kmax):
    """Records of the prefix, then the rest mixed with the special records at random positions; the
    addends of a special marked ``ordered`` keep their order. A special is (element, addends, ordered):
    each addend one record on key element // width whose column element % width holds it.
    Returns keys, vals, and the integer sums / magnitudes of everything but the special cells."""
    s_keys, s_col, s_val, groups = [], [], [], []
    for e, addends, ordered in specials:
        at = len(s_keys)
        for a in addends:
            s_keys.append(e // width)
            s_col.append(e % width)
            s_val.append(special(a, dtype))
        if ordered:
            groups.append(np.arange(at, len(s_keys)) + rest.size)
    mixed = np.concatenate([rest, np.array(s_keys, np.int64)]).astype(np.int64)
    pos = rng.random(mixed.size)
    for g in groups:
        pos[g] = np.sort(pos[g])
    order = np.argsort(pos, kind="stable")
    keys = np.concatenate([prefix, mixed[order]]).astype(np.int64)
    k = rng.integers(-kmax, kmax + 1, (keys.size, width))
    vals = scale(k, exponent, dtype)
    where = np.empty(mixed.size, np.int64)
    where[order] = np.arange(mixed.size) + prefix.size  # record index of mixed[i]
    sp = where[rest.size:]
    k[sp, s_col] = 0
    vals[sp, s_col] = np.array(s_val, NPD[dtype]) if s_val else 0
    sums, mags = _sums(keys, k, size, width)
    return keys, vals, sums, mags


class NonFinite(NamedTuple):
    pushes: list        # [(keys, vals), (keys, vals)]: the non-finite push, then one of ordinary values
    expect: np.ndarray  # (2, elements): the exact content after each push (chosen elements: ignored)
    cls: np.ndarray     # (elements,) int8: EXACT, or the class a chosen element must have


def nonfinite(dtype, keys_pattern, n, size, seed="", width=1, cols=0, unique=False):
    """n records in all (exact-grid traffic at 2^0 plus the chosen elements' addends). ``cols``: the
    flat elements are (row, col) cells of a matrix with that many columns (``width`` = cols for a row
    push, 1 for triplets). ``unique``: the pattern allows one record per key -- a chosen element's
    record is replaced, and only single-addend recipes are used."""
    rng = rng_for("nonfinite", dtype, _name(keys_pattern), n, size, seed, width, cols, unique)
    elems = size * width
    assert cols or elems % 2 == 1, "the last element of an odd-sized shard"
    chosen = chosen_elements(rng, elems, cols)
    cls = np.zeros(elems, np.int8)
    recipes = RECIPES_UNIQUE if unique else RECIPES
    specials = [(e, *recipes[i % len(recipes)]) for i, e in enumerate(chosen)]
    if unique:
        assert width == 1
        prefix, rest = pattern_keys(rng, keys_pattern, n, size)
        assert rest.size == 0
        keys = prefix
        k = rng.integers(-KMAX, KMAX + 1, (keys.size, 1))
        vals = scale(k, 0, dtype)
        for e, addends, c in specials:
            i = np.searchsorted(keys, e)
            if i < keys.size and keys[i] == e:  # (a key the pattern leaves out keeps its exact zero)
                k[i], vals[i], cls[e] = 0, special(addends[0], dtype), c
        sums, mags = _sums(keys, k, size, 1)
    else:
        nsp = sum(len(a) for _, a, _ in specials)
        prefix, rest = pattern_keys(rng, keys_pattern, n - nsp, size)
        keys, vals, sums, mags = _assemble(rng, dtype, 0, prefix, rest, [(e, a, False) for e, a, _ in specials],
                                           size, width, KMAX)
        for e, _, c in specials:
            cls[e] = c
    keys2, vals2, sums2, mags2 = _grid(dtype, 0, keys_pattern, n, size, KMAX, f"{seed}/second", width)
    vals2 = vals2 if width > 1 else vals2.reshape(-1)
    assert (mags + mags2).max() <= LIMIT[dtype], "outside the exactness condition"
    expect = np.stack([scale(sums, 0, dtype).reshape(-1), scale(sums + sums2, 0, dtype).reshape(-1)])
    return NonFinite([(keys, vals if width > 1 else vals.reshape(-1)), (keys2, vals2)], expect, cls)


# ---- ordered-only vectors ----------------------------------------------------------------------------
def ordered_vectors(dtype):
    """(start value, addends in message order): defined by the sequential order only."""
    return [(0.0, ["+max", "+max", "-max"]),   # inf; summed in a wider type, or -max first: MAX
            (0.0, ["+max", "-max", "+max"]),   # MAX
            (0.0, ["-max", "-max", "+max"]),   # -inf
            (-0.0, [-0.0, -0.0]),              # -0.0: the start value's sign survives only (-0) + (-0)
            (-0.0, [0.0])]                     # +0.0


def sequential(d0, addends, dtype, acc_type=None):
    """The JVM's loop ``data(k) += v`` in the shard's type (``acc_type``: a fold that accumulates in
    another type and rounds to the shard's type once, for the CPU tests' alternatives)."""
    npd = NPD[dtype]
    at = acc_type or npd
    acc = at(special(d0, dtype))
    with np.errstate(over="ignore", invalid="ignore"):
        for v in addends:
            acc = at(acc + at(special(v, dtype)))
        return npd(acc)


def presummed(d0, addends, dtype):
    """start + (the addends summed first), the fold a pre-reducing kernel would compute."""
    npd = NPD[dtype]
    with np.errstate(over="ignore", invalid="ignore"):
        s = npd(0)
        for v in reversed(addends):
            s = npd(s + special(v, dtype))
        return npd(special(d0, dtype) + s)


class Ordered(NamedTuple):
    keys: np.ndarray
    vals: np.ndarray    # (n,) or (n, width)
    init: np.ndarray    # (elements,): the shard's start image (-0.0 where a vector starts from it)
    expect: np.ndarray  # (elements,): after the one push, in message order
    cls: np.ndarray


def vector_elems(width):
    """One element per ordered vector; every other record stays off their keys (rows). Vectors: 30, 33,
    ... (both members of pairs, apart); row pushes: rows 10, 11, ... at different columns."""
    return [30 + 3 * i if width == 1 else (10 + i) * width + 3 * i % width for i in range(5)]


def ordered_case(dtype, n, size, chain=0, seed="", width=1, cols=0, hot_row=0):
    """One message of n records: the ordered vectors, each on its own element with its addends in order
    at random places in the message; a non-finite set; exact traffic on the subnormal grid everywhere
    else, ``chain`` records of it on one key (``hot_row``: as many whole-row records on one row)."""
    rng = rng_for("ordered", dtype, n, size, chain, seed, width, cols, hot_row)
    exponent = GRIDS[dtype]["subnormal"]
    elems = size * width
    vecs = ordered_vectors(dtype)
    velems = vector_elems(width)
    specials = [(e, a, True) for e, (_, a) in zip(velems, vecs)]
    vkeys = {e // width for e in velems}
    avoid = {k * width + c for k in vkeys for c in range(width)}
    chosen = chosen_elements(rng, elems, cols, extra=8, avoid=avoid)
    chosen = [e for e in chosen if e // width not in vkeys]
    assert {0, elems - 1} <= set(chosen)
    specials += [(e, *RECIPES[i % len(RECIPES)][:1], False) for i, e in enumerate(chosen)]
    nsp = sum(len(a) for _, a, _ in specials)
    allowed = np.setdiff1d(np.arange(size), np.array(sorted(vkeys)))
    quiet = np.setdiff1d(allowed, np.array(chosen) // width)
    hot = quiet[rng.integers(0, quiet.size)]
    n_hot = chain + hot_row
    rest = np.concatenate([allowed[rng.integers(0, allowed.size, n - nsp - n_hot)], np.full(n_hot, hot)])
    keys, vals, sums, mags = _assemble(rng, dtype, exponent, np.zeros(0, np.int64), rest, specials, size, width, KMAX)
    assert keys.size == n and mags.max() <= LIMIT[dtype]
    init = np.zeros(elems, NPD[dtype])
    expect = scale(sums, exponent, dtype).reshape(-1)
    cls = np.zeros(elems, np.int8)
    for e, (d0, a) in zip(velems, vecs):
        init[e] = special(d0, dtype)
        expect[e] = sequential(d0, a, dtype)
    for i, e in enumerate(chosen):
        cls[e] = RECIPES[i % len(RECIPES)][1]
    return Ordered(keys, vals if width > 1 else vals.reshape(-1), init, expect, cls)


# ---- the shapes the tests use (computed once, shared, read-only) -----------------------------------------
# name -> (keys pattern, records, shard size in keys, row width, matrix columns). Sizes are odd; 20 485 is
# five 4096-element slabs and a partial one.
SHAPES = {
    "dense": ("dense", 9001, 9001, 1, 0),
    "dense_odd_start": ("dense", 9000, 9001, 1, 0),     # starts at element 1: pairs straddle the records
    "dups1000": ("dups", 1000, 9001, 1, 0),
    "dups4096": ("dups", 4096, 9001, 1, 0),
    "prefix_tail": ("prefix_tail", 20_000, 20_485, 1, 0),
    "uniform5000": ("uniform", 5000, 9001, 1, 0),
    "uniform30000": ("uniform", 30_000, 9001, 1, 0),
    "binned": ("binned", 310_000, 20_485, 1, 0),
    "binned_mat3": ("binned", 310_000, 6827 * 3, 1, 3),   # flat cells of a 6827 x 3 matrix
    "binned_mat64": ("binned", 310_000, 321 * 64, 1, 64),
    "rows3": ("rows", 657, 257, 3, 3),
    "rows64": ("rows", 657, 257, 64, 64),
}
# name -> ordered_case arguments
ORDERED_SHAPES = {
    "msg1000": dict(n=1000, size=9001),
    "fold4097": dict(n=4097, size=9001),
    "sort131073": dict(n=131_073, size=20_485, chain=70_000),
    "sort524289": dict(n=524_289, size=20_485, chain=80_000),
    "mat3": dict(n=1000, size=3001 * 3, cols=3),
    "rows3": dict(n=900, size=257, width=3, cols=3, hot_row=300),
    "rows64": dict(n=900, size=257, width=64, cols=64, hot_row=300),
}


def _freeze(x):
    for a in (x if isinstance(x, (tuple, list)) else [x]):
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
        elif isinstance(a, (tuple, list)):
            _freeze(a)
    return x


@functools.lru_cache(maxsize=None)
def grid_case(shape, dtype, grid):
    pattern, n, size, width, _ = SHAPES[shape]
    return _freeze(exact_grid(dtype, GRIDS[dtype][grid], pattern, n, size, seed=shape, width=width))


@functools.lru_cache(maxsize=None)
def nonfinite_case(shape, dtype):
    pattern, n, size, width, cols = SHAPES[shape]
    return _freeze(nonfinite(dtype, pattern, n, size, seed=shape, width=width, cols=cols, unique=pattern == "dense"))


@functools.lru_cache(maxsize=None)
def ordered_shape(shape, dtype):
    return _freeze(ordered_case(dtype, seed=shape, **ORDERED_SHAPES[shape]))


# name -> (keys pattern over the touched keys, records, shard size in keys, row width, matrix columns)
UNTOUCHED_SHAPES = {
    "dense": ("dense", 5122, 20_485, 1, 0),
    "dups1000": ("dups", 1000, 9001, 1, 0),
    "prefix_tail": ("prefix_tail", 5000, 20_485, 1, 0),
    "uniform1000": ("uniform", 1000, 9001, 1, 0),
    "uniform4097": ("uniform", 4097, 9001, 1, 0),
    "uniform5000": ("uniform", 5000, 9001, 1, 0),
    "uniform30000": ("uniform", 30_000, 9001, 1, 0),
    "uniform131073": ("uniform", 131_073, 20_485, 1, 0),
    "binned": ("binned", 310_000, 20_485, 1, 0),
    "binned_mat3": ("binned", 310_000, 6827 * 3, 1, 3),
    "binned_mat64": ("binned", 310_000, 321 * 64, 1, 64),
    "rows3": ("rows", 400, 257, 3, 3),
    "rows64": ("rows", 400, 257, 64, 64),
}


@functools.lru_cache(maxsize=None)
def untouched_case(shape, dtype):
    """``(keys, vals, image, untouched)``: the shard starts as an image in which every element is an
    edge value or an ordinary one (``edge_image``); the records -- the shape's pattern, integer values
    -- fall only on keys that are multiples of 4. ``untouched`` marks the elements (flat) that no
    record addresses: three of every four, among them the other half of every touched pair. What the
    reference never writes keeps its bits: -0.0 stays -0.0, a NaN its payload."""
    pattern, n, size, width, _ = UNTOUCHED_SHAPES[shape]
    rng = rng_for("untouched", shape, dtype)
    prefix, rest = pattern_keys(rng, pattern, n, (size + 3) // 4)
    keys = 4 * np.concatenate([prefix, rng.permutation(rest)]).astype(np.int64)
    assert keys.size == n and keys.max() < size
    vals = scale(rng.integers(-KMAX, KMAX + 1, (n, width)), 0, dtype)
    img = edge_image(dtype, size, width)
    untouched = np.repeat(np.arange(size) % 4 != 0, width)
    return _freeze((keys, vals if width > 1 else vals.reshape(-1), img, untouched))


def flat_records(keys, vals):
    """A row push's records as element records: (keys[i] * width + c, vals[i][c]), c inside each i."""
    if vals.ndim == 1:
        return keys, vals
    w = vals.shape[1]
    return (np.repeat(keys, w) * w + np.tile(np.arange(w, dtype=np.int64), keys.size)), vals.reshape(-1)


# ---- comparison ----------------------------------------------------------------------------------------
def bits(a):
    a = np.ascontiguousarray(a)
    return a.view(UINT[a.dtype])


def classify(a):
    a = np.asarray(a)
    out = np.zeros(a.shape, np.int8)
    out[a == np.inf], out[a == -np.inf], out[np.isnan(a)] = PINF, NINF, NAN
    return out


def assert_matches(got, expect, cls=None, what=""):
    """Bit for bit (through an integer view: signed zeros and NaNs compare) wherever the class map says
    EXACT; the class alone (a NaN of any payload and sign) where it names one."""
    got, expect = np.asarray(got).reshape(-1), np.asarray(expect).reshape(-1)
    assert got.dtype == expect.dtype and got.size == expect.size, what
    exact = np.ones(got.size, bool) if cls is None else cls == EXACT
    bad = np.flatnonzero((bits(got) != bits(expect)) & exact)
    assert bad.size == 0, (f"{what}: {bad.size} elements differ, first at {bad[:6]}: got {got[bad[:6]]!r} "
                           f"expected {expect[bad[:6]]!r}")
    if cls is not None:
        bad = np.flatnonzero((classify(got) != cls) & ~exact)
        assert bad.size == 0, f"{what}: class differs at {bad[:6]}: got {got[bad[:6]]!r}, want class {cls[bad[:6]]}"


# ---- raw images ------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def edge_image(dtype, rows, cols):
    """A (rows, cols) image for the pulls: -0.0, quiet NaNs of several payloads and both signs, a
    signalling NaN, +/-inf, the smallest and largest subnormal, the smallest normal and +/-MAX, among
    ordinary values; every edge value occurs, the first ones in the image's corners."""
    npd = NPD[dtype]
    rng = rng_for("image", dtype, rows, cols)
    if npd == np.float32:
        pat = [0x80000000, 0x7FC00000, 0x7FC00001, 0xFFC00001, 0x7FD55555, 0xFFFFFFFF, 0x7F800001, 0x7F800000,
               0xFF800000, 0x00000001, 0x007FFFFF, 0x807FFFFF, 0x00800000, 0x7F7FFFFF, 0xFF7FFFFF]
    else:
        pat = [0x8000000000000000, 0x7FF8000000000000, 0x7FF8000000000123, 0xFFF8000000000123, 0x7FFD555555555555,
               0xFFFFFFFFFFFFFFFF, 0x7FF0000000000001, 0x7FF0000000000000, 0xFFF0000000000000, 0x0000000000000001,
               0x000FFFFFFFFFFFFF, 0x800FFFFFFFFFFFFF, 0x0010000000000000, 0x7FEFFFFFFFFFFFFF, 0xFFEFFFFFFFFFFFFF]
    pat = np.array(pat, UINT[np.dtype(npd)]).view(npd)
    img = rng.uniform(-1, 1, rows * cols).astype(npd)
    pick = rng.random(img.size) < 0.5
    img[pick] = pat[rng.integers(0, pat.size, int(pick.sum()))]
    m = min(pat.size, img.size)
    img[:m] = pat[:m]
    if img.size >= 2 * pat.size:
        img[-pat.size:] = pat
    img = img.reshape(rows, cols)
    img.setflags(write=False)
    return img


def write_image(sh, gpu, img, pad_value):
    """The image into the shard's memory as it lies (row pitch from glint_shard_pitch), the pitch
    padding set to a NON-ZERO value: a kernel that read it would count it."""
    import torch
    from glint_amd import _native as N
    lib = N.load()
    pitch = C.c_int64()
    assert lib.glint_shard_pitch(sh.handle, C.byref(pitch)) == N.GLINT_OK
    assert pitch.value >= img.shape[1]
    padded = np.full((img.shape[0], pitch.value), pad_value, img.dtype)
    padded[:, :img.shape[1]] = img
    d = torch.device("cuda", gpu)
    src = torch.from_numpy(padded).to(d)
    segs = np.array([0, 0, padded.nbytes], np.int64)
    assert lib.glint_copy_segments_dev(src.data_ptr(), sh.data_ptr(), segs.ctypes.data_as(C.POINTER(C.c_int64)), 1,
                                       torch.cuda.current_stream(d).cuda_stream) == N.GLINT_OK
    torch.cuda.synchronize(d)
