"""Shard fill and uniform init, the parts that need no GPU: the numpy generator against the published
Philox4x32-10 answers, the contract header (through tests/c/init_probe.cpp) against the numpy replay bit for
bit, the ABI's symbols and NULL-shard checks, what the contract's rounding fixes, and the fan-out of
BigVector / BigMatrix fill and initUniform over fake shards."""
import ctypes as C
import importlib.util
from pathlib import Path

import numpy as np
import pytest

import glint_amd
from glint_amd import _native as N
from glint_amd import CyclicPartitioner, IndexOutOfBoundsException, RangePartitioner
from glint_amd.client import BigMatrix, BigVector
from init_cases import (bits, block_len, fma_f32, global_rows, host_range, philox4x32_10, replay_fill,
                        replay_uniform, uniform_elems, uniform_rows, unit_to_value, words_to_unit)

ROOT = Path(__file__).resolve().parent.parent
TYPES = [np.float32, np.float64]

# Philox4x32-10 known answers (Random123's kat_vectors): counter, key, output
KAT = [
    ((0, 0, 0, 0), (0, 0), (0x6627e8d5, 0xe169c58d, 0xbc57ac4c, 0x9b00dbd8)),
    ((0xffffffff,) * 4, (0xffffffff,) * 2, (0x408f276d, 0x41c83b0e, 0xa20bc7c6, 0x6d5451fd)),
    ((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0),
     (0xd16cfe09, 0x94fdcceb, 0x5001e420, 0x24126ea1)),
]


@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("_glint_build", ROOT / "glint_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = C.CDLL(str(mod.build_init_probe()))
    u64p, u32p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint32)
    lib.init_philox.argtypes = [u32p, u32p, u32p]
    lib.init_elems_f32.argtypes = [u64p, u64p, u32p, C.c_int64, C.c_float, C.c_float, C.POINTER(C.c_float)]
    lib.init_elems_f64.argtypes = [u64p, u64p, u32p, C.c_int64, C.c_double, C.c_double, C.POINTER(C.c_double)]
    lib.init_values_f32.argtypes = [u32p, C.c_float, C.c_float, C.POINTER(C.c_float)]
    lib.init_values_f64.argtypes = [u32p, C.c_double, C.c_double, C.POINTER(C.c_double)]
    lib.init_range_f32.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_float), C.POINTER(C.c_float)]
    lib.init_range_f64.argtypes = [C.c_double, C.c_double, C.POINTER(C.c_double), C.POINTER(C.c_double)]
    for f in (lib.init_philox, lib.init_elems_f32, lib.init_elems_f64, lib.init_values_f32, lib.init_values_f64):
        f.restype = None
    return lib


def _p(a, ct):
    return a.ctypes.data_as(C.POINTER(ct))


def _ct(npd):
    return C.c_float if np.dtype(npd) == np.float32 else C.c_double


def _sfx(npd):
    return "f32" if np.dtype(npd) == np.float32 else "f64"


# ---- 1. the generator ---------------------------------------------------------------------------------
@pytest.mark.parametrize("ctr,key,want", KAT)
def test_numpy_philox_known_answers(ctr, key, want):
    got = philox4x32_10(np.array(ctr), np.array(key))
    assert [hex(x) for x in got.tolist()] == [hex(x) for x in want]


def test_numpy_philox_broadcasts():
    ctr = np.array([k[0] for k in KAT])
    key = np.array([k[1] for k in KAT])
    np.testing.assert_array_equal(philox4x32_10(ctr, key), np.array([k[2] for k in KAT], np.uint32))


@pytest.mark.parametrize("ctr,key,want", KAT)
def test_header_philox_known_answers(probe, ctr, key, want):
    c, k, o = np.array(ctr, np.uint32), np.array(key, np.uint32), np.zeros(4, np.uint32)
    probe.init_philox(_p(c, C.c_uint32), _p(k, C.c_uint32), _p(o, C.c_uint32))
    assert o.tolist() == list(want)


# ---- 2. the contract header against the replay --------------------------------------------------------
def _probe_elems(probe, npd, seed, g, c, lo, w):
    seed, g = np.ascontiguousarray(seed, np.uint64), np.ascontiguousarray(g, np.uint64)
    c = np.ascontiguousarray(c, np.uint32)
    out = np.zeros(g.size, npd)
    getattr(probe, "init_elems_" + _sfx(npd))(_p(seed, C.c_uint64), _p(g, C.c_uint64), _p(c, C.c_uint32), g.size,
                                              lo, w, _p(out, _ct(npd)))
    return out


@pytest.mark.parametrize("npd", TYPES)
@pytest.mark.parametrize("lo,hi", [(-0.5 / 128, 0.5 / 128), (-1e6, 3e7), (0.1, 0.1), (0.0, 1.0)])
def test_header_equals_replay(probe, npd, lo, hi):
    rng = np.random.default_rng(5)
    n = 4000
    seed = rng.integers(0, 1 << 64, n, dtype=np.uint64)
    g = rng.integers(0, 1 << 40, n, dtype=np.uint64)
    c = rng.integers(0, 1 << 20, n, dtype=np.uint64)
    # g and seed above 2^32 (the second counter word and the second key word carry), and small ones
    g[:500] = rng.integers(1 << 32, 1 << 63, 500, dtype=np.uint64)
    seed[500:1000] = rng.integers(1 << 32, 1 << 64, 500, dtype=np.uint64)
    g[1000:1200] = rng.integers(0, 1000, 200, dtype=np.uint64)
    seed[1200:1400] = rng.integers(0, 1000, 200, dtype=np.uint64)
    c[1400:1800] = rng.integers(0, 9, 400, dtype=np.uint64)  # every position of the first blocks
    assert (g >> np.uint64(32)).any() and (seed >> np.uint64(32)).any()
    lo_v, w = host_range(lo, hi, npd)
    want = uniform_elems(seed, g, c, lo_v, w, npd)
    got = _probe_elems(probe, npd, seed, g, c, lo_v, w)
    np.testing.assert_array_equal(bits(got), bits(want))
    assert (want >= lo_v).all() and (want <= npd(hi)).all()
    if lo != hi:
        assert np.unique(want).size > n // 2


@pytest.mark.parametrize("npd", TYPES)
def test_header_counter_words(probe, npd):
    """The words of the counter and the key are where the contract puts them: (g, c) and seed pairs that a
    swapped or dropped word would confuse give different values, each equal to the replay."""
    L = block_len(npd)
    g = np.array([1, 1 << 32, 1, 0, 0, (1 << 32) + 1], np.uint64)
    c = np.array([0, 0, L, 1 * L, 0, 0], np.uint32)
    seed = np.array([7, 7, 7, 7, 7, 7 << 32], np.uint64)
    got = _probe_elems(probe, npd, seed, g, c, npd(0), npd(1))
    np.testing.assert_array_equal(bits(got), bits(uniform_elems(seed, g, c.astype(np.uint64), npd(0), npd(1), npd)))
    assert np.unique(got).size == g.size


@pytest.mark.parametrize("npd", TYPES)
def test_header_forced_words(probe, npd):
    """Output words forced to all ones give u = 1 - 2^-24 (1 - 2^-53), to zero u = 0."""
    L = block_len(npd)
    eps = 2.0 ** -24 if npd == np.float32 else 2.0 ** -53
    for words, u in ((np.full(4, 0xFFFFFFFF, np.uint32), 1.0 - eps), (np.zeros(4, np.uint32), 0.0)):
        assert words_to_unit(words, npd).tolist() == [u] * L and words_to_unit(words, npd).dtype == npd
        for lo, hi in ((-0.5 / 128, 0.5 / 128), (-3.0, 5.0), (1.0, 1.0 + 2 * float(np.finfo(npd).eps))):
            lo_v, w = host_range(lo, hi, npd)
            out = np.zeros(L, npd)
            getattr(probe, "init_values_" + _sfx(npd))(_p(words, C.c_uint32), lo_v, w, _p(out, _ct(npd)))
            want = unit_to_value(words_to_unit(words, npd), lo_v, w)
            np.testing.assert_array_equal(bits(out), bits(want))
            assert (out >= lo_v).all() and (out <= npd(hi)).all()
            if u == 0.0:
                assert (out == lo_v).all()
    # rounding may give hi itself: the largest u over a range of two ulps
    lo_v, w = host_range(1.0, 1.0 + 2 * float(np.finfo(npd).eps), npd)
    top = unit_to_value(words_to_unit(np.full(4, 0xFFFFFFFF, np.uint32), npd), lo_v, w)
    assert (top == npd(1.0) + w).all()


@pytest.mark.parametrize("npd", TYPES)
def test_header_range(probe, npd):
    big = float(np.finfo(npd).max)
    cases = [(-1.0, 1.0), (0.1, 0.1), (-0.5 / 128, 0.5 / 128), (1.0, -1.0), (float("nan"), 1.0), (0.0, float("nan")),
             (float("-inf"), 0.0), (0.0, float("inf")), (-big, big), (-big, 0.0), (1e-300, 1e-300), (0.1, 0.1 + 1e-12)]
    if npd == np.float32:
        cases += [(0.0, 1e39), (-1e39, 0.0), (1e-46, 1e-46)]
    for lo, hi in cases:
        l, w = _ct(npd)(), _ct(npd)()
        ok = getattr(probe, "init_range_" + _sfx(npd))(lo, hi, C.byref(l), C.byref(w))
        want = host_range(lo, hi, npd)
        assert bool(ok) == (want is not None), (lo, hi)
        if want is not None:
            assert bits(np.array([l.value, w.value], npd)).tolist() == bits(np.array(want, npd)).tolist(), (lo, hi)
    assert host_range(1.0, -1.0, npd) is None and host_range(-big, big, npd) is None  # (w overflows)
    assert host_range(0.1, 0.1, npd)[1] == 0


# ---- 3. ABI -------------------------------------------------------------------------------------------
def test_abi():
    lib = N.load()
    one = np.ones(1, np.float64)
    assert lib.glint_shard_fill(None, None, 0, one.ctypes.data) == N.GLINT_EINVAL
    assert lib.glint_shard_fill_dev(None, None, 0, one.ctypes.data, None) == N.GLINT_EINVAL
    assert lib.glint_shard_init_uniform(None, None, 0, 1, 0.0, 1.0) == N.GLINT_EINVAL
    assert lib.glint_shard_init_uniform_dev(None, None, 0, 1, 0.0, 1.0, None) == N.GLINT_EINVAL
    for name in ("glint_shard_fill", "glint_shard_fill_dev", "glint_shard_init_uniform",
                 "glint_shard_init_uniform_dev"):
        assert name in N.SIGNATURES
    assert lib.glint_version() > 900
    assert N.GLINT_K_COUNT == 13 and N.GLINT_K_PUSH_ROWS == 8  # no new kernel id


def test_methods_are_public():
    for cls in (glint_amd.PartialVector, glint_amd.PartialMatrix, glint_amd.BigVector, glint_amd.BigMatrix):
        assert callable(cls.fill) and callable(cls.initUniform)


# ---- 4. what the contract fixes shows in the bits -----------------------------------------------------
@pytest.mark.parametrize("lo,hi", [(-0.5 / 128, 0.5 / 128), (-0.5 / 100, 0.5 / 100), (-1000.0, 3.0e4)])
def test_contract_rounding_shows(lo, hi):
    """Float: a fused fma(u, w, lo) and the form lo * (1 - u) + hi * u are other functions; the share of
    elements each changes is printed (DESIGN.md records it), and only its being non-zero is asserted.

    One exception, by arithmetic and not by measurement: for the word2vec range of 128 dimensions lo, hi
    and w = 1/128 are powers of two, so with u = k * 2^-24 every product and 1 - u are exact and all three
    forms equal 2^-8 * (2 u - 1), itself representable: no rounding happens at all and no form CAN differ.
    There both shares are asserted to be exactly 0; they are asserted above 0 for the same range at 100
    dimensions (w = 0.01 rounded) and for the wide one."""
    npd = np.float32
    lo_v, w = host_range(lo, hi, npd)
    g = np.arange(512, dtype=np.uint64)[:, None]
    c = np.arange(128, dtype=np.uint64)[None, :]
    L = np.uint64(4)
    zero = np.zeros_like(g + c)
    ctr = np.stack(np.broadcast_arrays(g, zero, c // L, zero), axis=-1)
    u = np.take_along_axis(words_to_unit(philox4x32_10(ctr, np.array([99, 0])), npd),
                           np.broadcast_to(c % L, zero.shape).astype(np.int64)[..., None], axis=-1)[..., 0]
    want = unit_to_value(u, lo_v, w)
    np.testing.assert_array_equal(bits(want), bits(uniform_rows(99, np.arange(512), 128, lo, hi, npd)))
    fused = fma_f32(u, np.full_like(u, w), np.full_like(u, lo_v))
    one = npd(1)
    lerp = np.add(np.multiply(lo_v, np.subtract(one, u, dtype=npd), dtype=npd),
                  np.multiply(npd(hi), u, dtype=npd), dtype=npd)
    s_fused = (bits(fused) != bits(want)).mean()
    s_lerp = (bits(lerp) != bits(want)).mean()
    print(f"float32 [{lo}, {hi}]: fused fma changes {s_fused:.4f} of the elements, lo*(1-u)+hi*u {s_lerp:.4f}")
    if np.frexp(w)[0] == 0.5 and lo_v == -npd(hi):  # powers of two: nothing is rounded
        assert hi == 0.5 / 128 and s_fused == 0 and s_lerp == 0
    else:
        assert s_fused > 0 and s_lerp > 0


# ---- 5. replay sanity ---------------------------------------------------------------------------------
@pytest.mark.parametrize("npd", TYPES)
def test_replay_sanity(npd):
    lo, hi = -0.5 / 128, 0.5 / 128
    t = uniform_rows(1234, np.arange(512) + (1 << 33), 128, lo, hi, npd)  # 2^16 values
    assert t.shape == (512, 128) and t.dtype == npd
    assert (t >= npd(lo)).all() and (t <= npd(hi)).all()
    se = (hi - lo) / np.sqrt(12.0) / np.sqrt(t.size)
    assert abs(float(t.astype(np.float64).mean()) - (lo + hi) / 2) < 4 * se
    assert np.unique(bits(t), axis=0).shape[0] == 512  # no two rows equal
    other = uniform_rows(1235, np.arange(512) + (1 << 33), 128, lo, hi, npd)
    assert (bits(other) != bits(t)).mean() > 0.99  # the same (g, c) under another seed
    # a row's values do not depend on which rows are asked for, nor a column's on cols
    np.testing.assert_array_equal(bits(uniform_rows(1234, [5 + (1 << 33)], 128, lo, hi, npd)[0]), bits(t[5]))
    np.testing.assert_array_equal(bits(uniform_rows(1234, np.arange(3) + (1 << 33), 67, lo, hi, npd)), bits(t[:3, :67]))


def test_replay_fill_keeps_bits():
    t = np.arange(12, dtype=np.float32).reshape(4, 3)
    nan = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
    out = replay_fill(t, [2, 0, 2], nan)
    assert bits(out)[[0, 2]].tolist() == [[0x7FC12345] * 3] * 2
    np.testing.assert_array_equal(out[[1, 3]], t[[1, 3]])
    assert bits(replay_fill(t, [1], -0.0))[1].tolist() == [0x80000000] * 3
    tl = np.zeros((2, 2), np.int64)
    assert replay_fill(tl, [1], np.iinfo(np.int64).min)[1].tolist() == [np.iinfo(np.int64).min] * 2


# ---- 6. fan-out over fake shards ----------------------------------------------------------------------
class FakeShard:
    """Applies fill / initUniform to its slice of a numpy table by the replay, and records the calls."""

    def __init__(self, table, partition):
        self.table, self.partition, self.calls = table, partition, []
        self.np_dtype = table.dtype.type

    def _local(self, rows):
        if rows is None:
            return np.arange(self.table.shape[0])
        p = self.partition
        rows = np.asarray(rows, dtype=np.int64)
        local = (rows - p.index) // p.numberOfPartitions if hasattr(p, "numberOfPartitions") else rows - p.start
        assert ((local >= 0) & (local < self.table.shape[0])).all()
        np.testing.assert_array_equal(global_rows(p, local), rows)  # only its own rows
        return local

    def fill(self, value, rows=None, sync=True):
        self.calls.append(("fill", value, None if rows is None else np.array(rows)))
        self.table[:] = replay_fill(self.table, self._local(rows), value)
        return True

    def initUniform(self, seed, lo, hi, rows=None, sync=True):
        self.calls.append(("uniform", (seed, lo, hi), None if rows is None else np.array(rows)))
        local = self._local(rows)
        self.table[:] = replay_uniform(self.table, local, global_rows(self.partition, local), seed, lo, hi)
        return True


def _matrix(partitioner, nrows=300, cols=7, dtype=np.float32):
    shards = [FakeShard(np.full((p.size, cols), 9, dtype), p) for p in partitioner.all()]
    return shards, BigMatrix(partitioner, shards, nrows, cols)


def _whole(partitioner, shards, nrows):
    out = np.zeros((nrows,) + shards[0].table.shape[1:], shards[0].table.dtype)
    for s in shards:
        out[global_rows(s.partition, np.arange(s.table.shape[0]))] = s.table
    return out


@pytest.mark.parametrize("make", [lambda: RangePartitioner.apply(3, 300), lambda: CyclicPartitioner.apply(3, 300),
                                  lambda: RangePartitioner.apply(2, 300)])
def test_fanout_whole_model(make):
    partitioner = make()
    shards, m = _matrix(partitioner)
    assert m.initUniform(77, -1.0, 1.0)
    for s in shards:
        assert len(s.calls) == 1 and s.calls[0][0] == "uniform" and s.calls[0][1] == (77, -1.0, 1.0) \
            and s.calls[0][2] is None  # every shard once, the same seed, rows=None
    # the model's bits do not depend on the layout
    np.testing.assert_array_equal(bits(_whole(partitioner, shards, 300)),
                                  bits(uniform_rows(77, np.arange(300), 7, -1.0, 1.0, np.float32)))
    assert m.fill(0.1)
    for s in shards:
        assert len(s.calls) == 2 and s.calls[1][0] == "fill" and s.calls[1][2] is None
    assert (_whole(partitioner, shards, 300) == np.float32(0.1)).all()


@pytest.mark.parametrize("make", [lambda: RangePartitioner.apply(3, 300), lambda: CyclicPartitioner.apply(3, 300)])
def test_fanout_row_list(make):
    partitioner = make()
    shards, m = _matrix(partitioner)
    rng = np.random.default_rng(3)
    rows = rng.integers(0, 300, 150).astype(np.int64)  # every partition hit, interleaved, with repeats
    rows[10:13] = rows[10]
    owner = partitioner.partition_indices(rows)
    assert set(owner.tolist()) == {0, 1, 2}
    assert m.initUniform(5, 0.0, 2.0, rows=rows)
    for p, s in enumerate(shards):
        assert len(s.calls) == 1 and s.calls[0][1] == (5, 0.0, 2.0)  # one call, the same seed
        np.testing.assert_array_equal(s.calls[0][2], rows[owner == p])  # its own rows, in the caller's order
    want = replay_uniform(np.full((300, 7), 9, np.float32), rows, rows, 5, 0.0, 2.0)
    np.testing.assert_array_equal(bits(_whole(partitioner, shards, 300)), bits(want))
    assert m.fill(-0.0, rows=rows[:4])
    want = replay_fill(want, rows[:4], -0.0)
    np.testing.assert_array_equal(bits(_whole(partitioner, shards, 300)), bits(want))


def test_fanout_skips_partitions_without_rows_and_empty_lists():
    shards, m = _matrix(RangePartitioner.apply(3, 300))
    m.fill(1.5, rows=np.array([250, 203, 250, 299, 3, 0], np.int64))  # nothing from partition 1
    assert len(shards[0].calls) == 1 and not shards[1].calls and len(shards[2].calls) == 1
    for s in shards:
        s.calls.clear()
    assert m.initUniform(1, 0.0, 1.0, rows=np.zeros(0, np.int64)) and m.fill(2.0, rows=[])
    assert all(not s.calls for s in shards)  # an empty list names nothing (it is not rows=None)


def test_fanout_rejects_before_any_shard_is_called():
    shards, m = _matrix(RangePartitioner.apply(3, 300))
    for bad in ([3, 299, 300, 5], [-1]):
        with pytest.raises(IndexOutOfBoundsException):
            m.initUniform(1, 0.0, 1.0, rows=np.array(bad, np.int64))
        with pytest.raises(IndexOutOfBoundsException):
            m.fill(1.0, rows=np.array(bad, np.int64))
    assert all(not s.calls for s in shards)


def test_fanout_vector():
    partitioner = CyclicPartitioner.apply(3, 100)
    shards = [FakeShard(np.full((p.size, 1), 9, np.float64), p) for p in partitioner.all()]
    v = BigVector(partitioner, shards, 100)
    keys = np.array([99, 0, 50, 51, 52, 0], np.int64)
    assert v.initUniform(8, -2.0, 2.0, rows=keys)
    want = replay_uniform(np.full((100, 1), 9, np.float64), keys, keys, 8, -2.0, 2.0)
    np.testing.assert_array_equal(bits(_whole(partitioner, shards, 100)), bits(want))
    assert v.fill(3.0) and all(s.calls[-1] == ("fill", 3.0, None) for s in shards)
    with pytest.raises(IndexOutOfBoundsException):
        v.fill(1.0, rows=[100])
