"""Row sampler on the GPU (glint_sampler_*): every draw is compared, bit for bit, with the numpy / Python-int
replay (sampler_cases) -- over the table sizes at which the build's scan and the draw's two-level search
change shape, weight patterns whose zero runs make the search's tie case, the counter's wrap, the host and
device forms, the exclusion rule, the three creates and their refusals, two streams at once, and the
skip-gram chain the sampler exists for.

A total near 2^63 needs a table of nearly 2^31 entries (16 GB) and is not run: the largest total cheaply
reachable, every weight 2^32 - 1 at m = 1025, stands in for it."""
import ctypes as C

import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import (ArrayIndexOutOfBoundsException, BigMatrix, Client, CyclicPartition, PartialMatrix, PartialVector,
                       RangePartition, RangePartitioner, Sampler)
from init_cases import bits
from sampler_cases import EXCLUSION, W_MAX, cdf_of, replay_draw, table, zipf_counts

pytestmark = pytest.mark.gpu

COARSE = N.GLINT_SAMPLE_COARSE
FIRSTS = [0, (7 << 32) + 99, (1 << 64) - 2]
SEED = (0xFEED << 40) | 12345  # above 2^32: the second key word carries
NS = [0, 1, 63, 64, 65, 1000]
# (m, pattern): one entry; two with one zero; around the coarse table's size (one entry per coarse block, then
# two); two and three scan levels (the scan tile is 1024)
SHAPES = ([(1, "ones"), (2, "zero_first"), (2, "zero_last")]
          + [(m, p) for m in (COARSE - 1, COARSE, COARSE + 1) for p in ("ones", "zipf", "zeros_coarse")]
          + [(1025, p) for p in ("ones", "zipf", "zeros_start", "zeros_end", "zeros_coarse", "max")]
          + [(1024 ** 2 + 1, p) for p in ("zipf", "zeros_start", "zeros_end", "zeros_coarse")])
_tables = {}


def weights_of(m, pattern):
    """(weights, cdf) of a shape, computed once."""
    if (m, pattern) not in _tables:
        if m == 2:
            w = np.array([0, 5] if pattern == "zero_first" else [5, 0], np.int64)
        else:
            w = table(m, pattern, COARSE)
        _tables[(m, pattern)] = (w, cdf_of(w))
    return _tables[(m, pattern)]


def dev_draw(s, n, seed, first, gpu, exclude=None, per=1, **kw):
    """The device form: exclude (if any) as a tensor; with neither exclude nor out, an out tensor asks for it."""
    import torch
    d = torch.device("cuda", gpu)
    ex = None if exclude is None else torch.from_numpy(np.ascontiguousarray(exclude, np.int64)).to(d)
    if ex is None and "out" not in kw:
        kw["out"] = torch.full((max(n, 0),), -77, dtype=torch.int64, device=d)
    return s.draw(n, seed, first, exclude=ex, per=per, **kw).cpu().numpy()


@pytest.mark.parametrize("m,pattern", SHAPES)
def test_sizes_and_patterns(gpu, m, pattern):
    w, cdf = weights_of(m, pattern)
    fk = -(1 << 40) + m
    with Sampler(w, firstKey=fk, device=gpu) as s:
        assert s.info() == (m, fk, int(cdf[-1]), gpu)
        for first in FIRSTS:
            want = replay_draw(w, fk, SEED, first, 1000, cdf=cdf)
            np.testing.assert_array_equal(s.draw(1000, SEED, first), want)
            np.testing.assert_array_equal(dev_draw(s, 1000, SEED, first, gpu), want)
            assert (w[want - fk] > 0).all()


def test_every_step_of_a_coarse_block_is_reachable(gpu):
    """All of a small table's entries are drawn, each zero-weight one never: a search that stops one short
    at either level, or steps over a tie, loses an entry."""
    m = 2 * COARSE + 3  # blocks of two entries, the last one cut short
    w = np.ones(m, np.int64)
    w[5:9] = 0
    w[COARSE - 1:COARSE + 2] = 0
    w[m - 2] = 0
    n = 40 * m
    with Sampler(w, device=gpu) as s:
        got = s.draw(n, 3, 0)
    np.testing.assert_array_equal(got, replay_draw(w, 0, 3, 0, n))
    counts = np.bincount(got, minlength=m)
    assert (counts[w == 0] == 0).all() and (counts[w > 0] > 0).all()


@pytest.mark.parametrize("n", NS)
def test_draw_counts(gpu, n):
    w, cdf = weights_of(COARSE + 1, "zipf")
    with Sampler(w, firstKey=10, device=gpu) as s:
        for first in FIRSTS:
            want = replay_draw(w, 10, SEED, first, n, cdf=cdf)
            got = s.draw(n, SEED, first)
            assert got.dtype == np.int64 and got.shape == (n,)
            np.testing.assert_array_equal(got, want)
            np.testing.assert_array_equal(dev_draw(s, n, SEED, first, gpu), want)
        # a range of counters split over two calls is the concatenation
        if n > 1:
            a, b = s.draw(n // 3, SEED, FIRSTS[2]), s.draw(n - n // 3, SEED, (FIRSTS[2] + n // 3) % (1 << 64))
            np.testing.assert_array_equal(np.concatenate([a, b]), replay_draw(w, 10, SEED, FIRSTS[2], n, cdf=cdf))


def test_host_draw_in_several_launches(gpu):
    """A host draw longer than one launch's share (2^22 draws), with exclusion: the launches' parts of
    exclude line up (per = 3 does not divide the share)."""
    w, cdf = weights_of(1025, "zipf")
    n, per = (1 << 22) + 1001, 3
    ex = (np.arange(-(-n // per), dtype=np.int64) * 5) % 1025
    with Sampler(w, device=gpu) as s:
        got = s.draw(n, 5, (1 << 64) - 1000, exclude=ex, per=per)
    tail = slice((1 << 22) - 500, n)  # the replay of the seam and of the second launch
    want = replay_draw(w, 0, 5, (1 << 64) - 1000 + tail.start, n - tail.start, exclude=np.repeat(ex, per)[tail], cdf=cdf)
    np.testing.assert_array_equal(got[tail], want)
    np.testing.assert_array_equal(got[:2000], replay_draw(w, 0, 5, (1 << 64) - 1000, 2000, exclude=ex[:667], per=per, cdf=cdf))
    assert (got != np.repeat(ex, per)[:n]).all()


def test_out_slice_at_odd_offset(gpu):
    import torch
    w, cdf = weights_of(1025, "zipf")
    buf = torch.full((1003,), -5, dtype=torch.int64, device=torch.device("cuda", gpu))
    with Sampler(w, device=gpu) as s:
        ret = s.draw(1000, SEED, 17, out=buf[1:1001])
        assert ret.data_ptr() == buf.data_ptr() + 8
    got = buf.cpu().numpy()
    np.testing.assert_array_equal(got[1:1001], replay_draw(w, 0, SEED, 17, 1000, cdf=cdf))
    assert got[0] == -5 and (got[1001:] == -5).all()


# ---- exclusion -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("per,n", [(1, 1000), (5, 1003)])
def test_exclusion_hot_keys(gpu, per, n):
    """Zipf counts and positives drawn from the same table: the hot keys are excluded often, so the retries
    and their order show."""
    w, cdf = weights_of(COARSE + 1, "zipf")
    fk = 1 << 35
    ex = replay_draw(w, fk, 99, 0, -(-n // per), cdf=cdf)
    ex[::7] = fk + int(np.argmax(w))  # the hottest key
    ex[3] = fk - 1                    # outside the table
    want = replay_draw(w, fk, SEED, FIRSTS[1], n, exclude=ex, per=per, cdf=cdf)
    plain = replay_draw(w, fk, SEED, FIRSTS[1], n, cdf=cdf)
    assert (want != plain).sum() >= 3 and (want != np.repeat(ex, per)[:n]).all()
    with Sampler(w, firstKey=fk, device=gpu) as s:
        np.testing.assert_array_equal(s.draw(n, SEED, FIRSTS[1], exclude=ex, per=per), want)
        np.testing.assert_array_equal(dev_draw(s, n, SEED, FIRSTS[1], gpu, exclude=ex, per=per), want)


@pytest.mark.parametrize("name,weights,first_key,forb", EXCLUSION)
def test_exclusion_tables(gpu, name, weights, first_key, forb):
    n, per = 23, 5
    ex = np.full(-(-n // per), forb, np.int64)
    want = replay_draw(weights, first_key, 77, 1 << 40, n, exclude=ex, per=per)
    with Sampler(weights, firstKey=first_key, device=gpu) as s:
        np.testing.assert_array_equal(s.draw(n, 77, 1 << 40, exclude=ex, per=per), want)
        np.testing.assert_array_equal(dev_draw(s, n, 77, 1 << 40, gpu, exclude=ex, per=per), want)
        with pytest.raises(ValueError):
            s.draw(n, 77, 0, exclude=ex, per=0)
        with pytest.raises(ValueError):
            s.draw(-1, 77)
    if name == "concentrated_hot":
        assert (want == 103).all()
    if name == "concentrated_wrap":
        assert (want == 101).all()
    if name == "single":
        assert (want == forb).all()


def test_draw_argument_checks(gpu):
    lib = N.load()
    out = np.zeros(4, np.int64)
    ex = np.zeros(4, np.int64)
    with Sampler(np.array([1, 2, 3]), device=gpu) as s:
        h = s.handle
        assert lib.glint_sampler_draw(h, 1, 0, -1, None, 1, out.ctypes.data) == N.GLINT_EINVAL
        assert lib.glint_sampler_draw(h, 1, 0, 1 << 31, None, 1, out.ctypes.data) == N.GLINT_EINVAL
        assert lib.glint_sampler_draw(h, 1, 0, 4, None, 1, None) == N.GLINT_EINVAL
        assert lib.glint_sampler_draw(h, 1, 0, 4, ex.ctypes.data, 0, out.ctypes.data) == N.GLINT_EINVAL
        assert lib.glint_sampler_draw_dev(h, 1, 0, 4, None, 1, None, None) == N.GLINT_EINVAL
        assert lib.glint_sampler_draw(h, 1, 0, 0, None, 0, None) == N.GLINT_OK  # n == 0: nothing to do
        assert lib.glint_sampler_draw_dev(h, 1, 0, 0, None, 0, None, None) == N.GLINT_OK
        assert lib.glint_sampler_draw(h, 1, 0, 4, None, -3, out.ctypes.data) == N.GLINT_OK  # per ignored
        np.testing.assert_array_equal(out, replay_draw(np.array([1, 2, 3]), 0, 1, 0, 4))


# ---- creates ---------------------------------------------------------------------------------------------
def test_create_from_device_tensor(gpu):
    import torch
    w, cdf = weights_of(1025, "zeros_coarse")
    t = torch.from_numpy(w).to(torch.device("cuda", gpu))
    with Sampler(t, firstKey=3) as s:
        assert s.info() == (1025, 3, int(cdf[-1]), gpu)
        np.testing.assert_array_equal(s.draw(500, 1, 2), replay_draw(w, 3, 1, 2, 500, cdf=cdf))
    np.testing.assert_array_equal(t.cpu().numpy(), w)  # only read
    with Client([gpu]).sampler(w, firstKey=3) as s:
        assert s.info() == (1025, 3, int(cdf[-1]), gpu)


@pytest.mark.parametrize("dtype,npd", [("int", np.int32), ("long", np.int64)])
def test_create_from_counts_shard(gpu, dtype, npd):
    m, start = 3000, 1 << 33
    rng = np.random.default_rng(4)
    with PartialVector(RangePartition(0, start, start + m), dtype, gpu) as v:
        counts = np.zeros(m, np.int64)
        for _ in range(2):  # two pushes with repeated keys
            k = rng.integers(0, m // 2, 4000).astype(np.int64)
            c = rng.integers(1, 9, 4000).astype(npd)
            v.update(k + start, c)
            np.add.at(counts, k, c.astype(np.int64))
        before = v.to_numpy()
        np.testing.assert_array_equal(before.astype(np.int64), counts)
        with Sampler.fromShard(v) as s:
            assert s.info() == (m, start, int(counts.sum()), gpu)
            np.testing.assert_array_equal(s.draw(1000, 6, 1), replay_draw(counts, start, 6, 1, 1000))
            np.testing.assert_array_equal(dev_draw(s, 1000, 6, 1, gpu), replay_draw(counts, start, 6, 1, 1000))
        np.testing.assert_array_equal(bits(v.to_numpy()), bits(before))  # the shard is only read
        # a negative count: the lowest index, no handle
        v.update(np.array([start + 2500, start + 1700], np.int64), np.array([-1, -50], npd))
        with pytest.raises(ArrayIndexOutOfBoundsException) as e:
            Sampler.fromShard(v)
        assert e.value.record == 1700
        h, bad = C.c_void_p(1), C.c_int64(-9)
        assert N.load().glint_sampler_create_from_shard(v.handle, C.byref(bad), C.byref(h)) == N.GLINT_EOUTOFRANGE
        assert not h.value and bad.value == 1700
        if npd == np.int64:  # a count of 2^32 (in front of the negative ones)
            v.update(np.array([start + 9], np.int64), np.array([(1 << 32) - int(counts[9])], npd))
            with pytest.raises(ArrayIndexOutOfBoundsException) as e:
                Sampler.fromShard(v)
            assert e.value.record == 9
        v.zero()
        with pytest.raises(ValueError):  # T == 0
            Sampler.fromShard(v)


def test_create_refuses_bad_weights(gpu):
    import torch
    d = torch.device("cuda", gpu)
    lib = N.load()
    base = zipf_counts(5000)
    for bad_value in (-1, 1 << 32):
        w = base.copy()
        w[[3000, 1500, 4999]] = bad_value  # in three scan tiles: the lowest index is reported
        with pytest.raises(ArrayIndexOutOfBoundsException) as e:
            Sampler(w, device=gpu)
        assert e.value.record == 1500
        with pytest.raises(ArrayIndexOutOfBoundsException) as e:
            Sampler(torch.from_numpy(w).to(d))
        assert e.value.record == 1500
        h, bad = C.c_void_p(1), C.c_int64(-9)
        assert lib.glint_sampler_create(gpu, w.ctypes.data, w.size, 0, C.byref(bad), C.byref(h)) == N.GLINT_EOUTOFRANGE
        assert not h.value and bad.value == 1500
        h = C.c_void_p(1)
        assert lib.glint_sampler_create(gpu, w.ctypes.data, w.size, 0, None, C.byref(h)) == N.GLINT_EOUTOFRANGE
        assert not h.value
    w = base.copy()
    w[0] = W_MAX  # the largest weight is fine
    with Sampler(w, device=gpu) as s:
        assert s.total == int(w.sum())
    for m in (1, 1025):  # all-zero weights
        with pytest.raises(ValueError):
            Sampler(np.zeros(m, np.int64), device=gpu)
        with pytest.raises(ValueError):
            Sampler(torch.zeros(m, dtype=torch.int64, device=d))
        h = C.c_void_p(1)
        z = np.zeros(m, np.int64)
        assert lib.glint_sampler_create(gpu, z.ctypes.data, m, 0, None, C.byref(h)) == N.GLINT_EINVAL and not h.value


def test_create_refuses_other_shards(gpu):
    lib = N.load()
    shards = [PartialMatrix(RangePartition(0, 0, 64), 4, "long", gpu), PartialVector(RangePartition(0, 0, 64), "float", gpu),
              PartialVector(RangePartition(0, 0, 64), "double", gpu), PartialVector(CyclicPartition(1, 2, 128), "long", gpu)]
    for sh in shards:
        with sh:
            h = C.c_void_p(1)
            assert lib.glint_sampler_create_from_shard(sh.handle, None, C.byref(h)) == N.GLINT_EINVAL and not h.value
            with pytest.raises((ValueError, TypeError)):
                Sampler.fromShard(sh)


# ---- streams and the use case -------------------------------------------------------------------------
def test_two_streams_draw_at_once(gpu):
    import torch
    d = torch.device("cuda", gpu)
    w, cdf = weights_of(1024 ** 2 + 1, "zipf")
    n = 300_000
    with Sampler(w, device=gpu) as s:
        s1, s2 = torch.cuda.Stream(d), torch.cuda.Stream(d)
        outs = []
        for st, seed, first in ((s1, 1, 0), (s2, 2, 1 << 50), (s1, 3, 5), (s2, 4, 6)):
            with torch.cuda.stream(st):
                outs.append((seed, first, s.draw(n, seed, first, out=torch.empty(n, dtype=torch.int64, device=d), sync=False)))
        s1.synchronize()
        s2.synchronize()
    for seed, first, t in outs:
        np.testing.assert_array_equal(t.cpu().numpy(), replay_draw(w, 0, seed, first, n, cdf=cdf))


def test_skipgram_chain(gpu):
    """draw_dev -> getPairsDot(sync=False) on one stream equals pullPairDot with the host-drawn ids, and the
    same (seed, first) given to a second draw feeds the adjusting push the same rows."""
    import torch
    d = torch.device("cuda", gpu)
    rows, cols, npos, k = 64, 8, 40, 5
    counts = zipf_counts(rows, top=500)
    part = RangePartitioner.apply(1, rows)

    def model(seed):
        sh = PartialMatrix(part.all()[0], cols, "float", gpu)
        sh.initUniform(seed, -0.5, 0.5)
        return sh

    syn0, syn1, syn0_twin = model(1), model(2), model(1)
    big0, big1, big0_twin = (BigMatrix(part, [sh], rows, cols) for sh in (syn0, syn1, syn0_twin))
    centres = np.random.default_rng(0).integers(0, rows, npos).astype(np.int64)
    centres_rep = np.repeat(centres, k)
    seed, first = 2024, 7 * npos * k
    with Sampler(counts, device=gpu) as s:
        host_neg = s.draw(npos * k, seed, first, exclude=centres, per=k)
        np.testing.assert_array_equal(host_neg, replay_draw(counts, 0, seed, first, npos * k, exclude=centres, per=k))
        assert (host_neg != centres_rep).all()
        c_dev, cr_dev = torch.from_numpy(centres).to(d), torch.from_numpy(centres_rep).to(d)
        st = torch.cuda.Stream(d)
        st.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(st):
            neg = s.draw(npos * k, seed, first, exclude=c_dev, per=k, sync=False)
            scores = syn1.getPairsDot(syn0, neg, cr_dev, sync=False)
            # the adjusting call regenerates its negatives
            neg2 = s.draw(npos * k, seed, first, exclude=c_dev, per=k, sync=False)
            coef = -0.05 * torch.sigmoid(scores)
            syn0.updatePairsAxpy(syn1, cr_dev, neg2, coef, deterministic=True, sync=False)
        st.synchronize()
        syn0.sync(st.cuda_stream)
        syn1.sync(st.cuda_stream)
    np.testing.assert_array_equal(neg.cpu().numpy(), host_neg)
    np.testing.assert_array_equal(neg2.cpu().numpy(), host_neg)
    want = big1.pullPairDot(big0_twin, host_neg, centres_rep)
    np.testing.assert_array_equal(bits(scores.cpu().numpy()), bits(want))
    big0_twin.pushPairAxpy(big1, centres_rep, host_neg, coef.cpu().numpy())
    allrows = np.arange(rows, dtype=np.int64)
    np.testing.assert_array_equal(bits(syn0.getRows(allrows)), bits(syn0_twin.getRows(allrows)))
    fresh = model(1)
    assert (bits(syn0.getRows(allrows)) != bits(fresh.getRows(allrows))).any()  # (the push did change rows)
    for sh in (syn0, syn1, syn0_twin, fresh):
        sh.destroy()
