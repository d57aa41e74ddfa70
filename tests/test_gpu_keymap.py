"""Device key map on the GPU (glint_keymap_*): every row is compared with a Python dict replayed in call order
-- over the wave, scan-tile and scan-level edges of a call's size (the scan tile is 1024), tables one key
short of full whose chains wrap the table's end, one hot key, calls that mix present and new keys, the
roll-back of an overflowing call, the reserved key, both forms, and the device-resident chain the map exists
for. Everything is integer-exact."""
import numpy as np
import pytest

from glint_amd import ArrayIndexOutOfBoundsException, KeyMap, KeyMapFullException, PartialMatrix, RangePartition

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
FIRST = 1 << 40
FORMS = ("host", "dev")


class Replay:
    """The contract as a dict: rows in call order, an overflowing or reserved-key call changes nothing."""

    def __init__(self, capacity, first=FIRST):
        self.rows, self.capacity, self.first = {}, capacity, first

    def insert(self, keys):
        keys = [int(k) for k in keys]
        new = dict.fromkeys(k for k in keys if k not in self.rows)
        if I64_MIN in new or len(self.rows) + len(new) > self.capacity:
            return self.lookup(keys)
        for k in new:
            self.rows[k] = self.first + len(self.rows)
        return self.lookup(keys)

    def lookup(self, keys, missing=-1):
        return np.array([self.rows.get(int(k), missing) for k in keys], np.int64)


def call(fn, x, form, gpu, **kw):
    """fn over x in the host form, or in the device form with a pre-filled out tensor."""
    x = np.ascontiguousarray(x, np.int64)
    if form == "host":
        return fn(x, **kw)
    import torch
    d = torch.device("cuda", gpu)
    out = torch.full((x.size,), -77, dtype=torch.int64, device=d)
    return fn(torch.from_numpy(x).to(d), out=out, **kw).cpu().numpy()


_cases = {}


def sized_case(n):
    """(keys, rows, distinct keys in insertion order) of a size, computed once: about half of the records
    repeat, and the keys include negatives, INT64_MAX and INT64_MIN + 1."""
    if n not in _cases:
        keys = np.random.default_rng(n).integers(-(n // 3) - 1, n // 3 + 1, n).astype(np.int64)
        keys[:1] = I64_MAX
        keys[n // 2:n // 2 + 1] = I64_MIN + 1
        keys[max(n - 1, 2):] = I64_MAX
        ref = Replay(n + 8)
        _cases[n] = (keys, ref.insert(keys), np.array(list(ref.rows), np.int64))
    return _cases[n]


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("n", (0, 1, 63, 64, 65, 1024, 1025, 1024 ** 2 + 1))
def test_sizes(gpu, n, form):
    keys, rows, order = sized_case(n)
    with KeyMap(n + 8, FIRST, gpu) as km:
        assert km.info() == (n + 8, FIRST, km.slots, 0, gpu) and km.slots >= 2 * (n + 8) > km.slots // 2
        np.testing.assert_array_equal(call(km.insert, keys, form, gpu), rows)
        assert km.size() == order.size
        probe = np.concatenate([keys, keys[:4096] + (10 * n + 7)])  # the shifted ones (one wraps) are absent
        want = np.concatenate([rows, np.full(probe.size - n, -5)])
        np.testing.assert_array_equal(call(km.lookup, probe, form, gpu, missing=-5), want)
        np.testing.assert_array_equal(call(km.keysOf, FIRST + np.arange(order.size), form, gpu), order)
        if n:
            with pytest.raises(ArrayIndexOutOfBoundsException) as e:
                km.keysOf(np.array([FIRST, FIRST + order.size, FIRST - 1]))
            assert e.value.record == 1


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("slots", (2, 8, 1024))
def test_tight_tables(gpu, slots, form):
    cap = slots - 1
    keys = np.random.default_rng(slots).choice(np.arange(-5 * slots, 5 * slots), cap, replace=False) * 7919
    ref = Replay(cap)
    with KeyMap(cap, FIRST, gpu, slots=slots) as km:
        assert km.slots == slots
        done = keys[:0]
        for part in np.array_split(keys, 3):  # each call repeats the keys before it
            batch = np.concatenate([done[::-1], part, part])
            np.testing.assert_array_equal(call(km.insert, batch, form, gpu), ref.insert(batch))
            done = np.concatenate([done, part])
        assert km.size() == cap
        probe = np.concatenate([keys, keys + 1])  # one empty slot ends every miss
        np.testing.assert_array_equal(call(km.lookup, probe, form, gpu), ref.lookup(probe))
        np.testing.assert_array_equal(call(km.keysOf, FIRST + np.arange(cap), form, gpu), keys)


def test_one_hot_key(gpu):
    with KeyMap(16, FIRST, gpu) as km:
        km.insert(np.array([5, 6, 7]))
        rows = call(km.insert, np.full(65537, -42), "dev", gpu)
        assert (rows == FIRST + 3).all() and km.size() == 4


@pytest.mark.parametrize("form", FORMS)
def test_present_and_new_keys_and_a_split_call(gpu, form):
    rng = np.random.default_rng(3)
    old = rng.permutation(3000)[:1500] - 1500
    mixed = rng.integers(-1500, 4000, 2501)
    ref = Replay(8000)
    ref.insert(old)
    want = ref.insert(mixed)
    with KeyMap(8000, FIRST, gpu) as one, KeyMap(8000, FIRST, gpu, slots=1 << 17) as two:
        for km in (one, two):
            km.insert(old)
        np.testing.assert_array_equal(call(one.insert, mixed, form, gpu), want)
        parts = [call(two.insert, p, form, gpu) for p in (mixed[:1237], mixed[1237:])]
        np.testing.assert_array_equal(np.concatenate(parts), want)
        assert one.size() == two.size() == len(ref.rows)
        np.testing.assert_array_equal(one.lookup(old), ref.lookup(old))


@pytest.mark.parametrize("form", FORMS)
def test_overflow_rolls_back(gpu, form):
    ref = Replay(7)
    old = np.array([11, -3, 19, 27])
    over = np.array([19, 100, 101, 11, 100, 102, 103, -3])  # four new keys, three free rows
    absent = np.array([100, 101, 102, 103, 3, 35])
    with KeyMap(7, FIRST, gpu, slots=8) as km:
        km.insert(old)
        ref.insert(old)
        if form == "host":
            with pytest.raises(KeyMapFullException) as e:
                km.insert(over)
        else:
            import torch
            out = torch.full((over.size,), -77, dtype=torch.int64, device=f"cuda:{gpu}")
            km.insert(torch.from_numpy(over).to(out.device), out=out, sync=False)
            with pytest.raises(KeyMapFullException) as e:
                km.sync()
            np.testing.assert_array_equal(out.cpu().numpy(), ref.insert(over))
            km.sync()  # reported once
        assert e.value.free == 3 and e.value.record == -1 and len(ref.rows) == 4
        assert km.size() == 4
        np.testing.assert_array_equal(km.lookup(old), ref.lookup(old))
        np.testing.assert_array_equal(km.lookup(absent), np.full(absent.size, -1))
        fill = np.array([103, 11, 3, 103, 101])  # exactly the free count
        np.testing.assert_array_equal(call(km.insert, fill, form, gpu), ref.insert(fill))
        assert km.size() == 7
        np.testing.assert_array_equal(km.keysOf(FIRST + np.arange(7)), np.array(list(ref.rows)))


@pytest.mark.parametrize("form", FORMS)
def test_reserved_key(gpu, form):
    old = np.array([4, 5])
    bad = np.array([5, 9, 8, I64_MIN, 4, I64_MIN, 9])
    with KeyMap(16, FIRST, gpu) as km:
        km.insert(old)
        for fn in (km.insert, km.lookup):
            with pytest.raises(ArrayIndexOutOfBoundsException) as e:
                call(fn, bad, form, gpu)
            assert e.value.record == 3 and not isinstance(e.value, KeyMapFullException)
        assert km.size() == 2
        np.testing.assert_array_equal(km.lookup(np.array([4, 5, 8, 9])), [FIRST, FIRST + 1, -1, -1])
        np.testing.assert_array_equal(km.insert(np.array([9, 8])), [FIRST + 2, FIRST + 3])


def test_device_resident_chain(gpu):
    """insert -> updateRows -> lookup -> getRows on one non-default stream with nothing waiting in between,
    bit for bit the host-form twin on a second shard."""
    import torch
    d = torch.device("cuda", gpu)
    rng = np.random.default_rng(9)
    ids = rng.integers(-400, 400, 3001) * ((1 << 50) + 12345)
    vals = rng.standard_normal((ids.size, 24)).astype(np.float32)
    part = RangePartition(0, 0, 1024)
    with KeyMap(1024, 0, gpu) as km, KeyMap(1024, 0, gpu) as twin, \
            PartialMatrix(part, 24, "float", gpu) as sh, PartialMatrix(part, 24, "float", gpu) as sh2:
        st = torch.cuda.Stream(d)
        ids_d, vals_d = torch.from_numpy(ids).to(d), torch.from_numpy(vals).to(d)
        st.wait_stream(torch.cuda.current_stream(d))
        with torch.cuda.stream(st):
            rows_d = km.insert(ids_d, sync=False)
            sh.updateRows(rows_d, vals_d, deterministic=True, sync=False)
            got = sh.getRows(km.lookup(ids_d, sync=False), sync=False)
            km.sync()
            sh.sync(st.cuda_stream)
        sh2.updateRows(twin.insert(ids), vals)
        want = sh2.getRows(twin.lookup(ids))
        np.testing.assert_array_equal(rows_d.cpu().numpy(), twin.lookup(ids))
        assert got.cpu().numpy().tobytes() == want.tobytes()
