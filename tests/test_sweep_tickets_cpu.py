"""The affine sweep's ticket arithmetic on a CPU (glint_push_plan.h sweep_ticket_count / sweep_ticket,
through tests/c/sweep_probe.cpp): for a push of n records swept by S blocks, the tickets [0, count)
cover the record pairs [0, n >> 1) exactly once and touch no pair outside. Small sizes are walked pair
by pair in the probe; the large ones are checked in closed form at the boundaries: every row of 256
pairs belongs to exactly one (ticket, row) and that ticket is below the count."""
import ctypes
import importlib.util
import random
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
TILE = 1024                          # kTile: records per wave tile
N_MAX = (0xFFFFFFF0 - 1) * TILE      # the largest n launch_push accepts (ntiles < 0xFFFFFFF0)
BLOCKS = (1, 256, 304)


@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("_glint_build", ROOT / "glint_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    lib = ctypes.CDLL(str(mod.build_sweep_probe()))
    lib.sweep_count.restype = ctypes.c_uint64
    lib.sweep_count.argtypes = [ctypes.c_int64, ctypes.c_uint32]
    lib.sweep_ticket_at.argtypes = [ctypes.c_uint64, ctypes.c_uint32, ctypes.POINTER(ctypes.c_int64)]
    lib.sweep_cover.restype = ctypes.c_int
    lib.sweep_cover.argtypes = [ctypes.c_int64, ctypes.c_uint32]
    lib.sweep_constants.argtypes = [ctypes.POINTER(ctypes.c_int64)]
    lib.tile_count.restype = ctypes.c_uint64
    lib.tile_count.argtypes = [ctypes.c_int64, ctypes.c_uint32]
    lib.tile_cover.restype = ctypes.c_int
    lib.tile_cover.argtypes = [ctypes.c_int64, ctypes.c_uint32]
    return lib


def constants(probe):
    out = (ctypes.c_int64 * 3)()
    probe.sweep_constants(out)
    return int(out[0]), int(out[1]), int(out[2])  # records per ticket, rows per ticket, pairs per row


def ticket(probe, t, S):
    out = (ctypes.c_int64 * 2)()
    probe.sweep_ticket_at(t, S, out)
    return int(out[0]), int(out[1])


def small_sizes(C, S):
    return [1, 2, 3, C - 1, C, C + 1, S * C - 1, S * C, S * C + 1, 3 * S * C + C // 2 + 1]


def test_constants(probe):
    C, rows, row_pairs = constants(probe)
    assert C == 2 * rows * row_pairs
    assert row_pairs == 256  # one pair per thread of a push_apply block


@pytest.mark.parametrize("S", BLOCKS)
def test_cover_exhaustive(probe, S):
    C, _, _ = constants(probe)
    for n in small_sizes(C, S):
        assert probe.sweep_cover(n, S) == 0, (n, S)


@pytest.mark.parametrize("S", BLOCKS)
def test_count_small(probe, S):
    C, _, _ = constants(probe)
    assert probe.sweep_count(1, S) == 0          # one record: no pair, the odd record is added apart
    assert probe.sweep_count(2, S) == 1
    assert probe.sweep_count(3, S) == 1
    assert probe.sweep_count(S * C, S) == S      # one super-window: every ticket is some block's first
    assert probe.sweep_count(S * C + 1, S) == S  # ... and the odd record adds no pair
    assert probe.sweep_count(S * C + 2, S) == S + 1  # the first ticket that comes from the counter


@pytest.mark.parametrize("S", BLOCKS)
@pytest.mark.parametrize("n", [1 << 30, N_MAX, N_MAX - 1, N_MAX - 2 * 256 * 7 - 1])
def test_cover_closed_form(probe, n, S):
    """Row rho of 256 pairs sits in super-window rho // (rows * S), at row (rho % (rows * S)) // S of
    slot rho % S. That map is one to one, so the cover is exact iff sweep_ticket agrees with it, every
    row below ceil(npairs / 256) lands on a ticket below the count, and the ticket `count` and its
    successors start at or past the last pair."""
    C, rows, rp = constants(probe)
    npairs = n >> 1
    nrows = (npairs + rp - 1) // rp
    count = probe.sweep_count(n, S)
    assert count + S < 1 << 32  # the counter is 32 bits and runs at most S past the count
    per_sw = rows * S
    rng = random.Random(n ^ S)
    edge = [0, 1, S - 1, S, per_sw - 1, per_sw, nrows - 1, nrows - 2, nrows - S, nrows - per_sw,
            nrows // per_sw * per_sw, nrows // per_sw * per_sw - 1]
    for rho in [r for r in edge if 0 <= r < nrows] + [rng.randrange(nrows) for _ in range(2000)]:
        sw, within = divmod(rho, per_sw)
        r, slot = divmod(within, S)
        t = sw * S + slot
        assert t < count, (rho, t, count)
        first, stride = ticket(probe, t, S)
        assert stride == S * rp
        assert first + r * stride == rho * rp
        assert 0 <= first < npairs
    # the rows past the last one belong to no counted ticket's in-range part, and no ticket from
    # `count` on starts inside the range
    for t in (count, count + 1, count + S - 1, count + S):
        first, _ = ticket(probe, t, S)
        assert first >= npairs, (t, first, npairs)
    # tickets are counted densely: the last one exists, and the tickets of the last super-window are
    # its first slots
    first, _ = ticket(probe, count - 1, S)
    assert first < npairs
    full, rem = divmod(npairs, per_sw * rp)
    assert count == full * S + min(S, (rem + rp - 1) // rp)


@pytest.mark.parametrize("G", [1, 256, 512, 608])
def test_tile_tickets_cover(probe, G):
    """The tile path of push_apply takes tickets by the same arithmetic in wave tiles (rows of the 4
    tiles of a block's waves): the tickets cover the tiles [0, tiles) exactly once. G = blocks of the
    launch; a ticket is 4 * rows tiles."""
    per = G * 4  # tiles per row of the whole grid
    for tiles in [0, 1, 3, 4, 5, per - 1, per, per + 1, 8 * per - 1, 8 * per, 8 * per + 1, 3 * 8 * per + 17,
                  (1 << 28) // TILE]:
        assert probe.tile_cover(tiles, G) == 0, (tiles, G)
    assert probe.tile_count(0, G) == 0
    assert probe.tile_count(8 * per, G) == G
    assert probe.tile_count(8 * per + 1, G) == G + 1
