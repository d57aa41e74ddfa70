"""The dense push's affine sweep in one launch with ticketed chunks (apply_sweep, glint_gpu.hip).

A dense push (keys start, start + 1, ...) is one affine run: push_apply sweeps it with S = one block per CU,
each block taking tickets of C records (sweep_ticket, glint_push_plan.h). Block b starts on ticket b; the
tickets from S on come from the push's counter (LaunchCtl.ticket), which the previous push's check -- or
the binned count of a whole-push bin -- zeroes. Values are integer-valued, so every dtype compares bit for
bit against the closed form: element e holds (pushes so far) x (value of record e - delta).
"""
import ctypes as C

import pytest

from glint_amd import _native as N
from glint_amd import PartialMatrix, PartialVector, RangePartition

pytestmark = pytest.mark.gpu

TICKET = 8192  # C: records per ticket, kSweepTicketRecords (16 rows of 256 record pairs)
TILE_TICKET = 8 * 4 * 1024  # records per ticket of the tile path: kTileTicketRows rows of kTileRowTiles wave tiles
MARGIN = 5     # shard elements past the push: they must stay zero
TORCH_DT = {"double": "float64", "float": "float32", "long": "int64", "int": "int32"}


def cus(gpu):
    import torch
    return torch.cuda.get_device_properties(gpu).multi_processor_count


def sizes(gpu):
    """Around one ticket, around the S tickets that need no counter (S * C + 2 records are the first to
    take a ticket from it: an odd last record adds no pair), and three super-windows and a half ticket."""
    S, c = cus(gpu), TICKET
    return [1, 2, 3, c - 1, c, c + 1, 2 * c + 1, S * c - 1, S * c + 1, S * c + 2, 3 * S * c + c // 2 + 1]


def values(n, dtype, d):
    """Record r carries r % 1021 + 1: integer-valued and small enough that a few pushes stay exact in
    every dtype."""
    import torch
    return (torch.arange(n, dtype=torch.int64, device=d) % 1021 + 1).to(getattr(torch, TORCH_DT[dtype]))


def launches(sh, kid):
    ms, cnt = C.c_double(), C.c_int64()
    assert N.load().glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt)) == N.GLINT_OK
    return cnt.value


@pytest.mark.parametrize("off", [0, 1], ids=["even_delta", "odd_delta"])
@pytest.mark.parametrize("dtype", ["double", "long", "float", "int"])
def test_dense_push_sizes(gpu, dtype, off):
    """Every size, pushed twice with no sync in between, keys from the partition's start (even delta)
    or one past it (odd delta); the shard is a few elements longer than the push."""
    import torch
    d = torch.device("cuda", gpu)
    ns = sizes(gpu) if dtype in ("double", "long") else sizes(gpu)[-4:]  # Float/Int: the 8-byte pair path
    for n in ns:
        size = n + off + MARGIN
        with PartialVector(RangePartition(0, 0, size), dtype, gpu) as sh:
            keys = torch.arange(off, off + n, dtype=torch.int64, device=d)
            vals = values(n, dtype, d)
            sh.update(keys, vals, sync=False)
            sh.update(keys, vals)
            got = sh.get(torch.arange(size, dtype=torch.int64, device=d))
            want = torch.zeros(size, dtype=vals.dtype, device=d)
            want[off:off + n] = 2 * vals
            assert torch.equal(got, want), f"{dtype} n={n} delta={off}"


@pytest.mark.parametrize("dtype", ["double", "long"])
def test_counter_is_zeroed_for_the_next_push(gpu, dtype):
    """The ticket counter of a push is zeroed by the push before it: three dense pushes back to back,
    a push of shuffled keys (check + an unordered tail), a gated push whose gate is set (it applies
    nothing and takes no ticket), then dense pushes again -- the first of them may be taken whole by the
    unordered path the shuffled push announced, the ones after it sweep again."""
    import torch
    d = torch.device("cuda", gpu)
    n = 3 * cus(gpu) * TICKET + TICKET // 2 + 1
    size = n + MARGIN
    tdt = getattr(torch, TORCH_DT[dtype])
    all_keys = torch.arange(size, dtype=torch.int64, device=d)
    with PartialVector(RangePartition(0, 0, size), dtype, gpu) as sh:
        keys = torch.arange(n, dtype=torch.int64, device=d)
        vals = values(n, dtype, d)
        ref = torch.zeros(size, dtype=tdt, device=d)
        for _ in range(3):
            sh.update(keys, vals, sync=False)
            ref[:n] += vals
        assert torch.equal(sh.get(all_keys), ref), "three dense pushes"
        g = torch.Generator(device="cpu").manual_seed(5)
        shuffled = torch.randperm(size, generator=g)[:1 << 21].to(d)
        svals = values(1 << 21, dtype, d)
        sh.update(shuffled, svals)
        ref[shuffled] += svals  # distinct keys
        assert torch.equal(sh.get(all_keys), ref), "shuffled push"
        on = torch.ones(1, dtype=torch.int64, device=d)
        sh.update(keys, vals, gate=on)
        assert torch.equal(sh.get(all_keys), ref), "gated push with its gate set"
        for i in range(3):
            sh.update(keys, vals)
            ref[:n] += vals
            assert torch.equal(sh.get(all_keys), ref), f"dense push {i + 1} after the gated one"


@pytest.mark.parametrize("off", [0, 1], ids=["even_delta", "odd_delta"])
@pytest.mark.parametrize("dtype", ["double", "long"])
def test_dense_matrix_push(gpu, dtype, off):
    """A dense row-major matrix push (element off, off + 1, ... of a 512-column shard whose pitch is its
    width) is one affine run too: the MAT instance of the sweep."""
    import torch
    d = torch.device("cuda", gpu)
    cols = 512
    for n in sizes(gpu)[-4:]:
        rows = (n + off + MARGIN + cols - 1) // cols
        with PartialMatrix(RangePartition(0, 0, rows), cols, dtype, gpu) as sh:
            flat = torch.arange(off, off + n, dtype=torch.int64, device=d)
            r, c = flat // cols, (flat % cols).to(torch.int32)
            vals = values(n, dtype, d)
            sh.update(r, c, vals, sync=False)
            sh.update(r, c, vals)
            got = sh.getRows(torch.arange(rows, dtype=torch.int64, device=d)).reshape(-1)
            want = torch.zeros(rows * cols, dtype=vals.dtype, device=d)
            want[off:off + n] = 2 * vals
            assert torch.equal(got, want), f"{dtype} n={n} delta={off}"


@pytest.mark.parametrize("dtype", ["long", "double"])
def test_one_apply_launch_per_push(gpu, dtype):
    """A push of 2 * 2^26 + 1 records -- three launches when the sweep ran in 2^26-record windows -- is
    one push_apply launch, and its odd last record is added once per push (the shard's state is what
    test_windowed_sweep_odd_record_once expects after two pushes)."""
    import torch
    d = torch.device("cuda", gpu)
    n = (2 << 26) + 1
    with PartialVector(RangePartition(0, 0, n + 5), dtype, gpu) as sh:
        keys = torch.arange(n, dtype=torch.int64, device=d)
        if dtype == "long":
            vals = torch.arange(1, n + 1, dtype=torch.int64, device=d)
        else:
            vals = torch.arange(1, n + 1, dtype=torch.float64, device=d) * 0.5
        assert N.load().glint_prof_enable(sh.handle, 1) == N.GLINT_OK
        sh.update(keys, vals)
        assert launches(sh, N.GLINT_K_PUSH_APPLY) == 1
        assert N.load().glint_prof_enable(sh.handle, 0) == N.GLINT_OK
        sh.update(keys, vals)
        got = sh.get(torch.arange(n + 5, dtype=torch.int64, device=d))
        want = torch.zeros(n + 5, dtype=vals.dtype, device=d)
        want[:n] = 2 * vals
        assert torch.equal(got, want), f"{dtype} n={n}"


def tile_sizes(gpu):
    """Around one ticket of the tile path and around the G tickets that need no counter, G = the blocks
    of the launch: one or two per CU, whatever the kernel's occupancy allows."""
    S, c = cus(gpu), TILE_TICKET
    return [c + 1, S * c - 1, S * c + 1025, 2 * S * c - 1, 2 * S * c + 1025, 6 * S * c + c // 2 + 1]


@pytest.mark.parametrize("dtype", ["double", "long"])
def test_ordered_non_affine_push(gpu, dtype):
    """Keys 2 i + 1: increasing, so push_apply takes every record, and no wave tile is affine, so it
    takes them by wave tiles (apply_general), in tickets of tile groups. Pushed twice back to back."""
    import torch
    d = torch.device("cuda", gpu)
    for n in tile_sizes(gpu):
        size = 2 * n + MARGIN
        with PartialVector(RangePartition(0, 0, size), dtype, gpu) as sh:
            keys = torch.arange(n, dtype=torch.int64, device=d) * 2 + 1
            vals = values(n, dtype, d)
            sh.update(keys, vals, sync=False)
            sh.update(keys, vals)
            got = sh.get(torch.arange(size, dtype=torch.int64, device=d))
            want = torch.zeros(size, dtype=vals.dtype, device=d)
            want[1:2 * n:2] = 2 * vals
            assert torch.equal(got, want), f"{dtype} n={n}"


def test_tile_path_stops_at_the_break(gpu):
    """An ordered head of mixed tiles (an affine run, then keys two apart) in front of a shuffled tail:
    the tickets cover the tiles before the break, the tail goes its own way, and the dense pushes after
    it sweep on a zeroed counter."""
    import torch
    d = torch.device("cuda", gpu)
    S = cus(gpu)
    h_aff, h_gen = S * TILE_TICKET + 1024, 2 * S * TILE_TICKET + 1024 * 3
    size = h_aff + 2 * h_gen + MARGIN
    g = torch.Generator(device="cpu").manual_seed(11)
    tail = torch.randint(0, size, (1 << 20,), generator=g).to(d)
    keys = torch.cat([torch.arange(h_aff, dtype=torch.int64, device=d),
                      h_aff + 2 * torch.arange(h_gen, dtype=torch.int64, device=d), tail])
    vals = values(keys.numel(), "long", d)
    all_keys = torch.arange(size, dtype=torch.int64, device=d)
    dense = torch.arange(size - MARGIN, dtype=torch.int64, device=d)
    dvals = values(dense.numel(), "long", d)
    with PartialVector(RangePartition(0, 0, size), "long", gpu) as sh:
        ref = torch.zeros(size, dtype=torch.int64, device=d)
        for i in range(2):
            sh.update(keys, vals, sync=False)
            ref.index_add_(0, keys, vals)
            sh.update(dense, dvals, sync=False)
            ref[:dense.numel()] += dvals
        assert torch.equal(sh.get(all_keys), ref)
