"""The push planners, on a CPU: which kernels a push takes (glint_push_plan.h push_route), which front
end a binned push gets (glint_bin_plan.h bin_front_next) and how its scratch is laid out (bin_layout),
through tests/c/plan_probe.cpp's C wrappers. The expected routes are launch_push's decisions for the
stated inputs; the expected layout is push_binned's size arithmetic restated here in Python."""
import ctypes
import importlib.util
import itertools
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent

DET, UNORDERED, VALIDATE = 1, 2, 4  # GLINT_PUSH_*
HOST_SEQ = 1 << 16                  # kPushHostSequential
INVALID, ORDERED, BINNED_ALL, WHOLE_BIN, SCATTER_ALL, DET_ALL, CHECKED = range(7)  # PushKind
T_SCATTER, T_DET, T_BINNED = range(3)                                              # PushTail


@pytest.fixture(scope="module")
def probe():
    spec = importlib.util.spec_from_file_location("_glint_build", ROOT / "glint_amd" / "build.py")
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return ctypes.CDLL(str(mod.build_plan_probe()))


# ---- routes ------------------------------------------------------------------------------------------
QUERY = ("n", "flags", "fp", "vec_ok", "gated", "ring", "elems", "binnable", "hint_tail", "hint_head",
         "whole_probe", "binned_mode", "bin_density", "whole_on")
ROUTE = ("kind", "tail", "validate", "fuse", "gate_kernel", "scatter_mode", "probe_consumed")
# a 2^22-element Double vector shard, aligned pointers, default knobs
BASE = dict(n=0, flags=0, fp=1, vec_ok=1, gated=0, ring=0, elems=1 << 22, binnable=1, hint_tail=0, hint_head=0,
            whole_probe=0, binned_mode=-1, bin_density=512, whole_on=1)
M = 1 << 20
SPARSE = dict(n=M, hint_tail=M, hint_head=0, bin_density=1 << 40)  # a whole tail, too sparse to bin
GATED = dict(n=M, gated=1, binned_mode=1)

ROUTE_CASES = [
    ("det_message", dict(n=1000, flags=DET), dict(kind=ORDERED)),
    ("det_large", dict(n=(1 << 17) + 1, flags=DET), dict(kind=CHECKED, tail=T_DET)),
    ("det_large_unaligned", dict(n=(1 << 17) + 1, flags=DET, vec_ok=0), dict(kind=DET_ALL)),
    ("int_det_message", dict(n=1000, flags=DET, fp=0), dict(kind=SCATTER_ALL, scatter_mode=1)),
    ("host_message", dict(n=5000, flags=HOST_SEQ), dict(kind=ORDERED)),
    ("host_unordered", dict(n=5000, flags=HOST_SEQ | UNORDERED), dict(kind=BINNED_ALL)),
    ("host_unordered_never_bin", dict(n=5000, flags=HOST_SEQ | UNORDERED, binned_mode=0),
     dict(kind=CHECKED, tail=T_SCATTER, scatter_mode=0)),
    ("small", dict(n=4096), dict(kind=SCATTER_ALL, scatter_mode=1)),
    ("above_small", dict(n=4097), dict(kind=CHECKED, tail=T_SCATTER, scatter_mode=0, probe_consumed=0)),
    ("whole_bin", dict(n=M, hint_tail=M, hint_head=0), dict(kind=WHOLE_BIN, validate=0)),
    ("tail_after_head", dict(n=M, hint_tail=M, hint_head=1024), dict(kind=CHECKED, tail=T_BINNED)),
    *[(f"whole_scatter_probe{p}", dict(SPARSE, whole_probe=p), dict(kind=SCATTER_ALL, scatter_mode=2, probe_consumed=1))
      for p in range(7)],
    ("whole_scatter_8th", dict(SPARSE, whole_probe=7),
     dict(kind=CHECKED, tail=T_SCATTER, scatter_mode=0, probe_consumed=1)),
    ("whole_scatter_off", dict(SPARSE, whole_on=0),
     dict(kind=CHECKED, tail=T_SCATTER, scatter_mode=0, probe_consumed=1)),
    ("gated_validating", dict(GATED, flags=VALIDATE),
     dict(kind=CHECKED, validate=1, fuse=1, gate_kernel=0, tail=T_BINNED)),
    ("gated", dict(GATED), dict(kind=CHECKED, validate=0, fuse=0, gate_kernel=1, tail=T_BINNED)),
    ("gated_message", dict(n=100, gated=1), dict(kind=CHECKED, tail=T_SCATTER, gate_kernel=1)),
    ("gated_det", dict(n=M, gated=1, flags=DET), dict(kind=INVALID)),
    ("gated_unaligned", dict(n=M, gated=1, vec_ok=0), dict(kind=INVALID)),
    ("ring_int", dict(n=1000, fp=0, ring=1), dict(kind=ORDERED)),
]


def route(probe, **over):
    q = dict(BASE, **over)
    inp = (ctypes.c_int64 * len(QUERY))(*[q[k] for k in QUERY])
    out = (ctypes.c_int32 * len(ROUTE))()
    probe.plan_route(inp, out)
    return dict(zip(ROUTE, out))


@pytest.mark.parametrize("query,expect", [c[1:] for c in ROUTE_CASES], ids=[c[0] for c in ROUTE_CASES])
def test_route(probe, query, expect):
    got = route(probe, **query)
    assert {k: got[k] for k in expect} == expect, got


def test_route_wide_shard_is_not_ordered(probe):
    # the ordered fold addresses elements with 32 bits (and such a shard cannot be binned either)
    got = route(probe, n=1000, flags=DET, elems=1 << 32, binnable=0)
    assert got["kind"] == CHECKED and got["tail"] == T_DET, got
    assert route(probe, n=1000, flags=DET, elems=(1 << 32) - 1)["kind"] == ORDERED


# ---- front end ---------------------------------------------------------------------------------------
NO_HINT = (0, 0, 0, -1)


def fronts(probe, steps):
    """steps: (hint m, hint tail, hint cold, hint_bin_front[, forced]) per push of a fresh shard ->
    (front, hot_refresh, pushes, last_front, hot_age) per push"""
    flat = [v for s in steps for v in (tuple(s) + (-1,))[:5]]
    inp = (ctypes.c_int64 * len(flat))(*flat)
    out = (ctypes.c_int32 * (5 * len(steps)))()
    probe.plan_front(inp, len(steps), out)
    return [tuple(out[5 * i:5 * i + 5]) for i in range(len(steps))]


def test_front_fresh_state_probes_every_16th(probe):
    got = fronts(probe, [NO_HINT] * 17)
    assert [g[0] for g in got] == [2] + [0] * 15 + [2]
    assert [g[2] for g in got] == list(range(1, 18))


def test_front_dedup_that_merges_stays(probe):
    merged = (500, 1000, 1000, 2)  # the dedup push kept half of its cold records
    got = fronts(probe, [NO_HINT] + [merged] * 20)
    assert [g[0] for g in got] == [2] * 21


def test_front_hot_split_keeps_its_table_for_eight_pushes(probe):
    hot = (700, 1000, 700, 2)  # dedup merged nothing (ratio 1.0), the hot elements took 30 % of the tail
    got = fronts(probe, [NO_HINT] + [hot] * 18)
    assert [g[0] for g in got] == [2] + [1] * 15 + [2] + [1] * 2  # push 16 is the dedup probe
    refresh = [g[1] for g in got]
    assert refresh[1] == 1            # the first hot push samples
    assert refresh[2:9] == [0] * 7    # ... the next seven keep the table
    assert refresh[9] == 1            # ... and the eighth after it samples again
    assert refresh[10:16] == [0] * 6
    assert refresh[17] == 1           # a push after another front end samples at once
    assert refresh[18] == 0
    assert [g[4] for g in got[1:10]] == [1, 2, 3, 4, 5, 6, 7, 8, 1]
    assert all(r == 1 for g, r in zip(got, refresh) if g[0] != 1)


@pytest.mark.parametrize("writer", [0, 1])
def test_front_hint_of_another_front_end_changes_nothing(probe, writer):
    # m, tail and cold that would call for dedup (and for the hot split), had a dedup push measured them
    got = fronts(probe, [NO_HINT] + [(100, 1000, 500, writer)] * 16)
    assert got == fronts(probe, [NO_HINT] * 17)


def test_front_forced_still_advances_history(probe):
    got = fronts(probe, [NO_HINT + (0,), NO_HINT + (1,), NO_HINT + (2,), NO_HINT])
    assert [g[0] for g in got] == [0, 1, 2, 0]
    assert [g[2] for g in got] == [1, 2, 3, 4]
    assert [g[3] for g in got] == [0, 1, 2, 0]
    assert got[1][1] == 1 and got[1][4] == 1


# ---- layout ------------------------------------------------------------------------------------------
SCALARS = ("small_push", "per", "kchunk", "nchunks_max", "wpc", "G", "item", "max_fitems", "max_units", "nstride",
           "ctstride", "fb", "nb", "nf", "nslab")
BUFFERS = ("ct", "P", "Q", "Bb", "Ib", "fitems", "cwin", "off2", "units", "runs", "hot_tags", "wpart", "addr_a",
           "val_a", "val_b", "e_b")
LAYOUT = SCALARS + BUFFERS + ("need",)


def pad256(b):
    return (b + 255) & ~255


def u32(x):
    return x & 0xFFFFFFFF


def parent_geometry(elems, cbmin):
    slabs = (elems + 4096 - 1) // 4096
    sb = 0
    while (1 << sb) < slabs:
        sb += 1
    cb = min(sb, max(cbmin, sb - 10 if sb > 10 else 0))
    fb = sb - cb
    return fb, 1 << cb, 1 << fb, u32((1 << cb) * (1 << fb))


def parent_layout(elems, n, cus, front, acc, hot_occ):
    """push_binned's sizes and pointer carving as it stood before bin_layout, at the default build knobs
    (slabs of 4096, 1024-thread partition chunks of 4 or 8 records per thread, 1024 x 12-record fine
    items, units of 4096 records / 128 runs, 2048 / 8192 hot slots, 7 coarse bits at least)."""
    small = parent_geometry(elems, 7)[1] + n // (1024 * 12) + 1 <= 4 * cus
    per = 8 if front == 0 and not small else 4
    fb, nb, nf, nslab = parent_geometry(elems, 7 if per == 8 else 6)
    kchunk = 1024 * per
    nchunks_max = (n + kchunk - 1) // kchunk
    wpc = 1 if front == 2 else min(1, hot_occ) if front == 1 else 1
    G = u32(max(1, min(nchunks_max, cus * wpc)))
    item = 1024 * 12
    max_fitems = nb + n // item + 1
    max_units = nslab + n // 4096 + min(n, max_fitems * nf) // 128 + 1
    nstride = u32(nchunks_max)
    ctstride = u32(nstride + 1)
    b_ct = pad256(ctstride * nb * 4)
    b_p = pad256(nb * u32(nstride + 1) * 4)
    b_pq = b_p + pad256(nb * nstride * 4)
    b_nb = pad256(nb * 4)
    b_fit = 2 * pad256(max_fitems * 8)
    b_off2 = pad256(max_fitems * u32(nf + 1) * 4)
    b_units = pad256(max_units * 16) + pad256(max_units * 128 * 8)
    b_hot = pad256(2048 * 4)
    b_wpart = pad256(G * 8192 * acc) if front == 1 else 0
    b_a, b_v, b_e = pad256(n * 4), pad256(n * acc), pad256(n * 2)
    need = b_ct + b_pq + 2 * b_nb + b_fit + b_off2 + b_units + b_hot + b_wpart + b_a + 2 * b_v + b_e
    out = dict(small_push=int(small), per=per, kchunk=kchunk, nchunks_max=nchunks_max, wpc=wpc, G=G, item=item,
               max_fitems=max_fitems, max_units=max_units, nstride=nstride, ctstride=ctstride, fb=fb, nb=nb, nf=nf,
               nslab=nslab, need=need)
    p = 0
    out["ct"] = p
    p += b_ct
    out["P"], out["Q"] = p, p + b_p
    p += b_pq
    out["Bb"], out["Ib"] = p, p + b_nb
    p += 2 * b_nb
    out["fitems"], out["cwin"] = p, p + pad256(max_fitems * 8)
    p += b_fit
    out["off2"] = p
    p += b_off2
    out["units"], out["runs"] = p, p + pad256(max_units * 16)
    p += b_units
    out["hot_tags"] = p
    p += b_hot
    out["wpart"] = p
    p += b_wpart
    out["addr_a"], out["val_a"], out["val_b"], out["e_b"] = p, p + b_a, p + b_a + b_v, p + b_a + 2 * b_v
    return out


def layout(probe, *args):
    inp = (ctypes.c_int64 * 6)(*args)
    out = (ctypes.c_int64 * len(LAYOUT))()
    probe.plan_layout(inp, out)
    return dict(zip(LAYOUT, out))


ELEMS = (1, 4096, 4097, 1 << 20, 1 << 28, (1 << 32) - 2)
RECORDS = (1, 4095, 4096, 1 << 20, 1 << 26)


@pytest.mark.parametrize("elems", ELEMS)
def test_layout_is_the_parents(probe, elems):
    for n, cus, front, acc in itertools.product(RECORDS, (1, 256), (0, 1, 2), (4, 8)):
        got = layout(probe, elems, n, cus, front, acc, 1)
        case = (elems, n, cus, front, acc)
        assert got == parent_layout(elems, n, cus, front, acc, 1), case
        offs = [got[b] for b in BUFFERS] + [got["need"]]
        assert all(o % 256 == 0 for o in offs), case
        assert offs[0] == 0 and offs == sorted(offs), case  # the parent's order, none overlapping
        size = {b: offs[i + 1] - offs[i] for i, b in enumerate(BUFFERS)}
        assert (size["wpart"] > 0) == (front == 1), case
        assert size["wpart"] == (pad256(got["G"] * 8192 * acc) if front == 1 else 0), case
        # every buffer holds what its kernels index: the record buffers n entries, the tables their rows
        assert size["addr_a"] >= 4 * n and size["val_a"] >= acc * n and size["val_b"] >= acc * n, case
        assert size["e_b"] >= 2 * n and size["ct"] >= 4 * got["ctstride"] * got["nb"], case
        assert size["hot_tags"] == 2048 * 4, case


def test_layout_hot_occupancy_caps_the_hot_front_end_only(probe):
    for occ in (1, 2, 4):
        for front in (0, 1, 2):
            got = layout(probe, 1 << 28, 1 << 26, 256, front, 8, occ)
            assert got == parent_layout(1 << 28, 1 << 26, 256, front, 8, occ)
            assert got["wpc"] == 1
