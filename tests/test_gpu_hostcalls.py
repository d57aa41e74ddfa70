"""The host-pointer calls that tests/sequence_cases.py does not run -- the Adagrad row push, the row-pair
dot pull and axpy push, fill and uniform init -- under both staging routes: GLINT_PINNED_STAGE_MAX=0 (every
section its own copy from pageable memory, answers straight into the caller's array) and the default (one
pinned block, the pair dot's answer through it).

Expected values are the single-operation tests' replays (adagrad_cases, pair_cases, init_cases), compared
bit for bit. With 257 records each family also takes a rejected message first: a row outside the partition
at index 5 raises with that index and changes neither shard, and the same call with the row put right then
gives the replay's result, so the rejected call left the staging buffers usable."""
import zlib

import numpy as np
import pytest

import glint_amd._native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, RangePartition
from adagrad_cases import adagrad_inputs, replay_adagrad, start_tables
from axpy_cases import assert_bits
from dot_cases import assert_dot_bits
from ieee_cases import write_image
from init_cases import global_rows, replay_fill, replay_uniform
from pair_cases import pair_coef, pair_values, replay_pair_axpy, replay_pair_dot

pytestmark = pytest.mark.gpu

SIZE, COLS = 300, 33
PAD = 777
LR, EPS = 0.05, 1e-6
SEED, LO, HI = (0xC0FFEE << 32) | 0x1234567, -0.005, 0.005
NPD = {"float": "float32", "long": "int64"}
# (partition of the first shard, records): one record; 257 with repeated rows -- the pair dot's answer is
# then larger than one 256-byte pad of the pinned block; the same on a cyclic partition
CASES = [("range", 1), ("range", 257), ("cyclic", 257)]
CASE_IDS = [f"{p}-{n}" for p, n in CASES]


@pytest.fixture(params=["0", "default"])
def staging(request, monkeypatch):
    if request.param == "0":
        monkeypatch.setenv("GLINT_PINNED_STAGE_MAX", "0")
    else:
        monkeypatch.delenv("GLINT_PINNED_STAGE_MAX", raising=False)
    N.reload_env()
    yield request.param
    monkeypatch.undo()
    N.reload_env()


def part_of(kind):
    if kind == "cyclic":
        return CyclicPartition(1, 3, 3 * SIZE)  # keys 1, 4, 7, ...
    return RangePartition(2, 1_000_003, 1_000_003 + SIZE)


OTHER = RangePartition(1, 77, 77 + SIZE)  # the second shard of a pair call: a partition of its own


def local_rows(n, what):
    """n local rows; from 257 on every sixteenth record names the row of record 3."""
    rng = np.random.default_rng(zlib.crc32(f"hostcalls/{what}/{n}".encode()))
    local = rng.integers(0, SIZE, n)
    if n > 16:
        local[::16] = local[3]
    return local


def shard(gpu, part, dtype, table):
    sh = PartialMatrix(part, COLS, dtype, gpu)
    write_image(sh, gpu, table, PAD)
    return sh


def rejected_first(call, arrays, parts, shards, tables):
    """For each of the key arrays in turn, the call with record 5 of that array one row past its partition:
    raised with index 5, every shard as it was. Nothing to do for a call of fewer than six records."""
    if arrays[0].size <= 5:
        return
    for j, part in enumerate(parts):
        bad = [np.array(a) for a in arrays]
        bad[j][5] = global_rows(part, SIZE)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            call(*bad)
        assert ei.value.record == 5
        for sh, table in zip(shards, tables):
            assert_bits(sh.to_numpy(), table, "after the rejected call")


@pytest.mark.parametrize("kind,n", CASES, ids=CASE_IDS)
def test_adagrad_push(gpu, staging, kind, n):
    part = part_of(kind)
    w0, h0 = start_tables("float32", SIZE, COLS)
    local = local_rows(n, "adagrad")
    g = adagrad_inputs("float32", n, COLS, "hostcalls")
    want_w, want_h = replay_adagrad(w0, h0, local, g, LR, EPS)
    with shard(gpu, part, "float", w0) as w, shard(gpu, part, "float", h0) as h:
        call = lambda rows: w.updateRowsAdagrad(h, rows, g, LR, EPS)  # noqa: E731
        rows = global_rows(part, local)
        rejected_first(call, [rows], [part], [w, h], [w0, h0])
        assert call(rows)
        assert_bits(h.to_numpy(), want_h, "state")
        assert_bits(w.to_numpy(), want_w, "weights")


@pytest.mark.parametrize("kind,n", CASES, ids=CASE_IDS)
def test_pair_dot(gpu, staging, kind, n):
    part = part_of(kind)
    A, B = pair_values("float32", SIZE, COLS, "hostcalls/a"), pair_values("float32", SIZE, COLS, "hostcalls/b")
    la, lb = local_rows(n, "dot/a"), local_rows(n, "dot/b")
    with shard(gpu, part, "float", A) as a, shard(gpu, OTHER, "float", B) as b:
        call = lambda ra, rb: a.getPairsDot(b, ra, rb)  # noqa: E731
        ra, rb = global_rows(part, la), global_rows(OTHER, lb)
        rejected_first(call, [ra, rb], [part, OTHER], [a, b], [A, B])
        assert_dot_bits(call(ra, rb), replay_pair_dot(A[la], B[lb]), "dots")
        assert_bits(a.to_numpy(), A, "a is only read")
        assert_bits(b.to_numpy(), B, "b is only read")


@pytest.mark.parametrize("dtype", ["float", "long"])
@pytest.mark.parametrize("kind,n", CASES, ids=CASE_IDS)
def test_pair_axpy(gpu, staging, kind, n, dtype):
    part = part_of(kind)
    D, S = pair_values(NPD[dtype], SIZE, COLS, "hostcalls/dst"), pair_values(NPD[dtype], SIZE, COLS, "hostcalls/src")
    ld, ls = local_rows(n, "axpy/dst"), local_rows(n, "axpy/src")
    coef = pair_coef(NPD[dtype], n, "hostcalls/coef")
    with shard(gpu, part, dtype, D) as dst, shard(gpu, OTHER, dtype, S) as src:
        call = lambda rd, rs: dst.updatePairsAxpy(src, rd, rs, coef)  # noqa: E731
        rd, rs = global_rows(part, ld), global_rows(OTHER, ls)
        rejected_first(call, [rd, rs], [part, OTHER], [dst, src], [D, S])
        assert call(rd, rs)
        assert_bits(dst.to_numpy(), replay_pair_axpy(D, ld, coef, S[ls]), "destination")
        assert_bits(src.to_numpy(), S, "the source is only read")


@pytest.mark.parametrize("dtype,value", [("float", 1.5), ("long", -7)])
@pytest.mark.parametrize("kind,n", CASES, ids=CASE_IDS)
def test_fill(gpu, staging, kind, n, dtype, value):
    part = part_of(kind)
    T = pair_values(NPD[dtype], SIZE, COLS, "hostcalls/fill")
    local = local_rows(n, "fill")
    with shard(gpu, part, dtype, T) as sh:
        call = lambda rows: sh.fill(value, rows=rows)  # noqa: E731
        rows = global_rows(part, local)
        rejected_first(call, [rows], [part], [sh], [T])
        assert call(rows)
        assert_bits(sh.to_numpy(), replay_fill(T, local, value), "filled")


@pytest.mark.parametrize("kind,n", CASES, ids=CASE_IDS)
def test_init_uniform(gpu, staging, kind, n):
    part = part_of(kind)
    T = pair_values("float32", SIZE, COLS, "hostcalls/uniform")
    local = local_rows(n, "uniform")
    with shard(gpu, part, "float", T) as sh:
        call = lambda rows: sh.initUniform(SEED, LO, HI, rows=rows)  # noqa: E731
        rows = global_rows(part, local)
        rejected_first(call, [rows], [part], [sh], [T])
        assert call(rows)
        assert_bits(sh.to_numpy(), replay_uniform(T, local, rows, SEED, LO, HI), "initialised")
