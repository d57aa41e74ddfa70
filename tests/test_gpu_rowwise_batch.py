"""Batched row-wise Adagrad row push (PartialMatrix.updateRowsAdagradRowwiseBatch) on the GPU, against
rowwise_cases.rowwise_terms of an exact G and ss, or of updateRowsAxpyBatch's G and this file's ss; by bits."""
import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from dot_cases import assert_dot_bits, bits
from ieee_cases import write_image
from rowwise_cases import EPS, LR, rowwise_terms
from test_gpu_axpy_batch import dev, image, np_dtype, records  # the batched axpy push's shapes and helpers
from test_gpu_step_batch import check_images, product
from topk_cases import global_rows

pytestmark = pytest.mark.gpu
R, QMAX, START, SIZE = 128, N.GLINT_AXPY_BATCH_MAX_VECTORS, 1_000_003, 300  # the tile is R distinct rows
DT, COLS, US, QS, HOW = ["double", "float"], [2, 67, 300], [1, R - 1, R + 1, 2 * R + 3], [1, 17, 33, 130], ["host", "device"]
signs = lambda rng, shape, npd: rng.integers(-1, 2, shape).astype(npd)  # noqa: E731
normal = lambda rng, shape, npd: rng.standard_normal(shape).astype(npd)  # noqa: E731
check = lambda pair, gpu, w, h, what: (check_images(pair[:1], gpu, (w,), what),  # noqa: E731
                                       assert_dot_bits(pair[1].to_numpy(), h, f"{what}: state"))
start_images = lambda rng, size, cols, npd: (normal(rng, (size, cols), npd), np.abs(normal(rng, size, npd)))  # noqa: E731


def shards_of(gpu, dtype, w, h, part=None, glob=None):  # (weights with NaN padding, state): 0 + h is h
    part = part or RangePartition(2, START, START + w.shape[0])
    pair = PartialMatrix(part, w.shape[1], dtype, gpu), PartialVector(part, dtype, gpu)
    write_image(pair[0], gpu, np.ascontiguousarray(w), np.nan)
    pair[1].update(global_rows(len(h), START) if glob is None else glob, h)
    return pair


def push(pair, gpu, how, rows, coef, x, **kw):
    if how == "device":
        rows, coef, x = dev(gpu, rows), dev(gpu, coef), dev(gpu, x)
    assert pair[0].updateRowsAdagradRowwiseBatch(pair[1], rows, coef, x, LR, EPS, **kw)
    return rows


def stepped(w, h, G, named, ss=None):  # rows `named` stepped with G (size, cols) and their ss (len(named),)
    if ss is None:  # the premise: every row's sum of squares is exact in any order
        ss = (G[named] * G[named]).sum(1)
        assert ss.max() < 2 ** (24 if w.dtype == np.float32 else 53)
    w2, h2 = w.copy(), h.copy()
    t = rowwise_terms(w[named], h[named], G[named].astype(w.dtype), LR, EPS, ss=np.asarray(ss, w.dtype))
    w2[named], h2[named] = t["w2"], t["h2"]
    return w2, h2


def contract_ss(G):  # step 3 of include/glint_gpu.h, every operation one numpy call in G's type
    dt, (m, cols), lanes = G.dtype, G.shape, 128 // G.dtype.itemsize
    t, ss = np.arange(lanes), np.zeros(m, dt)
    for p in range(-(-cols // 64)):
        a = np.zeros((m, lanes), dt)
        for b in range(64 // lanes):
            ok = (c := 64 * p + lanes * b + t) < cols
            a[:, ok] = np.add(a[:, ok], np.multiply(G[:, c[ok]], G[:, c[ok]], dtype=dt), dtype=dt)
        for d in (16, 8, 4, 2, 1)[-lanes.bit_length() + 1:]:  # lanes / 2 .. 1
            a = np.add(a, a[:, t ^ d], dtype=dt)
        ss = np.add(ss, a[:, 0], dtype=dt)
    return ss


@pytest.mark.parametrize("dtype,cols,u", [(dt, COLS[(j + k) % 3], u) for j, dt in enumerate(DT) for k, u in enumerate(US)])
def test_bit_exact_step_on_an_exact_product(gpu, dtype, cols, u):
    npd, rng = np_dtype(dtype), np.random.default_rng(u * 1000 + cols)
    (w, h), local = start_images(rng, SIZE, cols, npd), records(rng, u, SIZE)
    coef, x = signs(rng, (local.size, QS[-1]), npd), signs(rng, (QS[-1], cols), npd)
    pair, named = shards_of(gpu, dtype, w, h), np.unique(local)
    with pair[0], pair[1]:
        for q in QS:
            for how in HOW:  # q == 1: coef (n,), x (cols,)
                c, xs = (coef[:, 0].copy(), x[0]) if q == 1 else (np.ascontiguousarray(coef[:, :q]), x[:q])
                push(pair, gpu, how, local + START, c, xs)
                w, h = stepped(w, h, product(local, coef[:, :q], x[:q], SIZE), named)
                check(pair, gpu, w, h, f"{how} q={q}")


@pytest.mark.parametrize("dtype,cols,variant", zip(DT * 2, [67, 300, 300, 67], ["cyclic", "shift", "host", "host"]))
def test_general_data_in_the_contracts_order(gpu, dtype, cols, variant):
    """G: updateRowsAxpyBatch's bits. `shift`: device coef and x one element past a 16-B boundary."""
    import torch
    npd, rng, q, size = np_dtype(dtype), np.random.default_rng(cols + len(variant)), 65, SIZE
    cyclic = (1, 3) if variant == "cyclic" else None
    part = CyclicPartition(1, 3, 3 * size) if cyclic else RangePartition(2, START, START + size)
    glob, local = global_rows(size, START, cyclic), records(rng, R + 1, size)
    (w, h), coef, x = start_images(rng, size, cols, npd), normal(rng, (local.size, q), npd), normal(rng, (q, cols), npd)
    named, G = np.unique(local), np.zeros((size, cols), npd)
    with PartialMatrix(part, cols, dtype, gpu) as scratch:
        scratch.updateRowsAxpyBatch(glob[local], coef, x)
        G[named] = scratch.getRows(glob[named])
    pair = shards_of(gpu, dtype, w, h, part, glob)
    with pair[0], pair[1]:
        if variant == "shift":
            bufs = [torch.zeros(a.size + 4, dtype=pair[0].torch_dtype, device=torch.device("cuda", gpu)) for a in (coef, x)]
            views = [b[1:1 + a.size].copy_(dev(gpu, a).reshape(-1)).view(a.shape) for b, a in zip(bufs, (coef, x))]
            assert all(v.data_ptr() % 16 == v.element_size() for v in views)
            assert pair[0].updateRowsAdagradRowwiseBatch(pair[1], dev(gpu, glob[local]), *views, LR, EPS)
        else:
            push(pair, gpu, "host", glob[local], coef, x)
        check(pair, gpu, *stepped(w, h, G, named, contract_ss(G[named])), variant)


@pytest.mark.parametrize("dtype,cols", [("float", 300), ("double", 67)])
def test_bits_do_not_depend_on_the_batch(gpu, dtype, cols):  # alone; the first, R-th and last of 259 distinct rows
    npd, rng, q, size = np_dtype(dtype), np.random.default_rng(cols), 68, 2 * R + 20
    x, mine, named = normal(rng, (q, cols), npd), normal(rng, (3, q), npd), np.arange(5, 5 + 2 * R + 3)
    w, h = start_images(rng, size, cols, npd)
    w[named], h[named] = w[7], h[7]  # every target starts from the one row's old weights and accumulator

    def row_after(how, local, coef, target):
        pair = shards_of(gpu, dtype, w, h)
        with pair[0], pair[1]:
            push(pair, gpu, how, local + START, coef, x)
            return np.concatenate([bits(image(pair[0], gpu, size)[target, :cols]), bits(pair[1].to_numpy()[[target]])])

    alone = row_after("host", np.full(3, 7), mine, 7)
    assert (alone != np.concatenate([bits(w[7]), bits(h[[7]])])).any()
    for target, how in zip((named[0], named[R - 1], named[-1]), ("host", "device", "host")):
        others = rng.permutation(np.repeat(named[named != target], 2))
        at = np.sort(rng.choice(others.size + 3, 3, replace=False))  # its records keep their order
        local, coef = np.empty(others.size + 3, np.int64), normal(rng, (others.size + 3, q), npd)
        local[at], coef[at] = target, mine
        local[np.setdiff1d(np.arange(local.size), at)] = others
        np.testing.assert_array_equal(row_after(how, local, coef, target), alone, err_msg=f"{target} {how}")


@pytest.mark.parametrize("dtype,how", list(zip(DT, HOW)) + list(zip(DT, HOW[::-1])))
def test_padded_columns_and_non_finite_values(gpu, dtype, how):
    """cols = 67: in the 61 slots past the row's end the zero-filled x leaves inf * 0 = NaN; h' is +inf all the same."""
    npd, rng, cols, q = np_dtype(dtype), np.random.default_rng(4), 67, 33
    local = records(rng, R + 9, SIZE)
    (r_inf, r_nan), (w, h) = np.setdiff1d(np.arange(SIZE), local)[[0, -1]], start_images(rng, SIZE, cols, npd)
    coef, x = signs(rng, (local.size + 2, q), npd), signs(rng, (q, cols), npd)
    x[x == 0], coef[-2:], coef[-2, 2], coef[-1, 5] = 1, 0, np.inf, np.nan  # assigned left to right
    pair = shards_of(gpu, dtype, w, h)
    with pair[0], pair[1]:  # a run without the two records: what every other row must keep
        push(pair, gpu, how, local + START, coef[:-2], x)
        w2, h2 = image(pair[0], gpu, SIZE)[:, :cols], pair[1].to_numpy()
    w2[[r_inf, r_nan]], h2[r_inf], h2[r_nan] = np.nan, np.inf, np.nan
    pair = shards_of(gpu, dtype, w, h)
    with pair[0], pair[1]:
        push(pair, gpu, how, np.concatenate([local, [r_inf, r_nan]]) + START, coef, x)
        assert pair[1].to_numpy()[r_inf] == np.inf  # not NaN: the slots past cols are masked by a select
        check(pair, gpu, w2, h2, how)


def test_errors(gpu):
    rng, cols, q = np.random.default_rng(5), 67, 17
    local, (w, h) = records(rng, R + 9, SIZE), start_images(rng, SIZE, cols, np.float64)
    coef, x = signs(rng, (local.size, q), np.float64), signs(rng, (q, cols), np.float64)
    bad, keep = local + START, np.setdiff1d(np.arange(local.size), [40, R + 3])
    bad[[40, R + 3]] = START - 1, START + SIZE
    lib, part, pair = N.load(), RangePartition(2, START, START + SIZE), shards_of(gpu, "double", w, h)
    host = lambda wh, sh, n=3, qq=q, lr=LR: lib.glint_mat_push_rows_adagrad_rowwise_batch(  # noqa: E731
        wh.handle, sh.handle, bad.ctypes.data, n, coef.ctypes.data, x.ctypes.data, qq, lr, EPS, 0)
    with pair[0], pair[1], PartialMatrix(part, cols, "double", gpu) as mat, PartialMatrix(part, cols, "int", gpu) as ints, \
            PartialVector(part, "int", gpu) as intv:
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            push(pair, gpu, "host", bad, coef, x)
        assert ei.value.record == 40  # the lowest such record
        assert host(pair[0], mat) == host(ints, intv) == N.GLINT_EINVAL  # a matrix state, an Int shard
        assert host(*pair, qq=0) == host(*pair, qq=QMAX + 1) == host(*pair, lr=np.nan) == N.GLINT_EINVAL
        assert host(*pair, n=0) == N.GLINT_OK and pair[0].updateRowsAdagradRowwiseBatch(pair[1], bad[:0], coef[:0], x, LR) is True
        check(pair, gpu, w, h, "neither shard changed: the rejected message, the refused calls, n == 0")
        rows = push(pair, gpu, "device", bad, coef, x, sync=False)
        with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
            pair[0].sync(pair[0]._stream_of(rows))
        assert ei.value.record == 40
        check(pair, gpu, *stepped(w, h, product(local[keep], coef[keep], x, SIZE), np.unique(local[keep])), "skipped")
