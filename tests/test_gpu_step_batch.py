"""Batched optimizer row pushes (PartialMatrix.updateRowsAdagradBatch / AdamBatch / FtrlBatch,
glint_mat_push_rows_*_batch*) on the GPU. Expected values never come from the code under test: they are the
numpy restatements of the step contracts (adagrad_cases, adam_cases, ftrl_cases) applied to a float64 G, or the
composition of calls that existed before. Both shards' pitch padding is NaN (ieee_cases.write_image) and their
whole images, padding included, are read back and compared by their bits (a NaN by its class), so a touched
padding element or a touched row that was not named shows."""
import numpy as np
import pytest

from glint_amd import _native as N
from glint_amd import ArrayIndexOutOfBoundsException, CyclicPartition, PartialMatrix, PartialVector, RangePartition
from adagrad_cases import adagrad_step
from adam_cases import BETA1, BETA2, EPS, adam_scalars, adam_step
from dot_cases import assert_dot_bits, bits
from ftrl_cases import ftrl_scalars, ftrl_step
from ieee_cases import write_image
from test_gpu_axpy_batch import dev, image, ints, np_dtype, records  # the batched axpy push's shapes and helpers
from topk_cases import global_rows

pytestmark = pytest.mark.gpu
R, QMAX, START, SIZE = 128, N.GLINT_AXPY_BATCH_MAX_VECTORS, 1_000_003, 300  # the tile is R distinct rows
DT = ["double", "float"]
OPTS = ["adagrad", "adam", "ftrl"]
COLS = [2, 67, 300]  # one column block; part 1 unaligned with a partial second pass; by 16 B, the fifth pass partial
US = [1, R - 1, R + 1, 2 * R + 3]  # distinct rows
QS = [1, 16, 17, 33, 130]
HOW = ["host", "device"]
PARTS = dict(adagrad=1, adam=2, ftrl=2)
ARGS = dict(adagrad=(0.05, 1e-6), adam=(0.01, 3), ftrl=(0.05, 1.0, 0.3, 1e-4))  # the methods' scalars: Adam step 3, l1 > 0
CARGS = dict(adagrad=ARGS["adagrad"], adam=(0.01, BETA1, BETA2, EPS, 3), ftrl=ARGS["ftrl"])  # the C calls' scalars
BAD = dict(adagrad=[(np.nan, 1e-6)], adam=[(np.nan, BETA1, BETA2, EPS, 3), (0.01, BETA1, BETA2, EPS, 0)],
           ftrl=[(0.0, 1.0, 0.3, 1e-4)])
BATCH = dict(adagrad="updateRowsAdagradBatch", adam="updateRowsAdamBatch", ftrl="updateRowsFtrlBatch")
PLAIN = dict(adagrad="updateRowsAdagrad", adam="updateRowsAdam", ftrl="updateRowsFtrl")


def start_images(rng, opt, size, cols, npd):  # general weights and state, the part under a square root >= 0
    w, s = rng.standard_normal((size, cols)).astype(npd), rng.standard_normal((size, PARTS[opt] * cols)).astype(npd)
    s[:, -cols:] = np.abs(s[:, -cols:])
    return w, s


def shards_of(gpu, dtype, w, s, part=None):  # (weights, state) with NaN padding
    part = part or RangePartition(2, START, START + w.shape[0])
    pair = [PartialMatrix(part, img.shape[1], dtype, gpu) for img in (w, s)]
    for sh, img in zip(pair, (w, s)):
        write_image(sh, gpu, np.ascontiguousarray(img), np.nan)
    return pair


def check_images(pair, gpu, exp, what):  # named rows, rows that were not named and the padding, bit for bit
    for sh, e, name in zip(pair, exp, ("weights", "state")):
        raw = image(sh, gpu, e.shape[0])
        want = np.full(raw.shape, np.nan, raw.dtype)
        want[:, :e.shape[1]] = e
        assert_dot_bits(raw, want, f"{what}: {name}")


def push(pair, gpu, opt, how, rows, coef, x, **kw):
    if how == "device":
        rows, coef, x = dev(gpu, rows), dev(gpu, coef), dev(gpu, x)
    assert getattr(pair[0], BATCH[opt])(pair[1], rows, coef, x, *ARGS[opt], **kw)
    return rows


def product(local, coef, x, size):  # G of every row in float64, every product formed: 0 * inf is NaN
    Cs = np.zeros((size, coef.shape[1]))
    with np.errstate(invalid="ignore"):
        np.add.at(Cs, local, coef.astype(np.float64))
        if np.isfinite(Cs).all() and np.isfinite(x).all():
            return Cs @ x.astype(np.float64)
        return (Cs[:, :, None] * x.astype(np.float64)[None]).sum(1)


def stepped(opt, w, s, G, named):  # the numpy contract step of rows `named` with G rounded to the shards' type
    w2, s2, cols, dt = w.copy(), s.copy(), w.shape[1], w.dtype
    parts = [s[named, p * cols:(p + 1) * cols] for p in range(PARTS[opt])]
    g = G[named].astype(dt)
    if opt == "adagrad":
        out = adagrad_step(w[named], parts[0], g, *ARGS[opt])
    elif opt == "adam":
        out = adam_step(w[named], *parts, g, adam_scalars(dt, ARGS[opt][0], BETA1, BETA2, EPS, ARGS[opt][1]))
    else:
        out = ftrl_step(w[named], *parts, g, ftrl_scalars(dt, *ARGS[opt]))
    w2[named], s2[named] = out[0], np.concatenate(out[1:], 1)
    return w2, s2


CASES = [(opt, dt, COLS[(i + j + k) % 3], u) for i, opt in enumerate(OPTS) for j, dt in enumerate(DT) for k, u in enumerate(US)]


@pytest.mark.parametrize("opt,dtype,cols,u", CASES)
def test_bit_exact_step_on_an_exact_product(gpu, opt, dtype, cols, u):
    """coef and x are integers in [-8, 8]: every partial sum of G is an integer below 2^24, any order is exact,
    and the step's bits are the numpy contract's. The pushes step one pair of shards again and again. Column 0 of
    x is zero, so G is 0 there: FTRL with |z| <= l1 in that column must store exact zeros."""
    npd, rng = np_dtype(dtype), np.random.default_rng(u * 1000 + cols)
    w, s = start_images(rng, opt, SIZE, cols, npd)
    local = records(rng, u, SIZE)
    named = np.unique(local)
    coef, x = ints(rng, (local.size, QS[-1]), npd), ints(rng, (QS[-1], cols), npd)
    x[:, 0] = 0
    if opt == "ftrl":
        s[:, 0] = rng.uniform(-0.25, 0.25, SIZE)  # z of column 0, where G is 0: z' = z
    pair = shards_of(gpu, dtype, w, s)
    for q in QS:
        for how in HOW:
            push(pair, gpu, opt, how, local + START, np.ascontiguousarray(coef[:, :q]), x[:q])
            G = product(local, coef[:, :q], x[:q], SIZE)
            assert np.abs(G).max() < 2 ** 24
            w, s = stepped(opt, w, s, G, named)
            check_images(pair, gpu, (w, s), f"{how} q={q}")
    push(pair, gpu, opt, "host", local + START, coef[:, 3].copy(), x[3])  # x of shape (cols,), coef (n,): q = 1
    w, s = stepped(opt, w, s, product(local, coef[:, 3:4], x[3:4], SIZE), named)
    check_images(pair, gpu, (w, s), "1-d")
    if opt == "ftrl":
        assert not bits(w[named, 0]).any() and w[named].any()  # exact +0 where |z'| <= l1, and only there
    for sh in pair:
        sh.destroy()


@pytest.mark.parametrize("opt,dtype,cols,variant", [(opt, dt, COLS[(i + j) % 3], ("host", "cyclic", "shift")[(i + 2 * j) % 3])
                                                    for i, opt in enumerate(OPTS) for j, dt in enumerate(DT)])
def test_composition_identity_on_general_data(gpu, opt, dtype, cols, variant):
    """The new call against what existed before it: updateRowsAxpyBatch into a zeroed shard, those rows read
    back, then the unbatched push of the distinct rows with them. Bit-identical shards; on a CyclicPartition
    (`cyclic`) and with device coef and x one element past a 16-B boundary (`shift`) too."""
    import torch
    npd, rng, q, size = np_dtype(dtype), np.random.default_rng(cols + len(opt)), 65, SIZE
    cyclic = (1, 3) if variant == "cyclic" else None
    part = CyclicPartition(1, 3, 3 * size) if cyclic else None
    glob = global_rows(size, START, cyclic)
    local = records(rng, R + 1, size)
    w, s = start_images(rng, opt, size, cols, npd)
    coef, x = rng.standard_normal((local.size, q)).astype(npd), rng.standard_normal((q, cols)).astype(npd)
    named = np.unique(local)
    old = shards_of(gpu, dtype, w, s, part)
    with PartialMatrix(part or RangePartition(2, START, START + size), cols, dtype, gpu) as scratch:
        scratch.updateRowsAxpyBatch(glob[local], coef, x)
        G = scratch.getRows(glob[named])
    assert G.any() and getattr(old[0], PLAIN[opt])(old[1], glob[named], G, *ARGS[opt])
    exp = [image(sh, gpu, size) for sh in old]
    new = shards_of(gpu, dtype, w, s, part)
    if variant == "shift":
        bufs = [torch.zeros(a.size + 4, dtype=new[0].torch_dtype, device=torch.device("cuda", gpu)) for a in (coef, x)]
        views = [b[1:1 + a.size].copy_(dev(gpu, a).reshape(-1)).view(a.shape) for b, a in zip(bufs, (coef, x))]
        assert all(v.data_ptr() % 16 == v.element_size() for v in views)
        assert getattr(new[0], BATCH[opt])(new[1], dev(gpu, glob[local]), *views, *ARGS[opt])
    else:
        push(new, gpu, opt, "host", glob[local], coef, x)
    for sh, e, name in zip(new, exp, ("weights", "state")):
        assert_dot_bits(image(sh, gpu, size), e, f"{variant}: {name}")
    for sh in old + new:
        sh.destroy()


@pytest.mark.parametrize("opt,dtype,cols", [("adam", "float", 300), ("ftrl", "double", 67)])
def test_bits_do_not_depend_on_the_batch(gpu, opt, dtype, cols):
    """One row's three records, alone and as the first, the R-th and the last distinct row of a 259-row push with
    the other rows' records between its own: the same weights and state bits each time."""
    npd, rng, q, size = np_dtype(dtype), np.random.default_rng(cols), 68, 2 * R + 20
    x, mine = rng.standard_normal((q, cols)).astype(npd), rng.standard_normal((3, q)).astype(npd)
    named = np.arange(5, 5 + 2 * R + 3)
    w, s = start_images(rng, opt, size, cols, npd)
    w[named], s[named] = w[7], s[7]  # every target starts from the one row's old weights and state

    def row_after(how, local, coef, target):
        pair = shards_of(gpu, dtype, w, s)
        push(pair, gpu, opt, how, local + START, coef, x)
        out = [bits(image(sh, gpu, size)[target, :sh.cols]) for sh in pair]
        for sh in pair:
            sh.destroy()
        return np.concatenate(out)

    alone = row_after("host", np.full(3, 7), mine, 7)
    assert (alone != np.concatenate([bits(w[7]), bits(s[7])])).any()
    for target, how in zip((named[0], named[R - 1], named[-1]), ("host", "device", "host")):
        others = rng.permutation(np.repeat(named[named != target], 2))
        at = np.sort(rng.choice(others.size + 3, 3, replace=False))  # its records keep their order
        local, coef = np.empty(others.size + 3, np.int64), rng.standard_normal((others.size + 3, q)).astype(npd)
        local[at], coef[at] = target, mine
        local[np.setdiff1d(np.arange(local.size), at)] = others
        np.testing.assert_array_equal(row_after(how, local, coef, target), alone, err_msg=f"{target} {how}")


@pytest.mark.parametrize("opt,dtype", [(opt, dt) for opt in OPTS for dt in DT])
def test_non_finite_values_and_rows_outside_the_partition(gpu, opt, dtype):
    npd, rng, cols, q = np_dtype(dtype), np.random.default_rng(4), 67, 33
    local = records(rng, R + 9, SIZE)
    named = np.unique(local)
    w, s = start_images(rng, opt, SIZE, cols, npd)
    coef, x = ints(rng, (local.size, q), npd), ints(rng, (q, cols), npd)
    x[x == 0], coef[:, 7] = 1, 0
    coef[np.flatnonzero(local == local[0])[0], 2] = np.inf  # one row's coefficient: that row only
    x[7, 11] = np.inf  # against zero coefficients: NaN in column 11 of G of every named row
    G = product(local, coef, x, SIZE)
    assert np.isinf(np.delete(G[local[0]], 11)).all() and np.isnan(G[named, 11]).all() and np.isnan(G[named]).sum() == named.size
    for how in HOW:
        pair = shards_of(gpu, dtype, w, s)
        push(pair, gpu, opt, how, local + START, coef, x)
        check_images(pair, gpu, stepped(opt, w, s, G, named), how)
        for sh in pair:
            sh.destroy()
    bad = local + START
    bad[[40, R + 3]] = START - 1, START + SIZE
    pair = shards_of(gpu, dtype, w, s)
    with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
        push(pair, gpu, opt, "host", bad, coef, x)
    assert ei.value.record == 40  # the lowest such record
    check_images(pair, gpu, (w, s), "rejected: neither shard changes")
    rows = push(pair, gpu, opt, "device", bad, coef, x, sync=False)
    with pytest.raises(ArrayIndexOutOfBoundsException) as ei:
        pair[0].sync(pair[0]._stream_of(rows))
    assert ei.value.record == 40
    keep = np.setdiff1d(np.arange(local.size), [40, R + 3])
    check_images(pair, gpu, stepped(opt, w, s, product(local[keep], coef[keep], x, SIZE), np.unique(local[keep])), "skipped")
    for sh in pair:
        sh.destroy()


@pytest.mark.parametrize("opt", OPTS)
def test_argument_errors(gpu, opt):
    lib, x, rows, coef = N.load(), np.ones((2, 4)), np.full(3, START, np.int64), np.ones((3, 2))
    fn = f"glint_mat_push_rows_{opt}_batch"
    host = lambda w, s, r, n, c, xp, q, f, k=CARGS[opt]: getattr(lib, fn)(w, s, r, n, c, xp, q, *k, f)  # noqa: E731
    devc = lambda w, s, r, n, c, xp, q, f, k=CARGS[opt]: getattr(lib, fn + "_dev")(w, s, r, n, c, xp, q, *k, f, None)  # noqa: E731
    calls = ((host, [a.ctypes.data for a in (rows, coef, x)]),
             (devc, [a.data_ptr() for a in (dev(gpu, rows), dev(gpu, coef), dev(gpu, x))]))
    part, P = RangePartition(0, START, START + 10), PARTS[opt]
    method = lambda w, s, c=coef, xs=x: getattr(w, BATCH[opt])(s, rows, c, xs, *ARGS[opt])  # noqa: E731
    for dtype in ("int", "long"):
        with PartialMatrix(part, 4, dtype, gpu) as sh, PartialMatrix(part, 4 * P, dtype, gpu) as st:
            for call, (rp, cp, xp) in calls:
                assert call(sh.handle, st.handle, rp, 3, cp, xp, 2, 0) == N.GLINT_EINVAL
            with pytest.raises(TypeError):
                method(sh, st, np.ones((3, 2), sh.np_dtype), np.ones((2, 4), sh.np_dtype))
    with PartialVector(part, "double", gpu) as vec, PartialMatrix(part, 4 * P, "double", gpu) as st:
        for call, (rp, cp, xp) in calls:
            assert call(vec.handle, st.handle, rp, 3, cp, xp, 1, 0) == N.GLINT_EINVAL
    with PartialMatrix(part, 4, "double", gpu) as sh, PartialMatrix(part, 4 * P, "double", gpu) as st, \
            PartialMatrix(part, 4 * (3 - P), "double", gpu) as wrong, PartialMatrix(part, 4 * P, "float", gpu) as other:
        for call, (rp, cp, xp) in calls:
            for state in (sh, wrong, other):  # the same shard, Adagrad 2 * cols / Adam and FTRL cols, another type
                assert call(sh.handle, state.handle, rp, 3, cp, xp, 2, 0) == N.GLINT_EINVAL
            for n, q, flag in ((3, 0, 0), (3, QMAX + 1, 0), (-1, 2, 0), (3, 2, N.GLINT_PUSH_DETERMINISTIC), (3, 2, 64)):
                assert call(sh.handle, st.handle, rp, n, cp, xp, q, flag) == N.GLINT_EINVAL
            assert call(sh.handle, st.handle, rp, 3, None, xp, 2, 0) == N.GLINT_EINVAL
            assert call(sh.handle, st.handle, rp, 3, cp, None, 2, 0) == N.GLINT_EINVAL
            for k in BAD[opt]:  # NaN lr, Adam step 0, FTRL alpha 0
                assert call(sh.handle, st.handle, rp, 3, cp, xp, 2, 0, k) == N.GLINT_EINVAL
            assert call(sh.handle, st.handle, None, 0, None, None, 2, 0) == N.GLINT_OK  # n == 0 launches nothing
        for state in (sh, wrong, other):
            with pytest.raises(ValueError):
                method(sh, state)
        with pytest.raises(ValueError):
            method(sh, st, np.ones((3, 3)))
        with pytest.raises(ValueError):
            method(sh, st, np.ones((3, QMAX + 1)), np.ones((QMAX + 1, 4)))
        sh.sync(None)
        assert not sh.to_numpy().any() and not st.to_numpy().any()  # nothing above was applied
        for call, (rp, cp, xp) in calls:
            assert call(sh.handle, st.handle, rp, 3, cp, xp, 2, 0) == N.GLINT_OK
        sh.sync(None)
        assert sh.to_numpy()[0].all() and st.to_numpy()[0].all() and not sh.to_numpy()[1:].any() and not st.to_numpy()[1:].any()
