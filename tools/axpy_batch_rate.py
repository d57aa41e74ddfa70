"""Batched row axpy push against the row axpy push it stands beside (DESIGN.md "Batched row axpy push", Measured).

    python tools/axpy_batch_rate.py [--out FILE] [--rows N]

cfg5's per-GPU shard, 2^17 x 512, Float and Double; row lists: 2^12 and 2^15 distinct rows and 2^15 records
drawn from a Zipf law (repeats); q in {1, 8, 64, 256, 1024}. coef and x hold -1, 0 and 1, so every leg's sums
are exact integers: each leg pushes once onto a zeroed shard and the tool compares the shard with a float64
torch reference (`same_answer`). Baselines: for q <= 64 glint_mat_push_rows_axpy_dev on the same operands, with
the device default flags (`base`) and with GLINT_PUSH_DETERMINISTIC (`base_det`); above that the only thing a
caller can do without the new call, ceil(q / 64) such calls (default flags) over column blocks of coef copied
contiguous, the copies timed on their own (`copy_ms`). After a warm-up round the legs alternate inside each of
5 rounds, one HIP event pair around a leg. Then the two launches the batched call counts
(glint_prof_read_launches: the coefficient run-sum, the product), the product as a share of its bound: the
larger of 2 * u * qp * cols flops at the published matrix peak and (u * qp + q * cols + 2 * u * cols) values at
the published HBM peak, u the distinct rows and qp = q rounded up to 128 B (AMD Instinct MI355X data sheet:
157.3 TFLOP/s FP32 matrix, 78.6 TFLOP/s FP64 matrix, 8 TB/s). One JSON line per (type, list, q), appended to
FILE (profiles/axpybatch/axpy_batch.jsonl)."""
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import glint_amd  # noqa: E402
from glint_amd import _native as N  # noqa: E402

dev = torch.device("cuda", 0)
lib = N.load()
stream = torch.cuda.current_stream(dev).cuda_stream
PEAK_FLOPS = {"float": 157.3e12, "double": 78.6e12}
PEAK_HBM = 8.0e12
CAP = N.GLINT_AXPY_MAX_VECTORS


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches_ms(h, fn):
    """Device ms of the launches fn counts under GLINT_K_PUSH_ROWS_AXPY, in launch order."""
    lib.glint_prof_reset(h)
    lib.glint_prof_enable(h, 1)
    fn()
    torch.cuda.synchronize()
    cnt = C.c_int64()
    lib.glint_prof_read_launches(h, N.GLINT_K_PUSH_ROWS_AXPY, None, 0, C.byref(cnt))
    ms = (C.c_double * cnt.value)()
    lib.glint_prof_read_launches(h, N.GLINT_K_PUSH_ROWS_AXPY, ms, cnt.value, C.byref(cnt))
    lib.glint_prof_enable(h, 0)
    return [float(v) for v in ms]


def stats(ms):
    return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def row_lists(rows):
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    perm = torch.randperm(rows, device=dev, generator=gen)
    zipf = np.random.default_rng(3).zipf(1.2, 1 << 15) % rows
    return [("distinct_2p12", perm[:1 << 12].contiguous()), ("distinct_2p15", perm[:1 << 15].contiguous()),
            ("zipf_2p15", torch.from_numpy(zipf.astype(np.int64)).to(dev))]


def rate(dtype, rows, cols, out):
    sh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, rows), cols, dtype, 0)
    h, tdt, vs = sh.handle, sh.torch_dtype, np.dtype(sh.np_dtype).itemsize
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    ks = 128 // vs
    for name, d_rows in row_lists(rows):
        n, u = d_rows.numel(), int(torch.unique(d_rows).numel())
        for q in (1, 8, 64, 256, 1024):
            d_x = torch.randint(-1, 2, (q, cols), device=dev, generator=gen).to(tdt)
            d_c = torch.randint(-1, 2, (n, q), device=dev, generator=gen).to(tdt)
            blocks = [(d_c[:, j:j + CAP].contiguous(), d_x[j:j + CAP]) for j in range(0, q, CAP)]

            def axpy(flags):
                for cb, xb in blocks:
                    assert lib.glint_mat_push_rows_axpy_dev(h, d_rows.data_ptr(), n, cb.data_ptr(), xb.data_ptr(),
                                                            xb.shape[0], flags, stream) == 0

            legs = {"batch": lambda: lib.glint_mat_push_rows_axpy_batch_dev(
                        h, d_rows.data_ptr(), n, d_c.data_ptr(), d_x.data_ptr(), q, 0, stream),
                    "base": lambda: axpy(0)}
            if q <= CAP:
                legs["base_det"] = lambda: axpy(N.GLINT_PUSH_DETERMINISTIC)
            else:
                legs["copy"] = lambda: [d_c[:, j:j + CAP].contiguous() for j in range(0, q, CAP)]
            ref = torch.zeros((rows, cols), dtype=torch.float64, device=dev)
            ref.index_add_(0, d_rows, d_c.double() @ d_x.double())
            same = bool(ref.abs().max() < 2 ** 24)
            for leg in ("batch", "base"):  # one push each onto zeros: exact integers
                assert lib.glint_shard_zero(h) == 0
                legs[leg]()
                sh.sync(stream)
                same = same and bool(torch.equal(torch.from_numpy(sh.to_numpy()).to(dev).double(), ref))
            del ref
            t = {leg: [] for leg in legs}
            for rnd in range(6):  # round 0 warms up; the legs alternate inside every round
                for leg, fn in legs.items():
                    ms = ev_ms(fn)
                    if rnd:
                        t[leg].append(ms)
            sh.sync(stream)
            k_sum, k_prod = launches_ms(h, legs["batch"])
            k_base = sum(launches_ms(h, legs["base"]))
            qp = (q + ks - 1) // ks * ks
            flops, nbytes = 2.0 * u * qp * cols, (u * qp + q * cols + 2 * u * cols) * vs
            bound = max(flops / PEAK_FLOPS[dtype], nbytes / PEAK_HBM) * 1e3
            spread = max(t["base"]) - min(t["base"])
            line = dict(op="mat_push_rows_axpy_batch", dtype=dtype, shape=[rows, cols], rows=name, n=n, distinct=u,
                        vectors=q, rounds=5, **{leg + "_ms": stats(v) for leg, v in t.items()},
                        speedup=float(np.mean(t["base"]) / np.mean(t["batch"])),
                        faster_by_more_than_baseline_spread=bool(np.mean(t["base"]) - np.mean(t["batch"]) > spread),
                        coef_sum_kernel_ms=k_sum, product_kernel_ms=k_prod, baseline_fold_kernels_ms=k_base,
                        product_bound_ms=bound, product_bound_is="flops" if flops / PEAK_FLOPS[dtype] * 1e3 == bound else "bytes",
                        product_share_of_bound=bound / k_prod, product_TFLOPs=flops / (k_prod * 1e-3) / 1e12,
                        product_GBs=nbytes / (k_prod * 1e-3) / 1e9, same_answer=same)
            print(json.dumps(line), flush=True)
            with open(out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del blocks, d_c, d_x
    sh.destroy()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        str(Path(__file__).resolve().parent.parent / "profiles" / "axpybatch" / "axpy_batch.jsonl")
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1 << 17
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    for dtype in ("float", "double"):
        rate(dtype, rows, 512, out)


if __name__ == "__main__":
    main()
