"""Batched row dot pull against the row dot pull it stands beside (DESIGN.md "Batched row dot pull", Measured).

    python tools/dot_batch_rate.py [--out FILE] [--rows N]

cfg5's per-GPU shard, 2^17 x 512, Float and Double; requests drawn at random with repeats, n in
{2^12, 2^15, 2^17}; q in {1, 8, 64, 256, 1024}. The shard and the vectors hold integers in [-8, 8], so both
calls compute exact scores and must answer the same n x q values: the tool asserts it. Baseline:
glint_mat_pull_rows_dot_dev on the same shard, rows and vectors. After a warm-up round the two legs alternate
inside each of 5 rounds, one HIP event pair around a leg. Then the one launch of each call
(glint_prof_read_launches), the batched one as a share of its bound: the larger of 2 * n * q * cols flops at
the published matrix peak and the bytes read and written at the published HBM peak (AMD Instinct MI355X data
sheet: 157.3 TFLOP/s FP32 matrix, 78.6 TFLOP/s FP64 matrix, 8 TB/s). One JSON line per (type, n, q), appended
to FILE (profiles/dotbatch/dot_batch.jsonl)."""
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


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launch_ms(h, fn):
    """Device ms of the one launch of fn."""
    lib.glint_prof_reset(h)
    lib.glint_prof_enable(h, 1)
    fn()
    torch.cuda.synchronize()
    cnt = C.c_int64()
    lib.glint_prof_read_launches(h, N.GLINT_K_PULL_ROWS_DOT, None, 0, C.byref(cnt))
    ms = (C.c_double * cnt.value)()
    lib.glint_prof_read_launches(h, N.GLINT_K_PULL_ROWS_DOT, ms, cnt.value, C.byref(cnt))
    lib.glint_prof_enable(h, 0)
    assert cnt.value == 1
    return float(ms[0])


def stats(ms):
    return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def rate(dtype, rows, cols, out):
    sh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, rows), cols, dtype, 0)
    h, tdt, vs = sh.handle, sh.torch_dtype, np.dtype(sh.np_dtype).itemsize
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    d_all = torch.arange(rows, dtype=torch.int64, device=dev)
    step = min(rows, 1 << 14)
    for r0 in range(0, rows, step):  # fill in slices of whole rows
        vv = torch.randint(-8, 9, (min(step, rows - r0), cols), device=dev, generator=gen).to(tdt)
        sh.updateRows(d_all[r0:r0 + step].contiguous(), vv)
    for n in (1 << 12, 1 << 15, 1 << 17):
        d_rows = torch.randint(0, rows, (n,), device=dev, generator=gen)  # with repeats
        for q in (1, 8, 64, 256, 1024):
            d_x = torch.randint(-8, 9, (q, cols), device=dev, generator=gen).to(tdt)
            ans = {name: torch.empty((n, q), dtype=tdt, device=dev) for name in ("base", "batch")}

            def base():
                assert lib.glint_mat_pull_rows_dot_dev(h, d_rows.data_ptr(), n, d_x.data_ptr(), q,
                                                       ans["base"].data_ptr(), stream) == 0

            def batch():
                assert lib.glint_mat_pull_rows_dot_batch_dev(h, d_rows.data_ptr(), n, d_x.data_ptr(), q,
                                                             ans["batch"].data_ptr(), stream) == 0

            t = {"base": [], "batch": []}
            for rnd in range(6):  # round 0 warms up; the legs alternate inside every round
                got = {"base": ev_ms(base), "batch": ev_ms(batch)}
                if rnd:
                    for name, v in got.items():
                        t[name].append(v)
            sh.sync(stream)
            assert torch.equal(ans["base"], ans["batch"])  # exact scores
            k_batch, k_base = launch_ms(h, batch), launch_ms(h, base)
            t_flops = 2.0 * n * q * cols / PEAK_FLOPS[dtype]
            t_bytes = (n * cols + q * cols + n * q) * vs / PEAK_HBM
            spread = max(t["base"]) - min(t["base"])
            line = dict(op="mat_pull_rows_dot_batch", dtype=dtype, shape=[rows, cols], n=n, queries=q, rounds=5,
                        batch_ms=stats(t["batch"]), baseline_ms=stats(t["base"]),
                        speedup=float(np.mean(t["base"]) / np.mean(t["batch"])),
                        faster_by_more_than_baseline_spread=bool(np.mean(t["base"]) - np.mean(t["batch"]) > spread),
                        batch_kernel_ms=k_batch, baseline_kernel_ms=k_base,
                        bound_ms=max(t_flops, t_bytes) * 1e3, bound_is="flops" if t_flops > t_bytes else "bytes",
                        share_of_bound=max(t_flops, t_bytes) * 1e3 / k_batch,
                        TFLOPs=2.0 * n * q * cols / (k_batch * 1e-3) / 1e12, same_answer=True)
            print(json.dumps(line), flush=True)
            with open(out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del ans
    sh.destroy()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        str(Path(__file__).resolve().parent.parent / "profiles" / "dotbatch" / "dot_batch.jsonl")
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1 << 17
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    for dtype in ("float", "double"):
        rate(dtype, rows, 512, out)


if __name__ == "__main__":
    main()
