"""Batched row mix pull against what a caller could do without it (DESIGN.md "Batched row mix pull", Measured).

    python tools/mix_batch_rate.py [--out FILE] [--rows N] [--only-mix] [--chunk C]

cfg5's per-GPU shard, 2^17 x 512, Float and Double; n in {2^12, 2^15} distinct rows; q in {1, 8, 64, 256,
1024}. The shard holds integers in [-8, 8] and coef holds -1, 0, 1, so every leg is exact and is compared with
a float64 product. Legs, device calls on one stream:
  mix    glint_mat_pull_rows_mix_batch_dev;
  wsum   what the library offered before: glint_mat_pull_rows_wsum_dev with q groups of all n rows, n * q
         records (run where n * q <= 2^25; else reported as not run);
  pull   glint_mat_pull_rows_dev of the n rows, then torch.matmul(coef.T, rows).
After a warm-up round the legs alternate inside each of 5 rounds, one HIP event pair around a leg. Then the
launches of one mix call (glint_prof_read_launches under GLINT_K_PULL_ROWS_SUM: the product, then the reduce
when there is more than one chunk), the product as a share of its bound: the larger of 2 * n * q * cols flops
at the published matrix peak and the bytes it reads and writes -- the rows, coef and one partial per chunk --
at the published HBM peak (AMD Instinct MI355X data sheet: 157.3 TFLOP/s FP32 matrix, 78.6 TFLOP/s FP64
matrix, 8 TB/s). One JSON line per (type, n, q), appended to FILE (profiles/mixbatch/mix_batch.jsonl).

--only-mix times the mix leg alone; with GLINT_GPU_LIB naming a library built with
-DGLINT_MIX_BATCH_CHUNK=C and --chunk C it is the chunk-size comparison (profiles/mixbatch/chunk_sweep.jsonl)."""
import ctypes as C
import json
import os
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
WSUM_MAX_RECORDS = 1 << 25


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches_ms(h, fn):
    """Device ms of every GLINT_K_PULL_ROWS_SUM launch of fn, in launch order."""
    lib.glint_prof_reset(h)
    lib.glint_prof_enable(h, 1)
    fn()
    torch.cuda.synchronize()
    cnt = C.c_int64()
    lib.glint_prof_read_launches(h, N.GLINT_K_PULL_ROWS_SUM, None, 0, C.byref(cnt))
    ms = (C.c_double * cnt.value)()
    lib.glint_prof_read_launches(h, N.GLINT_K_PULL_ROWS_SUM, ms, cnt.value, C.byref(cnt))
    lib.glint_prof_enable(h, 0)
    return [float(v) for v in ms]


def stats(ms):
    return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def chunk_count(n, chunk):
    length = chunk
    while -(-n // length) > N.GLINT_MIX_BATCH_MAX_CHUNKS:
        length *= 2
    return -(-n // length)


def rate(dtype, rows, cols, out, only_mix, chunk):
    sh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, rows), cols, dtype, 0)
    h, tdt, vs = sh.handle, sh.torch_dtype, np.dtype(sh.np_dtype).itemsize
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    d_all = torch.arange(rows, dtype=torch.int64, device=dev)
    table = torch.randint(-8, 9, (rows, cols), device=dev, generator=gen).to(tdt)
    step = min(rows, 1 << 14)
    for r0 in range(0, rows, step):  # fill in slices of whole rows
        sh.updateRows(d_all[r0:r0 + step].contiguous(), table[r0:r0 + step].contiguous())
    for n in (1 << 12, 1 << 15):
        d_rows = torch.randperm(rows, device=dev, generator=gen)[:n].contiguous()  # distinct
        picked = table[d_rows].double()
        for q in (1, 8, 64, 256, 1024):
            d_coef = torch.randint(-1, 2, (n, q), device=dev, generator=gen).to(tdt)
            ref = (d_coef.double().T @ picked).to(tdt)  # exact: integers far below 2^24
            names = ["mix"] if only_mix else ["mix", "pull"] + (["wsum"] if n * q <= WSUM_MAX_RECORDS else [])
            ans = {name: torch.empty((q, cols), dtype=tdt, device=dev) for name in names}
            pulled = torch.empty((n, cols), dtype=tdt, device=dev)
            if "wsum" in names:
                w_rows, w_coef = d_rows.repeat(q), d_coef.T.contiguous().reshape(-1)
                w_ptr = torch.arange(q + 1, dtype=torch.int64, device=dev) * n

            def mix():
                assert lib.glint_mat_pull_rows_mix_batch_dev(h, d_rows.data_ptr(), n, d_coef.data_ptr(), q,
                                                             ans["mix"].data_ptr(), stream) == 0

            def wsum():
                assert lib.glint_mat_pull_rows_wsum_dev(h, w_rows.data_ptr(), n * q, w_ptr.data_ptr(), q,
                                                        w_coef.data_ptr(), ans["wsum"].data_ptr(), stream) == 0

            def pull():
                assert lib.glint_mat_pull_rows_dev(h, d_rows.data_ptr(), pulled.data_ptr(), n, stream) == 0
                torch.matmul(d_coef.T, pulled, out=ans["pull"])

            legs = {"mix": mix, "wsum": wsum, "pull": pull}
            t = {name: [] for name in names}
            for rnd in range(6):  # round 0 warms up; the legs alternate inside every round
                got = {name: ev_ms(legs[name]) for name in names}
                if rnd:
                    for name, v in got.items():
                        t[name].append(v)
            sh.sync(stream)
            for name in names:
                assert torch.equal(ans[name], ref), name
            k = launches_ms(h, mix)
            nchunks = chunk_count(n, chunk)
            assert len(k) == (1 if nchunks == 1 else 2)
            t_flops = 2.0 * n * q * cols / PEAK_FLOPS[dtype]
            t_bytes = (n * cols + n * q + nchunks * q * cols) * vs / PEAK_HBM
            line = dict(op="mat_pull_rows_mix_batch", dtype=dtype, shape=[rows, cols], n=n, vectors=q, rounds=5,
                        chunk=chunk, chunks=nchunks, library=os.path.basename(os.environ.get("GLINT_GPU_LIB", "in-tree")),
                        mix_ms=stats(t["mix"]), product_kernel_ms=k[0], reduce_kernel_ms=k[1] if len(k) > 1 else None,
                        bound_ms=max(t_flops, t_bytes) * 1e3, bound_is="flops" if t_flops > t_bytes else "bytes",
                        share_of_bound=max(t_flops, t_bytes) * 1e3 / k[0],
                        TFLOPs=2.0 * n * q * cols / (k[0] * 1e-3) / 1e12, same_answer=True)
            if not only_mix:
                line["pull_matmul_ms"] = stats(t["pull"])
                line["pull_matmul_over_mix"] = float(np.mean(t["pull"]) / np.mean(t["mix"]))
                line["wsum_ms"] = stats(t["wsum"]) if "wsum" in names else "not run"
                line["wsum_over_mix"] = float(np.mean(t["wsum"]) / np.mean(t["mix"])) if "wsum" in names else None
            print(json.dumps(line), flush=True)
            with open(out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del ans
    sh.destroy()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        str(Path(__file__).resolve().parent.parent / "profiles" / "mixbatch" / "mix_batch.jsonl")
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1 << 17
    chunk = int(sys.argv[sys.argv.index("--chunk") + 1]) if "--chunk" in sys.argv else N.GLINT_MIX_BATCH_CHUNK
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    for dtype in ("float", "double"):
        rate(dtype, rows, 512, out, "--only-mix" in sys.argv, chunk)


if __name__ == "__main__":
    main()
