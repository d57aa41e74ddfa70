"""Batched top-k pull against the top-k pull it stands beside (DESIGN.md "Batched top-k pull", Measured).

    python tools/topk_batch_rate.py [--out FILE] [--rows N]

cfg5's per-GPU shard, 2^17 x 512, Float and Double, k = 16, q in {1, 8, 64, 256, 1024}. The shard and the
queries hold integers in [-8, 8], so both calls compute exact scores and must answer the same rows and
values: the tool asserts it. Baseline: glint_mat_pull_topk_dev issued ceil(q / 64) times. After a warm-up
round the two legs alternate inside each of 5 rounds, one HIP event pair around a leg. Then the launches of a
batched call apart (glint_prof_read_launches): the scores launch of a full pass as a share of its bound,
the larger of 2 * size * cols * 64 flops at the published matrix peak and the bytes read and written at
the published HBM peak (AMD Instinct MI355X data sheet: 157.3 TFLOP/s FP32 matrix, 78.6 TFLOP/s FP64
matrix, 8 TB/s). Last, what the matrix pipeline does with subnormal products, observed once per type.
One JSON line per (type, q) and one per type for the subnormals, appended to FILE
(profiles/topkbatch/topk_batch.jsonl)."""
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
PASS = N.GLINT_TOPK_MAX_QUERIES


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def launches(h, fn):
    """Per-launch device ms of one call of fn, in launch order."""
    lib.glint_prof_reset(h)
    lib.glint_prof_enable(h, 1)
    fn()
    torch.cuda.synchronize()
    cnt = C.c_int64()
    lib.glint_prof_read_launches(h, N.GLINT_K_PULL_ROWS_DOT, None, 0, C.byref(cnt))
    ms = (C.c_double * cnt.value)()
    lib.glint_prof_read_launches(h, N.GLINT_K_PULL_ROWS_DOT, ms, cnt.value, C.byref(cnt))
    lib.glint_prof_enable(h, 0)
    return np.array(ms[:])


def stats(ms):
    return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def rate(dtype, rows, cols, k, out):
    sh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, rows), cols, dtype, 0)
    h, tdt, vs = sh.handle, sh.torch_dtype, np.dtype(sh.np_dtype).itemsize
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    d_all = torch.arange(rows, dtype=torch.int64, device=dev)
    step = min(rows, 1 << 14)
    for r0 in range(0, rows, step):  # fill in slices of whole rows
        vv = torch.randint(-8, 9, (min(step, rows - r0), cols), device=dev, generator=gen).to(tdt)
        sh.updateRows(d_all[r0:r0 + step].contiguous(), vv)
    for q in (1, 8, 64, 256, 1024):
        d_x = torch.randint(-8, 9, (q, cols), device=dev, generator=gen).to(tdt)
        ans = {name: (torch.empty((q, k), dtype=torch.int64, device=dev), torch.empty((q, k), dtype=tdt, device=dev))
               for name in ("base", "batch")}

        def base():
            r, v = ans["base"]
            for q0 in range(0, q, PASS):
                n = min(PASS, q - q0)
                assert lib.glint_mat_pull_topk_dev(h, d_x[q0:].data_ptr(), n, k, r[q0:].data_ptr(), v[q0:].data_ptr(),
                                                   stream) == 0

        def batch():
            r, v = ans["batch"]
            assert lib.glint_mat_pull_topk_batch_dev(h, d_x.data_ptr(), q, k, r.data_ptr(), v.data_ptr(), stream) == 0

        t = {"base": [], "batch": []}
        for rnd in range(6):  # round 0 warms up; the legs alternate inside every round
            got = {"base": ev_ms(base), "batch": ev_ms(batch)}
            if rnd:
                for name, v in got.items():
                    t[name].append(v)
        sh.sync(stream)
        for a, b in zip(ans["base"], ans["batch"]):  # exact scores: the same rows, ties included
            assert torch.equal(a, b)
        each = launches(h, batch)
        per_pass = len(each) // -(-q // PASS)
        k_scores, k_select = float(each[0]), float(each[1:per_pass].sum())
        base_each = launches(h, base)
        qp = min(q, PASS)
        t_flops = 2.0 * rows * cols * PASS / PEAK_FLOPS[dtype]
        t_bytes = (rows * cols + qp * cols + qp * rows) * vs / PEAK_HBM
        line = dict(op="mat_pull_topk_batch", dtype=dtype, shape=[rows, cols], k=k, queries=q, rounds=5,
                    batch_ms=stats(t["batch"]), baseline_ms=stats(t["base"]),
                    speedup=float(np.mean(t["base"]) / np.mean(t["batch"])),
                    launches_per_pass=per_pass, scores_kernel_ms=k_scores, selection_kernels_ms=k_select,
                    baseline_scores_kernel_ms=float(base_each[0]),
                    bound_ms=max(t_flops, t_bytes) * 1e3, bound_is="flops" if t_flops > t_bytes else "bytes",
                    scores_share_of_bound=max(t_flops, t_bytes) * 1e3 / k_scores,
                    scores_TFLOPs=2.0 * rows * cols * qp / (k_scores * 1e-3) / 1e12,
                    scores_GBps=rows * cols * vs / (k_scores * 1e-3) / 1e9, same_answer=True)
        print(json.dumps(line), flush=True)
        with open(out, "a") as f:
            f.write(json.dumps(line) + "\n")
    sh.destroy()


def subnormals(dtype, out):
    """Scores whose products, inputs or sum are subnormal, against the exact values."""
    npd = glint_amd.shard.resolve_dtype(dtype)[1]
    fi = np.finfo(npd)
    tiny, sub = npd(fi.tiny), npd(fi.smallest_subnormal)
    table = np.zeros((3, 4), npd)
    table[0, 0] = 5 * sub          # a subnormal input times 1
    table[1, 0] = tiny             # normal inputs, a subnormal product
    table[2, :2] = [1.5 * tiny, -tiny]  # normal products, a subnormal sum
    x = np.array([[1, 1, 0, 0], [0.25, 0, 0, 0]], npd)
    exact = [5 * sub, tiny * npd(0.25), npd(0.5) * tiny]
    with glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, 3), 4, dtype, 0) as sh:
        sh.updateRows(np.arange(3, dtype=np.int64), table)
        rows, vals = sh.getTopKBatch(x, 3)
    got = [vals[0][rows[0] == 0][0], vals[1][rows[1] == 1][0], vals[0][rows[0] == 2][0]]
    line = dict(op="mat_pull_topk_batch_subnormals", dtype=dtype,
                subnormal_input_over_exact=float(got[0] / exact[0]),
                subnormal_product_over_exact=float(got[1] / exact[1]),
                subnormal_sum_over_exact=float(got[2] / exact[2]))
    print(json.dumps(line), flush=True)
    with open(out, "a") as f:
        f.write(json.dumps(line) + "\n")


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        str(Path(__file__).resolve().parent.parent / "profiles" / "topkbatch" / "topk_batch.jsonl")
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1 << 17
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    for dtype in ("float", "double"):
        subnormals(dtype, out)
        rate(dtype, rows, 512, 16, out)


if __name__ == "__main__":
    main()
