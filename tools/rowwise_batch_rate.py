"""Batched row-wise Adagrad row push against what a caller could do before it (DESIGN.md "Batched row-wise
Adagrad push", Measured).

    python tools/rowwise_batch_rate.py [--out FILE] [--rows N]

The batched optimizer row pushes' shard and lists (tools/step_batch_rate.py): 2^17 x 512, Float and Double; 2^12
and 2^15 distinct rows and 2^15 records drawn from a Zipf law (repeats); q in {8, 64, 256, 1024}. coef and x
hold -1, 0 and 1, so G is an exact integer in every order. Legs, all device-resident on one stream with no host
synchronisation inside:
  batch  the new call, glint_mat_push_rows_adagrad_rowwise_batch_dev;
  base   what the package offered before it: torch.unique of the rows, fill of those rows of a scratch shard
         with zeros, updateRowsAxpyBatch into it, getRows of the distinct rows, updateRowsAdagradRowwise of them;
  full   for information: updateRowsAdagradBatch with a full table of state, one product instead of two.
batch and base first step zeroed weights and accumulators once: they must leave the same bits in both shards
(`same_as_base`) wherever every row's sum of squares is below 2^24 (Float) / 2^53 (Double) and so exact in
either call's order (`exact_ss`), and the weights must match the step computed by torch in float64 within 64
ulp of the shard's type (`max_err_ulp`). After a warm-up round the legs alternate inside each of 5 rounds, one
HIP event pair around a leg. One JSON line per (type, list, q), appended to FILE
(profiles/rowwisebatch/rowwise_batch.jsonl)."""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import glint_amd  # noqa: E402
from glint_amd import _native as N  # noqa: E402
from step_batch_rate import ev_ms, row_lists, stats  # noqa: E402

dev = torch.device("cuda", 0)
lib = N.load()
stream = torch.cuda.current_stream(dev).cuda_stream
LR, EPS = 0.05, 1e-6


def rate(dtype, rows, cols, out):
    part = glint_amd.RangePartition(0, 0, rows)
    w, scratch, full = (glint_amd.PartialMatrix(part, cols, dtype, 0) for _ in range(3))
    h = glint_amd.PartialVector(part, dtype, 0)
    tdt = w.torch_dtype
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    for name, d_rows in row_lists(rows):
        n, u = d_rows.numel(), int(torch.unique(d_rows).numel())
        for q in (8, 64, 256, 1024):
            d_x = torch.randint(-1, 2, (q, cols), device=dev, generator=gen).to(tdt)
            d_c = torch.randint(-1, 2, (n, q), device=dev, generator=gen).to(tdt)
            args = (d_rows.data_ptr(), n, d_c.data_ptr(), d_x.data_ptr(), q, LR, EPS, 0, stream)

            def batch():
                assert lib.glint_mat_push_rows_adagrad_rowwise_batch_dev(w.handle, h.handle, *args) == 0

            def base():
                distinct = torch.unique(d_rows)
                scratch.fill(0, distinct, sync=False)
                scratch.updateRowsAxpyBatch(d_rows, d_c, d_x, sync=False)
                w.updateRowsAdagradRowwise(h, distinct, scratch.getRows(distinct, sync=False), LR, EPS, sync=False)

            def full_state():
                assert lib.glint_mat_push_rows_adagrad_batch_dev(w.handle, full.handle, *args) == 0

            legs = {"batch": batch, "base": base, "full": full_state}
            G = torch.zeros((rows, cols), dtype=torch.float64, device=dev)
            G.index_add_(0, d_rows, d_c.double() @ d_x.double())
            ss = (G * G).sum(1)
            exact_ss = bool(ss.max() < (2 ** 24 if dtype == "float" else 2 ** 53))
            ref = -(LR / ((ss / cols).sqrt() + EPS))[:, None] * G  # the first step from zeroed shards
            del G, ss
            got = {}
            for leg in ("batch", "base"):
                w.zero(), h.zero()
                legs[leg]()
                w.sync(stream)
                got[leg] = (torch.from_numpy(w.to_numpy()).to(dev), torch.from_numpy(h.to_numpy()).to(dev))
            same = all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(got["batch"], got["base"]))
            ulp = torch.finfo(tdt).eps * ref.abs().clamp_min(torch.finfo(tdt).tiny)
            err_ulp = float(((got["batch"][0].double() - ref).abs() / ulp).max())
            del got, ref
            t = {leg: [] for leg in legs}
            for rnd in range(6):  # round 0 warms up; the legs alternate inside every round
                for leg, fn in legs.items():
                    ms = ev_ms(fn)
                    if rnd:
                        t[leg].append(ms)
            w.sync(stream)
            spread = max(t["base"]) - min(t["base"])
            line = dict(op="mat_push_rows_adagrad_rowwise_batch", dtype=dtype, shape=[rows, cols], rows=name, n=n,
                        distinct=u, vectors=q, rounds=5, **{leg + "_ms": stats(v) for leg, v in t.items()},
                        speedup=float(np.mean(t["base"]) / np.mean(t["batch"])),
                        faster_by_more_than_baseline_spread=bool(np.mean(t["base"]) - np.mean(t["batch"]) > spread),
                        over_full_state=float(np.mean(t["batch"]) / np.mean(t["full"])),
                        exact_ss=exact_ss, same_as_base=same, max_err_ulp=err_ulp)
            print(json.dumps(line), flush=True)
            with open(out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del d_c, d_x
    for sh in (w, h, scratch, full):
        sh.destroy()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        str(Path(__file__).resolve().parent.parent / "profiles" / "rowwisebatch" / "rowwise_batch.jsonl")
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1 << 17
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    for dtype in ("float", "double"):
        rate(dtype, rows, 512, out)


if __name__ == "__main__":
    main()
