"""Batched optimizer row pushes against what a caller could do before them (DESIGN.md "Batched optimizer row
pushes", Measured).

    python tools/step_batch_rate.py [--out FILE] [--rows N]

The batched row axpy push's shard and lists (tools/axpy_batch_rate.py): 2^17 x 512, Float and Double; 2^12 and
2^15 distinct rows and 2^15 records drawn from a Zipf law (repeats); q in {8, 64, 256, 1024}; Adagrad, Adam and
FTRL-proximal. coef and x hold -1, 0 and 1, so G is an exact integer in every order. Legs, all device-resident
on one stream with no host synchronisation inside:
  batch  the new call, glint_mat_push_rows_<opt>_batch_dev;
  base   what the package offered before it: torch.unique of the rows, fill of those rows of a scratch shard
         with zeros (cheaper than zeroing the whole shard), updateRowsAxpyBatch into it, getRows of the distinct
         rows, the unbatched optimizer push of those rows.
Each leg first steps zeroed weights and state once: the two legs must leave the same bits (`same_as_base`: G is
exact, so both take the same step), and the weights must match the step computed by torch in float64 from the
float64 G within 64 ulp of the shard's type (`max_err_ulp`). After a warm-up round the legs alternate inside
each of 5 rounds, one HIP event pair around a leg. One JSON line per (optimizer, type, list, q), appended to
FILE (profiles/stepbatch/step_batch.jsonl), with both times and their ratio."""
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
SCALARS = dict(adagrad=(0.05, 1e-6), adam=(0.01, 0.9, 0.999, 1e-8, 3), ftrl=(0.05, 1.0, 0.3, 1e-4))  # the C calls'
PARTS = dict(adagrad=1, adam=2, ftrl=2)


def ev_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def stats(ms):
    return {"mean": float(np.mean(ms)), "min": float(np.min(ms)), "max": float(np.max(ms))}


def row_lists(rows):
    gen = torch.Generator(device=dev)
    gen.manual_seed(7)
    perm = torch.randperm(rows, device=dev, generator=gen)
    zipf = np.random.default_rng(3).zipf(1.2, 1 << 15) % rows
    return [("distinct_2p12", perm[:1 << 12].contiguous()), ("distinct_2p15", perm[:1 << 15].contiguous()),
            ("zipf_2p15", torch.from_numpy(zipf.astype(np.int64)).to(dev))]


def first_step(opt, G):
    """The weights after one step from zeroed weights and state, in float64 (G float64, exact)."""
    k = SCALARS[opt]
    if opt == "adagrad":
        return -(k[0] * G) / (G.abs() + k[1])
    if opt == "adam":
        lr, b1, b2, eps, step = k
        m, v = (1 - b1) * G, (1 - b2) * G * G
        return -(lr / (1 - b1 ** step) * m) / (v.sqrt() / (1 - b2 ** step) ** 0.5 + eps)
    alpha, beta, l1, l2 = k
    w = -(G - torch.sign(G) * l1) / ((beta + G.abs()) / alpha + l2)
    return torch.where(G.abs() <= l1, torch.zeros_like(G), w)


def rate(opt, dtype, rows, cols, out):
    part = glint_amd.RangePartition(0, 0, rows)
    w, s, scratch = (glint_amd.PartialMatrix(part, c, dtype, 0) for c in (cols, PARTS[opt] * cols, cols))
    tdt, k = w.torch_dtype, SCALARS[opt]
    batch_dev = getattr(lib, f"glint_mat_push_rows_{opt}_batch_dev")
    plain = getattr(w, {"adagrad": "updateRowsAdagrad", "adam": "updateRowsAdam", "ftrl": "updateRowsFtrl"}[opt])
    plain_args = k if opt != "adam" else (k[0], k[4], k[1], k[2], k[3])  # (lr, step, beta1, beta2, eps)
    gen = torch.Generator(device=dev)
    gen.manual_seed(11)
    for name, d_rows in row_lists(rows):
        n, u = d_rows.numel(), int(torch.unique(d_rows).numel())
        for q in (8, 64, 256, 1024):
            d_x = torch.randint(-1, 2, (q, cols), device=dev, generator=gen).to(tdt)
            d_c = torch.randint(-1, 2, (n, q), device=dev, generator=gen).to(tdt)

            def batch():
                assert batch_dev(w.handle, s.handle, d_rows.data_ptr(), n, d_c.data_ptr(), d_x.data_ptr(), q, *k, 0,
                                 stream) == 0

            def base():
                distinct = torch.unique(d_rows)
                scratch.fill(0, distinct, sync=False)
                scratch.updateRowsAxpyBatch(d_rows, d_c, d_x, sync=False)
                plain(s, distinct, scratch.getRows(distinct, sync=False), *plain_args, sync=False)

            legs = {"batch": batch, "base": base}
            G = torch.zeros((rows, cols), dtype=torch.float64, device=dev)
            G.index_add_(0, d_rows, d_c.double() @ d_x.double())
            ref = first_step(opt, G)
            exact = bool(G.abs().max() < 2 ** 24)
            del G
            got = {}
            for leg, fn in legs.items():  # one step each from zeroed shards
                w.zero(), s.zero()
                fn()
                w.sync(stream)
                got[leg] = (torch.from_numpy(w.to_numpy()).to(dev), torch.from_numpy(s.to_numpy()).to(dev))
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
            line = dict(op=f"mat_push_rows_{opt}_batch", dtype=dtype, shape=[rows, cols], rows=name, n=n, distinct=u,
                        vectors=q, rounds=5, **{leg + "_ms": stats(v) for leg, v in t.items()},
                        speedup=float(np.mean(t["base"]) / np.mean(t["batch"])),
                        faster_by_more_than_baseline_spread=bool(np.mean(t["base"]) - np.mean(t["batch"]) > spread),
                        exact_product=exact, same_as_base=same, max_err_ulp=err_ulp, same_answer=same and err_ulp <= 64)
            print(json.dumps(line), flush=True)
            with open(out, "a") as f:
                f.write(json.dumps(line) + "\n")
            del d_c, d_x
    for sh in (w, s, scratch):
        sh.destroy()


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else \
        str(Path(__file__).resolve().parent.parent / "profiles" / "stepbatch" / "step_batch.jsonl")
    rows = int(sys.argv[sys.argv.index("--rows") + 1]) if "--rows" in sys.argv else 1 << 17
    Path(out).parent.mkdir(parents=True, exist_ok=True)
    for opt in ("adagrad", "adam", "ftrl"):
        for dtype in ("float", "double"):
            rate(opt, dtype, rows, 512, out)


if __name__ == "__main__":
    main()
