#!/usr/bin/env python3
"""Row push against the equivalent triplet push, same process, alternating (DESIGN.md "Row push").

Shape: cfg5's per-GPU shard (2^17 rows x 512 Double) and its per-GPU push size in elements: 2^14 whole
rows = 2^23 elements per push, device-resident. Two seeded lines:

  once   a permutation's first 2^14 rows: every row at most once;
  zipf   rows drawn Zipf(1.0) through a seeded permutation, as bench.py --pattern matrix draws them.

Legs per line, each on a shard of its own, timed in alternating rounds of --pushes pushes between
device synchronisations (the median round is reported):

  rows       glint_mat_push_rows_dev, default flags;
  rows_det   the same with GLINT_PUSH_DETERMINISTIC (zipf line only);
  triplets   the same update expanded to (row, col, value) triplets through glint_mat_push_dev.

Each shape is warmed up with a sync after every push (the triplet path's adaptive switch decides from
the last sync point). After timing, every shard is checked against a torch index_add_ of the records
it received (Double: within 1e-9 of sum |v| per element), and one Long row push against an exact
index_add_; a mismatch exits non-zero. One JSON line per leg on stdout.

  python tools/rowpush_bench.py [--pushes 500] [--rounds 5] [--warmup 20] [--device 0]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import statistics
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

ROWS, COLS, NPUSH = 1 << 17, 512, 1 << 14
PEAK = 8.0e12  # HBM bytes/s the fraction is taken of


def zipf_rows(rng, n, count):
    """Zipf(1.0) ranks over [0, n): bench.py's draw."""
    import numpy as np
    return np.minimum(np.floor(np.power(float(n), rng.random(count))).astype(np.int64) - 1, n - 1)


def main() -> int:
    ap = argparse.ArgumentParser()
    ap.add_argument("--pushes", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--device", type=int, default=0)
    args = ap.parse_args()
    if args.pushes < 50:
        ap.error("--pushes: at least 50 pushes per timed leg")

    import numpy as np
    import torch
    from glint_amd import PartialMatrix, RangePartition
    from glint_amd import _native as N

    lib = N.load()
    dev = torch.device("cuda", args.device)
    torch.cuda.set_device(dev)
    stream = torch.cuda.current_stream(dev).cuda_stream
    part = RangePartition(0, 0, ROWS)
    rng = np.random.default_rng(42)
    perm = rng.permutation(ROWS)
    lines = {"once": perm[:NPUSH].astype(np.int64), "zipf": perm[zipf_rows(rng, ROWS, NPUSH)].astype(np.int64)}
    gen = torch.Generator(device=dev)
    gen.manual_seed(42)
    col_t = torch.arange(COLS, dtype=torch.int32, device=dev).repeat(NPUSH)
    ok = True

    for name, r_np in lines.items():
        rows = torch.from_numpy(r_np).to(dev)
        vals = torch.rand((NPUSH, COLS), dtype=torch.float64, device=dev, generator=gen) * 2 - 1
        row_t = rows.repeat_interleave(COLS)
        uniq = int(np.unique(r_np).size)
        nbytes = NPUSH * 8 + NPUSH * COLS * 8 + uniq * 2 * COLS * 8
        legs = ["rows", "triplets"] + (["rows_det"] if name == "zipf" else [])
        shards = {leg: PartialMatrix(part, COLS, "double", device=args.device) for leg in legs}
        pushed = {leg: 0 for leg in legs}

        def push(leg):
            h = shards[leg].handle
            if leg == "triplets":
                rc = lib.glint_mat_push_dev(h, row_t.data_ptr(), col_t.data_ptr(), vals.data_ptr(), NPUSH * COLS, 0,
                                            stream)
            else:
                flags = N.GLINT_PUSH_DETERMINISTIC if leg == "rows_det" else 0
                rc = lib.glint_mat_push_rows_dev(h, rows.data_ptr(), vals.data_ptr(), NPUSH, flags, stream)
            if rc:
                raise RuntimeError(N.strerror(rc))
            pushed[leg] += 1

        for leg in legs:
            for _ in range(args.warmup):
                push(leg)
                shards[leg].sync(stream)
            lib.glint_prof_reset(shards[leg].handle)
        times = {leg: [] for leg in legs}
        for _ in range(args.rounds):  # alternating: every leg sees the same box state
            for leg in legs:
                lib.glint_prof_enable(shards[leg].handle, 1)
                torch.cuda.synchronize(dev)
                t0 = time.perf_counter()
                for _ in range(args.pushes):
                    push(leg)
                torch.cuda.synchronize(dev)
                times[leg].append((time.perf_counter() - t0) / args.pushes * 1e3)
                lib.glint_prof_enable(shards[leg].handle, 0)
                shards[leg].sync(stream)

        # check: every shard holds `pushed` times the push
        ref1 = torch.zeros((ROWS, COLS), dtype=torch.float64, device=dev)
        ref1.index_add_(0, rows, vals)
        mag1 = torch.zeros((ROWS, COLS), dtype=torch.float64, device=dev)
        mag1.index_add_(0, rows, vals.abs())
        all_rows = torch.arange(ROWS, dtype=torch.int64, device=dev)
        ms_of = {leg: statistics.median(times[leg]) for leg in legs}
        for leg in legs:
            got = shards[leg].getRows(all_rows)
            k = pushed[leg]
            # k pushes of the same values: the reference k * sum is exact up to one rounding per
            # element, the shard's k-fold accumulation stays within 1e-9 of the k-fold sum |v|
            err = (got - ref1 * k).abs()
            bad = int((err > 1e-9 * mag1 * k).sum())
            if bad:
                ok = False
            ms, cnt = C.c_double(), C.c_int64()
            lib.glint_prof_read(shards[leg].handle, N.GLINT_K_PUSH_ROWS, C.byref(ms), C.byref(cnt))
            t = ms_of[leg]
            print(json.dumps({
                "line": name, "leg": leg, "rows_per_push": NPUSH, "cols": COLS, "distinct_rows": uniq,
                "ms_per_push": round(t, 4), "ms_rounds": [round(x, 4) for x in times[leg]],
                "algorithmic_bytes": nbytes, "GBps": round(nbytes / t / 1e6, 1),
                "frac_of_8TBps": round(nbytes / (t * 1e-3) / PEAK, 4),
                "push_rows_kernel_ms": round(ms.value / cnt.value, 4) if cnt.value else None,
                "push_rows_launches": cnt.value,
                "speedup_vs_triplets": round(ms_of["triplets"] / t, 3),
                "pushes_checked": k, "check": "ok" if not bad else f"{bad} elements off by more than 1e-9 sum|v|",
            }), flush=True)
        for sh in shards.values():
            sh.destroy()
        del ref1, mag1, row_t

        # Long: exact
        lv = torch.randint(-(1 << 40), 1 << 40, (NPUSH, COLS), dtype=torch.int64, device=dev, generator=gen)
        with PartialMatrix(part, COLS, "long", device=args.device) as sh:
            sh.updateRows(rows, lv)
            want = torch.zeros((ROWS, COLS), dtype=torch.int64, device=dev)
            want.index_add_(0, rows, lv)
            exact = bool(torch.equal(sh.getRows(all_rows), want))
        print(json.dumps({"line": name, "leg": "rows_long_check", "check": "ok" if exact else "MISMATCH"}), flush=True)
        ok = ok and exact
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
