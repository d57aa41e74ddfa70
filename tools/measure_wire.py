#!/usr/bin/env python
"""A/B of the narrow-format row transport against the wide row calls on one MI355X (profiles/wire/README.md).

One Float shard of 2^16 rows x 512 columns (128 MiB as float, 64 MiB as a 16-bit wire type); every call names
every row once, in a shuffled order.

* host: wall time of getRows against getRowsAs (float16, bfloat16) and of updateRows against updateRowsAs, each
  into / from preallocated numpy arrays; the legs alternate call by call inside one process, `--calls` calls
  each after `--warmup`;
* device: kernel time (glint_prof_read_launches) of the unchanged mat_pull_rows_kernel and rows_fold_kernel
  against rows_pull_as and rows_fold_as at that shape, the device calls alternating likewise.

The whole A/B runs `--passes` times in the process; the spread between passes is what a ratio is read against.
One JSON line per pass, to stdout and appended to --out.
"""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

import glint_amd  # noqa: E402
from glint_amd import _native as N  # noqa: E402
from glint_amd import PartialMatrix, RangePartition  # noqa: E402


def stats(ms):
    ms = np.asarray(ms, np.float64)
    return {"median": round(float(np.median(ms)), 4), "min": round(float(ms.min()), 4),
            "max": round(float(ms.max()), 4), "n": int(ms.size)}


def launches(sh, kid):
    lib = N.load()
    cnt = C.c_int64()
    lib.glint_prof_read_launches(sh.handle, kid, None, 0, C.byref(cnt))
    ms = (C.c_double * max(cnt.value, 1))()
    lib.glint_prof_read_launches(sh.handle, kid, ms, cnt.value, C.byref(cnt))
    return np.array(ms[:cnt.value])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=1 << 16)
    ap.add_argument("--cols", type=int, default=512)
    ap.add_argument("--calls", type=int, default=24)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--passes", type=int, default=2)
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "wire" / "wire.jsonl"))
    a = ap.parse_args()
    import torch

    lib = N.load()
    rows_n, cols, gpu = a.rows, a.cols, a.device
    rng = np.random.default_rng(7)
    d = torch.device("cuda", gpu)
    rows = rng.permutation(rows_n).astype(np.int64)
    wide = rng.standard_normal((rows_n, cols)).astype(np.float32)
    narrow = {"float16": wide.astype(np.float16), "bfloat16": glint_amd.to_bfloat16(wide)}
    out_wide = np.empty((rows_n, cols), np.float32)
    out_narrow = {w: np.empty((rows_n, cols), v.dtype) for w, v in narrow.items()}
    wires = list(narrow)
    Path(a.out).parent.mkdir(parents=True, exist_ok=True)

    with PartialMatrix(RangePartition(0, 0, rows_n), cols, "float", gpu) as sh:
        sh.initUniform(1, -1.0, 1.0)
        rows_d = torch.from_numpy(rows).to(d)
        wide_d = torch.from_numpy(wide).to(d)
        narrow_d = {"float16": torch.from_numpy(narrow["float16"]).to(d),
                    "bfloat16": torch.from_numpy(narrow["bfloat16"].view(np.int16)).to(d).view(torch.bfloat16)}
        outw_d = torch.empty((rows_n, cols), dtype=torch.float32, device=d)
        outn_d = {w: torch.empty((rows_n, cols), dtype=getattr(torch, w), device=d) for w in wires}

        host_legs = {"getRows": lambda: sh.getRows(rows, out=out_wide),
                     "updateRows": lambda: sh.updateRows(rows, wide)}
        for w in wires:
            host_legs[f"getRowsAs[{w}]"] = lambda w=w: sh.getRowsAs(rows, w, out=out_narrow[w])
            host_legs[f"updateRowsAs[{w}]"] = lambda w=w: sh.updateRowsAs(rows, narrow[w], w)

        for p in range(a.passes):
            # ---- host: wall time, the legs alternating call by call
            wall = {k: [] for k in host_legs}
            for i in range(a.warmup + a.calls):
                for k, f in host_legs.items():
                    t0 = time.perf_counter()
                    f()
                    if i >= a.warmup:
                        wall[k].append((time.perf_counter() - t0) * 1e3)
            # ---- device: kernel time per launch; the wide and the narrow calls are told apart by running each
            # kind in a block of its own between two reads of the per-launch times
            assert lib.glint_prof_enable(sh.handle, 1) == N.GLINT_OK
            kern = {}
            dev_legs = [("mat_pull_rows_kernel", N.GLINT_K_MAT_PULL_ROWS,
                         lambda: sh.getRows(rows_d, out=outw_d, sync=False)),
                        ("rows_fold_kernel", N.GLINT_K_PUSH_ROWS,
                         lambda: sh.updateRows(rows_d, wide_d, sync=False))]
            for w in wires:
                dev_legs.append((f"rows_pull_as[{w}]", N.GLINT_K_MAT_PULL_ROWS,
                                 lambda w=w: sh.getRowsAs(rows_d, w, out=outn_d[w], sync=False)))
                dev_legs.append((f"rows_fold_as[{w}]", N.GLINT_K_PUSH_ROWS,
                                 lambda w=w: sh.updateRowsAs(rows_d, narrow_d[w], w, sync=False)))
            for r in range(4):  # four blocks per leg, the legs alternating block by block
                for name, kid, f in dev_legs:
                    assert lib.glint_prof_reset(sh.handle) == N.GLINT_OK
                    for _ in range(a.warmup if r == 0 else 0):
                        f()
                    sh.sync(sh._stream_of(rows_d))
                    assert lib.glint_prof_reset(sh.handle) == N.GLINT_OK
                    for _ in range(a.calls // 4):
                        f()
                    sh.sync(sh._stream_of(rows_d))
                    kern.setdefault(name, []).extend(launches(sh, kid).tolist())
            assert lib.glint_prof_enable(sh.handle, 0) == N.GLINT_OK
            line = {"tool": "measure_wire", "pass": p, "rows": rows_n, "cols": cols, "dtype": "float",
                    "wide_MiB": rows_n * cols * 4 / 2 ** 20, "narrow_MiB": rows_n * cols * 2 / 2 ** 20,
                    "host_wall_ms": {k: stats(v) for k, v in wall.items()},
                    "kernel_ms": {k: stats(v) for k, v in kern.items()}}
            hw, km = line["host_wall_ms"], line["kernel_ms"]
            ratio = lambda tab, narrow, wide: round(tab[narrow]["median"] / tab[wide]["median"], 3)  # noqa: E731
            line["ratios_narrow_over_wide"] = {
                **{f"getRowsAs[{w}]": ratio(hw, f"getRowsAs[{w}]", "getRows") for w in wires},
                **{f"updateRowsAs[{w}]": ratio(hw, f"updateRowsAs[{w}]", "updateRows") for w in wires},
                **{f"rows_pull_as[{w}]": ratio(km, f"rows_pull_as[{w}]", "mat_pull_rows_kernel") for w in wires},
                **{f"rows_fold_as[{w}]": ratio(km, f"rows_fold_as[{w}]", "rows_fold_kernel") for w in wires}}
            print(json.dumps(line), flush=True)
            with open(a.out, "a") as f:
                f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
