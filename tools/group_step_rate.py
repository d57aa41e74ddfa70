"""Times of the grouped optimizer row pushes (updateRows* with ``offsets``) beside the way the same step is
done without them, in one run: device-form calls of 2^20 records in bags of 32 against a 2^22-row Float shard.

  grouped   updateRowsX(state, rows, values, ..., offsets=offsets, weights=weights): g x cols value rows
  expand    the yardstick: values.index_select(0, group) * weights[:, None] on the stream with torch, then
            updateRowsX(state, rows, expanded, ...) of the n x cols result; both timed together

for the four optimizers, cols 64 and 128, rows drawn uniformly from the shard and from a hot set of 2^12 rows.
The two are run alternately, ROUNDS rounds of REPS back-to-back unsynchronised calls each between two device
events; one JSON line per case with both medians, each one's spread over the rounds and the ratio
grouped / expand. Run it as one step under its own time limit:

    timeout -k 10 600 python tools/group_step_rate.py [--rounds R] [--reps K]
"""
import json
import statistics
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
from glint_amd import PartialMatrix, PartialVector, RangePartition  # noqa: E402


def arg(name, default):
    return int(sys.argv[sys.argv.index(name) + 1]) if name in sys.argv else default


ROUNDS, REPS = arg("--rounds", 7), arg("--reps", 5)
SHARD, HOT, N, BAG = 1 << 22, 1 << 12, 1 << 20, 32
# name -> (method, scalars, state columns per weights column; 0: a vector)
OPT = {
    "adagrad": ("updateRowsAdagrad", (0.05, 1e-6), 1),
    "rowwise": ("updateRowsAdagradRowwise", (0.05, 1e-6), 0),
    "adam": ("updateRowsAdam", (0.05, 1), 2),
    "ftrl": ("updateRowsFtrl", (0.1, 1.0, 0.5, 0.01), 2),
}


def timed(fn, dev):
    """Milliseconds per call of fn, REPS calls back to back between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(REPS):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / REPS


def main():
    if not torch.cuda.is_available():
        raise SystemExit("group_step_rate: no GPU (there is nothing to measure without one)")
    dev = torch.device("cuda", 0)
    torch.manual_seed(1)
    part = RangePartition(0, 0, SHARD)
    g = N // BAG
    offsets = torch.arange(0, N + 1, BAG, device=dev)
    group = torch.arange(N, device=dev) // BAG
    weights = torch.rand(N, device=dev)
    for cols in (64, 128):
        values = torch.randn(g, cols, device=dev) * 0.01
        for name, (method, k, parts) in OPT.items():
            w = PartialMatrix(part, cols, "float", 0)
            s = PartialMatrix(part, parts * cols, "float", 0) if parts else PartialVector(part, "float", 0)
            with w, s:
                call = getattr(w, method)
                for dist, span in (("uniform", SHARD), ("hot", HOT)):
                    rows = torch.randint(0, span, (N,), device=dev)
                    grouped = lambda: call(s, rows, values, *k, sync=False, offsets=offsets,  # noqa: E731
                                           weights=weights)
                    expand = lambda: call(s, rows, values.index_select(0, group) * weights[:, None], *k,  # noqa: E731
                                          sync=False)
                    ms = {"grouped": [], "expand": []}
                    for r in range(ROUNDS + 1):  # round 0 warms both up
                        for what, fn in (("grouped", grouped), ("expand", expand)):
                            t = timed(fn, dev)
                            if r:
                                ms[what].append(t)
                    w.sync()
                    s.sync()
                    med = {what: statistics.median(v) for what, v in ms.items()}
                    print(json.dumps({
                        "optimizer": name, "cols": cols, "rows": dist, "records": N, "bag": BAG,
                        "grouped_ms": round(med["grouped"], 4), "expand_ms": round(med["expand"], 4),
                        "grouped_spread": [round(min(ms["grouped"]), 4), round(max(ms["grouped"]), 4)],
                        "expand_spread": [round(min(ms["expand"]), 4), round(max(ms["expand"]), 4)],
                        "ratio": round(med["grouped"] / med["expand"], 3)}), flush=True)


if __name__ == "__main__":
    main()
