"""Rates of the device key map (glint_amd.KeyMap) beside the project's own random gather, in one run: device-form
calls of 2^20 records against a map that holds 2^24 keys at the default load factor, timed with device events
around back-to-back unsynchronised calls on one stream.

  lookup_hit / lookup_miss   2^20 random present / absent keys
  insert_present             2^20 random present keys (no atomics, nothing committed)
  insert_new                 the last batches of the fill: 2^20 distinct new keys each, the map 13/16 .. 15/16 full
  gather                     the yardstick: PartialVector.get of 2^20 random keys of a 2^24-key Long shard

One JSON line per figure on stdout, then one with the ratios. Run it as one step under its own time limit:

    timeout -k 10 600 python tools/keymap_rate.py [--reps R]
"""
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
from glint_amd import KeyMap, PartialVector, RangePartition  # noqa: E402

REPS = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 1000
HELD, BATCH = 1 << 24, 1 << 20
ODD = 0x5851F42D4C957F2D  # key i = i * ODD + 1 (mod 2^64): distinct, spread over all 64 bits


def timed(fn, reps, dev):
    """Milliseconds per call of fn, reps calls back to back between two events."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize(dev)
    a.record()
    for _ in range(reps):
        fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / reps


def report(op, ms, **kw):
    print(json.dumps({"op": op, "records": BATCH, "ms_per_call": round(ms, 4),
                      "records_per_s": round(BATCH / ms * 1e3), **kw}), flush=True)
    return BATCH / ms * 1e3


def main():
    if not torch.cuda.is_available():
        raise SystemExit("keymap_rate: no GPU (there is nothing to measure without one)")
    dev = torch.device("cuda", 0)
    key = lambda i: i * ODD + 1  # noqa: E731  (int64 arithmetic wraps)
    out = torch.empty(BATCH, dtype=torch.int64, device=dev)
    pick = lambda lo, hi: key(torch.randint(lo, hi, (BATCH,), device=dev))  # noqa: E731
    torch.manual_seed(1)
    rate = {}
    with KeyMap(HELD, 0, 0) as km:
        new_ms = []
        for b in range(HELD // BATCH):  # the fill: each batch 2^20 distinct new keys
            batch = key(torch.arange(b * BATCH, (b + 1) * BATCH, device=dev))
            new_ms.append(timed(lambda: km.insert(batch, out=out, sync=False), 1, dev))
        assert km.size() == HELD and bool((out == torch.arange(HELD - BATCH, HELD, device=dev)).all())
        for b in (13, 14, 15):
            rate["insert_new"] = report("insert_new", new_ms[b], held=b * BATCH, slots=km.slots)
        hit, miss = pick(0, HELD), pick(HELD, 2 * HELD)
        for op, fn in (("lookup_hit", lambda: km.lookup(hit, out=out, sync=False)),
                       ("lookup_miss", lambda: km.lookup(miss, out=out, sync=False)),
                       ("insert_present", lambda: km.insert(hit, out=out, sync=False))):
            timed(fn, 5, dev)
            rate[op] = report(op, timed(fn, REPS, dev), held=HELD, slots=km.slots)
        km.sync()
    with PartialVector(RangePartition(0, 0, HELD), "long", 0) as vec:
        keys = torch.randint(0, HELD, (BATCH,), device=dev)
        fn = lambda: vec.get(keys, out=out, sync=False)  # noqa: E731
        timed(fn, 5, dev)
        rate["gather"] = report("gather", timed(fn, REPS, dev), held=HELD)
        vec.sync()
    print(json.dumps({"op": "ratio_to_gather", **{k: round(rate["gather"] / v, 2) for k, v in rate.items()}}))


if __name__ == "__main__":
    main()
