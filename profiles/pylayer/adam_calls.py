#!/usr/bin/env python3
"""Wall time of back-to-back PartialMatrix.updateRowsAdam calls on device tensors: n = 1, cols = 4, sync=False,
one sync at the end -- the call that pays the Python layer's per-call cost and next to nothing else.

    python profiles/pylayer/adam_calls.py [--tree DIR] [--calls 10000] [--rounds 5]

``--tree`` names the checkout whose glint_amd is imported (default: this one), so one visit can alternate two
commits. Prints one JSON line: per round, microseconds per call until the last call returned (``enqueue_us``)
and until the final sync returned (``synced_us``)."""
import argparse
import json
import sys
import time
from pathlib import Path

ap = argparse.ArgumentParser()
ap.add_argument("--tree", default=str(Path(__file__).resolve().parents[2]))
ap.add_argument("--calls", type=int, default=10000)
ap.add_argument("--rounds", type=int, default=5)
args = ap.parse_args()
sys.path.insert(0, str(Path(args.tree).resolve()))

import torch  # noqa: E402
from glint_amd import PartialMatrix, RangePartition  # noqa: E402

dev = torch.device("cuda", 0)
enqueue, synced = [], []
with PartialMatrix(RangePartition(0, 0, 8), 4, "float", device=0) as w, \
        PartialMatrix(RangePartition(0, 0, 8), 8, "float", device=0) as state:
    rows = torch.tensor([3], dtype=torch.int64, device=dev)
    grads = torch.full((1, 4), 0.5, dtype=torch.float32, device=dev)
    for _ in range(1000):  # warm-up
        w.updateRowsAdam(state, rows, grads, 0.01, 1, sync=False)
    w.sync(w._stream_of(rows))
    for _ in range(args.rounds):
        t0 = time.perf_counter()
        for step in range(1, args.calls + 1):
            w.updateRowsAdam(state, rows, grads, 0.01, step, sync=False)
        t1 = time.perf_counter()
        w.sync(w._stream_of(rows))
        t2 = time.perf_counter()
        enqueue.append(round((t1 - t0) / args.calls * 1e6, 3))
        synced.append(round((t2 - t0) / args.calls * 1e6, 3))
print(json.dumps({"tree": args.tree, "calls": args.calls, "enqueue_us": enqueue, "synced_us": synced}), flush=True)
