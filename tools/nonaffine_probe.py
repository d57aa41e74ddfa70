"""The tile path of push_apply, timed (tuning probe): an ordered but non-affine device push -- keys 2 i,
so every wave tile is increasing and none is affine -- of 2^LOG2 records into a shard of twice as many
keys. Prints the wall time per push over REPS back-to-back pushes and the summed push_check /
push_apply device times. GLINT_GPU_LIB selects another build of the library for a same-box A/B.

    python tools/nonaffine_probe.py [LOG2=28] [REPS=10]
"""
import ctypes as C
import sys
import time
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import torch  # noqa: E402
from glint_amd import _native as N  # noqa: E402
from glint_amd import PartialVector, RangePartition  # noqa: E402

LOG2 = int(sys.argv[1]) if len(sys.argv) > 1 else 28
REPS = int(sys.argv[2]) if len(sys.argv) > 2 else 10
n = 1 << LOG2
d = torch.device("cuda", 0)
with PartialVector(RangePartition(0, 0, 2 * n), "double", 0) as sh:
    keys = torch.arange(n, dtype=torch.int64, device=d) * 2
    vals = torch.ones(n, dtype=torch.float64, device=d)
    for _ in range(3):
        sh.update(keys, vals)
    lib = N.load()
    lib.glint_prof_reset(sh.handle)
    lib.glint_prof_enable(sh.handle, 1)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(REPS):
        sh.update(keys, vals, sync=False)
    torch.cuda.synchronize()
    wall = (time.perf_counter() - t0) / REPS * 1e3
    lib.glint_prof_enable(sh.handle, 0)
    sh.sync()
    out = {}
    for name, kid in (("push_check", N.GLINT_K_PUSH_CHECK), ("push_apply", N.GLINT_K_PUSH_APPLY)):
        ms, cnt = C.c_double(), C.c_int64()
        lib.glint_prof_read(sh.handle, kid, C.byref(ms), C.byref(cnt))
        out[name] = (ms.value / REPS, cnt.value // REPS)
    probe = torch.tensor([0, 2, 2 * n - 2, 1], dtype=torch.int64, device=d)
    got = sh.get(probe).tolist()
    assert got == [3.0 + REPS] * 3 + [0.0], got
    print(f"ordered non-affine 2^{LOG2}: {wall:.4f} ms per push, push_check {out['push_check'][0]:.4f} ms, "
          f"push_apply {out['push_apply'][0]:.4f} ms in {out['push_apply'][1]} launch(es)", flush=True)
