"""Kernel time of the grouped row-dot pull at one batch width, beside the row dot pull with one vector:
what DESIGN.md's choice of kGdotBatch (glint_rowdot.hip) rests on.

    GLINT_GPU_LIB=path/to/libglint_gpu.so python tools/gdot_batch_sweep.py LABEL >> profiles/wbag/gdot_sweep.jsonl

The width is a compile-time constant, so a sweep is one run per library: compile glint_rowdot.hip with
-DGLINT_GDOT_BATCH=B, link it with the other objects of build/obj into a library of its own and name that
with GLINT_GPU_LIB; LABEL (say B16) goes into every line. cfg5's per-GPU 2^17 x 512 Double shard, uniform
values, Zipf(1.0) rows, n = 2^8, 2^11, 2^14 and 2^16 records in groups of 1, 16 and 128, one standard-normal
vector per group. Both kernels by their prof id (GLINT_K_PULL_ROWS_DOT), mean of 10 launches after a
warm-up. One JSON line per (n, group length) on stdout."""
import ctypes as C
import json
import sys
from pathlib import Path

sys.path.insert(0, str(Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import glint_amd  # noqa: E402
from glint_amd import _native as N  # noqa: E402


def main():
    label = sys.argv[1] if len(sys.argv) > 1 else "default"
    dev = torch.device("cuda", 0)
    lib = N.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    shard_rows, cols = 1 << 17, 512
    msh = glint_amd.PartialMatrix(glint_amd.RangePartition(0, 0, shard_rows), cols, "double", 0)
    h = msh.handle
    msh.initUniform(7, -0.5, 0.5)
    rng = np.random.default_rng(42)

    def prof(fn, reps=10):
        fn()
        torch.cuda.synchronize()
        lib.glint_prof_reset(h)
        lib.glint_prof_enable(h, 1)
        for _ in range(reps):
            fn()
        torch.cuda.synchronize()
        ms, cnt = C.c_double(), C.c_int64()
        lib.glint_prof_read(h, N.GLINT_K_PULL_ROWS_DOT, C.byref(ms), C.byref(cnt))
        lib.glint_prof_enable(h, 0)
        assert cnt.value == reps
        return ms.value / reps

    for n in (1 << 8, 1 << 11, 1 << 14, 1 << 16):
        # Zipf(1.0) ranks through a seeded permutation (measure_paths.zipf_keys)
        ranks = np.minimum(np.floor(np.power(float(shard_rows), rng.random(n))).astype(np.int64) - 1, shard_rows - 1)
        rows = rng.permutation(shard_rows)[ranks].astype(np.int64)
        d_rows = torch.from_numpy(rows).to(dev)
        for glen in (1, 16, 128):
            g = n // glen
            d_off = torch.arange(g + 1, dtype=torch.int64, device=dev) * glen
            d_x = torch.randn((g, cols), dtype=torch.float64, device=dev)
            d_out = torch.empty(n, dtype=torch.float64, device=dev)
            k_gdot = prof(lambda: lib.glint_mat_pull_rows_gdot_dev(h, d_rows.data_ptr(), n, d_off.data_ptr(), g,
                                                                   d_x.data_ptr(), d_out.data_ptr(), stream))
            k_dot1 = prof(lambda: lib.glint_mat_pull_rows_dot_dev(h, d_rows.data_ptr(), n, d_x.data_ptr(), 1,
                                                                  d_out.data_ptr(), stream))
            print(json.dumps(dict(lib=label, rows=n, group_len=glen, gdot_kernel_ms=k_gdot, dot1_kernel_ms=k_dot1,
                                  ratio=k_gdot / k_dot1)), flush=True)
    msh.sync(stream)
    msh.destroy()


if __name__ == "__main__":
    main()
