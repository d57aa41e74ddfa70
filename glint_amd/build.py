"""Builds the in-tree native libraries.

* ``glint_amd/lib/libglint_gpu.so`` -- the product: HIP kernels + C ABI (include/glint_gpu.h),
  compiled for gfx950 only. hipcc cross-compiles it without a GPU.
* ``oracle/build/libglint_oracle.so`` -- the CPU restatement used by tests as the parity checker
  (never linked into the product).

Outputs stay in-tree so they travel to the GPU box with the repository snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent
PKG = ROOT / "glint_amd"
LIB_DIR = PKG / "lib"
LIB = LIB_DIR / "libglint_gpu.so"
ORACLE_DIR = ROOT / "oracle"
ORACLE_LIB = ORACLE_DIR / "build" / "libglint_oracle.so"

CSRC = PKG / "csrc"
HIP_SOURCES = [CSRC / "glint_gpu.hip", CSRC / "glint_sort.hip", CSRC / "glint_route.hip", CSRC / "glint_ordered.hip", CSRC / "glint_bin.hip",
               CSRC / "glint_exchange.hip", CSRC / "glint_rows.hip", CSRC / "glint_sparse.hip",
               CSRC / "glint_rowsum.hip", CSRC / "glint_rowdot.hip", CSRC / "glint_rowaxpy.hip",
               CSRC / "glint_topk.hip", CSRC / "glint_rowadagrad.hip", CSRC / "glint_pairs.hip",
               CSRC / "glint_init.hip", CSRC / "glint_rowgroup.hip", CSRC / "glint_rowadam.hip",
               CSRC / "glint_rowwire.hip", CSRC / "glint_sample.hip", CSRC / "glint_rowadagrad_rowwise.hip",
               CSRC / "glint_rowftrl.hip"]
# plain C++: the push planners, the top-k pull's level plan, the uniform init's value contract, the
# narrow-format row transport's conversion contract and the row sampler's value contract
PLAN_HEADERS = [CSRC / "glint_push_plan.h", CSRC / "glint_bin_plan.h", CSRC / "glint_topk_plan.h",
                CSRC / "glint_init_plan.h", CSRC / "glint_wire_plan.h", CSRC / "glint_sample_plan.h"]
HIP_HEADERS = [CSRC / "glint_kernels.h", CSRC / "glint_device.h", CSRC / "glint_host.h", CSRC / "glint_dot.h",
               CSRC / "glint_axpy.h", CSRC / "glint_group.h", CSRC / "glint_rowstep.h",
               ROOT / "include" / "glint_gpu.h", *PLAN_HEADERS]
HIP_DEPS = HIP_SOURCES + HIP_HEADERS
OBJ_DIR = ROOT / "build" / "obj"
ORACLE_SOURCES = [ORACLE_DIR / "glint_oracle.c"]
LOOPBACK_SRC = ROOT / "tools" / "loopback" / "glint_loopback.c"
LOOPBACK_BIN = ROOT / "tools" / "loopback" / "build" / "glint_loopback"


def _hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and Path(cand).exists():
            return cand
    raise RuntimeError("hipcc not found: the glint_amd native library cannot be built")


def _stale(out: Path, deps) -> bool:
    if not out.exists():
        return True
    t = out.stat().st_mtime
    return any(Path(d).stat().st_mtime > t for d in deps)


def build_gpu_lib(force: bool = False, verbose: bool = False) -> Path:
    """Compile libglint_gpu.so for gfx950 (no other target): one object per source, rebuilt when
    it or a header changed (sources compile in parallel), then one link. No library beyond the HIP
    runtime is linked: every sort, scan and partition is hand-written."""
    if not force and not _stale(LIB, HIP_DEPS):
        return LIB
    OBJ_DIR.mkdir(parents=True, exist_ok=True)
    LIB_DIR.mkdir(parents=True, exist_ok=True)
    flags = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-Wall", "-Wno-unused-result"]
    objs, procs = [], []
    for src in HIP_SOURCES:
        obj = OBJ_DIR / (src.stem + ".o")
        objs.append(obj)
        if force or _stale(obj, [src] + HIP_HEADERS):
            cmd = [_hipcc(), *flags, "-c", "-o", str(obj) + ".tmp", str(src)]
            if verbose:
                print(" ".join(cmd), file=sys.stderr)
            procs.append((subprocess.Popen(cmd, cwd=str(ROOT)), obj))
    for p, obj in procs:  # sources compile in parallel
        if p.wait() != 0:
            raise subprocess.CalledProcessError(p.returncode, f"hipcc -c {obj.name}")
        os.replace(str(obj) + ".tmp", obj)
    tmp = LIB.with_suffix(".so.tmp")
    cmd = [_hipcc(), "--offload-arch=gfx950", "-shared", "-fPIC", "-o", str(tmp), *map(str, objs)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, LIB)
    return LIB


def build_oracle(force: bool = False, verbose: bool = False) -> Path:
    """Compile the CPU restatement (test infrastructure) with gcc."""
    if not force and not _stale(ORACLE_LIB, ORACLE_SOURCES):
        return ORACLE_LIB
    ORACLE_LIB.parent.mkdir(parents=True, exist_ok=True)
    tmp = ORACLE_LIB.with_suffix(".so.tmp")
    cc = shutil.which("gcc") or "cc"
    cmd = [cc, "-O2", "-std=c11", "-fPIC", "-shared", "-fwrapv", "-pthread", "-o", str(tmp),
           *map(str, ORACLE_SOURCES)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, ORACLE_LIB)
    return ORACLE_LIB


def build_loopback(force: bool = False, verbose: bool = False) -> Path:
    """The loopback-TCP client/server harness (BASELINE.json configs[0]); it dlopens its shard
    backend at run time and links neither library."""
    if not force and not _stale(LOOPBACK_BIN, [LOOPBACK_SRC]):
        return LOOPBACK_BIN
    LOOPBACK_BIN.parent.mkdir(parents=True, exist_ok=True)
    tmp = LOOPBACK_BIN.with_suffix(".tmp")
    cc = shutil.which("gcc") or "cc"
    cmd = [cc, "-O2", "-std=c11", "-Wall", "-pthread", "-o", str(tmp), str(LOOPBACK_SRC), "-ldl", "-lm"]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, LOOPBACK_BIN)
    return LOOPBACK_BIN


JNI_SHIM = ROOT / "integration" / "jni" / "glint_jni.c"
JNI_DRIVER_SRC = ROOT / "tests" / "c" / "fake_jvm.c"
JNI_DRIVER = ROOT / "tests" / "c" / "build" / "fake_jvm"


def build_jni_driver(force: bool = False, verbose: bool = False) -> Path:
    """The JNI shim (integration/jni/glint_jni.c) compiled against tests/c/jni.h -- a minimal JNI
    environment -- and linked with a driver that calls its native methods as the actors do. This is
    the shim's compile check (there is no JDK in the image) and, on a GPU, its end-to-end test."""
    deps = [JNI_SHIM, JNI_DRIVER_SRC, ROOT / "tests" / "c" / "jni.h", ROOT / "include" / "glint_gpu.h", LIB]
    if not force and not _stale(JNI_DRIVER, deps):
        return JNI_DRIVER
    JNI_DRIVER.parent.mkdir(parents=True, exist_ok=True)
    tmp = JNI_DRIVER.with_suffix(".tmp")
    cc = shutil.which("gcc") or "cc"
    cmd = [cc, "-O2", "-Wall", "-Werror", "-std=c11", "-I", str(ROOT / "tests" / "c"), "-I", str(ROOT / "include"),
           str(JNI_DRIVER_SRC), str(JNI_SHIM), "-L", str(LIB_DIR), "-lglint_gpu", f"-Wl,-rpath,{LIB_DIR}",
           "-o", str(tmp)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, JNI_DRIVER)
    return JNI_DRIVER


PLAN_PROBE_SRC = ROOT / "tests" / "c" / "plan_probe.cpp"
PLAN_PROBE = ROOT / "tests" / "c" / "build" / "libplan_probe.so"


def build_plan_probe(force: bool = False, verbose: bool = False) -> Path:
    """The push planners (glint_push_plan.h, glint_bin_plan.h) as a host-only library of C wrappers:
    what tests/test_plan_cpu.py loads. g++ alone compiles it, which is also the check that the two
    headers need nothing of HIP."""
    deps = [PLAN_PROBE_SRC, *PLAN_HEADERS, ROOT / "include" / "glint_gpu.h"]
    if not force and not _stale(PLAN_PROBE, deps):
        return PLAN_PROBE
    PLAN_PROBE.parent.mkdir(parents=True, exist_ok=True)
    tmp = PLAN_PROBE.with_suffix(".so.tmp")
    cxx = shutil.which("g++") or "c++"
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(tmp), str(PLAN_PROBE_SRC)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, PLAN_PROBE)
    return PLAN_PROBE


SWEEP_PROBE_SRC = ROOT / "tests" / "c" / "sweep_probe.cpp"
SWEEP_PROBE = ROOT / "tests" / "c" / "build" / "libsweep_probe.so"


def build_sweep_probe(force: bool = False, verbose: bool = False) -> Path:
    """The affine sweep's ticket arithmetic (glint_push_plan.h sweep_ticket_count, sweep_ticket) as a
    host-only library: what tests/test_sweep_tickets_cpu.py loads. Compiled by g++ alone."""
    deps = [SWEEP_PROBE_SRC, *PLAN_HEADERS, ROOT / "include" / "glint_gpu.h"]
    if not force and not _stale(SWEEP_PROBE, deps):
        return SWEEP_PROBE
    SWEEP_PROBE.parent.mkdir(parents=True, exist_ok=True)
    tmp = SWEEP_PROBE.with_suffix(".so.tmp")
    cxx = shutil.which("g++") or "c++"
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(tmp), str(SWEEP_PROBE_SRC)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, SWEEP_PROBE)
    return SWEEP_PROBE


TOPK_PROBE_SRC = ROOT / "tests" / "c" / "topk_probe.cpp"
TOPK_PROBE = ROOT / "tests" / "c" / "build" / "libtopk_probe.so"


def build_topk_probe(force: bool = False, verbose: bool = False) -> Path:
    """The top-k pull's level plan (glint_topk_plan.h) as a host-only library: what
    tests/test_topk_cpu.py loads. Compiled by g++ alone."""
    deps = [TOPK_PROBE_SRC, *PLAN_HEADERS, ROOT / "include" / "glint_gpu.h"]
    if not force and not _stale(TOPK_PROBE, deps):
        return TOPK_PROBE
    TOPK_PROBE.parent.mkdir(parents=True, exist_ok=True)
    tmp = TOPK_PROBE.with_suffix(".so.tmp")
    cxx = shutil.which("g++") or "c++"
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(tmp), str(TOPK_PROBE_SRC)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, TOPK_PROBE)
    return TOPK_PROBE


INIT_PROBE_SRC = ROOT / "tests" / "c" / "init_probe.cpp"
INIT_PROBE = ROOT / "tests" / "c" / "build" / "libinit_probe.so"


def build_init_probe(force: bool = False, verbose: bool = False) -> Path:
    """The uniform init's value contract (glint_init_plan.h: Philox4x32-10 and the bits-to-value mapping)
    as a host-only library: what tests/test_init_cpu.py loads. Compiled by g++ alone, with contraction
    off as the contract asks (the header's clang pragma is unknown to g++)."""
    deps = [INIT_PROBE_SRC, CSRC / "glint_init_plan.h"]
    if not force and not _stale(INIT_PROBE, deps):
        return INIT_PROBE
    INIT_PROBE.parent.mkdir(parents=True, exist_ok=True)
    tmp = INIT_PROBE.with_suffix(".so.tmp")
    cxx = shutil.which("g++") or "c++"
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-ffp-contract=off", "-fPIC",
           "-shared", "-o", str(tmp), str(INIT_PROBE_SRC)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, INIT_PROBE)
    return INIT_PROBE


WIRE_PROBE_SRC = ROOT / "tests" / "c" / "wire_probe.cpp"
WIRE_PROBE = ROOT / "tests" / "c" / "build" / "libwire_probe.so"


def build_wire_probe(force: bool = False, verbose: bool = False) -> Path:
    """The narrow-format row transport's conversion contract (glint_wire_plan.h: the supported pairs and the
    integer narrowing and widening of each) as a host-only library: what tests/test_wire_cpu.py loads.
    Compiled by g++ alone."""
    deps = [WIRE_PROBE_SRC, CSRC / "glint_wire_plan.h"]
    if not force and not _stale(WIRE_PROBE, deps):
        return WIRE_PROBE
    WIRE_PROBE.parent.mkdir(parents=True, exist_ok=True)
    tmp = WIRE_PROBE.with_suffix(".so.tmp")
    cxx = shutil.which("g++") or "c++"
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-fPIC", "-shared", "-o", str(tmp), str(WIRE_PROBE_SRC)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, WIRE_PROBE)
    return WIRE_PROBE


SAMPLER_PROBE_SRC = ROOT / "tests" / "c" / "sampler_probe.cpp"
SAMPLER_PROBE = ROOT / "tests" / "c" / "build" / "libsampler_probe.so"


def build_sampler_probe(force: bool = False, verbose: bool = False) -> Path:
    """The row sampler's value contract (glint_sample_plan.h: the attempt, the search and the exclusion rule
    over a host cdf) as a host-only library: what tests/test_sampler_cpu.py loads. Compiled by g++ alone."""
    deps = [SAMPLER_PROBE_SRC, CSRC / "glint_sample_plan.h", CSRC / "glint_init_plan.h"]
    if not force and not _stale(SAMPLER_PROBE, deps):
        return SAMPLER_PROBE
    SAMPLER_PROBE.parent.mkdir(parents=True, exist_ok=True)
    tmp = SAMPLER_PROBE.with_suffix(".so.tmp")
    cxx = shutil.which("g++") or "c++"
    cmd = [cxx, "-O2", "-std=c++17", "-Wall", "-Werror", "-Wno-unknown-pragmas", "-fPIC", "-shared", "-o", str(tmp),
           str(SAMPLER_PROBE_SRC)]
    if verbose:
        print(" ".join(cmd), file=sys.stderr)
    subprocess.run(cmd, check=True, cwd=str(ROOT))
    os.replace(tmp, SAMPLER_PROBE)
    return SAMPLER_PROBE


def build_all(force: bool = False, verbose: bool = False) -> None:
    build_gpu_lib(force=force, verbose=verbose)
    build_oracle(force=force, verbose=verbose)
    build_loopback(force=force, verbose=verbose)
    build_jni_driver(force=force, verbose=verbose)
    build_plan_probe(force=force, verbose=verbose)
    build_sweep_probe(force=force, verbose=verbose)
    build_topk_probe(force=force, verbose=verbose)
    build_init_probe(force=force, verbose=verbose)
    build_wire_probe(force=force, verbose=verbose)
    build_sampler_probe(force=force, verbose=verbose)


if __name__ == "__main__":
    build_all(force="--force" in sys.argv, verbose=True)
    print(LIB)
    print(ORACLE_LIB)
    print(LOOPBACK_BIN)
