"""Build libcfnerf_hip.so (gfx950 only) in-tree with hipcc.  No CPU fallback is produced."""
import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "libcfnerf_hip.so")
CONSUMER = os.path.join(OBJ, "abi_consumer")
HOOKS = os.path.join(OBJ, "libcfnerf_testhooks.so")        # TEST artefact (tests/cfnerf_debug.h); the product never loads it
SOURCES = ["cfnerf_fwd.hip", "cfnerf_bwd.hip", "cfnerf_tail.hip", "cfnerf_inputgrad.hip", "cfnerf_raygrad.hip", "cfnerf_cull.hip", "cfnerf_abi.hip", "cfnerf_rayreg.hip", "cfnerf_kscores.hip", "cfnerf_ssim.hip"]
# per-file flags: the flow-adjoint kernels are long straight-line scalar code that the SLP vectoriser makes slower (cfnerf_tail.hip)
EXTRA_FLAGS = {"cfnerf_tail.hip": ["-fno-slp-vectorize"]}
# -ffp-contract=off: the sampling / encoding arithmetic must round like the reference's separate
# torch ops (an fma in pts = o + d*z moves sin(2^9 x) by ~3e-5); MFMA code is unaffected.
# -fvisibility=hidden + the linker version script: the dynamic symbol table holds the CFNERF_API entry points of include/cfnerf.h and
# nothing else (tests/test_abi_cpu.py compares `nm -D` with the header).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fvisibility=hidden", "-Wno-unused-result", "-Wno-unused-value"]


def _hipcc():
    for c in (os.environ.get("HIPCC"), shutil.which("hipcc"), "/opt/rocm/bin/hipcc"):
        if c and os.path.exists(c):
            return c
    raise RuntimeError("hipcc not found: the CF-NeRF hot path needs the ROCm toolchain to build")


def _newer(target, deps):
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force=False, verbose=False):
    os.makedirs(OBJ, exist_ok=True)
    hipcc = _hipcc()
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers.append(os.path.join(os.path.dirname(HERE), "include", "cfnerf.h"))
    headers.append(os.path.join(CSRC, "cfnerf_exports.map"))
    jobs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        if force or _newer(o, [s] + headers):
            jobs.append([hipcc, *FLAGS, *EXTRA_FLAGS.get(src, []), "-c", s, "-o", o])
    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        r = subprocess.run(cmd, capture_output=True, text=True)
        if r.returncode != 0:
            raise RuntimeError("hipcc failed:\n" + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    with ThreadPoolExecutor(max_workers=4) as ex:
        list(ex.map(run, jobs))
    objs = [os.path.join(OBJ, s.replace(".hip", ".o")) for s in SOURCES]
    if force or jobs or _newer(LIB, objs):
        run([hipcc, "--offload-arch=gfx950", "-shared", "-fPIC", "-Wl,--version-script=" + os.path.join(CSRC, "cfnerf_exports.map"), "-o", LIB, *objs])
    # the plain-C consumer of the ABI and the test-hooks library are TEST artefacts: their builds must never fail the library's (a box
    # without the C HIP headers, another ROCm layout); the tests that need them report a missing file themselves
    for what, fn in (("tests/abi_consumer.c", build_consumer), ("tests/csrc/cfnerf_testhooks.hip", build_test_hooks)):
        try:
            fn(force=force, verbose=verbose)
        except Exception as e:                      # noqa: BLE001
            print(f"cf-nerf_amd/build.py: warning: {what} was not built ({str(e).splitlines()[0]})", file=sys.stderr)
    return LIB


def build_test_hooks(force=False, verbose=False):
    """tests/csrc/cfnerf_testhooks.hip -> cf-nerf_amd/build/libcfnerf_testhooks.so: the six cfnerf_debug_* hooks of tests/cfnerf_debug.h,
    compiled against the library's internal headers (header-only host planners + the layout of the opaque handle).  Not linked against
    libcfnerf_hip.so and never loaded by the product."""
    root = os.path.dirname(HERE)
    src = os.path.join(root, "tests", "csrc", "cfnerf_testhooks.hip")
    if not os.path.exists(src):
        raise RuntimeError("no tests/csrc/cfnerf_testhooks.hip")
    headers = [os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")]
    headers += [os.path.join(root, "include", "cfnerf.h"), os.path.join(root, "tests", "cfnerf_debug.h")]
    if not (force or _newer(HOOKS, [src] + headers)):
        return HOOKS
    os.makedirs(OBJ, exist_ok=True)
    cmd = [_hipcc(), *FLAGS, "-I" + CSRC, "-I" + os.path.join(root, "include"), "-shared", src, "-o", HOOKS]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("test-hooks build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return HOOKS


def build_consumer(force=False, verbose=False):
    """tests/abi_consumer.c: gcc -std=c99 over include/cfnerf.h + the HIP runtime's C API -> cf-nerf_amd/build/abi_consumer"""
    root = os.path.dirname(HERE)
    csrc = os.path.join(root, "tests", "abi_consumer.c")
    cc = shutil.which("gcc") or shutil.which("cc")
    if not cc or not os.path.exists(csrc):
        raise RuntimeError("no C compiler or no tests/abi_consumer.c")
    if not (force or _newer(CONSUMER, [csrc, os.path.join(root, "include", "cfnerf.h"), LIB])):
        return CONSUMER
    os.makedirs(OBJ, exist_ok=True)
    rocm = os.path.dirname(os.path.dirname(os.path.realpath(_hipcc())))
    cmd = [cc, "-std=c99", "-O1", "-Wall", "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(root, "include"), "-I" + os.path.join(rocm, "include"), csrc,
           "-o", CONSUMER, "-L" + HERE, "-lcfnerf_hip", "-L" + os.path.join(rocm, "lib"), "-lamdhip64", "-lm",
           "-Wl,-rpath,$ORIGIN/..", "-Wl,-rpath," + os.path.join(rocm, "lib")]
    if verbose:
        print(" ".join(cmd), flush=True)
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0:
        raise RuntimeError("C consumer build failed: " + " ".join(cmd) + "\n" + r.stdout + r.stderr)
    return CONSUMER


if __name__ == "__main__":
    print(build(force="--force" in sys.argv, verbose=True))
