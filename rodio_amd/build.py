"""Builds librodio_hip.so (gfx950 only) in-tree with hipcc.

    python rodio_amd/build.py [--force]      (run by path: importing the package needs the .so)

hipcc cross-compiles without a GPU.  The .so is git-ignored but travels to the GPU box with
the gpurun snapshot.
"""
from __future__ import annotations

import os
import shutil
import subprocess
import sys
from concurrent.futures import ThreadPoolExecutor

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(HERE, "csrc")
OBJ = os.path.join(HERE, "build")
LIB = os.path.join(HERE, "librodio_hip.so")
SOURCES = ["rh_runtime.hip", "rh_elementwise.hip", "rh_resample.hip", "rh_recurrence.hip", "rh_limit.hip", "rh_agc.hip", "rh_biquad_scan.hip", "rh_stream.hip", "rh_uniform.hip", "rh_widemix.hip", "rh_formats.hip", "rh_wav.hip", "rh_comm.hip", "rh_pipeline.hip", "rh_pipeline_plan.hip", "rh_pipeline_stream.hip", "rh_pipeline_sblk.hip", "rh_live.hip", "rh_generators.hip", "rh_noise.hip", "rh_mix2.hip"]
# -ffp-contract=off: the reference's f32 expressions (lerp, biquad, mixer sum) must not be
# fused; kernels that want an FMA spell it __builtin_fmaf.
# -fno-slp-vectorize: hipcc's SLP pass pairs the two stereo channels into v_pk_*_f32; on gfx950
# that costs more v_mov shuffling and VGPRs than it saves (measured: fused kernel 1.25 -> 0.89 ms).
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-fPIC", "-ffp-contract=off", "-fno-fast-math",
         "-fno-slp-vectorize", "-Wall", "-Wno-unused-function"] + os.environ.get("RH_EXTRA_HIPCC_FLAGS", "").split()


def hipcc() -> str:
    for cand in (os.environ.get("HIPCC"), "/opt/rocm/bin/hipcc", shutil.which("hipcc")):
        if cand and os.path.exists(cand):
            return cand
    raise RuntimeError("hipcc not found: librodio_hip.so cannot be built (there is no CPU fallback)")


def _stale(target: str, deps) -> bool:
    if not os.path.exists(target):
        return True
    t = os.path.getmtime(target)
    return any(os.path.getmtime(d) > t for d in deps)


def build(force: bool = False, verbose: bool = True) -> str:
    os.makedirs(OBJ, exist_ok=True)
    # every header: one that is left out here means a stale .so wherever the tree is built next
    headers = sorted(os.path.join(CSRC, f) for f in os.listdir(CSRC) if f.endswith(".h")) + [os.path.join(HERE, "..", "include", "rodio_hip.h")]
    cc = hipcc()
    jobs = []
    objs = []
    for src in SOURCES:
        s = os.path.join(CSRC, src)
        o = os.path.join(OBJ, src.replace(".hip", ".o"))
        objs.append(o)
        if force or _stale(o, [s] + headers):
            jobs.append([cc, *FLAGS, "-c", s, "-o", o])

    def run(cmd):
        if verbose:
            print(" ".join(cmd), flush=True)
        subprocess.check_call(cmd)

    with ThreadPoolExecutor(max_workers=min(len(jobs), os.cpu_count() or 4) or 1) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, "-ldl"])
    build_host_mirror_test(force, run)
    build_live_test(force, run)
    build_generators_test(force, run)
    build_noise_test(force, run)
    build_mix_test(force, run)
    build_scan_launch_test(force, run)
    build_wide_filtered_test(force, run)
    return LIB


def build_host_mirror_test(force: bool, run) -> str:
    """The C++ host mirror (include/rodio_hip.hpp) is header-only; its test driver is a plain g++ program over
    the C ABI -- no HIP headers, the way a host application links the library."""
    root = os.path.join(HERE, "..")
    src = os.path.join(root, "tests", "cpp", "host_mirror_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "host_mirror_test")
    deps = [src, os.path.join(root, "include", "rodio_hip.hpp"), os.path.join(root, "include", "rodio_hip.h"), LIB]
    if force or _stale(exe, deps):
        run([shutil.which("g++") or "g++", "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-I", os.path.join(root, "include"), src, "-L", HERE, "-lrodio_hip",
             "-Wl,-rpath,$ORIGIN/../../rodio_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    # ... and the same driver over tests/cpp/fake_device.cpp (a CPU stand-in for the library: TEST INFRASTRUCTURE, it lets the host logic of the
    # header run in the `-m "not gpu"` suite; nothing of the product links or loads it)
    fakes = _fakes(root)
    fake_exe = os.path.join(root, "tests", "cpp", "host_mirror_test_fake")
    if force or _stale(fake_exe, [src, *fakes, deps[1], deps[2]]):
        run([shutil.which("g++") or "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", os.path.join(root, "include"), src, *fakes, "-o", fake_exe])
    return exe


def _fakes(root: str, *more: str):
    """The CPU stand-ins every *_fake driver links: the header-only mirror names rh_wide_mix_block_filtered (fake_widemix_filtered.cpp) wherever
    GpuMixer is instantiated, beside the entries of fake_device.cpp."""
    return [os.path.join(root, "tests", "cpp", f) for f in ("fake_device.cpp", "fake_widemix_filtered.cpp", *more)]


def build_wide_filtered_test(force: bool, run) -> str:
    """tests/cpp/wide_filtered_test.cpp: GpuMixer's filtered wide generations (Options::wide_filters) against the library
    (wide_filtered_test) and over the CPU stand-ins (wide_filtered_test_fake).  TEST INFRASTRUCTURE: plain g++."""
    root = os.path.join(HERE, "..")
    inc = os.path.join(root, "include")
    src = os.path.join(root, "tests", "cpp", "wide_filtered_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "wide_filtered_test")
    if not os.path.exists(src):  # (as build_scan_launch_test: an older suite on this library still builds)
        return exe
    hdrs = [os.path.join(inc, "rodio_hip.hpp"), os.path.join(inc, "rodio_hip.h")]
    gxx = shutil.which("g++") or "g++"
    if force or _stale(exe, [src, LIB] + hdrs):
        run([gxx, "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-I", inc, src, "-L", HERE, "-lrodio_hip",
             "-Wl,-rpath,$ORIGIN/../../rodio_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    fakes = _fakes(root)
    fexe = os.path.join(root, "tests", "cpp", "wide_filtered_test_fake")
    if force or _stale(fexe, [src, *fakes] + hdrs):
        run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", inc, src, *fakes, "-o", fexe])
    return exe


def build_live_test(force: bool, run) -> str:
    """tests/cpp/live_test.cpp (chains with adjustable stages and periodic_access) against the library, and against
    tests/cpp/fake_device.cpp + tests/cpp/fake_live.cpp (TEST INFRASTRUCTURE: the CPU stand-in, for the `-m "not gpu"` suite)."""
    root = os.path.join(HERE, "..")
    inc = os.path.join(root, "include")
    src = os.path.join(root, "tests", "cpp", "live_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "live_test")
    hdrs = [os.path.join(inc, "rodio_hip.hpp"), os.path.join(inc, "rodio_hip.h")]
    gxx = shutil.which("g++") or "g++"
    if force or _stale(exe, [src, LIB] + hdrs):
        run([gxx, "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-I", inc, src, "-L", HERE, "-lrodio_hip",
             "-Wl,-rpath,$ORIGIN/../../rodio_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    fakes = _fakes(root, "fake_live.cpp")
    fake_exe = os.path.join(root, "tests", "cpp", "live_test_fake")
    if force or _stale(fake_exe, [src] + fakes + hdrs):
        run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", inc, src, *fakes, "-o", fake_exe])
    return exe


def build_generators_test(force: bool, run) -> str:
    """tests/cpp/generators_test.cpp: the host build of the phase walk (csrc/rh_generators.h) against brute-force stepping, and the
    serial f32 phases the GPU tests compare the generator kernels with (TEST INFRASTRUCTURE: plain g++, no library)."""
    root = os.path.join(HERE, "..")
    src = os.path.join(root, "tests", "cpp", "generators_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "generators_test")
    if force or _stale(exe, [src, os.path.join(CSRC, "rh_generators.h")]):
        run([shutil.which("g++") or "g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wall", "-Wextra", "-I", CSRC, src, "-o", exe])
    # the C++ mirror's generators (include/rodio_hip.hpp) against the library, and against the CPU stand-in (fake_device.cpp + fake_generators.cpp)
    inc = os.path.join(root, "include")
    msrc = os.path.join(root, "tests", "cpp", "generators_mirror_test.cpp")
    mexe = os.path.join(root, "tests", "cpp", "generators_mirror_test")
    hdrs = [os.path.join(inc, "rodio_hip.hpp"), os.path.join(inc, "rodio_hip.h"), os.path.join(CSRC, "rh_generators.h")]
    gxx = shutil.which("g++") or "g++"
    if force or _stale(mexe, [msrc, LIB] + hdrs):
        run([gxx, "-std=c++17", "-O2", "-pthread", "-Wall", "-Wextra", "-I", inc, msrc, "-L", HERE, "-lrodio_hip",
             "-Wl,-rpath,$ORIGIN/../../rodio_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-o", mexe])
    fakes = _fakes(root, "fake_generators.cpp")
    fexe = os.path.join(root, "tests", "cpp", "generators_mirror_test_fake")
    if force or _stale(fexe, [msrc] + fakes + hdrs):
        run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", inc, "-I", CSRC, msrc, *fakes, "-o", fexe])
    return exe


def build_noise_test(force: bool, run) -> str:
    """tests/cpp/noise_mirror_test.cpp: the C++ mirror's noise sources (include/rodio_hip.hpp) against the library (noise_mirror_test), and
    against the CPU stand-in of rh_noise_init / rh_noise_generate (fake_device.cpp + fake_noise.cpp: noise_mirror_test_fake).  TEST
    INFRASTRUCTURE: plain g++."""
    root = os.path.join(HERE, "..")
    inc = os.path.join(root, "include")
    msrc = os.path.join(root, "tests", "cpp", "noise_mirror_test.cpp")
    mexe = os.path.join(root, "tests", "cpp", "noise_mirror_test")
    hdrs = [os.path.join(inc, "rodio_hip.hpp"), os.path.join(inc, "rodio_hip.h"), os.path.join(CSRC, "rh_noise.h")]
    gxx = shutil.which("g++") or "g++"
    if force or _stale(mexe, [msrc, LIB] + hdrs):
        run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", inc, msrc, "-L", HERE, "-lrodio_hip",
             "-Wl,-rpath,$ORIGIN/../../rodio_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-o", mexe])
    fakes = _fakes(root, "fake_noise.cpp")
    fexe = os.path.join(root, "tests", "cpp", "noise_mirror_test_fake")
    if force or _stale(fexe, [msrc] + fakes + hdrs):
        run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", inc, "-I", CSRC, msrc, *fakes, "-o", fexe])
    return mexe


def build_mix_test(force: bool, run) -> str:
    """tests/cpp/mix_mirror_test.cpp: the C++ mirror's Mix and Crossfade (include/rodio_hip.hpp) against the library (mix_mirror_test), and
    against the CPU stand-ins (fake_device.cpp + fake_generators.cpp + fake_noise.cpp + fake_mix.cpp: mix_mirror_test_fake).  TEST
    INFRASTRUCTURE: plain g++."""
    root = os.path.join(HERE, "..")
    inc = os.path.join(root, "include")
    msrc = os.path.join(root, "tests", "cpp", "mix_mirror_test.cpp")
    mexe = os.path.join(root, "tests", "cpp", "mix_mirror_test")
    hdrs = [os.path.join(inc, "rodio_hip.hpp"), os.path.join(inc, "rodio_hip.h"), os.path.join(CSRC, "rh_noise.h"), os.path.join(CSRC, "rh_generators.h")]
    gxx = shutil.which("g++") or "g++"
    if force or _stale(mexe, [msrc, LIB] + hdrs):
        run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", inc, msrc, "-L", HERE, "-lrodio_hip",
             "-Wl,-rpath,$ORIGIN/../../rodio_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-o", mexe])
    fakes = _fakes(root, "fake_generators.cpp", "fake_noise.cpp", "fake_mix.cpp")
    fexe = os.path.join(root, "tests", "cpp", "mix_mirror_test_fake")
    if force or _stale(fexe, [msrc] + fakes + hdrs):
        run([gxx, "-std=c++17", "-O2", "-ffp-contract=off", "-pthread", "-Wall", "-Wextra", "-I", inc, "-I", CSRC, msrc, *fakes, "-o", fexe])
    return mexe


def build_scan_launch_test(force: bool, run) -> str:
    """tests/cpp/scan_launch_test.cpp: the scan kernels' host protocol (csrc/rh_scan_launch.h: variant pick, scratch layout, the launch that needs no
    initialisation in front of it, table rotation, ticket base) against a model of the device (TEST INFRASTRUCTURE: plain g++, no library)."""
    root = os.path.join(HERE, "..")
    src = os.path.join(root, "tests", "cpp", "scan_launch_test.cpp")
    exe = os.path.join(root, "tests", "cpp", "scan_launch_test")
    if not os.path.exists(src):  # the library does not need the driver: a tree whose tests/ lacks it (an older suite run on this library) still builds
        return exe
    if force or _stale(exe, [src, os.path.join(CSRC, "rh_scan_launch.h")]):
        run([shutil.which("g++") or "g++", "-std=c++17", "-O2", "-Wall", "-Wextra", "-I", CSRC, src, "-o", exe])
    return exe


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
