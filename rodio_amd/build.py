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
# (the units that take longest to compile come first: the pool never starts a long pole last)
SOURCES = ["rh_pipeline_wave.hip", "rh_limit.hip", "rh_pipeline_fast_hi.hip", "rh_pipeline_fast_lo.hip", "rh_pipeline_fast1.hip",
           "rh_runtime.hip", "rh_elementwise.hip", "rh_resample.hip", "rh_recurrence.hip", "rh_agc.hip", "rh_biquad_scan.hip", "rh_stream.hip", "rh_uniform.hip", "rh_widemix.hip", "rh_formats.hip", "rh_wav.hip", "rh_comm.hip", "rh_pipeline.hip", "rh_pipeline_chunk.hip", "rh_pipeline_mix.hip", "rh_pipeline_plan.hip", "rh_pipeline_stream.hip", "rh_pipeline_sblk.hip", "rh_live.hip", "rh_generators.hip", "rh_noise.hip", "rh_mix2.hip", "rh_spatialmix.hip", "rh_widebatch.hip", "rh_playermix.hip", "rh_loopmix.hip", "rh_queuemix.hip", "rh_clipmix.hip"]
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

    # MAX_JOBS, where it is set, says how many CPUs this build may use; a machine's own count can be many times that
    workers = int(os.environ.get("MAX_JOBS") or 0) or min(os.cpu_count() or 4, 16)
    with ThreadPoolExecutor(max_workers=min(len(jobs), workers) or 1) as ex:
        list(ex.map(run, jobs))
    if force or jobs or _stale(LIB, objs):
        run([cc, "--offload-arch=gfx950", "-shared", "-fPIC", "-o", LIB, *objs, "-ldl"])
    for name in DRIVERS:
        build_driver(name, force, run)
    return LIB


# The test drivers under tests/cpp (TEST INFRASTRUCTURE: plain g++ programs, nothing of the product links or loads them).  A driver over the C ABI
# or the header-only C++ mirror (include/rodio_hip.hpp) is built twice: against the library (`lib`: no HIP headers, the way a host application
# links it) and, as NAME_fake, over the CPU stand-ins tests/cpp/fake_device.cpp + fake_widemix_filtered.cpp + `fakes`, which let the host logic
# run in the `-m "not gpu"` suite (`fake`).  A driver with neither is a program over headers of csrc alone.
#   hdrs: headers of csrc the driver includes (the fake build and the csrc-only build get -I csrc);  fpc: -ffp-contract=off on the first build
#   (the fake build always has it: the stand-ins compute what the kernels compute, unfused)
DRIVERS = {
    "host_mirror_test": dict(lib=True, fake=True),
    "live_test": dict(lib=True, fake=True, fakes=["fake_live.cpp"]),
    "live_filter_test": dict(lib=True, fake=True, fakes=["fake_live.cpp", "fake_live_filter.cpp"]),  # live_low_pass / live_high_pass under periodic_access
    "generators_test": dict(hdrs=["rh_generators.h"], fpc=True),  # the phase walk against brute-force stepping, and the serial f32 phases
    "generators_mirror_test": dict(lib=True, fake=True, hdrs=["rh_generators.h"], fakes=["fake_generators.cpp"]),
    "noise_mirror_test": dict(lib=True, fake=True, fpc=True, hdrs=["rh_noise.h"], fakes=["fake_noise.cpp"]),
    "mix_mirror_test": dict(lib=True, fake=True, fpc=True, hdrs=["rh_noise.h", "rh_generators.h"], fakes=["fake_generators.cpp", "fake_noise.cpp", "fake_mix.cpp"]),
    "scan_launch_test": dict(hdrs=["rh_scan_launch.h"]),  # the scan kernels' host protocol against a model of the device
    "wide_filtered_test": dict(lib=True, fake=True),
    "rlm_launch_test": dict(hdrs=["rh_rlm_launch.h"]),  # the fused path's launch decisions: route, row cut, tickets, stream-block geometry
    "pcm16_launch_test": dict(hdrs=["rh_rlm_pcm16.h", "rh_rlm_launch.h"]),  # PCM16 sources: the rows themselves or a converted copy
    "wide_batch_plan_test": dict(hdrs=["rh_wide_batch_plan.h", "rh_mix_plan.h"]),  # rh_wide_mix_batch: refusals, source ranges, and the tiles that cover every mixer's block once
    "player_mix_plan_test": dict(hdrs=["rh_player_mix_plan.h", "rh_mix_plan.h"]),  # rh_player_mix_block: refusals, table sizes, the ramp that is a constant, launches and their kernel
    "loop_mix_plan_test": dict(hdrs=["rh_loop_mix_plan.h", "rh_mix_plan.h"]),  # rh_loop_mix_block: the two rules, the cursor, exact reciprocals, refusals, the 32-bit bound, launches
    "queue_mix_plan_test": dict(hdrs=["rh_queue_mix_plan.h", "rh_mix_plan.h"]),  # rh_queue_mix_block: chains across sounds, the cursor, segments and pieces, refusals, the 32-bit bound
    "mix_plan_test": dict(hdrs=["rh_mix_plan.h"]),  # what the block mixers share: the source rule, the step index, the slots and launches, the alike cut
    "clip_mix_plan_test": dict(hdrs=["rh_clip_mix_plan.h", "rh_mix_plan.h"]),  # rh_clip_mix_block: the stream, the grid, the cursor, the fade's steps, refusals, the 32-bit bound
}


def build_driver(name: str, force: bool, run) -> str:
    """tests/cpp/NAME.cpp -> tests/cpp/NAME [and NAME_fake] by its entry in DRIVERS; returns the first.  The library does not need the drivers: one
    whose source is missing (an older tests/ run on this library) is skipped."""
    d = DRIVERS[name]
    root = os.path.join(HERE, "..")
    inc = os.path.join(root, "include")
    src = os.path.join(root, "tests", "cpp", name + ".cpp")
    exe = os.path.join(root, "tests", "cpp", name)
    if not os.path.exists(src):
        return exe
    csrc_hdrs = [os.path.join(CSRC, h) for h in d.get("hdrs", [])]
    hdrs = [os.path.join(inc, "rodio_hip.hpp"), os.path.join(inc, "rodio_hip.h")] + csrc_hdrs
    gxx = [shutil.which("g++") or "g++", "-std=c++17", "-O2"]
    fpc = ["-ffp-contract=off"] if d.get("fpc") else []
    warn = ["-Wall", "-Wextra"]
    if d.get("lib"):
        if force or _stale(exe, [src, LIB] + hdrs):
            run([*gxx, *fpc, "-pthread", *warn, "-I", inc, src, "-L", HERE, "-lrodio_hip", "-Wl,-rpath,$ORIGIN/../../rodio_amd", "-Wl,-rpath-link,/opt/rocm/lib", "-o", exe])
    elif force or _stale(exe, [src] + csrc_hdrs):
        run([*gxx, *fpc, *warn, "-I", CSRC, src, "-o", exe])
    if d.get("fake"):
        fakes = [os.path.join(root, "tests", "cpp", f) for f in ("fake_device.cpp", "fake_widemix_filtered.cpp", *d.get("fakes", []))]
        if force or _stale(exe + "_fake", [src] + fakes + hdrs):
            run([*gxx, "-ffp-contract=off", "-pthread", *warn, "-I", inc, *(["-I", CSRC] if csrc_hdrs else []), src, *fakes, "-o", exe + "_fake"])
    return exe


def build_generators_test(force: bool, run) -> str:  # (the tests ask for these three by name)
    build_driver("generators_mirror_test", force, run)
    return build_driver("generators_test", force, run)


def build_noise_test(force: bool, run) -> str:
    return build_driver("noise_mirror_test", force, run)


def build_scan_launch_test(force: bool, run) -> str:
    return build_driver("scan_launch_test", force, run)


if __name__ == "__main__":
    build(force="--force" in sys.argv)
    print(LIB)
