"""The fused path's launch decisions (rodio_amd/csrc/rh_rlm_launch.h), no GPU: tests/cpp/rlm_launch_test runs the route of a launch over
the full cross product of its inputs against the conditions written out a second time, the cut of the mixed row around every boundary
by its properties and by hand-computed cases, the ticket accounting against a model of the device's counters (across their wrap) and
the geometry of a stream block in one kernel over random rates and blocks."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "rlm_launch_test")


def rlm_launch_exe():
    if not os.path.exists(EXE):  # build() makes it; a tree built before this driver existed gets it here
        spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_driver("rlm_launch_test", False, lambda cmd: subprocess.check_call(cmd))
    return EXE


def run(*args):
    r = subprocess.run([rlm_launch_exe(), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}


def test_route_row_cut_tickets_and_block_geometry():
    n = run()
    assert n["failures"] == 0
    # the run was not vacuous: every route taken, every boundary of the cut, launches across the counters' wrap, blocks taken and refused for every reason
    assert n["routes"] > 50_000 and n["routes_reached"] == 7
    assert n["cuts"] > 100_000
    assert n["launches"] >= 6000 and n["wraps"] >= 2
    assert n["blocks"] >= 60_000 and n["accepted"] > 2000 and n["refusal_reasons"] == 6


def test_other_seeds():
    for seed in (1, 2, 3):
        assert run(seed, 3000)["failures"] == 0
