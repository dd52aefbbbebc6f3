"""The scan kernels' host protocol (rodio_amd/csrc/rh_scan_launch.h), no GPU: tests/cpp/scan_launch_test runs begin / jump / launched /
failed against a model of the device (a ticket counter and two hand-off tables) over scripted and seeded random sequences of launches,
and the variant pick against the rule written out as a brute-force scan over both kernels' tables."""
import importlib.util
import os
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "scan_launch_test")


def scan_launch_exe():
    if not os.path.exists(EXE):  # build() makes it; a tree built before this driver existed gets it here
        spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_scan_launch_test(False, lambda cmd: subprocess.check_call(cmd))
    return EXE


def run(*args):
    r = subprocess.run([scan_launch_exe(), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}


def test_protocol_against_the_device_model_and_variant_pick_against_brute_force():
    n = run()
    assert n["failures"] == 0
    # the run was not vacuous: thousands of launches with and without the kernel in front, jumps and failures among them
    assert n["launches"] > 50_000 and n["skipped"] > 10_000 and n["inits"] > 10_000 and n["jumps"] > 1000 and n["failed"] > 1000
    assert n["picks"] > 4000


def test_other_seeds():
    for seed in (1, 2, 3):
        assert run(seed, 1500)["failures"] == 0
