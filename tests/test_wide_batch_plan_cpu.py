"""The plan of rh_wide_mix_batch (rodio_amd/csrc/rh_wide_batch_plan.h), no GPU: tests/cpp/wide_batch_plan_test plans random batches and the
shapes of the GPU tests and of the benchmark and checks that every output sample of every mixer lies in exactly one tile, that no tile
crosses a mixer, that the source ranges are the prefix sums of the counts, that every refusal of the header is answered and that the
32-bit fit is check_src's formula (rh_mix_plan.h).  The same stand-alone program runs a second time built with -fsanitize=address,undefined."""
import importlib.util
import os
import shutil
import subprocess

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "wide_batch_plan_test")
SRC = EXE + ".cpp"
HEADER = os.path.join(ROOT, "rodio_amd", "csrc", "rh_wide_batch_plan.h")


def plan_exe():
    spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "wide_batch_plan_test" in b.DRIVERS and os.path.exists(HEADER)
    b.build_driver("wide_batch_plan_test", False, lambda cmd: subprocess.check_call(cmd))  # (build() makes it; stale or missing: here)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}


def test_tiles_ranges_refusals_and_fit():
    n = run(plan_exe())
    assert n["failures"] == 0
    # the run was not vacuous: batches planned and walked, every refusal asked for, the fit on both sides of its boundary
    assert n["batches"] == 400 and n["uniform"] >= 100 and n["refusals"] == 17 and n["fits"] >= 18 and n["shapes"] == 27


def test_other_seeds():
    for seed in (1, 2, 3):
        assert run(plan_exe(), seed, 150)["failures"] == 0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Host code with a main of its own: built with the sanitizers and run as it is."""
    exe = str(tmp_path / "wide_batch_plan_test_san")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rodio_amd", "csrc"), SRC, "-o", exe])
    n = run(exe, 4, 150)
    assert n["failures"] == 0 and n["batches"] == 150 and n["refusals"] == 17
