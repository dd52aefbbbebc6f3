"""rodio_amd/csrc/rh_mix_plan.h -- the host rules the block mixers share -- against Python integers, no GPU: tests/cpp/mix_plan_test prints
what the header answers (the step index of rh_live.hip's rule, check_src, the (F, T, r0) slots and launches of walk_rates, alike_cut), as
built by build() and once more as a stand-alone program under -fsanitize=address,undefined.

The step index is asked at k = 0, 1, n - 1 and one either side of EVERY boundary below n (period 96000 at n = 2^30: 11184 of them).
Period 1 has a boundary at every sample: its first and last three.  Periods 2 and 3 have 2^29 and 2^30 / 3 of them below n = 2^30, more
than a test can hand to Python: the first and last three and 4096 spread evenly are held against Python integers, and EVERY sample any of
the four `at` reaches against the quotient counted up sample by sample by the program (stepsweep).  One sweep a period does that: for a
period up to 2^31 step(k) is a function of x = at % period + k alone -- the multiplier and the shifts are the period's, which the test
holds for each `at` (stepwords) --, so the sweep from at = 0 over n + period samples passes every x that any `at` below reaches."""
import importlib.util
import os
import shutil
import subprocess
from math import gcd

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "mix_plan_test")
SRC = EXE + ".cpp"
OK, INVALID, UNSUPPORTED = 0, 1, 3
NONE = 0xFFFFFFFF
U32 = (1 << 32) - 1


def built_exe():
    spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert b.DRIVERS["mix_plan_test"] == dict(hdrs=["rh_mix_plan.h"])
    b.build_driver("mix_plan_test", False, lambda cmd: subprocess.check_call(cmd))  # (build() makes it; stale or missing: here)
    return EXE


@pytest.fixture(scope="module", params=["build", "sanitizers"])
def exe(request, tmp_path_factory):
    if request.param == "build":
        return built_exe()
    # host code with a main of its own: built with the sanitizers and run as it is
    out = str(tmp_path_factory.mktemp("san") / "mix_plan_test_san")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rodio_amd", "csrc"), SRC, "-o", out])
    return out


def ask(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr + r.stdout
    return r.stdout.split("\n")[:-1]


# ---- stepdiv ----------------------------------------------------------------------------------------------------------------------------
PERIODS = [1, 2, 3, 96000, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, 1 << 40]
DENSE = (1, 2, 3)  # more boundaries below 2^30 than can be handed over one by one
MANY = 4096
ATS = lambda period: (0, 1, period - 1, period + 5)  # noqa: E731


def boundaries(period, at, n):
    """The k < n at which (at % period + k) // period steps up: every one; of the DENSE periods' the first and last three (period 1), and
    MANY spread evenly between them (periods 2 and 3)."""
    first = period - at % period  # (k = 0 is no boundary: the quotient there is 0)
    if first >= n:
        return []
    count = (n - 1 - first) // period + 1
    if period in DENSE and count > MANY:
        picks = {0, 1, 2, count - 3, count - 2, count - 1} | (set() if period == 1 else {i * count // MANY for i in range(MANY)})
        return [first + b * period for b in sorted(picks)]
    return [first + b * period for b in range(count)]


@pytest.mark.parametrize("n", [1, 1 << 30])
@pytest.mark.parametrize("period", PERIODS)
def test_the_step_index_is_the_quotient(exe, period, n):
    for at in ATS(period):
        ks = {0, 1, n - 1}
        for b in boundaries(period, at, n):
            ks |= {b - 1, b, b + 1}
        ks = sorted(k for k in ks if 0 <= k < n)
        got = []
        for i in range(0, len(ks), 2000):  # (an argument list has its limits)
            got += [int(v) for v in ask(exe, "stepdiv", period, at, n, *ks[i:i + 2000])]
        want = [(at % period + k) // period for k in ks]
        assert got == want, (period, at, n, next((k, g, w) for k, g, w in zip(ks, got, want) if g != w))


def test_every_boundary_is_asked_where_the_periods_are_not_dense():
    assert len(boundaries(96000, 0, 1 << 30)) == ((1 << 30) - 1) // 96000 == 11184
    assert boundaries(96000, 5, 1 << 30)[:2] == [95995, 191995] and boundaries(1 << 40, (1 << 40) - 1, 1 << 30) == [1] and boundaries(1 << 40, 0, 1 << 30) == []
    many = boundaries(3, 1, 1 << 30)
    assert len(many) == MANY + 5 and many[0] == 2 and many[-1] == (1 << 30) - 2 and max(b - a for a, b in zip(many, many[1:])) <= 3 * (((1 << 30) // 3) // MANY + 1)


@pytest.mark.parametrize("period", DENSE)
def test_every_sample_of_the_dense_periods(period):
    """(2^30 samples: the optimised build only)  The words of every `at` are the period's, so one sweep holds all four (the module's docstring)."""
    n = 1 << 30
    words = [[int(v) for v in ask(built_exe(), "stepwords", period, at, n)[0].split()] for at in ATS(period)]
    assert [w[0] for w in words] == [at % period for at in ATS(period)] and all(w[1:] == words[0][1:] for w in words)
    assert ask(built_exe(), "stepsweep", period, 0, n + period) == ["0"]


# ---- check_src ---------------------------------------------------------------------------------------------------------------------------
def test_check_src_on_the_eight_sources(exe):
    """Three sources of 64 frames into a mix of 64 frames at 48000 Hz (tests/test_gpu_mix_refusals.py): what source 1 is replaced by."""
    F, T = 44100 // gcd(44100, 48000), 48000 // gcd(44100, 48000)
    fit = (U32 - T) // F
    #        to_rate out  data channels from_rate phase frames last   status F T fit
    cases = [(48000, 64, 0, 2, 44100, 0, 64, NONE, [INVALID, 0, 0, 0]),       # data NULL
             (48000, 64, 1, 0, 44100, 0, 64, NONE, [INVALID, 0, 0, 0]),       # channels 0
             (48000, 64, 1, 2, 0, 0, 64, NONE, [INVALID, 0, 0, 0]),           # from_rate 0
             (48000, 64, 1, 2, 44100, 0, 65, NONE, [INVALID, 0, 0, 0]),       # frames 65
             (48000, 64, 1, 2, 44100, T, 64, NONE, [INVALID, F, T, 0]),       # phase = T
             (65537, 64, 1, 2, 65539, 0, 64, NONE, [UNSUPPORTED, 65539, 65537, 0]),  # both prime: F T = 65538^2 - 1 > 2^32 - 1
             (48000, 64, 1, 0, 0, 0xFFFFFFF0, 0, 7, "skip"),                  # frames 0, everything else garbage: not looked at
             (48000, 64, 1, 2, 44100, 0, 64, NONE, [OK, F, T, fit])]          # a valid source
    assert 65539 * 65537 == 65538 ** 2 - 1 > U32 and (F, T) == (147, 160)
    for *args, want in cases:
        got = ask(exe, "check", *args)
        assert got == ([want] if want == "skip" else [" ".join(map(str, want))]), (args, got)


# ---- the slots and launches ----------------------------------------------------------------------------------------------------------------
def launches(to_rate, table, rates=4, chunk=32):
    """walk_rates restated: find-or-add of up to four (F, T, r0) slots; a fifth, or the 32nd source, sends what has been gathered."""
    out, slots, srcs = [], [], []
    for s, (rate, phase, frames) in enumerate(table):
        if frames == 0:
            continue
        key = (rate // gcd(rate, to_rate), to_rate // gcd(rate, to_rate), phase)
        if key not in slots and len(slots) == rates:
            out.append((slots, srcs))
            slots, srcs = [], []
        if key not in slots:
            slots.append(key)
        srcs.append((s, slots.index(key)))
        if len(srcs) == chunk:
            out.append((slots, srcs))
            slots, srcs = [], []
    return out + ([(slots, srcs)] if srcs or not out else [])


def test_forty_sources_of_five_slots(exe):
    A, B, C, D, E = (44100, 0), (48000, 0), (22050, 3), (96000, 0), (44100, 7)  # E: A's rate at another phase
    keys = [[A, B, C, D][s % 4] for s in range(9)] + [E] + [[A, B, C][s % 3] for s in range(10, 37)] + [D, A, E]
    table = [(rate, phase, 64) for rate, phase in keys]
    assert len(table) == 40
    want = launches(48000, table)
    assert [[s for s, _ in srcs] for _, srcs in want] == [list(range(9)), list(range(9, 37)), list(range(37, 40))], "the fifth slot arrives at source 9 and at 37"
    got = ask(exe, "slots", 48000, *[":".join(map(str, t)) for t in table])
    assert len(got) == len(want)
    for k, (line, (slots, srcs)) in enumerate(zip(got, want)):
        head, tail = line.split(" |")
        cont, nr, n, *r = head.split()
        assert (int(cont), int(nr), int(n)) == (1 if k else 0, len(slots), len(srcs))
        assert r == [":".join(map(str, q)) for q in slots] + ["0:1:0"] * (4 - len(slots))  # (an unused slot: F = 0, T = 1)
        assert tail.split() == [f"{s}:{q}" for s, q in srcs]
    # a launch is full at 32 sources; a table that reaches no frame is still one launch, of no source; sources of no frames are not looked at
    assert [len(srcs) for _, srcs in launches(48000, [(44100, 0, 64)] * 70)] == [32, 32, 6]
    lines = ask(exe, "slots", 48000, *["44100:0:64"] * 70)
    assert [ln.split()[:3] for ln in lines] == [["0", "1", "32"], ["1", "1", "32"], ["1", "1", "6"]]
    assert ask(exe, "slots", 48000, "44100:0:0", "0:9:0") == ["0 0 0 0:1:0 0:1:0 0:1:0 0:1:0 |"] == ask(exe, "slots", 48000)
    assert ask(exe, "slots", 48000, "0:9:0", "44100:5:64")[0].endswith("| 1:0")


def test_the_alike_cut(exe):
    """The frames in front of the first alike source that ends go to the kernel for alike sources where there are at least 1024 of them."""
    def cut(out_frames, *srcs, channels=2, to_rate=48000):
        return int(ask(exe, "cut", channels, to_rate, out_frames, *[":".join(map(str, s)) for s in srcs])[0])

    live = (2, 44100, 5, 4096, NONE)
    assert cut(4096, live, live, live) == 0                            # no source ends
    assert cut(4096, live, (2, 44100, 5, 1023, NONE), live) == 0       # one ends at 1023 frames: no cut
    assert cut(4096, live, (2, 44100, 5, 1024, NONE), live) == 1024    # one ends at 1024: the cut falls there
    # ... or where a tap reaches a source's last frame: il(j) >= last  <=>  phase + j F >= last T
    last = 1000
    jl = -(-(last * 160 - 5) // 147)
    assert jl >= 1024 and (5 + jl * 147) // 160 >= last > (5 + (jl - 1) * 147) // 160
    assert cut(4096, live, (2, 44100, 5, 4096, last)) == jl
    # not alike: another layout, rate or phase
    for other in ((1, 44100, 5, 1024, NONE), (2, 48000, 0, 1024, NONE), (2, 44100, 6, 1024, NONE)):
        assert cut(4096, live, other) == 0
    assert cut(4096, (1, 44100, 5, 4096, NONE), (1, 44100, 5, 2000, NONE), channels=1) == 2000
