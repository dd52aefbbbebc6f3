"""tests/player_mix_ref.py -- the numpy restatement the GPU tests of rh_player_mix_block compare with -- held against the oracle, no GPU:
the bits of `Mixer(ch, to_rate)` fed `TestSource(x, c, rate).amplify(g).linear_gain_ramp(d, s, e, clamp).amplify(f)`, with factor tables
whose entries are all f.  Then the meaning of the position words: a stream cut into three unequal blocks, with phase, first_frame and the
factor table's `first` carried across them, equals the one pass.  Then the entry's host decisions (rodio_amd/csrc/rh_player_mix_plan.h):
tests/cpp/player_mix_plan_test, as built by build() and once more under -fsanitize=address,undefined."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import player_mix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [(44100, 48000), (48000, 44100), (48000, 48000), (8000, 48000)]
LAYOUTS = [(1, 2), (2, 2), (2, 1), (6, 2), (2, 6)]
MS = 1_000_000
# (kind, start, end): fade_in, fade_out, and a ramp between two gains of its own with either clamp setting
RAMPS = [(R.RAMP, 0.0, 1.0), (R.CLAMP, 1.0, 0.0), (R.RAMP, 0.3, -1.7), (R.CLAMP, 1.4, 0.6)]
DURATIONS = [5 * MS, 1000 * MS, 0]  # shorter than the sources (40 frames at 8 kHz, 240 at 48 kHz), longer than them, none


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_source(O, x, ch, rate, g, kind, ns, start, end, f):
    s = O.TestSource(x, ch, rate).amplify(float(g))
    if kind != R.NONE:
        s = s.linear_gain_ramp(ns, float(start), float(end), kind == R.CLAMP)
    return s if f is None else s.amplify(float(f))


@pytest.mark.parametrize("ch,to_ch", LAYOUTS)
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_the_restatement_is_the_oracles_mixer(O, rate, to_rate, ch, to_ch):
    rng = np.random.default_rng(rate % 97 + 10 * ch + to_ch)
    F, T = R.reduced(rate, to_rate)
    for ns in DURATIONS:
        for kind, start, end in RAMPS:
            mx, srcs = O.Mixer(to_ch, to_rate), []
            for n, g, f, period, first in ((700, 0.7, 1.3, 7, 5), (333, -1.1, 0.25, 882, (1 << 33) + 871), (1, 1.0, None, 1, 0), (2, 0.5, 2.0, 1, 3)):
                x = rng.uniform(-1, 1, n * ch).astype(np.float32)
                mx.add(oracle_source(O, x, ch, rate, g, kind, ns, start, end, f))
                table = None if f is None else np.full(R.entries_needed(first, period, n * ch), f, np.float32)
                srcs.append(R.block_of(x, ch, rate, to_rate, 0, R.stream_out_frames(n, F, T), gain=g, kind=kind, ramp_ns=ns, start=start, end=end,
                                       factors=table, factor_period=period, factor_first=first))
            # a source without a ramp beside them
            x = rng.uniform(-1, 1, 500 * ch).astype(np.float32)
            mx.add(oracle_source(O, x, ch, rate, 0.9, R.NONE, 0, 1, 1, 0.8))
            srcs.append(R.block_of(x, ch, rate, to_rate, 0, R.stream_out_frames(500, F, T), gain=0.9, factors=np.float32([0.8]), factor_period=1 << 40))
            want = mx.collect()
            M = max(s.frames for s in srcs)
            got = R.player_mix(to_ch, to_rate, M, srcs)
            assert got.size == want.size, (ns, kind)
            bad = np.flatnonzero(bits(got) != bits(want))
            assert bad.size == 0, (ns, kind, start, end, int(bad[0]), got[bad[0]], want[bad[0]])


def test_the_ramp_runs_at_the_rate_in_front_of_speed(O):
    """speed(1.5) relabels 44100 as 66150 (speed.rs); a fade_in inside it still counts time at 44100.  Player::append's order:
    the sound -- here source.fade_in(d) -- then speed, then amplify."""
    rng = np.random.default_rng(5)
    n = 900
    x = rng.uniform(-1, 1, 2 * n).astype(np.float32)
    mx = O.Mixer(2, 48000)
    mx.add(O.TestSource(x, 2, 44100).fade_in(10 * MS).speed(1.5).amplify(0.6))
    want = mx.collect()
    F, T = R.reduced(66150, 48000)
    # the restatement multiplies by the gain FIRST and by the ramp second; with gain 1 and the Amplify as a one-entry table it is this chain
    s = R.block_of(x, 2, 66150, 48000, 0, R.stream_out_frames(n, F, T), kind=R.RAMP, ramp_ns=10 * MS, start=0.0, end=1.0, ramp_rate=44100,
                   factors=np.float32([0.6]), factor_period=1 << 40)
    got = R.player_mix(2, 48000, s.frames, [s])
    assert got.size == want.size and np.array_equal(bits(got), bits(want))
    wrong = R.block_of(x, 2, 66150, 48000, 0, s.frames, kind=R.RAMP, ramp_ns=10 * MS, start=0.0, end=1.0, factors=np.float32([0.6]), factor_period=1 << 40)
    assert not np.array_equal(bits(R.player_mix(2, 48000, s.frames, [wrong])), bits(want))  # (a ramp at the relabelled rate is another ramp)


@pytest.mark.parametrize("cuts", [(0, 1, 2, None), (0, 137, 138, None), (0, 300, 1111, None), (0, 7, 1500, None)])
def test_three_unequal_blocks_are_the_one_pass(cuts):
    """Sources of four rates and three layouts, ramps that end in the first, the second and the third block (and one that outlasts the
    stream), stepped tables with a period that is odd on a stereo source and firsts beyond 2^32; two sources end inside the stream."""
    rng = np.random.default_rng(11)
    to_rate, to_ch = 48000, 2
    specs = []
    for k, (rate, ch, n) in enumerate([(44100, 2, 1800), (48000, 1, 1700), (8000, 6, 320), (96000, 2, 2500), (44100, 1, 600), (22050, 2, 150)]):
        x = rng.uniform(-1, 1, n * ch).astype(np.float32)
        period, first = (441, 3, 882, 1 << 40, 5, 1)[k], (0, (1 << 33) + 1, 871, 12345, 4, 0)[k]
        table = rng.uniform(0.2, 1.5, R.entries_needed(first, period, n * ch)).astype(np.float32)
        kind, start, end = RAMPS[k % 4]
        ns = (2 * MS, 10 * MS, 30 * MS, 3000 * MS, 1 * MS, 0)[k]
        specs.append((x, ch, rate, dict(gain=0.5 + 0.1 * k, kind=kind if k != 4 else R.NONE, ramp_ns=ns, start=start, end=end, first_frame=(0, 0, 100, 7, 0, 0)[k],
                                        factors=table if k != 3 else None, factor_period=period, factor_first=first)))
    total = max(R.stream_out_frames(len(x) // ch, *R.reduced(rate, to_rate)) for x, ch, rate, _ in specs)
    whole = R.player_mix(to_ch, to_rate, total, [R.block_of(x, ch, rate, to_rate, 0, total, **a) for x, ch, rate, a in specs])
    edges = [c if c is not None else total for c in cuts]
    parts = []
    for m0, m1 in zip(edges[:-1], edges[1:]):
        srcs = [R.block_of(x, ch, rate, to_rate, m0, m1, **a) for x, ch, rate, a in specs]
        assert all(0 <= s.frames <= m1 - m0 for s in srcs)
        parts.append(R.player_mix(to_ch, to_rate, m1 - m0, srcs))
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))


def test_the_restatement_counts_what_a_block_touches():
    """touched_frames / reached_samples / entries_needed: what the entry's table check counts."""
    s = R.Src(np.zeros(64, np.float32), 2, 44100, 10)
    assert R.touched_frames(s, 48000) == 9 * 147 // 160 + 2  # both taps of the last frame
    assert R.reached_samples(s, 2, 48000) == 2 * R.touched_frames(s, 48000)
    assert R.reached_samples(s, 1, 48000) == 2 * R.touched_frames(s, 48000) - 1  # a mono mix reads channel 0 only
    s.last = 8
    assert R.touched_frames(s, 48000) == 9  # frame 9's first tap is the last frame: verbatim, no second tap
    s6 = R.Src(np.zeros(64, np.float32), 6, 48000, 10)
    assert R.touched_frames(s6, 48000) == 10 and R.reached_samples(s6, 2, 48000) == 9 * 6 + 2
    assert R.entries_needed(5, 3, 1) == 1 and R.entries_needed(5, 3, 2) == 2 and R.entries_needed((1 << 33) + 2, 3, 4) == 2


def test_ramp_factors_by_hand():
    """fade_in over 1 ms at 8 kHz: step 125 000 ns, frames 0 .. 7 run, frame 8 is elapsed == total: 1.0 from there on."""
    f = R.ramp_factors(R.RAMP, MS, 0.0, 1.0, 8000, np.arange(10))
    p = (np.arange(8) * 125_000).astype(np.float32) / np.float32(1e9) / (np.float32(MS) / np.float32(1e9))
    assert np.array_equal(bits(f[:8]), bits(np.float32(0.0) * (np.float32(1.0) - p) + np.float32(1.0) * p)) and f[8] == 1.0 and f[9] == 1.0
    assert np.all(R.ramp_factors(R.CLAMP, 0, 1.0, 0.25, 8000, np.arange(4)) == np.float32(0.25))
    assert np.all(R.ramp_factors(R.RAMP, 0, 0.0, 0.25, 8000, np.arange(4)) == np.float32(1.0))


# ---- the plan header ------------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "tests", "cpp", "player_mix_plan_test")
SRC = EXE + ".cpp"
HEADER = os.path.join(ROOT, "rodio_amd", "csrc", "rh_player_mix_plan.h")


def plan_exe():
    spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "player_mix_plan_test" in b.DRIVERS and os.path.exists(HEADER)
    b.build_driver("player_mix_plan_test", False, lambda cmd: subprocess.check_call(cmd))  # (build() makes it; stale or missing: here)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}


def test_refusals_reach_ramps_launches_and_kernels():
    n = run(plan_exe())
    assert n["failures"] == 0
    # the run was not vacuous: every refusal asked for, reaches walked, launches planned, both kernels chosen
    assert n["refusals"] == 27 and n["reach"] == 400 and n["ramps"] == 14 and n["calls"] == 400 and n["stereo"] >= 20 and n["shapes"] == 16
    assert run(plan_exe(), 2, 150)["failures"] == 0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Host code with a main of its own: built with the sanitizers and run as it is."""
    exe = str(tmp_path / "player_mix_plan_test_san")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rodio_amd", "csrc"), SRC, "-o", exe])
    n = run(exe, 4, 150)
    assert n["failures"] == 0 and n["calls"] == 150 and n["refusals"] == 27
