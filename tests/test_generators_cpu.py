"""On-device signal generators, host logic (no GPU): the phase walk of rodio_amd/csrc/rh_generators.h against brute-force f32
stepping (tests/cpp/generators_test, and the library's own host build through rh_signal_phase_advance), the generator setup and
try_seek of signal_generator.rs, and chirp's total_samples / total_duration / try_seek (chirp.rs).  The helpers here are shared
with tests/test_gpu_generators.py."""
import ctypes as C
import importlib.util
import math
import os
import random
import struct
import subprocess
from fractions import Fraction

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GEN_EXE = os.path.join(ROOT, "tests", "cpp", "generators_test")
f32 = np.float32
TAU = f32(6.2831855)


def generators_exe():
    if not os.path.exists(GEN_EXE):  # build() makes it; a tree built before this driver existed gets it here
        spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_generators_test(False, lambda cmd: subprocess.check_call(cmd))
    return GEN_EXE


def fbits(x) -> int:
    return struct.unpack("<I", struct.pack("<f", float(f32(x))))[0]


def bits_f(b: int):
    return f32(struct.unpack("<f", struct.pack("<I", b))[0])


def phase_step(rate, freq):
    """signal_generator.rs:106-107: period = rate as f32 / freq; phase_step = 1.0 / period."""
    return f32(1.0) / (f32(rate) / f32(freq))


def walk(cases):
    """[(step, phase, n)] -> [(advance bits, brute-force bits)] from tests/cpp/generators_test."""
    inp = "".join(f"{fbits(s):08x} {fbits(p):08x} {int(n)}\n" for s, p, n in cases)
    out = subprocess.run([generators_exe(), "walk"], input=inp, capture_output=True, text=True, check=True, timeout=600).stdout.split()
    return [(int(out[2 * k], 16), int(out[2 * k + 1], 16)) for k in range(len(cases))]


def serial_phases(step, phase, n) -> np.ndarray:
    """The n phases rodio's next() sees from `phase` on: `(phase + step).rem_euclid(1.0)` in f32, one at a time."""
    r = subprocess.run([generators_exe(), "phases"], input=f"{fbits(step):08x} {fbits(phase):08x} {int(n)}\n".encode(), capture_output=True, check=True, timeout=600)
    return np.frombuffer(r.stdout, dtype=np.float32).copy()


def wave_ref(function, ph):
    """signal_generator.rs:32-55 over f32 phases (numpy f32 arithmetic: no contraction)."""
    ph = ph.astype(f32)
    if function == "triangle":
        return (f32(4.0) * np.abs(ph - np.floor(ph + f32(0.5))) - f32(1.0)).astype(f32)
    if function == "square":
        return np.where(np.fmod(ph, f32(1.0)) < f32(0.5), f32(1.0), f32(-1.0)).astype(f32)
    if function == "sawtooth":
        return (f32(2.0) * (ph - np.floor(ph + f32(0.5)))).astype(f32)
    return np.sin((TAU * ph).astype(np.float64))  # sine: f64 sin of the f32 argument


def secs_f32(ns):
    return f32(ns // 1_000_000_000) + f32(ns % 1_000_000_000) / f32(1e9)


def rem_euclid(x):
    x = f32(x)
    r = f32(math.fmod(float(x), 1.0)) if np.isfinite(x) else f32("nan")
    return f32(r + f32(1.0)) if r < 0 else r


def seek_phase_ref(rate, freq, pos_ns):
    """signal_generator.rs:148-153: (as_secs_f32(d) * rate as f32 / period).rem_euclid(1.0), left to right."""
    period = f32(rate) / f32(freq)
    with np.errstate(all="ignore"):
        return rem_euclid(f32(f32(secs_f32(pos_ns) * f32(rate)) / period))


def chirp_total_ref(rate, duration_ns):
    """chirp.rs:40: (duration.as_secs_f64() * rate as f64) as u64."""
    v = (float(duration_ns // 1_000_000_000) + float(duration_ns % 1_000_000_000) / 1e9) * float(rate)
    return 0 if not v > 0 else min(int(v), (1 << 64) - 1)


def from_secs_f64_ns(v: float) -> int:
    """Duration::from_secs_f64: the exact value of the f64, rounded to the nearest nanosecond, ties to even."""
    q = Fraction(v) * 1_000_000_000
    fl = q.numerator // q.denominator
    r = q - fl
    return fl + (1 if r > Fraction(1, 2) or (r == Fraction(1, 2) and fl % 2) else 0)


def walk_cases(seed=7, count=2500):
    rng = random.Random(seed)
    rates = [200, 8000, 22050, 44100, 48000, 96000, 192000]
    cases = []
    for _ in range(count):
        rate = rng.choice(rates + [rng.randint(200, 192000)])
        k = rng.random()
        if k < 0.45:
            freq = 10 ** rng.uniform(-2, math.log10(rate / 2))
        elif k < 0.55:
            freq = rate / 4  # step 0.25, exact
        elif k < 0.65:
            freq = rate / 3
        elif k < 0.72:
            freq = rate / 2
        elif k < 0.8:
            freq = rate  # step 1
        elif k < 0.9:
            freq = rate * rng.uniform(1.0, 7.0)  # step > 1
        else:
            freq = rng.choice([0.01, 20, 440, 5000, 20000])
        p0 = f32(0.0) if rng.random() < 0.3 else seek_phase_ref(rate, freq, rng.randrange(0, 10**13))
        n = rng.choice([0, 1, 2, 3, 64, 65, rng.randint(0, 5000), rng.randint(0, 200000)])
        cases.append((phase_step(rate, freq), p0, n))
    return cases


def test_walk_matches_brute_force_stepping():
    cases = walk_cases()
    got = walk(cases)
    bad = [(c, g) for c, g in zip(cases, got) if g[0] != g[1]]
    assert not bad, bad[:5]
    # the walk is not trivially serial: most of these cases land on a phase that is not (p0 + n * step) mod 1 in f64
    assert sum(1 for (s, p, n), (a, _) in zip(cases, got) if n and bits_f(a) != f32((float(p) + n * float(s)) % 1.0)) > len(cases) // 3


@pytest.mark.parametrize("rate,freq", [(48000, 440), (192000, 20), (200, 0.01), (48000, 12000), (44100, 14700), (48000, 48000), (44100, 30000), (8000, 3999.5)])
def test_walk_2_pow_24_samples(rate, freq):
    s = phase_step(rate, freq)
    cases = [(s, f32(0.0), 1 << 24), (s, seek_phase_ref(rate, freq, 123_456_789_012), (1 << 24) - 3)]
    for a, b in walk(cases):
        assert a == b, (rate, freq, hex(a), hex(b))


def test_walk_ties_and_odd_steps():
    # steps whose last bits make in-binade ties (s / ulp = m + 1/2) in several binades, and tiny steps that stall
    cases = []
    for e in range(-24, 0):
        for m in (0x400001, 0x400003, 0x7fffff, 0x600000, 0x000001):
            s = f32(np.ldexp(f32(1.0) + f32(m) / f32(1 << 23), e))
            for p in (f32(0.0), f32(0.5), f32(0.75) + f32(2.0**-24), f32(0.25) - f32(2.0**-26)):
                cases.append((s, p, 70000))
    cases += [(f32(1e-9), f32(0.5), 1000), (f32(5.2e-8), f32(0.9), 100000), (f32(0.0), f32(0.3), 10)]
    bad = [(c, g) for c, g in zip(cases, walk(cases)) if g[0] != g[1]]
    assert not bad, bad[:5]


def test_library_host_walk_matches(rh):
    assert rh.signal_phase_advance(0.25, 0.0, (1 << 63) + 5) == 0.25  # step 0: returns at once
    cases = walk_cases(seed=11, count=400)
    for (s, p, n), (_, ref) in zip(cases, walk(cases)):
        got = rh.signal_phase_advance(p, s, n)
        assert fbits(got) == ref, (s, p, n, got, bits_f(ref))


def test_generator_setup_and_refusals(rh):
    lib = rh.lib
    st = (C.c_float * 2)()
    for rate, freq in [(48000, 440.0), (2000, 500.0), (44100, 0.01), (192000, 192000.0), (8000, 1e7)]:
        assert lib.rh_signal_generator_init(st, rate, freq) == 0
        assert fbits(st[0]) == fbits(phase_step(rate, freq)) and st[1] == 0.0
    for rate, freq in [(48000, 0.0), (48000, -1.0), (48000, float("nan")), (0, 440.0)]:
        assert lib.rh_signal_generator_init(st, rate, freq) == 1  # RH_ERR_INVALID: rodio's assert!(frequency > 0.0), NonZero rate
    # +inf: period 0, step inf, and the first step leaves a NaN phase (as the reference's)
    assert lib.rh_signal_generator_init(st, 48000, float("inf")) == 0 and math.isinf(st[0])
    assert math.isnan(rh.signal_phase_advance(0.0, st[0], 1))


def test_generator_seek(rh):
    lib = rh.lib
    ph = (C.c_float * 1)()
    rng = random.Random(3)
    for _ in range(2000):
        rate = rng.choice([200, 44100, 48000, 192000, rng.randint(1, 400000)])
        freq = float(f32(10 ** rng.uniform(-2, 6)))
        pos = rng.choice([0, 1, 999_999_999, 10**9, rng.randrange(0, 10**12), rng.randrange(0, 1 << 64)])
        assert lib.rh_signal_generator_seek(ph, rate, freq, pos) == 0
        want = seek_phase_ref(rate, freq, pos)
        assert fbits(ph[0]) == fbits(want) or (math.isnan(ph[0]) and math.isnan(want)), (rate, freq, pos, ph[0], want)
        assert math.isnan(ph[0]) or 0.0 <= ph[0] < 1.0
    assert lib.rh_signal_generator_seek(ph, 48000, 0.0, 5) == 1


def test_chirp_totals_durations_and_seek_positions(rh):
    lib = rh.lib
    t = C.c_uint64()
    s, ns = C.c_uint64(), C.c_uint32()
    rng = random.Random(5)
    for _ in range(3000):
        rate = rng.choice([1, 200, 44100, 48000, 96000, 192000, rng.randint(1, 1 << 32 - 1)])
        d = rng.choice([0, 1, 20833, 10**9, 1_500_000_000, rng.randrange(0, 10**12), rng.randrange(0, 1 << 64)])
        assert lib.rh_chirp_total_samples(rate, d, C.byref(t)) == 0
        assert t.value == chirp_total_ref(rate, d), (rate, d)
        total = t.value
        assert lib.rh_chirp_total_duration(rate, total, C.byref(s), C.byref(ns)) == 0
        want = from_secs_f64_ns(float(total) / float(rate))
        assert s.value * 10**9 + ns.value == want, (rate, total, s.value, ns.value, want)
        assert ns.value < 10**9
    # a position past 2^32 samples is a legal u64 seek target (chirp.rs:88-96)
    assert lib.rh_chirp_total_samples(48000, 100_000 * 10**9, C.byref(t)) == 0 and t.value == 4_800_000_000


def test_reference_vectors_restated():
    """The reference's own unit tests (signal_generator.rs:158-230) hold for the f32 restatement the GPU tests compare with."""
    sq = wave_ref("square", serial_phases(phase_step(2000, 500), 0.0, 8))
    assert sq.tolist() == [1, 1, -1, -1, 1, 1, -1, -1]
    tri = wave_ref("triangle", serial_phases(phase_step(8000, 1000), 0.0, 16))
    assert tri.tolist() == [-1, -0.5, 0, 0.5, 1, 0.5, 0, -0.5, -1, -0.5, 0, 0.5, 1, 0.5, 0, -0.5]
    saw = wave_ref("sawtooth", serial_phases(phase_step(200, 50), 0.0, 7))
    assert saw.tolist() == [0, 0.5, -1, -0.5, 0, 0.5, -1]


# ---- the C++ mirror's generators (include/rodio_hip.hpp) through tests/cpp/generators_mirror_test[_fake] ----
MIRROR_EXE = os.path.join(ROOT, "tests", "cpp", "generators_mirror_test")
MIRROR_FAKE = os.path.join(ROOT, "tests", "cpp", "generators_mirror_test_fake")


def mirror_exe(fake: bool):
    exe = MIRROR_FAKE if fake else MIRROR_EXE
    if not os.path.exists(exe):
        generators_exe()
        spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_generators_test(True, lambda cmd: subprocess.check_call(cmd))
    return exe


def run_mirror(fake, *args):
    r = subprocess.run([mirror_exe(fake), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        k, v = line.split(" ", 1)
        out.setdefault(k, []).append(v)
    return out


def check_mirror_trait(fake):
    o = run_mirror(fake, "trait")
    endless = f"{(1 << 64) - 1} -1"
    for name, rate in [("signal", 2000), ("sine", 48000), ("square", 48000), ("triangle", 48000), ("sawtooth", 48000)]:
        assert o[name + ".size_hint"] == [endless] and o[name + ".total_duration"] == ["-1"] and o[name + ".span"] == ["-1"]
        assert o[name + ".format"] == [f"1 {rate}"]
    want = [seek_phase_ref(48000, 440.0, 123456789)] * 4 + [seek_phase_ref(2000, 500.0, 123456789)]
    got = [v.split() for v in o["seek"]]
    assert all(g[0] == "1" and f32(float(g[1])) == w for g, w in zip(got, want)), (got, want)
    assert o["refused"] == ["1"]
    total = chirp_total_ref(48000, 1_500_000_001)
    dur = from_secs_f64_ns(total / 48000)
    assert o["chirp.size_hint"] == [f"{total} {total}"] and o["chirp.total_duration"] == [str(dur)] and o["chirp.span"] == ["-1"]
    assert o["chirp_after10.size_hint"] == [f"{total - 10} {total - 10}"]
    assert o["chirp_seek"] == ["1 48000"] and o["chirp_sought.size_hint"] == [f"{total - 48000} {total - 48000}"]
    assert o["chirp_end.size_hint"] == ["0 0"] and o["chirp_next_at_end"] == ["0"]
    big = chirp_total_ref(48000, 200_000 * 10**9) - (1 << 32) - 7
    assert o["chirp_big.size_hint"] == [f"{big} {big}"]


def check_mirror_chain(fake, tmp_path, block_frames):
    o = run_mirror(fake, "chain", tmp_path / "c.f32", block_frames)
    got = np.fromfile(tmp_path / "c.f32", dtype=np.float32)
    s = phase_step(44100, 441.7)
    want = np.concatenate([wave_ref("triangle", serial_phases(s, 0.0, 100_000)), wave_ref("triangle", serial_phases(s, seek_phase_ref(44100, 441.7, 2_500_000_000), 50_000))])
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32))
    assert o["uploaded"] == ["0"] and int(o["generated"][0]) >= 150_000


def check_mirror_mixer(fake, tmp_path):
    o = run_mirror(fake, "mixer", tmp_path)
    a = np.fromfile(tmp_path / "gen.f32", dtype=np.float32)
    b = np.fromfile(tmp_path / "host.f32", dtype=np.float32)
    assert a.size == 96_000 and np.abs(a).max() > 0.1
    assert np.array_equal(a.view(np.uint32), b.view(np.uint32))
    assert o["uploaded_gen"] == ["0"] and int(o["uploaded_host"][0]) >= 8 * 44_100


def test_cpp_mirror_trait_on_cpu_stand_in():
    check_mirror_trait(True)


@pytest.mark.parametrize("block_frames", [1000, 4096])
def test_cpp_mirror_chain_on_cpu_stand_in(tmp_path, block_frames):
    check_mirror_chain(True, tmp_path, block_frames)


def test_cpp_mirror_mixer_on_cpu_stand_in(tmp_path):
    check_mirror_mixer(True, tmp_path)


def test_walk_with_zero_step_returns():
    # freq so small that the period is inf: step 0; the walk must not step n times (n = 2^63 would never end)
    st = phase_step(48000, 1e-38)
    assert st == 0.0
    assert walk([(st, f32(0.25), 5)]) == [(fbits(0.25), fbits(0.25))]
