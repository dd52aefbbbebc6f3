"""On-device noise sources, host logic (no GPU): a numpy restatement of the noise contract of rodio_hip.h (u64 arithmetic), Pink's
closed-form draw index against a brute-force replay of rodio's counters (noise.rs:491-512), rodio's serial f32 integrators against the
f64 recurrence, and the C++ mirror's noise sources (include/rodio_hip.hpp) on the CPU stand-in (tests/cpp/fake_noise.cpp).  The helpers
here are shared with tests/test_gpu_noise.py."""
import importlib.util
import math
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
f32 = np.float32
u64 = np.uint64
KINDS = ["white_uniform", "white_triangular", "white_gaussian", "pink", "blue", "violet", "brownian", "red", "velvet"]
CODE = {k: i for i, k in enumerate(KINDS)}
EXACT = ["white_uniform", "white_triangular", "pink", "blue", "violet", "velvet"]
INTEGRATORS = ["brownian", "red"]
INTEGRATOR_TOL = 4e-5  # absolute, against the f64 recurrence on the same white samples
GAUSS_TOL = 2e-6  # absolute, against the same Box-Muller in f64 on the same fields


# ---- the contract, restated ------------------------------------------------------------------------------------------------------
def mix(z):
    z = np.asarray(z, dtype=u64)
    z = z ^ (z >> u64(30))
    z = z * u64(0xBF58476D1CE4E5B9)
    z = z ^ (z >> u64(27))
    z = z * u64(0x94D049BB133111EB)
    return z ^ (z >> u64(31))


def hash_(seed, k):
    k = np.asarray(k, dtype=u64)
    return mix(u64(seed) ^ mix(k + u64(1)))


def u1(h):
    return ((h >> u64(40)).astype(np.int64) - 8388608).astype(f32) * f32(2.0**-23)


def u2(h):
    return (((h >> u64(16)) & u64(0xFFFFFF)).astype(np.int64) - 8388608).astype(f32) * f32(2.0**-23)


def white(seed, k):
    return u1(hash_(seed, k))


def idx(k0, n):
    with np.errstate(over="ignore"):
        return u64(k0) + np.arange(n, dtype=u64)


def gaussian_f64(h):
    """rh_dither's GPDF expression in f64 on the same (exact) f32 fields."""
    a = ((h >> u64(40)).astype(np.float64) + 1.0) * 2.0**-24
    b = ((h >> u64(16)) & u64(0xFFFFFF)).astype(np.float64) * 2.0**-24
    return np.sqrt(-2.0 * np.log(a)) * np.cos(2.0 * math.pi * b) * 0.6


def draws_before(m):
    """D(m) = sum_{j<16} floor((m-1) / 2^j), m >= 1, as 2x - popc(x) - (2y - popc(y)) with x = m - 1, y = x >> 16 (mod 2^64)."""
    with np.errstate(over="ignore"):
        x = np.asarray(m, dtype=u64) - u64(1)
        y = x >> u64(16)
        return (u64(2) * x - np.bitwise_count(x).astype(u64)) - (u64(2) * y - np.bitwise_count(y).astype(u64))


def pink_ref(seed, k):
    k = np.asarray(k, dtype=u64)
    s = np.zeros(k.shape, f32)
    for i in range(16):
        m = k & ~u64((1 << i) - 1)
        with np.errstate(over="ignore"):
            v = np.where(m == 0, f32(0), white(seed, draws_before(np.maximum(m, u64(1))) + u64(i)))
        s = (s + v).astype(f32)
    return (s / f32(16)).astype(f32)


def velvet_grid(rate, density):
    return int(math.ceil(f32(rate) / f32(density)))


def velvet_ref(seed, k, grid):
    k = np.asarray(k, dtype=u64)
    c = k // u64(grid)
    hc = hash_(seed, c)
    pos = ((hc >> u64(32)) * u64(grid)) >> u64(32)
    sign = np.where((hc & u64(0x80000000)) != 0, f32(1), f32(-1))
    return np.where(k - c * u64(grid) == pos, sign, f32(0)).astype(f32)


def reference(kind, seed, k0, n, rate=48000, density=2000):
    """Samples k0 .. k0+n of an exact kind (white_gaussian: f64 values) by the contract."""
    k = idx(k0, n)
    h = hash_(seed, k)
    if kind == "white_uniform":
        return u1(h)
    if kind == "white_triangular":
        return ((u1(h) + u2(h)) * f32(0.5)).astype(f32)
    if kind == "white_gaussian":
        return gaussian_f64(h)
    if kind in ("blue", "violet"):
        km = idx(k0 - 2, n + 2) if k0 >= 2 else None
        if km is None:
            w = np.concatenate([np.zeros(2 - k0, f32), white(seed, idx(0, n + k0))])
        else:
            w = white(seed, km)
        b = (w[1:] - w[:-1]).astype(f32)  # b[q] = B(k0 - 1 + q)
        if k0 == 0:
            b[0] = f32(0)  # B(-1) = 0
        return b[1:] if kind == "blue" else (b[1:] - b[:-1]).astype(f32)
    if kind == "pink":
        return pink_ref(seed, k)
    if kind == "velvet":
        return velvet_ref(seed, k, velvet_grid(rate, density))
    raise ValueError(kind)


def integrator_consts(kind, rate):
    leak = f32(1) - (f32(2) * f32(math.pi) * f32(5)) / f32(rate)
    sigma = np.sqrt(f32(1) / f32(3)).astype(f32) if kind == "red" else f32(0.6)
    var = f32(f32(sigma * sigma) / f32(f32(1) - f32(leak * leak)))
    return leak, f32(f32(1) / np.sqrt(var).astype(f32))


def recurrence_f64(w, leak, scale, acc=0.0):
    """acc = acc * leak + w; out = acc * scale, in f64 (a first-order IIR: scipy's lfilter with the carried acc as its state)."""
    from scipy.signal import lfilter

    y = lfilter([1.0], [1.0, -float(leak)], np.asarray(w, np.float64), zi=[float(leak) * float(acc)])[0]
    return y * float(scale)


def serial_f32(w, leak, scale, acc=0.0):
    """rodio's loop (noise.rs:705-711) in f32, one sample at a time."""
    acc, leak, scale = f32(acc), f32(leak), f32(scale)
    out = np.empty(w.size, f32)
    w = w.astype(f32)
    for j in range(w.size):
        acc = f32(f32(acc * leak) + w[j])
        out[j] = f32(acc * scale)
    return out


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_values(a, b):
    return a.shape == b.shape and bool(np.all((a == b) | (np.isnan(a) & np.isnan(b))))


# ---- Pink: the closed form against rodio's counters --------------------------------------------------------------------------------
def pink_replay_draws(k0, n):
    """noise.rs:491-512 replayed: for samples k0 .. k0+n, the draw number each of the 16 generators holds (-1: still 0.0).  The state
    at k0 is set up as the counters would be: generator i last drew at the largest multiple m of 2^i with 2^i <= m < k0 (none: its
    counter is k0), and the white stream has given out D(k0) draws; D(k0) for k0 > 0 is itself checked against the plain sum."""
    counters, held = [], []
    for i in range(16):
        m = ((k0 - 1) >> i) << i if k0 > 0 else 0
        if k0 > 0 and m >= (1 << i):
            counters.append(k0 - m)
            held.append(draws_before_int(m) + i)
        else:
            counters.append(k0)
            held.append(-1)
    d = draws_before_int(k0) if k0 > 0 else 0
    out = np.empty((n, 16), np.int64)
    for s in range(n):
        for i in range(16):
            if counters[i] >= (1 << i):
                held[i] = d
                d += 1
                counters[i] = 0
            counters[i] += 1
        out[s] = held
    return out


def draws_before_int(m):
    return sum((m - 1) >> j for j in range(16))


def pink_closed_draws(k0, n):
    k = idx(k0, n)
    out = np.empty((n, 16), np.int64)
    for i in range(16):
        m = k & ~u64((1 << i) - 1)
        d = (draws_before(np.maximum(m, u64(1))) + u64(i)).astype(np.int64)
        out[:, i] = np.where(m == 0, -1, d)
    return out


def test_pink_draw_count_closed_form():
    rng = np.random.default_rng(3)
    ms = [1, 2, 3, 4, 65535, 65536, 65537, (1 << 32) - 5, 1 << 32, (1 << 40) + 3, (1 << 63) + 11] + [int(x) for x in rng.integers(1, 1 << 62, 2000)]
    got = draws_before(np.array(ms, dtype=u64))
    want = np.array([draws_before_int(m) % (1 << 64) for m in ms], dtype=u64)
    assert np.array_equal(got, want)


@pytest.mark.parametrize("k0,n", [(0, (1 << 17) + 50), ((1 << 32) - 5, 1 << 13), ((1 << 40) + 3, 1 << 13), ((1 << 32) - 4096, 8192)])
def test_pink_closed_form_matches_counter_replay(k0, n):
    assert np.array_equal(pink_closed_draws(k0, n), pink_replay_draws(k0, n))


def test_pink_generator_0_first_updates_at_sample_1():
    d = pink_closed_draws(0, 4)
    assert list(d[0]) == [-1] * 16 and d[1, 0] == 0 and d[1, 1] == -1 and d[2, 0] == 1 and d[2, 1] == 2


# ---- the restatement's own invariants --------------------------------------------------------------------------------------------
def test_blue_violet_restatement_is_split_invariant():
    for kind in ("blue", "violet"):
        one = reference(kind, 9, 0, 4000)
        for k0 in (1, 2, 3, 1000):
            assert np.array_equal(bits(reference(kind, 9, k0, 4000 - k0)), bits(one[k0:]))
    w = white(9, idx(0, 3))
    assert reference("blue", 9, 0, 1)[0] == w[0] and reference("violet", 9, 0, 2)[1] == f32(f32(w[1] - w[0]) - w[0])


def test_velvet_one_impulse_per_cell():
    rate, density = 44100, 2000
    grid = velvet_grid(rate, density)
    assert grid == 23  # ceil(22.05)
    y = velvet_ref(4, idx(0, grid * 500), grid).reshape(500, grid)
    assert np.all(np.count_nonzero(y, axis=1) == 1) and set(np.unique(y[y != 0])) <= {f32(1), f32(-1)}
    assert 0.4 < np.mean(y[y != 0] > 0) < 0.6
    assert velvet_grid(48000, 1) == 48000 and velvet_grid(48000, 96000) == 1


# ---- rodio's serial f32 integrators against f64 (the yardstick of the device's bound) --------------------------------------------
NOISE_EXE = os.path.join(ROOT, "tests", "cpp", "noise_mirror_test")
NOISE_FAKE = os.path.join(ROOT, "tests", "cpp", "noise_mirror_test_fake")


def noise_exe(fake: bool):
    exe = NOISE_FAKE if fake else NOISE_EXE
    if not os.path.exists(exe):  # build() makes it; a tree built before this driver existed gets it here
        spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
        b = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(b)
        b.build_noise_test(True, lambda cmd: subprocess.check_call(cmd))
    return exe


def run_noise(fake, *args):
    r = subprocess.run([noise_exe(fake), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        k, v = line.split(" ", 1)
        out.setdefault(k, []).append(v)
    return out


def serial_and_f64(kind, rate, seed, n, tmp_path):
    """rodio's serial f32 loop (the C++ mirror's host next()) and the f64 recurrence on the same white samples."""
    run_noise(True, "serial", CODE[kind], rate, seed, n, tmp_path)
    return np.fromfile(tmp_path / "f32.bin", dtype=f32), np.fromfile(tmp_path / "f64.bin", dtype=np.float64)


@pytest.mark.parametrize("kind", INTEGRATORS)
@pytest.mark.parametrize("rate", [8000, 44100, 48000, 192000])
def test_serial_integrators_within_bound_of_f64(kind, rate, tmp_path):
    y32, y64 = serial_and_f64(kind, rate, 12345, 1 << 24, tmp_path)
    err = np.max(np.abs(y32.astype(np.float64) - y64))
    assert 1e-7 < err <= INTEGRATOR_TOL, err


def test_serial_integrator_matches_restatement(tmp_path):
    for kind in INTEGRATORS:
        y32, _ = serial_and_f64(kind, 44100, 5, 5000, tmp_path)
        leak, scale = integrator_consts(kind, 44100)
        if kind == "red":
            assert np.array_equal(bits(y32), bits(serial_f32(white(5, idx(0, 5000)), leak, scale)))
        else:  # the host's logf / cosf: compare with f64 Box-Muller
            assert np.max(np.abs(y32 - serial_f32(gaussian_f64(hash_(5, idx(0, 5000))).astype(f32), leak, scale))) < 1e-5


def test_library_init_words_and_refusals(rh):
    for kind in KINDS:
        st = rh.noise_state(kind, 44100, (1 << 63) + 17, 1000)
        assert st[0] == 17 and st[1] == 1 << 31 and st[2] == 0 and st[3] == 0 and st[4] == CODE[kind] and st[7] == 0
        if kind == "velvet":
            assert st[5] == velvet_grid(44100, 1000) and st[6] == 0
        elif kind in INTEGRATORS:
            leak, scale = integrator_consts(kind, 44100)
            assert st[5:7].view(f32)[0] == leak and st[5:7].view(f32)[1] == scale
        else:
            assert st[5] == 0 and st[6] == 0
    assert rh.noise_state("velvet", 4294967295, 1, 1)[5:7].tolist() == [0, 1]  # a grid of 2^32: the high word
    for bad in [dict(kind=9), dict(kind=-1), dict(kind="velvet", density=0), dict(kind="red", rate=0)]:
        with pytest.raises((rh.RhError, ValueError)):
            rh.noise_state(bad.get("kind"), bad.get("rate", 48000), 1, bad.get("density", 2000))
    C = __import__("ctypes")
    st = (C.c_uint32 * 8)()
    assert rh.lib.rh_noise_init(st, 9, 48000, 1, 2000) == 1 and rh.lib.rh_noise_init(st, 8, 48000, 1, 0) == 1
    assert rh.lib.rh_noise_init(st, 3, 0, 1, 2000) == 1 and rh.lib.rh_noise_init(st, 3, 48000, 1, 0) == 0  # density matters to velvet only


def test_python_classes_host_side(rh):
    assert rh.WhiteUniform.KIND == "white_uniform" and rh.source.NOISE_KINDS["velvet"] == 8
    with pytest.raises(ValueError):
        rh.source._noise_kind("grey")
    assert rh.source.entropy_seed() != rh.source.entropy_seed()


# ---- the C++ mirror on the CPU stand-in --------------------------------------------------------------------------------------------
def check_noise_trait(fake):
    o = run_noise(fake, "trait")
    endless = f"{(1 << 64) - 1} -1"
    for name in ["WhiteUniform", "WhiteTriangular", "WhiteGaussian", "Pink", "Blue", "Violet", "Brownian", "Red", "Velvet"]:
        assert o[name + ".size_hint"] == [endless] and o[name + ".total_duration"] == ["-1"] and o[name + ".span"] == ["-1"]
        assert o[name + ".format"] == ["1 44100"] and o[name + ".seek"] == ["1"]
    sd = [f32(float(x)) for x in o["std_dev"][0].split()]
    assert sd == [np.sqrt(f32(1) / f32(3)).astype(f32), f32(2) / np.sqrt(f32(6)).astype(f32), f32(0.6)] and o["mean"] == ["0"]
    assert o["entropy_seeds_differ"] == ["1"] and o["velvet_grid"] == ["24 48"]
    assert o["refused"] == ["0 1", "1 1", "2 1"]


def check_noise_follow(fake, kind, rate, seed, tmp_path):
    o = run_noise(fake, "follow", CODE[kind], rate, seed, tmp_path)
    a = np.fromfile(tmp_path / "mixed.f32", dtype=f32)
    b = np.fromfile(tmp_path / "host.f32", dtype=f32)
    assert a.size == b.size == 5500 and o["k"] == ["5500 5500"]
    return a, b


def check_noise_chain(fake, kind, tmp_path, block_frames):
    o = run_noise(fake, "chain", CODE[kind], tmp_path / "c.f32", block_frames)
    got = np.fromfile(tmp_path / "c.f32", dtype=f32)
    k1 = int(o["k_at_seek"][0])
    assert k1 >= 100_000 and o["uploaded"] == ["0"] and int(o["generated"][0]) >= 150_000
    assert o["chain.format"] == ["1 48000"] and o["chain.total_duration"] == ["-1"]
    return got, k1


def test_cpp_noise_trait_on_cpu_stand_in():
    check_noise_trait(True)


@pytest.mark.parametrize("kind", KINDS)
def test_cpp_noise_follow_on_cpu_stand_in(kind, tmp_path):
    a, b = check_noise_follow(True, kind, 44100, 31, tmp_path)
    assert np.array_equal(bits(a), bits(b))  # the stand-in and next() share every bit, the integrators' serial loop included
    if kind in EXACT:
        assert np.array_equal(bits(a), bits(reference(kind, 31, 0, 5500, rate=44100)))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("block_frames", [1000, 4096])
def test_cpp_noise_chain_on_cpu_stand_in(kind, block_frames, tmp_path):
    got, k1 = check_noise_chain(True, kind, tmp_path, block_frames)
    if kind in EXACT:
        want = np.concatenate([reference(kind, 77, 0, 100_000), reference(kind, 77, k1, 50_000)])
        assert np.array_equal(bits(got), bits(want))
    elif kind == "red":  # try_seek: acc = 0, k where the chain's pulls left it
        leak, scale = integrator_consts(kind, 48000)
        want = np.concatenate([serial_f32(white(77, idx(0, 100_000)), leak, scale), serial_f32(white(77, idx(k1, 50_000)), leak, scale)])
        assert np.array_equal(bits(got), bits(want))
    else:
        assert np.all(np.isfinite(got)) and got[100_000] == f32(f32(0) + f32(got[100_000]))


def test_cpp_noise_mixer_on_cpu_stand_in(tmp_path):
    check_noise_mixer(True, tmp_path)


def check_noise_mixer(fake, tmp_path):
    o = run_noise(fake, "mixer", tmp_path)
    a = np.fromfile(tmp_path / "gen.f32", dtype=f32)
    b = np.fromfile(tmp_path / "host.f32", dtype=f32)
    assert a.size == 96_000 and np.abs(a).max() > 0.05
    assert np.array_equal(bits(a), bits(b))
    assert o["uploaded_gen"] == ["0"] and int(o["uploaded_host"][0]) >= 9 * 44_100
