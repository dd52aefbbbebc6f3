"""Parameters that change while a source plays (periodic_access over live_amplify / live_channel_volume / live_spatial), host
logic: rh_periodic_update_samples against the f32 formula of periodic.rs, and the schedule of the closures through
tests/cpp/live_test_fake (the C++ host mirror over the CPU stand-in tests/cpp/fake_device.cpp + fake_live.cpp).  The helpers
here restate the chains for tests/test_gpu_live.py too."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE_EXE = os.path.join(ROOT, "tests", "cpp", "live_test")
FAKE_EXE = os.path.join(ROOT, "tests", "cpp", "live_test_fake")
f32 = np.float32
LEFT, RIGHT = [-1.0, 0.0, 0.0], [1.0, 0.0, 0.0]


def update_samples_ref(period_ns, rate, ch):
    """periodic.rs:14-22 in f32, left to right: (as_secs_f32 * rate as f32 * channels as f32) as usize, at least 1."""
    secs = f32(period_ns // 1_000_000_000) + f32(period_ns % 1_000_000_000) / f32(1e9)
    u = f32(f32(secs) * f32(rate)) * f32(ch)
    return max(1, int(u)) if np.isfinite(u) else 1


def player_volume(lib, k):
    """live_test.cpp's volume(): the factor access k sets (0, a negative value, a dB step among others)."""
    if k % 7 == 3:
        return f32(0.0)
    if k % 5 == 1:
        return f32(-0.75)
    if k % 11 == 4:
        return f32(lib.rh_db_to_linear(-6.0))
    return f32(0.5) + f32(0.125) * f32(k % 5)


def spatial_emitter(k):
    return [f32(k % 17) * f32(0.25) - f32(2.0), f32(1.0) + f32(k % 5) * f32(0.5), f32(0.0)]


def sources(case):
    rng = np.random.default_rng(len(case))
    if case in ("player", "lowpass", "seek"):
        return [rng.uniform(-1, 1, 2 * 70_003).astype(f32)]
    if case in ("spatial", "spatial_mixer"):
        return [rng.uniform(-0.5, 0.5, 2 * 60_011).astype(f32), rng.uniform(-0.3, 0.3, 2 * 50_000).astype(f32), rng.uniform(-0.3, 0.3, 2 * 61_000).astype(f32)]
    return []  # (stereo_access, fast_access: the driver builds the reference's buffers)


SEEK_AT = 30_001  # samples served before try_seek(500 ms): inside a frame and inside an access period


def run_live(tmp_path, case, block, exe=FAKE_EXE):
    d = tmp_path / f"{case}_{block}"
    d.mkdir(exist_ok=True)
    for i, x in enumerate(sources(case)):
        x.tofile(d / f"src_{i}.f32")
    (d / "seek.txt").write_text(f"{SEEK_AT}\n")
    r = subprocess.run([exe, "run", str(d), case, str(block)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    calls = [tuple(int(v) for v in ln.split()) for ln in (d / "calls.txt").read_text().split("\n") if ln.strip()]
    got = np.fromfile(d / "out.f32", dtype=f32)
    if case == "seek":
        run_live.plain = np.fromfile(d / "plain.f32", dtype=f32)
    return got, calls


def _steps(n, U):
    return np.arange(n) // U


def expected_calls(schedule, total):
    """[(access, k)] in rodio's order for the accesses `schedule` = [(id, U)] listed from the outermost in, over a stream of `total`
    samples drained to its None: by sample, the outer access first at one sample."""
    ev = []
    for rank, (aid, U) in enumerate(schedule):
        for k in range(total // U + 1):
            ev.append((k * U, rank, aid, k))
    return [(a, k) for _, _, a, k in sorted(ev)]


def spatial_ref(lib, x, total_frames=None):
    """live_spatial (10 ms) -> live_amplify (5 ms) at 48 kHz stereo: gains of step j // 960, factor of step j // 480."""
    import ctypes as C

    fr = x.size // 2
    m = ((f32(0.0) + x[0::2][:fr]) + x[1::2][:fr]).astype(f32)
    m = (m / f32(2)).astype(f32)
    j = np.arange(2 * fr)
    kg = j // 960
    P = C.POINTER(C.c_float)
    gains = []
    for k in range(int(kg[-1]) + 1 if fr else 0):
        e, l, r = (np.ascontiguousarray(v, dtype=f32) for v in (spatial_emitter(k), LEFT, RIGHT))
        out = np.zeros(2, f32)
        assert lib.rh_spatial_gains(e.ctypes.data_as(P), l.ctypes.data_as(P), r.ctypes.data_as(P), out.ctypes.data_as(P)) == 0
        gains.append(out)
    g = np.array(gains, f32)
    vol = np.array([player_volume(lib, k) for k in range(int(j[-1]) // 480 + 1)], f32)
    return ((m[j // 2] * g[kg, j % 2]).astype(f32) * vol[j // 480]).astype(f32)


def expected_chain(O, case):
    """(samples, calls) rodio's chain gives: the adjustable stage restated in numpy f32, the fixed stages by the oracle."""
    from rodio_amd import _lib

    lib = _lib.lib
    xs = sources(case)
    if case in ("player", "lowpass", "seek"):
        x = run_live.plain if case == "seek" else xs[0]
        vol = np.array([player_volume(lib, k) for k in range(x.size // 441 + 1)], f32)
        y = (x * vol[_steps(x.size, 441)]).astype(f32)
        if case == "lowpass":
            y = O.TestSource(y, 2, 44100).low_pass(200).collect()
        return y, expected_calls([(5, 441)], x.size)
    if case == "spatial":
        y = spatial_ref(lib, xs[0])
        return y, expected_calls([(5, 480), (10, 960)], y.size)
    if case == "spatial_mixer":
        m = O.Mixer(2, 48000)
        m.add(O.TestSource(spatial_ref(lib, xs[0]), 2, 48000))
        for x in xs[1:]:
            m.add(O.TestSource(x, 2, 48000))
        return m.collect(), None
    raise ValueError(case)


def _need_fake():
    if not os.path.exists(FAKE_EXE):
        pytest.fail(f"{FAKE_EXE} is missing: run python rodio_amd/build.py")


# ------------------------------------------------------------------------------------------------------------------ tests
def test_periodic_update_samples_is_the_f32_formula(rh):
    from rodio_amd import _lib

    for want, args in ((441, (5_000_000, 44100, 2)), (220, (5_000_000, 44100, 1)), (1323, (5_000_000, 44100, 6)), (480, (5_000_000, 48000, 2)),
                       (960, (10_000_000, 48000, 2)), (2, (1_000_000_000, 1, 2)), (1, (5_000_000, 1, 1))):
        assert _lib.lib.rh_periodic_update_samples(*args) == want, args
        assert rh.periodic_update_samples(*args) == want
    for p in (0, 1, 999, 1_000_000, 5_000_000, 10_000_000, 20_833_333, 123_456_789, 1_000_000_000, 1_500_000_001, 3_000_000_000_000):
        for rate in (1, 8000, 22050, 44100, 48000, 96000, 192000):
            for ch in (1, 2, 3, 6, 8):
                assert _lib.lib.rh_periodic_update_samples(p, rate, ch) == update_samples_ref(p, rate, ch), (p, rate, ch)


def test_stepped_entries_refuse_without_init(rh):
    """Without rh_init the compute entries answer RH_ERR_NOT_INITIALIZED -- checked in a fresh process that never calls it, so that it
    holds on a box with a GPU too."""
    import sys

    code = ("import ctypes as C\nfrom rodio_amd import _lib\nb = (C.c_float * 8)()\n"
            "print(_lib.lib.rh_amplify_steps(b, b, 8, 0, 4, b, 2, None), _lib.lib.rh_channel_volume_steps(b, b, 4, 2, 2, 0, 4, b, 2, 0, 4, None, 0, None))")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    assert r.stdout.split() == ["6", "6"]


@pytest.mark.parametrize("case,channels,want_samples,want_counts", [
    ("stereo_access", 2, [10, -10, 10, -10, 20, -20], 4),  # periodic.rs:143-171: calls 1,1,2,2,3,3 -- and once more at the None (sample 6 = 3U)
    ("fast_access", 1, [10, -10, 10, -10, 20, -20], 7),    # periodic.rs:173-181: U = max(1, 0) = 1, no overflow; one call per ask
])
@pytest.mark.parametrize("block", [1, 2, 4096])
def test_reference_vectors_of_periodic_access(tmp_path, case, channels, want_samples, want_counts, block):
    _need_fake()
    got, calls = run_live(tmp_path, case, block)
    assert got.tolist() == want_samples
    assert calls == [(0, k) for k in range(want_counts)]  # one call per index, in order
    counts = [int(v) for v in (tmp_path / f"{case}_{block}" / "counts.txt").read_text().split()]
    U = 2 if case == "stereo_access" else 1
    rodio = [0] + [i // U + 1 for i in range(6)] + [want_counts]  # rodio's count after every next() (the None included)
    lookahead = 2 * block * channels + 1  # what the pump may have computed ahead of the consumer
    for c, r, i in zip(counts, rodio, range(len(rodio))):
        assert r <= c <= min(want_counts, r + lookahead // U + 1), (i, counts, rodio)
    assert counts[-1] == want_counts


@pytest.mark.parametrize("case", ["player", "lowpass", "seek", "spatial"])
@pytest.mark.parametrize("block", [256, 32768])
def test_calls_in_order_one_per_index(O, tmp_path, case, block):
    """On the fake: the closures run once per access index, in increasing order -- after try_seek and after the drain too; nested
    accesses (10 ms spatial inside a 5 ms volume) interleave by sample, the outer access first."""
    _need_fake()
    got, calls = run_live(tmp_path, case, block)
    want, want_calls = expected_chain(O, case)
    if case == "seek":
        # the count goes on over the samples served: what was computed ahead of the seek is not called again
        n = got.size
        assert calls == [(5, k) for k in range(max(n // 441, max(k for _, k in calls)) + 1)]
        assert max(k for _, k in calls) >= n // 441
    else:
        assert calls == want_calls
    assert got.shape == want.shape
    assert np.max(np.abs(got - want)) <= 1e-5


def test_refused_across_a_converter():
    _need_fake()
    r = subprocess.run([FAKE_EXE, "refuse"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, (r.stdout, r.stderr)
    assert r.stdout.split()[0] == "3" and "one sample per sample" in r.stdout  # RH_ERR_UNSUPPORTED, at build time


def test_a_channel_volume_behind_another_adjustable_stage_is_refused():
    """mono -> live_amplify -> periodic_access -> live_channel_volume({1, 1}): the channel volume counts twice the samples of the stages in
    front of it, so the schedule would not hold for them -- refused at build time."""
    _need_fake()
    r = subprocess.run([FAKE_EXE, "refuse", "cv"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, (r.stdout, r.stderr)
    assert r.stdout.split()[0] == "3" and "live_channel_volume" in r.stdout


@pytest.mark.parametrize("chain,block,bound", [("player", 256, 8), ("player", 32768, 2 * 2 * 32768 // 441 + 8), ("spatial", 256, 16),
                                               ("spatial", 32768, 2 * (2 * 2 * 32768 // 480) + 16)])
def test_steps_held_stay_within_the_lookahead(chain, block, bound):
    """A value that changes at every access over a long stream (240 s): the steps the chain holds stay within what its two blocks of
    lookahead need, and every access is called once (host time and memory grow with the stream, not with its square)."""
    _need_fake()
    r = subprocess.run([FAKE_EXE, "steps", "240", str(block), chain], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    n, calls, held = int(w[0]), int(w[2]), int(w[4])
    assert n == 2 * 44100 * 240
    want_calls = n // 441 + 1 if chain == "player" else (n // 441 + 1) + (n // 882 + 1)  # (44.1 kHz stereo: U = 441 at 5 ms, 882 at 10 ms)
    assert calls == want_calls
    assert held <= bound, r.stdout


def test_size_hint_span_and_duration_pass_through(tmp_path):
    _need_fake()
    sources("player")[0].tofile(tmp_path / "src_0.f32")
    r = subprocess.run([FAKE_EXE, "hints", str(tmp_path), "1024"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    plain = (tmp_path / "hints_plain.txt").read_text()
    assert plain == (tmp_path / "hints_live.txt").read_text()
    assert len(plain.split("\n")) > 100


@pytest.mark.parametrize("block", [64, 256, 32768])
def test_spatial_player_tail_is_one_launch_a_block(block):
    _need_fake()
    r = subprocess.run([FAKE_EXE, "launches", str(block)], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    w = r.stdout.split()
    blocks, launches = int(w[2]), int(w[4])
    assert 0 < launches <= blocks and launches >= blocks - 1, r.stdout  # (the last block of a stream that ends on a block boundary is empty)
