"""Source::mix and Source::take_crossfade_with, host logic (no GPU): the CPU restatement of Mix (mix.rs:10-22,43-53) over the oracle's
UniformSourceIterator -- the oracle has no Mix of its own -- against the reference's own crossfade vectors (crossfade.rs:46-80) and
against the oracle's reverb (which IS Mix(x, Delay(Amplify(x))), source/mod.rs:628-634); the C++ mirror's Mix and Crossfade
(include/rodio_hip.hpp) on the CPU stand-in (tests/cpp/fake_mix.cpp); the Python classes' host-side refusals.  The helpers here are
shared with tests/test_gpu_mix.py."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.abspath(__file__)).rsplit(os.sep, 1)[0]
f32 = np.float32
MS = 1_000_000


def bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def same_bits(a, b):
    a, b = np.asarray(a, dtype=f32), np.asarray(b, dtype=f32)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


# ---- the restatement ---------------------------------------------------------------------------------------------------------------
def mix_rows(ua, ub):
    """Mix::next (mix.rs:43-53) over the two uniformised streams: s1 + s2 while both run, then the longer one's rest verbatim."""
    ua, ub = np.asarray(ua, dtype=f32), np.asarray(ub, dtype=f32)
    n = min(ua.size, ub.size)
    with np.errstate(invalid="ignore", over="ignore"):
        head = (ua[:n] + ub[:n]).astype(f32)
    return np.concatenate([head, ua[n:] if ua.size > n else ub[n:]])


def mix_restated(O, a, b):
    """Mix::new (mix.rs:10-22): channels and rate are a's; both inputs go through UniformSourceIterator::new(_, channels, rate)."""
    ch, rate = a.channels(), a.sample_rate()
    return mix_rows(O.UniformSourceIterator(a, ch, rate).collect(), O.UniformSourceIterator(b, ch, rate).collect())


def crossfade_restated(O, a, b, duration_ns):
    """crossfade.rs:10-23: mix(a.take_duration(d) with set_filter_fadeout(), b.take_duration(d).fade_in(d))."""
    return mix_restated(O, a.take_duration(duration_ns, True), b.take_duration(duration_ns).fade_in(duration_ns))


def signal(n, seed):
    """n samples in [-1, 1), seeded."""
    return np.random.default_rng(seed).uniform(-1.0, 1.0, n).astype(f32)


# ---- the restatement against the reference's vectors -----------------------------------------------------------------------------
def dummy_source(O, length):  # crossfade.rs:40-43
    return O.SamplesBuffer(1, 1, np.arange(1, length + 1, dtype=f32))


CROSSFADE_D = 5_000_000_001  # Duration::from_secs(5) + Duration::from_nanos(1)


def test_restatement_crossfade_with_self(O):  # crossfade.rs:46-63
    got = crossfade_restated(O, dummy_source(O, 10), dummy_source(O, 10), CROSSFADE_D)
    assert got.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]


def test_restatement_crossfade_with_zero(O):  # crossfade.rs:66-80 (Zero: endless silence; ten samples of it outlast the duration)
    got = crossfade_restated(O, dummy_source(O, 10), O.TestSource(np.zeros(10, f32), 1, 1), CROSSFADE_D)
    assert got.size == 5
    assert np.all(np.abs(got - np.array([1.0, 2.0 * 0.8, 3.0 * 0.6, 4.0 * 0.4, 5.0 * 0.2])) < 1e-6)


@pytest.mark.parametrize("channels,delay_ns", [(2, 7 * MS), (2, 7 * MS + 10_417), (1, 3 * MS)])
def test_restatement_reverb_identity(O, channels, delay_ns):
    """reverb(d, g) = Mix(x, Delay(Amplify(x, g), d)) (source/mod.rs:628-634): the oracle's own reverb has the restatement's bits --
    an odd delay (a mix that ends inside a frame) included."""
    x = signal(3000 * channels, 11)
    x[5] = -0.0
    want = O.TestSource(x, channels, 48000).reverb(delay_ns, 0.3).collect()
    got = mix_restated(O, O.TestSource(x, channels, 48000), O.TestSource(x, channels, 48000).amplify(0.3).delay(delay_ns))
    assert same_bits(got, want)
    assert got.size == x.size + O.delay_samples(delay_ns, 48000, channels)


def test_restatement_arms(O):
    """-0.0 + -0.0 stays -0.0 (no leading zero), and the longer side's rest is verbatim: a -0.0 and a NaN payload keep their bits."""
    a = np.array([-0.0, 1.0, -0.0], f32)
    b = np.array([-0.0, 2.0, 0.0, -0.0, 0.0], f32)
    b.view(np.uint32)[4] = 0x7FC12345
    got = mix_restated(O, O.TestSource(a, 1, 8000), O.TestSource(b, 1, 8000))
    assert bits(got).tolist() == [0x80000000, bits(f32(3.0)).item(), 0, 0x80000000, 0x7FC12345]


# ---- the Python classes' host-side refusals ---------------------------------------------------------------------------------------
def test_python_classes_host_side(rh):
    src = rh.GpuSource(None, 2, 48000)  # (no device memory: every refusal below comes before the first call into the library)
    with pytest.raises(TypeError):
        src.mix([0.0, 1.0])
    with pytest.raises(TypeError):
        src.take_crossfade_with(None, MS)
    with pytest.raises(ValueError):
        src.take_crossfade_with(src, -1)
    with pytest.raises(ValueError):
        rh.crossfade_batch([src], [], MS)
    with pytest.raises(TypeError):
        rh.crossfade_batch([src], [3], MS)
    with pytest.raises(ValueError):
        rh.crossfade_batch([src], [src], -5)
    assert rh.crossfade_batch([], [], MS) == []
    assert rh._lib.CROSSFADE_PAIR_WORDS == 11


CROSSFADE_CASES = {  # name: (a samples (stereo, 48 kHz), b samples (mono, 44.1 kHz), duration)
    "50ms": (6000, 3000, 50 * MS),
    "cut_frame": (6000, 3000, 50 * MS + 10_416),  # the duration expires inside a frame of a
    "800ms": (80000, 40000, 800 * MS),            # b crosses a chain restart at 32 768 samples
    "500us": (6000, 3000, 500_000),               # the 0 / 0 fade-out
    "0ns": (6000, 3000, 0),
    "a_short": (1000, 3000, 50 * MS),
    "b_short": (6000, 500, 50 * MS),
}


def crossfade_case(O, name):
    """(a, b, duration, restated crossfade) of a case: stereo 48 kHz into mono 44.1 kHz, seeded."""
    na, nb, d = CROSSFADE_CASES[name]
    a, b = signal(na, 21), signal(nb, 22)
    return a, b, d, crossfade_restated(O, O.TestSource(a, 2, 48000), O.TestSource(b, 1, 44100), d)


def test_restatement_crossfade_lengths(O):
    n = {k: crossfade_case(O, k)[3].size for k in CROSSFADE_CASES}
    assert n["50ms"] == 4800 and n["cut_frame"] == 4801 and n["800ms"] == 76804 and n["0ns"] == 0 and n["a_short"] == 4800 and n["b_short"] == 4800
    x = crossfade_case(O, "500us")[3]
    assert x.size == 48 and np.all(np.isnan(x))  # x * 0 / 0 on every sample of a, which outlasts b here


def test_library_shapes_and_refusals(rh, O):
    """rh_crossfade_out_samples and rh_uniform_row_out_samples are host arithmetic: the counts of the restatement, and the refusals."""
    C = rh._lib.C
    m = C.c_uint64(0)

    def out(na, ca, ra, nb, cb, rb, d, span=0):
        p = (C.c_uint64 * 11)(0, na, ca, ra, 0, nb, cb, rb, span, 0, 0)
        st = rh.lib.rh_crossfade_out_samples(p, d, C.byref(m))
        return st, m.value

    for name, (na, nb, d) in CROSSFADE_CASES.items():
        assert out(na, 2, 48000, nb, 1, 44100, d) == (0, crossfade_case(O, name)[3].size), name
    for bad in [(1, 0, 48000, 1, 1, 44100), (1, 2, 0, 1, 1, 44100), (1, 2, 48000, 1, 0, 44100), (1, 2, 48000, 1, 1, 0)]:
        assert out(*bad, MS)[0] == 1
    # UniformSourceIterator over a row: spans of 1000 samples of a 6-channel source cut every chain inside a frame
    for n, fc, fr, tc, tr, span, src in [(6000, 6, 48000, 6, 48000, 1000, O.SpanSource), (5004, 6, 48000, 1, 8000, 1000, O.SpanSource), (4001, 2, 44100, 6, 48000, 1000, O.SpanSource),
                                         (100, 1, 44100, 2, 48000, 0, None), (40001, 2, 44100, 2, 48000, 0, None), (70000, 2, 44100, 2, 48000, 70000, O.SpanSource)]:
        want = O.UniformSourceIterator(src(signal(n, 5), fc, fr, span) if src else O.TestSource(signal(n, 5), fc, fr), tc, tr).collect().size
        assert rh.lib.rh_uniform_row_out_samples(n, fc, fr, tc, tr, span, C.byref(m)) == 0 and m.value == want, (n, fc, fr, tc, tr, span)
    assert rh.lib.rh_uniform_row_out_samples(100, 0, 48000, 6, 48000, 0, C.byref(m)) == 1


# ---- the C++ mirror: Mix and Crossfade of include/rodio_hip.hpp ------------------------------------------------------------------
def mix_exe(fake):
    return os.path.join(ROOT, "tests", "cpp", "mix_mirror_test_fake" if fake else "mix_mirror_test")


def run_mix(fake, *args):
    r = subprocess.run([mix_exe(fake), *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out = {}
    for line in r.stdout.splitlines():
        k, v = line.split(" ", 1)
        out.setdefault(k, []).append(v)
    return out


def oracle_source(O, x, ch, rate, span):
    """span: -1 a TestSource (None), -2 a SamplesBuffer, > 0 a constant Some(span) -- the driver's codes."""
    return O.SamplesBuffer(ch, rate, x) if span == -2 else O.SpanSource(x, ch, rate, span) if span > 0 else O.TestSource(x, ch, rate)


def restated_sides(O, kind, a, fa, b, fb, d):
    """The two uniformised inputs of the Mix (fresh oracle sources): fa / fb = (channels, rate, span)."""
    sa, sb = oracle_source(O, a, *fa), oracle_source(O, b, *fb)
    if kind == "crossfade":
        sa, sb = sa.take_duration(d, True), sb.take_duration(d).fade_in(d)
    return O.UniformSourceIterator(sa, fa[0], fa[1]), O.UniformSourceIterator(sb, fa[0], fa[1])


def check_mirror_run(fake, O, tmp_path, kind, a, fa, b, fb, d, block_frames, pull):
    """Mix / Crossfade of two host-fed sources through the driver against the restatement: the samples, and with pull == 1 (one
    sample at a time) the trait's answers at every position."""
    a.tofile(tmp_path / "a.f32"), b.tofile(tmp_path / "b.f32")
    o = run_mix(fake, "run", tmp_path, kind, *fa, *fb, d, block_frames, pull, 0)
    got = np.fromfile(tmp_path / "out.f32", dtype=f32)
    ua, ub = restated_sides(O, kind, a, fa, b, fb, d)
    da, db = ua.total_duration(), ub.total_duration()
    assert o["format"] == [f"{fa[0]} {fa[1]}"] and o["seek"] == ["0"]  # try_seek: NotSupported (mix.rs:116-120)
    assert o["duration"] == [str(max(da, db) if da is not None and db is not None else -1)]  # mix.rs:104-112
    if pull:
        lows, xs, a_runs, b_runs = [], [], True, True
        while True:  # (max(lower1, lower2), None) where the consumer stands (mix.rs:56-67)
            # An input that has ended counts 0, which is what GpuSource::uniform answers there and what Mix is specified to take.  (rodio's
            # converter -- and the oracle's -- keeps answering a stale (to - position) * channels of its last chunk after its None,
            # sample_rate.rs:204-238: 318 here, for a stream that has nothing left.)
            lows.append(max(ua.size_hint()[0] if a_runs else 0, ub.size_hint()[0] if b_runs else 0))
            x, y = ua.pull(1), ub.pull(1)
            a_runs, b_runs = a_runs and len(x) > 0, b_runs and len(y) > 0
            if not len(x) and not len(y):
                break
            xs.append(mix_rows(x, y))
        want = np.concatenate(xs) if xs else np.empty(0, f32)
        assert o["spans_some"] == ["0"] and o["uppers_some"] == ["0"]  # current_span_len() is None (mix.rs:83-91), no upper bound
        assert np.array_equal(np.fromfile(tmp_path / "lower.u64", dtype=np.uint64), np.array(lows, dtype=np.uint64))
    else:
        want = mix_rows(ua.collect(), ub.collect())
    assert same_bits(got, want), (kind, fa, fb, d, block_frames, pull, got.size, want.size)
    return got


MIRROR_MIX = {  # name: (a samples, (channels, rate, span)), (b ...)
    "a_ends_first": ((3000, (2, 48000, -1)), (5000, (1, 44100, -1))),
    "b_ends_first": ((12000, (2, 48000, -1)), (3000, (1, 44100, -1))),
    "buffers": ((6000, (2, 48000, -2)), (9000, (2, 44100, -2))),     # SamplesBuffers: both durations known -> the larger
    "spans": ((6000, (2, 48000, 1000)), (5000, (1, 44100, 1000))),
    "wide": ((3000, (1, 8000, -1)), (30000, (6, 48000, 1000))),        # six channels in spans of 1000 samples: every chain cuts a frame
}


@pytest.mark.parametrize("name", list(MIRROR_MIX))
@pytest.mark.parametrize("block_frames,pull", [(1000, 0), (4096, 0), (4096, 1)])
def test_cpp_mix_on_cpu_stand_in(O, name, block_frames, pull, tmp_path):
    (na, fa), (nb, fb) = MIRROR_MIX[name]
    check_mirror_run(True, O, tmp_path, "mix", signal(na, 71), fa, signal(nb, 72), fb, 0, block_frames, pull)


@pytest.mark.parametrize("name", list(CROSSFADE_CASES))
@pytest.mark.parametrize("block_frames,pull", [(1000, 0), (4096, 0), (4096, 1)])
def test_cpp_crossfade_on_cpu_stand_in(O, name, block_frames, pull, tmp_path):
    na, nb, d = CROSSFADE_CASES[name]
    got = check_mirror_run(True, O, tmp_path, "crossfade", signal(na, 21), (2, 48000, -1), signal(nb, 22), (1, 44100, -1), d, block_frames, pull)
    assert same_bits(got, crossfade_case(O, name)[3])


def check_mirror_endless(fake, O, tmp_path, block_frames):
    """b endless (the samples repeat) under an outer take_duration: the Mix is the head of a chain."""
    a, b = signal(3000, 81), signal(441, 82)
    a.tofile(tmp_path / "a.f32"), b.tofile(tmp_path / "b.f32")
    take = 200 * MS
    run_mix(fake, "run", tmp_path, "mix", 2, 48000, -1, 1, 44100, -3, 0, block_frames, 0, take)
    got = np.fromfile(tmp_path / "out.f32", dtype=f32)
    mixed = mix_restated(O, O.TestSource(a, 2, 48000), O.TestSource(np.tile(b, 30), 1, 44100))
    want = O.TestSource(mixed, 2, 48000).take_duration(take).collect()
    assert want.size == 19202 and same_bits(got, want)  # 19201 samples admitted, and the silence that completes the frame


@pytest.mark.parametrize("block_frames", [1000, 4096])
def test_cpp_mix_endless_b_on_cpu_stand_in(O, block_frames, tmp_path):
    check_mirror_endless(True, O, tmp_path, block_frames)


def check_mirror_generators(fake, tmp_path):
    """SineWave(440).mix(white noise) under take_duration through a chain: nothing uploaded, and the host's own next() of the two
    generators, added, within the bound the generators' tests hold the device's sine to (2.4e-7: its last bit); the noise is exact."""
    o = run_mix(fake, "generators", tmp_path)
    dev, twin, host = (np.fromfile(tmp_path / f, dtype=f32) for f in ("dev.f32", "twin.f32", "host.f32"))
    assert o["uploaded"] == ["0 0"] and int(o["generated"][0].split()[0]) >= 4800 and int(o["generated"][0].split()[1]) >= 9600
    assert dev.size == twin.size == host.size == 4800
    assert same_bits(dev, twin)  # the Mix pulled on the host reads the same device blocks
    err = np.max(np.abs(dev.astype(np.float64) - host.astype(np.float64)))
    print("max |device - host next()|:", err)
    assert err <= 2.4e-7  # the bound the generators' tests hold the device's sine to
    return dev


def test_cpp_mix_of_generators_on_cpu_stand_in(tmp_path):
    check_mirror_generators(True, tmp_path)


def check_mirror_host_fed(fake, O, block_frames, tmp_path):
    (na, fa), (nb, fb) = MIRROR_MIX["b_ends_first"]
    check_mirror_run(fake, O, tmp_path, "mix", signal(na, 71), fa, signal(nb, 72), fb, 0, block_frames, 0)
    na, nb, d = CROSSFADE_CASES["800ms"]
    check_mirror_run(fake, O, tmp_path, "crossfade", signal(na, 21), (2, 48000, -1), signal(nb, 22), (1, 44100, -1), d, block_frames, 0)
    check_mirror_endless(fake, O, tmp_path, block_frames)


def check_mirror_mixer(fake, tmp_path):
    """GpuMixer::add(Mix) equals adding the Mix's collected samples as a host source, bit for bit; a Mix of generators inside a chain
    enters the mixer with nothing uploaded."""
    signal(20000, 91).tofile(tmp_path / "a.f32"), signal(6000, 92).tofile(tmp_path / "b.f32")
    o = run_mix(fake, "mixer", tmp_path)
    a, b, c = (np.fromfile(tmp_path / f, dtype=f32) for f in ("mix.f32", "host.f32", "collected.f32"))
    assert c.size == 20000 and a.size >= 20000 and np.abs(a).max() > 0.1
    assert same_bits(a, b)
    assert same_bits(a[:20000], (f32(0.0) + c * f32(0.5)).astype(f32))  # Amplify, then the mixer's sum from 0.0
    gen = np.fromfile(tmp_path / "gen.f32", dtype=f32)
    assert o["uploaded_gen"] == ["0"] and gen.size == 4800 and np.abs(gen).max() > 0.1


def test_cpp_mixer_add_mix_on_cpu_stand_in(tmp_path):
    check_mirror_mixer(True, tmp_path)
