"""GpuMixer of more than two channels with Options::wide_filters, host logic (no GPU): filtered and plain continuous sources of three
layouts in one-launch generations over the CPU stand-in of rh_wide_mix_block_filtered (tests/cpp/fake_widemix_filtered.cpp, which runs
every filter in the reference's order) -- a source that joins the running mixer, sources that end inside a block.  Every pulled sample
against the oracle's mixer bit for bit, size_hint() in front of every sample; with the option off the mixer is today's.  The helpers are
shared with tests/test_gpu_widemix_filtered.py (the same driver against the library)."""
import json
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXE = os.path.join(ROOT, "tests", "cpp", "wide_filtered_test_fake")
f32 = np.float32

# (channels, rate, gain, frames, kind, freq, q): three layouts, filters of three kinds interleaved with plain sources; the last one joins late
SPEC = [
    (6, 44100, 0.8, 5000, 0, 1000, 0.5),
    (2, 48000, 1.0, 7000, -1, 0, 0.5),
    (1, 22050, -0.6, 1500, 1, 2000, 0.5),
    (6, 48000, 0.5, 3100, 0, 1000, 0.5),
    (2, 44100, 0.9, 2600, 0, 300, 0.9),
    (6, 44100, 0.7, 2000, 1, 2000, 0.5),
]
N_FIRST, N_LATE = 5, 1
BLOCK = 1024


def _bits(a):
    return np.ascontiguousarray(a, dtype=f32).view(np.uint32)


def _inputs():
    rng = np.random.default_rng(4100)
    return [rng.uniform(-0.25, 0.25, ch * n).astype(f32) for ch, _, _, n, _, _, _ in SPEC]


def _source(O, x, spec):
    ch, rate, gain, _, kind, freq, q = spec
    s = O.TestSource(x, ch, rate)
    if gain != 1.0:
        s = s.amplify(float(f32(gain)))
    if kind < 0:
        return s
    u = O.UniformSourceIterator(s, 6, 48000)
    return u.low_pass(freq, q) if kind == 0 else u.high_pass(freq, q)


def _oracle(O, xs, pull_first):
    """The oracle's mixer driven as the driver drives GpuMixer: size_hint() in front of every sample and behind the last, the late source
    added after pull_first samples."""
    m = O.Mixer(6, 48000)
    for i in range(N_FIRST):
        m.add(_source(O, xs[i], SPEC[i]))
    out, hints, joined = [], [], False
    while True:
        if not joined and len(out) == pull_first:
            for i in range(N_FIRST, N_FIRST + N_LATE):
                m.add(_source(O, xs[i], SPEC[i]))
            joined = True
        lo, hi = m.rx.size_hint()
        hints += [lo, -1 if hi is None else hi]
        v = m.next()
        if v is None:
            break
        out.append(v)
    return np.asarray(out, dtype=f32), np.asarray(hints, dtype=np.int64)


def _run(tmp_path, xs, pull_first, on, exe=EXE):
    if not os.path.exists(exe):
        pytest.fail(os.path.relpath(exe, ROOT) + " is missing: run python rodio_amd/build.py")
    for i, x in enumerate(xs):
        x.tofile(tmp_path / f"src_{i}.f32")
    (tmp_path / "spec.txt").write_text("".join(f"{ch} {rate} {float(f32(g))!r} {kind} {freq} {q}\n" for ch, rate, g, _, kind, freq, q in SPEC))
    r = subprocess.run([exe, str(tmp_path), str(N_FIRST), str(N_LATE), "6", "48000", str(BLOCK), str(pull_first), "1" if on else "0"], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr
    return np.fromfile(tmp_path / "out.f32", dtype=f32), np.fromfile(tmp_path / "hints.i64", dtype=np.int64), json.loads((tmp_path / "stats.txt").read_text())


@pytest.fixture(scope="module")
def reference(O):
    xs = _inputs()
    return xs, {p: _oracle(O, xs, p) for p in (6 * 2500 + 1, 11)}


@pytest.mark.parametrize("pull_first", [6 * 2500 + 1, 11])
def test_filtered_wide_generations_are_the_oracles_mixer_bit_for_bit(reference, tmp_path, pull_first):
    """Option on: no chain is built, every block of a generation with a filter runs rh_wide_mix_block_filtered, the late source is
    admitted at the next frame (mixer.rs:175-183) with a fresh filter state, the sources of 1 500 .. 7 000 frames end inside blocks of
    1 024 -- and every sample and every size_hint() is the oracle's."""
    xs, refs = reference
    want, want_hints = refs[pull_first]
    got, hints, st = _run(tmp_path, xs, pull_first, True)
    assert st["chains"] == 0 and st["wide_filtered_blocks"] > 0 and st["wide_fused_blocks"] >= st["wide_filtered_blocks"], st
    assert st["total_duration_none"] == 1  # mixer.rs:104-106
    assert got.shape == want.shape, (got.shape, want.shape)
    assert np.array_equal(_bits(got), _bits(want)), int(np.argmax(_bits(got) != _bits(want)))
    assert len(hints) == len(want_hints) == 2 * (len(got) + 1)
    bad = np.nonzero(hints != want_hints)[0]
    assert len(bad) == 0, ("sample", int(bad[0]) // 2, hints[bad[0] // 2 * 2:bad[0] // 2 * 2 + 2].tolist(), want_hints[bad[0] // 2 * 2:bad[0] // 2 * 2 + 2].tolist(), len(bad))


def test_option_off_keeps_the_chains(reference, tmp_path):
    """Option off (the default): a filter on one source of a generation makes chains of all of them, as before -- no block goes through
    either one-launch entry, a chain per source, and (the stand-in filters in the reference's order) the oracle's samples."""
    xs, refs = reference
    want, _ = refs[11]
    got, _, st = _run(tmp_path, xs, 11, False)
    assert st["wide_filtered_blocks"] == 0 and st["wide_fused_blocks"] == 0 and st["chains"] == len(SPEC), st
    assert got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want))
