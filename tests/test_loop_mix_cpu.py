"""tests/loop_mix_ref.py -- the numpy restatement the GPU tests of rh_loop_mix_block compare with -- held against the oracle, no GPU: the bits
of `Mixer(ch, to_rate)` fed K unrolled passes of every loop -- `SpanSource(unrolled, ..)` where one converter chain is a constant run of the
unrolled stream (rule 1, and rule 0 with one chain per pass), `SeqSource` of the Buffered spans of every pass in turn where a pass has several
chains -- up to the chain in which the finite copy ends; and the first pass of `SamplesBuffer(..).buffered()` and `TestSource(..).buffered()`,
which is what Repeat plays.  Then the cursor: a stream cut into three unequal blocks with rh_loop_advance's cursor equals the one pass, the
cuts on a chain's verbatim last frame, on a chain's first frame, inside a chain and on the seam.  Then rh_loop_plan against what the
oracle's Buffered reports span after span, and the entry's host decisions (rodio_amd/csrc/rh_loop_mix_plan.h): tests/cpp/loop_mix_plan_test,
as built by build() and once more under -fsanitize=address,undefined."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import loop_mix_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = [(44100, 48000), (48000, 44100), (48000, 48000), (8000, 48000)]
LAYOUTS = [(1, 2), (2, 2), (2, 1), (6, 2), (2, 6)]
# (L, c, rule): every output frame verbatim; one chain a pass; chains 4, 4, 2; a tail chain of ONE frame; the grid meets the seam every time;
# drifts by one frame a chain; 4 against 10
SHAPES = [(1, 1, 0), (5, 5, 0), (10, 4, 0), (9, 4, 0), (4, 4, 1), (5, 4, 1), (10, 4, 1)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def oracle_loop(O, x, ch, rate, words, passes):
    """`passes` unrolled passes of the loop as a finite source whose chains are the loop's."""
    L, c, rule, _, _ = words
    if rule == 0 and c < L:
        parts = [(x[s * ch:(s + n) * ch], ch, rate) for s, n in R.chains_of_pass(L, c)]
        return O.SeqSource(parts * passes)
    return O.SpanSource(R.unrolled(x, ch, passes), ch, rate, c * ch)  # (rule 0 here: c == L, a pass a chain)


@pytest.mark.parametrize("ch,to_ch", LAYOUTS)
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_the_restatement_is_the_oracles_mixer(O, rate, to_rate, ch, to_ch):
    rng = np.random.default_rng(rate % 89 + 10 * ch + to_ch)
    mx, srcs, reach = O.Mixer(to_ch, to_rate), [], []
    for k, (L, c, rule) in enumerate(SHAPES):
        x = rng.uniform(-1, 1, L * ch).astype(np.float32)
        g = (0.7, -1.1, 1.0, 0.5, -0.3, 1.9, 0.25)[k]
        words, passes = [L, c, rule, 0, 0], 64 // L + 9
        mx.add(oracle_loop(O, x, ch, rate, words, passes).amplify(float(g)))
        reach.append(R.stream_out_frames(words, rate, to_rate, passes))
        srcs.append((x, g, words))
        if k == 3:  # a one-shot between the loops: it ends inside the comparison
            n = 17
            y = rng.uniform(-1, 1, n * ch).astype(np.float32)
            mx.add(O.TestSource(y, ch, rate).amplify(0.9))
            srcs.append((y, 0.9, None))
    want = mx.collect()
    M = min(reach)
    assert M >= 30 and want.size >= M * to_ch
    F, T = R.reduced(rate, to_rate)
    table = [R.Src(x, ch, rate, M if w else min(M, R.span_out(len(x) // ch, F, T)), gain=g, words=w, last=len(x) // ch - 1) for x, g, w in srcs]
    got = R.loop_mix(to_ch, to_rate, M, table)
    bad = np.flatnonzero(bits(got) != bits(want[: M * to_ch]))
    assert bad.size == 0, (int(bad[0]), got[bad[0]], want[bad[0]])


@pytest.mark.parametrize("span", ["samples_buffer", "none"])
def test_two_rodio_sized_sounds_against_the_oracles_mixer(O, span):
    """20 000 stereo frames: as a SamplesBuffer rule 1 with chains of 16384 frames of the unrolled stream, as a None-span source rule 0 with
    chains of 16384 + 3616."""
    rng = np.random.default_rng(3)
    L, ch, rate, to_rate = 20000, 2, 44100, 48000
    x = rng.uniform(-1, 1, L * ch).astype(np.float32)
    words = R.loop_plan(L * ch, ch, L * ch if span == "samples_buffer" else 0)
    assert words == [L, 16384, 1 if span == "samples_buffer" else 0, 0, 0]
    mx = O.Mixer(2, to_rate)
    if span == "samples_buffer":
        mx.add(O.SpanSource(R.unrolled(x, ch, 4), ch, rate, L * ch).amplify(0.8))
    else:
        mx.add(O.SeqSource([(x[: 32768], ch, rate), (x[32768:], ch, rate)] * 4).amplify(0.8))
    want = mx.collect()
    M = R.stream_out_frames(words, rate, to_rate, 4)
    assert M > 60000
    got = R.loop_mix(2, to_rate, M, [R.Src(x, ch, rate, M, gain=0.8, words=words)])
    assert np.array_equal(bits(got), bits(want[: 2 * M]))


@pytest.mark.parametrize("kind", ["SamplesBuffer", "TestSource"])
@pytest.mark.parametrize("n_frames", [300, 20000])
def test_the_first_pass_of_buffered(O, kind, n_frames):
    """What Repeat plays is source.buffered() (repeat.rs:14): its first pass through the mixer, up to the end of its last whole chain (the
    infinite loop never has the finite stream's end, except where a pass ends a chain: rule 0)."""
    rng = np.random.default_rng(n_frames)
    ch, rate, to_rate = 2, 44100, 48000
    x = rng.uniform(-1, 1, n_frames * ch).astype(np.float32)
    src = O.SamplesBuffer(ch, rate, x) if kind == "SamplesBuffer" else O.TestSource(x, ch, rate)
    words = R.loop_plan(x.size, ch, x.size if kind == "SamplesBuffer" else 0)
    mx = O.Mixer(2, to_rate)
    mx.add(src.buffered().amplify(-0.6))
    want = mx.collect()
    F, T = R.reduced(rate, to_rate)
    L, c, rule, _, _ = words
    M = sum(R.span_out(n, F, T) for _, n in R.chains_of_pass(L, c)) if rule == 0 else (L // c) * R.span_out(c, F, T)
    assert (rule == 1) == (kind == "SamplesBuffer" and n_frames == 20000) and want.size >= 2 * M
    if rule == 0:
        assert want.size == 2 * M  # the pass ends where its last chain ends
    got = R.loop_mix(2, to_rate, M, [R.Src(x, ch, rate, M, gain=-0.6, words=words)])
    assert np.array_equal(bits(got), bits(want[: 2 * M]))


# 44100 -> 48000, c = 4: a chain emits 5 frames (the fifth verbatim), a chain of 2 emits 3.  L = 10: rule 0 passes of 13 frames; under rule 1
# chain 2 starts at frame 8 and its output frame 12 lerps from frame 9 to frame 0.
CUTS = [(4, 5), (5, 7), (7, 12), (12, 13), (13, 26), (1, 64)]


@pytest.mark.parametrize("cuts", CUTS)
@pytest.mark.parametrize("L,c,rule", SHAPES)
def test_three_unequal_blocks_are_the_one_pass(L, c, rule, cuts):
    rng = np.random.default_rng(L + c)
    to_rate, to_ch, total = 48000, 2, 90
    specs = [(rng.uniform(-1, 1, L * ch).astype(np.float32), ch, rate, 0.5 + 0.2 * k) for k, (ch, rate) in enumerate([(2, 44100), (1, 48000), (6, 8000), (2, 96000)])]
    F, T = R.reduced(44100, 48000)
    if (L, c) == (10, 4):  # the cuts are where the comment above says
        s = R.Src(specs[0][0], 2, 44100, 14, words=[L, c, rule, 0, 0])
        ia, ib, two, _, _ = R.loop_taps(s, to_rate)
        assert not two[4] and two[5] and ia[5] == 4 and two[7]
        assert (rule == 0 and not two[12] and ia[12] == 9 and ia[13] == 0) or (rule == 1 and two[12] and ia[12] == 9 and ib[12] == 0)
    whole = R.loop_mix(to_ch, to_rate, total, [R.Src(x, ch, rate, total, gain=g, words=[L, c, rule, 0, 0]) for x, ch, rate, g in specs])
    words = [[L, c, rule, 0, 0] for _ in specs]
    parts = []
    for m0, m1 in zip((0,) + cuts, cuts + (total,)):
        parts.append(R.loop_mix(to_ch, to_rate, m1 - m0, [R.Src(x, ch, rate, m1 - m0, gain=g, words=w) for (x, ch, rate, g), w in zip(specs, words)]))
        words = [R.loop_advance(w, rate, to_rate, m1 - m0) for (_, _, rate, _), w in zip(specs, words)]
        assert all(w[3] < L and (rule == 1 or w[3] % c == 0) for w in words)
    assert np.array_equal(bits(np.concatenate(parts)), bits(whole))


# ---- the plan header ------------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "tests", "cpp", "loop_mix_plan_test")
SRC = EXE + ".cpp"
HEADER = os.path.join(ROOT, "rodio_amd", "csrc", "rh_loop_mix_plan.h")
STATUS = {0: R.OK, 1: R.INVALID, 3: R.UNSUPPORTED}


def plan_exe():
    spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "loop_mix_plan_test" in b.DRIVERS and os.path.exists(HEADER)
    b.build_driver("loop_mix_plan_test", False, lambda cmd: subprocess.check_call(cmd))  # (build() makes it; stale or missing: here)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}


def ask(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
    v = [int(t) for t in r.stdout.split()]
    return v[0], v[1:]


def buffered_spans(src):
    """What Buffered reports for one pass of a sound: current_span_len(), span after span."""
    b, out = src.buffered(), []
    while b.current_span_len():
        n = b.current_span_len()
        assert len(b.pull(n)) == n
        out.append(n)
    return out


# (n_samples, channels, what the fresh sound answers to current_span_len(): "none", "samples_buffer", or a constant)
PLANS = [(20000, 2, "none"), (40000, 2, "none"), (32768, 2, "none"), (32770, 2, "none"), (20000, 2, "samples_buffer"), (40000, 2, "samples_buffer"), (32768, 1, "samples_buffer"),
         (32769, 1, "samples_buffer"), (88200, 2, "samples_buffer"), (40000, 2, 1152), (1000, 2, 1152), (40000, 2, 32768), (30000, 6, "none"), (60000, 4, "samples_buffer"),
         (60000, 6, "none"), (60000, 6, "samples_buffer"), (60000, 3, "samples_buffer"), (60000, 5, "none"), (70000, 7, "none"), (40000, 2, 1001)]


@pytest.mark.parametrize("n,ch,span", PLANS)
def test_the_plan_is_what_buffered_reports(O, n, ch, span):
    x = np.zeros(n, np.float32)
    src = O.TestSource(x, ch, 44100) if span == "none" else (O.SamplesBuffer(ch, 44100, x) if span == "samples_buffer" else O.SpanSource(x, ch, 44100, span))
    span_len = {"none": 0, "samples_buffer": n}.get(span, span)
    assert (src.current_span_len() or 0) == span_len
    spans = buffered_spans(src)
    assert sum(spans) == n
    # Repeat over these spans: ONE span longer than a chain is cut every 32768 samples of the unrolled stream (rule 1); otherwise a span a chain
    if len(spans) == 1 and spans[0] > R.CHAIN_SAMPLES:
        chain, rule = R.CHAIN_SAMPLES, 1
    else:
        assert all(s == spans[0] for s in spans[:-1]) and spans[-1] <= spans[0] <= R.CHAIN_SAMPLES
        chain, rule = spans[0], 0
    want = R.UNSUPPORTED if n % ch or chain % ch else [n // ch, chain // ch, rule, 0, 0]
    assert R.loop_plan(n, ch, span_len) == want
    st, words = ask(plan_exe(), "plan", n, ch, span_len)
    assert (STATUS[st] if st else words) == want
    if want != R.UNSUPPORTED and rule == 0:  # the tail chain is the last span
        assert spans[-1] == (((n // ch) % (chain // ch)) or chain // ch) * ch


def test_spans_that_are_no_sounds_span():
    for n, ch, span_len in [(40000, 2, 50000), (40000, 2, 32769)]:
        assert R.loop_plan(n, ch, span_len) == R.UNSUPPORTED and STATUS[ask(plan_exe(), "plan", n, ch, span_len)[0]] == R.UNSUPPORTED


def test_the_headers_cursor_is_the_walked_cursor():
    rng = np.random.default_rng(1)
    for L, c, rule in SHAPES + [(20000, 16384, 1), (20000, 16384, 0)]:
        for rate, to_rate in RATES:
            w = [L, c, rule, 0, 0]
            for _ in range(4):
                n = int(rng.integers(0, 70 if L < 100 else 70000))
                want = R.loop_advance(w, rate, to_rate, n)
                st, got = ask(plan_exe(), "advance", *w, rate, to_rate, n)
                assert st == 0 and got == want, (w, rate, to_rate, n)
                w = want


def test_reciprocals_positions_refusals_bounds_and_launches():
    n = run(plan_exe())
    assert n["failures"] == 0
    # the run was not vacuous
    assert n["divs"] > 100000 and n["spans"] == 290 and n["located"] >= 700 and n["cuts"] == 225 and n["plans"] == 26 and n["refusals"] == 25 and n["bounds"] == 8 and n["launches"] == 7
    assert run(plan_exe(), 2, 150)["failures"] == 0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Host code with a main of its own: built with the sanitizers and run as it is."""
    exe = str(tmp_path / "loop_mix_plan_test_san")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rodio_amd", "csrc"), SRC, "-o", exe])
    n = run(exe, 4, 150)
    assert n["failures"] == 0 and n["refusals"] == 25 and n["bounds"] == 8 and n["located"] >= 400
