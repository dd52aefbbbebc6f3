"""tests/clip_mix_ref.py -- the numpy restatement the GPU tests of rh_clip_mix_block compare with -- held against the oracle, no GPU: every
case of CASES as `UniformSourceIterator(src.amplify(g).take_duration(D, fade).delay(d))` over a `TestSource` (answers None), a
`SamplesBuffer` (answers its whole length) or, for an in-point, a sliced sound given as `SpanSource(.., span_len = whole length)`; all frames,
bitwise (NaN positions where the duration is under 1 ms); then the cases of a mixer's format in ONE oracle `Mixer` with plain sources
between the clips.  Then rh_clip_plan's refusals, the cursor (a stream cut into unequal blocks equals the one pass), and the entry's host
decisions (rodio_amd/csrc/rh_clip_mix_plan.h): tests/cpp/clip_mix_plan_test, as built by build() and once more under
-fsanitize=address,undefined."""
import importlib.util
import os
import shutil
import subprocess

import numpy as np
import pytest

import clip_mix_ref as R
import wide_positions as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(got, want):
    """Bitwise, except that NaN answers NaN whatever the payload."""
    got, want = np.ascontiguousarray(got, np.float32).reshape(-1), np.ascontiguousarray(want, np.float32).reshape(-1)
    if got.size != want.size:
        return False
    nan = np.isnan(want)
    return bool(np.array_equal(np.isnan(got), nan) and np.array_equal(bits(got)[~nan], bits(want)[~nan]))


def ns_for(samples, ch, rate):
    """The shortest duration Delay turns into `samples` zeros."""
    ns = -(-samples * 10**9 // (ch * rate))
    assert R.delay_samples(ns, ch, rate) == samples
    return ns


def take_for(samples, ch, rate, extra=0):
    """A duration that admits exactly `samples` samples."""
    ns = samples * R.ns_per_sample(ch, rate) + extra
    assert ns // R.ns_per_sample(ch, rate) == samples
    return ns


class Case:
    """One clip: a sound of n samples (`kind`: "test" answers None, "buffer" its whole length), `skip` samples of it in front of the
    in-point, Z zeros of delay, a take that admits `take` samples (None: no take; an int: that many; ("ns", x): that duration)."""

    def __init__(self, name, n, Z, take=None, fade=False, kind="buffer", ch=2, rate=44100, to_ch=2, to_rate=48000, gain=0.8, skip=0):
        self.name, self.n, self.Z, self.fade, self.kind, self.ch, self.rate, self.to_ch, self.to_rate, self.gain, self.skip = name, n, Z, fade, kind, ch, rate, to_ch, to_rate, gain, skip
        self.delay_ns = ns_for(Z, ch, rate)
        self.take_ns = None if take is None else (take[1] if isinstance(take, tuple) else take_for(take, ch, rate, 37))
        rng = np.random.default_rng(n + 3 * Z + ch)
        self.sound = rng.uniform(-1, 1, n).astype(np.float32)
        if n > 8:  # zeros of both signs among the samples
            z = rng.integers(0, n, 4)
            self.sound[z[:2]], self.sound[z[2:]] = 0.0, -0.0
        self.x = self.sound[skip:]  # what the clip's `data` points at
        self.span_len = 0 if kind == "test" else n

    def words(self):
        return R.clip_plan(self.x.size, self.ch, self.rate, self.span_len, self.delay_ns, self.take_ns, self.fade)

    def oracle(self, O):
        if self.kind == "test":
            src = O.TestSource(self.x, self.ch, self.rate)
        elif self.skip:
            src = O.SpanSource(self.x, self.ch, self.rate, self.n)  # a skipped SamplesBuffer goes on answering its whole length
        else:
            src = O.SamplesBuffer(self.ch, self.rate, self.x)
        src = src.amplify(float(self.gain))
        if self.take_ns is not None:
            src = src.take_duration(self.take_ns, self.fade)
        return src.delay(self.delay_ns)

    def src(self, frames=None, done=0):
        w = self.words()
        total = R.clip_out_frames(w, self.ch, self.rate, self.to_rate)
        w[5], w[6] = done, total
        return R.Src(self.x, self.ch, self.rate, total - done if frames is None else frames, gain=self.gain, words=w)


LARGE_F, LARGE_T = WP.BY_ID["65521-48000"], WP.BY_ID["48000-65521"]  # F = 65521, T = 65521: next to 2^16

# The smallest sizes at which the rule can go wrong.  Stereo 44.1 -> 48 kHz unless said otherwise; 88.2 samples a millisecond.
CASES = [
    Case("no delay, a grid line inside the sound", 40000, 0),
    Case("odd delay, odd sound that ends before its take: the channels shift", 4001, 777, take=9000, kind="test"),
    Case("odd delay, a take that expires inside a frame, fading", 6000, 1001, take=3001, fade=True),
    Case("delay just below a grid line", 5000, 32766),
    Case("delay on a grid line, with a take", 5000, 32768, take=4000, fade=True),
    Case("delay just above a grid line", 5000, 32770, kind="test", take=6000),
    Case("odd delay beyond two grid lines", 3001, 70001, take=5000, kind="test"),
    Case("take expiring in the first chain", 50000, 1000, take=2000),
    Case("take expiring in a later chain, fading across grid lines", 100000, 100, take=70000, fade=True, gain=-1.1),
    Case("a take of nothing behind a delay: zeros only", 3000, 500, take=0),
    Case("a take of nothing and no delay: no frame at all", 3000, 0, take=0, fade=True),
    Case("the sound ends before the take, in the second chain", 40000, 0, take=60000, kind="test", fade=True),
    Case("a short SamplesBuffer pushed across a grid line", 20000, 26460),
    Case("rule C with an odd delay", 9001, 5001, kind="test"),
    Case("rule C across grid lines: ONE chain", 80000, 40000, kind="test"),
    Case("a duration under a millisecond, fading: x * 0 / 0", 3000, 11, take=("ns", 900_000), fade=True),
    Case("a take of 58 days, fading: more than 2^32 milliseconds remain", 5001, 301, take=("ns", 5 * 10**15), fade=True, kind="test"),
    Case("an in-point, rule G", 50000, 3000, take=40000, fade=True, skip=10000),
    Case("an in-point without a take", 50000, 29999, skip=40001),
    Case("48 -> 44.1 kHz", 40000, 30001, take=9999, fade=True, rate=48000, to_rate=44100),
    Case("equal rates", 40000, 32001, take=5001, fade=True, rate=48000, to_rate=48000),
    Case("equal rates, rule C", 40000, 101, kind="test", rate=48000, to_rate=48000, skip=101),
    Case("F near 2^16", 40000, 32000, take=9000, fade=True, rate=LARGE_F.from_rate, to_rate=LARGE_F.to_rate),
    Case("T near 2^16", 40000, 501, kind="test", take=30001, rate=LARGE_T.from_rate, to_rate=LARGE_T.to_rate),
    Case("mono into stereo", 40000, 32767, take=3000, fade=True, ch=1),
    Case("mono into stereo, rule C", 5000, 33, kind="test", ch=1),
    Case("stereo into mono", 40000, 1001, take=36001, fade=True, to_ch=1),
    Case("stereo into six", 6000, 32769, take=5001, to_ch=6),
    Case("six into stereo, one chain", 30000, 2766, take=18000, fade=True, ch=6),
    Case("six into stereo, a delay that is no whole frame", 12000, 3001, take=5999, kind="test", ch=6),
]
IDS = [c.name for c in CASES]


def test_the_cases_are_what_they_say():
    by = {c.name: c for c in CASES}
    for c in CASES:
        w = c.words()
        assert isinstance(w, list), (c.name, w)  # no case of the list is refused
        assert w[1] == c.Z and (3000 <= c.n <= 100000)
    w = by["odd delay, a take that expires inside a frame, fading"].words()
    assert w[1] % 2 == 1 and w[2] == 3001 and (w[1] + w[2]) % 2 == 0
    w = by["odd delay, odd sound that ends before its take: the channels shift"].words()
    assert w[2] == 4001 and w[3] // R.ns_per_sample(2, 44100) == 9000
    assert by["take expiring in a later chain, fading across grid lines"].words()[2] == 70000
    assert by["the sound ends before the take, in the second chain"].words()[2] == 40000
    assert by["rule C across grid lines: ONE chain"].words()[0] == R.RULE_C and by["a short SamplesBuffer pushed across a grid line"].words()[0] == R.RULE_G
    assert by["a duration under a millisecond, fading: x * 0 / 0"].words()[2] == 79
    assert by["six into stereo, one chain"].words()[1] + 18000 <= 32768
    # a fade-out step between the two taps of a lerp: remaining milliseconds differ between a frame and the next
    c = by["take expiring in a later chain, fading across grid lines"]
    k = np.arange(c.words()[2], dtype=np.int64)
    ms = (c.take_ns - k * R.ns_per_sample(2, 44100)) // R.NS_PER_MS
    assert np.count_nonzero(ms[2:] != ms[:-2]) > 100


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_restatement_is_the_oracles_adapter_chain(O, case):
    want = O.UniformSourceIterator(case.oracle(O), case.to_ch, case.to_rate).collect()
    s = case.src()
    got = R.converted(s, case.to_ch, case.to_rate).reshape(-1)  # (not the mixer's 0 + v: a -0.0 of the chain stays -0.0)
    assert got.size == want.size, (got.size, want.size)
    assert same(got, want)
    if case.fade and case.take_ns < R.NS_PER_MS and want.size:
        assert np.isnan(want).any()


FORMATS = sorted({(c.to_ch, c.to_rate) for c in CASES})


@pytest.mark.parametrize("to_ch,to_rate", FORMATS)
def test_clips_and_plain_sources_in_one_oracle_mixer(O, to_ch, to_rate):
    rng = np.random.default_rng(to_ch + to_rate)
    mx, srcs = O.Mixer(to_ch, to_rate), []
    for k, c in enumerate(c for c in CASES if (c.to_ch, c.to_rate) == (to_ch, to_rate)):
        mx.add(c.oracle(O))
        srcs.append(c.src())
        if k % 2 == 0:  # a one-shot behind every other clip
            n, ch, rate = 300 + 4000 * k, (2, 1)[k % 4 // 2], (44100, 48000)[k % 3 == 0]
            y = rng.uniform(-1, 1, n * ch).astype(np.float32)
            mx.add(O.TestSource(y, ch, rate).amplify(0.9))
            srcs.append(R.Src(y, ch, rate, R.span_out(n, *R.reduced(rate, to_rate)), gain=0.9, last=n - 1))
    want = mx.collect()
    M = max(s.frames for s in srcs)
    assert want.size == M * to_ch
    assert same(R.clip_mix(to_ch, to_rate, M, srcs), want)


@pytest.mark.parametrize("case", [c for c in CASES if c.n >= 40000 or c.Z > 30000][::2], ids=lambda c: c.name)
def test_unequal_blocks_with_the_cursor_are_the_one_pass(case):
    s = case.src()
    whole = R.clip_mix(case.to_ch, case.to_rate, s.frames, [s])
    rng = np.random.default_rng(s.frames)
    M = int(R.span_out(R.CHAIN_SAMPLES // case.ch, *R.reduced(case.rate, case.to_rate)))
    cuts = sorted({int(v) for v in rng.integers(0, s.frames + 1, 3)} | {v for v in (M - 1, M, M + 1) if v <= s.frames})
    w, parts = s.words, []
    for m0, m1 in zip([0] + cuts, cuts + [s.frames]):
        assert w[5] == m0
        parts.append(R.clip_mix(case.to_ch, case.to_rate, m1 - m0, [R.Src(case.x, case.ch, case.rate, m1 - m0, gain=case.gain, words=w)]))
        w = R.clip_advance(w, case.ch, case.rate, case.to_rate, m1 - m0)
    assert w[5] == w[6] == s.frames and R.clip_advance(w, case.ch, case.rate, case.to_rate, 5)[5] == s.frames
    assert same(np.concatenate(parts), whole)


# ---- the windowed form: only the chains (rule G) or frames (rule C) a block touches ------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_windowed_form_is_the_whole_stream_one(case):
    """clip_window() never builds the delay's zeros and walks no chain in front of the block.  The whole clip, and blocks at random cursors
    -- one frame, one chain's end, anything --, against the form that was held against the oracle above."""
    s = case.src()
    whole = R.clip_whole(s, case.to_rate)
    assert whole.shape[0] == s.frames == R.clip_out_frames_wide(s.words, case.ch, case.rate, case.to_rate)
    if s.frames == 0:
        return
    assert same(R.clip_window(s, case.to_rate), whole)
    assert same(R.clip_mix_window(case.to_ch, case.to_rate, s.frames + 3, [s]), R.clip_mix(case.to_ch, case.to_rate, s.frames + 3, [s]))
    rng = np.random.default_rng(case.n + case.Z)
    M = int(R.span_out(R.CHAIN_SAMPLES // case.ch, *R.reduced(case.rate, case.to_rate)))
    cuts = [(int(d), int(n)) for d, n in zip(rng.integers(0, s.frames, 12), rng.integers(1, 700, 12))] + [(M - 1, 1), (M, 1), (M - 3, 7), (s.frames - 1, 1), (0, 1)]
    for done, n in cuts:
        if done < 0 or done >= s.frames:
            continue
        part = case.src(min(n, s.frames - done), done)
        assert same(R.clip_window(part, case.to_rate), whole[done:done + part.frames]), (done, n)
    # ... and the pure-int tap of single frames is the frame the stream form reads
    S = R.stream(s.x, s.gain, s.words, case.ch, case.rate).reshape(-1, case.ch)
    F, T = R.reduced(case.rate, case.to_rate)
    for x in {0, s.frames - 1, s.frames // 2, min(M, s.frames - 1), min(M - 1, s.frames - 1)}:
        ia, two, num = R.tap_of(s.words, case.ch, case.rate, case.to_rate, x)
        with np.errstate(all="ignore"):
            v = S[ia] + (S[ia + 1] - S[ia]) * np.float32(num) / np.float32(T) if two else S[ia]
        assert same(v, whole[x]), x


def test_the_windowed_form_with_the_rule_c_phase_at_a_large_done():
    """Rule C keeps ONE converter: output frame `done + m` lies at (done + m) F of it, whatever done is.  65521 -> 65519 Hz, a delay of
    200 002 samples and cursors up to the end: the phase done F mod T takes values all over [0, T), the whole-stream form still reaches."""
    pair = WP.BY_ID["65521-65519"]
    c = Case("rule C, a large phase", 60000, 200002, kind="test", rate=pair.from_rate, to_rate=pair.to_rate)
    s = c.src()
    whole = R.clip_whole(s, c.to_rate)
    rng = np.random.default_rng(4)
    phases = []
    for done in [int(v) for v in rng.integers(90000, s.frames - 400, 10)] + [s.frames - 400, 99990]:
        part = c.src(400, done)
        assert same(R.clip_window(part, c.to_rate), whole[done:done + 400]), done
        phases.append(done * pair.F % pair.T)
        for m in (0, 399):
            ia, two, num = R.tap_of(s.words, 2, c.rate, c.to_rate, done + m)
            assert (ia, num) == ((done + m) * pair.F // pair.T, (done + m) * pair.F % pair.T)
    assert max(phases) > pair.T * 3 // 4 and min(phases) < pair.T // 4


# (n, ch, rate, span_len, Z, take, fade) the plan refuses
REFUSED = [
    (40000, 2, 44100, 1152, 0, None, False, R.UNSUPPORTED),     # decoder packets
    (40000, 2, 44100, 39999, 0, None, False, R.UNSUPPORTED),
    (4001, 2, 44100, 4001, 100, None, False, R.UNSUPPORTED),    # Ls odd
    (6000, 2, 44100, 6000, 1000, 3001, True, R.UNSUPPORTED),    # the take expires inside a frame
    (6000, 2, 44100, 0, 1001, None, False, R.UNSUPPORTED),      # rule C, Ls odd
    (60000, 6, 44100, 60000, 0, None, False, R.UNSUPPORTED),    # Ls > 32768 with 6 channels
    (30000, 3, 44100, 30000, 3000, 30000, False, R.UNSUPPORTED),
    (30000, 5, 44100, 0, 5000, 30000, False, R.UNSUPPORTED),
    (28000, 7, 44100, 28000, 7000, None, False, R.UNSUPPORTED),
    (4000, 2, 44100, 0, 0, None, True, R.INVALID),              # the fade-out without a take
]


@pytest.mark.parametrize("n,ch,rate,span_len,Z,take,fade,want", REFUSED)
def test_what_the_plan_refuses(n, ch, rate, span_len, Z, take, fade, want):
    take_ns = None if take is None else take_for(take, ch, rate)
    assert R.clip_plan(n, ch, rate, span_len, ns_for(Z, ch, rate), take_ns, fade) == want
    flags = (1 if take is not None else 0) | (2 if fade else 0)
    st, _ = ask(plan_exe(), "plan", n, ch, rate, span_len, ns_for(Z, ch, rate), take_ns or 0, flags)
    assert STATUS[st] == want


# ---- the plan header ------------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "tests", "cpp", "clip_mix_plan_test")
SRC = EXE + ".cpp"
HEADER = os.path.join(ROOT, "rodio_amd", "csrc", "rh_clip_mix_plan.h")
STATUS = {0: R.OK, 1: R.INVALID, 3: R.UNSUPPORTED}


def plan_exe():
    spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "clip_mix_plan_test" in b.DRIVERS and os.path.exists(HEADER)
    b.build_driver("clip_mix_plan_test", False, lambda cmd: subprocess.check_call(cmd))  # (build() makes it; stale or missing: here)
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


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_the_headers_plan_and_cursor_are_the_restatements(case):
    flags = (1 if case.take_ns is not None else 0) | (2 if case.fade else 0)
    st, w = ask(plan_exe(), "plan", case.x.size, case.ch, case.rate, case.span_len, case.delay_ns, case.take_ns or 0, flags)
    assert st == 0 and w == case.words()
    rng = np.random.default_rng(case.n)
    for n in [0] + [int(v) for v in rng.integers(0, 40000, 4)] + [10**6]:
        want = R.clip_advance(w, case.ch, case.rate, case.to_rate, n)
        st, got = ask(plan_exe(), "advance", *w, case.ch, case.rate, case.to_rate, n)
        assert st == 0 and got == want, (w, n)
        w = want
    assert w[5] == w[6]


def test_positions_fade_steps_refusals_and_bounds():
    n = run(plan_exe())
    assert n["failures"] == 0
    # the run was not vacuous
    assert n["divs"] > 100000 and n["clips"] >= 300 and n["blocks"] >= 900 and n["taps"] > 200000 and n["faded"] > 20000 and n["delay_taps"] > 1000
    assert n["refusals"] >= 25 and n["bounds"] >= 16 and n["fade64"] >= 1
    assert run(plan_exe(), 2, 100)["failures"] == 0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Host code with a main of its own: built with the sanitizers and run as it is."""
    exe = str(tmp_path / "clip_mix_plan_test_san")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rodio_amd", "csrc"), SRC, "-o", exe])
    n = run(exe, 4, 100)
    assert n["failures"] == 0 and n["refusals"] >= 25 and n["bounds"] >= 8 and n["taps"] > 50000
