"""tests/queue_mix_ref.py -- the numpy restatement the GPU tests of rh_queue_mix_block compare with -- held against the oracle, no GPU: the bits
of `Mixer(ch, to_rate)` fed `SeqSource(parts)`, the oracle's model of a queue of sounds of formats of their own (each part behind its own
Amplify), with plain `SamplesBuffer`s mixed in between for order; a keep-alive tail is written for the oracle as one-frame parts of zeros in
the exhausted sound's format.  Then the cursor: a stream cut into three unequal blocks at every position near a seam or a chain's end equals
the one pass, and the cursor stays small however long the queue plays.  Then the entry's host decisions (rodio_amd/csrc/rh_queue_mix_plan.h):
tests/cpp/queue_mix_plan_test, as built by build() and once more under -fsanitize=address,undefined, and its tables against what the
restatement walks."""
import importlib.util
import itertools
import os
import shutil
import subprocess

import numpy as np
import pytest

import queue_mix_ref as R
import wide_positions as WP

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIXES = [(2, 48000), (1, 44100), (6, 48000)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sound(rng, n, ch, rate, gain=1.0):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if n > 8:  # zeros of both signs among the samples
        z = rng.integers(0, n, 4)
        x[z[:2]], x[z[2:]] = 0.0, -0.0
    return R.Sound(x, ch, rate, gain)


def abc(rng):
    """A = 32776 samples stereo at 44.1 kHz, B = 6 mono at 8 kHz, C = 10 stereo at 22.05 kHz: chain 1 is samples 0 .. 32768 of A, chain 2 the
    next 24 samples of the stream -- 8 of A, all of B, all of C -- as 12 stereo frames at 44.1 kHz."""
    return [sound(rng, 32776, 2, 44100, 0.8), sound(rng, 6, 1, 8000, -1.25), sound(rng, 10, 2, 22050, 0.5)]


def small3(rng):
    return [sound(rng, 8, 1, 48000, 0.7), sound(rng, 12, 2, 44100, -1.1), sound(rng, 5, 1, 44100, 1.9)]


QUEUES = {
    "abc": abc,
    "small3": small3,
    "one": lambda rng: [sound(rng, 14, 2, 44100, 0.9)],
    "same_rate": lambda rng: [sound(rng, 10, 2, 48000, 0.6), sound(rng, 6, 1, 48000, 1.0)],       # F == T into 48 kHz
    "down": lambda rng: [sound(rng, 20, 2, 96000, 0.6), sound(rng, 18, 1, 88200, -0.4)],            # a downsampling pair
    "empty_between": lambda rng: [sound(rng, 6, 2, 44100), sound(rng, 0, 1, 8000), sound(rng, 4, 2, 22050, 2.0)],
}


def oracle_queue(O, sounds, tail_frames=0):
    """The queue as the oracle's SeqSource: every sound behind its Amplify, then tail_frames one-frame parts of zeros in the last sound's format."""
    with np.errstate(all="ignore"):
        parts = [((s.x * s.gain).astype(np.float32), s.ch, s.rate) for s in sounds if s.samples]
    last = [s for s in sounds if s.samples][-1]
    parts += [(np.zeros(last.ch, np.float32), last.ch, last.rate)] * tail_frames
    return O.SeqSource(parts)


def one_shot(rng, n, ch, rate, to_rate, gain):
    """A plain SamplesBuffer of n frames (<= 32768 samples: one chain) as (oracle source factory, restatement source)."""
    y = rng.uniform(-1, 1, n * ch).astype(np.float32)
    F, T = R.reduced(rate, to_rate)
    return y, R.Src(R.span_out(n, F, T), x=y, ch=ch, from_rate=rate, gain=gain, last=n - 1)


@pytest.mark.parametrize("to_ch,to_rate", MIXES)
@pytest.mark.parametrize("name", sorted(QUEUES))
def test_the_restatement_is_the_oracles_mixer(O, name, to_ch, to_rate):
    """A one-shot, the queue (no keep_alive: it ends with its sounds), another one-shot: the whole mix."""
    rng = np.random.default_rng(len(name) + to_ch)
    sounds = QUEUES[name](rng)
    M = R.stream_frames(sounds, False, to_rate)
    mx, srcs = O.Mixer(to_ch, to_rate), []
    for k in range(3):
        if k == 1:
            mx.add(oracle_queue(O, sounds))
            srcs.append(R.Src(M + 3, sounds, [0, 0, R.PLAYING, 0]))  # (it reaches three frames behind its end: nothing is added there)
        else:
            y, s = one_shot(rng, 9 + 30 * k, (2, 1, 1)[k], (22050, 0, 48000)[k], to_rate, 0.5 + k)
            mx.add(O.SamplesBuffer(s.ch, s.from_rate, y).amplify(float(s.gain)))
            srcs.append(s)
    want = mx.collect()
    total = max(M + 3, max(s.frames for s in srcs))
    for s in srcs:
        s.frames = min(s.frames, total)
    got = R.queue_mix(to_ch, to_rate, total, srcs)
    assert want.size == max(M, srcs[0].frames, srcs[2].frames) * to_ch
    got = got[: want.size]
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (int(bad[0]), got[bad[0]], want[bad[0]])
    if name == "abc":  # the crossing chain is where the header says, and it lerps across both seams
        segs = R.walk(sounds, [0, 0, 0, 0], to_rate, M)[0]
        assert [(c.n, c.ch, c.rate, [(k, off, start) for k, off, start, _ in c.runs]) for c, _, _, _ in segs] == [(32768, 2, 44100, [(0, 0, 0)]), (24, 2, 44100, [(0, 32768, 0), (1, 0, 8), (2, 0, 14)])]


@pytest.mark.parametrize("name,extra", [("abc", 0), ("abc", 9), ("small3", 0), ("small3", 4)])
def test_a_keep_alive_tail(O, name, extra):
    """With keep_alive the chain in progress when the sounds run out goes on to its full count through zeros, and behind it the queue adds
    +0.0.  `abc` without C: the second chain starts inside A, so it takes 32768 samples -- 8 of A, 6 of B and 32754 of silence; small sounds
    end their chains with themselves, so `small3` lacks nothing.  extra: one-frame zero parts behind what the chain swallows."""
    rng = np.random.default_rng(7 + extra)
    to_ch, to_rate = 2, 48000
    sounds = QUEUES[name](rng)[:2]
    segs, end, dropped = R.walk(sounds, [0, 0, 0, 1], to_rate, 10 ** 6)
    lacking = sum(cnt for k, _, _, cnt in segs[-1][0].runs if k is None)
    assert lacking == (32754 if name == "abc" else 0) and end == [0, 0, R.SILENT, 1] and dropped == 2
    M = segs[-1][1] + segs[-1][2]
    last = sounds[-1]
    assert lacking % last.ch == 0
    mx = O.Mixer(to_ch, to_rate)
    mx.add(oracle_queue(O, sounds, lacking // last.ch + extra))
    want = mx.collect()
    assert want.size == (M + extra) * to_ch  # every one-frame chain behind the swallowed ones emits one frame
    got = R.queue_mix(to_ch, to_rate, M + extra, [R.Src(M + extra, sounds, [0, 0, 0, 1])])
    assert np.array_equal(bits(got), bits(want))
    assert not bits(got[M * to_ch:]).any()


def interesting(sounds, keep, to_rate):
    """Output frames within +-2 of every chain's end and of every seam inside a chain."""
    total = R.stream_frames(sounds, keep, to_rate)
    out = set()
    for c, m0, cnt, _ in R.walk(sounds, [0, 0, 0, 1 if keep else 0], to_rate, total)[0]:
        F, T, _, _ = c.conv(to_rate)
        marks = [m0, m0 + cnt] + [m0 + ((start // c.ch) * T) // F for _, _, start, _ in c.runs[1:]]
        out.update(m + d for m in marks for d in range(-2, 3))
    return sorted(m for m in out if 0 <= m <= total + 3), total + 3


@pytest.mark.parametrize("keep", [False, True])
@pytest.mark.parametrize("name", sorted(QUEUES))
def test_three_unequal_blocks_are_the_one_pass(name, keep):
    rng = np.random.default_rng(3)
    to_ch, to_rate = 2, 48000
    sounds = QUEUES[name](rng)
    marks, total = interesting(sounds, keep, to_rate)
    fresh = [0, 0, 0, 1 if keep else 0]
    whole = R.queue_mix(to_ch, to_rate, total, [R.Src(total, sounds, fresh)]).reshape(total, to_ch)
    pairs = list(itertools.combinations(marks, 2))
    if len(pairs) > 150:  # (abc: every mark as a first cut with a second one next to it, and a spread of the rest)
        pairs = [(a, b) for a, b in pairs if b - a <= 1] + pairs[:: len(pairs) // 100]
    assert len(pairs) >= 10
    for c1, c2 in pairs:
        words, rest, at = fresh, list(sounds), 0
        for m0, m1 in ((0, c1), (c1, c2), (c2, total)):
            n = m1 - m0
            if rest:  # (a queue whose sounds have all been dropped adds nothing)
                part = R.queue_mix(to_ch, to_rate, n, [R.Src(n, rest, words)]).reshape(n, to_ch)
            else:
                part = np.zeros((n, to_ch), np.float32)
            assert np.array_equal(bits(part), bits(whole[m0:m1])), (c1, c2, m0)
            words, dropped = R.queue_advance(words, rest, to_rate, n)
            rest, at = rest[dropped:], at + dropped
            assert words[2] == R.PLAYING or not rest
        assert words[2] == (R.SILENT if keep else R.ENDED)


def test_the_cursor_stays_small_however_long_the_queue_plays():
    """10^6 output frames of a playlist of one-second stereo sounds: chain_start stays inside the front sound, chain_out below the output
    count of a whole chain, 17833 at 44.1 -> 48 kHz; nothing in the words grows with the play time."""
    lens = [88200, 44100, 88202, 12000, 66000] * 8
    sounds = [R.Sound(np.zeros(n, np.float32), 2, 44100) for n in lens]
    bound = R.span_out(R.CHAIN_SAMPLES // 2, 147, 160)
    assert bound == 17833 and R.stream_frames(sounds, True, 48000) > 1.2e6
    words, rest, played, rng = [0, 0, 0, 1], list(sounds), 0, np.random.default_rng(0)
    _, one, one_dropped = R.walk(sounds, words, 48000, 10 ** 6)
    while played < 10 ** 6:
        n = min(int(rng.integers(1, 9000)), 10 ** 6 - played)
        words, dropped = R.queue_advance(words, rest, 48000, n)
        rest, played = rest[dropped:], played + n
        assert words[2] == R.PLAYING and words[0] < rest[0].samples and words[1] < bound and max(words) < 88202
    assert words == one and len(sounds) - len(rest) == one_dropped > 25  # ... and any cut of the stream leaves the cursor of the one pass


# ---- the plan header ------------------------------------------------------------------------------------------------------------------------
EXE = os.path.join(ROOT, "tests", "cpp", "queue_mix_plan_test")
SRC = EXE + ".cpp"
HEADER = os.path.join(ROOT, "rodio_amd", "csrc", "rh_queue_mix_plan.h")
STATUS = {0: R.OK, 1: R.INVALID, 3: R.UNSUPPORTED}


def plan_exe():
    spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    assert "queue_mix_plan_test" in b.DRIVERS and os.path.exists(HEADER)
    b.build_driver("queue_mix_plan_test", False, lambda cmd: subprocess.check_call(cmd))  # (build() makes it; stale or missing: here)
    return EXE


def run(exe, *args):
    r = subprocess.run([exe, *map(str, args)], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr + r.stdout
    words = r.stdout.split()
    return {k: int(v) for k, v in zip(words[::2], words[1::2])}


def gain_bits(g):
    return int(np.float32(g).view(np.uint32))


def ask_plan(to_rate, channels, out_frames, srcs):
    """The status and the tables of rh_queue_mix_plan.h for a call, in the form of R.tables()."""
    args = ["plan", to_rate, channels, out_frames, len(srcs)]
    for s in srcs:
        sounds = s.sounds or []
        args += [s.frames, len(sounds), *s.words, s.ch, s.from_rate, s.phase, s.last, gain_bits(s.gain)]
        for q in sounds:
            args += [q.samples, q.ch, q.rate, gain_bits(q.gain)]
    r = subprocess.run([plan_exe(), *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
    lines = [l.split() for l in r.stdout.strip().split("\n")]
    st = STATUS[int(lines[0][0])]
    if st != R.OK:
        return st, None
    out = []
    for l in lines[1:]:
        if l[0] == "src":
            out.append([])
        elif l[0] == "seg":
            m0, cnt, prior, ch, F, T, nl, _, sane = map(int, l[1:])
            assert sane == 1
            out[-1].append((m0, cnt, prior, ch, F, T, nl, []))
        else:
            out[-1][-1][7].append(tuple(map(int, l[1:])))
    return st, out


def want_tables(srcs, to_rate):
    """R.tables() with each piece's gain, as the bits the plan must carry."""
    out = []
    for s, segs in zip(srcs, R.tables(srcs, to_rate)):
        out.append([(m0, cnt, prior, ch, F, T, nl, [(k, off, start, gain_bits(s.gain) if k == -2 else (0 if k == -1 else gain_bits(s.sounds[k].gain))) for k, off, start in pieces])
                    for m0, cnt, prior, ch, F, T, nl, pieces in segs])
    return out


@pytest.mark.parametrize("name", sorted(QUEUES))
def test_the_plans_tables_are_what_the_restatement_walks(name):
    rng = np.random.default_rng(11)
    to_rate = 48000
    sounds = QUEUES[name](rng)
    marks, total = interesting(sounds, True, to_rate)
    for played in [0] + marks[1::3]:
        words, dropped = R.queue_advance([0, 0, 0, 1], sounds, to_rate, played)
        rest = sounds[dropped:]
        st, exe_words = ask_advance(to_rate, played, [0, 0, 0, 1], sounds)
        assert st == R.OK and exe_words == (words, dropped)
        if not rest:
            continue
        M = min(total - played + 2, 40000)
        srcs = [R.Src(min(20, M), x=np.zeros(64, np.float32), ch=2, from_rate=44100, gain=0.5, phase=3, last=17), R.Src(M, rest, words), R.Src(0, rest, words), R.Src(M // 2, sounds, [0, 0, 0, 0])]
        st, got = ask_plan(to_rate, 2, M, srcs)
        assert st == R.OK and got == want_tables(srcs, to_rate), (played, got, want_tables(srcs, to_rate))


def ask_advance(to_rate, out_frames, words, sounds):
    args = ["advance", to_rate, out_frames, *words, len(sounds)]
    for q in sounds:
        args += [q.samples, q.ch, q.rate]
    r = subprocess.run([plan_exe(), *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
    v = [int(t) for t in r.stdout.split()]
    return STATUS[v[0]], (v[1:5], v[5])


def test_chains_that_cut_a_frame_are_refused():
    """A 6-channel sound of 32772 samples (its first chain takes 32768 = 5461 frames and 2 samples), and a stereo sound of more than a chain
    followed by a mono sound of odd length that ends the seam chain: the restatement and the header refuse both as unsupported."""
    z = np.zeros
    for sounds, keep, frames in [([R.Sound(z(32772, np.float32), 6, 48000)], 1, 10), ([R.Sound(z(32776, np.float32), 2, 44100), R.Sound(z(5, np.float32), 1, 44100)], 0, 40000)]:
        s = R.Src(frames, sounds, [0, 0, 0, keep])
        with pytest.raises(R.Refused) as e:
            R.queue_mix(2, 48000, frames, [s])
        assert e.value.status == R.UNSUPPORTED
        assert ask_plan(48000, 2, frames, [s])[0] == R.UNSUPPORTED
        assert ask_advance(48000, frames, [0, 0, 0, keep], sounds)[0] == R.UNSUPPORTED
    # the seam chain is taken where keep_alive fills it up to whole frames, and a block that ends in front of it is taken either way
    s = R.Src(40000, sounds, [0, 0, 0, 1])
    assert ask_plan(48000, 2, 40000, [s]) == (R.OK, want_tables([s], 48000))
    s = R.Src(17833, sounds, [0, 0, 0, 0])
    assert ask_plan(48000, 2, 40000, [s]) == (R.OK, want_tables([s], 48000))


def edge_cases():
    """(from_rate, to_rate, frames of a mono sound, status): per rate pair of tests/wide_positions.py the longest chain that passes and the
    shortest that does not, and the bound M F <= 2^32 - 1 to the frame: from 1 Hz a sound of n frames emits M = (n - 1) T + 1."""
    out = [(1, 2147483647, 3, R.OK), (1, 2147483648, 3, R.UNSUPPORTED), (1, 4294967294, 2, R.OK), (1, 4294967295, 2, R.UNSUPPORTED)]
    sizes = (1, 2, 3, 64, 255, 256, 257, 1000, 16384, 32768)
    for p in WP.BANK:
        fits = [n for n in sizes if R.span_out(n, p.F, p.T) * p.F <= 0xFFFFFFFF]
        over = [n for n in sizes if R.span_out(n, p.F, p.T) * p.F > 0xFFFFFFFF]
        out += [(p.from_rate, p.to_rate, fits[-1], R.OK)] + [(p.from_rate, p.to_rate, n, R.UNSUPPORTED) for n in over[:1]]
    return out


@pytest.mark.parametrize("from_rate,to_rate,n,want", edge_cases())
def test_the_32_bit_bound_at_its_edge(from_rate, to_rate, n, want):
    """A chain's positions j F stay inside 32 bits exactly where M F <= 2^32 - 1 (M: the chain's output frames).  A chain that passes is
    planned at its last 50 output frames, where j F is largest."""
    F, T = R.reduced(from_rate, to_rate)
    sounds = [R.Sound(np.zeros(n, np.float32), 1, from_rate)]
    M = R.span_out(n, F, T)
    assert (M * F <= 0xFFFFFFFF) == (want == R.OK)
    s = R.Src(min(M, 50), sounds, [0, max(0, M - 50) if want == R.OK else 0, 0, 1])
    st, got = ask_plan(to_rate, 1, 50, [s])
    assert st == want, (n, M, F, T)
    if want == R.OK:
        assert got == want_tables([s], to_rate)
    else:
        with pytest.raises(R.Refused):
            R.walk(sounds, [0, 0, 0, 1], to_rate, 50)


def test_chains_cursor_tables_refusals_and_bounds_against_the_sample_by_sample_model():
    n = run(plan_exe())
    assert n["failures"] == 0
    # the run was not vacuous
    assert n["located"] > 100000 and n["cuts"] > 3000 and n["refusals"] > 100 and n["bounds"] == 8 and n["chains"] > 400 and n["seams"] > 50 and n["tails"] > 20
    assert run(plan_exe(), 300, 150)["failures"] == 0


def test_the_same_program_under_address_and_undefined_behaviour_sanitizers(tmp_path):
    """Host code with a main of its own: built with the sanitizers and run as it is."""
    exe = str(tmp_path / "queue_mix_plan_test_san")
    subprocess.check_call([shutil.which("g++") or "g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=undefined", "-Wall", "-Wextra",
                           "-I", os.path.join(ROOT, "rodio_amd", "csrc"), SRC, "-o", exe])
    n = run(exe, 150, 100)
    assert n["failures"] == 0 and n["bounds"] == 8 and n["located"] > 100000 and n["seams"] > 20
