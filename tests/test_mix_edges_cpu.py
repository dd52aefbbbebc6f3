"""The premises of tests/test_gpu_mix_edges.py, no GPU: every case of tests/mix_edges.py is where it claims to be.  Part A: the blocks
take more than two and less than three sweeps and are no multiple of 256 samples, and a chain end, a seam and a source end lie behind the
first sweep.  Part B: the positions are in the upper half of 32 bits -- M F within 1443 of the bound, its neighbour refused, P >= 2^31 --
and locate() of the plan headers, run through tests/cpp/loop_mix_plan_test and clip_mix_plan_test, names the taps Python ints name there.
Part C: describe() chooses the 32-bit fade for eleven chains and the 64-bit one for a frame more, and fade_ms() is the millisecond Python
ints give.  Part D: the far cursors are as far as they say, and clip_window() agrees with single taps worked out in Python ints."""
import importlib.util
import os
import subprocess
from math import gcd

import numpy as np
import pytest

import clip_mix_ref as CR
import loop_mix_ref as LR
import mix_edges as E
import player_mix_ref as PR
import queue_mix_ref as QR
import wide_positions as W
from test_clip_mix_cpu import same

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
RATES = pytest.mark.parametrize("rate,to_rate", E.RATES_A)


def exe(name):
    spec = importlib.util.spec_from_file_location("_rh_build", os.path.join(ROOT, "rodio_amd", "build.py"))
    b = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(b)
    b.build_driver(name, False, lambda cmd: subprocess.check_call(cmd))  # (build() makes it; stale or missing: here)
    return os.path.join(ROOT, "tests", "cpp", name)


def ask(name, *args):
    r = subprocess.run([exe(name), *map(str, args)], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr + r.stdout
    return [[int(t) for t in line.split()] for line in r.stdout.splitlines()]


def loop_locate(s, to_ch, to_rate, M, ms):
    out = ask("loop_mix_plan_test", "locate", *s.words, s.ch, s.from_rate, to_ch, to_rate, s.frames, M, *ms)
    return out[0][0], out[1:]


def clip_locate(s, to_ch, to_rate, M, ms):
    out = ask("clip_mix_plan_test", "locate", *s.words, s.ch, s.from_rate, to_ch, to_rate, s.frames, M, *ms)
    return out[0][0], out[1:]


def in_two_to_three_sweeps(frames, ch):
    sweeps, rest = E.sweeps_of(frames, ch)
    assert 2 < sweeps < 3 and rest != 0


# ---- A ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_sweep_sizes_are_the_launch_lines():
    """The constants restate `grid_for(.., 256u * 16u)` of the kernels' launch lines: 4096 workgroups of 256 samples or 64 frames."""
    assert E.SWEEP_SAMPLES == 1 << 20 and E.SWEEP_FAST_FRAMES == 262144
    csrc = os.path.join(ROOT, "rodio_amd", "csrc")
    for name, n in (("rh_widemix.hip", 3), ("rh_playermix.hip", 2), ("rh_spatialmix.hip", 2), ("rh_loopmix.hip", 1), ("rh_queuemix.hip", 1), ("rh_clipmix.hip", 1)):
        text = open(os.path.join(csrc, name)).read()
        assert text.count("256u * 16u") == n, name
    assert "constexpr uint32_t kFastFrames = 64;" in open(os.path.join(csrc, "rh_playermix.hip")).read()
    assert "constexpr uint32_t kSpFastFrames = 64;" in open(os.path.join(csrc, "rh_spatialmix.hip")).read()
    for ch in (1, 2, 5):  # (the layouts the cases use)
        in_two_to_three_sweeps(E.long_frames(ch), ch)
    assert 2 < E.LONG_FAST_FRAMES / E.SWEEP_FAST_FRAMES < 3 and E.LONG_FAST_FRAMES * 2 % 256


@RATES
def test_the_long_loop_case(rate, to_rate):
    for many in (False, True):
        c = E.loop_long(rate, to_rate, many)
        M, F, T = c["M"], *W.reduced(rate, to_rate)
        in_two_to_three_sweeps(M, 2)
        assert len(c["srcs"]) == (33 if many else 3) and c["srcs"][-1] is c["small"] and c["small"].frames == c["big"].frames == M
        assert c["big"].words[:3] == [20000, 16384, 1] and c["small"].words[:3] == [9, 4, 0]
        Mc = PR.stream_out_frames(16384, F, T)
        out = c["big"].words[4]
        assert (out + M - 1) // Mc > (out + E.SWEEP_SAMPLES // 2) // Mc >= 1, "a chain end behind the first sweep"
        assert E.behind_first_sweep(c["plain"].frames, 2) and 2 * E.SWEEP_SAMPLES < c["plain"].frames * 2 < M * 2, "a source end in the third sweep"
        if many:
            assert sum(1 for s in c["srcs"][:32] if s.frames == M) == 1 and all(s.frames == 300 for s in c["srcs"][2:32])


@pytest.mark.parametrize("to_rate", [48000, 44100])
def test_the_long_queue_case(to_rate):
    c = E.queue_long(to_rate)
    M = c["M"]
    in_two_to_three_sweeps(M, 2)
    q, plain, short = c["srcs"]
    assert len(q.sounds) >= 40 and {(s.ch, s.rate) for s in q.sounds} == set(E.QUEUE_FORMATS)
    sizes = [s.samples for s in q.sounds]
    assert min(sizes) == 3 and max(sizes) == 50000
    segs, end, _ = QR.walk(q.sounds, q.words, to_rate, M)
    assert sum(cnt for _, _, cnt, _ in segs) == M and end[2] == QR.PLAYING, "the queue outlasts the block"
    starts, seams = E.queue_seams(q, to_rate)
    for lo in (0, 1, 2):  # a chain start in every sweep, and a seam between two sounds inside a chain in the two whole ones
        assert any(lo * E.SWEEP_SAMPLES <= 2 * m < (lo + 1) * E.SWEEP_SAMPLES for m in starts[1:]), lo
        assert lo == 2 or any(lo * E.SWEEP_SAMPLES <= 2 * m < (lo + 1) * E.SWEEP_SAMPLES for m in seams), lo
    assert E.SWEEP_SAMPLES + 1000 in starts
    assert any(len(ch.runs) >= 3 for ch, _, _, _ in segs), "a chain over three sounds"
    assert E.SWEEP_SAMPLES < 2 * c["silent_from"] < 2 * E.SWEEP_SAMPLES and QR.walk(short.sounds, short.words, to_rate, M)[1][2] == QR.SILENT
    assert 2 * E.SWEEP_SAMPLES < plain.frames * 2 < M * 2


@RATES
def test_the_long_clip_case(rate, to_rate):
    for many in (False, True) if rate != to_rate else (False,):
        c = E.clip_long(rate, to_rate, many)
        M, F, T = c["M"], *W.reduced(rate, to_rate)
        in_two_to_three_sweeps(M, 2)
        f, whole, waiting = c["fading"], c["whole"], c["waiting"]
        assert len(c["srcs"]) == (33 if many else 4) and c["srcs"][-1] is whole
        assert f.words[0] == CR.RULE_G and f.words[1] % 2 == 1 and f.words[4] == CR.TAKE | CR.FADE
        assert E.SWEEP_SAMPLES < f.frames * 2 < 2 * E.SWEEP_SAMPLES and f.frames == f.words[6], "it ends inside the second sweep"
        Mc = PR.stream_out_frames(16384, F, T)
        assert f.frames > Mc * 30, "chain ends behind the first sweep"
        assert whole.words[0] == CR.RULE_C and whole.frames == M <= whole.words[6]
        assert waiting.frames == M and (M - 1) * F // T + 2 <= waiting.words[1] // 2, "still in its delay at the block's last tap"
        assert E.fade_mode(f, to_rate) == E.FADE64
        plain = c["srcs"][1]
        assert plain.words is None and 2 * E.SWEEP_SAMPLES < plain.frames * 2 < M * 2
    # the windowed form at this size: the bits of the whole-stream one
    srcs = E.clip_long(rate, to_rate)["srcs"]
    assert same(CR.clip_mix_window(2, to_rate, M, srcs), CR.clip_mix(2, to_rate, M, srcs))


@RATES
def test_the_long_wide_cases(rate, to_rate):
    for to_ch, alike in ((2, False), (5, False), (2, True)):
        c = E.wide_long(rate, to_rate, to_ch, alike)
        in_two_to_three_sweeps(c["M"], to_ch)
        assert len(c["srcs"]) == 5 and 2 * E.SWEEP_SAMPLES < c["end"] * to_ch < c["M"] * to_ch
        assert not alike or {(ch, r) for _, ch, r, _ in c["srcs"]} == {(to_ch, rate)}
    small, big = E.batch_long(rate, to_rate)
    assert small["M"] * small["ch"] < E.SWEEP_SAMPLES and big["M"] * big["ch"] > 2 * E.SWEEP_SAMPLES


@RATES
def test_the_long_player_and_spatial_cases(rate, to_rate):
    F, T = W.reduced(rate, to_rate)
    for fast in (True, False):
        c = E.player_long(rate, to_rate, fast)
        sweep = E.SWEEP_FAST_FRAMES if fast else E.SWEEP_SAMPLES // 2
        assert 2 < c["M"] / sweep < 3 and c["M"] * 2 % 256 and all(s.frames == c["M"] and s.last == PR.LIVE and s.ch == 2 for s in c["srcs"])
        assert sweep < c["ramp_end"] < c["M"], "the ramp ends behind the first sweep"
        f = PR.ramp_factors(PR.RAMP, c["srcs"][1].ramp_ns, 0.1, 1.3, rate, np.array([sweep * F // T, c["ramp_end"] * F // T - 5, c["M"] * F // T - 5]))
        assert f[0] < f[1] < 1.3 and f[2] == 1.0
        c = E.spatial_long(rate, to_rate, fast)
        sweep = E.SWEEP_FAST_FRAMES if fast else E.SWEEP_SAMPLES // 5
        assert 2 < c["M"] / sweep < 3 and c["M"] * c["ch"] % 256 and all(s.frames == c["M"] for s in c["srcs"])
        assert {s.in_ch for s in c["srcs"]} == ({1} if fast else {1, 6}) and c["ch"] == (2 if fast else 5)
        s = c["srcs"][0]
        k = sweep * F // T * c["ch"]  # the emitter's output sample under the first frame behind the first sweep
        entry = lambda i: (s.gain_first + i) // s.gain_period - s.gain_first // s.gain_period  # noqa: E731
        assert entry(c["M"] * F // T * c["ch"] - 1) > entry(k) + 3 > 3, "gain steps behind the first sweep"


# ---- B ------------------------------------------------------------------------------------------------------------------------------------------
def test_the_numbers_of_the_rate_pairs():
    F, T, M, MF = E.chain_numbers(E.T24.from_rate, E.T24.to_rate, 255)
    assert (F, T, M, MF) == (100, 16777259, 42614239, 4261423900) and E.HALF <= MF <= E.U32 - 1
    assert E.chain_numbers(E.T24.from_rate, E.T24.to_rate, 256)[3] <= E.U32 - 1 < E.chain_numbers(E.T24.from_rate, E.T24.to_rate, 257)[3]
    n = E.big_loop_numbers()
    assert n["P"] == 2344789782 and E.HALF <= n["P"] <= E.U32 - 1 and n["chains"] == 55
    assert LR.loop_plan(E.BIG_LOOP["L"], 1, 255) == [14032, 255, 0, 0, 0]
    assert gcd(*E.EDGE) == 1 and gcd(*E.OVER) == 1
    F, T, M, MF = E.chain_numbers(*E.EDGE, 32768)
    assert M == 131148 and E.U32 - 1 - MF == 1443
    assert E.chain_numbers(*E.OVER, 32768)[3] > E.U32 - 1
    assert (M - 1) * F > E.U32 - (1 << 16), "j F of the chain's last frame"


@pytest.mark.parametrize("which", ["chain", "pass"])
def test_the_big_loop_is_above_2_31_and_locate_names_the_ints_taps(which):
    c = E.big_loop_case(which)
    s, n = c["srcs"][0], E.big_loop_numbers()
    assert c["x0"] >= E.HALF and s.words[3] // 255 >= 51 and c["x0"] + c["M"] - 1 <= E.U32 - 1
    if which == "pass":
        assert c["x0"] < n["P"] <= c["x0"] + c["M"] - 1, "x passes P inside the block"
    else:
        assert s.words[4] < n["M"] <= s.words[4] + c["M"] - 1, "the block crosses a chain end"
    ms = list(range(0, c["M"], 7)) + [148, 149, 150, 151, c["M"] - 1]
    st, got = loop_locate(s, 2, c["to_rate"], c["M"], ms)
    assert st == 0 and got[0] == [c["x0"], n["P"], n["M"]]
    ia, ib, two, num, T = LR.loop_taps(s, c["to_rate"])
    for m, (a, b, lerp, nm) in zip(ms, got[1:]):
        p = (c["x0"] + m) % n["P"]  # Python ints all the way
        k, j = p // n["M"], p % n["M"]
        i = j * n["F"] // n["T"]
        assert (a, nm) == (k * 255 + i, j * n["F"] % n["T"]) == (int(ia[m]), int(num[m])) and bool(lerp) == bool(two[m]) and (not lerp or b == int(ib[m])), m
    assert np.isfinite(LR.loop_mix(2, c["to_rate"], c["M"], c["srcs"])).all()


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("c_frames", [255, 256])
def test_the_edge_loops_lie_above_2_31(c_frames, rule):
    c = E.edge_loops(c_frames, rule)
    assert c["j"] * c["F"] > E.HALF and c["Mc"] * c["F"] <= E.U32 - 1
    for s in c["srcs"][:2]:
        st, got = loop_locate(s, 2, c["to_rate"], c["M"], [0, 100, 142, 143, 149, 150, 299])
        assert st == 0
        ia, ib, two, num, _ = LR.loop_taps(s, c["to_rate"])
        for m, (a, b, lerp, nm) in zip([0, 100, 142, 143, 149, 150, 299], got[1:]):
            assert (a, nm, bool(lerp)) == (int(ia[m]), int(num[m]), bool(two[m])), m
    bad = LR.Src(np.zeros(600, np.float32), 2, E.T24.from_rate, 300, words=[300, 257, rule, 0, 0])
    assert loop_locate(bad, 2, c["to_rate"], 300, [0])[0] == 3, "c = 257 leaves 32 bits: refused"


@pytest.mark.parametrize("rule", [0, 1])
def test_the_loops_at_a_divisor_just_below_a_power_of_two(rule):
    c = E.below_loops(rule)
    s = c["srcs"][0]
    assert s.words[:3] == [33000, 32768, rule] and c["j"] * c["F"] > E.HALF and c["Mc"] * c["F"] <= E.U32 - 1
    ms = [0, 100, 148, 149, 150, 299]
    st, got = loop_locate(s, 2, c["to_rate"], c["M"], ms)
    assert st == 0
    ia, ib, two, num, _ = LR.loop_taps(s, c["to_rate"])
    for m, (a, b, lerp, nm) in zip(ms, got[1:]):
        assert (a, nm, bool(lerp)) == (int(ia[m]), int(num[m]), bool(two[m])), m


def test_the_reciprocal_is_small_only_just_below_a_power_of_two():
    """Why BELOW is there: with t = mulhi(x, m), x - t >= 2^31 needs a small m.  At the other pairs' T it is next to 2^32."""
    def m_of(d):
        l = (d - 1).bit_length()
        return (E.U32 * ((1 << l) - d)) // d + 1

    x = E.U32 - 40000
    for T, top in ((E.T24.T, False), (E.EDGE[1], False), (E.BELOW[1], True), (E.FIT_C.T, True), (1_000_000, True)):
        t = x * m_of(T) >> 32
        assert (x - t >= E.HALF) == top, T
    assert E.BELOW[1] == (1 << 17) - 1 and gcd(*E.BELOW) == 1
    F, T, M, MF = E.chain_numbers(*E.BELOW, 32768)
    assert E.HALF < (M - 150) * F and MF <= E.U32 - 1 and (M, E.U32 - 1 - MF) == (131145, 99690)


@pytest.mark.parametrize("pair", E.EDGE_PAIRS, ids=["131074", "131071"])
@pytest.mark.parametrize("which", E.EDGE_BLOCKS)
def test_the_edge_clip_and_queue(which, pair):
    c = E.edge_clip_case(which, pair=pair)
    s = c["srcs"][0]
    F, T, Mc, MF = E.chain_numbers(*pair, 32768)
    assert s.words[0] == CR.RULE_G and s.words[1] + s.words[2] > 32768 and s.ch == 1
    done, M = c["done"], c["M"]
    assert {"ends with the chain's last frame": done + M == Mc, "starts behind it": done == Mc, "straddles it": done < Mc < done + M}[which]
    ms = list(range(0, M, 13)) + [M - 1] + ([Mc - 1 - done] if done < Mc else [])
    st, got = clip_locate(s, 2, c["to_rate"], M, ms)
    assert st == 0
    base = (done // Mc) * 32768
    for m, (ia, lerp, num, _) in zip(ms, got[1:]):
        fr, two, nm = CR.tap_of(s.words, 1, *pair, done + m)
        assert (base + ia, bool(lerp), num) == (fr, two, nm), m
    if done < Mc:
        assert (Mc - 1) * F > E.U32 - (1 << (16 if pair is E.EDGE else 18)) and CR.tap_of(s.words, 1, *pair, Mc - 1) == (32767, False, (Mc - 1) * F % T)
    q = E.edge_queue_case(which, pair=pair)["srcs"][0]
    assert q.words[:2] == ([0, done] if done < Mc else [32768, 0])
    if pair is E.EDGE:  # the neighbour is refused, by the clip's plan and by the queue's
        over = E.edge_clip_case(which, to_rate=E.OVER[1])["srcs"][0]
        assert clip_locate(over, 2, E.OVER[1], M, [0])[0] == 3
        with pytest.raises(QR.Refused):
            QR.walk(E.edge_queue_sounds(), [0, 0, 0, 1], E.OVER[1], 10)


def test_rule_c_at_its_fit():
    done, r0, fit = E.fit_c()
    F, T = E.FIT_C.F, E.FIT_C.T
    assert r0 >= T - T // 100 and r0 + (fit - 1) * F <= E.U32 - 1 < r0 + fit * F and 65000 < fit < 66000
    c = E.fit_c_clip()
    assert c.words()[0] == CR.RULE_C
    for frames, want in ((fit - 1, 0), (fit, 0), (fit + 1, 3)):
        s = c.src(frames, done)
        st, got = clip_locate(s, 2, E.FIT_C.to_rate, frames, [0, frames - 1])
        assert st == want, frames
        if st == 0:
            i0 = done * F // T
            for m, (ia, lerp, num, _) in zip((0, frames - 1), got[1:]):
                fr, two, nm = CR.tap_of(s.words, 2, E.FIT_C.from_rate, E.FIT_C.to_rate, done + m)
                assert (i0 + ia, bool(lerp), num) == (fr, two, nm)
    assert r0 + (fit - 1) * F >= E.HALF


# ---- C ------------------------------------------------------------------------------------------------------------------------------------------
def test_eleven_chains_fade_in_32_bits_and_a_frame_more_in_64():
    c = E.fade_clip()
    w = c.words()
    assert w[0] == CR.RULE_G and w[4] == 3 and -(-(w[1] + w[2]) // 32768) >= 13 and w[1] % 2 == 1
    dps = CR.ns_per_sample(2, 44100)
    for frames, mode, over in zip(E.FADE_BLOCKS, (E.FADE32, E.FADE64, E.FADE64), (False, False, True)):
        s = c.src(frames, 0)
        assert E.fade_mode(s, 48000) == mode and E.fade_overflows(s, 48000) == over
        ms = [0, 60, 17832, 17833, frames // 2, frames - 2, frames - 1]
        st, got = clip_locate(s, 2, 48000, frames, ms)
        assert st == 0 and got[0][0] == mode, "describe()'s own choice"
        for m, (ia, lerp, num, rbits) in zip(ms, got[1:]):
            k = ia * 2 - w[1]  # the sound's sample under channel 0 of the first tap
            want = np.float32((w[3] - k * dps) // CR.NS_PER_MS) if k >= 0 else np.float32(0)
            assert rbits == int(want.view(np.uint32)), m
    assert E.FADE_BLOCKS == [17833 * 11, 17833 * 11 + 1, 17833 * 12] and PR.stream_out_frames(16384, 147, 160) == E.M_CHAIN


def test_a_take_beyond_2_32_ms_and_one_under_a_millisecond():
    c = E.long_take_clip()
    s = c.src()
    assert c.take_ns > 43 * 10**14 and c.take_ns // CR.NS_PER_MS > E.U32 and 300 <= s.words[2] <= 500
    assert E.fade_mode(s, 48000) == E.FADE64 and clip_locate(s, 2, 48000, s.frames, [0])[1][0][0] == E.FADE64
    t = E.short_take_clip()
    assert t.take_ns < CR.NS_PER_MS and np.isnan(CR.clip_mix(2, 48000, t.src().frames, [t.src()])).any()


# ---- D ------------------------------------------------------------------------------------------------------------------------------------------
def int_frame(x, s, to_rate, m):
    """Frame m of the block in the source's layout from tap_of()'s Python ints and single f32 operations."""
    kind, Z, N, take_ns, flags, done = s.words[:6]
    fr, two, num = CR.tap_of(s.words, s.ch, s.from_rate, to_rate, done + m)
    dps = CR.ns_per_sample(s.ch, s.from_rate) if flags & CR.TAKE else 0

    def sample(p):
        k = p - Z
        if k < 0:
            return np.float32(0)
        v = np.float32(x[k]) * s.gain
        if flags & CR.FADE:
            v = np.float32(v * np.float32((take_ns - k * dps) // CR.NS_PER_MS)) / np.float32(take_ns // CR.NS_PER_MS)
        return np.float32(v)

    _, T = CR.reduced(s.from_rate, to_rate)
    out = []
    for c in range(s.ch):
        a = sample(fr * s.ch + c)
        if two:
            b = sample((fr + 1) * s.ch + c)
            a = np.float32(a + np.float32(np.float32(np.float32(b - a) * np.float32(num)) / np.float32(T)))
        out.append(a)
    return np.array(out, np.float32)


def test_the_far_rule_g_clip():
    x, words, dones = E.far_g()
    assert words[1] == (1 << 40) + 1 and words[1] % 2 == 1 and CR.clip_plan(x.size, 2, 44100, 0, -(-words[1] * 10**9 // 88200), words[3], True)[:5] == words[:5]
    q = words[1] // 32768
    assert dones[0] // E.M_CHAIN * 32768 + (1 << 32) < words[1], "zrel saturates: the delay ends more than 2^32 samples behind the chain in progress"
    assert dones[1] < q * E.M_CHAIN < dones[1] + 300 and dones[2] == dones[1] + 300 and dones[2] + 300 < words[6]
    for done in dones:
        s = CR.Src(x, 2, 44100, 300, gain=0.8, words=words[:5] + [done, words[6]])
        got = CR.clip_window(s, 48000)
        for m in (0, 99, 100, 101, 150, 299):
            assert same(got[m], int_frame(x, s, 48000, m)), (done, m)
        assert (np.abs(got).max() > 0) == (done != dones[0])
        st, loc = clip_locate(s, 2, 48000, 300, [0])
        assert st == 0 and (loc[0][5] == E.U32 - 1) == (done == dones[0])
    assert CR.clip_advance_wide(words, 2, 44100, 48000, dones[1])[5] == dones[1]


def test_the_far_rule_c_clips():
    x, words, done = E.far_c()
    assert words[1] > 1 << 45 and words[0] == CR.RULE_C
    x2, words2, done2 = E.far_c_128()
    assert done2 >= 1 << 50 and done2 * E.FIT_C.F >= 1 << 64 and words2[1] + words2[2] < 1 << 62 and words2[6] <= 1 << 63
    for xx, w, d, rate, to_rate in ((x, words, done, 44100, 48000), (x2, words2, done2, E.FIT_C.from_rate, E.FIT_C.to_rate)):
        s = CR.Src(xx, 2, rate, 300, gain=0.8, words=w[:5] + [d, w[6]])
        got = CR.clip_window(s, to_rate)
        assert not got[:40].any() and np.abs(got[150:]).max() > 0, "the sound starts inside the block"
        for m in (0, 40, 100, 101, 150, 299):
            assert same(got[m], int_frame(xx, s, to_rate, m)), m
        assert clip_locate(s, 2, to_rate, 300, [0])[0] == 0


def test_the_far_queue():
    sounds, M1 = E.far_queue()
    s = E.queue_at(10, sounds, True, M1 + 777, 48000)
    assert s.words == [32768, 777, 0, 1] and len(s.sounds) == 4 and sounds[0].samples == 50000
    c = QR.walk(s.sounds, s.words, 48000, 10)[0][0][0]
    assert c.n == 32768 and len(c.runs) >= 3, "the chain reads on into the sounds behind"
