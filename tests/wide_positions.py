"""Tap positions near 32 bits and blocks that are cut (tests/test_wide_positions_cpu.py, tests/test_gpu_wide_positions.py; a plain helper
module like spatial_mix_ref.py: no fixtures, numpy and Python ints only).

The one-launch block mixers form a source's tap position as the u32 `p = r0 + j F` and keep it there with `fit = (2^32 - 1 - T) / F`.  At
audio rates F <= 320 and p never passes 2^28.  BANK holds rate pairs whose F is large enough for a block of a few hundred KiB to cross
`fit` -- every number worked out with Python ints --, `converted` / `mix` restate one converted source and the ordered sum with integer
positions (numpy f32, one rounded operation a line), `uniform_segment` restates rh_uniform_segments with Python-int positions, and
`plan` fills an rh_wide_src for a block that starts at mix frame m0 of a resident stream.

    Amplify::next           amplify.rs:64             sample * factor
    SampleRateConverter     sample_rate.rs:131-201    i = floor(m F / T), num = m F mod T; a + (b - a) * num / T (math.rs:25); the last frame
                                                      verbatim; F == T passes samples through
    ChannelCountConverter   channels.rs:57-85         channel c < from: the input's; channel 1 of a mono source: its only one; otherwise 0.0
    Mixer                   mixer.rs:185-198          ((0 + v_0) + v_1) + ... in insertion order; a source that has ended adds nothing
"""
from math import gcd

import numpy as np

f32 = np.float32
LIVE = 0xFFFFFFFF
U32 = 1 << 32
U64_MAX = (1 << 64) - 1
GAINS = [0.5, -1.5, 0.75, 2.0, -0.25, 1.25]  # (none of them 1: every source has its Amplify)


def reduced(rate, to_rate):
    g = gcd(rate, to_rate)
    return rate // g, to_rate // g


def fit_of(rate, to_rate):
    """Output frames a launch may cover before r0 + j F leaves 32 bits, whatever the phase r0 < T (rh_widemix.hip)."""
    F, T = reduced(rate, to_rate)
    return (U32 - 1 - T) // F


class Pair:
    """One rate pair of the bank.  block: the block length the tests use (a number, or a function of fit); cuts: what the table of the bank
    says -- the block is longer than fit; others: four more rates a mixer at to_rate takes (F T < 2^32) whose own fit lies beyond the
    block, the first of them the second rate of the mixed cases; m0_min / phase_min: where a block may start in the mix."""

    def __init__(self, from_rate, to_rate, block, cuts, others, what, m0_min=1000, phase_min=None):
        self.from_rate, self.to_rate, self.cuts, self.others, self.what, self.m0_min = from_rate, to_rate, cuts, tuple(others), what, m0_min
        self.F, self.T = reduced(from_rate, to_rate)
        self.fit = (U32 - 1 - self.T) // self.F
        self.block = block(self.fit) if callable(block) else block
        self.phase_min = 3 * self.T // 4 if phase_min is None else phase_min

    @property
    def id(self):
        return f"{self.from_rate}-{self.to_rate}"

    @property
    def cut(self):
        """The block frame the second launch starts with; where nothing is cut, a frame 4000 in front of the block's end stands in."""
        return self.fit if self.fit < self.block else self.block - 4000


BANK = [
    Pair(65521, 48000, 70000, True, (44100, 32000, 22050, 8000), "F large, down-conversion; fit = 65550"),
    Pair(65521, 65519, lambda fit: fit + 4000, True, (44100, 48000, 32000, 22050), "F, T both large, ratio next to 1; F T just under 2^32"),
    Pair(48000, 65521, lambda fit: fit + 4000, True, (44100, 32000, 22050, 8000), "up-conversion with large T"),
    # 44 100 into 16 777 259 has F T = 7.4e11: the second rate of this pair is 147, which F T < 2^32 admits (F <= 255)
    Pair(100, 16777259, 300000, False, (147, 200, 250, 255), "T > 2^24: (float)num and (float)T round; no cut", m0_min=200000, phase_min=1),
    Pair(44100, 48000, 70000, False, (32000, 22050, 96000, 8000), "the control: the same tests, no cut"),
    # T > 2 F: the one pair at which (2^32 - 1) / F frames do not fit where (2^32 - 1 - T) / F do -- r0 + j F wraps for a phase above 47 296
    Pair(40000, 100003, lambda fit: fit + 4000, True, (32000, 22050, 11025, 8000), "T > 2 F: a fit without the - T wraps for large phases"),
]
BY_ID = {p.id: p for p in BANK}
CUT_PAIRS = [p for p in BANK if p.cuts]
LARGE_F = [BY_ID["65521-48000"], BY_ID["65521-65519"]]
CONTROL = BY_ID["44100-48000"]


# ---- the planner's arithmetic ---------------------------------------------------------------------------------------------------------------
def lerp_ready(n, F, T):  # #m with floor(m F / T) <= n - 2: both taps of the lerp exist
    return 0 if n == 0 else ((n - 1) * T + F - 1) // F


def out_frames(n, F, T):  # ... plus the verbatim last frame, when an output frame lands on it (sample_rate.rs:193-200)
    if n == 0:
        return 0
    if F == T:
        return n
    c1 = lerp_ready(n, F, T)
    return c1 + (1 if c1 * F < n * T else 0)


def frames_for_total(F, T, target):
    """The shortest stream whose converter emits at least `target` frames."""
    lo, hi = 0, 1
    while out_frames(hi, F, T) < target:
        hi *= 2
    while lo < hi:
        mid = (lo + hi) // 2
        if out_frames(mid, F, T) >= target:
            hi = mid
        else:
            lo = mid + 1
    return lo


def live_frames(F, T, m_end):
    """Frames a stream must have for every mix frame below m_end to find both taps, and three more: the block never sees its end."""
    return (m_end - 1) * F // T + (1 if F == T else 2) + 3


def plan(n, rate, to_rate, m0, M):
    """The rh_wide_src fields of a resident stream of n frames for the block [m0, m0 + M) of a mix at to_rate, and the frames [lo, hi) of
    the stream the header lets the block read: data at frame lo = floor(m0 F / T), phase = m0 F mod T, frames, last."""
    F, T = reduced(rate, to_rate)
    i0, phase = m0 * F // T, m0 * F % T
    frames = max(0, min(out_frames(n, F, T), m0 + M) - m0)
    if frames == 0:
        return dict(i0=i0, phase=phase, frames=0, last=0, lo=0, hi=0)
    i_last = (m0 + frames - 1) * F // T
    if frames == M and i_last + (0 if F == T else 1) <= n - 1:  # both taps of the block's last frame exist: the block does not see the end
        return dict(i0=i0, phase=phase, frames=M, last=LIVE, lo=i0, hi=i_last + (1 if F == T else 2))
    assert i0 <= n - 1
    return dict(i0=i0, phase=phase, frames=frames, last=n - 1 - i0, lo=i0, hi=n)


def fill(e, p, ptr, ch, rate, gain):
    """One rh_wide_src (a ctypes WideSrc) from a plan; ptr: the device address of frame p["lo"] (None where the plan reaches nothing)."""
    e.data, e.channels, e.from_rate, e.phase, e.frames, e.last, e.gain = (ptr if p["frames"] else None), ch, rate, p["phase"], p["frames"], p["last"], gain


# ---- one converted source and the mix, with integer positions ---------------------------------------------------------------------------------
def converted(x, ch, rate, gain, to_ch, to_rate, m0, M):
    """Frames [m0, m0 + M) of ChannelCountConverter(SampleRateConverter(Amplify(x))) for the whole ended stream x: [frames, to_ch] (fewer
    than M frames where the stream ends inside the block)."""
    n = len(x) // ch
    F, T = reduced(rate, to_rate)
    frames = max(0, min(out_frames(n, F, T), m0 + M) - m0)
    if frames == 0:
        return np.zeros((0, to_ch), f32)
    assert (m0 + M) * F < 1 << 62
    m = m0 + np.arange(frames, dtype=np.int64)
    p = m * F
    i = p // T
    num = p - i * T
    two = (i < n - 1) & (F != T)
    with np.errstate(all="ignore"):
        v = np.ascontiguousarray(x, f32).reshape(n, ch) * f32(gain)
        a = v[i]
        b = v[np.where(two, i + 1, i)]
        d = b - a
        e = d * num.astype(f32)[:, None]
        q = e / f32(T)
        lerp = a + q
    r = np.where(two[:, None], lerp, a).astype(f32)
    out = np.zeros((frames, to_ch), f32)
    for c in range(to_ch):
        if c < ch:
            out[:, c] = r[:, c]
        elif c == 1 and ch == 1:
            out[:, c] = r[:, 0]
    return out


def mix(srcs, to_ch, to_rate, m0, M):
    """Frames [m0, m0 + M) of mixer::mixer(to_ch, to_rate) fed `TestSource(x, ch, rate).amplify(gain)` for srcs = [(x, ch, rate, gain)]."""
    out = np.zeros((M, to_ch), f32)
    with np.errstate(all="ignore"):
        for x, ch, rate, gain in srcs:
            v = converted(x, ch, rate, gain, to_ch, to_rate, m0, M)
            out[: len(v)] = out[: len(v)] + v
    return out.reshape(-1)


# ---- rh_uniform_segments with Python-int positions ----------------------------------------------------------------------------------------------
def uniform_segment(x, src_frame0, from_ch, rate, to_ch, to_rate, m0, m1, span_frames, gain=1.0):
    """Output frames [m0, m1) of the span's converter chain (uniform.rs:58-67 behind amplify.rs:64): x holds the span's frames from
    src_frame0 on; span_frames: the span's length, U64_MAX while it is open.  Positions are Python ints: m F may leave 64 bits."""
    F, T = reduced(rate, to_rate)
    v = np.ascontiguousarray(x, f32).reshape(-1, from_ch)
    ms = [m0 + k for k in range(m1 - m0)]
    i = [m if F == T else (m * F) // T for m in ms]
    num = [0 if F == T else m * F - ii * T for m, ii in zip(ms, i)]
    verbatim = np.array([F == T or ii + 1 >= span_frames for ii in i], bool)
    rel = np.array([ii - src_frame0 for ii in i], np.int64)
    assert rel.min() >= 0 and int(rel.max()) + (0 if verbatim[int(rel.argmax())] else 1) < len(v)
    with np.errstate(all="ignore"):
        v = v * f32(gain)
        a = v[rel]
        b = v[np.where(verbatim, rel, rel + 1)]
        d = b - a
        e = d * np.array(num, np.float64).astype(f32)[:, None]  # (num < 2^32: exact in f64, rounded once to f32 as (float)num is)
        q = e / f32(T)
        lerp = a + q
    r = np.where(verbatim[:, None], a, lerp).astype(f32)
    out = np.zeros((m1 - m0, to_ch), f32)
    for c in range(to_ch):
        if c < from_ch:
            out[:, c] = r[:, c]
        elif c == 1 and from_ch == 1:
            out[:, c] = r[:, 0]
    return out.reshape(-1)


# ---- case data ----------------------------------------------------------------------------------------------------------------------------------
def signal(rng, n):
    """n finite samples in [-1, 1) with -0.0, +0.0 and a few exact values among them"""
    x = rng.uniform(-1, 1, n).astype(f32)
    if n:
        k = rng.integers(0, n, max(1, n // 17))
        x[k] = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], f32), k.size)
    return x


def ending_with(F, T, total):
    """The stream at F / T whose converter emits exactly `total` frames, or None (an up-converted stream cannot end on every frame)."""
    n = frames_for_total(F, T, total)
    return n if out_frames(n, F, T) == total else None


def start_for(pair, F, T, cut, also=None, tries=200000):
    """(m0, n): the first frame of a block and the length of a stream at F / T whose LAST output frame is block frame `cut` -- the block
    starts where the pair's own phase is at least phase_min, no earlier than m0_min, and where also[1](m0) holds (also[0]: what names the
    condition, for the table of starts found so far)."""
    key = (pair.id, F, T, cut, also[0] if also else None)
    if key not in _STARTS:
        n = frames_for_total(F, T, pair.m0_min + cut + 1)
        for _ in range(tries):
            m0 = out_frames(n, F, T) - cut - 1
            if m0 >= pair.m0_min and m0 * pair.F % pair.T >= pair.phase_min and (also is None or also[1](m0)):
                break
            n += 1
        else:
            raise AssertionError("no start of the block found")
        _STARTS[key] = (m0, n)
    return _STARTS[key]


_STARTS = {}


def mixed_case(pair, to_ch, n_sources=8, rates=None, M=None, seed=0):
    """Sources of a block of M frames (the pair's block) of a mixer (to_ch, pair.to_rate): layouts 1, 2, 6 and the mixer's own in turn, rates
    in turn from `rates` (the pair's rate and its second one), gains other than 1.  With c = the frame the second launch starts with:
    source 0 ends ON frame c (the block reaches c + 1 frames of it), source 1 ends with frame c - 1 (the block starts where its rate has a
    stream that does; at T > 2^24, where a source frame is 10^5 mix frames, it ends with the nearest frame in front), source 2 ends 777
    frames in front of c or earlier, source 3 1500 behind it or later; the others are live.
    -> dict(m0, M, cut, srcs=[(x, ch, rate, gain)], frames=[what the block reaches of each])."""
    rng = np.random.default_rng(seed)
    rates = rates or (pair.from_rate, pair.others[0])
    M = M or pair.block
    cut = pair.fit if pair.fit < M else M - 4000
    to_rate = pair.to_rate
    F0, T0 = reduced(rates[0], to_rate)
    F1, T1 = reduced(rates[1 % len(rates)], to_rate)
    m0, n0 = start_for(pair, F0, T0, cut, None if pair.T > 1 << 24 else ((F1, T1), lambda m: ending_with(F1, T1, m + cut) is not None))
    srcs, frames = [], []
    for k in range(n_sources):
        ch, rate = (1, 2, 6, to_ch)[k % 4], rates[k % len(rates)]
        F, T = reduced(rate, to_rate)
        if k == 0:
            n = n0
        elif k in (1, 2):  # the longest stream that ends no later than asked for
            want = m0 + cut - (0 if k == 1 else 777)
            n = frames_for_total(F, T, want)
            if out_frames(n, F, T) > want:
                n -= 1
        elif k == 3:
            n = frames_for_total(F, T, m0 + cut + 1500)
        else:
            n = live_frames(F, T, m0 + M)
        srcs.append((signal(rng, n * ch), ch, rate, GAINS[k % len(GAINS)]))
        frames.append(max(0, min(out_frames(n, F, T), m0 + M) - m0))
    return dict(m0=m0, M=M, cut=cut, srcs=srcs, frames=frames)


def alike_case(pair, to_ch=2, n_sources=6, seed=0):
    """Sources of the mixer's own layout and the pair's rate, all live but the last, which ends about 1500 frames behind the cut: the frames
    in front of its end are the uniform kernel's, cut once more where positions leave 32 bits."""
    rng = np.random.default_rng(seed)
    M, cut = pair.block, pair.cut
    m0, n_end = start_for(pair, pair.F, pair.T, cut + 1500)  # (the block starts where a stream of the pair's rate can end on frame cut + 1500)
    srcs = []
    for k in range(n_sources):
        n = live_frames(pair.F, pair.T, m0 + M) if k + 1 < n_sources else n_end
        srcs.append((signal(rng, n * to_ch), to_ch, pair.from_rate, GAINS[k % len(GAINS)]))
    end = out_frames(len(srcs[-1][0]) // to_ch, pair.F, pair.T) - m0
    return dict(m0=m0, M=M, cut=cut, srcs=srcs, end=end)


def largest_phase(pair, lo=1000, span=40000):
    """The mix frame in [lo, lo + span) at which the pair's phase m F mod T is largest."""
    return max(range(lo, lo + span), key=lambda m: m * pair.F % pair.T)
