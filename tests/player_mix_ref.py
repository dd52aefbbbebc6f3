"""rh_player_mix_block restated in numpy f32, one rounded operation at a time, from the Rust lines (a plain helper module like
spatial_mix_ref.py: no fixtures).  Arrays stand for "every sample": each line below is ONE f32 operation of the reference per element, in the
reference's order -- no sums or fused forms of numpy's.

    Amplify::next           amplify.rs:64             sample * factor
    LinearGainRamp::next    linear_ramp.rs:79-110     elapsed = frame * (1e9 / rate) ns; elapsed >= total: 1 (end_gain with clamp_end); otherwise
                                                      p = secs(elapsed) / secs(total), factor = start * (1 - p) + end * p; sample * factor; the
                                                      same factor for every channel of a frame
    steps                   periodic.rs:63-77         sample k of the adapter's output takes entry (first + k) / period - first / period
    SampleRateConverter     sample_rate.rs:131-201    i = floor((phase + j F) / T); a + (b - a) * num / T (math.rs:25); the last frame verbatim;
                                                      F == T passes samples through
    ChannelCountConverter   channels.rs:57-85         channel c < from: the input's; channel 1 of a mono source: its only one; otherwise 0.0
    Mixer                   mixer.rs:185-198          ((0 + v_0) + v_1) + ... in insertion order; a source that has ended adds nothing
"""
from math import gcd

import numpy as np

f32 = np.float32
LIVE = 0xFFFFFFFF
NONE, RAMP, CLAMP = 0, 1, 2  # ramp kinds: none, clamp_end false (fade_in, linear_gain_ramp(.., false)), clamp_end true (fade_out)


class Src:
    """One source as rh_player_mix_block sees it.  x: its samples from `data` on (ch interleaved floats a frame); gain: the innermost
    Amplify; kind, ramp_ns, start, end, first_frame, ramp_rate: the ramp (ramp_rate None: from_rate); factors [entries] or None."""

    def __init__(self, x, ch, from_rate, frames, gain=1.0, kind=NONE, ramp_ns=0, start=1.0, end=1.0, first_frame=0, ramp_rate=None, factors=None, factor_period=1, factor_first=0,
                 phase=0, last=LIVE):
        self.x, self.ch, self.from_rate, self.frames, self.phase, self.last = np.ascontiguousarray(x, dtype=f32).reshape(-1), ch, from_rate, frames, phase, last
        self.gain, self.kind, self.ramp_ns, self.start, self.end, self.first_frame = f32(gain), kind, ramp_ns, f32(start), f32(end), first_frame
        self.ramp_rate = from_rate if ramp_rate is None else ramp_rate
        self.factors, self.factor_period, self.factor_first = None if factors is None else np.ascontiguousarray(factors, dtype=f32).reshape(-1), factor_period, factor_first


def reduced(from_rate, to_rate):
    g = gcd(from_rate, to_rate)
    return from_rate // g, to_rate // g


def taps(s, to_rate):
    """Per output frame the source reaches: the first tap's frame, num, and whether there is a second tap."""
    F, T = reduced(s.from_rate, to_rate)
    p = s.phase + np.arange(s.frames, dtype=np.int64) * F
    i, num = p // T, p % T
    return i, num, (i < s.last) & (F != T), T


def touched_frames(s, to_rate):
    """Source frames the block's taps touch, counted from data: 0 .. this - 1."""
    if s.frames == 0:
        return 0
    i, _, two, _ = taps(s, to_rate)
    return int(i[-1] + (1 if two[-1] else 0) + 1)


def reached_samples(s, channels, to_rate):
    """Samples of the source's stream, counted from data, up to the last one a tap of the block reads (the channel rule reads input
    channels 0 .. min(from, to) - 1): what a factor table must cover."""
    n = touched_frames(s, to_rate)
    return 0 if n == 0 else (n - 1) * s.ch + min(s.ch, channels)


def entries_needed(first, period, n_samples):
    return 0 if n_samples == 0 else (first + n_samples - 1) // period - first // period + 1


def secs(ns):
    """Duration::as_secs_f32 (math.rs:118-122): secs as f32 + nanos as f32 / 1e9."""
    ns = np.asarray(ns, dtype=np.uint64)
    whole, nanos = (ns // np.uint64(1_000_000_000)).astype(f32), (ns % np.uint64(1_000_000_000)).astype(f32)
    return whole + nanos / f32(1_000_000_000.0)


def ramp_factors(kind, ramp_ns, start, end, rate, frames):
    """LinearGainRamp's factor of the given frames of its stream (linear_ramp.rs:83-102)."""
    frames = np.asarray(frames, dtype=np.uint64)
    step = np.uint64(1_000_000_000 // rate)
    elapsed = frames * step
    with np.errstate(all="ignore"):
        p = secs(elapsed) / secs(ramp_ns)
        a = f32(start) * (f32(1.0) - p)
        b = f32(end) * p
        running = a + b
    after = f32(end) if kind == CLAMP else f32(1.0)
    return np.where(elapsed >= np.uint64(ramp_ns), after, running).astype(f32)


def adapted(s, n_frames):
    """Amplify_steps(LinearGainRamp(Amplify_gain(x))) for the first n_frames frames from data: [n_frames, ch]."""
    x = s.x[: n_frames * s.ch]
    if x.size < n_frames * s.ch:  # the last frame's channels behind the last one a tap reads: NaN, so that a use of them shows
        x = np.concatenate([x, np.full(n_frames * s.ch - x.size, np.nan, f32)])
    x = x.reshape(n_frames, s.ch)
    with np.errstate(all="ignore"):
        out = x * s.gain
        if s.kind != NONE:
            out = out * ramp_factors(s.kind, s.ramp_ns, s.start, s.end, s.ramp_rate, s.first_frame + np.arange(n_frames, dtype=np.int64))[:, None]
        if s.factors is not None:
            k = np.arange(n_frames * s.ch, dtype=np.int64).reshape(n_frames, s.ch)
            e = (s.factor_first + k) // s.factor_period - s.factor_first // s.factor_period
            out = out * s.factors[np.minimum(e, s.factors.size - 1)]  # (an entry past the table: only for the NaN samples above)
    return out.astype(f32)


def converted(s, channels, to_rate):
    """ChannelCountConverter(SampleRateConverter(..)) over the adapted source: [frames, channels]."""
    if s.frames == 0:
        return np.zeros((0, channels), f32)
    i, num, two, T = taps(s, to_rate)
    v = adapted(s, touched_frames(s, to_rate))
    a = v[i]
    b = v[np.where(two, i + 1, i)]
    with np.errstate(all="ignore"):
        lerp = a + (b - a) * num.astype(f32)[:, None] / f32(T)
    r = np.where(two[:, None], lerp, a).astype(f32)
    out = np.zeros((s.frames, channels), f32)
    for c in range(channels):
        if c < s.ch:
            out[:, c] = r[:, c]
        elif c == 1 and s.ch == 1:
            out[:, c] = r[:, 0]
    return out


def player_mix(channels, to_rate, out_frames, srcs):
    out = np.zeros((out_frames, channels), f32)
    with np.errstate(all="ignore"):
        for s in srcs:
            out[: s.frames] = out[: s.frames] + converted(s, channels, to_rate)
    return out.reshape(-1)


# ---- the planner's arithmetic, for tests that cut a whole stream into blocks --------------------------------------------------------------
def stream_out_frames(n, F, T):
    """Output frames of a continuous source of n frames (sample_rate.rs: every frame with both taps, plus the verbatim last one where an
    output frame lands on it)."""
    if n == 0:
        return 0
    if F == T:
        return n
    c1 = ((n - 1) * T + F - 1) // F
    return c1 + (1 if c1 * F < n * T else 0)


def block_of(x, ch, from_rate, to_rate, m0, m1, **adapters):
    """Output frames [m0, m1) of the WHOLE ended stream x as one block's source: data at the frame of the first tap, the phase, `last`
    counted from there, and the position words -- first_frame, factor_first -- moved by what lies in front of data (the factor table
    from the entry of data's first sample on)."""
    n = len(x) // ch
    F, T = reduced(from_rate, to_rate)
    i0, phase = (m0 * F) // T, (m0 * F) % T
    if m0 >= stream_out_frames(n, F, T):  # the stream has ended in front of the block
        return Src(np.zeros(0, f32), ch, from_rate, 0)
    a = dict(adapters)
    a["first_frame"] = a.get("first_frame", 0) + i0
    ff, fp = a.get("factor_first", 0), a.get("factor_period", 1)
    if a.get("factors") is not None:
        a["factors"] = np.asarray(a["factors"], f32)[(ff + i0 * ch) // fp - ff // fp:]
    a["factor_first"] = ff + i0 * ch
    return Src(x[i0 * ch:], ch, from_rate, min(m1, stream_out_frames(n, F, T)) - m0, phase=phase, last=n - 1 - i0, **a)
