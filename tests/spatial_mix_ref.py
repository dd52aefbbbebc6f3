"""rh_spatial_mix_block restated in numpy f32, one rounded operation at a time, from the Rust lines (a plain helper module like
live_filter_ref.py: no fixtures).  Arrays stand for "every frame": each line below is ONE f32 operation of the reference per element, in the
reference's order -- no sums, means or fused forms of numpy's.

    ChannelVolume::next   channel_volume.rs:71-88   mean = ((0 + s0) + s1 + ..) / channels, once per frame; sample = mean * volume[c]
    Amplify::next         amplify.rs:64             sample * factor
    steps                 periodic.rs:63-77         sample k of the adapter's output takes entry (first + k) / period - first / period
    SampleRateConverter   sample_rate.rs:131-201    i = floor((phase + j F) / T); a + (b - a) * num / T (math.rs:25); the last frame verbatim;
                                                    F == T passes samples through
    Mixer                 mixer.rs:185-198          ((0 + v_0) + v_1) + ... in insertion order; a source that has ended adds nothing
"""
from math import gcd

import numpy as np

f32 = np.float32


class Src:
    """One emitter as rh_spatial_mix_block sees it.  x: the source's samples from `data` on (in_ch interleaved floats a frame); gains
    [entries, channels]; factors [entries] or None."""

    def __init__(self, x, in_ch, from_rate, frames, gains, gain_period, gain_first=0, factors=None, factor_period=1, factor_first=0, phase=0, last=0xFFFFFFFF):
        self.x, self.in_ch, self.from_rate, self.frames, self.phase, self.last = np.ascontiguousarray(x, dtype=f32).reshape(-1), in_ch, from_rate, frames, phase, last
        self.gains, self.gain_period, self.gain_first = np.ascontiguousarray(gains, dtype=f32), gain_period, gain_first
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


def entries_needed(first, period, n_samples):
    return 0 if n_samples == 0 else (first + n_samples - 1) // period - first // period + 1


def emitter(s, channels, n_frames):
    """Amplify(ChannelVolume(x)) for the first n_frames frames: [n_frames, channels]."""
    x = s.x[: n_frames * s.in_ch].reshape(n_frames, s.in_ch)
    with np.errstate(all="ignore"):
        mean = f32(0.0) + x[:, 0]
        for c in range(1, s.in_ch):
            mean = mean + x[:, c]
        mean = mean / f32(s.in_ch)
        k = np.arange(n_frames, dtype=np.int64)[:, None] * channels + np.arange(channels, dtype=np.int64)[None, :]
        ge = (s.gain_first + k) // s.gain_period - s.gain_first // s.gain_period
        out = mean[:, None] * s.gains.reshape(-1, channels)[ge, np.arange(channels)[None, :]]
        if s.factors is not None:
            fe = (s.factor_first + k) // s.factor_period - s.factor_first // s.factor_period
            out = out * s.factors[fe]
    return out.astype(f32)


def converted(s, channels, to_rate):
    """SampleRateConverter over the emitter's output: [frames, channels]."""
    if s.frames == 0:
        return np.zeros((0, channels), f32)
    i, num, two, T = taps(s, to_rate)
    v = emitter(s, channels, touched_frames(s, to_rate))
    a = v[i]
    b = v[np.where(two, i + 1, i)]
    with np.errstate(all="ignore"):
        lerp = a + (b - a) * num.astype(f32)[:, None] / f32(T)
    return np.where(two[:, None], lerp, a).astype(f32)


def spatial_mix(channels, to_rate, out_frames, srcs):
    out = np.zeros((out_frames, channels), f32)
    with np.errstate(all="ignore"):
        for s in srcs:
            out[: s.frames] = out[: s.frames] + converted(s, channels, to_rate)
    return out.reshape(-1)


# ---- the planner's arithmetic, for tests that cut a whole stream into a block -------------------------------------------------------------
def stream_out_frames(n, F, T):
    """Output frames of a continuous source of n frames (sample_rate.rs: every frame with both taps, plus the verbatim last one where an
    output frame lands on it)."""
    if n == 0:
        return 0
    if F == T:
        return n
    c1 = ((n - 1) * T + F - 1) // F
    return c1 + (1 if c1 * F < n * T else 0)
