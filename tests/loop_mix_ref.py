"""rh_loop_mix_block restated in numpy f32 with integer positions, from the Rust lines (a plain helper module like player_mix_ref.py: no
fixtures).  Each arithmetic line is ONE f32 operation of the reference per element, in the reference's order.

    Repeat                  repeat.rs:37-44,58-64     never None; once a pass is exhausted it reports the parameters of the sound's start
    Buffered                buffered.rs:97-126,207-214 spans of current_span_len().unwrap_or(32768) samples; reports the span's WHOLE length
    UniformSourceIterator   uniform.rs:56             a chain = current_span_len().min(32768) samples and a fresh SampleRateConverter
    SampleRateConverter     sample_rate.rs:131-201    output frame j of a chain: i = floor(j F / T); a + (b - a) * num / T (math.rs:25); the chain's
                                                      last frame verbatim; F == T passes samples through
    Amplify                 amplify.rs:64             sample * factor, in front of the converter
    ChannelCountConverter   channels.rs:57-85         channel c < from: the input's; channel 1 of a mono source: its only one; otherwise 0.0
    Mixer                   mixer.rs:185-198          ((0 + v_0) + v_1) + ... in insertion order

Where the chains cut (the words [L, c, rule, chain_start, chain_out] of include/rodio_hip.h):
    rule 0   chains start over at every pass: L // c chains of c frames and one of L % c; the positions below walk a table of the pass's chains
    rule 1   chains of c frames of the unrolled stream: chain k behind the cursor's starts at (chain_start + k c) % L, both taps % L
A source whose words are None (or start with 0) is player_mix_ref's plain source: rh_wide_mix_block's."""
from math import gcd

import numpy as np

import player_mix_ref as PR

f32 = np.float32
CHAIN_SAMPLES = 32768
OK, INVALID, UNSUPPORTED = 0, "invalid", "unsupported"


class Src:
    """One source as rh_loop_mix_block sees it.  A loop: x = the L frames of the pass, words = [L, c, rule, chain_start, chain_out].  A plain
    source: x = its samples from `data` on, words None, phase / last as rh_wide_mix_block reads them."""

    def __init__(self, x, ch, from_rate, frames, gain=1.0, words=None, phase=0, last=PR.LIVE):
        self.x, self.ch, self.from_rate, self.frames, self.gain = np.ascontiguousarray(x, dtype=f32).reshape(-1), ch, from_rate, frames, f32(gain)
        self.words = None if words is None or words[0] == 0 else [int(v) for v in words]
        self.phase, self.last = phase, last


def reduced(from_rate, to_rate):
    g = gcd(from_rate, to_rate)
    return from_rate // g, to_rate // g


def span_out(n, F, T):
    """Output frames of a complete chain of n input frames: rh_uniform_span_frames(n, F, T, 1)."""
    return PR.stream_out_frames(n, F, T)


def chains_of_pass(L, c):
    """(first frame, frames) of the chains of one pass under rule 0."""
    return [(s, min(c, L - s)) for s in range(0, L, c)]


def loop_plan(n_samples, channels, span_len):
    """rh_loop_plan: the words, or UNSUPPORTED.  span_len 0: None."""
    if n_samples % channels:
        return UNSUPPORTED
    if span_len == 0 or span_len == n_samples:
        chain = min(n_samples, CHAIN_SAMPLES)
        rule = 1 if span_len and n_samples > CHAIN_SAMPLES else 0
    elif span_len <= CHAIN_SAMPLES:
        chain, rule = min(span_len, n_samples), 0
    else:
        return UNSUPPORTED
    if chain % channels:
        return UNSUPPORTED
    return [n_samples // channels, chain // channels, rule, 0, 0]


def loop_advance(words, from_rate, to_rate, out_frames):
    """rh_loop_advance, by walking chains (not by dividing): the cursor behind out_frames more output frames."""
    L, c, rule, start, out = words
    if L == 0:
        return list(words)
    F, T = reduced(from_rate, to_rate)
    left = out_frames
    while True:
        n = min(c, L - start) if rule == 0 else c
        room = span_out(n, F, T) - out
        if left < room:
            return [L, c, rule, start, out + left]
        left -= room
        out = 0
        start = (start + n) % L  # rule 0: the tail chain ends the pass; rule 1: c frames of the unrolled stream


def loop_taps(s, to_rate):
    """Per output frame the loop reaches: the frames of both taps (inside the pass), whether the second is taken, num, T."""
    L, c, rule, start, out = s.words
    F, T = reduced(s.from_rate, to_rate)
    m = np.arange(s.frames, dtype=np.int64)
    M = span_out(c, F, T)
    if rule == 0:
        chains = chains_of_pass(L, c)
        outs = np.array([span_out(n, F, T) for _, n in chains], dtype=np.int64)
        first = np.concatenate([[0], np.cumsum(outs)])  # output frame of the pass at which chain k starts
        p = (first[start // c] + out + m) % first[-1]
        k = np.searchsorted(first, p, side="right") - 1
        j = p - first[k]
        base = np.array([b for b, _ in chains], dtype=np.int64)[k]
        n = np.array([n for _, n in chains], dtype=np.int64)[k]
    else:
        q = out + m
        k, j = q // M, q % M
        base = (start + k * c) % L
        n = np.full(s.frames, c, dtype=np.int64)
    i, num = (j * F) // T, (j * F) % T
    assert np.all(i < n)
    two = (i + 1 < n) & (F != T)
    return (base + i) % L, (base + i + 1) % L, two, num, T


def converted(s, channels, to_rate):
    """ChannelCountConverter(SampleRateConverter(Amplify(..))) of one source: [frames, channels]."""
    if s.words is None:
        return PR.converted(PR.Src(s.x, s.ch, s.from_rate, s.frames, gain=s.gain, phase=s.phase, last=s.last), channels, to_rate)
    if s.frames == 0:
        return np.zeros((0, channels), f32)
    ia, ib, two, num, T = loop_taps(s, to_rate)
    with np.errstate(all="ignore"):
        v = (s.x[: s.words[0] * s.ch].reshape(s.words[0], s.ch) * s.gain).astype(f32)
        a = v[ia]
        b = v[np.where(two, ib, ia)]
        lerp = a + (b - a) * num.astype(f32)[:, None] / f32(T)
    r = np.where(two[:, None], lerp, a).astype(f32)
    out = np.zeros((s.frames, channels), f32)
    for c in range(channels):
        if c < s.ch:
            out[:, c] = r[:, c]
        elif c == 1 and s.ch == 1:
            out[:, c] = r[:, 0]
    return out


def loop_mix(channels, to_rate, out_frames, srcs):
    out = np.zeros((out_frames, channels), f32)
    with np.errstate(all="ignore"):
        for s in srcs:
            out[: s.frames] = out[: s.frames] + converted(s, channels, to_rate)
    return out.reshape(-1)


def unrolled(x, ch, passes):
    return np.tile(np.ascontiguousarray(x, dtype=f32).reshape(-1, ch), (passes, 1)).reshape(-1)


def stream_out_frames(words, from_rate, to_rate, passes):
    """Output frames of `passes` passes of a loop played from a fresh cursor, up to the start of the chain in which the finite unrolled
    copy ends: in front of it the finite stream and the infinite loop are the same stream."""
    L, c, rule, _, _ = words
    F, T = reduced(from_rate, to_rate)
    if rule == 0:
        return (passes - 1) * sum(span_out(n, F, T) for _, n in chains_of_pass(L, c))
    return ((passes * L) // c) * span_out(c, F, T)  # (its whole chains; the chain that is cut short by the copy's end is not the loop's)
