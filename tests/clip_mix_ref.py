"""rh_clip_mix_block restated in numpy f32 with integer positions, from the Rust lines (a plain helper module like loop_mix_ref.py: no
fixtures).  Each arithmetic line is ONE f32 operation of the reference per element, in the reference's order.

    Amplify                 amplify.rs:64             sample * factor, innermost
    TakeDuration            take.rs:107-147           a sample is taken while remaining >= dps, dps = 10^9 // (rate * ch); remaining -= dps
      .. fade-out filter    take.rs:33-41             sample * float(remaining.as_millis()) / float(requested.as_millis()): two roundings
      .. current_span_len   take.rs:180-196           ALWAYS Some: min(inner span, samples the remaining duration admits)
    Delay                   delay.rs:8-16,68-75,94-98 Z = delay_ns * ch * rate // 10^9 samples of 0.0 first; adds what is left of them to the inner span
    UniformSourceIterator   uniform.rs:56             a chain = current_span_len().min(32768) samples and a fresh SampleRateConverter
    SampleRateConverter     sample_rate.rs:131-201    output frame j of a chain: i = floor(j F / T); a + (b - a) * num / T (math.rs:25); the chain's
                                                      last frame verbatim; F == T passes samples through
    ChannelCountConverter   channels.rs:57-85         channel c < from: the input's; channel 1 of a mono source: its only one; otherwise 0.0
    Mixer                   mixer.rs:185-198          ((0 + v_0) + v_1) + ... in insertion order

The stream of a clip is Z zeros and then the N admitted samples, read as frames of ch samples by STREAM position.  Rule G (a take, or a sound
that answers Some(whole length)): chains cut it at every multiple of 32768 samples from position 0.  Rule C (no take, the sound answers
None): one chain.  The words are [kind, Z, N, take_ns, flags, done, total] of include/rodio_hip.h; a source whose words are None (or start
with 0) is player_mix_ref's plain source: rh_wide_mix_block's."""
import numpy as np

import player_mix_ref as PR

f32 = np.float32
CHAIN_SAMPLES = 32768
OK, INVALID, UNSUPPORTED = 0, "invalid", "unsupported"
PLAIN, RULE_G, RULE_C = 0, 1, 2
TAKE, FADE = 1, 2
NS_PER_MS = 1_000_000

reduced = PR.reduced
span_out = PR.stream_out_frames  # output frames of a complete chain of n input frames: rh_uniform_span_frames(n, F, T, 1)


class Src:
    """One source as rh_clip_mix_block sees it.  A clip: x = the sound from its in-point on (at least N samples), words as above.  A plain
    source: x = its samples from `data` on, words None, phase / last as rh_wide_mix_block reads them."""

    def __init__(self, x, ch, from_rate, frames, gain=1.0, words=None, phase=0, last=PR.LIVE):
        self.x, self.ch, self.from_rate, self.frames, self.gain = np.ascontiguousarray(x, dtype=f32).reshape(-1), ch, from_rate, frames, f32(gain)
        self.words = None if words is None or words[0] == 0 else [int(v) for v in words]
        self.phase, self.last = phase, last


def delay_samples(delay_ns, ch, rate):
    return delay_ns * ch * rate // 1_000_000_000


def ns_per_sample(ch, rate):
    return 1_000_000_000 // (rate * ch)


def clip_plan(n_samples, ch, rate, span_len=0, delay_ns=0, take_ns=None, fade_out=False):
    """rh_clip_plan: the words, or the refusal.  span_len 0: None; take_ns None: no take."""
    if fade_out and take_ns is None:
        return INVALID
    if span_len != 0 and span_len < n_samples:
        return UNSUPPORTED
    Z, N = delay_samples(delay_ns, ch, rate), n_samples
    if take_ns is not None:
        N = min(N, take_ns // ns_per_sample(ch, rate))
    kind = RULE_G if take_ns is not None or span_len != 0 else RULE_C
    Ls = Z + N
    if Ls % ch or (kind == RULE_G and Ls > CHAIN_SAMPLES and CHAIN_SAMPLES % ch):
        return UNSUPPORTED
    return [kind, Z, N, take_ns or 0, (TAKE if take_ns is not None else 0) | (FADE if fade_out else 0), 0, 0]


def chains(words, ch):
    """(first stream sample, samples) of the converter chains of a clip, in order."""
    kind, Z, N = words[:3]
    Ls = Z + N
    assert Ls % ch == 0
    if kind == RULE_C:
        return [(0, Ls)] if Ls else []
    return [(p, min(CHAIN_SAMPLES, Ls - p)) for p in range(0, Ls, CHAIN_SAMPLES)]


def clip_out_frames(words, ch, from_rate, to_rate):
    F, T = reduced(from_rate, to_rate)
    return sum(span_out(n // ch, F, T) for _, n in chains(words, ch))


def clip_advance(words, ch, from_rate, to_rate, out_frames):
    """rh_clip_advance: the cursor behind out_frames more output frames (it stops at the end), and the clip's output frames."""
    if words[0] == PLAIN:
        return list(words)
    total = clip_out_frames(words, ch, from_rate, to_rate)
    return list(words[:5]) + [min(words[5] + out_frames, total), total]


def stream(x, gain, words, ch, rate):
    """The Z + N samples Delay(TakeDuration(Amplify(x))) emits."""
    _, Z, N, take_ns, flags = words[:5]
    with np.errstate(all="ignore"):
        v = (np.ascontiguousarray(x, dtype=f32).reshape(-1)[:N] * f32(gain)).astype(f32)
        assert v.size == N
        if flags & FADE:
            k = np.arange(N, dtype=np.int64)
            remaining = take_ns - k * ns_per_sample(ch, rate)
            assert N == 0 or remaining.min() >= ns_per_sample(ch, rate)
            R = (remaining // NS_PER_MS).astype(f32)
            v = (v * R).astype(f32)
            v = (v / f32(take_ns // NS_PER_MS)).astype(f32)
    return np.concatenate([np.zeros(Z, f32), v])  # (rodio's zeros are +0.0 and are not multiplied)


def chain_out(v, F, T):
    """A fresh SampleRateConverter over the f frames v [f, ch]: [span_out(f), ch]."""
    f = v.shape[0]
    j = np.arange(span_out(f, F, T), dtype=np.int64)
    i, num = (j * F) // T, (j * F) % T
    assert f == 0 or i[-1] <= f - 1
    two = (i + 1 < f) & (F != T)
    a = v[i]
    b = v[np.where(two, i + 1, i)]
    with np.errstate(all="ignore"):
        lerp = a + (b - a) * num.astype(f32)[:, None] / f32(T)
    return np.where(two[:, None], lerp, a).astype(f32)


def clip_whole(s, to_rate):
    """SampleRateConverter chain by chain over the whole clip: [total, ch] in the source's layout."""
    F, T = reduced(s.from_rate, to_rate)
    S = stream(s.x, s.gain, s.words, s.ch, s.from_rate)
    parts = [chain_out(S[p:p + n].reshape(-1, s.ch), F, T) for p, n in chains(s.words, s.ch)]
    return np.concatenate(parts) if parts else np.zeros((0, s.ch), f32)


def converted(s, channels, to_rate):
    """ChannelCountConverter(SampleRateConverter(..)) of one source for the block: [frames, channels]."""
    if s.words is None:
        return PR.converted(PR.Src(s.x, s.ch, s.from_rate, s.frames, gain=s.gain, phase=s.phase, last=s.last), channels, to_rate)
    if s.frames == 0:
        return np.zeros((0, channels), f32)
    whole = clip_whole(s, to_rate)
    done = s.words[5]
    assert done + s.frames <= whole.shape[0], "the block reaches behind the clip's end"
    r = whole[done:done + s.frames]
    out = np.zeros((s.frames, channels), f32)
    for c in range(channels):
        if c < s.ch:
            out[:, c] = r[:, c]
        elif c == 1 and s.ch == 1:
            out[:, c] = r[:, 0]
    return out


def clip_mix(channels, to_rate, out_frames, srcs):
    out = np.zeros((out_frames, channels), f32)
    with np.errstate(all="ignore"):
        for s in srcs:
            out[: s.frames] = out[: s.frames] + converted(s, channels, to_rate)
    return out.reshape(-1)
