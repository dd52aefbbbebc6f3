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
with 0) is player_mix_ref's plain source: rh_wide_mix_block's.

Two forms.  clip_whole() builds the whole stream, the Z zeros included, and converts it chain by chain: the one held against the oracle.
clip_window() computes only the chains (rule G) or frames (rule C) a block touches, with Python ints for everything that depends on Z or
on the cursor: the only one for delays and cursors beyond what can be built, held against clip_whole() by tests/test_clip_mix_cpu.py."""
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


def tap_of(words, ch, from_rate, to_rate, x):
    """Output frame x of a clip in Python ints, nothing else: (stream frame of the first tap, whether the next frame is read too, num)."""
    kind, Z, N = words[:3]
    F, T = reduced(from_rate, to_rate)
    Lf = (Z + N) // ch
    c = CHAIN_SAMPLES // ch if kind == RULE_G and Z + N > CHAIN_SAMPLES else Lf
    M = span_out(c, F, T)
    q, j = (x // M, x % M) if kind == RULE_G else (0, x)
    n = min(c, Lf - q * c)
    i, num = j * F // T, j * F % T
    assert i < n, "behind the clip's end"
    return q * c + i, i + 1 < n and F != T, num


def clip_window(s, to_rate):
    """The frames [done, done + frames) of a clip in the source's layout, [frames, ch], WITHOUT the stream: the delay's Z zeros are never
    built and no chain in front of the block is walked, so Z, done and take_ns may be anything below 2^62.  What depends on them is
    worked out in Python ints -- the chain in progress and the frame inside it (rule G), the first tap and its phase (rule C), the sound's
    sample under the block's first stream sample -- and only offsets from there, which a block keeps far inside 63 bits, are int64."""
    kind, Z, N, take_ns, flags, done = s.words[:6]
    ch, m = s.ch, np.arange(s.frames, dtype=np.int64)
    F, T = reduced(s.from_rate, to_rate)
    Lf = (Z + N) // ch
    assert (Z + N) % ch == 0
    if kind == RULE_G:
        c = CHAIN_SAMPLES // ch if Z + N > CHAIN_SAMPLES else Lf
        M = span_out(c, F, T)
        q0, j0 = done // M, done % M
        k, j = (j0 + m) // M, (j0 + m) % M            # chains behind the one in progress, the frame inside
        n = np.minimum(c, min(Lf - q0 * c, 1 << 62) - k * c)  # frames of chain q0 + k (the stream's last one may be shorter)
        assert n.min() > 0, "the block reaches behind the clip's end"
        i, num = (j * F) // T, (j * F) % T
        origin = q0 * c                                # stream frame the int64 offsets count from
        rel = k * c + i
    else:
        i0, r0 = done * F // T, done * F % T
        pos = r0 + m * F
        i, num = pos // T, pos % T
        origin, rel = i0, i
        n = np.full(s.frames, min(Lf - i0, 1 << 62), dtype=np.int64)
    assert np.all(i < n), "the block reaches behind the clip's end"
    two = (i + 1 < n) & (F != T)
    first = origin * ch - Z                            # the sound's sample under stream frame `origin` (negative: still in the delay)
    assert abs(first) < 1 << 62
    dps = ns_per_sample(ch, s.from_rate) if flags & TAKE else 0

    def frames_at(rel):
        kk = first + rel[:, None] * ch + np.arange(ch, dtype=np.int64)[None, :]  # samples of the sound
        on = kk >= 0
        if not on.any():  # the whole block lies in the delay: the sound is not looked at
            return np.zeros(kk.shape, f32)
        assert kk.max() < N
        safe = np.where(on, kk, 0)
        with np.errstate(all="ignore"):
            v = (s.x[safe] * s.gain).astype(f32)
            if flags & FADE:
                R = ((take_ns - safe * dps) // NS_PER_MS).astype(f32)
                v = (v * R).astype(f32)
                v = (v / f32(take_ns // NS_PER_MS)).astype(f32)
        return np.where(on, v, f32(0.0)).astype(f32)  # (rodio's zeros are +0.0 and are not multiplied)

    a = frames_at(rel)
    b = frames_at(np.where(two, rel + 1, rel))
    with np.errstate(all="ignore"):
        lerp = a + (b - a) * num.astype(f32)[:, None] / f32(T)
    return np.where(two[:, None], lerp, a).astype(f32)


def converted(s, channels, to_rate, windowed=False):
    """ChannelCountConverter(SampleRateConverter(..)) of one source for the block: [frames, channels].  windowed: clips by clip_window()."""
    if s.words is None:
        return PR.converted(PR.Src(s.x, s.ch, s.from_rate, s.frames, gain=s.gain, phase=s.phase, last=s.last), channels, to_rate)
    if s.frames == 0:
        return np.zeros((0, channels), f32)
    if windowed:
        r = clip_window(s, to_rate)
    else:
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


def clip_mix(channels, to_rate, out_frames, srcs, windowed=False):
    out = np.zeros((out_frames, channels), f32)
    with np.errstate(all="ignore"):
        for s in srcs:
            out[: s.frames] = out[: s.frames] + converted(s, channels, to_rate, windowed)
    return out.reshape(-1)


def clip_mix_window(channels, to_rate, out_frames, srcs):
    """clip_mix with every clip by clip_window(): the only form for delays, cursors and takes the whole stream cannot be built for."""
    return clip_mix(channels, to_rate, out_frames, srcs, windowed=True)


def clip_out_frames_wide(words, ch, from_rate, to_rate):
    """clip_out_frames without listing the chains: for streams of up to 2^62 samples."""
    kind, Z, N = words[:3]
    F, T = reduced(from_rate, to_rate)
    Lf = (Z + N) // ch
    if kind == RULE_C or Z + N <= CHAIN_SAMPLES:
        return span_out(Lf, F, T)
    c = CHAIN_SAMPLES // ch
    return (Lf // c) * span_out(c, F, T) + span_out(Lf % c, F, T)


def clip_advance_wide(words, ch, from_rate, to_rate, out_frames):
    total = clip_out_frames_wide(words, ch, from_rate, to_rate)
    return list(words[:5]) + [min(words[5] + out_frames, total), total]
