"""rh_queue_mix_block restated in numpy f32 with integer positions, from the Rust lines (a plain helper module like loop_mix_ref.py: no
fixtures).  Each arithmetic line is ONE f32 operation of the reference per element, in the reference's order.

    SourcesQueueOutput      queue.rs:130-192,218-241  forwards the CURRENT sound's span length, channels and rate (the next sound's once the
                                                      current one is exhausted); keep_alive_if_empty: silence behind the last sound
    SamplesBuffer           buffer.rs:76-82           current_span_len() = its WHOLE length, not what is left
    UniformSourceIterator   uniform.rs:56             a chain = current_span_len().min(32768) samples drawn from the QUEUE and a fresh converter
    SampleRateConverter     sample_rate.rs:131-201    output frame j of a chain: i = floor(j F / T); a + (b - a) * num / T (math.rs:25); the chain's
                                                      last frame verbatim; F == T passes samples through
    Amplify                 amplify.rs:64             sample * factor, per sound, in FRONT of the queue
    ChannelCountConverter   channels.rs:57-85         channel c < from: the input's; channel 1 of a mono source: its only one; otherwise 0.0
    Mixer                   mixer.rs:185-198          ((0 + v_0) + v_1) + ... in insertion order

The chain rule: a chain that starts at stream position p inside sound k takes min(samples_k, 32768) samples of the concatenated stream from p,
read as frames of (channels_k, rate_k).  It ends early only where the sounds run out without keep_alive (the queue has ENDED); with keep_alive
the samples it lacks are +0.0, no gain applied, and behind it the queue is SILENT.  The cursor [chain_start, chain_out, state, flags] of
include/rodio_hip.h.  A source without sounds is player_mix_ref's plain source: rh_wide_mix_block's."""
from math import gcd

import numpy as np

import player_mix_ref as PR

f32 = np.float32
CHAIN_SAMPLES = 32768
PLAYING, SILENT, ENDED = 0, 1, 2
OK, INVALID, UNSUPPORTED = 0, "invalid", "unsupported"


class Refused(Exception):
    def __init__(self, status):
        super().__init__(status)
        self.status = status


class Sound:
    def __init__(self, x, ch, rate, gain=1.0):
        self.x, self.ch, self.rate, self.gain = np.ascontiguousarray(x, dtype=f32).reshape(-1), ch, rate, f32(gain)

    @property
    def samples(self):
        return self.x.size


class Src:
    """One source as rh_queue_mix_block sees it.  A queue: sounds (from the one in which the chain in progress started) and the cursor
    words; frames = the block's output frames it reaches.  A plain source: x = its samples from `data` on, sounds None."""

    def __init__(self, frames, sounds=None, words=None, x=(), ch=0, from_rate=0, gain=1.0, phase=0, last=PR.LIVE):
        self.frames, self.sounds = frames, None if not sounds else list(sounds)
        self.words = [0, 0, PLAYING, 1] if words is None else [int(v) for v in words]
        self.x, self.ch, self.from_rate, self.gain, self.phase, self.last = np.ascontiguousarray(x, dtype=f32).reshape(-1), ch, from_rate, f32(gain), phase, last


def reduced(from_rate, to_rate):
    g = gcd(from_rate, to_rate)
    return from_rate // g, to_rate // g


def span_out(n, F, T):
    """Output frames of a complete chain of n input frames: rh_uniform_span_frames(n, F, T, 1)."""
    return PR.stream_out_frames(n, F, T)


def settle(sounds, k, off):
    while k < len(sounds) and off >= sounds[k].samples:
        k, off = k + 1, 0
    return k, off


class Chain:
    """The chain that starts at sample `off` of sounds[k]: ch, rate, n samples, runs = [(sound index or None for +0.0, offset in the sound,
    start in the chain, count)], and (k_next, off_next) where the stream stands behind it (k_next == len(sounds): run out)."""

    def __init__(self, sounds, k, off, keep_alive):
        self.k, self.off, self.ch, self.rate = k, off, sounds[k].ch, sounds[k].rate
        want, have, self.runs = min(sounds[k].samples, CHAIN_SAMPLES), 0, []
        while have < want and k < len(sounds):
            take = min(sounds[k].samples - off, want - have)
            self.runs.append((k, off, have, take))
            have, off = have + take, off + take
            k, off = settle(sounds, k, off)
        if have < want and keep_alive:
            self.runs.append((None, 0, have, want - have))
            have = want
        self.n, self.k_next, self.off_next = have, k, off

    def conv(self, to_rate):
        """(F, T, input frames, output frames); raises Refused(UNSUPPORTED) for what the entry leaves to the host path."""
        F, T = reduced(self.rate, to_rate)
        if F * T > 0xFFFFFFFF or self.n % self.ch:
            raise Refused(UNSUPPORTED)
        M = span_out(self.n // self.ch, F, T)
        if M * F > 0xFFFFFFFF:
            raise Refused(UNSUPPORTED)
        return F, T, self.n // self.ch, M

    def samples(self, sounds):
        """Its n samples behind their sounds' Amplify."""
        with np.errstate(all="ignore"):
            parts = [np.zeros(cnt, f32) if k is None else (sounds[k].x[off:off + cnt] * sounds[k].gain).astype(f32) for k, off, _, cnt in self.runs]
        return np.concatenate(parts)


def walk(sounds, words, to_rate, frames):
    """The chains of `frames` output frames from the cursor on: ([(chain, first output frame, count, frames of the chain emitted earlier)],
    the cursor behind them, dropped)."""
    sounds = sounds or []
    start, out, state, flags = words
    if state > ENDED or flags > 1 or (state != PLAYING and (start or out)):
        raise Refused(INVALID)
    if any(s.ch == 0 or s.rate == 0 for s in sounds):
        raise Refused(INVALID)
    if state == PLAYING and start and (not sounds or start >= sounds[0].samples):
        raise Refused(INVALID)
    segs, m = [], 0
    k, off = settle(sounds, 0, start) if state == PLAYING else (0, 0)
    while state == PLAYING:
        if k == len(sounds):
            if out:
                raise Refused(INVALID)
            state = SILENT if flags & 1 else ENDED
            break
        if m == frames:
            break
        c = Chain(sounds, k, off, bool(flags & 1))
        _, _, _, M = c.conv(to_rate)
        if out >= M:
            raise Refused(INVALID)
        cnt = min(M - out, frames - m)
        segs.append((c, m, cnt, out))
        m += cnt
        if out + cnt < M:
            out += cnt
            break
        out, k, off = 0, c.k_next, c.off_next
    if state == PLAYING:
        return segs, [off, out, state, flags], k
    return segs, [0, 0, state, flags], len(sounds)


def queue_advance(words, sounds, to_rate, out_frames):
    """rh_queue_advance: (the cursor behind out_frames more output frames, dropped)."""
    _, end, dropped = walk(sounds, words, to_rate, out_frames)
    return end, dropped


def converted(s, channels, to_rate):
    """ChannelCountConverter(SampleRateConverter(..)) of one source: [frames, channels]; a queue's frames behind its last chain are +0.0."""
    if s.sounds is None:
        return PR.converted(PR.Src(s.x, s.ch, s.from_rate, s.frames, gain=s.gain, phase=s.phase, last=s.last), channels, to_rate)
    out = np.zeros((s.frames, channels), f32)
    if s.frames == 0:
        return out
    for c, m0, cnt, prior in walk(s.sounds, s.words, to_rate, s.frames)[0]:
        F, T, n, _ = c.conv(to_rate)
        v = c.samples(s.sounds).reshape(n, c.ch)
        j = prior + np.arange(cnt, dtype=np.int64)
        i, num = (j * F) // T, (j * F) % T
        assert np.all(i < n)
        two = (i + 1 < n) & (F != T)
        with np.errstate(all="ignore"):
            a = v[i]
            b = v[np.where(two, i + 1, i)]
            lerp = a + (b - a) * num.astype(f32)[:, None] / f32(T)
        r = np.where(two[:, None], lerp, a).astype(f32)
        for k in range(channels):
            if k < c.ch:
                out[m0:m0 + cnt, k] = r[:, k]
            elif k == 1 and c.ch == 1:
                out[m0:m0 + cnt, k] = r[:, 0]
    return out


def queue_mix(channels, to_rate, out_frames, srcs):
    out = np.zeros((out_frames, channels), f32)
    with np.errstate(all="ignore"):
        for s in srcs:
            out[: s.frames] = out[: s.frames] + converted(s, channels, to_rate)
    return out.reshape(-1)


def tables(srcs, to_rate):
    """What the plan's tables must hold, source after source: segments as (m0, count, prior, ch, F, T, last frame, pieces) with pieces
    [(sound index within the source or -1, offset in the sound, start in the chain)]; a plain source: one segment of one piece (-2, 0, 0)."""
    out = []
    for s in srcs:
        if s.frames == 0:
            out.append([])
        elif s.sounds is None:
            F, T = reduced(s.from_rate, to_rate)
            out.append([(0, s.frames, 0, s.ch, F, T, s.last, [(-2, 0, 0)])])
        else:
            segs = []
            for c, m0, cnt, prior in walk(s.sounds, s.words, to_rate, s.frames)[0]:
                F, T, n, _ = c.conv(to_rate)
                segs.append((m0, cnt, prior, c.ch, F, T, n - 1, [(-1 if k is None else k, off, start) for k, off, start, _ in c.runs]))
            out.append(segs)
    return out


def stream_frames(sounds, keep_alive, to_rate):
    """Output frames of a queue played from a fresh cursor up to the end of its last chain."""
    total = 0
    k, off = settle(sounds, 0, 0)
    while k < len(sounds):
        c = Chain(sounds, k, off, keep_alive)
        total += c.conv(to_rate)[3]
        k, off = c.k_next, c.off_next
    return total
