"""Case data for rh_wide_mix_batch (tests/test_gpu_wide_batch.py; a plain helper module like spatial_mix_ref.py: no fixtures, numpy only).

A block of a mixer is the frames m0 .. m0 + M - 1 of its mix; `block_source` makes one source as the header of rh_wide_mix_block describes
it for that block -- the rows it holds from the first tap of frame m0 on, exactly up to where the header lets the block read, so that
an arena's poison begins where reading must end -- and `stream_block` describes a block of a source that is resident as a whole."""
from math import gcd

import numpy as np

NONE = 0xFFFFFFFF
f32 = np.float32
GAINS = [1.0, 0.5, -1.5, 0.0, 2.0, -0.25]  # zero and negative ones among them
RATES = [8000, 11025, 22050, 44100, 48000, 96000]


def reduced(rate, to_rate):
    g = gcd(rate, to_rate)
    return rate // g, to_rate // g


def lerp_ready(n, F, T):  # #m with floor(m F / T) <= n - 2: both taps of the lerp exist
    return 0 if n == 0 else ((n - 1) * T + F - 1) // F


def out_frames(n, F, T):  # ... plus the verbatim last frame, when an output frame lands on it (sample_rate.rs:193-200)
    if n == 0:
        return 0
    if F == T:
        return n
    c1 = lerp_ready(n, F, T)
    return c1 + (1 if c1 * F < n * T else 0)


def signal(rng, n):
    """n finite samples in [-1, 1) with -0.0, +0.0 and a few exact values among them"""
    x = rng.uniform(-1, 1, n).astype(f32)
    if n:
        k = rng.integers(0, n, max(1, n // 17))
        x[k] = rng.choice(np.array([-0.0, 0.0, 1.0, -1.0], f32), k.size)
    return x


def block_source(rng, ch, rate, gain, to_rate, m0, M, role):
    """-> dict(x, ch, rate, gain, phase, frames, last): x holds the source's frames from floor(m0 F / T) on.  role: "live" (it reaches every
    frame of the block; x ends with the second tap of frame m0 + M - 1), "ended" (its stream ends inside the block; x ends with its last
    frame) or "silent" (it ended before the block: frames == 0, no rows at all)."""
    F, T = reduced(rate, to_rate)
    i0, phase = m0 * F // T, m0 * F % T
    if role == "silent":
        return dict(x=np.zeros(0, f32), ch=ch, rate=rate, gain=gain, phase=phase, frames=0, last=0)
    if role == "live":
        n = m0 + M if F == T else (m0 + M - 1) * F // T + 2
        frames, last = M, NONE
    else:
        assert role == "ended"
        n = i0 + 1
        while out_frames(n, F, T) < m0 + max(1, M // 2):
            n += 1
        frames, last = out_frames(n, F, T) - m0, n - 1 - i0
        assert 1 <= frames <= M and n - 1 >= i0, (rate, to_rate, m0, M)
    return dict(x=signal(rng, (n - i0) * ch), ch=ch, rate=rate, gain=gain, phase=phase, frames=frames, last=last)


def mixed_batch(seed=2026):
    """The five mixers of the first test: (channels, rate, M, [sources]).  A mixer without sources, one source, five, 37 (more than a launch
    of rh_wide_mix_block holds; six rates, so more than four (rate, phase) pairs; layouts of 1, 2 and 6 channels), four.  Among the
    sources: blocks that are not the stream's first (phase != 0), sources that end inside the block, sources of no frames, F == T."""
    rng = np.random.default_rng(seed)
    mixers = [(1, 48000, 1, [])]
    mixers.append((2, 44100, 257, [block_source(rng, 6, 48000, 0.5, 44100, 1000, 257, "live")]))
    mixers.append((6, 48000, 1000, [block_source(rng, ch, rate, gain, 48000, 777, 1000, role) for ch, rate, gain, role in
                                    [(6, 44100, 1.0, "live"), (2, 44100, -1.5, "ended"), (1, 48000, 0.5, "live"), (3, 11025, 2.0, "silent"), (6, 96000, 0.0, "live")]]))
    many = []
    for k in range(37):
        role = "ended" if k % 9 == 4 else ("silent" if k == 20 else "live")
        many.append(block_source(rng, [1, 2, 6][k % 3], RATES[(k * 5 + k // 6) % 6], GAINS[k % 6], 96000, 12345, 4099, role))
    assert len({(s["rate"], s["phase"]) for s in many if s["frames"]}) == 6 and any(s["rate"] == 96000 and s["frames"] for s in many)
    mixers.append((3, 96000, 4099, many))
    mixers.append((2, 48000, 64, [block_source(rng, ch, rate, gain, 48000, 0, 64, role) for ch, rate, gain, role in
                                  [(2, 48000, 1.0, "live"), (1, 22050, -0.25, "live"), (2, 8000, 1.0, "ended"), (6, 44100, 0.5, "live")]]))
    return mixers


def ragged_batch(seed=7):
    """300 mixers of 2 sources x 33 frames and one of 3 sources x 70 000 frames: more mixers than CUs, and a ragged grid"""
    rng = np.random.default_rng(seed)
    mixers = [(2, 48000, 33, [block_source(rng, 2, 44100, GAINS[b % 6], 48000, b, 33, "live"), block_source(rng, 1, 22050, -0.5, 48000, b, 33, "ended" if b % 7 == 0 else "live")])
              for b in range(300)]
    mixers.append((2, 48000, 70000, [block_source(rng, 2, 44100, 1.0, 48000, 0, 70000, "live"), block_source(rng, 1, 22050, -0.5, 48000, 0, 70000, "ended"),
                                     block_source(rng, 2, 48000, 0.5, 48000, 0, 70000, "live")]))
    return mixers


def fill_table(arr, at, srcs, ptrs):
    """arr[at ..]: the WideSrc entries of one mixer's sources; ptrs: the device address of each source's x (None: no rows)"""
    for k, (s, p) in enumerate(zip(srcs, ptrs)):
        e = arr[at + k]
        e.data, e.channels, e.from_rate, e.phase, e.frames, e.last, e.gain = (p if s["frames"] else None), s["ch"], s["rate"], s["phase"], s["frames"], s["last"], s["gain"]
    return at + len(srcs)


def stream_block(n, ch, rate, to_rate, m, m_end):
    """Frames [m, m_end) of a mix, for a source whose whole stream of n frames is resident: (frame offset of `data`, phase, frames, last)"""
    F, T = reduced(rate, to_rate)
    i0 = m * F // T
    frames = max(0, min(out_frames(n, F, T), m_end) - m)
    return i0, m * F % T, frames, (n - 1 - i0 if n - 1 >= i0 else 0)
