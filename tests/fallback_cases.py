"""What tests/test_gpu_fallbacks.py (the device) and tests/test_fallback_refs_cpu.py (the oracle) share: the numpy references of the one-row
entries, written from the reference's source and independent of the library, the inputs, and the shape tables with the host gates'
arithmetic that picked them.  Not a test module: nothing here touches a GPU."""
from math import gcd

import numpy as np

f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def signal(seed, n, scale=1.0):
    """Uniform noise with -0.0, +0.0 and full-scale samples sprinkled in (every 41st sample from the third on, in turn)."""
    x = (np.random.default_rng(seed).uniform(-1, 1, n) * scale).astype(f32)
    special = f32([-0.0, 1.0, -1.0, 0.99999994, -0.99999994, 0.0])
    pos = np.arange(2, n, 41)
    x[pos] = special[np.arange(len(pos)) % len(special)]
    return x


# ---------------------------------------------------------------------------------------------------------------- resampler ----
def reduced(frm, to):
    g = gcd(frm, to)
    return frm // g, to // g


def run_out_frames(n, F, T):
    """sample_rate.rs:131-201: every m whose two taps exist (floor(m F / T) <= n - 2), then ONE verbatim last frame if the next m lands on it."""
    if n == 0:
        return 0
    if F == T:
        return n
    c1 = ((n - 1) * T + F - 1) // F
    return c1 + (1 if c1 * F < n * T else 0)


def chunk_frames(frames, ch, span):
    """uniform.rs:50-97: the converter restarts every min(span, 32768) samples."""
    return frames if not span else max(1, min(frames, min(span, 32768) // ch))


def out_frames(frames, frm, to, ch, span=0):
    F, T = reduced(frm, to)
    c = chunk_frames(frames, ch, span)
    return sum(run_out_frames(min(c, frames - s), F, T) for s in range(0, frames, c)) if frames else 0


def ref_resample(x, frm, to, ch, span=0):
    """The closed form of the streaming lerp: i = m F // T and num = m F % T in Python integers per chunk, then a + (b - a) * f32(num) / f32(T) as
    three separate float32 operations (math.rs:23-26), the frame verbatim at i == n_chunk - 1."""
    F, T = reduced(frm, to)
    X = np.ascontiguousarray(x, dtype=f32).reshape(-1, ch)
    n = len(X)
    c = chunk_frames(n, ch, span)
    Tf = f32(T)
    outs = []
    for s in range(0, n, c):
        xs = X[s: s + c]
        nc = len(xs)
        if F == T:
            outs.append(xs)
            continue
        M = run_out_frames(nc, F, T)
        i = np.array([m * F // T for m in range(M)], dtype=np.int64)
        num = np.array([m * F % T for m in range(M)], dtype=np.int64).astype(f32)
        assert M == 0 or (i[-1] <= nc - 1 and (M == 1 or i[-2] <= nc - 2))
        verbatim = i == nc - 1
        a, b = xs[i], xs[np.minimum(i + 1, nc - 1)]
        d = b - a
        p = d * num[:, None]
        q = p / Tf
        o = a + q
        o[verbatim] = a[verbatim]
        outs.append(o)
    return np.concatenate(outs).reshape(-1) if outs else np.zeros(0, f32)


def oracle_resample(O, x, frm, to, ch, span=0):
    if span:
        return O.UniformSourceIterator(O.SpanSource(x, ch, frm, span), ch, to).collect()
    return O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()


def resample_tile_frames(outf, frm, to, ch, kb_knob=None):
    """rh_resample_linear's gate, restated: the output frames of a tile.  Below 16 the row goes to the lane-per-frame kernel."""
    F, T = reduced(frm, to)
    per_frame = 4.0 * ch * (1.0 + F / T)
    kb = 32
    if kb_knob is not None and 1 <= kb_knob <= 48:
        kb = kb_knob
    else:
        while kb > 8 and outf * per_frame < 128.0 * kb * 1024.0:
            kb //= 2
    return int(kb * 1024.0 / per_frame) & ~3


# (from, to, channels): channels * (1 + F / T) > 128, so a tile of 8 KiB holds fewer than 16 frames (> 256 where the row is long enough for 16 KiB)
LANE_RATES = [(192000, 1000, 1), (192000, 1000, 2), (96000, 1001, 2), (96000, 1001, 3), (48000, 4000, 16), (44100, 48000, 96)]


def lane_lengths(frm, to):
    """1 frame, 2 frames, one frame either side of a multiple of F, and a row of about 2000 output frames (a few workgroups; 3000 would let the
    narrower layouts back into the tile kernel: their rows then pass 2 MiB and the gate doubles the tile)."""
    F, T = reduced(frm, to)
    k = 3 if 3 * T <= 2000 else 1
    return [1, 2, k * F - 1, k * F, k * F + 1, (2001 * F) // T + 5]


def lane_spans(ch):
    return [ch, ch * 40] + ([32768] if 32768 % ch == 0 else [])


# the rate / channel / span table of test_gpu_rows_alignment.py::test_resampler_rows_anywhere
ORDINARY_RATES = [(44100, 48000, 2, 0), (44100, 48000, 1, 0), (48000, 44100, 6, 0), (8000, 48000, 3, 0), (44100, 48000, 2, 96), (48000, 8000, 2, 32768)]
ORDINARY_FRAMES = (1, 2, 50, 20011)

# positions beyond 32 bits in under 1 MB: F = 65521 and T = 48000 are co-prime, F T < 2^32, and (out_frames + 1) F > 2^32 from 65 551 output
# frames on.  The spanned one needs a CHUNK that long, and a chunk is at most 32768 samples: 30000 -> 140003 mono (F T = 4 200 090 000).
WIDE_POS = [(65521, 48000, 1, 100000, 0), (65521, 48000, 2, 100000, 0), (65521, 48000, 5, 100000, 0), (30000, 140003, 1, 32768 + 1, 32768)]


def fits32(frames, frm, to, ch, span):
    F, T = reduced(frm, to)
    return (run_out_frames(chunk_frames(frames, ch, span), F, T) + 1) * F < 2 ** 32


# RH_PCM_TILE_KB: the rows of the issue (20011 frames), and a 12-channel one -- at 1 KiB a tile stereo still has 64 frames and 5.1 has 20, both
# stay on the tile kernel; 12 channels have 8 and drop to the lane kernel (from 2 KiB on they are back: 20 frames)
KB_ROWS = [(44100, 48000, 2, 0), (44100, 48000, 6, 0), (44100, 48000, 2, 96), (44100, 48000, 12, 0)]
KB_FRAMES = 20011
KB_VALUES = [1, 2, 5, 48, 0, 49]
KB_PCM = [("i16", 6, 2), ("f32", 2, 6)]


# -------------------------------------------------------------------------------------------------------------------- mixer ----
def ref_mix(srcs, starts, out_len):
    """mixer.rs:185-198: an f32 sum from +0.0 in insertion order, clipped to out_len."""
    acc = np.zeros(out_len, f32)
    for x, s in zip(srcs, starts):
        n = max(0, min(len(x), out_len - s))
        if n:
            acc[s: s + n] = acc[s: s + n] + x[:n]
    return acc


def oracle_mix(O, srcs, starts, out_len):
    """The oracle's Mixer has no late joins in the middle of an insertion order: a source that starts at s is `s` zeros and then its samples
    (adding +0.0 leaves a sum that began at +0.0 as it is)."""
    m = O.Mixer(1, 48000)
    for x, s in zip(srcs, starts):
        m.add(O.TestSource(np.concatenate([np.zeros(s, f32), x]), 1, 48000))
    got = m.collect()[:out_len]
    return np.concatenate([got, np.zeros(out_len - len(got), f32)])


def mix_layout(seed, n_sources, out_len, aligned, max_len=None):
    """Late joins, sources that end inside a 16-byte vector, a zero-length source, one that starts at out_len and one that would run past it.
    aligned: every start a multiple of 4 -- otherwise starts of every residue mod 4."""
    rng = np.random.default_rng(seed)
    max_len = max_len or out_len
    srcs, starts = [], []
    for s in range(n_sources):
        start = int(rng.integers(0, out_len // 4)) * 4 if s % 3 else 0
        if not aligned:
            start += s % 4
        ln = int(rng.integers(1, max_len + 1))
        if s % 5 == 1:
            ln = max(1, min(ln, out_len - start) - (s % 4))       # ends 0..3 samples in front of the end of the mix
        if s == 2:
            ln = 0                                                 # nothing to add
        if s == 4:
            start = (out_len + 3) // 4 * 4 if aligned else out_len  # starts where the mix ends (the next multiple of 4 where starts must be one)
        if s == 7:
            start, ln = ((out_len - 8) & ~3) + (0 if aligned else 1), 64   # would run past out_len
        starts.append(start)
        x = signal(seed * 1000 + s, ln)
        srcs.append(x)
    return srcs, starts


# ------------------------------------------------------------------------------------------------- channel count, channel volume ----
def ref_channels(x, frm_ch, to_ch):
    """channels.rs:57-85: out[f, k] = in[f, k] for k < from, in[f, 0] for k == 1 when from == 1, +0.0 otherwise."""
    X = np.ascontiguousarray(x, dtype=f32).reshape(-1, frm_ch)
    out = np.zeros((len(X), to_ch), f32)
    k = min(frm_ch, to_ch)
    out[:, :k] = X[:, :k]
    if frm_ch == 1 and to_ch >= 2:
        out[:, 1] = X[:, 0]
    return out.reshape(-1)


def oracle_channels(O, x, frm_ch, to_ch):
    return O.ChannelCountConverter(O.TestSource(x, frm_ch, 48000), frm_ch, to_ch).collect()


def ref_channel_volume(x, in_ch, gains):
    """channel_volume.rs:71-88: the frame's samples summed from 0.0 in order, / in_ch, times the channel's gain -- float32 throughout."""
    X = np.ascontiguousarray(x, dtype=f32).reshape(-1, in_ch)
    m = np.zeros(len(X), f32)
    for c in range(in_ch):
        m = m + X[:, c]
    m = m / f32(in_ch)
    return (m[:, None] * np.asarray(gains, f32)[None, :]).reshape(-1)


def oracle_channel_volume(O, x, in_ch, gains):
    return O.ChannelVolume(O.TestSource(x, in_ch, 48000), gains).collect()


# the smallest frames the tile kernels decline: 10240 // (frame_in_bytes + frame_out_bytes), rounded down to a multiple of 4, is below 8
WIDE_CHANNELS = [(319, 2), (2, 319), (1, 330), (400, 400)]
WIDE_CHANNELS_CONTROL = (318, 2)           # from + to = 320: still the tile kernel
WIDE_VOLUME = [(305, 16), (400, 2), (320, 1)]
WIDE_FRAMES = (1, 5, 1023)
# (format, from, to)
WIDE_PCM = [("i16", 640, 2), ("u8", 1300, 2), ("i24", 430, 1), ("i32", 319, 2), ("f32", 319, 2)]
WIDE_PCM24_CHANNELS = 183                  # rh_wav_decode keeps the layout: 183 * 3 + 183 * 4 = 1281 bytes a frame
ORDINARY_LAYOUTS = [(6, 2), (2, 6), (1, 2), (2, 1), (3, 5)]
ORDINARY_LAYOUT_FRAMES = (1, 5, 2049)
BYTE_OFFSETS = (0, 1, 2, 3, 5)
DECODE_LAYOUTS = [("u8", 2), ("i16", 6), ("i32", 3), ("f32", 2), ("u8", 1), ("i16", 1)]   # rh_wav_decode: the layout stays


def cut(frames, ch):
    """Samples of a data chunk that ends inside its last frame (a mono one cannot)."""
    return frames * ch - min(3, ch - 1)


def wide_pcm24_samples(frames):
    ch = WIDE_PCM24_CHANNELS
    return (frames * ch - 7, frames * ch - (ch - 1), frames * ch)


def pcm_tile_frames(frame_in_bytes, frame_out_bytes, kb=10):
    """rh::pcm_tile_try's (and rh_channel_volume's) gate, restated: the frames of a tile.  Below 8 the lane-per-output kernel runs."""
    return (kb * 1024 // (frame_in_bytes + frame_out_bytes)) & ~3


# ------------------------------------------------------------------------------------------------------------ samples from bytes ----
PCM = {  # format: (bytes a sample, bits_per_sample, is_float)
    "u8": (1, 8, 0), "i16": (2, 16, 0), "i24": (3, 24, 0), "i32": (4, 32, 0), "f32": (4, 32, 1),
}
INT_FORMATS = {"i8": (np.int8, 0, 128), "u8": (np.uint8, 128, 128), "i16": (np.int16, 0, 32768), "u16": (np.uint16, 32768, 32768)}


def ref_int_to_f32(v, fmt):
    """dasp_sample 0.11.0: unsigned goes through the signed type, then `s as f32 / 2^(bits - 1)`."""
    _, offset, scale = INT_FORMATS[fmt]
    return (np.asarray(v).astype(np.int64) - offset).astype(f32) / f32(scale)


def pcm_bytes(seed, fmt, n):
    """n samples of the format as the file holds them (little-endian), with both ends of the range among them."""
    rng = np.random.default_rng(seed)
    if fmt == "f32":
        return signal(seed, n).astype("<f4").view(np.uint8).copy()
    if fmt == "u8":
        v = rng.integers(0, 256, n, dtype=np.int64)
        v[:2] = [0, 255][: len(v[:2])]
        return v.astype(np.uint8)
    nbytes = PCM[fmt][0]
    lo, hi = -(1 << (8 * nbytes - 1)), (1 << (8 * nbytes - 1))
    v = rng.integers(lo, hi, n, dtype=np.int64)
    edge = [lo, hi - 1, -1, 0]
    v[: min(n, 4)] = edge[: min(n, 4)]
    return v.astype("<i4").view(np.uint8).reshape(-1, 4)[:, :nbytes].reshape(-1).copy()


def pcm_values(raw, fmt, n):
    """The integer (or float) samples, put together from their bytes: hound reads a byte stream (wav.rs:107-151)."""
    nbytes = PCM[fmt][0]
    b = np.asarray(raw[: n * nbytes], np.uint8).reshape(n, nbytes)
    if fmt == "f32":
        return np.ascontiguousarray(b).view("<f4").reshape(-1).astype(f32)
    if fmt == "u8":
        return b[:, 0].astype(np.int64) - 128
    v = np.zeros(n, np.int64)
    for j in range(nbytes - 1):
        v |= b[:, j].astype(np.int64) << (8 * j)
    return v | (b[:, nbytes - 1].view(np.int8).astype(np.int64) << (8 * (nbytes - 1)))   # sign-extended from the last byte


def ref_pcm_decode(raw, fmt, n, channels, to_channels=None):
    """wav.rs:94-172 then channels.rs:57-85: the samples / 2^(bits - 1) in float32, a cut last frame completed with +0.0, then the channel rule."""
    v = pcm_values(raw, fmt, n)
    if fmt != "f32":
        v = v.astype(f32) / f32(1 << (8 * PCM[fmt][0] - 1)) if fmt != "u8" else v.astype(f32) / f32(128)
    frames = (n + channels - 1) // channels
    x = np.concatenate([v, np.zeros(frames * channels - n, f32)])
    return x if to_channels is None else ref_channels(x, channels, to_channels)


def oracle_pcm_decode(O, raw, fmt, n, channels, to_channels=None):
    v = pcm_values(raw, fmt, n)
    if fmt == "u8":
        v = O.convert("u8_to_f32", (v + 128).astype(np.uint8))
    elif fmt != "f32":
        v = O.convert(fmt + "_to_f32", v.astype(np.int16 if fmt == "i16" else np.int32))
    frames = (n + channels - 1) // channels
    x = np.concatenate([v, np.zeros(frames * channels - n, f32)])
    return x if to_channels is None else oracle_channels(O, x, channels, to_channels)


# ---------------------------------------------------------------------------------------------------------- uniform wide blocks ----
# (channels, rate, to_rate): the blocks of test_gpu_widemix.py::test_wide_mix_alike_sources_take_the_uniform_kernel, every source live
WIDE_UNIFORM = [(6, 44100, 48000), (2, 44100, 48000), (6, 48000, 48000), (4, 96000, 44100), (1, 22050, 48000)]
WIDE_UNIFORM_SOURCES, WIDE_UNIFORM_FRAMES = 40, 3001


def wide_uniform_sources(ch, rate, to_rate):
    F, T = reduced(rate, to_rate)
    need = (WIDE_UNIFORM_FRAMES - 1) * F // T + 2
    rng = np.random.default_rng(800 + ch)
    return [(signal(9000 + 50 * ch + s, need * ch), float(f32(rng.uniform(0.2, 1.5)))) for s in range(WIDE_UNIFORM_SOURCES)]


def ref_wide_uniform(srcs, ch, rate, to_rate, frames):
    """Amplify, the lerp between the amplified taps, the ordered sum (amplify.rs:64, sample_rate.rs, mixer.rs:185-198) -- every source still running."""
    F, T = reduced(rate, to_rate)
    i = np.array([m * F // T for m in range(frames)], dtype=np.int64)
    num = np.array([m * F % T for m in range(frames)], dtype=np.int64).astype(f32)
    acc = np.zeros((frames, ch), f32)
    for x, g in srcs:
        X = x.reshape(-1, ch) * f32(g)
        a = X[i]
        if F != T:
            d = X[i + 1] - a
            p = d * num[:, None]
            a = a + p / f32(T)
        acc = acc + a
    return acc.reshape(-1)


def oracle_wide_uniform(O, srcs, ch, rate, to_rate, frames):
    m = O.Mixer(ch, to_rate)
    for x, g in srcs:
        m.add(O.TestSource(x, ch, rate).amplify(g))
    return m.collect()[: frames * ch]
