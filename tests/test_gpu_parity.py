"""Parity of the HIP path (through the C ABI) against the CPU oracle.  Needs an MI355X.

Bit-exact (np.array_equal) for conversions, channel mapping, resampling, amplify, reverb,
channel volume, sequential biquad and the ordered mixer sum; <= 1e-5 abs for limiter / AGC
(device log2f/exp2f/sqrtf) and for the fused, time-parallel filter pipeline (BASELINE tolerance:
"<=1e-5 abs f32 for resample/filter/mix").  Tests mirror the reference's own tests where those
exist (cited per test) and then widen to seeded random inputs and edge cases.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

TOL = 1e-5  # BASELINE.json north_star


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def rnd(seed, n, scale=1.0):
    return (np.random.default_rng(seed).uniform(-1, 1, n) * scale).astype(np.float32)


# =============================================================== reference golden vectors ====
def test_golden_resampler(G):
    # src/conversions/sample_rate.rs:356-387
    out = G.SampleRateConverter(G.TestSource([2.0, 16.0, 4.0, 18.0, 6.0, 20.0, 8.0, 22.0], 2, 2000), 2000, 3000, 2).collect()
    assert len(out) == 12
    assert np.trunc(out).tolist() == [2.0, 16.0, 3.0, 17.0, 4.0, 18.0, 6.0, 20.0, 7.0, 21.0, 8.0, 22.0]
    out = G.SampleRateConverter(G.TestSource([1.0, 14.0], 1, 1000), 1000, 7000, 1).collect()
    assert np.trunc(out).tolist() == [1.0, 2.0, 4.0, 6.0, 8.0, 10.0, 12.0, 14.0]
    out = G.SampleRateConverter(G.TestSource(np.arange(17), 1, 12000), 12000, 2400, 1).collect()
    assert out.tolist() == [0.0, 5.0, 10.0, 15.0]


def test_golden_resampler_properties(G):
    # quickcheck empty / identity / divide / multiply, sample_rate.rs:254-334
    assert len(G.SampleRateConverter(G.TestSource([], 2, 44100), 44100, 48000, 2).collect()) == 0
    rng = np.random.default_rng(11)
    for _ in range(6):
        ch, k = int(rng.integers(1, 6)), int(rng.integers(1, 12))
        base = int(rng.integers(1, 48001))
        x = rng.integers(-32768, 32767, size=int(rng.integers(0, 400))).astype(np.float32)
        x = x[: ch * (len(x) // ch)]
        assert np.array_equal(G.SampleRateConverter(G.TestSource(x, ch, base), base, base, ch).collect(), x)
        down = G.SampleRateConverter(G.TestSource(x, ch, base * k), base * k, base, ch).collect()
        assert np.array_equal(down, x.reshape(-1, ch)[::k].reshape(-1))
        up = G.SampleRateConverter(G.TestSource(x, ch, base), base, base * k, ch).collect()
        assert np.array_equal(up.reshape(-1, ch)[::k].reshape(-1), x)


def test_golden_channels(G):
    # src/conversions/channels.rs:114-143
    assert G.ChannelCountConverter(G.TestSource([1, 2, 3, 4, 5, 6], 3, 1), 3, 2).collect().tolist() == [1, 2, 4, 5]
    assert G.ChannelCountConverter(G.TestSource([1, 2, 3, 4, 5, 6, 7, 8], 4, 1), 4, 1).collect().tolist() == [1, 5]
    assert G.ChannelCountConverter(G.TestSource([1, 2, 3, 4], 1, 1), 1, 2).collect().tolist() == [1, 1, 2, 2, 3, 3, 4, 4]
    assert G.ChannelCountConverter(G.TestSource([1, 2], 1, 1), 1, 4).collect().tolist() == [1, 1, 0, 0, 2, 2, 0, 0]
    assert G.ChannelCountConverter(G.TestSource([1, 2, 3, 4], 2, 1), 2, 4).collect().tolist() == [1, 2, 0, 0, 3, 4, 0, 0]
    assert len(G.ChannelCountConverter(G.TestSource([1, 2, 3, 4], 2, 1), 2, 3).collect()) == 6
    assert len(G.ChannelCountConverter(G.TestSource([1, 2, 3, 4], 2, 1), 2, 1).collect()) == 2


def test_golden_mixer(G):
    # src/mixer.rs:208-341
    m = G.Mixer(1, 48000)
    m.add(G.SamplesBuffer(1, 48000, [10.0, -10.0, 10.0, -10.0]))
    m.add(G.SamplesBuffer(1, 48000, [5.0, 5.0, 5.0, 5.0]))
    assert [m.next() for _ in range(5)] == [15.0, -5.0, 15.0, -5.0, None]
    m = G.Mixer(2, 48000)  # channels_conv
    m.add(G.SamplesBuffer(1, 48000, [10.0, -10.0, 10.0, -10.0]))
    m.add(G.SamplesBuffer(1, 48000, [5.0, 5.0, 5.0, 5.0]))
    assert [m.next() for _ in range(9)] == [15.0, 15.0, -5.0, -5.0, 15.0, 15.0, -5.0, -5.0, None]
    m = G.Mixer(1, 96000)  # rate_conv
    m.add(G.SamplesBuffer(1, 48000, [10.0, -10.0, 10.0, -10.0]))
    m.add(G.SamplesBuffer(1, 48000, [5.0, 5.0, 5.0, 5.0]))
    assert [m.next() for _ in range(8)] == [15.0, 5.0, -5.0, 5.0, 15.0, 5.0, -5.0, None]
    m = G.Mixer(1, 48000)  # start_afterwards
    m.add(G.SamplesBuffer(1, 48000, [10.0, -10.0, 10.0, -10.0]))
    assert [m.next(), m.next()] == [10.0, -10.0]
    m.add(G.SamplesBuffer(1, 48000, [5.0, 5.0, 6.0, 6.0, 7.0, 7.0, 7.0]))
    assert [m.next() for _ in range(4)] == [15.0, -5.0, 6.0, 6.0]
    m.add(G.SamplesBuffer(1, 48000, [2.0]))
    assert [m.next() for _ in range(4)] == [9.0, 7.0, 7.0, None]
    m = G.Mixer(2, 48000)  # added_taking_phase_into_account
    m.add(G.SamplesBuffer(2, 48000, [10.0, -10.0, 10.0, -10.0]))
    assert m.next() == 10.0
    m.add(G.SamplesBuffer(2, 48000, [5.0, -5.0, 6.0, -6.0]))
    assert m.next() == -10.0
    assert m.next() == 15.0


def test_mixer_channel_position_advances_on_none_like_the_reference(G, O):
    """mixer.rs:120-136: an empty MixerSource returns None AND advances its channel position; a source added after an odd
    number of such calls waits for the next frame boundary (one more None).  The mirror and the oracle's MixerSource are driven
    with the same sequence of calls."""
    rng = np.random.default_rng(77)
    for trial in range(6):
        gm, om = G.Mixer(2, 48000), O.Mixer(2, 48000)
        got, ref = [], []
        for step in range(8):
            kind = rng.integers(0, 3)
            if kind == 0:  # a few calls, empty or not
                k = int(rng.integers(1, 6))
                got += [gm.next() for _ in range(k)]
                ref += [om.next() for _ in range(k)]
            else:  # a short stereo source joins
                x = rng.uniform(-1, 1, 2 * int(rng.integers(1, 5))).astype(np.float32)
                gm.add(G.SamplesBuffer(2, 48000, x))
                om.add(O.TestSource(x, 2, 48000))
                k = int(rng.integers(0, 4))
                got += [gm.next() for _ in range(k)]
                ref += [om.next() for _ in range(k)]
        got += [gm.next() for _ in range(12)]
        ref += [om.next() for _ in range(12)]
        assert got == ref, (trial, got, ref)


def test_golden_channel_volume(G):
    # src/source/channel_volume.rs:135-166
    f = np.float32
    out = G.ChannelVolume(G.TestSource([1.0, 2.0, 3.0], 1, 44100), [0.5, 0.8]).collect()
    assert out.tolist() == [f(1) * f(0.5), f(1) * f(0.8), f(2) * f(0.5), f(2) * f(0.8), f(3) * f(0.5), f(3) * f(0.8)]
    assert G.ChannelVolume(G.TestSource([1.0, 2.0, 3.0, 4.0], 2, 44100), [1.0]).collect().tolist() == [1.5, 3.5]
    assert G.ChannelVolume(G.TestSource([1.0, 3.0, 2.0, 4.0], 2, 44100), [0.5, 2.0]).collect().tolist() == [1.0, 4.0, 1.5, 6.0]


def test_golden_channel_volume_six_channels_from_stereo(G, O):
    # tests/channel_volume.rs:9-62
    x = rnd(12, 2 * 4001)
    out = G.ChannelVolume(G.TestSource(x, 2, 44100), [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]).collect()
    assert len(out) == 6 * 4001
    fr = out.reshape(-1, 6)
    assert np.all(fr[:, 2:] == 0.0) and np.any(fr[:, :2] != 0.0)
    assert np.array_equal(out, O.ChannelVolume(O.TestSource(x, 2, 44100), [1.0, 1.0, 0.0, 0.0, 0.0, 0.0]).collect())


# ==================================================================== random parity ====
@pytest.mark.parametrize("frm,to,ch,n", [
    (44100, 48000, 2, 100003), (48000, 44100, 2, 65537), (8000, 48000, 1, 5001), (44100, 40000, 2, 33333),
    (11025, 48000, 6, 4097), (48000, 8000, 3, 40001), (44100, 48000, 2, 1), (44100, 48000, 2, 2),
    (44100, 48000, 1, 147), (96000, 44100, 2, 321), (44100, 48000, 5, 999),
])
def test_resample_bit_exact(G, O, frm, to, ch, n):
    x = rnd(n, n * ch)
    ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
    out = G.SampleRateConverter(G.TestSource(x, ch, frm), frm, to, ch).collect()
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("frm,to,ch,n,span", [
    (44100, 48000, 1, 31_000_001, 0),   # longer than 2^32 / F frames: the position no longer fits 32 bits (sample_rate.rs keeps it per span; one span here)
    (44101, 48000, 2, 9_000_001, 0),    # F = 44101, T = 48000: a tile's remainder times its index passes 2^32 (the 64-bit branch of the tile's base)
    (48000, 44100, 2, 2_000_001, 0), (44100, 48000, 6, 700_001, 0), (44100, 48000, 2, 3_000_000, 32768), (44100, 48000, 2, 400_001, 96), (8000, 48000, 1, 300_001, 40),
])
def test_resample_tiles_long_rows_bit_exact(G, O, frm, to, ch, n, span):
    """rh_resample_linear's tile kernel (k_resample_tile): rows of many tiles, positions beyond 32 bits, spans shorter than a tile (a tile across
    several chunk boundaries: the frame-by-frame branch, and runs that do not fit the tile's LDS) -- against the oracle's pull loop, bit for bit."""
    x = rnd(n + 7, n * ch)
    if span:
        ref = O.UniformSourceIterator(O.SpanSource(x, ch, frm, span), ch, to).collect()
        out = G.UniformSourceIterator(G.SpanSource(x, ch, frm, span), ch, to).collect()
    else:
        ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
        out = G.SampleRateConverter(G.TestSource(x, ch, frm), frm, to, ch).collect()
    assert out.shape == ref.shape and np.array_equal(out.view(np.uint32), ref.view(np.uint32))


@pytest.mark.parametrize("seed", range(6))
def test_resample_tiles_random_geometries_bit_exact(G, O, seed):
    """Seeded random rates (small and large reduced denominators, up- and down-sampling by up to 8), layouts, lengths and spans through
    rh_resample_linear: tiles of whole converter periods and not, rows shorter than a tile, spans shorter than a tile, a last chunk of one frame."""
    rng = np.random.default_rng(4242 + seed)
    rates = [8000, 11025, 16000, 22050, 32000, 44100, 44101, 48000, 88200, 96000, 47999, 12345, 7, 3, 1000, 999, 192000]
    for _ in range(20):
        frm, to = (int(v) for v in rng.choice(rates, 2, replace=False))
        gq = int(np.gcd(frm, to))
        if max(frm, to) > 8 * min(frm, to) or (frm // gq) * (to // gq) > 0xffffffff:  # (the reference multiplies the reduced rates in u32, sample_rate.rs:157,173: refused)
            continue
        ch = int(rng.integers(1, 9))
        n = int(rng.choice([1, 2, 3, int(rng.integers(4, 400)), int(rng.integers(400, 30000)), int(rng.integers(30000, 250000))]))
        span = 0
        if rng.random() < 0.5:
            span = ch * int(rng.choice([1, 2, int(rng.integers(3, 60)), int(rng.integers(60, 5000)), 32768 // ch, 40000]))
            if span > 32768 and 32768 % ch:
                span = 0  # (uniform.rs:56 caps a span at 32768 samples: a cap that splits a frame is a case of its own, refused by the stand-alone entry)
        x = rnd(n + seed, n * ch)
        if span:
            ref = O.UniformSourceIterator(O.SpanSource(x, ch, frm, span), ch, to).collect()
            out = G.UniformSourceIterator(G.SpanSource(x, ch, frm, span), ch, to).collect()
        else:
            ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
            out = G.SampleRateConverter(G.TestSource(x, ch, frm), frm, to, ch).collect()
        assert out.shape == ref.shape and np.array_equal(out.view(np.uint32), ref.view(np.uint32)), (frm, to, ch, n, span)


@pytest.mark.parametrize("frm,to,ch,n,span", [
    (44100, 48000, 2, 100000, 32768), (44100, 48000, 2, 16384 * 3, 32768), (44100, 48000, 2, 16384 * 3 + 1, 32768),
    (48000, 44100, 2, 70001, 32768), (44100, 48000, 1, 5000, 300), (8000, 48000, 2, 999, 64),
    (48000, 8000, 2, 5003, 1000), (44100, 48000, 2, 100000, 1 << 22),
])
def test_uniform_chunked_bit_exact(G, O, frm, to, ch, n, span):
    # UniformSourceIterator restarts the converter every min(span,32768) samples: uniform.rs:50-97
    x = rnd(n + 1, n * ch)
    ref = O.UniformSourceIterator(O.SpanSource(x, ch, frm, span), ch, to).collect()
    out = G.UniformSourceIterator(G.SpanSource(x, ch, frm, span), ch, to).collect()
    assert np.array_equal(out, ref)


def test_uniform_samples_buffer_with_channel_change(G, O):
    x = rnd(5, 4 * 50000)
    ref = O.UniformSourceIterator(O.SamplesBuffer(4, 44100, x), 2, 48000).collect()
    out = G.UniformSourceIterator(G.SamplesBuffer(4, 44100, x), 2, 48000).collect()
    assert np.array_equal(out, ref)
    ref = O.UniformSourceIterator(O.SamplesBuffer(1, 22050, x[:40001]), 2, 48000).collect()
    out = G.UniformSourceIterator(G.SamplesBuffer(1, 22050, x[:40001]), 2, 48000).collect()
    assert np.array_equal(out, ref)
    # 3 channels, one span (< 32768 samples): fine
    ref = O.UniformSourceIterator(O.SamplesBuffer(3, 44100, x[:29997]), 2, 48000).collect()
    out = G.UniformSourceIterator(G.SamplesBuffer(3, 44100, x[:29997]), 2, 48000).collect()
    assert np.array_equal(out, ref)
    # 3 channels and more than 32768 samples: the reference's 32768-sample span cuts a frame in
    # two (uniform.rs:56) and rotates the channels from the second span on; the kernels do not
    # reproduce that and say so instead of guessing
    with pytest.raises(G.RhError) as e:
        G.UniformSourceIterator(G.SamplesBuffer(3, 44100, x[:60000]), 2, 48000)
    assert e.value.status == 3  # RH_ERR_UNSUPPORTED


@pytest.mark.parametrize("frm,to,ch", [(44100, 48000, 2), (48000, 44100, 2), (8000, 48000, 1), (96000, 44100, 3), (44100, 44100, 2), (1000, 7000, 1)])
def test_streaming_resampler_block_splits_equal_one_pass(G, O, frm, to, ch):
    # rh_resampler_*: the converter's state (position + current frame, sample_rate.rs:110-122) carried
    # across blocks: every split of the stream gives the bits of the one-pass converter
    import torch

    rng = np.random.default_rng(frm + to + ch)
    n = 20000
    x = rnd(frm % 97 + ch, n * ch)
    ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
    xd = torch.from_numpy(x).cuda()
    for trial in range(4):
        cuts = sorted(set(int(c) for c in rng.integers(0, n + 1, size=[0, 1, 7, 40][trial])))
        cuts = [0] + cuts + [n]
        if trial == 3:
            cuts += [n, n]  # empty blocks, also an empty flush block
        r = G.StreamingResampler(frm, to, ch)
        outs = []
        for k in range(len(cuts) - 1):
            outs.append(r.feed(xd[cuts[k] * ch: cuts[k + 1] * ch], flush=(k == len(cuts) - 2)))
        got = torch.cat(outs).cpu().numpy()
        assert np.array_equal(got, ref), (trial, len(got), len(ref))
        r.close()
    # the empty stream
    r = G.StreamingResampler(frm, to, ch)
    assert r.feed(xd[:0], flush=True).numel() == 0


@pytest.mark.parametrize("n,ns,ch", [(20000, 20_833_333, 2), (20000, 682_666_667 // 16, 2), (300, 10_000_000, 2), (5000, 3_000_000, 1)])
def test_streaming_reverb_block_splits_equal_one_pass(G, O, n, ns, ch):
    # rh_echo_*: the delayed clone's history carried across blocks; also blocks shorter than the delay
    import torch

    rng = np.random.default_rng(n + ch)
    x = rnd(n + 11, n - n % ch, 0.25)
    ref = O.TestSource(x, ch, 48000).reverb(ns, 0.3).collect()
    xd = torch.from_numpy(x).cuda()
    for trial in range(3):
        cuts = [0] + sorted(set(int(c) for c in rng.integers(0, len(x) + 1, size=[0, 5, 60][trial]))) + [len(x)]
        r = G.StreamingReverb(ns, 0.3, 48000, ch)
        outs = [r.feed(xd[cuts[k]: cuts[k + 1]]) for k in range(len(cuts) - 1)]
        outs.append(r.flush())
        got = torch.cat(outs).cpu().numpy()
        assert np.array_equal(got, ref), (trial, len(got), len(ref))
        r.close()


@pytest.mark.parametrize("a,b", [(6, 2), (2, 6), (1, 2), (1, 4), (2, 1), (3, 8), (8, 3), (2, 2), (5, 5)])
def test_channels_bit_exact(G, O, a, b):
    x = rnd(a * 10 + b, a * 10007)
    ref = O.ChannelCountConverter(O.TestSource(x, a, 48000), a, b).collect()
    out = G.ChannelCountConverter(G.TestSource(x, a, 48000), a, b).collect()
    assert np.array_equal(out, ref)


def test_sample_type_converter_exhaustive(G, O):
    # dasp_sample 0.11.0 formulas (parity unpinned by the reference): every i16 / u16 / i8 / u8 value
    i16 = np.arange(-32768, 32768, dtype=np.int16)
    assert np.array_equal(G.SampleTypeConverter(i16, "i16", "f32"), O.convert("i16_to_f32", i16))
    assert np.array_equal(G.SampleTypeConverter(i16, "i16", "f32"), i16.astype(np.float32) / np.float32(32768))
    u16 = np.arange(0, 65536, dtype=np.uint16)
    assert np.array_equal(G.SampleTypeConverter(u16, "u16", "f32"), O.convert("u16_to_f32", u16))
    i8 = np.arange(-128, 128, dtype=np.int8)
    assert np.array_equal(G.SampleTypeConverter(i8, "i8", "f32"), O.convert("i8_to_f32", i8))
    u8 = np.arange(0, 256, dtype=np.uint8)
    assert np.array_equal(G.SampleTypeConverter(u8, "u8", "f32"), O.convert("u8_to_f32", u8))
    rng = np.random.default_rng(9)
    i32 = rng.integers(-2**31, 2**31 - 1, 100003, dtype=np.int64).astype(np.int32)
    assert np.array_equal(G.SampleTypeConverter(i32, "i32", "f32"), O.convert("i32_to_f32", i32))
    i24 = rng.integers(-2**23, 2**23 - 1, 100003, dtype=np.int64).astype(np.int32)
    assert np.array_equal(G.SampleTypeConverter(i24, "i24", "f32"), O.convert("i24_to_f32", i24))
    # ragged length + unaligned tail
    assert np.array_equal(G.SampleTypeConverter(i16[:12345], "i16", "f32"), O.convert("i16_to_f32", i16[:12345]))


def test_wav_ingest_and_egress(G, O):
    # src/decoder/wav.rs:94-172 and src/wav_output.rs:62-96.  The data chunk is converted
    # on the device from the file bytes; expected values from the cited conversions (numpy + oracle).
    import struct

    from test_host_logic import _wav_bytes

    rng = np.random.default_rng(55)
    n = 30001  # odd: the stereo cases end mid-frame and get one sample of silence (wav.rs:161-169)
    i16 = rng.integers(-32768, 32768, n, dtype=np.int64).astype("<i2")
    src = G.WavDecoder(_wav_bytes(2, 44100, 16, i16.tobytes(), junk=True))
    assert (src.channels(), src.sample_rate()) == (2, 44100)
    got = src.collect()
    assert len(got) == n + 1 and got[-1] == 0.0 and np.array_equal(got[:n], O.convert("i16_to_f32", i16))
    u8 = rng.integers(0, 256, n, dtype=np.int64).astype(np.uint8)
    got = G.WavDecoder(_wav_bytes(1, 8000, 8, u8.tobytes())).collect()
    assert np.array_equal(got, (u8.astype(np.float32) - 128) / np.float32(128))
    i24 = rng.integers(-2 ** 23, 2 ** 23, n, dtype=np.int64)
    i24[:4] = [-2 ** 23, 2 ** 23 - 1, -1, 0]
    packed = b"".join(struct.pack("<i", int(v))[:3] for v in i24)
    got = G.WavDecoder(_wav_bytes(3, 48000, 24, packed, extensible=True)).collect()
    assert len(got) == n + (3 - n % 3) % 3 and np.array_equal(got[:n], O.convert("i24_to_f32", i24.astype(np.int32)))
    i32 = rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype("<i4")
    assert np.array_equal(G.WavDecoder(_wav_bytes(1, 96000, 32, i32.tobytes())).collect(), O.convert("i32_to_f32", i32))
    f32 = rnd(56, 2 * 5000)
    src = G.WavDecoder(_wav_bytes(2, 48000, 32, f32.astype("<f4").tobytes(), fmt_tag=3))
    assert np.array_equal(src.collect(), f32)
    # egress: wav_to_writer writes 32-bit float, whole frames only; reading it back returns the source
    back = G.WavDecoder(G.wav_to_bytes(G.TestSource(f32[:9999], 2, 48000)))  # 9 999 samples: the half frame is dropped
    assert (back.channels(), back.sample_rate()) == (2, 48000) and np.array_equal(back.collect(), f32[:9998])
    # a file -> file job stays on the device: decode -> amplify -> wav
    out = G.wav_to_bytes(G.WavDecoder(_wav_bytes(2, 44100, 16, i16[:30000].tobytes())).amplify(0.5))
    assert np.array_equal(np.frombuffer(out[44:], "<f4"), O.convert("i16_to_f32", i16[:30000]) * np.float32(0.5))


def test_wav_decode_and_channel_conversion_in_one_launch(G, O):
    """BASELINE config 5 as ONE launch (rh_wav_decode_channels): `UniformSourceIterator::new(decoder, to_ch, rate)` = wav.rs:94-172 then
    channels.rs:57-85.  Every sample format x down / up / mono -> n / same, a data chunk that ends inside its last frame (the silence that
    completes it is converted like a frame), bit-identical to the two launches and to the oracle's ChannelCountConverter over the decoded stream;
    the committed excerpt of the reference's music.wav against its golden 6 -> 2 vector."""
    import os
    import struct

    from test_host_logic import _wav_bytes

    rng = np.random.default_rng(57)
    cases = [(6, 16, 2), (6, 16, 8), (1, 16, 4), (2, 8, 1), (3, 24, 2), (5, 32, 5), (2, "f32", 6), (1, 8, 1), (7, 16, 3)]
    for ch, bits, to in cases:
        n = int(rng.integers(1000, 40000))
        n -= 1 if n % ch == 0 else 0  # (ends inside a frame wherever ch > 1)
        if bits == "f32":
            x = rnd(58, n)
            wav = _wav_bytes(ch, 48000, 32, x.astype("<f4").tobytes(), fmt_tag=3)
        elif bits == 8:
            wav = _wav_bytes(ch, 48000, 8, rng.integers(0, 256, n, dtype=np.int64).astype(np.uint8).tobytes())
        elif bits == 16:
            wav = _wav_bytes(ch, 48000, 16, rng.integers(-32768, 32768, n, dtype=np.int64).astype("<i2").tobytes())
        elif bits == 24:
            wav = _wav_bytes(ch, 48000, 24, b"".join(struct.pack("<i", int(v))[:3] for v in rng.integers(-2 ** 23, 2 ** 23, n, dtype=np.int64)), extensible=True)
        else:
            wav = _wav_bytes(ch, 48000, 32, rng.integers(-2 ** 31, 2 ** 31, n, dtype=np.int64).astype("<i4").tobytes())
        two = G.WavDecoder(wav)
        decoded = two.collect()
        assert len(decoded) % ch == 0
        want = O.ChannelCountConverter(O.TestSource(decoded, ch, 48000), ch, to).collect()
        two_launches = G.ChannelCountConverter(G.TestSource(decoded, ch, 48000), ch, to).collect()
        one = G.WavDecoderChannels(wav, to)
        assert (one.channels(), one.sample_rate()) == (to, 48000)
        got = one.collect()
        assert got.shape == want.shape, (ch, bits, to)
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)) and np.array_equal(got.view(np.uint32), two_launches.view(np.uint32)), (ch, bits, to)
    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    i16 = np.load(os.path.join(gdir, "music_excerpt_i16.npy"))
    i16 = i16[: (len(i16) // 6) * 6]
    got = G.WavDecoderChannels(_wav_bytes(6, 44100, 16, i16.astype("<i2").tobytes()), 2).collect()
    assert np.array_equal(got, np.load(os.path.join(gdir, "music_excerpt_6to2.npy")))
    # arguments
    import ctypes as C

    from rodio_amd import _lib

    m = C.c_uint64(7)
    assert _lib.lib.rh_wav_decode_channels(None, None, 0, 2, 16, 0, 2, C.byref(m), None) == 0 and m.value == 0  # nothing to do
    assert _lib.lib.rh_wav_decode_channels(None, None, 4, 2, 16, 0, 0, C.byref(m), None) == 1                  # to_channels is NonZero
    assert _lib.lib.rh_wav_decode_channels(None, None, 4, 2, 12, 0, 2, C.byref(m), None) in (1, 3)             # null pointers / an unofficial depth


def test_golden_music_excerpt_config5(G):
    # BASELINE config 5 on the committed excerpt of the reference's assets/music.wav
    # (tests/golden/make_golden.py): i16 -> f32 and ChannelCountConverter 6 -> 2, bit-exact
    import os

    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    i16 = np.load(os.path.join(gdir, "music_excerpt_i16.npy"))
    f32 = np.load(os.path.join(gdir, "music_excerpt_f32.npy"))
    got = G.SampleTypeConverter(i16, "i16", "f32")
    assert got.dtype == np.float32 and np.array_equal(got, f32)
    six = f32[: (len(f32) // 6) * 6]
    out = G.ChannelCountConverter(G.TestSource(six, 6, 44100), 6, 2).collect()
    assert np.array_equal(out, np.load(os.path.join(gdir, "music_excerpt_6to2.npy")))
    # and at block scale (the excerpt tiled x1024, 32 Mi samples): same bits, size-independent
    big = np.tile(i16, 1024)
    assert np.array_equal(G.SampleTypeConverter(big, "i16", "f32"), np.tile(f32, 1024))


def test_device_formats_egress_and_ingress(G, O):
    # the rest of cpal's formats either side of the path (stream.rs:555-568,
    # microphone.rs:280-291).  dasp_sample 0.11.0 formulas restated twice: the C++ oracle and numpy here.
    x = np.concatenate([rnd(21, 200001, 1.5), np.float32([0, -0.0, 1, -1, 0.99999994, -0.99999994, 0.5, -0.5, 2, -2, 300, -300,
                                                          np.nan, np.inf, -np.inf, 1e-9, -1e-9, 2.0 ** -24, -(2.0 ** -24)])])
    for dst in ("u8", "i24", "u24", "u32", "i64", "u64", "f64"):
        got = G.SampleTypeConverter(x, "f32", dst)
        assert np.array_equal(got, O.convert("f32_to_" + dst, x), equal_nan=(dst == "f64")), dst
    fin = x[np.isfinite(x)]
    with np.errstate(invalid="ignore", over="ignore"):
        i8 = np.clip(np.trunc(fin.astype(np.float32) * np.float32(128)), -128, 127).astype(np.int64)
        assert np.array_equal(G.SampleTypeConverter(fin, "f32", "u8"), (i8 + 128).astype(np.uint8))
        i32 = np.clip(np.trunc((fin * np.float32(8388608.0)).astype(np.float64)), -2.0 ** 31, 2.0 ** 31 - 1).astype(np.int64)
        assert np.array_equal(G.SampleTypeConverter(fin, "f32", "i24"), i32.astype(np.int32))
        assert np.array_equal(G.SampleTypeConverter(fin, "f32", "f64"), fin.astype(np.float64))
    assert G.SampleTypeConverter(np.float32([1.0]), "f32", "i24")[0] == 8388608  # unchecked container, not clamped to 24 bits
    rng = np.random.default_rng(23)
    u24 = rng.integers(0, 2 ** 24, 100003, dtype=np.int64).astype(np.int32)
    assert np.array_equal(G.SampleTypeConverter(u24, "u24", "f32"), O.convert("u24_to_f32", u24))
    assert np.array_equal(G.SampleTypeConverter(u24, "u24", "f32"), ((u24.astype(np.int64) - 8388608).astype(np.float32) / np.float32(8388608)))
    u32 = np.concatenate([rng.integers(0, 2 ** 32, 100003, dtype=np.uint64).astype(np.uint32), np.uint32([0, 1, 2 ** 31 - 1, 2 ** 31, 2 ** 31 + 1, 2 ** 32 - 1])])
    assert np.array_equal(G.SampleTypeConverter(u32, "u32", "f32"), O.convert("u32_to_f32", u32))
    i64 = np.concatenate([rng.integers(-2 ** 63, 2 ** 63 - 1, 100003, dtype=np.int64), np.int64([0, 1, -1, 2 ** 62, -2 ** 63, 2 ** 63 - 1])])
    assert np.array_equal(G.SampleTypeConverter(i64, "i64", "f32"), O.convert("i64_to_f32", i64))
    u64 = i64.view(np.uint64)
    assert np.array_equal(G.SampleTypeConverter(u64, "u64", "f32"), O.convert("u64_to_f32", u64))
    # dasp_sample is not vendored: whether its i64 -> f32 rounds once (`s as f32 / 2^63`, what ships) or twice (through f64) cannot be checked here.
    # The two readings differ by one ulp on values such as 2^62 + 2^38 + 1; the second one sits behind RH_DASP_I64_VIA_F64=1.
    from conftest import knobs

    odd = np.int64([2 ** 62 + 2 ** 38 + 1, -(2 ** 62 + 2 ** 38 + 1), 2 ** 61 + 2 ** 37 + 1])
    once, twice = O.convert("i64_to_f32", odd), O.convert("i64_to_f32_via_f64", odd)
    assert not np.array_equal(once, twice)  # the doubt is real
    assert np.array_equal(G.SampleTypeConverter(odd, "i64", "f32"), once)
    with knobs(RH_DASP_I64_VIA_F64="1"):
        assert np.array_equal(G.SampleTypeConverter(odd, "i64", "f32"), twice)
        assert np.array_equal(G.SampleTypeConverter(i64, "i64", "f32"), O.convert("i64_to_f32_via_f64", i64))
        assert np.array_equal(G.SampleTypeConverter(u64, "u64", "f32"), O.convert("u64_to_f32_via_f64", u64))
    f64 = np.concatenate([rng.uniform(-2, 2, 100003), [0.1, 1e-50, 1e50, -1e50, np.nan]])
    a, b = G.SampleTypeConverter(f64, "f64", "f32"), O.convert("f64_to_f32", f64)
    assert np.array_equal(a, b, equal_nan=True) and np.array_equal(a[:-1], f64[:-1].astype(np.float32))


def test_sample_type_converter_egress(G, O):
    # f32 -> device formats (src/stream.rs:538-545): saturation, truncation toward zero, NaN -> 0
    x = np.concatenate([rnd(1, 100000, 1.5), np.float32([0, -0.0, 1, -1, 0.99999, -0.99999, 2, -2, np.nan, np.inf, -np.inf, 1e-9])])
    for dst in ("i16", "u16", "i8", "i32"):
        assert np.array_equal(G.SampleTypeConverter(x, "f32", dst), O.convert(f"f32_to_{dst}", x)), dst


def test_take_duration_golden_and_bit_exact(G, O):
    # the reference's vectors (take.rs:247-280) ...
    nps = 1_000_000_000 // (44100 * 2)
    assert G.TestSource(np.ones(10, np.float32), 2, 44100).take_duration(nps * 5).collect().tolist() == [1.0] * 5 + [0.0]
    assert len(G.TestSource(np.ones(100, np.float32), 1, 48000).take_duration(int(np.float32(1e9) / np.float32(48000)) * 10).collect()) == 10
    assert len(G.TestSource(np.ones(100, np.float32), 1, 48000).take_duration(0).collect()) == 0
    # ... and the oracle: expiry mid-stream / mid-frame, input shorter than the duration, fade-out filter
    x = rnd(35, 6 * 20000)
    for ch, rate, ns, fade in [(2, 48000, 100_000_000, False), (2, 48000, 100_000_000, True), (6, 44100, 123_456_789, True),
                               (3, 44100, 11_337 * 7, False), (2, 48000, 10_000_000_000, True), (1, 8000, 1_000_000, True)]:
        xs = x[: (len(x) // ch) * ch]
        ref = O.TestSource(xs, ch, rate).take_duration(ns, fade).collect()
        got = G.TestSource(xs, ch, rate).take_duration(ns, fade).collect()
        assert np.array_equal(got, ref), (ch, rate, ns, fade, len(got), len(ref))


def test_take_duration_in_front_of_a_uniform_source_iterator(G, O):
    # take.rs:176-195: TakeDuration answers Some(what it still admits) over a generator that says None, so the iterator behind it converts in
    # chains of 32768 samples (88 206 samples: three chains) -- or in one, when the duration admits less than that
    x = rnd(36, 2 * 60000)
    for ch, rate, ns in [(2, 44100, 1_000_000_000), (2, 44100, 300_000_000), (1, 8000, 2_000_000_000), (2, 48000, 5_000_000_000)]:
        xs = x[: (len(x) // ch) * ch]
        assert G.TestSource(xs, ch, rate).take_duration(ns).current_span_len() == O.TestSource(xs, ch, rate).take_duration(ns).current_span_len()
        ref = O.UniformSourceIterator(O.TestSource(xs, ch, rate).take_duration(ns), 2, 44100 if rate == 48000 else 48000).collect()
        got = G.UniformSourceIterator(G.TestSource(xs, ch, rate).take_duration(ns), 2, 44100 if rate == 48000 else 48000).collect()
        assert len(got) == len(ref) and np.array_equal(got, ref), (ch, rate, ns, len(got), len(ref))


def test_config1_sine_resample_amplify_bit_exact(G, O):
    # BASELINE configs[0]: 1 x SineWave at 44.1 kHz -> SampleRateConverter to 48 kHz -> amplify(0.8), 10 s
    from conftest import sine_generator

    x = sine_generator(44100, 440.0, 441000)
    ref = O.SampleRateConverter(O.TestSource(x, 1, 44100), 44100, 48000, 1).amplify(0.8).collect()
    out = G.SampleRateConverter(G.TestSource(x, 1, 44100), 44100, 48000, 1).amplify(0.8).collect()
    assert len(out) == 480000 and np.array_equal(out, ref)


def test_golden_crossfade(G, O):
    # source/crossfade.rs:45-81 through the GPU adapters (take_duration + fade-out filter, fade_in, a two-source mixer)
    from test_oracle_golden import _crossfade

    d = np.arange(1, 11, dtype=np.float32)
    out = _crossfade(G, G.TestSource(d, 1, 1), G.TestSource(d, 1, 1), 5_000_000_001)
    assert len(out) == 5 and np.all(np.abs(out - np.array([1, 2, 3, 4, 5], np.float32)) < 1e-6)
    out = _crossfade(G, G.TestSource(d, 1, 1), G.TestSource(np.zeros(10, np.float32), 1, 1), 5_000_000_001)
    assert np.all(np.abs(out - np.array([1.0, 2.0 * 0.8, 3.0 * 0.6, 4.0 * 0.4, 5.0 * 0.2], np.float32)) < 1e-6)
    x, y = rnd(61, 48000), rnd(62, 48000)
    assert np.array_equal(_crossfade(G, G.TestSource(x, 1, 48000), G.TestSource(y, 1, 48000), 300_000_000),
                          _crossfade(O, O.TestSource(x, 1, 48000), O.TestSource(y, 1, 48000), 300_000_000))


def test_distortion_bit_exact(G, O):
    # src/source/distortion.rs:66-72
    x = np.concatenate([rnd(31, 100003, 2.0), np.float32([0, -0.0, 0.5, -0.5, np.inf, -np.inf])])
    for gain, thr in [(3.0, 0.5), (0.5, 2.0), (1.0, 0.0), (-4.0, 0.25)]:
        ref = O.TestSource(x, 1, 48000).distortion(gain, thr).collect()
        assert np.array_equal(G.TestSource(x, 1, 48000).distortion(gain, thr).collect(), ref)
    with pytest.raises(G.RhError):
        G.TestSource(x, 1, 48000).distortion(1.0, -1.0)


def test_linear_gain_ramp_golden_and_bit_exact(G, O):
    # the reference's own vectors (linear_ramp.rs:176-210) ...
    ones = np.ones(10, np.float32)
    assert G.TestSource(ones, 1, 1).linear_gain_ramp(4_000_000_000, 0.0, 1.0, True).collect().tolist() == [0.0, 0.25, 0.5, 0.75] + [1.0] * 6
    assert G.TestSource(ones, 1, 1).linear_gain_ramp(4_000_000_000, 0.0, 0.5, True).collect().tolist() == [0.0, 0.125, 0.25, 0.375] + [0.5] * 6
    # ... and the oracle on realistic streams: stereo 48 kHz (20 833 ns steps), 6 channels, fades
    x = rnd(33, 2 * 60000, 0.8)
    for ns, a, b, clamp in [(500_000_000, 0.0, 1.0, False), (500_000_000, 1.0, 0.0, True), (1_234_567_891, 0.3, 2.5, True), (10_000, 0.0, 1.0, False)]:
        ref = O.TestSource(x, 2, 48000).linear_gain_ramp(ns, a, b, clamp).collect()
        assert np.array_equal(G.TestSource(x, 2, 48000).linear_gain_ramp(ns, a, b, clamp).collect(), ref)
    x6 = rnd(34, 6 * 9000)
    assert np.array_equal(G.TestSource(x6, 6, 44100).fade_in(150_000_000).collect(), O.TestSource(x6, 6, 44100).fade_in(150_000_000).collect())
    assert np.array_equal(G.TestSource(x6, 6, 44100).fade_out(150_000_000).collect(), O.TestSource(x6, 6, 44100).fade_out(150_000_000).collect())
    # block streaming through sample_offset
    ref = O.TestSource(x, 2, 48000).fade_in(700_000_000).collect()
    a = G.TestSource(x[:50002], 2, 48000).linear_gain_ramp(700_000_000, 0.0, 1.0, False).collect()
    b = G.TestSource(x[50002:], 2, 48000).linear_gain_ramp(700_000_000, 0.0, 1.0, False, sample_offset=50002).collect()
    assert np.array_equal(np.concatenate([a, b]), ref)


@pytest.mark.parametrize("alg", ["TPDF", "RPDF", "HighPass", "GPDF"])
@pytest.mark.parametrize("ch,bits", [(1, 16), (2, 16), (2, 24), (6, 8)])
def test_dither_counter_based_noise(G, O, alg, ch, bits):
    # the same (seed, sample index) -> noise contract on both sides: bit-exact (GPDF: logf/cosf differ in the last bit)
    import torch
    from rodio_amd import _lib
    import ctypes as C

    n = ch * 30011
    x = rnd(2600 + ch, n, 0.8)
    for seed in (0, 0xDEADBEEFCAFE):
        ref = O.TestSource(x, ch, 48000).dither(bits, alg, seed).collect()
        out = G.TestSource(x, ch, 48000).dither(bits, alg, seed).collect()
        if alg == "GPDF":
            assert float(np.max(np.abs(out - ref))) <= 1e-7
        else:
            assert np.array_equal(out, ref)
        # stateless: blocks with the running sample offset equal one pass
        xd = torch.from_numpy(x).cuda()
        got = torch.empty_like(xd)
        cuts = [0, ch * 1, ch * 777, ch * 20000, n]
        for a, b in zip(cuts[:-1], cuts[1:]):
            st = _lib.lib.rh_dither(C.c_void_p(got[a:].data_ptr()), C.c_void_p(xd[a:].data_ptr()), b - a, a, ch, bits, G.GpuSource.DITHER[alg], seed, None)
            assert st == 0
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), out)
    assert _lib.lib.rh_dither(None, None, 0, 0, 2, 0, 3, 0, None) == 1  # BitDepth is NonZero
    assert _lib.lib.rh_dither(None, None, 0, 0, 2, 16, 4, 0, None) == 1


def test_amplify_bit_exact(G, O):
    x = rnd(2, 100001)
    for f in (1.2, 0.8, -0.3, 0.0):
        assert np.array_equal(G.TestSource(x, 2, 48000).amplify(f).collect(), O.TestSource(x, 2, 48000).amplify(f).collect())


@pytest.mark.parametrize("n,ns,amp,ch", [(100000, 682_666_667 // 16, 0.3, 2), (5000, 50_000_000, 0.7, 2),
                                         (100, 10_000_000, 0.5, 1), (0, 1_000_000, 0.5, 2), (3001, 20_833_333, 0.3, 2)])
def test_reverb_bit_exact(G, O, n, ns, amp, ch):
    # source/mod.rs:628-634; the last case has an ODD delay on stereo (channel swap) -- reproduced, not fixed
    x = rnd(n + 3, n - n % ch, 0.25)
    ref = O.TestSource(x, ch, 48000).reverb(ns, amp).collect()
    out = G.TestSource(x, ch, 48000).reverb(ns, amp).collect()
    assert np.array_equal(out, ref)


def test_reverb_delay_longer_than_source(G, O):
    x = rnd(8, 100, 0.25)
    ref = O.TestSource(x, 2, 48000).reverb(10_000_000, 0.3).collect()  # 960 samples of delay > 100
    assert np.array_equal(G.TestSource(x, 2, 48000).reverb(10_000_000, 0.3).collect(), ref)


@pytest.mark.parametrize("n,ns", [(2 * 4096, 682_666_667 // 64), (2 * 3001, 20_833_333), (2 * 1000, 10_000_000), (2 * 777, 31_250)])
def test_reverb_spatial_fused_batch_bit_exact(G, O, n, ns):
    # BASELINE config 3 in miniature: 5 streams, reverb -> Spatial, one fused launch vs the oracle's
    # two-adapter chain.  Cases: delay % 4 == 0 (vector path), an ODD delay (channel swap, half frame
    # dropped at the end), delay > source, delay of 3 samples.
    import torch

    S = 5
    xs = np.stack([rnd(40 + s, n, 0.25) for s in range(S)])
    em = [[0.5 + 0.01 * s, 0, 1] for s in range(S)]
    out = G.reverb_spatial_batch(torch.from_numpy(xs).cuda(), 48000, ns, 0.3, em, [-1, 0, 0], [1, 0, 0]).cpu().numpy()
    for s in range(S):
        ref = O.Spatial(O.TestSource(xs[s], 2, 48000).reverb(ns, 0.3), em[s], [-1, 0, 0], [1, 0, 0]).collect()
        assert out.shape[1] == len(ref)
        assert np.array_equal(out[s], ref)


def test_reverb_spatial_config3_full_size(G, O):
    # 64 sources x 2*2^20 samples @ 48 kHz, reverb(682 666 667 ns = 65 536 samples, 0.3), Spatial per source.
    # Oracle on 3 of the 64 rows in full; all rows against the unfused GPU ops (themselves oracle-exact).
    import torch

    # Inputs are BASELINE's: default_rng(5678 + s) * 0.25.  (bench.py --config 3 compares ALL 64 rows of its timed launch.)
    S, n = 64, 2 << 20
    host = np.stack([(np.random.default_rng(5678 + s).uniform(-1, 1, n) * 0.25).astype(np.float32) for s in range(S)])
    x = torch.from_numpy(host).cuda()
    em = [[0.5 + 0.01 * s, 0, 1] for s in range(S)]
    out = G.reverb_spatial_batch(x, 48000, 682_666_667, 0.3, em, [-1, 0, 0], [1, 0, 0])
    assert out.shape == (S, n + 65536)
    for s in (0, 17, 31, 46, 63):
        ref = O.Spatial(O.TestSource(host[s], 2, 48000).reverb(682_666_667, 0.3), em[s], [-1, 0, 0], [1, 0, 0]).collect()
        assert np.array_equal(out[s].cpu().numpy(), ref)
    for s in range(0, S, 7):
        two_step = G.Spatial(G.GpuSource(x[s], 2, 48000).reverb(682_666_667, 0.3), em[s], [-1, 0, 0], [1, 0, 0]).samples
        assert torch.equal(out[s], two_step)


def test_spatial_bit_exact(G, O):
    x = rnd(4, 2 * 50001, 0.25)
    for s in (0, 7, 63):
        e = [0.5 + 0.01 * s, 0, 1]
        ref = O.Spatial(O.TestSource(x, 2, 48000), e, [-1, 0, 0], [1, 0, 0]).collect()
        out = G.Spatial(G.TestSource(x, 2, 48000), e, [-1, 0, 0], [1, 0, 0]).collect()
        assert np.array_equal(out, ref)
    x6 = rnd(6, 6 * 1001)
    g = [0.5, 0.25, 1.0]
    assert np.array_equal(G.ChannelVolume(G.TestSource(x6, 6, 48000), g).collect(), O.ChannelVolume(O.TestSource(x6, 6, 48000), g).collect())


@pytest.mark.parametrize("kind,freq,ch,n", [("low_pass", 200, 2, 30001), ("low_pass", 1000, 1, 20000), ("high_pass", 300, 2, 25000),
                                            ("low_pass", 200, 6, 5000)])
def test_biquad_sequential_bit_exact(G, O, kind, freq, ch, n):
    x = rnd(freq + ch, n * ch)
    ref = getattr(O.TestSource(x, ch, 48000), kind)(freq).collect()
    out = getattr(G.TestSource(x, ch, 48000), kind)(freq).collect()
    assert np.array_equal(out, ref)




@pytest.mark.parametrize("kind,freq,q", [("low_pass", 200, 0.5), ("low_pass", 1000, 0.5), ("high_pass", 300, 0.5), ("low_pass", 800, 2.0), ("high_pass", 2000, 0.7071)])
def test_biquad_time_parallel_mode1(G, O, kind, freq, q):
    # rh_biquad mode 1 (time-parallel scan) against the sequential reference order (mode 0 == oracle bit
    # for bit) and the f64 recurrence: <= 1e-5 abs and no further from the truth than the f32 reference
    import torch

    S, n = 5, 100000
    x = np.stack([rnd(70 + s, 2 * n, 0.5) for s in range(S)])
    co = G.biquad_coeffs(kind, freq, q, 48000)
    xd = torch.from_numpy(x).cuda()
    seq = G.biquad_batch(xd, co, mode=0).cpu().numpy()
    par = G.biquad_batch(xd, co, mode=1).cpu().numpy()
    for s in (0, S - 1):
        src = O.TestSource(x[s], 2, 48000)
        ref = (src.low_pass(freq, q) if kind == "low_pass" else src.high_pass(freq, q)).collect()
        assert np.array_equal(seq[s].view(np.uint32), ref.view(np.uint32)), (s, float(np.max(np.abs(seq[s] - ref))))
    # f64 truth of the same recurrence
    c = co.astype(np.float64)
    truth = np.zeros_like(x, dtype=np.float64)
    xs = x.astype(np.float64).reshape(S, n, 2)
    y = truth.reshape(S, n, 2)
    x1 = np.zeros((S, 2)); x2 = np.zeros((S, 2)); y1 = np.zeros((S, 2)); y2 = np.zeros((S, 2))
    for t in range(n):
        r = c[0] * xs[:, t] + c[1] * x1 + c[2] * x2 - c[3] * y1 - c[4] * y2
        y[:, t] = r
        x2, x1, y2, y1 = x1, xs[:, t].copy(), y1, r
    e_par = float(np.max(np.abs(par - truth)))
    e_seq = float(np.max(np.abs(seq - truth)))
    d = float(np.max(np.abs(par - seq)))
    print(f"[biquad mode1 {kind}{freq} q={q}] |par-seq|={d:.3e} |par-f64|={e_par:.3e} |seq-f64|={e_seq:.3e} peak={float(np.max(np.abs(truth))):.3e}")
    assert d <= TOL
    assert e_par <= 2.0 * e_seq + 1e-7


@pytest.mark.parametrize("ch", [1, 2, 3])
def test_limiter(G, O, ch):
    sr = 48000
    t = np.arange(sr // 4) / sr
    x = np.repeat((np.sin(2 * np.pi * 440 * t) * 2.0).astype(np.float32), ch) * np.tile(np.linspace(0.5, 1.0, ch, dtype=np.float32), len(t))
    for thr in (-1.0, -6.0):
        ref = O.TestSource(x, ch, sr).limit(threshold=thr).collect()
        out = G.TestSource(x, ch, sr).limit(threshold=thr).collect()
        assert np.max(np.abs(out - ref)) <= TOL


def test_agc(G, O):
    x = rnd(21, 2 * 30000, 0.3)
    x[20000:] *= 3.0
    ref = O.TestSource(x, 2, 48000).automatic_gain_control().collect()
    out = G.TestSource(x, 2, 48000).automatic_gain_control().collect()
    assert np.max(np.abs(out - ref)) <= TOL
    ref = O.TestSource(x, 2, 48000).automatic_gain_control(target_level=0.5, attack_ns=10_000_000, release_ns=5_000_000, absolute_max_gain=5.0).collect()
    out = G.TestSource(x, 2, 48000).automatic_gain_control(target_level=0.5, attack_ns=10_000_000, release_ns=5_000_000, absolute_max_gain=5.0).collect()
    assert np.max(np.abs(out - ref)) <= TOL


@pytest.mark.parametrize("S,n", [(37, 20001), (150, 6001)])  # 150: more sources than one launch's table holds (128) -- the sum continues from the stored partial
def test_mixer_random_ordered_sum_bit_exact(G, O, S, n):
    # full-scale sources: only the reference's own summation order reproduces these bits
    mo, mg = O.Mixer(2, 48000), G.Mixer(2, 48000)
    for s in range(S):
        x = rnd(100 + s, 2 * (n - 13 * s))
        mo.add(O.TestSource(x, 2, 48000))
        mg.add(G.TestSource(x, 2, 48000))
    assert np.array_equal(mg.collect(), mo.collect())


# ====================================================================== fused pipeline ====
def _oracle_pipeline(O, xs, frm, to, span, filt, freq, ch=2, q=0.5):
    m = O.Mixer(ch, to)
    for x in xs:
        src = O.TestSource(x, ch, frm) if not span else O.SpanSource(x, ch, frm, span)
        u = O.UniformSourceIterator(src, ch, to)
        if filt == "low_pass":
            u = u.low_pass(freq, q)
        elif filt == "high_pass":
            u = u.high_pass(freq, q)
        m.add(u)
    return m.collect()


def _truth_pipeline(O, xs, frm, to, span, filt, freq, ch=2, q=0.5):
    """f64 evaluation of the same chain on the (bit-exact) f32 resampled streams: what both the
    reference's f32 recurrence and the GPU's time-parallel evaluation approximate."""
    from scipy.signal import lfilter

    co = O.blt_coeffs(filt, freq, q, to).astype(np.float64)
    acc = None
    for x in xs:
        src = O.TestSource(x, ch, frm) if not span else O.SpanSource(x, ch, frm, span)
        r = O.UniformSourceIterator(src, ch, to).collect().astype(np.float64).reshape(-1, ch)
        y = lfilter(co[:3], [1.0, co[3], co[4]], r, axis=0) if len(r) else r
        if acc is None or len(y) > len(acc):
            acc, y = (y.copy(), acc) if acc is not None else (y.copy(), None)
        if y is not None:
            acc[: len(y)] += y
    return acc.reshape(-1)


def _check_filtered(tag, out, ref, truth, abs_tol=TOL):
    """|gpu - oracle| within the BASELINE tolerance, and the GPU result no further from the exact
    (f64) answer than the reference's own f32 recurrence is (x2 + 1e-7 slack)."""
    assert len(out) == len(ref) == len(truth)
    err = float(np.max(np.abs(out - ref))) if len(ref) else 0.0
    e_gpu = float(np.max(np.abs(out - truth))) if len(ref) else 0.0
    e_ref = float(np.max(np.abs(ref - truth))) if len(ref) else 0.0
    peak = float(np.max(np.abs(truth))) if len(ref) else 1.0
    print(f"[{tag}] |gpu-oracle|={err:.3e} |gpu-f64|={e_gpu:.3e} |oracle-f64|={e_ref:.3e} peak={peak:.3e}")
    assert err <= abs_tol, (tag, err)
    assert e_gpu <= 2.0 * e_ref + 1e-7, (tag, e_gpu, e_ref)
    return err, peak


def _gpu_pipeline(G, xs, frm, to, span, filt, freq, **kw):
    import torch

    p = G.ResampleLowpassMix(frm, to, 2, span, filt, freq, 0.5, max_sources=len(xs), max_in_frames=max(len(x) // 2 for x in xs) or 1, **kw)
    ts = [torch.from_numpy(np.ascontiguousarray(x)).cuda() if len(x) else torch.empty(0, device="cuda") for x in xs]
    p.set_sources(ts)
    out = p.run()
    p.check_status()
    res = out.cpu().numpy().copy()
    geo = p.geometry()
    p.close()
    return res, geo


# (frames per lane, ring stages, general kernel): k_rlm_fast is what equal-length batches take;
# force_general runs the same batch through the ragged-batch kernel k_rlm_wave.  A sample of the geometries at 44.1 -> 48 kHz, on larger
# batches and three filters: test_gpu_fused_instances.py runs the full matrix, every row of the six instance tables at the rates that select it
GEOS = [(3, 2, 0), (4, 3, 0), (5, 2, 0), (6, 3, 0), (7, 2, 0), (8, 2, 0), (8, 3, 0), (8, 4, 0), (9, 2, 0), (10, 3, 0), (12, 3, 0), (16, 3, 0),
        (6, 2, 1), (8, 2, 1), (8, 3, 1)]


@pytest.mark.parametrize("R,NS,general", GEOS)
@pytest.mark.parametrize("span", [None, 32768])
def test_fused_resample_mix_bit_exact(G, O, R, NS, general, span):
    # filter off: the fused kernel must reproduce resampler + ordered mixer sum bit for bit
    S, n = 9, 40000
    xs = [rnd(300 + s, 2 * n) for s in range(S)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, span, None, 0)
    out, geo = _gpu_pipeline(G, xs, 44100, 48000, span, None, 0, frames_per_lane=R, ring_stages=NS, force_general=general)
    assert geo["general_kernel"] == general and geo["frames_per_lane"] == R
    assert len(out) == len(ref)
    assert np.array_equal(out, ref)


@pytest.mark.parametrize("frm,to", [(48000, 44100), (44100, 40000), (96000, 48000), (32000, 48000)])
def test_fused_other_ratios_bit_exact(G, O, frm, to):
    S, n = 5, 30011
    xs = [rnd(400 + s, 2 * n) for s in range(S)]
    ref = _oracle_pipeline(O, xs, frm, to, None, None, 0)
    out, _ = _gpu_pipeline(G, xs, frm, to, None, None, 0)
    assert np.array_equal(out, ref)


def _same_bits(out, ref):
    """Bit for bit, the sign of a zero included; NaNs where the reference has NaNs (payloads are not compared)."""
    if out.shape != ref.shape:
        return False
    nan = np.isnan(ref)
    return bool(np.array_equal(np.isnan(out), nan) and np.array_equal(out.view(np.uint32)[~nan], ref.view(np.uint32)[~nan]))


def _specials(seed, n, tiny=True):
    """Samples among which the lerp's `(b - a) * num / T` meets what a shortened division gets wrong: -0.0 (a fall to silence on an exact frame),
    values below 2^-120 (the end of a decaying tail; tiny=False leaves them out), and a burst of Inf / NaN (a broken decoder)."""
    rng = np.random.default_rng(seed)
    x = rnd(seed, n)
    k = rng.integers(0, n, n // 3)
    pool = [0.0, -0.0, 1e-33, 6e-30, -7e-25] + ([1e-40, -1e-40, 3e-39, -2.5e-38, 1.1754944e-38, -1e-36] if tiny else [])
    x[k] = rng.choice(np.array(pool, np.float32), k.size)
    x[n // 2: n // 2 + 400] = -0.0  # frames that start on a tap exactly (num == 0) with a negative slope towards them: t = -0.0
    x[n // 2 - 7] = -0.25
    j = n - n // 5
    x[j: j + 6] = np.array([np.inf, 1.0, -np.inf, np.nan, 0.5, np.inf], np.float32)
    return x


@pytest.mark.parametrize("frm,to", [(44100, 48000), (48000, 44100), (8000, 48000), (44100, 96000), (44101, 48000)])
def test_lerp_division_is_the_ieee_quotient(G, O, frm, to):
    """math.rs:25 divides by `denominator as f32`; a kernel may take three instructions for it only where that is the IEEE quotient
    (rh_common.h: div_lerp / lerp_div_fast_ok; tools/ubench/div_check.hip is the exhaustive run).  The stand-alone converter (mono / stereo / 5.1:
    it divides) on samples with zeros of both signs, subnormals, Inf and NaN -- the oracle's bits, the sign of every zero included; the fused
    converter + ordered sum without a filter the same on zeros, Inf and NaN, and within 1e-44 where nonzero |t| < 2^-120 meets the short division
    (the documented exception: one unit of a subnormal's last place)."""
    for ch, n in [(1, 30011), (2, 30011), (6, 5003)]:
        x = _specials(frm + ch, n * ch)
        ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
        out = G.SampleRateConverter(G.TestSource(x, ch, frm), frm, to, ch).collect()
        assert _same_bits(out, ref), (ch, frm, to)
    xs = [_specials(900 + s, 2 * 20011, tiny=False) for s in range(3)]
    for general in (0, 1):
        ref = _oracle_pipeline(O, xs, frm, to, None, None, 0)
        out, _ = _gpu_pipeline(G, xs, frm, to, None, None, 0, force_general=general)
        assert _same_bits(out, ref), (frm, to, general)
    x1 = [_specials(950, 2 * 20011, tiny=True)]  # one source: the sum does not hide anything
    ref = _oracle_pipeline(O, x1, frm, to, None, None, 0)
    out, _ = _gpu_pipeline(G, x1, frm, to, None, None, 0)
    ok = ~np.isnan(ref)
    assert np.array_equal(np.isnan(out), ~ok) and np.array_equal(np.isinf(out), np.isinf(ref))
    fin = ok & ~np.isinf(ref)
    assert np.max(np.abs(out[fin].astype(np.float64) - ref[fin].astype(np.float64))) <= 1e-44


def test_fused_ragged_lengths_bit_exact(G, O):
    ns = [40000, 1, 0, 2, 39999, 12345, 147, 148]
    xs = [rnd(500 + i, 2 * n) for i, n in enumerate(ns)]
    for span in (None, 32768):
        ref = _oracle_pipeline(O, xs, 44100, 48000, span, None, 0)
        out, _ = _gpu_pipeline(G, xs, 44100, 48000, span, None, 0, frames_per_lane=4)
        assert np.array_equal(out, ref)


def _report(tag, out, ref):
    err = float(np.max(np.abs(out - ref))) if len(ref) else 0.0
    peak = float(np.max(np.abs(ref))) if len(ref) else 1.0
    print(f"[{tag}] max_abs_err={err:.3e} peak={peak:.3e} rel_to_peak={err / max(peak, 1e-30):.3e}")
    return err, peak


@pytest.mark.parametrize("R,NS,general", GEOS)
@pytest.mark.parametrize("filt,freq", [("low_pass", 200), ("low_pass", 1000), ("high_pass", 300)])
def test_fused_filtered_pipeline(G, O, R, NS, general, filt, freq):
    # BASELINE config 2 at oracle-friendly size: 16 sources x 60000 frames, amplitude 1/16
    S, n = 16, 60000
    xs = [rnd(600 + s, 2 * n, 1.0 / S) for s in range(S)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, filt, freq)
    out, geo = _gpu_pipeline(G, xs, 44100, 48000, None, filt, freq, frames_per_lane=R, ring_stages=NS, force_general=general)
    assert geo["general_kernel"] == general
    truth = _truth_pipeline(O, xs, 44100, 48000, None, filt, freq)
    err, peak = _check_filtered(f"{filt}{freq} R{R} NS{NS} {'wave' if general else 'fast'} J{geo['lookback_tiles']}", out, ref, truth)
    assert err <= 2e-5 * peak + 1e-7  # and not merely because the inputs were scaled down


def test_fused_filtered_full_scale_inputs(G, O):
    # unscaled inputs: the f32 recurrence itself moves by ~1e-6 relative between evaluation
    # orders; tolerance is relative to the peak here
    S, n = 4, 50000
    xs = [rnd(700 + s, 2 * n) for s in range(S)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, "low_pass", 200)
    out, _ = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 200)
    truth = _truth_pipeline(O, xs, 44100, 48000, None, "low_pass", 200)
    _check_filtered("full-scale", out, ref, truth, abs_tol=2e-5)


def test_fused_filtered_long_lookback(G, O):
    # a 20 Hz low-pass has poles at ~0.9974: with 512-frame tiles the carry reaches back
    # dozens of tiles (J > 4), exercising the wide multi-tile gather
    S, n = 6, 50000
    xs = [rnd(800 + s, 2 * n, 1.0 / S) for s in range(S)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, "low_pass", 20)
    truth = _truth_pipeline(O, xs, 44100, 48000, None, "low_pass", 20)
    for general in (0, 1):
        out, geo = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 20, frames_per_lane=8, force_general=general)
        assert geo["lookback_tiles"] > 4 and geo["general_kernel"] == general
        _check_filtered(f"lookback J{geo['lookback_tiles']} general={general}", out, ref, truth)


def test_fused_filtered_chunked_and_ragged(G, O):
    ns = [50000, 16384, 16385, 1, 0, 33000, 49999]
    xs = [rnd(900 + i, 2 * n, 0.2) for i, n in enumerate(ns)]
    for span in (None, 32768):
        ref = _oracle_pipeline(O, xs, 44100, 48000, span, "low_pass", 200)
        out, _ = _gpu_pipeline(G, xs, 44100, 48000, span, "low_pass", 200, frames_per_lane=8)
        truth = _truth_pipeline(O, xs, 44100, 48000, span, "low_pass", 200)
        _check_filtered(f"ragged span={span}", out, ref, truth)


@pytest.mark.parametrize("S", [1, 2, 3])
@pytest.mark.parametrize("general", [0, 1])
def test_fused_fewer_sources_than_ring_stages(G, O, S, general):
    n = 20011
    xs = [rnd(1100 + s, 2 * n, 0.5) for s in range(S)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, "low_pass", 200)
    truth = _truth_pipeline(O, xs, 44100, 48000, None, "low_pass", 200)
    for ns in (2, 3):
        out, geo = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 200, frames_per_lane=8, ring_stages=ns, force_general=general)
        _check_filtered(f"S={S} NS={ns} general={general}", out, ref, truth)
    refp = _oracle_pipeline(O, xs, 44100, 48000, None, None, 0)
    outp, _ = _gpu_pipeline(G, xs, 44100, 48000, None, None, 0, force_general=general)
    assert np.array_equal(outp, refp)


@pytest.mark.parametrize("general", [0, 1])
def test_fused_more_tiles_than_resident_waves(G, O, general):
    # 3 sources x 3 Mi frames with 256-frame tiles: ~14 000 tiles, several times what the chip holds at
    # once, so late tiles start only when early ones have finished (ticket order keeps that safe)
    S, n = 3, 3 << 20
    xs = [rnd(1200 + s, 2 * n, 0.3) for s in range(S)]
    out, geo = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 200, frames_per_lane=(6 if general else 4), ring_stages=2, force_general=general)
    assert geo["n_tiles"] > 256 * geo["resident_waves_per_cu"] or geo["n_tiles"] > 8000
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, "low_pass", 200)
    err, peak = _report(f"many tiles general={general} tiles={geo['n_tiles']}", out, ref)
    assert err <= TOL and err <= 2e-5 * peak + 1e-7


@pytest.mark.parametrize("filt,freq", [("low_pass", 200), ("high_pass", 300), (None, 0)])
def test_fused_batch_mode_per_source_rows(G, O, filt, freq):
    # rh_rlm_run_batch: the same kernel without the mixer -- row s = UniformSourceIterator(src_s).low_pass(f)
    import torch

    S, n = 7, 40011
    xs = [rnd(1300 + s, 2 * n, 0.5) for s in range(S)]
    p = G.ResampleLowpassMix(44100, 48000, 2, None, filt, freq, 0.5, max_sources=S, max_in_frames=n, frames_per_lane=8)
    p.set_sources([torch.from_numpy(x).cuda() for x in xs])
    rows = p.run_batch().cpu().numpy()
    p.check_status()
    for s in range(S):
        ref = _oracle_pipeline(O, [xs[s]], 44100, 48000, None, filt, freq)
        assert rows.shape[1] == len(ref)
        if filt is None:
            assert np.array_equal(rows[s], ref)
        else:
            truth = _truth_pipeline(O, [xs[s]], 44100, 48000, None, filt, freq)
            _check_filtered(f"batch row {s} {filt}", rows[s], ref, truth)
    p.close()


@pytest.mark.parametrize("filt,freq,R", [("low_pass", 200, 8), ("high_pass", 300, 4), ("low_pass", 20, 8), (None, 0, 9)])
def test_fused_block_streaming_equals_one_pass(G, O, filt, freq, R):
    # rh_rlm_stream_*: the same sources fed block by block (random block lengths, including tiny ones);
    # the concatenation equals the one-pass mix: bit for bit without the filter, <= 1e-6 with it
    import torch

    S, n = 6, 50000
    rng = np.random.default_rng(77 + R)
    xs = [rnd(1400 + s, 2 * n, 1.0 / S) for s in range(S)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, filt, freq)
    p = G.ResampleLowpassMix(44100, 48000, 2, None, filt, freq, 0.5, max_sources=S, max_in_frames=n, frames_per_lane=R)
    xd = [torch.from_numpy(x).cuda() for x in xs]
    p.set_sources(xd)
    one = p.run().cpu().numpy().copy()
    for trial in range(3):
        cuts = [0] + sorted(set(int(c) for c in rng.integers(1, n, size=[1, 6, 25][trial]))) + [n]
        p.stream_begin()
        outs = []
        for k in range(len(cuts) - 1):
            outs.append(p.stream_feed([x[2 * cuts[k]: 2 * cuts[k + 1]] for x in xd], flush=(k == len(cuts) - 2)))
        p.check_status()
        got = torch.cat(outs).cpu().numpy()
        assert len(got) == len(ref), (trial, len(got), len(ref))
        if filt is None:
            assert np.array_equal(got, ref)
        else:
            d1, d2 = float(np.max(np.abs(got - one))), float(np.max(np.abs(got - ref)))
            print(f"[stream {filt}{freq} R{R} blocks={len(cuts) - 1}] |stream-onepass|={d1:.2e} |stream-oracle|={d2:.2e}")
            assert d1 <= 1e-6 and d2 <= TOL
    p.close()


@pytest.mark.parametrize("filt,freq,R", [("low_pass", 200, 8), ("high_pass", 300, 4), ("low_pass", 1000, 6), (None, 0, 6)])
def test_fused_block_streaming_per_source_states(G, O, filt, freq, R):
    # rh_rlm_stream_block_v: sources that end at different times, fed block by block; each keeps its own filter state
    # across the blocks.  The concatenation equals the one-pass mix of the ragged batch.
    import torch

    ns = [50000, 31000, 12345, 50000, 147, 0, 49999, 2, 20480, 40001, 50000]
    gains = np.linspace(0.5, 1.2, len(ns)).astype(np.float32)
    xs = [rnd(2500 + i, 2 * n, 0.1) for i, n in enumerate(ns)]
    ref = _oracle_pipeline_gains(O, xs, gains, 44100, 48000, None, filt, freq)
    p = G.ResampleLowpassMix(44100, 48000, 2, None, filt, freq, 0.5, max_sources=len(ns), max_in_frames=max(ns), frames_per_lane=R)
    p.set_gains(gains)
    xd = [torch.from_numpy(x).cuda() if len(x) else torch.empty(0, device="cuda") for x in xs]
    p.set_sources(xd)
    one = p.run().cpu().numpy().copy()
    p.check_status()
    assert p.geometry()["general_kernel"] == 1
    rng = np.random.default_rng(99 + R)
    for trial in range(3):
        cuts = [0] + sorted(set(int(c) for c in rng.integers(1, max(ns), size=[1, 5, 20][trial]))) + [max(ns)]
        p.stream_begin()
        outs = []
        for k in range(len(cuts) - 1):
            lo, hi = cuts[k], cuts[k + 1]
            outs.append(p.stream_feed_v([x[2 * min(lo, n): 2 * min(hi, n)] for x, n in zip(xd, ns)], [n <= hi for n in ns]))
        p.check_status()
        got = torch.cat(outs).cpu().numpy()
        assert len(got) == len(ref), (trial, len(got), len(ref))
        if filt is None:
            assert np.array_equal(got, ref)
        else:
            d1, d2 = float(np.max(np.abs(got - one))), float(np.max(np.abs(got - ref)))
            print(f"[stream_v {filt}{freq} R{R} blocks={len(cuts) - 1}] |stream-onepass|={d1:.2e} |stream-oracle|={d2:.2e}")
            assert d1 <= 1e-6 and d2 <= TOL
    p.close()


@pytest.mark.parametrize("filt,freq", [(None, 0), ("low_pass", 200)])
@pytest.mark.parametrize("span", [32768, 2000])
def test_fused_block_streaming_of_spanned_sources(G, O, filt, freq, span):
    # rh_rlm_stream_begin with cfg.span_len: sources that report spans (a SamplesBuffer: any span_len >= 32768; a decoder's
    # packets), fed block by block: the converter restarts every min(span, 32768) samples at the same frames of every source
    # (uniform.rs:56-67), each span's last frame verbatim, while every source's filter state runs on across the seams
    import torch

    ns = [50000, 31000, 16384, 16385, 147, 0, 49999, 2, 32768, 40001]
    gains = np.linspace(0.5, 1.2, len(ns)).astype(np.float32)
    xs = [rnd(2550 + i, 2 * n, 0.1) for i, n in enumerate(ns)]
    ref = _oracle_pipeline_gains(O, xs, gains, 44100, 48000, span, filt, freq)
    p = G.ResampleLowpassMix(44100, 48000, 2, span, filt, freq, 0.5, max_sources=len(ns), max_in_frames=max(ns), frames_per_lane=8)
    p.set_gains(gains)
    xd = [torch.from_numpy(x).cuda() if len(x) else torch.empty(0, device="cuda") for x in xs]
    rng = np.random.default_rng(7 + span)
    for trial in range(3):
        cuts = [0] + sorted(set(int(c) for c in rng.integers(1, max(ns), size=[1, 6, 25][trial]))) + [max(ns)]
        p.stream_begin()
        outs = []
        for k in range(len(cuts) - 1):
            lo, hi = cuts[k], cuts[k + 1]
            outs.append(p.stream_feed_v([x[2 * min(lo, n): 2 * min(hi, n)] for x, n in zip(xd, ns)], [n <= hi for n in ns]))
        p.check_status()
        got = torch.cat(outs).cpu().numpy()
        assert len(got) == len(ref), (trial, len(got), len(ref))
        if filt is None:
            assert np.array_equal(got, ref), int(np.argmax(got != ref))
        else:
            assert float(np.max(np.abs(got - ref))) <= TOL
    # the summed-state entry (equal-length sources) takes the same spans
    n = 40000
    xs = [rnd(2580 + i, 2 * n, 0.1) for i in range(4)]
    ref = _oracle_pipeline_gains(O, xs, np.ones(4, dtype=np.float32), 44100, 48000, span, filt, freq)
    p2 = G.ResampleLowpassMix(44100, 48000, 2, span, filt, freq, 0.5, max_sources=4, max_in_frames=n, frames_per_lane=8)
    xd = [torch.from_numpy(x).cuda() for x in xs]
    cuts = [0, 999, 16384, 16385, 30000, n]
    p2.stream_begin()
    outs = [p2.stream_feed([x[2 * cuts[k]: 2 * cuts[k + 1]] for x in xd], flush=(k == len(cuts) - 2)) for k in range(len(cuts) - 1)]
    p2.check_status()
    got = torch.cat(outs).cpu().numpy()
    assert len(got) == len(ref)
    assert np.array_equal(got, ref) if filt is None else float(np.max(np.abs(got - ref))) <= TOL
    p.close()
    p2.close()


# ------------------------------------------------- per-source gains folded into the fused kernel ----
def _oracle_pipeline_gains(O, xs, gains, frm, to, span, filt, freq):
    """mixer.add(UniformSourceIterator(src.amplify(g)).low_pass(f)) -- rodio's per-source volume."""
    m = O.Mixer(2, to)
    for x, g in zip(xs, gains):
        src = O.TestSource(x, 2, frm) if not span else O.SpanSource(x, 2, frm, span)
        u = O.UniformSourceIterator(src.amplify(float(g)), 2, to)
        if filt == "low_pass":
            u = u.low_pass(freq)
        elif filt == "high_pass":
            u = u.high_pass(freq)
        m.add(u)
    return m.collect()


@pytest.mark.parametrize("general", [0, 1])
@pytest.mark.parametrize("span", [None, 32768])
def test_fused_gains_unfiltered_bit_exact(G, O, general, span):
    # without a filter the gain is applied to the taps before the lerp: amplify.rs:64 then math.rs:25, bit for bit
    import torch

    ns = [30000] * 7 if not general else [30000, 29999, 147, 0, 12345, 30000, 1]
    xs = [rnd(2100 + i, 2 * n) for i, n in enumerate(ns)]
    gains = np.array([1.0, 0.5, 0.3, 1.7, 0.0, -0.25, 0.999], dtype=np.float32)
    ref = _oracle_pipeline_gains(O, xs, gains, 44100, 48000, span, None, 0)
    p = G.ResampleLowpassMix(44100, 48000, 2, span, None, 0, 0.5, max_sources=len(xs), max_in_frames=30000, frames_per_lane=6, force_general=general)
    ts = [torch.from_numpy(x).cuda() if len(x) else torch.empty(0, device="cuda") for x in xs]
    p.set_gains(gains)
    p.set_sources(ts)
    out = p.run().cpu().numpy().copy()
    p.check_status()
    assert np.array_equal(out, ref)
    # changing the gains after set_sources refreshes the descriptors; fewer gains than sources: the rest are 1.0
    p.set_gains(gains[:2])
    out2 = p.run().cpu().numpy().copy()
    ref2 = _oracle_pipeline_gains(O, xs, [1.0, 0.5] + [1.0] * (len(xs) - 2), 44100, 48000, span, None, 0)
    assert np.array_equal(out2, ref2)
    p.close()


@pytest.mark.parametrize("R,general", [(8, 0), (18, 0), (5, 0), (8, 1), (6, 1)])
@pytest.mark.parametrize("filt,freq", [("low_pass", 200), ("high_pass", 300)])
def test_fused_gains_filtered(G, O, R, general, filt, freq):
    import torch
    from scipy.signal import lfilter

    S = 9
    ns = [40000] * S if not general else [40000, 39999, 20000, 148, 0, 40000, 3, 31000, 40000]
    xs = [rnd(2200 + i, 2 * n, 0.12) for i, n in enumerate(ns)]  # mix peak ~0.5: the f32 reference itself stays inside the tolerance
    gains = np.linspace(0.1, 1.3, S).astype(np.float32)
    gains[3] = 0.0
    ref = _oracle_pipeline_gains(O, xs, gains, 44100, 48000, None, filt, freq)
    co = O.blt_coeffs(filt, freq, 0.5, 48000).astype(np.float64)
    truth = np.zeros(len(ref) // 2 * 2).reshape(-1, 2)
    for x, g in zip(xs, gains):
        r = O.UniformSourceIterator(O.TestSource(x, 2, 44100).amplify(float(g)), 2, 48000).collect().astype(np.float64).reshape(-1, 2)
        if len(r):
            truth[: len(r)] += lfilter(co[:3], [1.0, co[3], co[4]], r, axis=0)
    p = G.ResampleLowpassMix(44100, 48000, 2, None, filt, freq, 0.5, max_sources=S, max_in_frames=40000, frames_per_lane=R, force_general=general)
    p.set_gains(gains)
    p.set_sources([torch.from_numpy(x).cuda() if len(x) else torch.empty(0, device="cuda") for x in xs])
    out = p.run().cpu().numpy().copy()
    p.check_status()
    _check_filtered(f"gains {filt}{freq} R{R} g{general}", out, ref, truth.reshape(-1))
    # batch rows carry the gain too (batch mode is for equal-length sources)
    rows = p.run_batch().cpu().numpy() if not general else []
    for s in (1, 3, 8) if not general else ():
        r1 = _oracle_pipeline_gains(O, [xs[s]], [gains[s]], 44100, 48000, None, filt, freq)
        assert float(np.max(np.abs(rows[s][: len(r1)] - r1), initial=0.0)) <= TOL
    p.close()


def test_fused_ragged_filtered_batches_take_the_kernel_pair(G, O):
    # one-shot filtered batches of different lengths: k_rlm_fast<RAG> (stable pairs) + k_rlm_resid (sources about to end);
    # batches whose sources all end together within a tile stay with k_rlm_wave; both agree with the oracle
    import torch

    n = 60000
    cases = {"one short": ([n] * 9 + [n // 2], 1), "spread": ([n - 1500 * i for i in range(12)], 1), "all end within a tile": ([n - i for i in range(40)], 0),
             "longest differ in frames only": ([n] * 3 + [n - 1] * 30, 0)}
    for tag, (ns, want_pair) in cases.items():
        xs = [rnd(2900 + i, 2 * m, 0.05) for i, m in enumerate(ns)]
        ref = _oracle_pipeline(O, xs, 44100, 48000, None, "low_pass", 300)
        truth = _truth_pipeline(O, xs, 44100, 48000, None, "low_pass", 300)
        out, geo = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 300)
        assert geo["general_kernel"] == 1 and geo["ragged_pair"] == want_pair, (tag, geo)
        _check_filtered("ragged pair " + tag, out, ref, truth)
        out2, geo2 = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 300, force_general=1)
        assert geo2["ragged_pair"] == 0
        assert float(np.max(np.abs(out - out2))) <= 1e-6


def test_fused_ragged_pairs_inside_the_first_kernel_equal_the_second_launch(G, O):
    # the pairs in which a source is about to end run inside k_rlm_fast<RAG> (Params::rag_merge), on the mix in registers;
    # RH_RAG_TWO_KERNELS=1 keeps them in a launch of their own (k_rlm_resid) on top of the stored tiles: the same operations in the
    # same order, so the same bits.  RH_RAG_RESIDENT limits the tiles a CU holds at once (later tiles fill in): same bits again.
    from conftest import knobs

    n = 90000
    ns = [n] * 5 + [n - 700 * i - 13 for i in range(1, 60)] + [n // 2, n // 3, 7000]
    xs = [rnd(5100 + i, 2 * m, 0.03) for i, m in enumerate(ns)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, "low_pass", 250)
    truth = _truth_pipeline(O, xs, 44100, 48000, None, "low_pass", 250)
    out, geo = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 250)
    assert geo["ragged_pair"] == 1, geo
    _check_filtered("ragged, pairs merged", out, ref, truth)
    with knobs(RH_RAG_TWO_KERNELS="1"):
        out2, geo2 = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 250)
    assert geo2["ragged_pair"] == 1
    assert np.array_equal(out, out2)
    with knobs(RH_RAG_RESIDENT="2"):
        out3, _ = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 250)
    assert np.array_equal(out, out3)


@pytest.mark.parametrize("general", [0, 1])
def test_fused_same_rate_is_the_ordered_mix(G, O, general):
    # from_rate == to_rate: the converter passes through (sample_rate.rs:133-136); without a filter the fused kernel is the
    # ordered mixer sum of the amplified sources, bit for bit; with one, the filtered mix
    import torch

    ns = [20000] * 5 if not general else [20000, 19999, 5, 0, 12000]
    xs = [rnd(2800 + i, 2 * n) for i, n in enumerate(ns)]
    gains = np.array([1.0, 0.9, 0.6, 1.3, 0.25], dtype=np.float32)
    for filt, freq in ((None, 0), ("high_pass", 300)):
        m = O.Mixer(2, 48000)
        for x, g in zip(xs, gains):
            a = O.TestSource(x, 2, 48000).amplify(float(g))
            m.add(a.high_pass(freq) if filt else a)
        ref = m.collect()
        p = G.ResampleLowpassMix(48000, 48000, 2, None, filt, freq, 0.5, max_sources=len(xs), max_in_frames=20000, frames_per_lane=6, force_general=general)
        p.set_gains(gains)
        p.set_sources([torch.from_numpy(x).cuda() if len(x) else torch.empty(0, device="cuda") for x in xs])
        out = p.run().cpu().numpy().copy()
        p.check_status()
        assert len(out) == len(ref)
        if filt is None:
            assert np.array_equal(out, ref)
        else:
            assert float(np.max(np.abs(out - ref))) <= 5e-5  # full-scale sources: the f32 reference recurrence itself is ~1e-5 from exact
        p.close()


@pytest.mark.parametrize("S", [1, 2, 3])
def test_fused_block_streaming_per_source_states_few_sources(G, O, S):
    # one source per stream is what a GpuMixer rate group often holds; full-size blocks against a small max_sources
    import torch

    n = 30000
    xs = [rnd(2700 + s, 2 * n, 0.1) for s in range(S)]
    ref = _oracle_pipeline(O, xs, 44100, 48000, None, "low_pass", 300)
    p = G.ResampleLowpassMix(44100, 48000, 2, None, "low_pass", 300, 0.5, max_sources=S, max_in_frames=8192 + 4096, frames_per_lane=4)
    xd = [torch.from_numpy(x).cuda() for x in xs]
    p.stream_begin()
    outs = []
    cuts = list(range(0, n, 8192)) + [n]
    for a, b in zip(cuts[:-1], cuts[1:]):
        outs.append(p.stream_feed_v([x[2 * a: 2 * b] for x in xd], [b >= n] * S))
        p.check_status()
    got = torch.cat(outs).cpu().numpy()
    assert len(got) == len(ref) and float(np.max(np.abs(got - ref))) <= TOL
    p.close()


def test_fused_gains_block_streaming(G, O):
    import torch

    S, n = 5, 30000
    xs = [rnd(2300 + s, 2 * n, 0.3) for s in range(S)]
    gains = np.array([0.9, 0.1, 1.5, 0.5, 0.7], dtype=np.float32)
    for filt, freq in ((None, 0), ("low_pass", 200)):
        ref = _oracle_pipeline_gains(O, xs, gains, 44100, 48000, None, filt, freq)
        p = G.ResampleLowpassMix(44100, 48000, 2, None, filt, freq, 0.5, max_sources=S, max_in_frames=n, frames_per_lane=8)
        p.set_gains(gains)
        xd = [torch.from_numpy(x).cuda() for x in xs]
        cuts = [0, 1000, 1001, 9000, 22222, n]
        p.stream_begin()
        outs = [p.stream_feed([x[2 * cuts[k]: 2 * cuts[k + 1]] for x in xd], flush=(k == len(cuts) - 2)) for k in range(len(cuts) - 1)]
        p.check_status()
        got = torch.cat(outs).cpu().numpy()
        assert len(got) == len(ref)
        if filt is None:
            assert np.array_equal(got, ref)
        else:
            assert float(np.max(np.abs(got - ref))) <= TOL
        p.close()


def _bench_long(M, src, reverb_via=None):
    """benches/pipeline.rs:16-37 (`long`), spelled with the adapter methods both mirrors share."""
    x = (src.high_pass(300).amplify(1.2).speed(0.9).automatic_gain_control()
         .delay(500_000_000).fade_in(2_000_000_000).take_duration(10_000_000_000, fade_out=True))
    x = x.reverb(50_000_000, 0.3)  # .buffered() only makes the clone possible; .skippable() passes through
    return M.UniformSourceIterator(x, 2, 40000)


def test_reference_bench_chains(G, O):
    # BASELINE config 1, as the reference really spells it: benches/pipeline.rs `short`
    # (amplify(1.2).low_pass(200)) and `long` (9 adapters -> reverb -> UniformSourceIterator to 40 kHz) on
    # the committed excerpt of assets/music.wav continued by 3 s of noise (44.1 kHz stereo)
    import os

    gdir = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
    x = np.concatenate([np.load(os.path.join(gdir, "music_excerpt_f32.npy")), rnd(77, 2 * 132300, 0.3)])
    ref = O.TestSource(x, 2, 44100).amplify(1.2).low_pass(200).collect()
    assert np.array_equal(G.TestSource(x, 2, 44100).amplify(1.2).low_pass(200).collect(), ref)  # `short`, sequential biquad: bit-exact
    par = G.TestSource(x, 2, 44100).amplify(1.2).low_pass(200, mode=1).collect()                # the time-parallel filter
    assert float(np.max(np.abs(par - ref))) <= TOL
    ref = _bench_long(O, O.TestSource(x, 2, 44100)).collect()
    got = _bench_long(G, G.TestSource(x, 2, 44100)).collect()
    assert len(got) == len(ref) and len(ref) > 2 * 40000
    err = float(np.max(np.abs(got - ref)))
    print(f"[bench long] samples={len(ref)} max_abs_err={err:.3e} peak={float(np.max(np.abs(ref))):.3e}")
    assert err <= TOL  # AGC uses sqrt/division chains: device libm rounding, everything else is exact


def test_fused_subset_and_argument_errors(G, O):
    import ctypes as C

    import torch

    from rodio_amd import _lib

    S, n = 6, 30000
    xs = [rnd(1500 + s, 2 * n, 0.2) for s in range(S)]
    p = G.ResampleLowpassMix(44100, 48000, 2, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=n)
    xd = [torch.from_numpy(x).cuda() for x in xs]
    p.set_sources(xd)
    sub = p.run_subset(2, 3).cpu().numpy()
    p.check_status()
    ref = _oracle_pipeline(O, xs[2:5], 44100, 48000, None, "low_pass", 200)
    assert len(sub) == len(ref) and float(np.max(np.abs(sub - ref))) <= TOL
    with pytest.raises(G.RhError):
        p.run_subset(4, 3)  # past the end
    small = torch.empty(16, device="cuda")
    with pytest.raises(G.RhError):
        p.run(small)  # RH_ERR_CAPACITY
    with pytest.raises(G.RhError):
        p.set_sources(xd + xd)  # more than max_sources
    with pytest.raises(G.RhError):
        p.set_sources([xd[0][1:]])  # not 16-byte aligned
    p.close()
    for bad in [dict(channels=3), dict(from_rate=96000 * 3, to_rate=44100), dict(filter="low_pass", freq=30000)]:
        kw = dict(from_rate=44100, to_rate=48000, channels=2, span_len=None, filter="low_pass", freq=200)
        kw.update(bad)
        with pytest.raises(G.RhError):
            G.ResampleLowpassMix(kw["from_rate"], kw["to_rate"], kw["channels"], kw["span_len"], kw["filter"], kw["freq"], 0.5)
    # streaming needs begin(); a finished stream refuses more blocks
    q = G.ResampleLowpassMix(44100, 48000, 2, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=n)
    with pytest.raises(G.RhError):
        q._left = None
        q.stream_feed([x[:2000] for x in xd])
    q.stream_begin()
    q.stream_feed([x[:2000] for x in xd], flush=True)
    with pytest.raises(G.RhError):
        q.stream_feed([x[:2000] for x in xd])
    q.close()


def test_fused_matches_unfused_gpu_ops(G, O):
    # fused kernel vs the standalone ops (resample -> sequential biquad -> ordered mix), 64 sources
    S, n = 64, 50000
    xs = [rnd(1000 + s, 2 * n, 1.0 / S) for s in range(S)]
    m = G.Mixer(2, 48000)
    for x in xs:
        m.add(G.UniformSourceIterator(G.TestSource(x, 2, 44100), 2, 48000).low_pass(200))
    unfused = m.collect()
    out, _ = _gpu_pipeline(G, xs, 44100, 48000, None, "low_pass", 200)
    err, _ = _report("fused vs unfused", out, unfused)
    assert err <= TOL


# ------------------------------------------- BASELINE config 2 at full size: properties ----
@pytest.fixture(scope="module")
def cfg2(G):
    import torch

    S, N = 256, 1 << 20
    g = torch.Generator(device="cuda")
    g.manual_seed(1234)
    data = (torch.rand((S, N * 2), generator=g, device="cuda", dtype=torch.float32) * 2 - 1) * (1.0 / S)
    return S, N, data


def test_cfg2_full_size_head_and_tail_vs_oracle(G, O, cfg2):
    """Full-size run (256 x 1 Mi stereo frames, 44.1->48 k, low_pass(200), mix).  The system is
    causal and the filter's memory is ~2k frames, so the oracle can check (a) the head from a
    prefix of every source and (b) the tail from a suffix that starts on a resampler period
    (input frame multiple of F=147 <-> output frame multiple of T=160) with a long warm-up."""
    import torch

    S, N, data = cfg2
    p = G.ResampleLowpassMix(44100, 48000, 2, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=N)
    p.set_sources([data[s] for s in range(S)])
    out = p.run()
    p.check_status()
    M = p.out_frames
    assert M == 1141308  # ceil((N-1)*160/147)+1
    full = out.cpu().numpy()
    # (a) head
    n_head = 6000
    head = data[:, : n_head * 2].cpu().numpy()
    ref = _oracle_pipeline(O, [head[s] for s in range(S)], 44100, 48000, None, "low_pass", 200)
    k = (len(ref) // 2 - 8) * 2  # the last oracle frames see the prefix's end-of-stream rule
    err, peak = _report("cfg2 head", full[:k], ref[:k])
    assert err <= TOL and err <= 2e-5 * peak + 1e-7
    # (b) tail
    i0 = ((N - 30000) // 147) * 147
    m0 = i0 // 147 * 160
    tail = data[:, i0 * 2:].cpu().numpy()
    ref = _oracle_pipeline(O, [tail[s] for s in range(S)], 44100, 48000, None, "low_pass", 200)
    assert m0 + len(ref) // 2 == M
    keep = 8000 * 2  # compare the last 8000 frames (warm-up of ~24000 frames before them)
    err, peak = _report("cfg2 tail", full[-keep:], ref[-keep:])
    assert err <= TOL and err <= 2e-5 * peak + 1e-7
    p.close()


def test_cfg2_full_size_linearity_is_bit_exact(G, cfg2):
    """Size-independent property: every stage is linear, and scaling by a power of two is exact in
    f32, so pipeline(2x) == 2 * pipeline(x) bit for bit (any lost carry, mis-indexed tap or
    race in the tile hand-off breaks this)."""
    import torch

    S, N, data = cfg2
    p = G.ResampleLowpassMix(44100, 48000, 2, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=N)
    p.set_sources([data[s] for s in range(S)])
    a = p.run().clone()
    b = p.run().clone()  # same input twice: the hand-off protocol must be deterministic
    p.check_status()
    assert torch.equal(a, b)
    data.mul_(2.0)
    c = p.run().clone()
    p.check_status()
    data.mul_(0.5)
    assert torch.equal(c, a * 2.0)
    assert float(a.abs().max()) > 0
    p.close()


def test_cfg2_autotune_keeps_the_result(G, cfg2):
    """rh_rlm_autotune swaps the launch geometry (tile length, ring depth, tables): the mixed block must
    stay within f32 re-association distance of the model geometry's, and repeat bit for bit."""
    import torch

    S, N, data = cfg2
    p = G.ResampleLowpassMix(44100, 48000, 2, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=N)
    p.set_sources([data[s] for s in range(S)])
    a = p.run().clone()
    g0 = p.geometry()
    r, ns = p.autotune()
    g1 = p.geometry()
    assert (g1["frames_per_lane"], g1["ring_stages"]) == (r, ns) and not g1["general_kernel"]
    b = p.run().clone()
    c = p.run().clone()
    p.check_status()
    assert torch.equal(b, c)
    err = float((a - b).abs().max())
    print(f"[autotune] {g0['frames_per_lane']},{g0['ring_stages']} -> {r},{ns}  |delta|={err:.2e} peak={float(a.abs().max()):.2e}")
    assert err <= 1e-6
    p.close()


def test_cfg2_chunked_variant_matches_unchunked_away_from_seams(G, cfg2):
    """span_len=32768 variant: 64 chunks x 17833 frames; inside a chunk the output
    equals the continuous stream's (same taps), only the seam frames differ."""
    S, N, data = cfg2
    pc = G.ResampleLowpassMix(44100, 48000, 2, 32768, None, 0, 0.5, max_sources=S, max_in_frames=N)
    pc.set_sources([data[s] for s in range(S)])
    oc = pc.run().cpu().numpy()
    pc.check_status()
    assert pc.out_frames == 64 * 17833
    pu = G.ResampleLowpassMix(44100, 48000, 2, None, None, 0, 0.5, max_sources=S, max_in_frames=N)
    pu.set_sources([data[s] for s in range(S)])
    ou = pu.run().cpu().numpy()
    # chunk 0 covers output frames [0, 17833): all but its last frame coincide with the continuous stream
    assert np.array_equal(oc[: 17832 * 2], ou[: 17832 * 2])
    pc.close()
    pu.close()


def test_native_comm_single_rank(G):
    # rh_comm_*: the RCCL entry points of the C ABI.  One GPU here, so one rank: the all-reduce and the reduce
    # are the identity, but id exchange, communicator set-up, the in-place collective on the caller's
    # stream and tear-down all run for real.
    import torch

    from rodio_amd.distributed import NativeComm

    uid = NativeComm.unique_id()
    assert len(uid) == 128 and any(uid)
    comm = NativeComm(0, 1, uid)
    x = torch.rand(1141308 * 2, device="cuda")
    y = x.clone()
    comm.all_reduce(y)
    comm.reduce(y, root=0)
    torch.cuda.synchronize()
    assert torch.equal(x, y)
    with pytest.raises(G.RhError):
        comm.reduce(y, root=1)
    comm.close()
