"""The numpy references of tests/test_gpu_fallbacks.py (tests/fallback_cases.py) against the oracle, at the shapes the GPU file uses: a wrong
reference is caught without a GPU.  Bit for bit (every one of these operations is exact by contract)."""
import numpy as np
import pytest

import fallback_cases as FC
from fallback_cases import bits, f32


def same(a, b):
    return a.shape == b.shape and np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("frm,to,ch", FC.LANE_RATES)
def test_resample_reference_at_the_lane_kernels_shapes(O, frm, to, ch):
    for n in FC.lane_lengths(frm, to):
        x = FC.signal(n + ch, n * ch)
        ref = FC.ref_resample(x, frm, to, ch)
        assert len(ref) == FC.out_frames(n, frm, to, ch) * ch
        assert same(ref, FC.oracle_resample(O, x, frm, to, ch)), (frm, to, ch, n)
        # what the gate does with the row: fewer than 16 frames a tile
        assert FC.resample_tile_frames(len(ref) // ch, frm, to, ch) < 16, (frm, to, ch, n)
    for span in FC.lane_spans(ch):
        c = FC.chunk_frames(10 ** 9, ch, span)
        n = min(1500, 3 * c) + 1 if c < 1500 else c + 1   # a last chunk of one frame
        x = FC.signal(span + ch, n * ch)
        ref = FC.ref_resample(x, frm, to, ch, span)
        assert len(ref) == FC.out_frames(n, frm, to, ch, span) * ch
        assert same(ref, FC.oracle_resample(O, x, frm, to, ch, span)), (frm, to, ch, span)
        assert FC.resample_tile_frames(len(ref) // ch, frm, to, ch) < 16, (frm, to, ch, span)


def test_resample_inputs_tell_a_fused_lerp_from_the_reference():
    """a + (b - a) * num / T with the division and the addition rounded ONCE (what a contraction of the last two operations gives) differs from
    the three-rounding reference somewhere in every input the GPU test uses: the comparison can see a fused lerp."""
    frm, to, ch = 44100, 48000, 96
    n = FC.lane_lengths(frm, to)[-1]
    x = FC.signal(n + ch, n * ch)
    ref = FC.ref_resample(x, frm, to, ch).reshape(-1, ch)
    F, T = FC.reduced(frm, to)
    X = x.reshape(-1, ch)
    m = np.arange(len(ref) - 1)
    i, num = m * F // T, (m * F % T).astype(f32)
    p = (X[i + 1] - X[i]) * num[:, None]
    fused = (X[i].astype(np.float64) + p.astype(np.float64) / T).astype(f32)
    assert np.count_nonzero(bits(fused) != bits(ref[:-1])) > 100
    assert np.any(bits(x) == 0x80000000) and np.any(x == 1.0) and np.any(x == -1.0)


@pytest.mark.parametrize("frm,to,ch,span", list(dict.fromkeys(FC.ORDINARY_RATES + FC.KB_ROWS)))
def test_resample_reference_at_the_ordinary_shapes(O, frm, to, ch, span):
    for n in FC.ORDINARY_FRAMES:
        if span and n * ch < span:
            continue
        x = FC.signal(n, n * ch)
        assert same(FC.ref_resample(x, frm, to, ch, span), FC.oracle_resample(O, x, frm, to, ch, span)), n


@pytest.mark.parametrize("frm,to,ch,n,span", FC.WIDE_POS)
def test_resample_reference_beyond_32_bit_positions(O, frm, to, ch, n, span):
    F, T = FC.reduced(frm, to)
    assert (F, T) == (frm, to) and F * T < 2 ** 32 and not FC.fits32(n, frm, to, ch, span)
    assert FC.resample_tile_frames(FC.out_frames(n, frm, to, ch, span), frm, to, ch) >= 16   # unpinned: the tile kernel
    x = FC.signal(n, n * ch)
    assert same(FC.ref_resample(x, frm, to, ch, span), FC.oracle_resample(O, x, frm, to, ch, span))


def test_tile_kb_rows_and_the_gate():
    """RH_PCM_TILE_KB=1: stereo and 5.1 at 44.1 -> 48 kHz keep the tile kernel (64 and 20 frames a tile), the 12-channel row does not (8)."""
    tf = [FC.resample_tile_frames(FC.out_frames(FC.KB_FRAMES, frm, to, ch, span), frm, to, ch, 1) for frm, to, ch, span in FC.KB_ROWS]
    assert tf == [64, 20, 64, 8]
    for kb in (2, 5, 48, 0, 49):
        assert all(FC.resample_tile_frames(FC.out_frames(FC.KB_FRAMES, frm, to, ch, span), frm, to, ch, kb) >= 16 for frm, to, ch, span in FC.KB_ROWS)


@pytest.mark.parametrize("n_sources,out_len,aligned", [(20, 4099, True), (3, 4099, True), (8, 4099, True), (15, 4099, True), (20, 4099, False),
                                                       (129, 2999, True), (257, 2999, True), (129, 2999, False), (257, 2999, False)])
def test_mix_reference(O, n_sources, out_len, aligned):
    srcs, starts = FC.mix_layout(n_sources, n_sources, out_len, aligned)
    assert all(s % 4 == 0 for s in starts) == aligned
    if n_sources >= 8:
        assert any(len(x) == 0 for x in srcs) and any(s >= out_len for s in starts) and any(s < out_len < s + len(x) for x, s in zip(srcs, starts))
        assert any((s + len(x)) % 4 for x, s in zip(srcs, starts) if s + len(x) < out_len)   # ends inside a vector
    ref = FC.ref_mix(srcs, starts, out_len)
    assert same(ref, FC.oracle_mix(O, srcs, starts, out_len))
    assert not np.any(bits(ref) == 0x80000000)


@pytest.mark.parametrize("frm_ch,to_ch", FC.WIDE_CHANNELS + [FC.WIDE_CHANNELS_CONTROL] + FC.ORDINARY_LAYOUTS)
def test_channels_reference(O, frm_ch, to_ch):
    wide = frm_ch + to_ch > 16
    for frames in (FC.WIDE_FRAMES if wide else FC.ORDINARY_LAYOUT_FRAMES):
        x = FC.signal(frames + frm_ch, frames * frm_ch)
        assert same(FC.ref_channels(x, frm_ch, to_ch), FC.oracle_channels(O, x, frm_ch, to_ch))
    if wide:
        assert (FC.pcm_tile_frames(4 * frm_ch, 4 * to_ch) < 8) == ((frm_ch, to_ch) != FC.WIDE_CHANNELS_CONTROL)


@pytest.mark.parametrize("in_ch,out_ch", FC.WIDE_VOLUME + FC.ORDINARY_LAYOUTS)
def test_channel_volume_reference(O, in_ch, out_ch):
    wide = in_ch > 16
    gains = np.linspace(0.2, 1.1, out_ch).astype(f32)
    for frames in (FC.WIDE_FRAMES if wide else FC.ORDINARY_LAYOUT_FRAMES):
        x = FC.signal(frames + in_ch, frames * in_ch)
        assert same(FC.ref_channel_volume(x, in_ch, gains), FC.oracle_channel_volume(O, x, in_ch, gains))
    if wide:
        assert FC.pcm_tile_frames(4 * in_ch, 4 * out_ch) < 8
    assert FC.pcm_tile_frames(4 * 304, 4 * 16) >= 8   # in + out = 320: still the tile kernel


def test_int_to_f32_reference(O):
    for fmt, (dt, _, _) in FC.INT_FORMATS.items():
        info = np.iinfo(dt)
        v = np.arange(info.min, info.max + 1, dtype=np.int64).astype(dt)
        assert same(FC.ref_int_to_f32(v, fmt), O.convert(fmt + "_to_f32", v)), fmt


@pytest.mark.parametrize("fmt,frm_ch,to_ch", FC.WIDE_PCM + [(fmt, a, b) for fmt in FC.PCM for a, b in FC.ORDINARY_LAYOUTS])
def test_pcm_decode_reference(O, fmt, frm_ch, to_ch):
    wide = frm_ch > 16
    for frames in (FC.WIDE_FRAMES if wide else FC.ORDINARY_LAYOUT_FRAMES) + ((FC.KB_FRAMES,) if (fmt, frm_ch, to_ch) in FC.KB_PCM else ()):
        n = FC.cut(frames, frm_ch)   # the data chunk ends inside the last frame
        raw = FC.pcm_bytes(frames, fmt, n)
        assert same(FC.ref_pcm_decode(raw, fmt, n, frm_ch, to_ch), FC.oracle_pcm_decode(O, raw, fmt, n, frm_ch, to_ch))
    if wide:
        assert FC.pcm_tile_frames(FC.PCM[fmt][0] * frm_ch, 4 * to_ch) < 8


def test_pcm_decode_reference_keeps_the_layout(O):
    ch = FC.WIDE_PCM24_CHANNELS
    assert FC.pcm_tile_frames(3 * ch, 4 * ch) < 8 <= FC.pcm_tile_frames(3 * (ch - 1), 4 * (ch - 1))
    for fmt, channels in [("i24", ch)] + FC.DECODE_LAYOUTS:
        for frames in (FC.WIDE_FRAMES if channels == ch else FC.ORDINARY_LAYOUT_FRAMES):
            for n in (FC.wide_pcm24_samples(frames) if channels == ch else (FC.cut(frames, channels), frames * channels)):
                raw = FC.pcm_bytes(frames, fmt, n)
                ref = FC.ref_pcm_decode(raw, fmt, n, channels)
                assert len(ref) == frames * channels and same(ref, FC.oracle_pcm_decode(O, raw, fmt, n, channels))


@pytest.mark.parametrize("ch,rate,to_rate", FC.WIDE_UNIFORM)
def test_wide_uniform_reference(O, ch, rate, to_rate):
    srcs = FC.wide_uniform_sources(ch, rate, to_rate)
    ref = FC.ref_wide_uniform(srcs, ch, rate, to_rate, FC.WIDE_UNIFORM_FRAMES)
    assert same(ref, FC.oracle_wide_uniform(O, srcs, ch, rate, to_rate, FC.WIDE_UNIFORM_FRAMES))
