"""The kernels BEHIND the one-row entries' host gates: every stand-alone entry chooses on the host between a vector / tile kernel
and an older lane-per-element one, and since round 6 the ordinary shapes -- and with them the rest of the suite -- take the first.  Here: the
shapes the gates decline (frames of hundreds of channels, steep decimations, rows off their vector boundary) with NO knob set, and the ordinary
shapes with the knob that pins the older kernel (RH_PCM_NO_TILE, RH_PCM_TILE_KB, RH_MIX_GROUPS, RH_WIDE_GENERAL).  Through the C ABI, rows inside
larger buffers between guard zones, against references written in numpy (tests/fallback_cases.py; tests/test_fallback_refs_cpu.py holds them
against the oracle) and against the oracle itself for the resampler.  Every comparison is of bits."""
import ctypes as C

import numpy as np
import pytest

import fallback_cases as FC
from fallback_cases import bits, f32

pytestmark = pytest.mark.gpu

GUARD = 7.0


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _src(x, so):
    """x inside a larger device buffer, `so` elements of x's own type behind a 256-byte boundary.  Returns (the buffer, the row's address)."""
    import torch

    raw = np.ascontiguousarray(x).view(np.uint8).reshape(-1)
    sob = so * x.itemsize
    buf = torch.zeros(raw.size + sob + 64, dtype=torch.uint8, device="cuda")
    if raw.size:
        buf[sob: sob + raw.size] = torch.from_numpy(raw).cuda()
    return buf, buf.data_ptr() + sob


def _dst(out_len, do):
    import torch

    buf = torch.full((out_len + 24,), GUARD, dtype=torch.float32, device="cuda")
    return buf, buf.data_ptr() + 4 * (8 + do)


def _take(buf, out_len, do, what=""):
    import torch

    torch.cuda.synchronize()
    h = buf.cpu().numpy()
    assert np.all(h[: 8 + do] == GUARD) and np.all(h[8 + do + out_len:] == GUARD), f"wrote outside its row {what}"
    return h[8 + do: 8 + do + out_len].copy()


def _run(call, x, out_len, so=0, do=0, what=""):
    """call(dst_ptr, src_ptr, stream) on src = buffer + so elements of x's type, dst = buffer + do floats; the out_len outputs, guard zones checked."""
    from rodio_amd import source

    sbuf, sp = _src(x, so)
    dbuf, dp = _dst(out_len, do)
    call(C.c_void_p(dp), C.c_void_p(sp), source._stream())
    return _take(dbuf, out_len, do, what)


def _same(got, want, what):
    assert got.shape == want.shape, what
    assert np.array_equal(bits(got), bits(want)), (what, int(np.count_nonzero(bits(got) != bits(want))), "samples differ")


# ================================================================================================================= resampler ====
def _resample(x, frames, frm, to, ch, span, so=0, do=0):
    from rodio_amd import _lib

    m = C.c_uint64(0)
    _lib.check(_lib.lib.rh_resample_out_frames(frames, frm, to, ch, span, C.byref(m)), "rh_resample_out_frames")
    assert m.value == FC.out_frames(frames, frm, to, ch, span), (frames, frm, to, ch, span)
    return _run(lambda d, s, st: _lib.check(_lib.lib.rh_resample_linear(d, s, frames, frm, to, ch, span, st), "rh_resample_linear"), x, m.value * ch, so, do,
                what=(frames, frm, to, ch, span, so, do))


@pytest.mark.parametrize("frm,to,ch", FC.LANE_RATES)
def test_resampler_rows_the_gate_declines(G, O, frm, to, ch):
    """k_resample_linear<C, true> with no knob set: channels * (1 + F / T) > 128, fewer than 16 frames would fit a tile (192 kHz -> 1 kHz has
    T = 1: every frame lands on a tap).  Lengths of 1 and 2 frames, either side of a multiple of F, a few workgroups; spans of one frame, 40 frames
    and 32768 samples with a last chunk of one frame; stereo 4 bytes off an 8-byte boundary (the general-channel-count instance, not float2)."""
    for n in FC.lane_lengths(frm, to):
        x = FC.signal(n + ch, n * ch)
        want = FC.ref_resample(x, frm, to, ch)
        _same(want, FC.oracle_resample(O, x, frm, to, ch), ("the two references", n))
        _same(_resample(x, n, frm, to, ch, 0), want, n)
        if ch == 2:
            for so, do in ((1, 0), (0, 1), (3, 1)):
                _same(_resample(x, n, frm, to, ch, 0, so, do), want, (n, so, do))
    for span in FC.lane_spans(ch):
        c = FC.chunk_frames(10 ** 9, ch, span)
        n = min(1500, 3 * c) + 1 if c < 1500 else c + 1
        x = FC.signal(span + ch, n * ch)
        want = FC.ref_resample(x, frm, to, ch, span)
        _same(want, FC.oracle_resample(O, x, frm, to, ch, span), ("the two references", span))
        _same(_resample(x, n, frm, to, ch, span, 0, 0), want, span)
        _same(_resample(x, n, frm, to, ch, span, 1, 3), want, (span, "shifted"))


def test_resampler_ordinary_rows_pinned_to_the_lane_kernel(G, O):
    """RH_PCM_NO_TILE=1 sends the rows of test_gpu_rows_alignment.py::test_resampler_rows_anywhere to k_resample_linear<1 | 2 | 0, true>: the bits of
    the unpinned call (k_resample_tile) and of both references."""
    from conftest import knobs

    rows = []
    for frm, to, ch, span in FC.ORDINARY_RATES:
        for n in FC.ORDINARY_FRAMES:
            if span and n * ch < span:
                continue
            x = FC.signal(n, n * ch)
            want = FC.ref_resample(x, frm, to, ch, span)
            _same(want, FC.oracle_resample(O, x, frm, to, ch, span), ("the two references", frm, to, ch, span, n))
            rows.append((x, n, frm, to, ch, span, want))
    for x, n, frm, to, ch, span, want in rows:
        _same(_resample(x, n, frm, to, ch, span), want, ("unpinned", frm, to, ch, span, n))
    with knobs(RH_PCM_NO_TILE="1"):
        for x, n, frm, to, ch, span, want in rows:
            for so, do in ((0, 0), (1, 0), (2, 3)):
                _same(_resample(x, n, frm, to, ch, span, so, do), want, ("pinned", frm, to, ch, span, n, so, do))


@pytest.mark.parametrize("frm,to,ch,n,span", FC.WIDE_POS)
def test_resampler_positions_beyond_32_bits(G, O, frm, to, ch, n, span):
    """fits32 == 0 in under 1 MB: F = 65521, T = 48000, 100 000 input frames -- (out_frames + 1) F > 2^32 (the spanned row: 30000 -> 140003, whose
    chunk of 32768 frames is that long).  Unpinned: k_resample_tile<false, 1 | 2 | 0>; RH_PCM_NO_TILE=1: k_resample_linear<1 | 2 | 0, false>."""
    from conftest import knobs

    assert not FC.fits32(n, frm, to, ch, span)
    x = FC.signal(n, n * ch)
    want = FC.ref_resample(x, frm, to, ch, span)
    _same(want, FC.oracle_resample(O, x, frm, to, ch, span), "the two references")
    _same(_resample(x, n, frm, to, ch, span), want, "unpinned")
    with knobs(RH_PCM_NO_TILE="1"):
        _same(_resample(x, n, frm, to, ch, span), want, "pinned")
        _same(_resample(x, n, frm, to, ch, span, 1, 1), want, "pinned, shifted")


def _decode_channels(raw, fmt, n, frm_ch, to_ch, so=0, do=0):
    from rodio_amd import _lib

    _, bps, is_float = FC.PCM[fmt]
    frames = (n + frm_ch - 1) // frm_ch
    m = C.c_uint64(0)
    out = _run(lambda d, s, st: _lib.check(_lib.lib.rh_wav_decode_channels(d, s, n, frm_ch, bps, is_float, to_ch, C.byref(m), st), "rh_wav_decode_channels"),
               raw, frames * to_ch, so, do, what=(fmt, n, frm_ch, to_ch, so, do))
    assert m.value == frames * to_ch
    return out


@pytest.mark.parametrize("kb", FC.KB_VALUES)
def test_tile_kb_sweep(G, kb):
    """RH_PCM_TILE_KB in {1, 2, 5, 48} sizes the tiles of k_resample_tile and k_pcm_to_channels_tile; 0 and 49 are out of range and behave as unset.
    The bits never change.  At 1 KiB a tile the 12-channel row has 8 frames a tile and drops to k_resample_linear (tf < 16); stereo (64 frames)
    and 5.1 (20) keep the tile kernel at every value."""
    from conftest import knobs

    n = FC.KB_FRAMES
    rows = [(FC.signal(n + ch, n * ch), frm, to, ch, span) for frm, to, ch, span in FC.KB_ROWS]
    pcm = [(FC.pcm_bytes(a, fmt, FC.cut(n, a)), fmt, FC.cut(n, a), a, b) for fmt, a, b in FC.KB_PCM]
    want_r = [FC.ref_resample(x, frm, to, ch, span) for x, frm, to, ch, span in rows]
    want_p = [FC.ref_pcm_decode(*p) for p in pcm]
    for (x, frm, to, ch, span), w in zip(rows, want_r):
        _same(_resample(x, n, frm, to, ch, span), w, ("default", ch, span))
    for p, w in zip(pcm, want_p):
        _same(_decode_channels(*p), w, ("default", p[1]))
    with knobs(RH_PCM_TILE_KB=kb):
        for (x, frm, to, ch, span), w in zip(rows, want_r):
            _same(_resample(x, n, frm, to, ch, span), w, (kb, ch, span))
            _same(_resample(x, n, frm, to, ch, span, 1, 2), w, (kb, ch, span, "shifted"))
        for p, w in zip(pcm, want_p):
            _same(_decode_channels(*p), w, (kb, p[1]))
            _same(_decode_channels(*p, so=1, do=1), w, (kb, p[1], "odd byte address"))


# ===================================================================================================================== mixer ====
def _mix(srcs, starts, out_len, do=0, shifts=None):
    """rh_mix_sum on sources that sit in one device buffer, each `shift` floats behind a 16-byte boundary, into a row between guard zones."""
    import torch

    from rodio_amd import _lib, source

    n = len(srcs)
    shifts = shifts or [0] * n
    offs, pos = [], 0
    for x, sh in zip(srcs, shifts):
        offs.append(pos + sh)
        pos += (len(x) + sh + 3) // 4 * 4 + 4
    host = np.zeros(pos + 4, f32)
    for x, o in zip(srcs, offs):
        host[o: o + len(x)] = x
    dev = torch.from_numpy(host).cuda()
    dbuf, dp = _dst(out_len, do)
    ptrs = (C.c_void_p * n)(*[dev.data_ptr() + 4 * o for o in offs]) if n else None
    st = (C.c_uint64 * n)(*starts) if n else None
    ln = (C.c_uint64 * n)(*[len(x) for x in srcs]) if n else None
    _lib.check(_lib.lib.rh_mix_sum(C.c_void_p(dp), out_len, ptrs, st, ln, n, source._stream()), "rh_mix_sum")
    out = _take(dbuf, out_len, do, what=("rh_mix_sum", n, out_len, do))
    assert not np.any(bits(out) == 0x80000000), "the mix is never -0.0"
    return out


def _mix_case(n_sources, out_len, aligned, do=0, shifted_sources=False):
    srcs, starts = FC.mix_layout(n_sources, n_sources, out_len, aligned)
    shifts = [(3 * s + 1) % 4 for s in range(n_sources)] if shifted_sources else None
    _same(_mix(srcs, starts, out_len, do, shifts), FC.ref_mix(srcs, starts, out_len), ("rh_mix_sum", n_sources, out_len, aligned, do, shifted_sources))


def test_mix_sum_rows_anywhere(G):
    """k_mix_sum_any<CONT>, no knob: starts of every residue mod 4, sources off their vector boundary, a destination 1-3 floats off its own
    (dst_vec == 0); 129 and 257 sources: the launches after the first continue from the stored partial sum.  No source: zeros."""
    for do in (0, 1, 2, 3):
        _mix_case(20, 4099, False, do)
        _mix_case(20, 4099, False, do, shifted_sources=True)
    _mix_case(20, 4099, True, 0, shifted_sources=True)   # starts on vectors, pointers not
    _mix_case(20, 4099, True, 2)                          # ... and only the destination off its boundary
    for n in (129, 257):
        _mix_case(n, 2999, False)
        _mix_case(n, 2999, False, 3, shifted_sources=True)
    for do in (0, 1):
        assert not np.any(bits(_mix([], [], 4099, do)))


def test_mix_sum_grouped_by_the_gate(G):
    """k_mix_sum_v4_grp as the gate picks it (16 or more sources, a grid of fewer than 8 workgroups a CU): late joins on vectors, sources that end
    inside one, an empty one, one behind the mix and one that would run past it."""
    for n in (20, 129, 257):
        _mix_case(n, 4099 if n == 20 else 2999, True)


def test_mix_sum_ungrouped_with_many_sources(G):
    """RH_MIX_GROUPS=1: k_mix_sum_v4<CONT> at 20, 129 and 257 sources (the gate gives it 16 or more only on rows of 2 Mi samples)."""
    from conftest import knobs

    with knobs(RH_MIX_GROUPS="1"):
        for n in (20, 129, 257):
            _mix_case(n, 4099 if n == 20 else 2999, True)


def test_mix_sum_grouped_with_few_sources(G):
    """RH_MIX_GROUPS=8: k_mix_sum_v4_grp at 3 (fewer than a group), 8 (one group) and 15 sources (a group and a tail), and the continuation launches."""
    from conftest import knobs

    with knobs(RH_MIX_GROUPS="8"):
        for n in (3, 8, 15, 20):
            _mix_case(n, 4099, True)
        for n in (129, 257):
            _mix_case(n, 2999, True)


def test_mix_sum_lane_per_sample(G):
    """RH_PCM_NO_TILE=1: k_mix_sum<CONT> on the rows that start anywhere."""
    from conftest import knobs

    with knobs(RH_PCM_NO_TILE="1"):
        for do in (0, 1, 3):
            _mix_case(20, 4099, False, do, shifted_sources=bool(do))
        for n in (129, 257):
            _mix_case(n, 2999, False, n % 4)


# =============================================================================================== frames of hundreds of channels ====
def _channels(x, frames, frm_ch, to_ch, so=0, do=0):
    from rodio_amd import _lib

    return _run(lambda d, s, st: _lib.check(_lib.lib.rh_channels_convert(d, s, frames, frm_ch, to_ch, st), "rh_channels_convert"), x, frames * to_ch, so, do,
                what=("rh_channels_convert", frames, frm_ch, to_ch, so, do))


def _volume(x, frames, in_ch, gains, so=0, do=0):
    from rodio_amd import _lib

    return _run(lambda d, s, st: _lib.check(_lib.lib.rh_channel_volume(d, s, frames, in_ch, gains.ctypes.data_as(_lib.f32p), len(gains), st), "rh_channel_volume"),
                x, frames * len(gains), so, do, what=("rh_channel_volume", frames, in_ch, len(gains), so, do))


def _decode(raw, fmt, n, channels, so=0, do=0):
    from rodio_amd import _lib

    _, bps, is_float = FC.PCM[fmt]
    total = (n + channels - 1) // channels * channels
    m = C.c_uint64(0)
    out = _run(lambda d, s, st: _lib.check(_lib.lib.rh_wav_decode(d, s, n, channels, bps, is_float, C.byref(m), st), "rh_wav_decode"), raw, total, so, do,
               what=("rh_wav_decode", fmt, n, channels, so, do))
    assert m.value == total
    return out


SAMPLE_OFFS = [(0, 0), (1, 0), (0, 1), (3, 2)]


@pytest.mark.parametrize("frm_ch,to_ch", FC.WIDE_CHANNELS + [FC.WIDE_CHANNELS_CONTROL])
def test_channels_convert_wide_frames(G, frm_ch, to_ch):
    """k_channels_convert with no knob set: from + to > 320, the tile kernel would hold fewer than 8 frames (319 -> 2 and 2 -> 319 are the smallest
    sum it declines; 318 -> 2 is the control that still takes it; 1 -> 330: the mono rule -- channel 1 repeats the sample, the rest is +0.0)."""
    for frames in FC.WIDE_FRAMES:
        x = FC.signal(frames + frm_ch, frames * frm_ch)
        want = FC.ref_channels(x, frm_ch, to_ch)
        for so, do in SAMPLE_OFFS:
            _same(_channels(x, frames, frm_ch, to_ch, so, do), want, (frames, so, do))


@pytest.mark.parametrize("in_ch,out_ch", FC.WIDE_VOLUME)
def test_channel_volume_wide_frames(G, in_ch, out_ch):
    """k_channel_volume with no knob set: in + out > 320."""
    gains = np.linspace(0.2, 1.1, out_ch).astype(f32)
    for frames in FC.WIDE_FRAMES:
        x = FC.signal(frames + in_ch, frames * in_ch)
        want = FC.ref_channel_volume(x, in_ch, gains)
        for so, do in SAMPLE_OFFS:
            _same(_volume(x, frames, in_ch, gains, so, do), want, (frames, so, do))


@pytest.mark.parametrize("fmt,frm_ch,to_ch", FC.WIDE_PCM)
def test_decode_channels_wide_frames(G, fmt, frm_ch, to_ch):
    """k_pcm_to_channels<FMT, BYTES> with no knob set: frame_in_bytes + frame_out_bytes > 1280, a data chunk that ends inside its last frame;
    PCM16, i32 and f32 also at an odd byte address (every sample put together from its bytes)."""
    for frames in FC.WIDE_FRAMES:
        n = FC.cut(frames, frm_ch)
        raw = FC.pcm_bytes(frames, fmt, n)
        want = FC.ref_pcm_decode(raw, fmt, n, frm_ch, to_ch)
        for so, do in [(0, 0), (0, 1)] + ([(1, 0), (3, 2)] if fmt in ("i16", "i32", "f32") else [(1, 1)]):
            _same(_decode_channels(raw, fmt, n, frm_ch, to_ch, so, do), want, (frames, so, do))


def test_decode_24_bit_wide_frames(G):
    """rh_wav_decode keeps the layout: 183 channels of packed 24-bit are 1281 bytes a frame in + out, so k_pcm24_to_f32 converts and k_fill_zero
    completes the cut frame."""
    ch = FC.WIDE_PCM24_CHANNELS
    for frames in FC.WIDE_FRAMES:
        for n in FC.wide_pcm24_samples(frames):
            raw = FC.pcm_bytes(frames, "i24", n)
            want = FC.ref_pcm_decode(raw, "i24", n, ch)
            for so, do in ((0, 0), (1, 3), (2, 0)):
                _same(_decode(raw, "i24", n, ch, so, do), want, (frames, n, so, do))


# ===================================================================================== the ordinary layouts, pinned to the lane kernels ====
def test_layout_entries_pinned_to_the_lane_kernels(G):
    """RH_PCM_NO_TILE=1 at 6 -> 2, 2 -> 6, 1 -> 2, 2 -> 1 and 3 -> 5: k_channels_convert, k_channel_volume, k_pcm_to_channels<FMT, BYTES> for every
    PCM format at byte offsets 0, 1, 2, 3 and 5, rh_wav_decode for 8-, 16- and 32-bit samples with and without a cut frame (k_int_to_f32<T>,
    k_int_to_f32_scalar<T>, k_fill_zero): the bits of the unpinned call and of the reference."""
    from conftest import knobs

    jobs = []   # (what, run(), want)
    for frm_ch, to_ch in FC.ORDINARY_LAYOUTS:
        gains = np.linspace(0.2, 1.1, to_ch).astype(f32)
        for frames in FC.ORDINARY_LAYOUT_FRAMES:
            x = FC.signal(frames + frm_ch, frames * frm_ch)
            wc, wv = FC.ref_channels(x, frm_ch, to_ch), FC.ref_channel_volume(x, frm_ch, gains)
            for so, do in SAMPLE_OFFS:
                jobs.append((("channels", frm_ch, to_ch, frames, so, do), lambda x=x, a=(frames, frm_ch, to_ch, so, do): _channels(x, *a), wc))
                jobs.append((("volume", frm_ch, to_ch, frames, so, do), lambda x=x, a=(frames, frm_ch, gains, so, do): _volume(x, *a), wv))
            for fmt in FC.PCM:
                n = FC.cut(frames, frm_ch)
                raw = FC.pcm_bytes(frames + to_ch, fmt, n)
                want = FC.ref_pcm_decode(raw, fmt, n, frm_ch, to_ch)
                for so in FC.BYTE_OFFSETS:
                    jobs.append((("decode_channels", fmt, frm_ch, to_ch, frames, so), lambda raw=raw, a=(fmt, n, frm_ch, to_ch, so, so % 4): _decode_channels(raw, *a), want))
    for fmt, ch in FC.DECODE_LAYOUTS:
        for frames in FC.ORDINARY_LAYOUT_FRAMES:
            for cut in (0, 1):
                n = FC.cut(frames, ch) if cut else frames * ch
                raw = FC.pcm_bytes(frames + ch, fmt, n)
                want = FC.ref_pcm_decode(raw, fmt, n, ch)
                for so in FC.BYTE_OFFSETS:
                    jobs.append((("decode", fmt, ch, frames, cut, so), lambda raw=raw, a=(fmt, n, ch, so, so % 4): _decode(raw, *a), want))
    for what, run, want in jobs:
        _same(run(), want, ("unpinned",) + what)
    with knobs(RH_PCM_NO_TILE="1"):
        for what, run, want in jobs:
            _same(run(), want, ("pinned",) + what)


# ======================================================================================================== integer converters ====
@pytest.mark.parametrize("fmt", list(FC.INT_FORMATS))
def test_int_converters_every_value_rows_anywhere(G, fmt):
    """rh_convert_{i8, u8, i16, u16}_to_f32 on every source value, rows of n, n - 1 and n - 3 samples, src and dst each 0-3 elements off their
    boundary.  Unset: k_int_to_f32_lines on aligned rows, k_int_to_f32_scalar<int8_t | uint16_t> on the others (i16 and u8 take the tile kernel
    there); RH_PCM_NO_TILE=1: k_int_to_f32<T> on aligned rows, k_int_to_f32_scalar<T> on the others."""
    from conftest import knobs

    from rodio_amd import _lib

    dt = FC.INT_FORMATS[fmt][0]
    info = np.iinfo(dt)
    v = np.arange(info.min, info.max + 1, dtype=np.int64).astype(dt)
    if v.size < 4096:
        v = np.tile(v, 17)   # a few workgroups
    fn = getattr(_lib.lib, f"rh_convert_{fmt}_to_f32")

    def sweep(tag):
        for n in (v.size, v.size - 1, v.size - 3):
            want = FC.ref_int_to_f32(v[:n], fmt)
            for so in range(4):
                for do in range(4):
                    _same(_run(lambda d, s, st: _lib.check(fn(d, s, n, st), fmt), v[:n], n, so, do, what=(tag, fmt, n, so, do)), want, (tag, fmt, n, so, do))

    sweep("unset")
    with knobs(RH_PCM_NO_TILE="1"):
        sweep("pinned")


# ======================================================================================================= uniform wide blocks ====
@pytest.mark.parametrize("ch,rate,to_rate", FC.WIDE_UNIFORM)
def test_wide_mix_general_kernel_on_uniform_blocks(G, ch, rate, to_rate):
    """RH_WIDE_GENERAL=1 keeps a uniform block (one rate, the mixer's layout, every source live: test_gpu_widemix.py's) on k_wide_mix: the bits of
    k_wide_mix_uniform and of the reference, for the lerp and for from == to; 40 sources are two launches, the second continues the sum."""
    import torch

    from conftest import knobs

    from rodio_amd import _lib, source

    frames = FC.WIDE_UNIFORM_FRAMES
    srcs = FC.wide_uniform_sources(ch, rate, to_rate)
    want = FC.ref_wide_uniform(srcs, ch, rate, to_rate, frames)
    dev = [torch.from_numpy(x).cuda() for x, _ in srcs]

    def block(do):
        arr = (_lib.WideSrc * len(srcs))()
        for k, (x, g) in enumerate(srcs):
            arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = dev[k].data_ptr(), ch, rate, 0, frames, 0xFFFFFFFF, g
        dbuf, dp = _dst(frames * ch, do)
        _lib.check(_lib.lib.rh_wide_mix_block(C.c_void_p(dp), ch, to_rate, frames, arr, len(srcs), source._stream()), "rh_wide_mix_block")
        return _take(dbuf, frames * ch, do, what=("rh_wide_mix_block", ch, rate, to_rate, do))

    _same(block(0), want, "k_wide_mix_uniform")
    with knobs(RH_WIDE_GENERAL="1"):
        for do in (0, 1):
            _same(block(do), want, ("k_wide_mix", do))
