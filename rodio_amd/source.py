"""Host-side mirror of rodio's `Source` adapter interface over the HIP C ABI.

rodio composes per-sample pull iterators (`trait Source: Iterator<Item = f32>`,
/root/reference/src/source/mod.rs:179-218).  Here a source is a whole block resident in HBM and
every adapter is one (or one fused) kernel launch through librodio_hip.so; names, argument
order and end-of-stream behaviour follow the reference so the parity tests read like rodio's
own tests:

    out = rh.SampleRateConverter(rh.TestSource(x, 2, 44100), 44100, 48000, 2).collect()
    mixer = rh.Mixer(2, 48000); mixer.add(rh.SamplesBuffer(1, 48000, x)); mixer.next()

Device memory, streams and (in bench.py) torch.distributed come from PyTorch-ROCm; no torch op
computes audio.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from ._lib import AgcParams, LimitParams, RhError, RlmConfig, RlmGeometry, check, lib

_torch = None
_initialized = False


def _t():
    global _torch
    if _torch is None:
        import torch

        _torch = torch
    return _torch


def init(device: int = 0):
    """rh_init(): binds the library to a gfx950 device.  Raises RhError if there is none."""
    global _initialized
    torch = _t()
    if torch.cuda.is_available():
        torch.cuda.set_device(device)
    check(lib.rh_init(device), "rh_init")
    _initialized = True


def async_status(synchronize: bool = True):
    """rh_async_status(): raises RhError(RH_ERR_TIMEOUT) if a hand-off inside a handle-less scan kernel (`limit`, `biquad_batch`
    mode 1) expired in a launch that has completed -- by default after a device synchronise."""
    if synchronize:
        _t().cuda.synchronize()
    check(lib.rh_async_status(), "rh_async_status")


def _ensure():
    if not _initialized:
        init(_t().cuda.current_device() if _t().cuda.is_available() else 0)


def _stream():
    return C.c_void_p(_t().cuda.current_stream().cuda_stream)


def _dev_empty(n, dtype=None):
    torch = _t()
    return torch.empty(int(n), dtype=dtype or torch.float32, device="cuda")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


SPAN_NONE = None


class GpuSource:
    """A block-resident `Source`: interleaved f32 samples in HBM + (channels, sample_rate,
    current_span_len).  Adapters return new GpuSources; `collect()` copies to the host."""

    def __init__(self, samples, channels: int, sample_rate: int, span_len=None):
        if channels <= 0 or sample_rate <= 0:
            raise ValueError("channels and sample_rate are NonZero in rodio")
        self.samples = samples  # torch.float32 CUDA tensor, 1-D
        self._channels = int(channels)
        self._sample_rate = int(sample_rate)
        self.span_len = span_len  # None, or int (samples)

    # -- Source trait ---------------------------------------------------------------------
    def channels(self) -> int:
        return self._channels

    def sample_rate(self) -> int:
        return self._sample_rate

    def current_span_len(self):
        return self.span_len

    def __len__(self):
        return int(self.samples.numel())

    def collect(self) -> np.ndarray:
        _t().cuda.current_stream().synchronize()
        return self.samples.detach().cpu().numpy().copy()

    # -- builder methods (src/source/mod.rs:255-731) ---------------------------------------
    def amplify(self, factor: float) -> "GpuSource":
        _ensure()
        out = _dev_empty(len(self))
        check(lib.rh_amplify(_ptr(out), _ptr(self.samples), len(self), factor, _stream()), "rh_amplify")
        return GpuSource(out, self._channels, self._sample_rate, self.span_len)

    def amplify_decibel(self, db: float) -> "GpuSource":
        """source/mod.rs amplify_decibel / Amplify::set_log_factor (amplify.rs:33-35): factor = db_to_linear(dB)."""
        return self.amplify(float(lib.rh_db_to_linear(db)))

    def speed(self, factor: float) -> "GpuSource":
        """src/source/speed.rs:104-133: the samples are untouched, the reported rate is scaled."""
        r = np.float32(self._sample_rate) * np.float32(factor)
        return GpuSource(self.samples, self._channels, int(max(r, np.float32(1.0))), self.span_len)

    def delay(self, duration_ns: int) -> "GpuSource":
        """src/source/delay.rs:8-16,68-75."""
        _ensure()
        d = delay_samples(duration_ns, self._sample_rate, self._channels)
        out = _dev_empty(len(self) + d)
        check(lib.rh_delay(_ptr(out), _ptr(self.samples), len(self), d, _stream()), "rh_delay")
        return GpuSource(out, self._channels, self._sample_rate, None if self.span_len is None else self.span_len + d)

    def take_duration(self, duration_ns: int, fade_out: bool = False) -> "GpuSource":
        """src/source/take.rs:96-148.  current_span_len() behind it is what the duration still admits unless the input's span is
        shorter -- Some(..) over an input that says None too, Some(0) once it is spent (take.rs:176-195): a UniformSourceIterator
        behind it converts in chains of 32768 samples and ends in front of the silence that completes a cut frame (`_admits`)."""
        _ensure()
        out = _dev_empty(len(self) + self._channels)
        m, ended = C.c_uint64(0), C.c_int32(0)
        check(lib.rh_take_duration(_ptr(out), _ptr(self.samples), len(self), 0, self._channels, self._sample_rate, duration_ns,
                                   int(fade_out), C.byref(m), C.byref(ended), _stream()), "rh_take_duration")
        per_sample = 1_000_000_000 // (self._sample_rate * self._channels)
        admits = duration_ns // per_sample if per_sample else 0
        span = self.span_len if (self.span_len is not None and self.span_len < admits) else admits
        res = GpuSource(out[: m.value], self._channels, self._sample_rate, span)
        res._admits = min(admits, m.value)
        return res

    def distortion(self, gain: float, threshold: float) -> "GpuSource":
        _ensure()
        out = _dev_empty(len(self))
        check(lib.rh_distortion(_ptr(out), _ptr(self.samples), len(self), gain, threshold, _stream()), "rh_distortion")
        return GpuSource(out, self._channels, self._sample_rate, self.span_len)

    DITHER = {"GPDF": 0, "HighPass": 1, "RPDF": 2, "TPDF": 3}

    def dither(self, target_bits: int, algorithm: str = "TPDF", seed: int = 0, sample_offset: int = 0) -> "GpuSource":
        """src/source/dither.rs:217-242 with a counter-based noise generator (see rh_dither)."""
        _ensure()
        out = _dev_empty(len(self))
        check(lib.rh_dither(_ptr(out), _ptr(self.samples), len(self), sample_offset, self._channels, target_bits, self.DITHER[algorithm], seed, _stream()), "rh_dither")
        return GpuSource(out, self._channels, self._sample_rate, self.span_len)

    def linear_gain_ramp(self, duration_ns: int, start_gain: float, end_gain: float, clamp_end: bool, sample_offset: int = 0) -> "GpuSource":
        _ensure()
        out = _dev_empty(len(self))
        check(lib.rh_linear_gain_ramp(_ptr(out), _ptr(self.samples), len(self), sample_offset, self._channels, self._sample_rate,
                                      duration_ns, start_gain, end_gain, int(clamp_end), _stream()), "rh_linear_gain_ramp")
        return GpuSource(out, self._channels, self._sample_rate, self.span_len)

    def fade_in(self, duration_ns: int) -> "GpuSource":  # fadein.rs:11-13
        return self.linear_gain_ramp(duration_ns, 0.0, 1.0, False)

    def fade_out(self, duration_ns: int) -> "GpuSource":  # fadeout.rs:13
        return self.linear_gain_ramp(duration_ns, 1.0, 0.0, True)

    def _blt(self, kind: int, freq: int, q: float, mode: int) -> "GpuSource":
        _ensure()
        co = biquad_coeffs(kind, freq, q, self._sample_rate)
        out = _dev_empty(len(self))
        frames = len(self) // self._channels
        check(lib.rh_biquad(_ptr(out), _ptr(self.samples), frames, self._channels, 1,
                            co.ctypes.data_as(_lib.f32p), None, mode, _stream()), "rh_biquad")
        return GpuSource(out[: frames * self._channels], self._channels, self._sample_rate, self.span_len)

    def low_pass(self, freq: int, q: float = 0.5, mode: int = 0) -> "GpuSource":
        return self._blt(0, freq, q, mode)

    def high_pass(self, freq: int, q: float = 0.5, mode: int = 0) -> "GpuSource":
        return self._blt(1, freq, q, mode)

    def reverb(self, duration_ns: int, amplitude: float) -> "GpuSource":
        _ensure()
        d = delay_samples(duration_ns, self._sample_rate, self._channels)
        out = _dev_empty(len(self) + d)
        check(lib.rh_echo_mix(_ptr(out), _ptr(self.samples), len(self), d, amplitude, _stream()), "rh_echo_mix")
        return GpuSource(out, self._channels, self._sample_rate, None)

    def limit(self, threshold=-1.0, knee_width=4.0, attack_ns=5_000_000, release_ns=100_000_000) -> "GpuSource":
        """src/source/limit.rs:94-130,853-988.  A stream that ends inside a frame (rodio's own reverb with an odd delay
        makes one) is still limited sample by sample (limit.rs:927-988 advances one channel per sample): the block is
        padded to a whole frame -- the limiter is causal, the padding cannot reach the real samples -- and trimmed."""
        _ensure()
        torch = _t()
        p = LimitParams(threshold, knee_width, attack_ns, release_ns)
        n = len(self)
        frames = -(-n // self._channels)
        src = self.samples
        if frames * self._channels != n:
            src = torch.zeros(frames * self._channels, dtype=torch.float32, device="cuda")
            src[:n] = self.samples
        out = _dev_empty(frames * self._channels)
        check(lib.rh_limit(_ptr(out), _ptr(src), frames, self._channels, self._sample_rate, 1,
                           C.byref(p), None, _stream()), "rh_limit")
        return GpuSource(out[:n], self._channels, self._sample_rate, self.span_len)

    def automatic_gain_control(self, target_level=1.0, attack_ns=4_000_000_000, release_ns=0,
                               absolute_max_gain=7.0, floor=0.0) -> "GpuSource":
        _ensure()
        p = AgcParams(target_level, attack_ns, release_ns, absolute_max_gain, floor)
        out = _dev_empty(len(self))
        check(lib.rh_agc(_ptr(out), _ptr(self.samples), len(self), self._sample_rate, 1, C.byref(p), None,
                         _stream()), "rh_agc")
        return GpuSource(out, self._channels, self._sample_rate, self.span_len)

    def mix(self, other: "GpuSource") -> "GpuSource":
        """Source::mix (src/source/mod.rs:255, mix.rs:10-22,43-53): both inputs as UniformSourceIterators in THIS source's format --
        the identity on this one's samples, the span-by-span conversion of uniform.rs:50-97 on `other` -- then s1 + s2 while both run
        and the longer one's rest verbatim (rh_mix_pair).  current_span_len() behind it is None (mix.rs:83-91)."""
        if not isinstance(other, GpuSource):
            raise TypeError("mix() takes a GpuSource")
        _ensure()
        b = _uniform_row(other, self._channels, self._sample_rate)
        admits = getattr(self, "_admits", None)  # (the identity wrapper never asks a TakeDuration for the silence that completes a cut frame)
        na, nb = len(self) if admits is None else min(admits, len(self)), int(b.numel())
        out = _dev_empty(max(na, nb))
        check(lib.rh_mix_pair(_ptr(out), _ptr(self.samples), na, _ptr(b), nb, _stream()), "rh_mix_pair")
        return GpuSource(out, self._channels, self._sample_rate, None)

    def take_crossfade_with(self, other: "GpuSource", duration_ns: int) -> "GpuSource":
        """Source::take_crossfade_with (src/source/mod.rs:448, crossfade.rs:10-23): mix(self.take_duration(d) with the fade-out
        filter, other.take_duration(d).fade_in(d)), through the stand-alone calls (crossfade_batch is the fused form)."""
        if not isinstance(other, GpuSource):
            raise TypeError("take_crossfade_with() takes a GpuSource")
        if duration_ns < 0:
            raise ValueError("a Duration is not negative")
        a = self.take_duration(duration_ns, True)
        b = other.take_duration(duration_ns)
        if b._admits:  # (LinearGainRamp::new refuses a zero duration, which admits nothing)
            admits, b = b._admits, b.fade_in(duration_ns)
            b._admits = admits
        return a.mix(b)



def _upload(samples):
    torch = _t()
    a = np.ascontiguousarray(samples, dtype=np.float32).reshape(-1)
    if a.size == 0:
        return torch.empty(0, dtype=torch.float32, device="cuda")
    return torch.from_numpy(a).to("cuda")


def TestSource(samples, channels, sample_rate) -> GpuSource:
    """benches/shared.rs:6-46: a Vec<f32> source with current_span_len() == None."""
    return GpuSource(_upload(samples), channels, sample_rate, None)


def SamplesBuffer(channels, sample_rate, samples) -> GpuSource:
    """src/buffer.rs:23-140: current_span_len() == Some(len)."""
    s = _upload(samples)
    return GpuSource(s, channels, sample_rate, int(s.numel()))


def SpanSource(samples, channels, sample_rate, span_len) -> GpuSource:
    return GpuSource(_upload(samples), channels, sample_rate, int(span_len))


# ---- conversions ---------------------------------------------------------------------------
def SampleRateConverter(inp: GpuSource, from_rate: int, to_rate: int, channels: int, span_len=0) -> GpuSource:
    """src/conversions/sample_rate.rs:52-57 (same argument order).  span_len applies
    UniformSourceIterator's chunking (0 = one continuous stream)."""
    _ensure()
    torch = _t()
    frames, rem = divmod(len(inp), channels)
    if from_rate == to_rate and rem:  # sample_rate.rs:133-136: pure pass-through, half frames included
        return GpuSource(inp.samples.clone(), channels, to_rate, None)
    m = C.c_uint64(0)
    check(lib.rh_resample_out_frames(frames, from_rate, to_rate, channels, span_len, C.byref(m)), "rh_resample_out_frames")
    out = _dev_empty(m.value * channels)
    check(lib.rh_resample_linear(_ptr(out), _ptr(inp.samples), frames, from_rate, to_rate, channels, span_len,
                                 _stream()), "rh_resample_linear")
    if rem and span_len == 0:
        # A stream that ends mid-frame (rodio's own `reverb` with an odd delay produces one; the sources'
        # contract source/mod.rs:169-178 forbids it).  sample_rate.rs:174-200: frames are Vecs, the zip of
        # the last whole frame with the partial one yields only `rem` samples per output position, then
        # the partial frame is drained verbatim.  A handful of samples: done here, on the host, in f32.
        g = np.gcd(from_rate, to_rate)
        F, T = from_rate // g, to_rate // g
        tail_in = inp.samples[max(frames - 1, 0) * channels:].cpu().numpy()
        part = tail_in[-rem:]
        if frames == 0:
            return GpuSource(_upload(part), channels, to_rate, None)
        last = tail_in[:channels]
        c1 = -((-(frames - 1) * T) // F)  # output positions whose two taps are whole frames
        tail, mm = [], c1
        while (mm * F) // T == frames - 1:
            num = np.float32((mm * F) % T)
            tail += [np.float32(last[c] + (part[c] - last[c]) * num / np.float32(T)) for c in range(rem)]  # math.rs:23-26
            mm += 1
        if (mm * F) // T == frames:
            tail += [np.float32(v) for v in part]
        out = torch.cat([out[: c1 * channels], _upload(np.asarray(tail, np.float32))]) if tail else out[: c1 * channels]
    return GpuSource(out, channels, to_rate, None)


def ChannelCountConverter(inp: GpuSource, from_ch: int, to_ch: int) -> GpuSource:
    """src/conversions/channels.rs:28."""
    _ensure()
    if from_ch == to_ch:  # channels.rs:57-85 degenerates to a pass-through, half frames included
        return GpuSource(inp.samples, to_ch, inp.sample_rate(), inp.span_len)
    frames = len(inp) // from_ch
    out = _dev_empty(frames * to_ch)
    check(lib.rh_channels_convert(_ptr(out), _ptr(inp.samples), frames, from_ch, to_ch, _stream()), "rh_channels_convert")
    return GpuSource(out, to_ch, inp.sample_rate(), inp.span_len)


def UniformSourceIterator(inp: GpuSource, channels: int, sample_rate: int) -> GpuSource:
    """src/source/uniform.rs:50-97: ChannelCountConverter<SampleRateConverter<Take<I>>> restarted
    every min(current_span_len, 32768) samples."""
    span = inp.current_span_len() or 0
    admits = getattr(inp, "_admits", None)
    if admits is not None and admits < len(inp):  # (a TakeDuration answers Some(0) there: the iterator never asks for the frame's padding)
        inp = GpuSource(inp.samples[:admits], inp.channels(), inp.sample_rate(), inp.span_len)
    if min(span, 32768) >= len(inp):  # one chain for everything: the same as a continuous stream (and the form that knows a cut last frame)
        span = 0
    r = SampleRateConverter(inp, inp.sample_rate(), sample_rate, inp.channels(), span)
    return ChannelCountConverter(r, inp.channels(), channels)


def _uniform_row(inp: GpuSource, channels: int, sample_rate: int):
    """UniformSourceIterator over the whole row as rh_uniform_row runs it: chains that cut a frame included."""
    admits = getattr(inp, "_admits", None)
    n = len(inp) if admits is None else min(admits, len(inp))  # (a TakeDuration answers Some(0) behind what it admits)
    span = inp.current_span_len() or 0
    m = C.c_uint64(0)
    check(lib.rh_uniform_row_out_samples(n, inp.channels(), inp.sample_rate(), channels, sample_rate, span, C.byref(m)), "rh_uniform_row_out_samples")
    out = _dev_empty(m.value)
    check(lib.rh_uniform_row(_ptr(out), m.value, _ptr(inp.samples), n, inp.channels(), inp.sample_rate(), channels, sample_rate, span, C.byref(m),
                             _stream()), "rh_uniform_row")
    return out


def crossfade_batch(a, b, duration_ns: int):
    """rh_crossfade: a[k].take_crossfade_with(b[k], duration) for every pair of the two lists in one call (one launch for the pairs
    the fused kernel takes).  Returns the crossfades as GpuSources in a[k]'s format."""
    a, b = list(a), list(b)
    if len(a) != len(b):
        raise ValueError("crossfade_batch takes as many second inputs as first ones")
    if any(not isinstance(x, GpuSource) for x in a + b):
        raise TypeError("crossfade_batch takes GpuSources")
    if duration_ns < 0:
        raise ValueError("a Duration is not negative")
    if not a:
        return []
    _ensure()
    W = _lib.CROSSFADE_PAIR_WORDS
    pairs = (C.c_uint64 * (W * len(a)))()
    outs = []
    for k, (x, y) in enumerate(zip(a, b)):
        pairs[W * k: W * k + 9] = [x.samples.data_ptr(), len(x), x.channels(), x.sample_rate(), y.samples.data_ptr(), len(y), y.channels(), y.sample_rate(), y.current_span_len() or 0]
        m = C.c_uint64(0)
        check(lib.rh_crossfade_out_samples(C.cast(C.byref(pairs, 8 * W * k), C.POINTER(C.c_uint64)), duration_ns, C.byref(m)), "rh_crossfade_out_samples")
        outs.append(_dev_empty(m.value))
        pairs[W * k + 9], pairs[W * k + 10] = outs[-1].data_ptr(), m.value
    got = (C.c_uint64 * len(a))()
    check(lib.rh_crossfade(pairs, len(a), duration_ns, got, _stream()), "rh_crossfade")
    return [GpuSource(o[: got[k]], x.channels(), x.sample_rate(), None) for k, (o, x) in enumerate(zip(outs, a))]


_CONV = {
    ("i8", "f32"): ("rh_convert_i8_to_f32", np.int8, np.float32),
    ("u8", "f32"): ("rh_convert_u8_to_f32", np.uint8, np.float32),
    ("i16", "f32"): ("rh_convert_i16_to_f32", np.int16, np.float32),
    ("u16", "f32"): ("rh_convert_u16_to_f32", np.uint16, np.float32),
    ("i24", "f32"): ("rh_convert_i24_to_f32", np.int32, np.float32),
    ("i32", "f32"): ("rh_convert_i32_to_f32", np.int32, np.float32),
    ("f32", "i8"): ("rh_convert_f32_to_i8", np.float32, np.int8),
    ("f32", "i16"): ("rh_convert_f32_to_i16", np.float32, np.int16),
    ("f32", "u16"): ("rh_convert_f32_to_u16", np.float32, np.uint16),
    ("f32", "i32"): ("rh_convert_f32_to_i32", np.float32, np.int32),
    ("f32", "u8"): ("rh_convert_f32_to_u8", np.float32, np.uint8),
    ("f32", "i24"): ("rh_convert_f32_to_i24", np.float32, np.int32),
    ("f32", "u24"): ("rh_convert_f32_to_u24", np.float32, np.int32),
    ("f32", "u32"): ("rh_convert_f32_to_u32", np.float32, np.uint32),
    ("f32", "i64"): ("rh_convert_f32_to_i64", np.float32, np.int64),
    ("f32", "u64"): ("rh_convert_f32_to_u64", np.float32, np.uint64),
    ("f32", "f64"): ("rh_convert_f32_to_f64", np.float32, np.float64),
    ("u24", "f32"): ("rh_convert_u24_to_f32", np.int32, np.float32),
    ("u32", "f32"): ("rh_convert_u32_to_f32", np.uint32, np.float32),
    ("i64", "f32"): ("rh_convert_i64_to_f32", np.int64, np.float32),
    ("u64", "f32"): ("rh_convert_u64_to_f32", np.uint64, np.float32),
    ("f64", "f32"): ("rh_convert_f64_to_f32", np.float64, np.float32),
}


def SampleTypeConverter(samples, src: str, dst: str) -> np.ndarray:
    """src/conversions/sample.rs:6-44 (`SampleTypeConverter<I, O>`; north_star's "DataConverter").
    Host array in, host array out; the conversion itself runs on the GPU."""
    _ensure()
    torch = _t()
    fn, st, dt = _CONV[(src, dst)]
    a = np.ascontiguousarray(samples, dtype=st)
    # torch has no uint16 arithmetic but can carry the bytes
    d_in = torch.from_numpy(a.view(np.uint8).reshape(-1)).to("cuda") if a.size else torch.empty(0, dtype=torch.uint8, device="cuda")
    d_out = torch.empty(a.size * np.dtype(dt).itemsize, dtype=torch.uint8, device="cuda")
    check(getattr(lib, fn)(_ptr(d_out), _ptr(d_in), a.size, _stream()), fn)
    torch.cuda.current_stream().synchronize()
    return d_out.cpu().numpy().view(dt).copy()


# ---- WAV either side of the path -----------------------------------------------------------------
def wav_probe(file_bytes: bytes):
    """RIFF chunk walk on the host (no GPU needed): dict of the fmt fields + data chunk position."""
    info = _lib.WavInfo()
    buf = (C.c_uint8 * len(file_bytes)).from_buffer_copy(file_bytes)
    check(lib.rh_wav_probe_host(buf, len(file_bytes), C.byref(info)), "rh_wav_probe_host")
    return {n: getattr(info, n) for n, _ in _lib.WavInfo._fields_}


def _wav_data_on_device(file_bytes: bytes, w, image: bool):
    """The data chunk on the device: a copy of its own, or (image=True) the whole file uploaded as it is and the chunk taken where it lies
    -- `file + data_offset`, whatever byte address that is."""
    torch = _t()
    if image and w["data_bytes"]:
        whole = torch.from_numpy(np.frombuffer(file_bytes, dtype=np.uint8).copy()).to("cuda")
        return whole[w["data_offset"]: w["data_offset"] + w["data_bytes"]]
    raw = np.frombuffer(file_bytes, dtype=np.uint8, count=w["data_bytes"], offset=w["data_offset"])
    return torch.from_numpy(raw.copy()).to("cuda") if raw.size else None


def WavDecoder(file_bytes: bytes, image: bool = False) -> "GpuSource":
    """src/decoder/wav.rs: the data chunk goes to the device as bytes and is converted there."""
    _ensure()
    torch = _t()
    w = wav_probe(file_bytes)
    d_in = _wav_data_on_device(file_bytes, w, image)
    raw = np.empty(0 if d_in is None else 1, np.uint8)
    if d_in is None:
        d_in = torch.empty(0, dtype=torch.uint8, device="cuda")
    out = _dev_empty(w["samples"] + w["channels"])
    m = C.c_uint64(0)
    check(lib.rh_wav_decode(_ptr(out), _ptr(d_in) if raw.size else None, w["samples"], w["channels"], w["bits_per_sample"],
                            w["is_float"], C.byref(m), _stream()), "rh_wav_decode")
    return GpuSource(out[: m.value], w["channels"], w["sample_rate"], None)


def WavDecoderChannels(file_bytes: bytes, to_channels: int, image: bool = False) -> "GpuSource":
    """`UniformSourceIterator::new(decoder, to_channels, the file's rate)`: src/decoder/wav.rs + src/conversions/channels.rs:57-85 in ONE
    launch (rh_wav_decode_channels) -- the decoded block in the file's own layout never exists."""
    _ensure()
    torch = _t()
    w = wav_probe(file_bytes)
    d_in = _wav_data_on_device(file_bytes, w, image)
    if d_in is None:
        d_in = torch.empty(1, dtype=torch.uint8, device="cuda")
    frames = (w["samples"] + w["channels"] - 1) // w["channels"]
    out = _dev_empty(frames * to_channels + 4)
    m = C.c_uint64(0)
    check(lib.rh_wav_decode_channels(_ptr(out), _ptr(d_in), w["samples"], w["channels"], w["bits_per_sample"], w["is_float"], to_channels, C.byref(m), _stream()),
          "rh_wav_decode_channels")
    return GpuSource(out[: m.value], to_channels, w["sample_rate"], None)


def wav_to_bytes(source: "GpuSource") -> bytes:
    """src/wav_output.rs:62-96: 32-bit float WAVE of the source's whole frames."""
    n = len(source)
    hdr = (C.c_uint8 * 44)()
    k = lib.rh_wav_header_f32_host(hdr, 44, source.channels(), source.sample_rate(), n)
    if k != 44:
        raise RhError(1, "rh_wav_header_f32_host")
    whole = n - n % source.channels()
    return bytes(hdr) + source.samples[:whole].cpu().numpy().astype("<f4").tobytes()


# ---- effects -------------------------------------------------------------------------------
def ChannelVolume(inp: GpuSource, gains) -> GpuSource:
    """src/source/channel_volume.rs:29-37,71-88."""
    _ensure()
    g = np.ascontiguousarray(gains, dtype=np.float32)
    frames = len(inp) // inp.channels()
    out = _dev_empty(frames * g.size)
    check(lib.rh_channel_volume(_ptr(out), _ptr(inp.samples), frames, inp.channels(), g.ctypes.data_as(_lib.f32p),
                                g.size, _stream()), "rh_channel_volume")
    return GpuSource(out, g.size, inp.sample_rate(), inp.span_len)


def spatial_gains(emitter, left, right) -> np.ndarray:
    e, l, r = (np.ascontiguousarray(x, dtype=np.float32) for x in (emitter, left, right))
    out = np.zeros(2, np.float32)
    P = _lib.f32p
    check(lib.rh_spatial_gains(e.ctypes.data_as(P), l.ctypes.data_as(P), r.ctypes.data_as(P), out.ctypes.data_as(P)),
          "rh_spatial_gains")
    return out


def Spatial(inp: GpuSource, emitter, left, right) -> GpuSource:
    """src/source/spatial.rs:26-46."""
    return ChannelVolume(inp, spatial_gains(emitter, left, right))


def spatial_gains_batch(emitters, left, right):
    """Device tensor [S, 2] of Spatial gains (one rh_spatial_gains per emitter)."""
    torch = _t()
    gains = np.stack([spatial_gains(e, left, right) for e in emitters]).astype(np.float32)
    return torch.from_numpy(gains).to("cuda")


def reverb_spatial_batch(x, sample_rate, duration_ns, amplitude, emitters, left, right, out=None, gains_dev=None):
    """BASELINE config 3 in one kernel: for every row s of the device tensor x [S, n] (interleaved stereo)
    `Spatial(reverb(x_s, duration, amplitude), emitters[s], left, right)`.  Returns [S, n_out] on device."""
    _ensure()
    torch = _t()
    S, n = x.shape
    d = delay_samples(duration_ns, sample_rate, 2)
    n_out = 2 * ((n + d) // 2)
    g_dev = gains_dev if gains_dev is not None else spatial_gains_batch(emitters, left, right)
    if out is None:
        stride = (n_out + 3) // 4 * 4
        out = torch.empty((S, stride), device="cuda", dtype=torch.float32)
    check(lib.rh_reverb_spatial(_ptr(out), _ptr(x), n, d, amplitude, _ptr(g_dev), S, x.stride(0), out.stride(0), _stream()),
          "rh_reverb_spatial")
    return out[:, :n_out]


def biquad_batch(x, coeffs5, mode=1, out=None):
    """rh_biquad over the rows of the device tensor x [S, frames*2] (stereo streams laid out back to
    back).  mode 0 = sequential (bit-exact), mode 1 = time-parallel scan."""
    _ensure()
    torch = _t()
    assert x.is_contiguous() and x.dim() == 2
    S, n = x.shape
    if out is None:
        out = torch.empty_like(x)
    co = np.ascontiguousarray(coeffs5, dtype=np.float32)
    check(lib.rh_biquad(_ptr(out), _ptr(x), n // 2, 2, S, co.ctypes.data_as(_lib.f32p), None, mode, _stream()), "rh_biquad")
    return out


def _check_state(state, shape, who):
    """A carried state is a contiguous float32 device tensor of exactly the elements the kernel will read and write."""
    if state is None:
        return
    torch = _t()
    want = int(np.prod(shape))
    if state.dtype != torch.float32 or not state.is_cuda or not state.is_contiguous() or state.numel() != want:
        raise ValueError(f"{who}: state must be a contiguous float32 CUDA tensor of {want} elements (shape {tuple(shape)}), got {state.dtype} {tuple(state.shape)} on {state.device}")


def limit_batch(x, channels, sample_rate, threshold=-1.0, knee_width=4.0, attack_ns=5_000_000, release_ns=100_000_000, state=None, out=None):
    """rh_limit over the rows of the device tensor x [S, frames*channels] (limit.rs:853-988, one limiter per row).
    state: optional device tensor [S, 2*channels] {integrator, peak} per channel, carried across blocks (updated in place)."""
    _ensure()
    torch = _t()
    assert x.is_contiguous() and x.dim() == 2
    S, n = x.shape
    if n % channels:
        raise ValueError(f"rows of {n} samples are not whole frames of {channels} channels (the kernel's row stride is frames * channels)")
    _check_state(state, (S, 2 * channels), "limit_batch")
    if out is None:
        out = torch.empty_like(x)
    p = LimitParams(threshold, knee_width, attack_ns, release_ns)
    check(lib.rh_limit(_ptr(out), _ptr(x), n // channels, channels, sample_rate, S, C.byref(p), _ptr(state) if state is not None else None, _stream()), "rh_limit")
    return out


def agc_state(n_streams):
    """Fresh AutomaticGainControl states (agc.rs:209-236) for n_streams rows, on the device."""
    _ensure()
    st = _dev_empty(int(lib.rh_agc_state_floats()) * n_streams)
    check(lib.rh_agc_state_init(_ptr(st), n_streams, _stream()), "rh_agc_state_init")
    return st


def agc_batch(x, sample_rate, target_level=1.0, attack_ns=4_000_000_000, release_ns=0, absolute_max_gain=7.0, floor=0.0, state=None, out=None):
    """rh_agc over the rows of the device tensor x [S, n_samples] (agc.rs:397-504, one AGC per row; all interleaved channels of a
    row share it).  state: agc_state(S), carried across blocks."""
    _ensure()
    torch = _t()
    assert x.is_contiguous() and x.dim() == 2
    S, n = x.shape
    _check_state(state, (S * int(lib.rh_agc_state_floats()),), "agc_batch")
    if out is None:
        out = torch.empty_like(x)
    p = AgcParams(target_level, attack_ns, release_ns, absolute_max_gain, floor)
    check(lib.rh_agc(_ptr(out), _ptr(x), n, sample_rate, S, C.byref(p), _ptr(state) if state is not None else None, _stream()), "rh_agc")
    return out


def biquad_coeffs(kind, freq, q, fs) -> np.ndarray:
    out = np.zeros(5, np.float32)
    k = 1 if kind in (1, "high_pass") else 0
    check(lib.rh_biquad_coeffs(k, freq, q, fs, out.ctypes.data_as(_lib.f32p)), "rh_biquad_coeffs")
    return out


def filter_scan_ok(kind, freq, q, fs) -> bool:
    """The filter contract (rodio_hip.h, rh_filter_scan_ok): does the time-parallel evaluation of this low_pass / high_pass stay within
    1e-5 of rodio's own f32 recurrence for full-scale white noise?  (On DC-heavy material through low cutoffs rodio's recurrence is biased
    by more, and the two differ by that bias: the table in rodio_hip.h.)"""
    return bool(lib.rh_filter_scan_ok(1 if kind in (1, "high_pass") else 0, int(freq), float(q), int(fs)))


def wide_mix_block_filtered(dst, channels, to_rate, out_frames, srcs, filters, mode=1, scratch=None):
    """rh_wide_mix_block_filtered: a block of a mixer of any channel count whose sources may carry a low_pass / high_pass.
    srcs: a `_lib.WideSrc` array; filters: per source None or (kind, freq, q[, state]) or (kind, coeffs5[, state]) -- kind 0 / "low_pass",
    1 / "high_pass", coeffs5 five floats {b0,b1,b2,a1,a2}, state a device tensor of 4 * channels floats carried across blocks (updated in
    place) or None.  scratch: a float32 device tensor for the rows (allocated here when None)."""
    _ensure()
    torch = _t()
    n = len(srcs)
    kinds = (C.c_int32 * max(n, 1))()
    coeffs = np.zeros((max(n, 1), 5), np.float32)
    states = (C.c_void_p * max(n, 1))()
    filtered = 0
    for k, f in enumerate(filters):
        kinds[k] = -1
        if f is None:
            continue
        filtered += 1
        kinds[k] = 1 if f[0] in (1, "high_pass") else 0
        if np.ndim(f[1]) == 0:
            coeffs[k] = biquad_coeffs(kinds[k], f[1], f[2], to_rate)
            state = f[3] if len(f) > 3 else None
        else:
            coeffs[k] = np.asarray(f[1], np.float32)
            state = f[2] if len(f) > 2 else None
        _check_state(state, (4 * channels,), "wide_mix_block_filtered")
        states[k] = _ptr(state) if state is not None else None
    need = C.c_uint64(0)
    check(lib.rh_wide_mix_filtered_scratch_bytes(channels, out_frames, filtered, C.byref(need)), "rh_wide_mix_filtered_scratch_bytes")
    if scratch is None and need.value:
        scratch = torch.empty(need.value // 4, device="cuda", dtype=torch.float32)
    check(lib.rh_wide_mix_block_filtered(_ptr(dst), channels, to_rate, out_frames, srcs, n, kinds, coeffs.ctypes.data_as(_lib.f32p), states, mode,
                                         _ptr(scratch) if scratch is not None else None, scratch.numel() * 4 if scratch is not None else 0, _stream()),
          "rh_wide_mix_block_filtered")
    return dst


class SpatialSrc:
    """One emitter of spatial_mix_block: a source as rh_wide_mix_block reads it (data: a float32 device tensor or a device address; in_ch,
    from_rate, phase, frames, last) with ChannelVolume's volumes by steps (gains: a float32 device tensor [entries, channels] or a device
    address with n_gains; gain_first, gain_period) and the Amplify behind it (factors: [entries] or None; factor_first, factor_period)."""

    def __init__(self, data, in_ch, from_rate, frames, gains, gain_period, gain_first=0, factors=None, factor_period=1, factor_first=0, phase=0,
                 last=0xFFFFFFFF, n_gains=None, n_factors=None):
        self.data, self.in_ch, self.from_rate, self.phase, self.frames, self.last = data, int(in_ch), int(from_rate), int(phase), int(frames), int(last)
        self.gains, self.gain_first, self.gain_period, self.n_gains = gains, int(gain_first), int(gain_period), n_gains
        self.factors, self.factor_first, self.factor_period, self.n_factors = factors, int(factor_first), int(factor_period), n_factors


def spatial_mix_block(dst, channels, to_rate, out_frames, srcs):
    """rh_spatial_mix_block: a block of a mixer of spatial emitters in one launch -- per source SampleRateConverter(Amplify(ChannelVolume(x)))
    with the volumes and the factor changing by steps, and the ordered sum.  dst: a float32 device tensor of out_frames * channels
    elements (or a device address); srcs: SpatialSrc objects in insertion order."""
    _ensure()
    n = len(srcs)
    arr = (_lib.WideSrc * max(n, 1))()
    gains, factors = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    gsteps, fsteps = (C.c_uint64 * (3 * max(n, 1)))(), (C.c_uint64 * (3 * max(n, 1)))()

    def table(t, entries, width, who):
        """(address, entries) of a step table: a contiguous float32 CUDA tensor of whole entries, or an address with its count"""
        if t is None:
            return None, 0
        if isinstance(t, int):
            if entries is None:
                raise ValueError(f"spatial_mix_block: {who} given as an address needs its number of entries")
            return t, int(entries)
        torch = _t()
        if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous() or t.numel() % width:
            raise ValueError(f"spatial_mix_block: {who} must be a contiguous float32 CUDA tensor of whole entries of {width}, got {t.dtype} {tuple(t.shape)} on {t.device}")
        return t.data_ptr(), (t.numel() // width if entries is None else int(entries))

    for k, s in enumerate(srcs):
        arr[k].data = s.data if isinstance(s.data, int) or s.data is None else s.data.data_ptr()
        arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = s.in_ch, s.from_rate, s.phase, s.frames, s.last, 1.0
        gains[k], gsteps[3 * k + 2] = table(s.gains, s.n_gains, channels, "gains")
        gsteps[3 * k], gsteps[3 * k + 1] = s.gain_first, s.gain_period
        factors[k], fsteps[3 * k + 2] = table(s.factors, s.n_factors, 1, "factors")
        fsteps[3 * k], fsteps[3 * k + 1] = s.factor_first, s.factor_period
    check(lib.rh_spatial_mix_block(C.c_void_p(dst) if isinstance(dst, int) else _ptr(dst), channels, to_rate, out_frames, arr, n, gains, gsteps, factors, fsteps, _stream()),
          "rh_spatial_mix_block")
    return dst


RAMP_KINDS = {None: 0, "none": 0, "ramp": 1, "fade_in": 1, "clamp": 2, "fade_out": 2}


class PlayerSrc:
    """One source of player_mix_block: a source as rh_wide_mix_block reads it (data: a float32 device tensor or a device address; channels,
    from_rate -- the rate behind `speed` --, phase, frames, last, gain: the innermost Amplify) with the two adapters a Player's sound carries:
    a LinearGainRamp (ramp: None, "ramp" / "fade_in" / 1 = clamp_end false, "clamp" / "fade_out" / 2 = clamp_end true; ramp_ns, start_gain,
    end_gain, first_frame = frames of the ramp's stream in front of data, ramp_rate = the rate in FRONT of `speed`, from_rate by default;
    fade_in and fade_out bring their gains) and the Amplify under periodic_access (factors: [entries] float32 device tensor, or an address
    with n_factors, or None; factor_first, factor_period)."""

    def __init__(self, data, channels, from_rate, frames, gain=1.0, ramp=None, ramp_ns=0, start_gain=None, end_gain=None, first_frame=0, ramp_rate=None,
                 factors=None, factor_period=1, factor_first=0, phase=0, last=0xFFFFFFFF, n_factors=None):
        self.data, self.channels, self.from_rate, self.phase, self.frames, self.last, self.gain = data, int(channels), int(from_rate), int(phase), int(frames), int(last), float(gain)
        self.kind = RAMP_KINDS[ramp] if ramp in RAMP_KINDS else int(ramp)
        preset = {"fade_in": (0.0, 1.0), "fade_out": (1.0, 0.0)}.get(ramp, (1.0, 1.0))
        self.ramp_ns, self.first_frame, self.ramp_rate = int(ramp_ns), int(first_frame), int(from_rate if ramp_rate is None else ramp_rate)
        self.start_gain, self.end_gain = float(preset[0] if start_gain is None else start_gain), float(preset[1] if end_gain is None else end_gain)
        self.factors, self.factor_first, self.factor_period, self.n_factors = factors, int(factor_first), int(factor_period), n_factors


def player_mix_block(dst, channels, to_rate, out_frames, srcs):
    """rh_player_mix_block: a block of a mixer of Players in one launch -- per source the gain, the LinearGainRamp, the stepped Amplify,
    the converter to the mixer's rate and layout, and the ordered sum.  dst: a float32 device tensor of out_frames * channels elements
    (or a device address); srcs: PlayerSrc objects in insertion order."""
    _ensure()
    n = len(srcs)
    arr = (_lib.WideSrc * max(n, 1))()
    ramps, gains = (C.c_uint64 * (4 * max(n, 1)))(), (C.c_float * (2 * max(n, 1)))()
    factors, fsteps = (C.c_void_p * max(n, 1))(), (C.c_uint64 * (3 * max(n, 1)))()
    for k, s in enumerate(srcs):
        arr[k].data = s.data if isinstance(s.data, int) or s.data is None else s.data.data_ptr()
        arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = s.channels, s.from_rate, s.phase, s.frames, s.last, s.gain
        ramps[4 * k], ramps[4 * k + 1], ramps[4 * k + 2], ramps[4 * k + 3] = s.kind, s.ramp_ns, s.first_frame, s.ramp_rate
        gains[2 * k], gains[2 * k + 1] = s.start_gain, s.end_gain
        t = s.factors
        if t is None:
            factors[k], entries = None, 0
        elif isinstance(t, int):
            if s.n_factors is None:
                raise ValueError("player_mix_block: factors given as an address need their number of entries")
            factors[k], entries = t, int(s.n_factors)
        else:
            torch = _t()
            if t.dtype != torch.float32 or not t.is_cuda or not t.is_contiguous():
                raise ValueError(f"player_mix_block: factors must be a contiguous float32 CUDA tensor, got {t.dtype} {tuple(t.shape)} on {t.device}")
            factors[k], entries = t.data_ptr(), (t.numel() if s.n_factors is None else int(s.n_factors))
        fsteps[3 * k], fsteps[3 * k + 1], fsteps[3 * k + 2] = s.factor_first, s.factor_period, entries
    check(lib.rh_player_mix_block(C.c_void_p(dst) if isinstance(dst, int) else _ptr(dst), channels, to_rate, out_frames, arr, n, ramps, gains, factors, fsteps, _stream()),
          "rh_player_mix_block")
    return dst


LOOP_WORDS = 5  # RH_LOOP_WORDS


def loop_plan(n_samples, channels, span_len=0):
    """rh_loop_plan: the words [loop_frames, chain_frames, rule, chain_start, chain_out] of a sound of n_samples samples handed to
    repeat_infinite(), as rodio would play it; span_len = what the sound answers to current_span_len() while fresh (0: None;
    n_samples: a SamplesBuffer).  The cursor starts at 0.  Host arithmetic: no device is touched."""
    w = (C.c_uint64 * LOOP_WORDS)()
    check(lib.rh_loop_plan(n_samples, channels, span_len, w), "rh_loop_plan")
    return list(w)


def loop_advance(words, from_rate, to_rate, out_frames):
    """rh_loop_advance: the words of a loop behind a block of out_frames output frames (a new list; words of a plain source come back as
    they are).  Any cut of a stream into blocks gives the bits of one pass."""
    w = (C.c_uint64 * LOOP_WORDS)(*[int(v) for v in words])
    check(lib.rh_loop_advance(w, from_rate, to_rate, out_frames), "rh_loop_advance")
    return list(w)


class LoopSrc:
    """One source of loop_mix_block.  With words (loop_plan's, moved by loop_advance): a loop -- data is frame 0 of the resident pass (a float32
    device tensor or a device address), frames the block's output frames it reaches; phase and last are not read.  Without: a source as
    rh_wide_mix_block reads it."""

    def __init__(self, data, channels, from_rate, frames, gain=1.0, words=None, phase=0, last=0xFFFFFFFF):
        self.data, self.channels, self.from_rate, self.phase, self.frames, self.last, self.gain = data, int(channels), int(from_rate), int(phase), int(frames), int(last), float(gain)
        self.words = [0] * LOOP_WORDS if words is None else [int(v) for v in words]
        if len(self.words) != LOOP_WORDS:
            raise ValueError(f"LoopSrc: a loop travels as {LOOP_WORDS} words, got {len(self.words)}")


def loop_mix_block(dst, channels, to_rate, out_frames, srcs):
    """rh_loop_mix_block: a block of a mixer whose sources may be loops (source.repeat_infinite()), each read from one resident pass: the
    gain, the converter chain by chain as rodio cuts it, the channel rule and the ordered sum, one launch per 32 sources.  dst: a float32
    device tensor of out_frames * channels elements (or a device address); srcs: LoopSrc objects in insertion order."""
    _ensure()
    n = len(srcs)
    arr = (_lib.WideSrc * max(n, 1))()
    words = (C.c_uint64 * (LOOP_WORDS * max(n, 1)))()
    for k, s in enumerate(srcs):
        arr[k].data = s.data if isinstance(s.data, int) or s.data is None else s.data.data_ptr()
        arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = s.channels, s.from_rate, s.phase, s.frames, s.last, s.gain
        words[LOOP_WORDS * k:LOOP_WORDS * (k + 1)] = s.words
    check(lib.rh_loop_mix_block(C.c_void_p(dst) if isinstance(dst, int) else _ptr(dst), channels, to_rate, out_frames, arr, n, words, _stream()), "rh_loop_mix_block")
    return dst


QUEUE_WORDS = 4  # RH_QUEUE_WORDS: chain_start, chain_out, state, flags
QUEUE_SOUND_WORDS = 4  # RH_QUEUE_SOUND_WORDS: data, samples, channels, rate
QUEUE_PLAYING, QUEUE_SILENT, QUEUE_ENDED = 0, 1, 2


class QueueSound:
    """One sound of a queue, resident as a whole: data (a float32 device tensor or a device address; None for an empty sound), samples
    (the tensor's element count by default), channels and rate as the sound reports them, gain = the Amplify in front of the queue."""

    def __init__(self, data, channels, rate, gain=1.0, samples=None):
        if samples is None:
            if data is None or isinstance(data, int):
                raise ValueError("QueueSound: data given as an address needs its number of samples")
            samples = data.numel()
        self.data, self.samples, self.channels, self.rate, self.gain = data, int(samples), int(channels), int(rate), float(gain)

    def address(self):
        return 0 if self.data is None else (self.data if isinstance(self.data, int) else self.data.data_ptr())


def _queue_sounds(sounds):
    n = len(sounds)
    words, gains = (C.c_uint64 * (QUEUE_SOUND_WORDS * max(n, 1)))(), (C.c_float * max(n, 1))()
    for k, q in enumerate(sounds):
        words[QUEUE_SOUND_WORDS * k:QUEUE_SOUND_WORDS * (k + 1)] = [q.address(), q.samples, q.channels, q.rate]
        gains[k] = q.gain
    return words, gains


def queue_plan(keep_alive=True):
    """rh_queue_plan: the cursor [chain_start, chain_out, state, flags] of a fresh queue (keep_alive: every Player's queue).  Host
    arithmetic: no device is touched."""
    w = (C.c_uint64 * QUEUE_WORDS)()
    check(lib.rh_queue_plan(w, 1 if keep_alive else 0), "rh_queue_plan")
    return list(w)


def queue_advance(words, sounds, to_rate, out_frames):
    """rh_queue_advance: (the cursor behind a block of out_frames output frames -- a new list --, how many of `sounds` the caller drops
    from the front before the next block).  sounds: QueueSound objects from the one in which the chain in progress started.  Any cut of a
    stream into blocks gives the bits of one pass."""
    w = (C.c_uint64 * QUEUE_WORDS)(*[int(v) for v in words])
    sw, _ = _queue_sounds(sounds)
    dropped = C.c_uint32(0)
    check(lib.rh_queue_advance(w, sw, len(sounds), to_rate, out_frames, C.byref(dropped)), "rh_queue_advance")
    return list(w), dropped.value


class QueueSrc:
    """One source of queue_mix_block.  With sounds (QueueSound objects from the one in which the chain in progress started) and words
    (queue_plan's, moved by queue_advance): a queue, frames the block's output frames it reaches.  Without: a source as rh_wide_mix_block
    reads it (data, channels, from_rate, phase, last, gain)."""

    def __init__(self, frames, sounds=None, words=None, data=None, channels=0, from_rate=0, gain=1.0, phase=0, last=0xFFFFFFFF):
        self.data, self.channels, self.from_rate, self.phase, self.frames, self.last, self.gain = data, int(channels), int(from_rate), int(phase), int(frames), int(last), float(gain)
        self.sounds = list(sounds or [])
        self.words = [0] * QUEUE_WORDS if words is None else [int(v) for v in words]
        if len(self.words) != QUEUE_WORDS:
            raise ValueError(f"QueueSrc: a cursor travels as {QUEUE_WORDS} words, got {len(self.words)}")


def queue_mix_block(dst, channels, to_rate, out_frames, srcs):
    """rh_queue_mix_block: a block of a mixer whose sources may be queues of resident sounds played back to back (what Player::append
    feeds its mixer): the converter chain by chain as rodio cuts it across the sounds, each tap behind its sound's gain, the channel rule
    and the ordered sum, one launch for any number of sources.  dst: a float32 device tensor of out_frames * channels elements (or a
    device address); srcs: QueueSrc objects in insertion order."""
    _ensure()
    n = len(srcs)
    arr = (_lib.WideSrc * max(n, 1))()
    counts, cursors = (C.c_uint32 * max(n, 1))(), (C.c_uint64 * (QUEUE_WORDS * max(n, 1)))()
    for k, s in enumerate(srcs):
        arr[k].data = s.data if isinstance(s.data, int) or s.data is None else s.data.data_ptr()
        arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = s.channels, s.from_rate, s.phase, s.frames, s.last, s.gain
        counts[k] = len(s.sounds)
        cursors[QUEUE_WORDS * k:QUEUE_WORDS * (k + 1)] = s.words
    words, gains = _queue_sounds([q for s in srcs for q in s.sounds])
    check(lib.rh_queue_mix_block(C.c_void_p(dst) if isinstance(dst, int) else _ptr(dst), channels, to_rate, out_frames, arr, n, words, gains, counts, cursors, _stream()),
          "rh_queue_mix_block")
    return dst


CLIP_WORDS = 7  # RH_CLIP_WORDS: kind, Z, N, take_ns, flags, done, total
CLIP_PLAIN, CLIP_RULE_G, CLIP_RULE_C = 0, 1, 2
CLIP_TAKE, CLIP_FADE_OUT = 1, 2


def clip_plan(n_samples, channels, rate, span_len=0, delay_ns=0, take_ns=None, fade_out=False):
    """rh_clip_plan: the words [kind, Z, N, take_ns, flags, done, total] of sound.take_duration(take_ns)[.set_filter_fadeout()].delay(delay_ns)
    over a sound of n_samples samples behind its in-point; span_len = what the sound answers to current_span_len() (0: None; n_samples: a
    SamplesBuffer); take_ns None: no take.  The cursor starts at 0; `total` is clip_advance's to write.  Host arithmetic: no device is touched."""
    w = (C.c_uint64 * CLIP_WORDS)()
    flags = (CLIP_TAKE if take_ns is not None else 0) | (CLIP_FADE_OUT if fade_out else 0)
    check(lib.rh_clip_plan(w, n_samples, channels, rate, span_len, delay_ns, take_ns or 0, flags), "rh_clip_plan")
    return list(w)


def clip_advance(words, channels, from_rate, to_rate, out_frames):
    """rh_clip_advance: the words of a clip behind a block of out_frames output frames (a new list; the cursor stops at the clip's end, words
    of a plain source come back as they are), with the clip's output frames at these rates in the last word: out_frames = 0 behind
    clip_plan states them.  Any cut of a stream into blocks gives the bits of one pass."""
    w = (C.c_uint64 * CLIP_WORDS)(*[int(v) for v in words])
    check(lib.rh_clip_advance(w, channels, from_rate, to_rate, out_frames), "rh_clip_advance")
    return list(w)


class ClipSrc:
    """One source of clip_mix_block.  With words (clip_plan's, moved by clip_advance): a clip -- data is sample 0 of the resident sound behind
    its in-point (a float32 device tensor or a device address), frames the block's output frames it reaches; phase and last are not read.
    Without: a source as rh_wide_mix_block reads it."""

    def __init__(self, data, channels, from_rate, frames, gain=1.0, words=None, phase=0, last=0xFFFFFFFF):
        self.data, self.channels, self.from_rate, self.phase, self.frames, self.last, self.gain = data, int(channels), int(from_rate), int(phase), int(frames), int(last), float(gain)
        self.words = [0] * CLIP_WORDS if words is None else [int(v) for v in words]
        if len(self.words) != CLIP_WORDS:
            raise ValueError(f"ClipSrc: a clip travels as {CLIP_WORDS} words, got {len(self.words)}")


def clip_mix_block(dst, channels, to_rate, out_frames, srcs):
    """rh_clip_mix_block: a block of a mixer whose sources may be clips on a timeline (a resident sound behind delay, take_duration and its
    fade-out): the delay's zeros, the gain, the fade, the converter chain by chain as rodio cuts the delayed stream, the channel rule and
    the ordered sum, one launch per 32 sources.  dst: a float32 device tensor of out_frames * channels elements (or a device address);
    srcs: ClipSrc objects in insertion order."""
    _ensure()
    n = len(srcs)
    arr = (_lib.WideSrc * max(n, 1))()
    words = (C.c_uint64 * (CLIP_WORDS * max(n, 1)))()
    for k, s in enumerate(srcs):
        arr[k].data = s.data if isinstance(s.data, int) or s.data is None else s.data.data_ptr()
        arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = s.channels, s.from_rate, s.phase, s.frames, s.last, s.gain
        words[CLIP_WORDS * k:CLIP_WORDS * (k + 1)] = s.words
    check(lib.rh_clip_mix_block(C.c_void_p(dst) if isinstance(dst, int) else _ptr(dst), channels, to_rate, out_frames, arr, n, words, _stream()), "rh_clip_mix_block")
    return dst


def wide_mix_batch(dsts, channels, to_rates, out_frames, srcs):
    """rh_wide_mix_batch: the current block of many mixers of any channel count in ONE launch; every mixer gets the bits rh_wide_mix_block
    writes for it.  dsts: per mixer a float32 device tensor of out_frames * channels elements, a device address, or None (out_frames == 0);
    channels, to_rates, out_frames: per mixer; srcs: per mixer a sequence of `_lib.WideSrc` in insertion order (a ctypes array or a list)."""
    _ensure()
    n = len(dsts)
    if not (len(channels) == len(to_rates) == len(out_frames) == len(srcs) == n):
        raise ValueError("wide_mix_batch: dsts, channels, to_rates, out_frames and srcs must have one entry per mixer")
    d = (C.c_void_p * max(n, 1))(*[x if isinstance(x, int) or x is None else x.data_ptr() for x in dsts])
    ch, rates = (C.c_uint32 * max(n, 1))(*map(int, channels)), (C.c_uint32 * max(n, 1))(*map(int, to_rates))
    frames, counts = (C.c_uint64 * max(n, 1))(*map(int, out_frames)), (C.c_uint32 * max(n, 1))(*[len(s) for s in srcs])
    total = sum(len(s) for s in srcs)
    table = (_lib.WideSrc * max(total, 1))()
    at = 0
    for s in srcs:  # all mixers' sources back to back
        for x in s:
            C.memmove(C.byref(table, at * C.sizeof(_lib.WideSrc)), C.byref(x), C.sizeof(_lib.WideSrc))
            at += 1
    check(lib.rh_wide_mix_batch(d, ch, rates, frames, counts, n, table, _stream()), "rh_wide_mix_batch")
    return dsts


def delay_samples(ns, rate, ch) -> int:
    return int(lib.rh_delay_samples(ns, rate, ch))


# ---- mixer ---------------------------------------------------------------------------------
class Mixer:
    """`let (tx, rx) = mixer::mixer(channels, rate)` as one object (src/mixer.rs:25-43).

    add() converts the source with UniformSourceIterator (mixer.rs:58-66) and admits it at the
    next frame boundary of the output position (mixer.rs:175-183); next()/pull() serve the
    ordered sum (mixer.rs:185-198) computed by rh_mix_sum."""

    def __init__(self, channels: int, sample_rate: int):
        self._channels, self._rate = int(channels), int(sample_rate)
        self._srcs: list[tuple[GpuSource, int]] = []
        self._pos = 0
        self._mixed = None

    def channels(self):
        return self._channels

    def sample_rate(self):
        return self._rate

    def add(self, src: GpuSource):
        u = UniformSourceIterator(src, self._channels, self._rate)
        start = -(-self._pos // self._channels) * self._channels  # next frame boundary
        self._srcs.append((u, start))
        self._mixed = None

    def _mix(self):
        if self._mixed is None:
            _ensure()
            n = len(self._srcs)
            out_len = max((st + len(u) for u, st in self._srcs), default=0)
            out = _dev_empty(out_len)
            if out_len:
                ptrs = (C.c_void_p * n)(*[u.samples.data_ptr() if len(u) else None for u, _ in self._srcs])
                starts = (C.c_uint64 * n)(*[st for _, st in self._srcs])
                lens = (C.c_uint64 * n)(*[len(u) for u, _ in self._srcs])
                check(lib.rh_mix_sum(_ptr(out), out_len, ptrs, starts, lens, n, _stream()), "rh_mix_sum")
            _t().cuda.current_stream().synchronize()
            self._mixed = out.cpu().numpy()
        return self._mixed

    def pull(self, n: int) -> np.ndarray:
        m = self._mix()
        out = m[self._pos: self._pos + n].copy()
        self._pos += len(out)
        return out

    def next(self):
        """MixerSource::next (mixer.rs:120-136): the channel position advances on EVERY call, also on the ones that return None
        (an empty mixer); a source added meanwhile starts at the next frame boundary, so an odd number of None calls is
        followed by one more None before its first sample."""
        m = self._mix()
        p = self._pos
        self._pos += 1
        if any(st <= p < st + len(u) for u, st in self._srcs):
            return float(m[p])
        return None

    def collect(self) -> np.ndarray:
        return self.pull(1 << 62)


# ---- block streaming -----------------------------------------------------------------------------
class StreamingResampler:
    """SampleRateConverter over a stream that arrives in blocks (rh_resampler_*): feed(block) returns the
    output frames that became computable; feed(block, flush=True) ends the stream (rodio's None)."""

    def __init__(self, from_rate, to_rate, channels):
        _ensure()
        self._h = C.c_void_p()
        self.channels = channels
        check(lib.rh_resampler_create(C.byref(self._h), from_rate, to_rate, channels), "rh_resampler_create")

    def feed(self, block, flush=False):
        frames = block.numel() // self.channels
        n = C.c_uint64(0)
        check(lib.rh_resampler_pending_frames(self._h, frames, int(flush), C.byref(n)), "rh_resampler_pending_frames")
        out = _dev_empty(max(n.value * self.channels, 1))
        m = C.c_uint64(0)
        check(lib.rh_resampler_process(self._h, _ptr(out), n.value, _ptr(block) if frames else None, frames, int(flush),
                                       C.byref(m), _stream()), "rh_resampler_process")
        return out[: m.value * self.channels]

    def close(self):
        if self._h:
            lib.rh_resampler_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class StreamingReverb:
    """reverb(duration, amplitude) over a stream that arrives in blocks (rh_echo_*)."""

    def __init__(self, duration_ns, amplitude, sample_rate, channels):
        _ensure()
        self.delay = delay_samples(duration_ns, sample_rate, channels)
        self._h = C.c_void_p()
        check(lib.rh_echo_create(C.byref(self._h), self.delay, amplitude), "rh_echo_create")

    def feed(self, block):
        out = _dev_empty(max(block.numel(), 1))
        check(lib.rh_echo_process(self._h, _ptr(out), _ptr(block) if block.numel() else None, block.numel(), _stream()), "rh_echo_process")
        return out[: block.numel()]

    def flush(self):
        out = _dev_empty(max(self.delay, 1))
        check(lib.rh_echo_flush(self._h, _ptr(out), _stream()), "rh_echo_flush")
        return out[: self.delay]

    def close(self):
        if self._h:
            lib.rh_echo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- fused headline pipeline ------------------------------------------------------------------
class ResampleLowpassMix:
    """BASELINE config 2 as one kernel: for every source
    `mixer.add(UniformSourceIterator::new(src, ch, to_rate).low_pass(freq))`, then the mixer sum.

    Sources are device tensors ([frames, 2] or flat interleaved f32).  `span_len` = the sources'
    current_span_len() (None/0 = continuous)."""

    def __init__(self, from_rate, to_rate, channels=2, span_len=None, filter="low_pass", freq=200, q=0.5,
                 max_sources=256, max_in_frames=1 << 20, frames_per_lane=0, ring_stages=0, no_balance=0, force_general=0, filter_first=False):
        _ensure()
        kind = {"low_pass": 0, "high_pass": 1, None: -1, "none": -1}[filter]
        self.cfg = RlmConfig(from_rate, to_rate, channels, int(span_len or 0), kind, freq, q, max_sources,
                             max_in_frames, frames_per_lane, ring_stages, no_balance, force_general)
        self.cfg.filter_first = 1 if filter_first else 0  # `mixer.add(src.low_pass(f))`: filter at from_rate, then convert (rodio_hip.h)
        self._h = C.c_void_p()
        check(lib.rh_rlm_create(C.byref(self._h), C.byref(self.cfg)), "rh_rlm_create")
        self.channels = channels
        self._keep = None
        self._keep_prev = None
        self.out_frames = 0

    def geometry(self):
        g = RlmGeometry()
        check(lib.rh_rlm_geometry(self._h, C.byref(g)), "rh_rlm_geometry")
        return {n: getattr(g, n) for n, _ in RlmGeometry._fields_}

    def set_sources(self, tensors):
        """Device tensors of interleaved samples, all torch.float32 or all torch.int16 (16-bit PCM as it lies in a WAV data chunk:
        rh_rlm_set_sources_pcm16 -- the same bits as converting first; source_format() tells whether a run read the PCM itself)."""
        n = len(tensors)
        kinds = {str(t.dtype) for t in tensors}
        if not kinds <= {"torch.float32", "torch.int16"}:
            raise ValueError(f"set_sources takes float32 or int16 tensors, not {sorted(kinds)}")
        if len(kinds) > 1:
            raise ValueError("set_sources takes sources of one dtype: all float32 or all int16")
        pcm16 = kinds == {"torch.int16"}
        self._keep = list(tensors)
        ptrs = (C.c_void_p * n)(*[t.data_ptr() if t.numel() else None for t in tensors])
        frames = (C.c_uint64 * n)(*[t.numel() // self.channels for t in tensors])
        if pcm16:
            check(lib.rh_rlm_set_sources_pcm16(self._h, ptrs, frames, n), "rh_rlm_set_sources_pcm16")
        else:
            check(lib.rh_rlm_set_sources(self._h, ptrs, frames, n), "rh_rlm_set_sources")
        # run() reports out_frames too; it is needed here to size the output allocation
        mx = 0
        for t in tensors:
            o = C.c_uint64(0)
            check(lib.rh_resample_out_frames(t.numel() // self.channels, self.cfg.from_rate, self.cfg.to_rate,
                                             self.channels, self.cfg.span_len, C.byref(o)), "rh_resample_out_frames")
            mx = max(mx, o.value)
        self.out_frames = mx

    def source_format(self):
        """{"format": 0 f32 rows / 1 PCM16 rows, "native": 1 = the last one-shot run read the PCM16 rows themselves}."""
        f, nat = C.c_int32(0), C.c_int32(0)
        check(lib.rh_rlm_source_format(self._h, C.byref(f), C.byref(nat)), "rh_rlm_source_format")
        return {"format": f.value, "native": nat.value}

    def run(self, out=None):
        """Enqueue one pass on the current stream; returns the mixed [out_frames*channels] tensor."""
        if out is None:
            out = _dev_empty(max(self.out_frames * self.channels, 4))
        m = C.c_uint64(0)
        check(lib.rh_rlm_run(self._h, _ptr(out), out.numel() // self.channels, C.byref(m), _stream()), "rh_rlm_run")
        return out[: m.value * self.channels]

    def set_gains(self, gains):
        """Per-source Amplify factors (`src.amplify(g)` / Player::set_volume): folded into the fused kernel."""
        g = np.ascontiguousarray(gains, dtype=np.float32)
        check(lib.rh_rlm_set_gains(self._h, g.ctypes.data_as(_lib.f32p), g.size), "rh_rlm_set_gains")

    def set_filters(self, filters):
        """A filter per source, rodio's `mixer.add(a.low_pass(200)); mixer.add(b.high_pass(300)); mixer.add(c)`: a list of
        ("low_pass" | "high_pass" | None, freq[, q = 0.5]) entries, one per source; [] returns to the handle's one filter.
        Before set_sources()."""
        n = len(filters)
        kinds = (C.c_int32 * max(n, 1))()
        freqs = (C.c_uint32 * max(n, 1))()
        qs = (C.c_float * max(n, 1))()
        for i, f in enumerate(filters):
            kind = f[0] if f is not None else None
            kinds[i] = {"low_pass": 0, "high_pass": 1, None: -1, "none": -1}[kind]
            freqs[i] = int(f[1]) if kind not in (None, "none") else 0
            qs[i] = float(f[2]) if (kind not in (None, "none") and len(f) > 2) else 0.5
        check(lib.rh_rlm_set_filters(self._h, kinds, freqs, C.cast(qs, _lib.f32p), n), "rh_rlm_set_filters")

    def set_exclusive(self, exclusive=True):
        """False: other work shares the CUs while this handle runs (a collective on a second stream, copy launches): tiles by
        ticket instead of by workgroup index (rodio_hip.h)."""
        check(lib.rh_rlm_set_exclusive(self._h, 1 if exclusive else 0), "rh_rlm_set_exclusive")

    def set_mix_first(self, enable=True):
        """False: every source goes through the converter and the filter on its own (the general path)."""
        check(lib.rh_rlm_set_mix_first(self._h, 1 if enable else 0), "rh_rlm_set_mix_first")

    def run_subset(self, first, count, out=None):
        """Mix of the sources [first, first+count) only."""
        if out is None:
            out = _dev_empty(max(self.out_frames * self.channels, 4))
        m = C.c_uint64(0)
        check(lib.rh_rlm_run_subset(self._h, first, count, _ptr(out), out.numel() // self.channels, C.byref(m), _stream()), "rh_rlm_run_subset")
        return out[: m.value * self.channels]

    # -- block streaming: feed(blocks) returns the mixed frames that became computable ------------------
    def stream_begin(self, keep_history=False):
        """keep_history: stream_feed_v() may run on the summed state while its sources run together (rh_rlm_stream_keep_history): the
        mirror then keeps the rows of the block before alive, as the recovery needs them."""
        check(lib.rh_rlm_stream_begin(self._h), "rh_rlm_stream_begin")
        check(lib.rh_rlm_stream_keep_history(self._h, 1 if keep_history else 0), "rh_rlm_stream_keep_history")
        self._left = None
        self._keep_prev = None

    def stream_stats(self):
        """(blocks on the summed state, blocks with one state per source, recoveries) of the current stream."""
        a, b, c = C.c_uint32(0), C.c_uint32(0), C.c_uint32(0)
        check(lib.rh_rlm_stream_stats(self._h, C.byref(a), C.byref(b), C.byref(c)), "rh_rlm_stream_stats")
        return a.value, b.value, c.value

    def stream_feed(self, blocks, flush=False):
        """blocks: one device tensor of NEW interleaved samples per source (equal lengths).  The unconsumed
        tail of the previous call is kept here, as a Rust shim would keep it in its own buffers."""
        torch = _t()
        ch = self.channels
        bufs = list(blocks) if self._left is None else [torch.cat([l, b]) for l, b in zip(self._left, blocks)]
        n = len(bufs)
        avail = bufs[0].numel() // ch
        ptrs = (C.c_void_p * n)(*[b.data_ptr() if b.numel() else 0 for b in bufs])
        cap = int(avail * (self.cfg.to_rate / self.cfg.from_rate + 1)) + 64
        out = _dev_empty(max(cap * ch, 4))
        m, c = C.c_uint64(0), C.c_uint64(0)
        check(lib.rh_rlm_stream_block(self._h, ptrs, n, avail, int(flush), _ptr(out), cap, C.byref(m), C.byref(c), _stream()),
              "rh_rlm_stream_block")
        self._keep = bufs  # the launch reads them asynchronously
        self._left = [b[c.value * ch:].clone() for b in bufs]
        return out[: m.value * ch]

    def stream_feed_v(self, blocks, ended):
        """Per-source states: blocks[s] = NEW interleaved samples of source s (any length, also empty), ended[s] = it
        will deliver no more.  Returns the mixed frames this block could emit (whole tiles until all have ended)."""
        torch = _t()
        ch = self.channels
        bufs = list(blocks) if self._left is None else [torch.cat([l, b]) if b.numel() else l for l, b in zip(self._left, blocks)]
        n = len(bufs)
        avail = (C.c_uint64 * n)(*[b.numel() // ch for b in bufs])
        end = (C.c_uint8 * n)(*[1 if e else 0 for e in ended])
        ptrs = (C.c_void_p * n)(*[b.data_ptr() if b.numel() else 0 for b in bufs])
        cap = int(max(avail) * (self.cfg.to_rate / self.cfg.from_rate + 1)) + 64
        out = _dev_empty(max(cap * ch, 4))
        m, c = C.c_uint64(0), C.c_uint64(0)
        check(lib.rh_rlm_stream_block_v(self._h, ptrs, avail, end, n, _ptr(out), cap, C.byref(m), C.byref(c), _stream()), "rh_rlm_stream_block_v")
        self._keep_prev = self._keep  # (keep_history: the next call may replay the end of this block's rows)
        self._keep = bufs  # the launch reads them asynchronously
        self._left = [b[min(c.value * ch, b.numel()):].clone() for b in bufs]
        return out[: m.value * ch]

    def run_batch(self):
        """No mixing: returns [S, out_frames*channels], row s = UniformSourceIterator(src_s).low_pass(...)."""
        torch = _t()
        S = len(self._keep)
        stride = (self.out_frames + 1) // 2 * 2
        out = torch.empty((S, stride * self.channels), device="cuda", dtype=torch.float32)
        m = C.c_uint64(0)
        check(lib.rh_rlm_run_batch(self._h, _ptr(out), stride, C.byref(m), _stream()), "rh_rlm_run_batch")
        return out[:, : m.value * self.channels]

    def autotune(self, out=None):
        """Time the candidate geometries on the current sources and keep the fastest (synchronises)."""
        if out is None:
            out = _dev_empty(max(self.out_frames * self.channels, 4))
        r, ns = C.c_uint32(0), C.c_uint32(0)
        check(lib.rh_rlm_autotune(self._h, _ptr(out), out.numel() // self.channels, _stream(), C.byref(r), C.byref(ns)), "rh_rlm_autotune")
        return r.value, ns.value

    def phase_cycles(self):
        out = (C.c_double * 8)()
        st = lib.rh_rlm_phase_cycles(self._h, out)
        return None if st != 0 else list(out)

    def late_carries(self):
        n = C.c_uint64(0)
        check(lib.rh_rlm_late_carries(self._h, C.byref(n)), "rh_rlm_late_carries")
        return n.value

    def check_status(self):
        _t().cuda.current_stream().synchronize()
        check(lib.rh_rlm_last_status(self._h), "rh_rlm_last_status")

    def close(self):
        if self._h:
            lib.rh_rlm_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---- parameters that change while a source plays (periodic.rs, amplify.rs:27-35, channel_volume.rs:71-88) ----------
def periodic_update_samples(period_ns: int, sample_rate: int, channels: int) -> int:
    """U of PeriodicAccess (periodic.rs:14-22): the closure runs before sample 0, U, 2U, ... -- samples, not frames."""
    return int(lib.rh_periodic_update_samples(int(period_ns), int(sample_rate), int(channels)))


def _table(values):
    torch = _t()
    if isinstance(values, torch.Tensor):
        return values.to(device="cuda", dtype=torch.float32).contiguous()
    return torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32).ravel()).to("cuda")


def amplify_steps(x, first: int, period: int, factors, out=None):
    """rh_amplify_steps over the 1-D device tensor x: x[i] * factors[(first + i) // period - first // period].  `out` may be x
    (in place) or any float32 view of the right length."""
    _ensure()
    f = _table(factors)
    if out is None:
        out = _dev_empty(x.numel())
    check(lib.rh_amplify_steps(_ptr(out), _ptr(x), x.numel(), int(first), int(period), _ptr(f), f.numel(), _stream()), "rh_amplify_steps")
    return out


def channel_volume_steps(x, in_ch: int, out_ch: int, first: int, gain_period: int, gains, factor_first: int = 0, factor_period: int = 1,
                         factors=None, out=None):
    """rh_channel_volume_steps over the interleaved device tensor x (whole frames of in_ch): gains is [steps, out_ch]; output
    sample j takes gains[step_g(j)][j % out_ch] and, with `factors`, then * factors[step_f(j)]."""
    _ensure()
    frames = x.numel() // in_ch
    g = _table(gains)
    f = _table(factors) if factors is not None else None
    if out is None:
        out = _dev_empty(frames * out_ch)
    check(lib.rh_channel_volume_steps(_ptr(out), _ptr(x), frames, in_ch, out_ch, int(first), int(gain_period), _ptr(g), g.numel() // out_ch,
                                      int(factor_first), int(factor_period), _ptr(f) if f is not None else None, f.numel() if f is not None else 0,
                                      _stream()), "rh_channel_volume_steps")
    return out


# rh_biquad_steps mode 1 (k_biquad_steps_scan in csrc/rh_live.hip): frames a lane owns in a tile (kRun) and frames a tile
# (kScanBlock * kRun).  tests/test_live_filter_cpu.py holds the two against the kernel's source.
BIQUAD_STEPS_RUN = 8
BIQUAD_STEPS_TILE = 256 * BIQUAD_STEPS_RUN


def biquad_steps(x, channels: int, first: int, period: int, coeffs, n_streams: int = 1, state=None, mode: int = 0, out=None):
    """rh_biquad_steps over the device tensor x (n_streams rows of whole interleaved frames, back to back): sample i of a row is
    filtered with coeffs[(first + i) // period - first // period] ({b0,b1,b2,a1,a2} per entry).  coeffs: [steps, 5] shared by the
    rows, or [n_streams, steps, 5].  state: a float32 device tensor of n_streams * channels * 4 ({x1,x2,y1,y2} per channel),
    updated in place, or None.  mode 0: rodio's bits; mode 1: the f64 evaluation, time-parallel (rodio_hip.h).  `out` may be x."""
    _ensure()
    torch = _t()
    co = coeffs if isinstance(coeffs, torch.Tensor) else np.ascontiguousarray(coeffs, dtype=np.float32)
    if co.ndim == 3:
        assert co.shape[0] == n_streams and co.shape[2] == 5
        n_steps, stride = co.shape[1], co.shape[1] * 5
    else:
        assert co.ndim == 2 and co.shape[1] == 5
        n_steps, stride = co.shape[0], 0
    t = _table(co)
    frames = x.numel() // (channels * n_streams) if channels and n_streams else 0
    if out is None:
        out = _dev_empty(x.numel())
    check(lib.rh_biquad_steps(_ptr(out), _ptr(x), frames, int(channels), int(n_streams), int(first), int(period), _ptr(t), n_steps, stride,
                              _ptr(state) if state is not None else None, int(mode), _stream()), "rh_biquad_steps")
    return out


# ---- sources that start on the device: rodio's synthetic generators (rh_signal_generate / rh_chirp) -------------------------
GEN_FUNCTIONS = {"sine": 0, "triangle": 1, "square": 2, "sawtooth": 3}  # rodio's Function (signal_generator.rs:24-30), RH_GEN_*
DEFAULT_SAMPLE_RATE = 48000  # rodio::DEFAULT_SAMPLE_RATE
USIZE_MAX = (1 << 64) - 1


def _gen_function(f) -> int:
    code = GEN_FUNCTIONS.get(f, f) if isinstance(f, str) else int(f)
    if code not in GEN_FUNCTIONS.values():
        raise ValueError(f"unknown generator function {f!r}: one of {sorted(GEN_FUNCTIONS)}")
    return code


def _gen_state(sample_rate, frequency):
    st = (C.c_float * 2)()
    check(lib.rh_signal_generator_init(st, int(sample_rate), float(frequency)), "rh_signal_generator_init (frequency must be > 0)")
    return st[0], st[1]


class GeneratorBank:
    """G SignalGenerators whose state (phase_step, phase) lives in device memory.  take(n) fills a [G, n] device tensor, row g
    with generator g's next n samples, and moves every phase on: the next take continues the streams.  Nothing is uploaded."""

    def __init__(self, sample_rates, frequencies, functions):
        torch = _t()
        _ensure()
        g = len(frequencies)
        rates = [int(r) for r in (sample_rates if hasattr(sample_rates, "__len__") else [sample_rates] * g)]
        fns = [_gen_function(f) for f in (functions if isinstance(functions, (list, tuple)) else [functions] * g)]
        if not (len(rates) == len(fns) == g) or g == 0:
            raise ValueError("one sample rate, frequency and function per generator")
        self.rates, self.freqs, self.functions = rates, [float(np.float32(f)) for f in frequencies], fns
        st = [_gen_state(r, f) for r, f in zip(rates, self.freqs)]
        self.state = torch.tensor(np.asarray(st, np.float32).reshape(-1), device="cuda")
        self._fns = torch.tensor(fns, dtype=torch.int32, device="cuda")

    def __len__(self):
        return len(self.freqs)

    def take(self, n: int, out=None):
        torch = _t()
        g = len(self)
        if out is None:
            out = torch.empty((g, int(n)), dtype=torch.float32, device="cuda")
        if out.dim() != 2 or out.shape[0] != g or out.shape[1] < n or out.stride(1) != 1:
            raise ValueError("out must be [G, >= n] with contiguous rows")
        check(lib.rh_signal_generate(_ptr(out), out.stride(0), int(n), _ptr(self.state), _ptr(self._fns), g, _stream()), "rh_signal_generate")
        return out[:, : int(n)]

    def phases(self) -> np.ndarray:
        return self.state.view(-1, 2)[:, 1].cpu().numpy()

    def try_seek(self, pos_ns: int):
        """Every generator's try_seek(pos) (signal_generator.rs:148-153)."""
        ph = (C.c_float * 1)()
        new = np.empty(len(self), np.float32)
        for k, (r, f) in enumerate(zip(self.rates, self.freqs)):
            check(lib.rh_signal_generator_seek(ph, r, f, int(pos_ns)), "rh_signal_generator_seek")
            new[k] = ph[0]
        self.state.view(-1, 2)[:, 1].copy_(_t().from_numpy(new).cuda())


class SignalGenerator:
    """rodio's SignalGenerator::new(sample_rate, frequency, Function) on the device: take(n) returns its next n samples as a
    device tensor (source(n): as a mono GpuSource).  Mono, endless: size_hint (usize::MAX, None), no span length, no total
    duration.  frequency <= 0 or NaN raises RhError (rodio panics)."""

    def __init__(self, sample_rate: int, frequency: float, function="sine"):
        self._bank = GeneratorBank([sample_rate], [frequency], [function])

    def channels(self) -> int:
        return 1

    def sample_rate(self) -> int:
        return self._bank.rates[0]

    def current_span_len(self):
        return None

    def total_duration(self):
        return None

    def size_hint(self):
        return (USIZE_MAX, None)

    def phase(self) -> float:
        return float(self._bank.phases()[0])

    def take(self, n: int):
        return self._bank.take(n)[0]

    def source(self, n: int) -> GpuSource:
        return GpuSource(self.take(n), 1, self.sample_rate())

    def try_seek(self, pos_ns: int):
        self._bank.try_seek(pos_ns)


def SineWave(frequency: float) -> SignalGenerator:  # sine.rs: SignalGenerator at DEFAULT_SAMPLE_RATE
    return SignalGenerator(DEFAULT_SAMPLE_RATE, frequency, "sine")


def SquareWave(frequency: float) -> SignalGenerator:
    return SignalGenerator(DEFAULT_SAMPLE_RATE, frequency, "square")


def TriangleWave(frequency: float) -> SignalGenerator:
    return SignalGenerator(DEFAULT_SAMPLE_RATE, frequency, "triangle")


def SawtoothWave(frequency: float) -> SignalGenerator:
    return SignalGenerator(DEFAULT_SAMPLE_RATE, frequency, "sawtooth")


def signal_phase_advance(phase: float, phase_step: float, n: int) -> float:
    """rh_signal_phase_advance (host): the phase n samples on, bit for bit n steps of rodio's recurrence."""
    return float(np.float32(lib.rh_signal_phase_advance(float(phase), float(phase_step), int(n))))


class Chirp:
    """rodio's chirp(sample_rate, start_frequency, end_frequency, duration) on the device (chirp.rs).  take(n) returns the next
    min(n, remaining) samples; try_seek takes any u64 sample position."""

    def __init__(self, sample_rate: int, start_frequency: float, end_frequency: float, duration_ns: int):
        _ensure()
        t = C.c_uint64(0)
        check(lib.rh_chirp_total_samples(int(sample_rate), int(duration_ns), C.byref(t)), "rh_chirp_total_samples")
        self._rate, self.f0, self.f1 = int(sample_rate), float(np.float32(start_frequency)), float(np.float32(end_frequency))
        self.total_samples, self.elapsed_samples = t.value, 0

    def channels(self) -> int:
        return 1

    def sample_rate(self) -> int:
        return self._rate

    def current_span_len(self):
        return None

    def size_hint(self):
        r = self.total_samples - self.elapsed_samples
        return (r, r)

    def total_duration(self) -> int:
        """Duration::from_secs_f64(total / rate), in nanoseconds."""
        s, ns = C.c_uint64(0), C.c_uint32(0)
        check(lib.rh_chirp_total_duration(self._rate, self.total_samples, C.byref(s), C.byref(ns)), "rh_chirp_total_duration")
        return s.value * 1_000_000_000 + ns.value

    def try_seek(self, pos_ns: int):
        t = C.c_uint64(0)  # (pos.as_secs_f64() * rate as f64) as u64: the same formula as the total
        check(lib.rh_chirp_total_samples(self._rate, int(pos_ns), C.byref(t)), "rh_chirp_total_samples")
        self.elapsed_samples = min(t.value, self.total_samples)

    def seek_sample(self, i: int):
        self.elapsed_samples = min(int(i), self.total_samples)

    def take(self, n: int):
        out = _dev_empty(max(int(n), 1))
        m = C.c_uint64(0)
        check(lib.rh_chirp(_ptr(out), self.elapsed_samples, int(n), self.total_samples, self._rate, self.f0, self.f1, C.byref(m), _stream()), "rh_chirp")
        self.elapsed_samples += m.value
        return out[: m.value]

    def source(self, n: int) -> GpuSource:
        return GpuSource(self.take(n), 1, self._rate)


def chirp(sample_rate: int, start_frequency: float, end_frequency: float, duration_ns: int) -> Chirp:
    return Chirp(sample_rate, start_frequency, end_frequency, duration_ns)


# ---- noise sources that start on the device: rodio's noise.rs (rh_noise_init / rh_noise_generate) -------------------------------
NOISE_KINDS = {"white_uniform": 0, "white_triangular": 1, "white_gaussian": 2, "pink": 3, "blue": 4, "violet": 5, "brownian": 6, "red": 7, "velvet": 8}
VELVET_DEFAULT_DENSITY = 2000  # noise.rs:434
_INTEGRATORS = (NOISE_KINDS["brownian"], NOISE_KINDS["red"])


def _noise_kind(k) -> int:
    code = NOISE_KINDS.get(k.lower(), k) if isinstance(k, str) else int(k)
    if code not in NOISE_KINDS.values():
        raise ValueError(f"unknown noise kind {k!r}: one of {sorted(NOISE_KINDS)}")
    return code


def entropy_seed() -> int:
    """A u64 from the OS entropy source: what new(rate) seeds with, where rodio calls rand::make_rng()."""
    import os

    return int.from_bytes(os.urandom(8), "little")


def noise_state(kind, sample_rate: int, seed: int, density: int = VELVET_DEFAULT_DENSITY) -> np.ndarray:
    """rh_noise_init: the eight u32 state words of a new stream (rodio_hip.h).  Unknown kind, rate 0, density 0: RhError."""
    st = (C.c_uint32 * 8)()
    check(lib.rh_noise_init(st, _noise_kind(kind), int(sample_rate), int(seed) & ((1 << 64) - 1), int(density)),
          "rh_noise_init (unknown kind, sample rate 0 or velvet density 0)")
    return np.frombuffer(st, dtype=np.uint32).copy()


class NoiseBank:
    """G noise streams of any kinds whose state (rodio_hip.h's eight words each) lives in device memory.  take(n) fills a [G, n] device
    tensor, row g with stream g's next n samples, and moves every stream on (k, and an integrator's acc): the next take continues
    them.  Nothing is uploaded.  seeds None: one from the OS entropy source per stream."""

    def __init__(self, kinds, sample_rates, seeds=None, densities=None):
        torch = _t()
        _ensure()
        kinds = list(kinds) if isinstance(kinds, (list, tuple)) else [kinds]
        g = len(kinds)
        rates = [int(r) for r in (sample_rates if hasattr(sample_rates, "__len__") else [sample_rates] * g)]
        seeds = [entropy_seed() for _ in range(g)] if seeds is None else [int(s) for s in (seeds if hasattr(seeds, "__len__") else [seeds] * g)]
        dens = [VELVET_DEFAULT_DENSITY] * g if densities is None else [int(d) for d in (densities if hasattr(densities, "__len__") else [densities] * g)]
        if not (len(rates) == len(seeds) == len(dens) == g) or g == 0:
            raise ValueError("one kind, sample rate, seed (and density) per stream")
        self.kinds = [_noise_kind(k) for k in kinds]
        self.rates, self.seeds, self.densities = rates, seeds, dens
        st = np.concatenate([noise_state(k, r, s, d) for k, r, s, d in zip(self.kinds, rates, seeds, dens)])
        self.state = torch.from_numpy(st.view(np.int32)).cuda()

    def __len__(self):
        return len(self.kinds)

    def take(self, n: int, out=None):
        torch = _t()
        g = len(self)
        if out is None:
            out = torch.empty((g, max(int(n), 1)), dtype=torch.float32, device="cuda")
        if out.dim() != 2 or out.shape[0] != g or out.shape[1] < n or out.stride(1) != 1 or out.dtype != torch.float32:
            raise ValueError("out must be a float32 [G, >= n] with contiguous rows")
        check(lib.rh_noise_generate(_ptr(out), out.stride(0), int(n), _ptr(self.state), g, _stream()), "rh_noise_generate")
        return out[:, : int(n)]

    def states(self) -> np.ndarray:
        """[G, 8] u32: the streams' state words as the device holds them."""
        return self.state.view(-1, 8).cpu().numpy().view(np.uint32)

    def positions(self) -> np.ndarray:
        s = self.states().astype(np.uint64)
        return s[:, 2] | (s[:, 3] << np.uint64(32))

    def try_seek(self, pos_ns: int = 0):
        """Every stream's try_seek(pos): Ok, and nothing moves but an integrator's acc, which goes to 0 (noise.rs:795-799, 875-879)."""
        torch = _t()
        rows = [g for g, k in enumerate(self.kinds) if k in _INTEGRATORS]
        if rows:
            self.state.view(-1, 8)[torch.tensor(rows, device="cuda"), 7] = 0


class NoiseSource:
    """One of rodio's noise sources on the device (noise.rs): take(n) returns its next n samples as a device tensor (source(n): as a
    mono GpuSource).  Mono, endless: size_hint (usize::MAX, None), no span length, no total duration.  seed None: from the OS
    entropy source (rodio's new); new_with_seed(rate, seed) is the reproducible form."""

    KIND = None

    def __init__(self, sample_rate: int, seed=None, density: int = VELVET_DEFAULT_DENSITY, kind=None):
        kind = self.KIND if kind is None else kind
        self._bank = NoiseBank([kind], [sample_rate], None if seed is None else [seed], [density])

    @classmethod
    def new(cls, sample_rate: int):
        return cls(sample_rate)

    @classmethod
    def new_with_seed(cls, sample_rate: int, seed: int):
        return cls(sample_rate, seed)

    @property
    def seed(self) -> int:
        return self._bank.seeds[0]

    def channels(self) -> int:
        return 1

    def sample_rate(self) -> int:
        return self._bank.rates[0]

    def current_span_len(self):
        return None

    def total_duration(self):
        return None

    def size_hint(self):
        return (USIZE_MAX, None)

    def position(self) -> int:
        return int(self._bank.positions()[0])

    def take(self, n: int):
        return self._bank.take(n)[0]

    def source(self, n: int) -> GpuSource:
        return GpuSource(self.take(n), 1, self.sample_rate())

    def try_seek(self, pos_ns: int = 0):
        self._bank.try_seek(pos_ns)


class WhiteUniform(NoiseSource):
    """Uniform in [-1, 1) (noise.rs:142-170)."""
    KIND = "white_uniform"

    def std_dev(self) -> float:
        return float(np.sqrt(np.float32(1.0) / np.float32(3.0)))


class WhiteTriangular(NoiseSource):
    """Triangular in (-1, 1), mode 0 (noise.rs:203-230)."""
    KIND = "white_triangular"

    def std_dev(self) -> float:
        return float(np.float32(2.0) / np.sqrt(np.float32(6.0)))


class WhiteGaussian(NoiseSource):
    """Normal, mean 0, sigma 0.6 (noise.rs:383-412): rh_dither's GPDF noise."""
    KIND = "white_gaussian"

    def mean(self) -> float:
        return 0.0

    def std_dev(self) -> float:
        return float(np.float32(0.6))


class Pink(NoiseSource):
    """Voss-McCartney over 16 generators (noise.rs:472-512)."""
    KIND = "pink"


class Blue(NoiseSource):
    """The first difference of white (noise.rs:570-583)."""
    KIND = "blue"


class Violet(NoiseSource):
    """The first difference of blue (noise.rs:638-651)."""
    KIND = "violet"


class Brownian(NoiseSource):
    """The leaky integral of WhiteGaussian (noise.rs:749-757); try_seek sets its accumulator to 0."""
    KIND = "brownian"


class Red(NoiseSource):
    """The leaky integral of WhiteUniform (noise.rs:832-840); try_seek sets its accumulator to 0."""
    KIND = "red"


class Velvet(NoiseSource):
    """One +-1 impulse per cell of ceil(rate / density) samples (noise.rs:282-330).  Density 0 raises RhError (rodio's NonZero)."""
    KIND = "velvet"

    def __init__(self, sample_rate: int, seed=None, density: int = VELVET_DEFAULT_DENSITY):
        super().__init__(sample_rate, seed, density)

    @classmethod
    def new_with_density(cls, sample_rate: int, density: int, seed=None):
        return cls(sample_rate, seed, density)


def white(sample_rate: int) -> WhiteUniform:
    """Deprecated as in rodio 0.21 (noise.rs:56-60): use WhiteUniform(rate)."""
    import warnings

    warnings.warn("white() is deprecated: use WhiteUniform(sample_rate)", DeprecationWarning, stacklevel=2)
    return WhiteUniform(sample_rate)


def pink(sample_rate: int) -> Pink:
    """Deprecated as in rodio 0.21 (noise.rs:62-66): use Pink(rate)."""
    import warnings

    warnings.warn("pink() is deprecated: use Pink(sample_rate)", DeprecationWarning, stacklevel=2)
    return Pink(sample_rate)
