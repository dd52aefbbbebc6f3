"""The one-row f32 entries in a hostile memory layout (tests/arena.py): rh_amplify, rh_distortion, rh_dither, rh_linear_gain_ramp, rh_delay,
rh_echo_mix, rh_take_duration(_from), rh_channels_convert, rh_channel_volume, rh_amplify_steps, rh_channel_volume_steps, rh_resample_linear,
rh_mix_sum, rh_mix_pair and rh_noise_generate.  Their kernels (rh::map4, rh::ld4_at, the tile kernels that park aligned vectors in LDS,
k_mix_sum_any) read 16-byte vectors that begin in front of the row and end behind it; here every source, step table and state lies between
NaN poison and every dst between NaN sentinels.  Every case asserts (a) the arena checks -- no store outside the row, nothing unwritten, the
sentinel intact behind a reported count, the sources unchanged; (b) the row against the reference of the entry's own parity test (the oracle,
or the numpy restatements of test_gpu_live.py / fallback_cases.py / test_mix_cpu.py / test_noise_cpu.py) at that test's tolerance: bit for
bit everywhere but rh_dither's GPDF (1e-7), the Gaussian noise (2e-6) and the noise integrators (4e-5); (c) the same bits as the same call
on rows in friendly surroundings (zeros) at the same leads.  Inputs are finite and include -0.0, values beyond +-1 and a subnormal, so a NaN
in an output is a finding.  Through the C ABI.

Sizes are the smallest that reach every path: n in SIZES (1027 = two workgroups of map4 plus a ragged vector, 4099 = where k_rlm_fast failed);
for a tile kernel two whole tiles plus 3 frames, and 1 and 7 frames, with the tile's frames derived as its launcher derives them."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

import arena
import fallback_cases as FC
from test_gpu_live import amplify_ref, channel_volume_ref
from test_mix_cpu import mix_rows
from test_noise_cpu import CODE, EXACT, GAUSS_TOL, INTEGRATOR_TOL, INTEGRATORS, KINDS, hash_, idx, integrator_consts, recurrence_f64, reference, u1

pytestmark = pytest.mark.gpu
f32 = np.float32

LEADS = [(0, 0), (1, 0), (0, 1), (3, 2), (2, 3), (1, 1), (3, 3)]  # (src, dst) in samples behind a 16-byte boundary
SIZES = [1, 3, 4, 5, 1027, 4099]
DITHER_TOL = 1e-7  # test_gpu_parity.py::test_dither_counter_based_noise: GPDF (logf / cosf differ in the last bit); the other three bit for bit


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _st():
    from rodio_amd import source

    return source._stream()


def L():
    from rodio_amd import _lib

    return _lib.lib


def vp(a):
    return C.c_void_p(a) if a is not None else None


def signal(seed, n, scale=1.5):
    """n finite samples beyond +-1, with -0.0, +0.0, a subnormal and values beyond +-2 spread over the row (as many as fit)."""
    x = np.random.default_rng(seed).uniform(-scale, scale, n).astype(f32)
    for k, v in enumerate([-0.0, 2.5, 1e-40, -3.25, 0.0]):
        if n > k:
            x[(k * n) // 5 if n >= 5 else k] = f32(v)
    assert np.all(np.isfinite(x))
    return x


def held(got, ref, tol=0.0):
    """got against the reference: the same bits, or for the entries held by a tolerance max |got - ref| <= tol (the reference in the
    precision it comes in), written so that a NaN fails"""
    got = np.asarray(got, f32).reshape(-1)
    ref = np.asarray(ref).reshape(-1)
    if got.shape != ref.shape:
        return False, f"{got.size} samples, the reference has {ref.size}"
    if tol:
        err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) if got.size else 0.0
        return err <= tol, err
    ref = ref.astype(f32)
    bad = np.flatnonzero(arena.bits(got) != arena.bits(ref))
    return bad.size == 0, (f"{bad.size} differ, the first at {int(bad[0])}: {got[bad[0]]!r} against {ref[bad[0]]!r}" if bad.size else "")


def plain_dst(n, lead):
    """a zeroed dst of n samples `lead` samples behind a 16-byte boundary, for the plain run"""
    t, p = arena.plain_dst(n + 4)
    return t, p + 4 * lead


def d2h(t, n, lead):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()[lead: lead + n].copy()


def one_row(call, x, out_len, ref, ls, ld, tag, tol=0.0, written=None, null_src=False):
    """call(dst, src) -> the count of samples the entry reports (None: all out_len).  x between poison `ls` samples behind a boundary, a dst
    arena of out_len words `ld` behind one; the three assertions of the module's docstring."""
    src = None if null_src else arena.src_arena(x, ls)
    dst = arena.dst_arena(out_len, ld)
    m = call(dst.ptr(), None if null_src else src.ptr())
    m = out_len if m is None else m
    assert written is None or m == written, (tag, m, written)
    got = dst.check(m)[:m]  # (a)
    if src is not None:
        src.unchanged()
    good, why = held(got, ref, tol)  # (b)
    assert good, (tag, ls, ld, why)
    if null_src:
        return got
    pt, pp = arena.plain(x, lead=ls)  # (c)
    dt, dp = plain_dst(out_len, ld)
    m2 = call(dp, pp)
    assert (out_len if m2 is None else m2) == m
    assert arena.same(d2h(dt, m, ld), got), (tag, ls, ld, "the arena run differs from the plain run")
    return got


def in_place(call, x, ref, lead, tag, tol=0.0):
    """dst == src: the signal between sentinels (map4 promises "works in place"); the same three assertions"""
    a = arena.inplace_arena(x, lead)
    call(a.ptr(), a.ptr())
    got = a.check()
    good, why = held(got, ref, tol)
    assert good, (tag, "in place", lead, why)
    pt, pp = arena.plain(x, lead=lead)
    call(pp, pp)
    import torch

    torch.cuda.synchronize()
    assert arena.same(pt.cpu().numpy()[arena.GUARD + lead: arena.GUARD + lead + x.size], got), (tag, "in place", lead)


def ok(status, tag):
    assert status == 0, (tag, status)


# ---- rh_amplify, rh_distortion, rh_dither, rh_linear_gain_ramp: rh::map4 and its hand-written twin --------------------------------------
# Routes (rows_vec_bits): src on a boundary -> one 16-byte load, else ld4_at's two aligned loads and a pick by residue (leads 1, 2, 3: every
# residue); dst on a boundary -> one 16-byte store, else four 4-byte stores; n % 4 != 0 -> the ragged last vector sample by sample (n = 1, 3,
# 5, 1027, 4099; n = 1 and 3 have nothing else); n = 1027 -> a second workgroup.
DITHER_K0, DITHER_CH = 7, 3  # sample_offset not a multiple of channels: HighPass looks `channels` samples back, across the block's start
RAMP_K0, RAMP_CH, RAMP_RATE = 5, 3, 48000  # the block starts on the last sample of frame 1


def _ramp_ns(n):
    """a ramp that ends inside the row: from the frame of the block's middle sample on `elapsed >= total` (frames are 20833 ns at 48 kHz)"""
    return max(1, (RAMP_K0 + n // 2) // RAMP_CH) * (1_000_000_000 // RAMP_RATE) - 7


def _elementwise_ops(O, x):
    """name -> (call(dst, src), reference, tolerance) for a row x"""
    n = x.size
    lib = L()
    ops = {
        "amplify": (lambda d, s: ok(lib.rh_amplify(vp(d), vp(s), n, 0.37, _st()), "amplify"), O.TestSource(x, 1, 48000).amplify(0.37).collect(), 0.0),
        "distortion": (lambda d, s: ok(lib.rh_distortion(vp(d), vp(s), n, 3.0, 0.6, _st()), "distortion"), O.TestSource(x, 1, 48000).distortion(3.0, 0.6).collect(), 0.0),
    }
    for code, alg in enumerate(["GPDF", "HighPass", "RPDF", "TPDF"]):  # the reference's enum order (dither.rs:40-69)
        # the oracle counts samples from 0: a block that starts at sample_offset is the tail of a stream with that many samples in front
        ref = O.TestSource(np.concatenate([np.zeros(DITHER_K0, f32), x]), DITHER_CH, 48000).dither(16, alg, 99).collect()[DITHER_K0:]
        ops["dither " + alg] = (lambda d, s, code=code: ok(lib.rh_dither(vp(d), vp(s), n, DITHER_K0, DITHER_CH, 16, code, 99, _st()), "dither"), ref, DITHER_TOL if alg == "GPDF" else 0.0)
    ns = _ramp_ns(n)
    ref = O.TestSource(np.concatenate([np.zeros(RAMP_K0, f32), x]), RAMP_CH, RAMP_RATE).linear_gain_ramp(ns, 0.1, 0.9, True).collect()[RAMP_K0:]
    ops["ramp"] = (lambda d, s: ok(lib.rh_linear_gain_ramp(vp(d), vp(s), n, RAMP_K0, RAMP_CH, RAMP_RATE, ns, 0.1, 0.9, 1, _st()), "ramp"), ref, 0.0)
    return ops


@pytest.mark.parametrize("n", SIZES)
def test_elementwise_rows(G, O, n):
    x = signal(n, n)
    for name, (call, ref, tol) in _elementwise_ops(O, x).items():
        assert ref.size == n
        for ls, ld in LEADS:
            one_row(call, x, n, ref, ls, ld, (name, n), tol)
        for lead in (0, 1, 2, 3):
            in_place(call, x, ref, lead, (name, n), tol)


def test_ramp_ends_inside_the_rows_and_the_block_starts_inside_a_frame():
    """what test_elementwise_rows relies on for rh_linear_gain_ramp, as arithmetic"""
    assert RAMP_K0 % RAMP_CH and DITHER_K0 % DITHER_CH
    for n in SIZES[1:]:
        step = 1_000_000_000 // RAMP_RATE
        done_frame = -(-_ramp_ns(n) // step)
        assert RAMP_K0 // RAMP_CH < done_frame <= (RAMP_K0 + n - 1) // RAMP_CH, n


# ---- rh_delay, rh_echo_mix: ld4_at at any index ------------------------------------------------------------------------------------------
# Delays 1 and 37: the tap's vector is off a boundary whatever the lead; 4: on one; n + 2: the tap leaves the row before the direct signal's
# vector does (the gap of Delay's zeros is 2 samples: inside one vector); 4n + 2: whole vectors of the gap.  ld4_at's branches: q < 0 entirely
# (the silence in front), q < 0 <= q + 3 (a vector across the row's start), the aligned pair inside, q + 4 > n (across the row's end), q >= n.
def _delays(n):
    return [1, 4, 37, n + 2, 4 * n + 2]


@pytest.mark.parametrize("n", SIZES)
def test_delay_and_echo_mix_rows(G, O, n):
    lib = L()
    x = signal(100 + n, n, 0.25)
    for D in _delays(n):
        ns = D * 1_000_000  # 1 kHz mono: a millisecond a sample (delay.rs:8-16)
        assert O.delay_samples(ns, 1000, 1) == D
        refs = {"delay": O.TestSource(x, 1, 1000).delay(ns).collect(), "echo_mix": O.TestSource(x, 1, 1000).reverb(ns, 0.7).collect()}
        calls = {"delay": lambda d, s: ok(lib.rh_delay(vp(d), vp(s), n, D, _st()), "delay"), "echo_mix": lambda d, s: ok(lib.rh_echo_mix(vp(d), vp(s), n, D, 0.7, _st()), "echo_mix")}
        for name in calls:
            assert refs[name].size == n + D
            for ls, ld in LEADS:
                one_row(calls[name], x, n + D, refs[name], ls, ld, (name, n, D))


def test_delay_of_nothing_is_silence_from_a_null_source(G):
    """rh_delay / rh_echo_mix with n == 0 take src == NULL (the header's `n && !src`): delay_samples zeros, nothing read"""
    lib = L()
    for D in (1, 5, 1027):
        for ld in (0, 1, 3):
            one_row(lambda d, s: ok(lib.rh_delay(vp(d), None, 0, D, _st()), "delay"), None, D, np.zeros(D, f32), 0, ld, ("delay of nothing", D), null_src=True)
            one_row(lambda d, s: ok(lib.rh_echo_mix(vp(d), None, 0, D, 0.7, _st()), "echo"), None, D, np.zeros(D, f32), 0, ld, ("echo of nothing", D), null_src=True)


# ---- rh_take_duration, rh_take_duration_from ---------------------------------------------------------------------------------------------
# 100 Hz: a sample of a 3-channel stream lasts 3.3 ms, so even a duration of one sample is above the millisecond under which the fade-out
# filter divides 0 by 0 (take.rs:33-41).  K = the samples the duration admits: n - 2 moved off a frame boundary (the duration ends inside a
# frame: the zeros that complete it follow), and n + 5 (the block ends first: exactly n written, nothing behind).
# Routes: k_take_duration is map4 over the `take` samples (its four alignments by the leads, the ragged last vector by K % 4) plus the pad
# stores of workgroup 0; fade 0 / 1 is the per-sample filter; take == 0 with pad > 0 launches for the pad alone (the test below).
TAKE_RATE = 100


def _take_cases(n, ch):
    dps = 1_000_000_000 // (TAKE_RATE * ch)
    k = max(1, n - 2)
    k -= 1 if k % ch == 0 else 0
    return dps, [(k, k * dps + dps // 2), (n + 5, (n + 5) * dps + 1)]


@pytest.mark.parametrize("ch", [3, 6])
@pytest.mark.parametrize("n", SIZES)
def test_take_duration_rows(G, O, n, ch):
    lib = L()
    x = signal(200 + n + ch, n)
    dps, cases = _take_cases(n, ch)
    for K, ns in cases:
        assert K % ch != 0 or K > n
        for fade in (0, 1):
            ref = O.TestSource(x, ch, TAKE_RATE).take_duration(ns, bool(fade)).collect()
            want = min(K, n) + ((ch - K % ch) if K <= n else 0)
            assert ref.size == want

            def call(d, s):
                m, e = C.c_uint64(0), C.c_int32(-1)
                ok(lib.rh_take_duration(vp(d), vp(s), n, 0, ch, TAKE_RATE, ns, fade, C.byref(m), C.byref(e), _st()), "take")
                assert e.value == (1 if K <= n else 0)
                return m.value

            for ls, ld in LEADS:
                one_row(call, x, n + ch, ref, ls, ld, ("take_duration", n, ch, K, fade), written=want)  # dst has capacity n + channels: the rest keeps the sentinel
            # the same from the state try_seek leaves (take.rs:222-231): two frames of the duration gone, frame position 0
            pos = 2 * ch * dps
            if ns > pos + dps:
                ref2 = O.TestSource(x, ch, TAKE_RATE).take_duration_sought(ns, pos, bool(fade)).collect()

                def call2(d, s):
                    m, e, r = C.c_uint64(0), C.c_int32(-1), C.c_uint64(0)
                    ok(lib.rh_take_duration_from(vp(d), vp(s), n, ns - pos, ns, 0, ch, TAKE_RATE, fade, C.byref(m), C.byref(e), C.byref(r), _st()), "take_from")
                    assert r.value == ns - pos - min(n, (ns - pos) // dps) * dps
                    return m.value

                for ls, ld in LEADS[:4]:
                    one_row(call2, x, n + ch, ref2, ls, ld, ("take_duration_from", n, ch, K, fade), written=ref2.size)


@pytest.mark.parametrize("ch", [3, 6])
def test_take_duration_from_completes_a_cut_frame_without_a_source(G, O, ch):
    """take == 0, pad > 0: what is left of the duration is below one sample and the frame has one sample out (frame_phase = 1) -- the entry
    writes the channels - 1 zeros that complete the frame and reads nothing: src == NULL is legal (the header's `take && !src`).  The oracle's
    adapter gets there by itself when the duration admits one sample: its output behind that sample."""
    lib = L()
    dps = 1_000_000_000 // (TAKE_RATE * ch)
    ref = O.TestSource(signal(7, 4 * ch), ch, TAKE_RATE).take_duration(dps + dps // 2).collect()
    assert ref.size == ch and np.all(arena.bits(ref[1:]) == 0)

    def call(d, s):
        m, e, r = C.c_uint64(99), C.c_int32(-1), C.c_uint64(99)
        ok(lib.rh_take_duration_from(vp(d), None, 4099, dps // 2, 10 * dps, 1, ch, TAKE_RATE, 1, C.byref(m), C.byref(e), C.byref(r), _st()), "take_from")
        assert (e.value, r.value) == (1, dps // 2)
        return m.value

    for ld in (0, 1, 2, 3):
        one_row(call, None, 4099 + ch, ref[1:], 0, ld, ("take_from pad only", ch), written=ch - 1, null_src=True)


def test_take_duration_refusals_write_nothing(G):
    """RH_ERR_INVALID: frame_phase >= channels, a NULL out_samples, a NULL src with samples to take; the dst arena keeps every sentinel"""
    lib = L()
    src, dst = arena.src_arena(signal(1, 64)), arena.dst_arena(70)
    m, e = C.c_uint64(0), C.c_int32(0)
    assert lib.rh_take_duration_from(vp(dst.ptr()), vp(src.ptr()), 64, 10**9, 10**9, 3, 3, TAKE_RATE, 0, C.byref(m), C.byref(e), None, _st()) == 1
    assert lib.rh_take_duration_from(vp(dst.ptr()), vp(src.ptr()), 64, 10**9, 10**9, 0, 3, TAKE_RATE, 0, None, C.byref(e), None, _st()) == 1
    assert lib.rh_take_duration_from(vp(dst.ptr()), None, 64, 10**9, 10**9, 0, 3, TAKE_RATE, 0, C.byref(m), C.byref(e), None, _st()) == 1
    assert lib.rh_take_duration(vp(dst.ptr()), vp(src.ptr()), 64, 0, 0, TAKE_RATE, 10**9, 0, C.byref(m), C.byref(e), _st()) == 1
    dst.check(0)
    src.unchanged()


# ---- rh_channels_convert, rh_channel_volume: the tile kernels ----------------------------------------------------------------------------
PAIRS = [(2, 2), (6, 2), (2, 6), (1, 2), (2, 1), (3, 5)]
WIDE_PAIR = (320, 2)  # 4 * (320 + 2) bytes a frame in + out: a tile of 10 KiB holds 7 frames, below the launchers' 8 -> the lane-per-frame kernels


def tile_frames(in_ch, out_ch):
    """Frames a tile of rh_channels_convert (rh::pcm_tile_try, f32 frames), rh_channel_volume and rh_channel_volume_steps: ~10 KiB in + out,
    a multiple of 4; below 8 the launcher takes its lane-per-frame / lane-per-output kernel."""
    return (10240 // (4 * (in_ch + out_ch))) & ~3


def layout_frames(in_ch, out_ch):
    """1 and 7 frames (less than a vector of output for some pairs, a ragged one for all), and two whole tiles plus 3 frames (the third
    workgroup's tile is cut; where there is no tile kernel: two workgroups of 256 lanes plus 3)"""
    tf = tile_frames(in_ch, out_ch)
    return [1, 7, 2 * (tf if tf >= 8 else 256) + 3]


def test_tile_frames_are_what_the_launchers_derive():
    assert [tile_frames(a, b) for a, b in PAIRS] == [640, 320, 320, 852, 852, 320] and tile_frames(*WIDE_PAIR) == 4
    assert layout_frames(6, 2) == [1, 7, 643] and layout_frames(*WIDE_PAIR) == [1, 7, 515]


@pytest.mark.parametrize("in_ch,out_ch", PAIRS + [WIDE_PAIR, (3, 3)])  # (3, 3): the tile kernel in place
def test_channels_convert_and_channel_volume_rows(G, O, in_ch, out_ch):
    """rh_channels_convert: the tile kernel (k_pcm_to_channels_tile, f32 frames; a src lead of s samples is a `shift` of 4 s bytes) for PAIRS,
    k_channels_convert for 320 -> 2.  rh_channel_volume: k_channel_volume_2x2 for (2, 2) -- its vector form only where src AND dst are on a
    boundary (leads (0, 0)), its scalar form elsewhere -- k_channel_volume_tile for the other PAIRS, k_channel_volume for 320 -> 2."""
    lib = L()
    from rodio_amd import _lib

    gains = np.linspace(0.2, 1.1, out_ch).astype(f32)
    for frames in layout_frames(in_ch, out_ch):
        x = signal(in_ch * 1000 + frames, frames * in_ch)
        refs = {"channels_convert": O.ChannelCountConverter(O.TestSource(x, in_ch, 48000), in_ch, out_ch).collect(),
                "channel_volume": O.ChannelVolume(O.TestSource(x, in_ch, 48000), gains).collect()}
        calls = {"channels_convert": lambda d, s: ok(lib.rh_channels_convert(vp(d), vp(s), frames, in_ch, out_ch, _st()), "channels_convert"),
                 "channel_volume": lambda d, s: ok(lib.rh_channel_volume(vp(d), vp(s), frames, in_ch, gains.ctypes.data_as(_lib.f32p), out_ch, _st()), "channel_volume")}
        for name in calls:
            assert refs[name].size == frames * out_ch
            for ls, ld in LEADS:
                one_row(calls[name], x, frames * out_ch, refs[name], ls, ld, (name, in_ch, out_ch, frames))
    # in place where the layout allows it (the same frame size: a lane's loads come before its stores, and a tile is parked before it is written)
    if in_ch == out_ch:
        frames = layout_frames(in_ch, out_ch)[-1]
        x = signal(77, frames * in_ch)
        for lead in (0, 1):
            in_place(lambda d, s: ok(lib.rh_channel_volume(vp(d), vp(s), frames, in_ch, gains.ctypes.data_as(_lib.f32p), out_ch, _st()), "cv"), x,
                     O.ChannelVolume(O.TestSource(x, in_ch, 48000), gains).collect(), lead, ("channel_volume", in_ch))


def test_channel_volume_refuses_more_than_16_outputs(G):
    lib = L()
    from rodio_amd import _lib

    src, dst = arena.src_arena(signal(3, 40)), arena.dst_arena(17 * 20)
    g = np.ones(17, f32)
    assert lib.rh_channel_volume(vp(dst.ptr()), vp(src.ptr()), 20, 2, g.ctypes.data_as(_lib.f32p), 17, _st()) == 3  # RH_ERR_UNSUPPORTED
    assert lib.rh_channel_volume(vp(dst.ptr()), vp(src.ptr()), 20, 0, g.ctypes.data_as(_lib.f32p), 2, _st()) == 1
    assert lib.rh_channels_convert(vp(dst.ptr()), vp(src.ptr()), 20, 2, 0, _st()) == 1
    dst.check(0)


# ---- rh_amplify_steps, rh_channel_volume_steps: the step tables in poison arenas of their own -----------------------------------------------
# A table holds exactly the entries the block reaches (steps_needed): the block's last sample uses the table's last entry, and an index one
# past it is a poison NaN in the output.  `first` lies in the middle of a period, so the first entry is used by fewer samples than a period.
def _first(period):
    return 5 * period + period // 2


def _entries(first, period, n):
    return (first + n - 1) // period - first // period + 1


def _table(seed, k, w=1):
    t = np.random.default_rng(seed).uniform(-2, 2, (k, w)).astype(f32)
    t[::7] = 0.0
    t[3::11] = -0.5
    return t.reshape(-1)


@pytest.mark.parametrize("period", [1, 3, 4, 441])
def test_amplify_steps_rows(G, period):
    """k_amplify_steps<false> (period < 4: a table load a sample) and <true> (period >= 4: two a lane; 4: a boundary in every vector after the
    first; 441: a vector that crosses one, most that do not), each with map4's four alignments and in place"""
    lib = L()
    first = _first(period)
    for n in SIZES:
        x = signal(period + n, n)
        k = _entries(first, period, n)
        fac = _table(period * 7 + n, k)
        assert (first + n - 1) // period - first // period == k - 1  # the last sample's entry is the table's last
        ref = amplify_ref(x, first, period, fac)
        tab = arena.src_arena(fac, 1)  # (the table one float behind a boundary: the kernel takes it entry by entry)
        call = lambda d, s: ok(lib.rh_amplify_steps(vp(d), vp(s), n, first, period, vp(tab.ptr()), k, _st()), "amplify_steps")  # noqa: E731
        for ls, ld in LEADS:
            one_row(call, x, n, ref, ls, ld, ("amplify_steps", period, n))
        for lead in (0, 1, 3):
            in_place(call, x, ref, lead, ("amplify_steps", period, n))
        tab.unchanged()
        # one entry too few: refused, and nothing is written
        if k > 1:
            dst = arena.dst_arena(n)
            assert lib.rh_amplify_steps(vp(dst.ptr()), vp(tab.ptr()), n, first, period, vp(tab.ptr()), k - 1, _st()) == 1
            dst.check(0)


@pytest.mark.parametrize("in_ch,out_ch", PAIRS + [WIDE_PAIR])
@pytest.mark.parametrize("gp,fp", [(3, 0), (441, 0), (441, 480), (3, 2)])
def test_channel_volume_steps_rows(G, in_ch, out_ch, gp, fp):
    """k_channel_volume_steps_2x2 for (2, 2) (vector form at leads (0, 0), scalar elsewhere), k_channel_volume_steps_tile for the other PAIRS,
    k_channel_volume_steps for 320 -> 2; with and without the factor table (fp = 0: factors_dev == NULL)"""
    lib = L()
    first, ff = _first(gp), (_first(fp) + 1 if fp else 0)
    for frames in layout_frames(in_ch, out_ch):
        total = frames * out_ch
        x = signal(in_ch + frames + gp, frames * in_ch)
        kg = _entries(first, gp, total)
        g = _table(gp + frames, kg, out_ch)
        gt = arena.src_arena(g, 1)
        kf, fac, ft = 0, None, None
        if fp:
            kf = _entries(ff, fp, total)
            fac = _table(fp + frames, kf)
            ft = arena.src_arena(fac, 3)
        ref = channel_volume_ref(x, in_ch, out_ch, first, gp, g, ff, fp or 1, fac)
        call = lambda d, s: ok(lib.rh_channel_volume_steps(vp(d), vp(s), frames, in_ch, out_ch, first, gp, vp(gt.ptr()), kg, ff, fp, vp(ft.ptr()) if ft else None, kf, _st()), "cvs")  # noqa: E731
        for ls, ld in LEADS:
            one_row(call, x, total, ref, ls, ld, ("channel_volume_steps", in_ch, out_ch, gp, fp, frames))
        gt.unchanged()
        if ft:
            ft.unchanged()
        if kg > 1:
            dst = arena.dst_arena(total)
            assert lib.rh_channel_volume_steps(vp(dst.ptr()), vp(gt.ptr()), frames, in_ch, out_ch, first, gp, vp(gt.ptr()), kg - 1, 0, 0, None, 0, _st()) == 1
            dst.check(0)


# ---- rh_resample_linear: k_resample_tile ---------------------------------------------------------------------------------------------------
def resample_tile_frames(frm, to, ch, span):
    """Output frames a tile of k_resample_tile for a SHORT row, as rh_resample_linear derives them: rows whose in + out stay below 1 MiB get
    tiles of 8 KiB (in + out: 4 ch (1 + F / T) bytes an output frame), a multiple of 4, cut to whole periods lcm(T, 4) of the converter
    where the row is one chunk and a period fits."""
    g = gcd(frm, to)
    F, T = frm // g, to // g
    tf = int(8 * 1024.0 / (4.0 * ch * (1.0 + F / T))) & ~3
    period = T * 4 // gcd(T, 4)
    if not span and tf >= period:
        tf -= tf % period
    return tf, F, T


RESAMPLE = [(44100, 48000, 2, 0), (44100, 48000, 1, 0), (48000, 44100, 6, 0), (8000, 48000, 3, 0), (44100, 48000, 2, 96), (44100, 44100, 2, 0)]


def test_resample_tile_frames_are_what_the_launcher_derives():
    assert [resample_tile_frames(*c)[0] for c in RESAMPLE[:5]] == [480, 960, 160, 576, 532]


@pytest.mark.parametrize("frm,to,ch,span", RESAMPLE)
def test_resample_rows(G, O, frm, to, ch, span):
    """1, 2 and 50 input frames (one cut tile) and as many as give three whole tiles of output plus 3 frames.  Unchunked rows: every tile in
    one chunk (resample_tile_out_fast from LDS; the last tile holds the verbatim last frame).  span 96 = chunks of 48 frames: every tile
    crosses ~10 chunk boundaries (resample_tile_out, frame by frame).  Equal rates: the device copy."""
    lib = L()
    tf, F, T = resample_tile_frames(frm, to, ch, span)
    big = -(-(3 * tf + 3) * F // T) + 1
    for frames in (1, 2, 50, big):
        m = C.c_uint64(0)
        ok(lib.rh_resample_out_frames(frames, frm, to, ch, span, C.byref(m)), "out_frames")
        out_frames = m.value
        if frames == big and F != T:
            assert 3 * tf < out_frames <= 4 * tf, (out_frames, tf)
        x = signal(frames + ch, frames * ch)
        if span:
            ref = O.UniformSourceIterator(O.SpanSource(x, ch, frm, span), ch, to).collect()
        else:
            ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
        assert ref.size == out_frames * ch, (ref.size, out_frames)
        call = lambda d, s: ok(lib.rh_resample_linear(vp(d), vp(s), frames, frm, to, ch, span, _st()), "resample")  # noqa: E731
        for ls, ld in LEADS:
            one_row(call, x, out_frames * ch, ref, ls, ld, ("resample", frm, to, ch, span, frames))


# ---- rh_mix_sum, rh_mix_pair ----------------------------------------------------------------------------------------------------------------
def _mix_sum(srcs, starts, out_len, leads, ld, tag, null_at=()):
    """rh_mix_sum over sources that each lie in a poison arena of their own (source i leads[i % len] samples behind a boundary); a source in
    null_at has no samples and a NULL pointer.  The three assertions."""
    lib = L()
    n = len(srcs)
    ars = [None if i in null_at else arena.src_arena(x, leads[i % len(leads)]) for i, x in enumerate(srcs)]
    ref = FC.ref_mix(srcs, starts, out_len)

    def run(dptr, ptr_of):
        ptrs = (C.c_void_p * n)(*[None if i in null_at else ptr_of(i) for i in range(n)]) if n else None
        st = (C.c_uint64 * n)(*starts) if n else None
        ln = (C.c_uint64 * n)(*[len(x) for x in srcs]) if n else None
        ok(lib.rh_mix_sum(vp(dptr), out_len, ptrs, st, ln, n, _st()), tag)

    dst = arena.dst_arena(out_len, ld)
    run(dst.ptr(), lambda i: ars[i].ptr())
    got = dst.check()
    for a in ars:
        if a is not None:
            a.unchanged()
    good, why = held(got, ref)
    assert good, (tag, ld, why)
    assert not np.any(arena.bits(got) == 0x80000000), "the mix is never -0.0"
    plains = [None if i in null_at else arena.plain(x, lead=leads[i % len(leads)]) for i, x in enumerate(srcs)]
    dt, dp = plain_dst(out_len, ld)
    run(dp, lambda i: plains[i][1])
    assert arena.same(d2h(dt, out_len, ld), got), (tag, ld, "the arena run differs from the plain run")


def test_mix_sum_aligned_starts(G):
    """k_mix_sum_v4: every pointer on a boundary, every start a multiple of 4, dst on a boundary; late joins, sources that end inside a vector
    (lengths 1027 and 4098) and before the output does, a zero-length source with a NULL pointer"""
    out_len = 4099
    srcs = [signal(1, 4099), signal(2, 1027), signal(3, 4098), np.zeros(0, f32), signal(4, 5), signal(5, 2000)]
    _mix_sum(srcs, [0, 4, 0, 8, 4092, 1028], out_len, [0], 0, "mix_sum v4", null_at=(3,))


def test_mix_sum_sixteen_short_aligned_sources(G):
    """k_mix_sum_v4_grp: 16 or more sources and a grid below 8 workgroups a CU; groups of eight that every lane can take whole, and groups
    that some lane cannot (a late join, a source that ends inside a vector), with a tail of 3 behind two groups"""
    out_len = 1027
    srcs = [signal(10 + s, 1027) for s in range(8)] + [signal(30 + s, [1027, 1026, 5, 1027, 513, 1027, 1024, 1027][s]) for s in range(8)] + [signal(50 + s, 1027 - 4 * s) for s in range(3)]
    starts = [0] * 8 + [0, 0, 1020, 0, 512, 0, 0, 0] + [0, 4, 8]
    _mix_sum(srcs, starts, out_len, [0], 0, "mix_sum v4 grouped")


@pytest.mark.parametrize("ld", [0, 1, 3])
def test_mix_sum_rows_anywhere(G, ld):
    """k_mix_sum_any: a late join 2 samples into a vector, sources that end inside a vector, one that ends before the output does, one that
    starts in the output's last vector, pointers at every residue (each source in its own poison arena: ld4_at's aligned loads reach into
    the poison on both sides of every source), a zero-length source with a NULL pointer; dst on a boundary (16-byte stores) and off it"""
    for out_len in (5, 1027, 4099):
        srcs = [signal(1, out_len), signal(2, max(1, out_len - 2)), signal(3, max(1, out_len // 2 + 1)), np.zeros(0, f32), signal(4, 3), signal(5, max(1, out_len - 6))]
        starts = [0, 2, 1, 3, out_len - 3, 6 if out_len > 6 else 0]
        _mix_sum(srcs, starts, out_len, [1, 0, 3, 0, 2, 1], ld, ("mix_sum any", out_len), null_at=(3,))


def test_mix_sum_130_sources_continue_from_dst(G):
    """more than one launch's table (128): the second launch reads dst, the partial sum, and adds sources 128 and 129 -- both forms"""
    out_len = 1027
    srcs = [signal(100 + s, out_len - (s % 5)) for s in range(130)]
    _mix_sum(srcs, [0] * 130, out_len, [0], 0, "mix_sum 130 aligned")  # k_mix_sum_v4_grp<false> over 128, then k_mix_sum_v4<true> over 2
    _mix_sum(srcs, [s % 4 for s in range(130)], out_len, [0, 1, 2, 3], 2, "mix_sum 130 anywhere")  # k_mix_sum_any<false>, then <true>
    more = srcs + [signal(300 + s, out_len - 4 * (s % 3)) for s in range(16)]
    _mix_sum(more, [0] * 146, out_len, [0], 0, "mix_sum 146 aligned")  # 18 sources in the second launch: k_mix_sum_v4_grp<true>


def test_mix_sum_of_no_source_is_zeros(G):
    for out_len in (1, 5, 4099):
        for ld in (0, 1, 3):
            _mix_sum([], [], out_len, [0], ld, ("mix_sum of nothing", out_len))


def test_mix_sum_refuses_a_null_source_that_has_samples(G):
    lib = L()
    dst = arena.dst_arena(64)
    ptrs, st, ln = (C.c_void_p * 1)(None), (C.c_uint64 * 1)(0), (C.c_uint64 * 1)(64)
    assert lib.rh_mix_sum(vp(dst.ptr()), 64, ptrs, st, ln, 1, _st()) == 1
    dst.check(0)


@pytest.mark.parametrize("na,nb", [(1027, 4099), (4099, 1026), (5, 3), (1, 4), (4098, 4098), (0, 5), (1027, 0)])
def test_mix_pair_rows(G, na, nb):
    """k_mix_pair: na != nb, each ending inside a vector -- the shorter row's last vector goes through ld4_at's sample-by-sample branch with
    poison behind it, and the longer one's rest follows verbatim; a and b at leads of their own; in place over either input"""
    lib = L()
    a, b = signal(na + 1, na), signal(nb + 2, nb)
    ref = mix_rows(a, b)
    total = max(na, nb)
    for (la, ld), lb in zip(LEADS, [0, 3, 1, 0, 2, 1, 3]):
        aa, bb = (arena.src_arena(a, la) if na else None), (arena.src_arena(b, lb) if nb else None)
        dst = arena.dst_arena(total, ld)
        ok(lib.rh_mix_pair(vp(dst.ptr()), vp(aa.ptr()) if na else None, na, vp(bb.ptr()) if nb else None, nb, _st()), "mix_pair")
        got = dst.check()
        for r in (aa, bb):
            if r is not None:
                r.unchanged()
        good, why = held(got, ref)
        assert good, ("mix_pair", na, nb, la, lb, ld, why)
        (at, ap), (bt, bp) = (arena.plain(a, lead=la) if na else (None, 0)), (arena.plain(b, lead=lb) if nb else (None, 0))
        dt, dp = plain_dst(total, ld)
        ok(lib.rh_mix_pair(vp(dp), vp(ap) if na else None, na, vp(bp) if nb else None, nb, _st()), "mix_pair")
        assert arena.same(d2h(dt, total, ld), got), ("mix_pair", na, nb, la, lb, ld, "the arena run differs from the plain run")
    # in place: dst is the LONGER input (dst holds max(na, nb) samples)
    if na and nb:
        long_is_a = na >= nb
        lo, sh = (a, b) if long_is_a else (b, a)
        for lead in (0, 1, 3):
            io = arena.inplace_arena(lo, lead)
            other = arena.src_arena(sh, (lead + 1) % 4)
            if long_is_a:
                ok(lib.rh_mix_pair(vp(io.ptr()), vp(io.ptr()), na, vp(other.ptr()), nb, _st()), "mix_pair in place")
            else:
                ok(lib.rh_mix_pair(vp(io.ptr()), vp(other.ptr()), na, vp(io.ptr()), nb, _st()), "mix_pair in place")
            good, why = held(io.check(), ref)
            assert good, ("mix_pair in place", na, nb, lead, why)
            other.unchanged()


# ---- rh_noise_generate ------------------------------------------------------------------------------------------------------------------------
# k_noise_fill: tiles of 1024 samples (four a lane, 256 lanes), and one more than n needs; k_noise_scan: the integrators' tiles.  n around the
# elementwise tile: 1023, 1024, 1025; around the scan's (256 lanes x 16 samples): 4096, 4097; and 1, 5 and 4099; ld = n + 13: rows start at every residue, the 13
# words between two rows keep the sentinel.  Every kind in one call plus a tenth stream, WhiteGaussian of Brownian's seed (the white samples
# Brownian integrates: test_gpu_noise.py's reference for it is the f64 recurrence over the device's own Gaussian); the states, 8 words each,
# in a state arena.
def _noise_states(kinds, rates, seeds, density):
    lib = L()
    st = np.zeros((len(kinds), 8), np.uint32)
    for r, (k, rate, seed) in enumerate(zip(kinds, rates, seeds)):
        row = (C.c_uint32 * 8)()
        ok(lib.rh_noise_init(row, CODE[k], rate, seed, density), "noise_init")
        st[r] = np.frombuffer(row, np.uint32)
    return st


@pytest.mark.parametrize("n", [1, 5, 1023, 1024, 1025, 4096, 4097, 4099])
def test_noise_generate_rows(G, n):
    lib = L()
    kinds = KINDS + ["white_gaussian"]
    rates = [44100, 48000, 8000, 192000, 22050, 44100, 48000, 96000, 44100, 48000]
    seeds = list(range(40, 49)) + [40 + KINDS.index("brownian")]
    ld = n + 13
    init = _noise_states(kinds, rates, seeds, 3000)
    outs = []
    for lead in (0, 1, 2, 3):
        states = arena.state_arena(init.size, init.view(f32))
        dst = arena.dst_arena_rows(len(kinds), n, ld, lead)
        ok(lib.rh_noise_generate(vp(dst.ptr()), ld, n, vp(states.ptr()), len(kinds), _st()), "noise_generate")
        y = dst.check().reshape(len(kinds), n)
        after = states.check(dtype=np.uint32).reshape(len(kinds), 8)
        assert np.all((after[:, 2].astype(np.uint64) | (after[:, 3].astype(np.uint64) << np.uint64(32))) == np.uint64(n)), "every stream's position moved by n"
        assert np.array_equal(after[:, [0, 1, 4, 5, 6]], init[:, [0, 1, 4, 5, 6]]), "seed, kind and parameters are not the call's to change"
        outs.append(y)
        for r, kind in enumerate(kinds):
            if kind in INTEGRATORS:
                leak, scale = integrator_consts(kind, rates[r])
                w = u1(hash_(seeds[r], idx(0, n))).astype(np.float64) if kind == "red" else y[-1].astype(np.float64)
                good, why = held(y[r], recurrence_f64(w, leak, scale, 0.0), INTEGRATOR_TOL)
            elif kind == "white_gaussian":
                good, why = held(y[r], reference(kind, seeds[r], 0, n), GAUSS_TOL)
            else:
                assert kind in EXACT
                good, why = held(y[r], reference(kind, seeds[r], 0, n, rate=rates[r], density=3000))
            assert good, ("noise", kind, n, lead, why)
    # (c) the plain run: a zeroed block and a plain state buffer
    import torch

    pd = torch.zeros(len(kinds) * ld + 8, dtype=torch.float32, device="cuda")
    ps = torch.from_numpy(init.view(np.int32).copy()).cuda()
    ok(lib.rh_noise_generate(vp(pd.data_ptr()), ld, n, vp(ps.data_ptr()), len(kinds), _st()), "noise_generate")
    torch.cuda.synchronize()
    plain = pd.cpu().numpy()[: len(kinds) * ld].reshape(len(kinds), ld)[:, :n]
    for y in outs:
        assert arena.same(y, plain), "the arena run differs from the plain run"


def test_noise_generate_refusals_write_nothing(G):
    lib = L()
    init = _noise_states(KINDS[:2], [48000, 48000], [1, 2], 2000)
    states = arena.state_arena(init.size, init.view(f32))
    dst = arena.dst_arena_rows(2, 100, 113)
    assert lib.rh_noise_generate(vp(dst.ptr()), 99, 100, vp(states.ptr()), 2, _st()) == 1  # ld < n
    assert lib.rh_noise_generate(vp(dst.ptr()), 113, 100, None, 2, _st()) == 1
    assert lib.rh_noise_generate(None, 113, 100, vp(states.ptr()), 2, _st()) == 1
    dst.check(0)
    states.unchanged()
