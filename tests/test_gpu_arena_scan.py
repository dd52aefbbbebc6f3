"""The batched and scan entries -- rh_limit, rh_biquad (modes 0 and 1), rh_agc, rh_reverb_spatial -- in a hostile memory layout
(tests/arena.py): dst, state in arenas of sentinel NaN, sources between zones of poison NaN.  A store past the row, a read outside it that
reaches the arithmetic and a sample that is never written all show; the values are held against the references and tolerances of the
entries' own tests (test_gpu_limit.py, test_gpu_effects.py, test_gpu_parity.py).  Through the C ABI."""
import ctypes as C

import numpy as np
import pytest
from conftest import knobs

import arena
from test_gpu_effects import TOL as TOL_EFFECTS  # 1e-5: rh_biquad mode 1 against mode 0 (test_biquad_mode1_channels_and_boundaries), the AGC against the oracle
from test_gpu_effects import _programme, _truth, rnd
from test_gpu_limit import TOL as TOL_LIMIT  # 1e-5
from test_gpu_limit import _signal

pytestmark = pytest.mark.gpu

LIMIT_KW = (dict(), dict(threshold=-6.0, knee_width=0.5, attack_ns=3_000_000, release_ns=12_000_000))  # test_limiter_matches_oracle_at_tile_and_lane_boundaries
AGC_KW = (dict(), dict(target_level=0.5, attack_ns=10_000_000, release_ns=5_000_000, absolute_max_gain=5.0, floor=0.2))  # test_gpu_effects.py


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _st():
    from rodio_amd import source

    return source._stream()


def vp(a):
    return C.c_void_p(a) if a is not None else None


bits, same = arena.bits, arena.same


def close(got, ref, tol):
    """max |got - ref| <= tol, written so that a NaN fails it"""
    got, ref = np.asarray(got, np.float32).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    assert got.shape == ref.shape
    err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) if got.size else 0.0
    return err <= tol, err


def d2h(t, n, first=0):
    """n floats of a device tensor (the plain runs' rows)"""
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()[first: first + n].copy()


# ---- rh_limit -------------------------------------------------------------------------------------------------------------------------
def _limit(dst, src, frames, ch, S, kw, state=None, rate=48000):
    from rodio_amd import _lib

    p = _lib.LimitParams(kw.get("threshold", -1.0), kw.get("knee_width", 4.0), kw.get("attack_ns", 5_000_000), kw.get("release_ns", 100_000_000))
    _lib.check(_lib.lib.rh_limit(vp(dst), vp(src), frames, ch, rate, S, C.byref(p), vp(state), _st()), "rh_limit")


def _limit_case(G, O, xs, frames, ch, kw, with_state, lead_src=0, lead_dst=0, in_place=False):
    """One rh_limit call over the rows xs (back to back: the entry's stride is frames * channels) in arenas; the rows against the oracle."""
    S, n = len(xs), frames * ch
    src = arena.inplace_arena_rows(xs, n, lead_src) if in_place else arena.src_arena_rows(xs, n, lead_src)
    dst = src if in_place else arena.dst_arena_rows(S, n, n, lead_dst)
    st = arena.state_arena(S * 2 * ch) if with_state else None
    _limit(dst.ptr(), src.ptr(), frames, ch, S, kw, st.ptr() if st else None)
    rows = dst.check().reshape(S, n)
    if not in_place:
        src.unchanged()
    G.async_status()
    for s in range(S):
        ok, err = close(rows[s], O.TestSource(xs[s], ch, 48000).limit(**kw).collect(), TOL_LIMIT)
        assert ok, (ch, frames, kw, with_state, s, err)
    if st:
        state = st.check()  # {integrator, peak} per channel: decibels of gain reduction, finite and not negative
        assert np.all(np.isfinite(state)) and np.all(state >= 0.0), state


@pytest.mark.parametrize("ch", [1, 2, 3, 6])
@pytest.mark.parametrize("frames", [1, 7, 257, 1025, 5000])
def test_limit_one_stream_scan_kernel(G, O, ch, frames):
    """n_streams = 1 on 16-byte boundaries: the scan kernel at any frames * channels, so rows that end inside a vector (frames * channels % 4
    takes 1, 2 and 3 here)."""
    x = _signal(100 * ch + frames % 97, frames, ch)
    for kw in LIMIT_KW:
        for with_state in (False, True):
            _limit_case(G, O, [x], frames, ch, kw, with_state)


def test_limit_one_stream_in_place(G, O):
    frames, ch = 1025, 3  # 3075 samples: the last vector holds three of them
    _limit_case(G, O, [_signal(11, frames, ch)], frames, ch, {}, True, in_place=True)


def test_limit_batched_scan_kernel(G, O):
    """3 stereo rows of 514 frames: a stride that is a multiple of 4, the scan kernel; 12 state floats."""
    frames, ch = 514, 2
    for kw in LIMIT_KW:
        _limit_case(G, O, [_signal(20 + s, frames, ch) for s in range(3)], frames, ch, kw, True)


def test_limit_batched_reference_order_kernel(G, O):
    """3 rows of 1001 frames of 3 channels (3003 samples: rows 1 and 2 start off 16-byte boundaries), and one stereo row that starts 1..3
    samples behind a boundary on either side: the one-lane-per-stream kernel."""
    frames, ch = 1001, 3
    _limit_case(G, O, [_signal(30 + s, frames, ch) for s in range(3)], frames, ch, {}, True)
    for ls, ld in [(1, 0), (0, 1), (3, 2)]:
        _limit_case(G, O, [_signal(40 + ls, 257, 2)], 257, 2, LIMIT_KW[1], ls == 1, lead_src=ls, lead_dst=ld)


def test_limit_io_wave_and_one_poll_point_variants(G, O):
    """RH_LIMIT_NIO=1 takes the I/O-wave variant from 3072 stereo frames on (a tile of 6144 frames must be half full: rh_limit's gate);
    RH_LIMIT_SKEW=1 the one-poll-point variant where the geometry has at least four waves: from 1024 stereo frames on (the 2048-frame tile
    of 8 x 4; below, single-wave tiles, which have no such variant).  One odd length each."""
    with knobs(RH_LIMIT_NIO="1"):
        _limit_case(G, O, [_signal(50, 3073, 2)], 3073, 2, {}, True)
    with knobs(RH_LIMIT_SKEW="1"):
        _limit_case(G, O, [_signal(51, 1025, 2)], 1025, 2, {}, True)


# ---- rh_biquad ------------------------------------------------------------------------------------------------------------------------
def _biquad(dst, src, frames, ch, S, co, mode, state=None):
    from rodio_amd import _lib

    _lib.check(_lib.lib.rh_biquad(vp(dst), vp(src), frames, ch, S, co.ctypes.data_as(_lib.f32p), vp(state), mode, _st()), "rh_biquad")


def _biquad_state_ok(state, xs, refs, ch, tol):
    """{x1, x2, y1, y2} per channel behind a zero state: the last two inputs (exactly) and the last two outputs"""
    for s, (x, ref) in enumerate(zip(xs, refs)):
        x, ref = x.reshape(-1, ch), np.asarray(ref, np.float32).reshape(-1, ch)
        for c in range(ch):
            x1, x2, y1, y2 = state[s * 4 * ch + 4 * c: s * 4 * ch + 4 * c + 4]
            want = [x[-1, c], x[-2, c] if len(x) > 1 else 0.0, ref[-1, c], ref[-2, c] if len(x) > 1 else 0.0]
            assert bits(x1) == bits(want[0]) and bits(x2) == bits(np.float32(want[1])), (s, c)
            assert abs(float(y1) - float(want[2])) <= tol and abs(float(y2) - float(want[3])) <= tol, (s, c)


def _biquad_mode1_case(G, O, ch, frames, S):
    xs = [rnd(200 + 7 * ch + s, frames * ch, 0.4) for s in range(S)]  # test_biquad_mode1_channels_and_boundaries' signal
    n = frames * ch
    for kind, freq in (("low_pass", 200), ("high_pass", 300)):
        co = G.biquad_coeffs(kind, freq, 0.5, 48000)
        src, dst, st = arena.src_arena_rows(xs, n), arena.dst_arena_rows(S, n, n), arena.state_arena(S * 4 * ch)
        _biquad(dst.ptr(), src.ptr(), frames, ch, S, co, 1, st.ptr())
        rows = dst.check().reshape(S, n)
        src.unchanged()
        G.async_status()
        refs = [getattr(O.TestSource(x, ch, 48000), kind)(freq).collect() for x in xs]  # = mode 0, bit for bit (test_biquad_mode0_batch_bit_exact)
        for s in range(S):
            ok, d = close(rows[s], refs[s], TOL_EFFECTS)
            assert ok, (kind, ch, frames, s, d)
            t = _truth(xs[s], co, ch)
            e_par, e_seq = float(np.max(np.abs(rows[s] - t))), float(np.max(np.abs(refs[s] - t)))
            assert e_par <= 2.0 * e_seq + 1e-7, (kind, ch, frames, s, e_par, e_seq)
        _biquad_state_ok(st.check(), xs, refs, ch, TOL_EFFECTS)


@pytest.mark.parametrize("ch", [1, 2, 3, 4, 5, 6, 7, 8])
def test_biquad_mode1_one_stream(G, O, ch):
    with knobs(RH_BIQUAD_NO_FALLBACK="1"):  # the scan kernel or nothing
        for frames in (1, 3, 255, 513, 4097):
            _biquad_mode1_case(G, O, ch, frames, 1)


@pytest.mark.parametrize("ch", [2, 4])
def test_biquad_mode1_batched(G, O, ch):
    with knobs(RH_BIQUAD_NO_FALLBACK="1"):
        _biquad_mode1_case(G, O, ch, 514, 3)


@pytest.mark.parametrize("ch", [1, 3, 6])
@pytest.mark.parametrize("S", [1, 3])
def test_biquad_mode0_bits(G, O, ch, S):
    """The reference-order kernels (the vector form for rows on 16-byte boundaries, the 4-byte one otherwise): the oracle's bits, and the
    same bits as on plain rows."""
    co = G.biquad_coeffs("low_pass", 300, 0.5, 48000)
    for frames in (1, 17, 4099):
        n = frames * ch
        xs = [rnd(10 + s + frames, n, 0.7) for s in range(S)]
        src, dst, st = arena.src_arena_rows(xs, n), arena.dst_arena_rows(S, n, n), arena.state_arena(S * 4 * ch)
        _biquad(dst.ptr(), src.ptr(), frames, ch, S, co, 0, st.ptr())
        rows = dst.check().reshape(S, n)
        src.unchanged()
        refs = [O.TestSource(x, ch, 48000).low_pass(300).collect() for x in xs]
        for s in range(S):
            assert np.array_equal(bits(rows[s]), bits(refs[s])), (ch, S, frames, s)
        _biquad_state_ok(st.check(), xs, refs, ch, 0.0)
        pt, pp = arena.plain(np.stack(xs), S)
        dt, dp = arena.plain_dst(S * n)
        _biquad(dp, pp, frames, ch, S, co, 0, None)
        assert same(d2h(dt, S * n), rows), (ch, S, frames)


def test_biquad_mode0_in_place(G, O):
    frames, ch, S = 4099, 3, 3
    co = G.biquad_coeffs("high_pass", 120, 0.5, 44100)
    xs = [rnd(70 + s, frames * ch) for s in range(S)]
    io = arena.inplace_arena_rows(xs, frames * ch)
    _biquad(io.ptr(), io.ptr(), frames, ch, S, co, 0, None)
    rows = io.check().reshape(S, -1)
    for s in range(S):
        assert np.array_equal(bits(rows[s]), bits(O.TestSource(xs[s], ch, 44100).high_pass(120).collect())), s


# ---- rh_agc ---------------------------------------------------------------------------------------------------------------------------
def _agc(dst, src, n, S, kw, state=None, rate=48000):
    from rodio_amd import _lib

    p = _lib.AgcParams(kw.get("target_level", 1.0), kw.get("attack_ns", 4_000_000_000), kw.get("release_ns", 0), kw.get("absolute_max_gain", 7.0), kw.get("floor", 0.0))
    _lib.check(_lib.lib.rh_agc(vp(dst), vp(src), n, rate, S, C.byref(p), vp(state), _st()), "rh_agc")


def _agc_state():
    from rodio_amd import _lib

    return int(_lib.lib.rh_agc_state_floats())


@pytest.mark.parametrize("kw", AGC_KW, ids=["default", "general"])
@pytest.mark.parametrize("S,n", [(1, 100), (3, 127), (17, 8492), (1, 40001)])  # (1, 40001): above the square-pass threshold, an odd length
def test_agc_rows_and_states(G, O, S, n, kw):
    from rodio_amd import _lib

    xs = [_programme(700 + s, n + 8)[:n] for s in range(S)]
    K = _agc_state()
    src, dst, st = arena.src_arena_rows(xs, n), arena.dst_arena_rows(S, n, n), arena.state_arena(S * K)
    _lib.check(_lib.lib.rh_agc_state_init(vp(st.ptr()), S, _st()), "rh_agc_state_init")
    fresh = st.check()
    assert np.array_equal(fresh.reshape(S, K)[:, 3], np.ones(S, np.float32)) and float(np.abs(fresh).sum()) == float(S)  # gain 1.0, the rest zero
    _agc(dst.ptr(), src.ptr(), n, S, kw, st.ptr())
    rows = dst.check().reshape(S, n)
    src.unchanged()
    state = st.check()
    assert np.all(np.isfinite(state))
    # the same call on plain rows (zeros around the sources, a fresh zeroed dst): the same bits, rows and state
    pt, pp = arena.plain(np.stack(xs), S)
    dt, dp = arena.plain_dst(S * n)
    st2 = G.agc_state(S)
    _agc(dp, pp, n, S, kw, st2.data_ptr())
    assert same(d2h(dt, S * n), rows)
    assert same(st2.cpu().numpy(), state)
    for s in range(S):  # bits against the oracle (test_gpu_effects.py holds the AGC to 1e-5: on these rows every sample is the reference's)
        ref = O.TestSource(xs[s], 1, 48000).automatic_gain_control(**kw).collect()
        ok, err = close(rows[s], ref, TOL_EFFECTS)
        assert ok, (S, n, s, err)
        assert same(rows[s], ref), (S, n, s, err, int(np.count_nonzero(bits(rows[s]) != bits(ref))))


def test_agc_without_a_state_in_place(G, O):
    S, n = 3, 8492
    xs = [_programme(1300 + s, n) for s in range(S)]
    io = arena.inplace_arena_rows(xs, n)
    _agc(io.ptr(), io.ptr(), n, S, {}, None, rate=44100)
    rows = io.check().reshape(S, n)
    pt, pp = arena.plain(np.stack(xs), S)
    _agc(pp, pp, n, S, {}, None, rate=44100)
    assert same(d2h(pt, S * n, arena.GUARD), rows)
    for s in range(S):
        ref = O.TestSource(xs[s], 2, 44100).automatic_gain_control().collect()
        ok, err = close(rows[s], ref, TOL_EFFECTS)
        assert ok and same(rows[s], ref), (s, err)


# ---- rh_reverb_spatial ----------------------------------------------------------------------------------------------------------------
def _delay_ns(d, rate=48000, ch=2):
    """a duration whose rh_delay_samples is d"""
    from rodio_amd import _lib

    ns = (d * 1_000_000_000 + rate * ch - 1) // (rate * ch)
    for cand in (ns, ns + 1, ns - 1):
        if int(_lib.lib.rh_delay_samples(cand, rate, ch)) == d:
            return cand
    raise AssertionError(f"no duration gives a delay of {d} samples")


def _reverb_spatial(dst, src, n, d, gain, gains, S, src_stride, dst_stride):
    from rodio_amd import _lib

    return _lib.lib.rh_reverb_spatial(vp(dst), vp(src), n, d, gain, vp(gains), S, src_stride, dst_stride, _st())


@pytest.mark.parametrize("n,d", [(2000, 37), (2000, 36), (300, 4801)])
def test_reverb_spatial_rows_with_gaps(G, O, n, d):
    """Strides = the row lengths rounded up to a multiple of 4, plus 8: gaps behind every row on both sides.  (2000, 36) takes the 16-byte
    path; an odd delay swaps the channels of the delayed clone and drops half a frame at the end; a delay beyond the source."""
    from rodio_amd import _lib

    S = 3
    ns = _delay_ns(d)
    xs = [rnd(40 + s, n, 0.25) for s in range(S)]
    em = [[0.5 + 0.01 * s, 0, 1] for s in range(S)]
    gains = np.stack([G.spatial_gains(e, [-1, 0, 0], [1, 0, 0]) for e in em]).astype(np.float32)
    n_out = 2 * ((n + d) // 2)
    ss, ds = (n + 3) // 4 * 4 + 8, (n_out + 3) // 4 * 4 + 8
    src, dst, g = arena.src_arena_rows(xs, ss), arena.dst_arena_rows(S, n_out, ds), arena.state_arena(2 * S, gains)
    _lib.check(_reverb_spatial(dst.ptr(), src.ptr(), n, d, 0.3, g.ptr(), S, ss, ds), "rh_reverb_spatial")
    rows = dst.check().reshape(S, n_out)
    src.unchanged()
    g.unchanged()
    for s in range(S):
        ref = O.Spatial(O.TestSource(xs[s], 2, 48000).reverb(ns, 0.3), em[s], [-1, 0, 0], [1, 0, 0]).collect()
        assert len(ref) == n_out and np.array_equal(bits(rows[s]), bits(ref)), s
    pt, pp = arena.plain(np.stack(xs), S, ss)
    dt, dp = arena.plain_dst(S * ds)
    _lib.check(_reverb_spatial(dp, pp, n, d, 0.3, g.ptr(), S, ss, ds), "rh_reverb_spatial")
    plain = d2h(dt, S * ds).reshape(S, ds)[:, :n_out]
    assert same(plain, rows)


def test_reverb_spatial_refuses_a_row_that_ends_inside_a_frame(G):
    """(2001, 36): rows are interleaved STEREO samples, whole frames of them -- RH_ERR_INVALID, and nothing is written."""
    S, n, d = 3, 2001, 36
    xs = [rnd(60 + s, n, 0.25) for s in range(S)]
    n_out = 2 * ((n + d) // 2)
    ss, ds = (n + 3) // 4 * 4 + 8, (n_out + 3) // 4 * 4 + 8
    src, dst, g = arena.src_arena_rows(xs, ss), arena.dst_arena_rows(S, n_out, ds), arena.state_arena(2 * S, np.full(2 * S, 0.5, np.float32))
    assert _reverb_spatial(dst.ptr(), src.ptr(), n, d, 0.3, g.ptr(), S, ss, ds) == 1  # RH_ERR_INVALID
    dst.check(written=0)
    # ... and rows an odd number of samples apart (their frames are stored as 8-byte pairs), or off an 8-byte boundary
    n = 2000
    xs = [rnd(60 + s, n, 0.25) for s in range(S)]
    n_out = 2 * ((n + d) // 2)
    src, dst = arena.src_arena_rows(xs, n + 8), arena.dst_arena_rows(S, n_out, n_out + 9)
    assert _reverb_spatial(dst.ptr(), src.ptr(), n, d, 0.3, g.ptr(), S, n + 8, n_out + 9) == 1
    dst.check(written=0)
    src, dst = arena.src_arena_rows(xs, n + 8), arena.dst_arena_rows(S, n_out, n_out + 8, lead=1)
    assert _reverb_spatial(dst.ptr(), src.ptr(), n, d, 0.3, g.ptr(), S, n + 8, n_out + 8) == 1
    dst.check(written=0)
