"""The mixers, converters, generators and the two streaming handles -- rh_wide_mix_block(_filtered), rh_uniform_segments, rh_uniform_row,
rh_crossfade, rh_signal_generate, rh_chirp, rh_resampler_*, rh_echo_* -- in a hostile memory layout (tests/arena.py): every output, state and
scratch in an arena of sentinel NaN, every source between zones of poison NaN that begin where the header says reading ends.  The values
are held against the references of the entries' own tests, and bit for bit against the same call on plain rows.  Through the C ABI."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

import arena
from test_generators_cpu import phase_step, wave_ref
from test_gpu_generators import SINE_TOL, chirp_ref  # 2.4e-7: 2 ulp at 1.0 against an f64 sin of the same f32 argument
from test_gpu_uniform import CASES as UNIFORM_CASES
from test_gpu_uniform import U64_MAX, _first_tap, _span_frames
from test_gpu_widemix import _oracle as wide_oracle
from test_gpu_widemix import out_frames
from test_gpu_widemix_filtered import _oracle as filtered_oracle
from test_mix_cpu import MS, crossfade_restated, signal

pytestmark = pytest.mark.gpu
NONE = 0xFFFFFFFF
f32 = np.float32


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


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


# ---- rh_wide_mix_block ----------------------------------------------------------------------------------------------------------------
def _wide_sources(to_rate, M, specs, seed):
    """One block of M output frames from mixer time 0.  specs: (channels, rate, gain, role).  A "live" source holds exactly the frames the
    header lets the block read -- up to the second tap of output frame M - 1; an "ended" one ends inside the block and holds its frames up
    to `last`; a "silent" one has ended before the block (no frames at all).  -> [(x, channels, rate, gain, frames, last)]"""
    rng = np.random.default_rng(seed)
    out = []
    for ch, rate, gain, role in specs:
        g = gcd(rate, to_rate)
        F, T = rate // g, to_rate // g
        if role == "live":
            n = (M - 1) * F // T + 2
            out.append((rng.uniform(-1, 1, n * ch).astype(f32), ch, rate, gain, M, NONE))
        elif role == "ended":
            n = 1
            while out_frames(n + 1, F, T) <= max(1, M // 2):
                n += 1
            assert 1 <= out_frames(n, F, T) <= M
            out.append((rng.uniform(-1, 1, n * ch).astype(f32), ch, rate, gain, out_frames(n, F, T), n - 1))
        else:
            out.append((np.zeros(0, f32), ch, rate, gain, 0, 0))
    return out


def _wide_table(srcs, ptrs):
    from rodio_amd import _lib

    arr = (_lib.WideSrc * len(srcs))()
    for k, ((x, ch, rate, gain, frames, last), p) in enumerate(zip(srcs, ptrs)):
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = p, ch, rate, 0, frames, last, gain
    return arr


def _wide_block(G, to_ch, to_rate, M, srcs):
    from rodio_amd import _lib

    ins = [arena.src_arena(x) for x, *_ in srcs]
    dst = arena.dst_arena(M * to_ch)
    _lib.check(_lib.lib.rh_wide_mix_block(vp(dst.ptr()), to_ch, to_rate, M, _wide_table(srcs, [a.ptr() for a in ins]), len(srcs), _st()), "rh_wide_mix_block")
    row = dst.check()
    for a in ins:
        a.unchanged()
    want = wide_oracle([(x, ch, rate, gain) for x, ch, rate, gain, _, _ in srcs], to_ch, to_rate)
    assert len(want) >= M * to_ch and same(row, want[: M * to_ch]), (to_ch, to_rate, M)
    plains = [arena.plain(x if x.size else np.zeros(1, f32)) for x, *_ in srcs]
    pd, pdp = arena.plain_dst(M * to_ch)
    _lib.check(_lib.lib.rh_wide_mix_block(vp(pdp), to_ch, to_rate, M, _wide_table(srcs, [p for _, p in plains]), len(srcs), _st()), "rh_wide_mix_block")
    assert same(host(pd)[: M * to_ch], row)


@pytest.mark.parametrize("to_ch,to_rate", [(6, 48000), (3, 22050), (1, 48000)])
@pytest.mark.parametrize("M", [1, 63, 1000])
def test_wide_mix_block(G, to_ch, to_rate, M):
    specs = [(6, 44100, 1.0, "live"), (2, 44100, 0.5, "live"), (1, 48000, -1.5, "ended"), (to_ch, to_rate, 1.0, "live"), (3, 11025, 2.0, "silent")]
    _wide_block(G, to_ch, to_rate, M, _wide_sources(to_rate, M, specs, 600 + to_ch + M))


def test_wide_mix_block_alike_sources(G):
    """Sources of the mixer's own layout and one rate, all live: k_wide_mix_uniform."""
    _wide_block(G, 6, 48000, 1000, _wide_sources(48000, 1000, [(6, 44100, g, "live") for g in (1.0, 0.5, -0.75)], 77))


# ---- rh_wide_mix_block_filtered -------------------------------------------------------------------------------------------------------
def _filtered_block(G, to_ch, to_rate, M, srcs, filts, mode, ins, states, scratch, scratch_bytes, dst):
    from rodio_amd import _lib

    n = len(srcs)
    kinds = (C.c_int32 * n)(*[-1 if f is None else {"lp": 0, "hp": 1}[f[0]] for f in filts])
    co = np.zeros((n, 5), f32)
    for k, f in enumerate(filts):
        if f is not None:
            co[k] = G.biquad_coeffs(kinds[k], f[1], f[2], to_rate)
    st = (C.c_void_p * n)(*states)
    return _lib.lib.rh_wide_mix_block_filtered(vp(dst), to_ch, to_rate, M, _wide_table(srcs, ins), n, kinds, co.ctypes.data_as(_lib.f32p), st, mode, vp(scratch), scratch_bytes, _st())


@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("M", [1000, 63])  # 6000 samples a row: a multiple of 4 (one rh_biquad call per coefficient set); 378: not (a call per row)
def test_wide_mix_block_filtered(G, mode, M):
    """2 filtered of 4 sources (one of them ends inside the block: a rh_biquad call of its own), the scratch exactly as large as
    rh_wide_mix_filtered_scratch_bytes says, every carried state in an arena of its own."""
    from rodio_amd import _lib

    to_ch, to_rate = 6, 48000
    specs = [(6, 44100, 1.0, "live"), (2, 44100, 0.5, "live"), (1, 48000, -1.5, "ended"), (6, 48000, 0.25, "live")]
    filts = [("lp", 1000, 0.5), None, ("hp", 2000, 0.5), None]
    assert all(f is None or G.filter_scan_ok({"lp": 0, "hp": 1}[f[0]], f[1], f[2], to_rate) for f in filts)
    srcs = _wide_sources(to_rate, M, specs, 4200 + M)
    need = C.c_uint64(0)
    _lib.check(_lib.lib.rh_wide_mix_filtered_scratch_bytes(to_ch, M, 2, C.byref(need)), "rh_wide_mix_filtered_scratch_bytes")
    assert need.value and need.value % 4 == 0
    ins = [arena.src_arena(x) for x, *_ in srcs]
    sts = [None if f is None else arena.state_arena(4 * to_ch) for f in filts]
    scr, dst = arena.dst_arena(need.value // 4), arena.dst_arena(M * to_ch)
    _lib.check(_filtered_block(G, to_ch, to_rate, M, srcs, filts, mode, [a.ptr() for a in ins], [s.ptr() if s else None for s in sts], scr.ptr(), need.value, dst.ptr()), "rh_wide_mix_block_filtered")
    row = dst.check()
    scr.check_guards()
    for a in ins:
        a.unchanged()
    states = [s.check() for s in sts if s]
    assert all(np.all(np.isfinite(s)) for s in states)
    G.async_status()
    want = filtered_oracle([(x, ch, rate, gain, f) for (x, ch, rate, gain, _, _), f in zip(srcs, filts)], to_ch, to_rate)[: M * to_ch]
    assert want.size == M * to_ch
    if mode == 0:
        assert same(row, want)
        plains = [arena.plain(x) for x, *_ in srcs]
        import torch

        pst = [None if f is None else torch.zeros(4 * to_ch, device="cuda") for f in filts]
        pscr = torch.zeros(need.value // 4 + 8, device="cuda")
        pd, pdp = arena.plain_dst(M * to_ch)
        _lib.check(_filtered_block(G, to_ch, to_rate, M, srcs, filts, mode, [p for _, p in plains], [s.data_ptr() if s is not None else None for s in pst], pscr.data_ptr(), need.value, pdp),
                   "rh_wide_mix_block_filtered")
        assert same(host(pd)[: M * to_ch], row)
        assert all(same(host(p), s) for p, s in zip([p for p in pst if p is not None], states))
    else:  # test_mode_1_stays_within_the_filter_contract: 1e-5 |gain| a filtered source of |x| <= 1
        bound = 1e-5 * sum(abs(g) for (_, _, _, g, _, _), f in zip(srcs, filts) if f is not None)
        err = float(np.max(np.abs(row.astype(np.float64) - want.astype(np.float64))))
        assert err <= bound, (err, bound)


# ---- rh_uniform_segments --------------------------------------------------------------------------------------------------------------
def _segments(lib, x, ch, rate, to_ch, to_rate, span_samples, cut, src_ptr, dst_ptr):
    """test_gpu_uniform._convert's table over rows that live somewhere else: every span cut once, each piece a segment."""
    from rodio_amd import _lib

    frames = len(x) // ch
    span_f = frames if span_samples is None else min(span_samples, 32768) // ch
    segs, off_out, f0 = [], 0, 0
    while f0 < frames:
        n = min(span_f, frames - f0)
        m_done = 0
        for upto in sorted({min(n, max(1, int(round(cut * n)))), n}):
            closed = upto == n
            ready = _span_frames(lib, upto, rate, to_rate, closed)
            if ready > m_done:
                first = min(_first_tap(lib, m_done, rate, to_rate), upto - 1)
                s = _lib.UniformSeg()
                s.src, s.dst = src_ptr + 4 * (f0 + first) * ch, dst_ptr + 4 * (off_out + m_done) * to_ch
                s.src_frame0, s.src_frames, s.m0, s.m1 = first, upto - first, m_done, ready
                s.span_frames = n if closed else U64_MAX
                s.from_rate, s.to_rate, s.from_ch, s.to_ch, s.gain, s.reserved = rate, to_rate, ch, to_ch, 1.0, 0
                segs.append(s)
                m_done = ready
        off_out += m_done
        f0 += n
    return (_lib.UniformSeg * len(segs))(*segs), off_out


@pytest.mark.parametrize("case", range(len(UNIFORM_CASES)))
def test_uniform_segments(G, O, case):
    from rodio_amd import _lib

    lib = _lib.lib
    ch, rate, to_ch, to_rate, frames, span = UNIFORM_CASES[case]
    x = (np.random.default_rng(900 + case).uniform(-1, 1, frames * ch)).astype(f32)
    if span == "buffer":
        ref_src, span_samples = O.SamplesBuffer(ch, rate, x), len(x)
    elif span is None:
        ref_src, span_samples = O.TestSource(x, ch, rate), None
    else:
        ref_src, span_samples = O.SpanSource(x, ch, rate, span), span
    ref = O.UniformSourceIterator(ref_src, to_ch, to_rate).collect()
    src, dst = arena.src_arena(x), arena.dst_arena(ref.size)
    table, total = _segments(lib, x, ch, rate, to_ch, to_rate, span_samples, 0.5, src.ptr(), dst.ptr())
    assert total * to_ch == ref.size
    _lib.check(lib.rh_uniform_segments(table, len(table), _st()), "rh_uniform_segments")
    row = dst.check()
    src.unchanged()
    assert same(row, ref), case
    pt, pp = arena.plain(x)
    pd, pdp = arena.plain_dst(ref.size)
    table, _ = _segments(lib, x, ch, rate, to_ch, to_rate, span_samples, 0.5, pp, pdp)
    _lib.check(lib.rh_uniform_segments(table, len(table), _st()), "rh_uniform_segments")
    assert same(host(pd)[: ref.size], row)


# ---- rh_uniform_row -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,fc,fr,tc,tr,span", [(30000, 6, 48000, 1, 8000, 1000),   # 6-channel spans of 1000 samples: every chain ends inside a frame
                                                (3001, 2, 48000, 2, 48000, 0),       # a row that ends in mid-frame
                                                (6000, 2, 44100, 6, 48000, 0)])
def test_uniform_row(G, O, n, fc, fr, tc, tr, span):
    from rodio_amd import _lib

    lib = _lib.lib
    x = signal(n, 57)
    ref = O.UniformSourceIterator(O.SpanSource(x, fc, fr, span) if span else O.TestSource(x, fc, fr), tc, tr).collect()
    m = C.c_uint64(0)
    _lib.check(lib.rh_uniform_row_out_samples(n, fc, fr, tc, tr, span, C.byref(m)), "rh_uniform_row_out_samples")
    assert m.value == ref.size
    src, dst = arena.src_arena(x), arena.dst_arena(m.value)
    got = C.c_uint64(0)
    _lib.check(lib.rh_uniform_row(vp(dst.ptr()), m.value, vp(src.ptr()), n, fc, fr, tc, tr, span, C.byref(got), _st()), "rh_uniform_row")
    assert got.value == m.value
    row = dst.check()
    src.unchanged()
    assert same(row, ref)
    pt, pp = arena.plain(x)
    pd, pdp = arena.plain_dst(m.value)
    _lib.check(lib.rh_uniform_row(vp(pdp), m.value, vp(pp), n, fc, fr, tc, tr, span, C.byref(got), _st()), "rh_uniform_row")
    assert same(host(pd)[: m.value], row)
    # a capacity one sample short: RH_ERR_INVALID, nothing written
    dst2 = arena.dst_arena(m.value)
    assert lib.rh_uniform_row(vp(dst2.ptr()), m.value - 1, vp(src.ptr()), n, fc, fr, tc, tr, span, C.byref(got), _st()) == 1
    dst2.check(written=0)


# ---- rh_crossfade ---------------------------------------------------------------------------------------------------------------------
def test_crossfade_three_pairs_one_call(G, O):
    """One pair on the fused kernel, one with a 6-channel b (the composed path on the stream's scratch), one whose duration expires inside a
    frame; every capacity exactly rh_crossfade_out_samples().  Then one capacity too small: RH_ERR_INVALID and no word of the three written."""
    from rodio_amd import _lib

    lib, W = _lib.lib, _lib.CROSSFADE_PAIR_WORDS
    d = 50 * MS + 10_416  # 4801 samples of a stereo 48 kHz `a`: inside a frame (test_mix_cpu.py's "cut_frame"); mono rows have no frame to cut
    shapes = [((signal(6000, 41), 1, 44100), (signal(3000, 42), 1, 48000)),
              ((signal(6000, 43), 2, 48000), (signal(18000, 44), 6, 48000)),
              ((signal(6000, 45), 2, 48000), (signal(3000, 46), 1, 44100))]
    wants = [crossfade_restated(O, O.TestSource(*a), O.TestSource(*b), d) for a, b in shapes]

    def table(a_ptrs, b_ptrs, d_ptrs, caps):
        pairs = (C.c_uint64 * (W * 3))()
        for k, ((a, ca, ra), (b, cb, rb)) in enumerate(shapes):
            pairs[W * k: W * k + W] = [a_ptrs[k], a.size, ca, ra, b_ptrs[k], b.size, cb, rb, 0, d_ptrs[k], caps[k]]
        return pairs

    caps = []
    for k in range(3):
        m = C.c_uint64(0)
        _lib.check(lib.rh_crossfade_out_samples(C.cast(C.byref(table([0] * 3, [0] * 3, [0] * 3, [0] * 3), 8 * W * k), C.POINTER(C.c_uint64)), d, C.byref(m)), "rh_crossfade_out_samples")
        caps.append(m.value)
        assert m.value == wants[k].size
    assert caps[2] % 2 == 1  # the third crossfade ends inside a frame
    ia, ib = [arena.src_arena(a) for (a, _, _), _ in shapes], [arena.src_arena(b) for _, (b, _, _) in shapes]
    outs = [arena.dst_arena(c) for c in caps]
    short = list(caps)
    short[1] -= 1
    assert lib.rh_crossfade(table([a.ptr() for a in ia], [b.ptr() for b in ib], [o.ptr() for o in outs], short), 3, d, None, _st()) == 1  # RH_ERR_INVALID
    for o in outs:
        o.check(written=0)
    got = (C.c_uint64 * 3)()
    _lib.check(lib.rh_crossfade(table([a.ptr() for a in ia], [b.ptr() for b in ib], [o.ptr() for o in outs], caps), 3, d, got, _st()), "rh_crossfade")
    assert list(got) == caps
    rows = [o.check() for o in outs]
    for a in ia + ib:
        a.unchanged()
    for k in range(3):
        assert same(rows[k], wants[k]), k
    pa, pb = [arena.plain(a) for (a, _, _), _ in shapes], [arena.plain(b) for _, (b, _, _) in shapes]
    pd = [arena.plain_dst(c) for c in caps]
    _lib.check(lib.rh_crossfade(table([p for _, p in pa], [p for _, p in pb], [p for _, p in pd], caps), 3, d, got, _st()), "rh_crossfade")
    for k in range(3):
        assert same(host(pd[k][0])[: caps[k]], rows[k]), k


# ---- rh_signal_generate, rh_chirp -----------------------------------------------------------------------------------------------------
def _phases(step, phase, n):
    """(phase + step).rem_euclid(1.0) in f32, one at a time (signal_generator.rs:137); phases are not negative here"""
    out = np.empty(n + 1, f32)
    p = f32(phase)
    for i in range(n + 1):
        out[i] = p
        p = f32(p + step)
        p = f32(p - np.floor(p))
    return out


def test_signal_generate_rows_states_and_functions(G):
    """5 generators of the four functions, rows of 1001 samples 1014 apart; the 10 state floats and the 5 function codes in arenas; a second
    call continues every stream."""
    from rodio_amd import _lib

    lib = _lib.lib
    rates, freqs, fns = [44100, 48000, 8000, 192000, 22050], [440.0, 20.0, 3999.0, 17.25, 30000.0], ["sine", "square", "sawtooth", "triangle", "square"]
    codes = np.array([{"sine": 0, "triangle": 1, "square": 2, "sawtooth": 3}[f] for f in fns], np.int32)
    n, ld, Sg = 1001, 1001 + 13, 5
    init = np.zeros(2 * Sg, f32)
    for g in range(Sg):
        _lib.check(lib.rh_signal_generator_init(init[2 * g:].ctypes.data_as(_lib.f32p), rates[g], freqs[g]), "rh_signal_generator_init")
    assert all(bits(init[2 * g])[0] == bits(phase_step(rates[g], freqs[g]))[0] for g in range(Sg))
    st, fn = arena.state_arena(2 * Sg, init), arena.src_arena(codes)
    import torch

    pst, pfn = torch.from_numpy(init.copy()).cuda(), torch.from_numpy(codes).cuda()
    ph = [_phases(init[2 * g], 0.0, 2 * n) for g in range(Sg)]
    for call in range(2):
        dst = arena.dst_arena_rows(Sg, n, ld)
        _lib.check(lib.rh_signal_generate(vp(dst.ptr()), ld, n, vp(st.ptr()), vp(fn.ptr()), Sg, _st()), "rh_signal_generate")
        rows = dst.check()
        fn.unchanged()
        state = st.check()
        pd, pdp = arena.plain_dst(Sg * ld)
        _lib.check(lib.rh_signal_generate(vp(pdp), ld, n, vp(pst.data_ptr()), vp(pfn.data_ptr()), Sg, _st()), "rh_signal_generate")
        assert same(host(pd)[: Sg * ld].reshape(Sg, ld)[:, :n], rows) and same(host(pst), state)
        for g in range(Sg):
            want = wave_ref(fns[g], ph[g][call * n: call * n + n])
            if fns[g] == "sine":
                err = float(np.max(np.abs(rows[g].astype(np.float64) - want)))
                assert err <= SINE_TOL, (g, err)
            else:
                assert same(rows[g], want), (call, g)
            assert bits(state[2 * g])[0] == bits(init[2 * g])[0] and bits(state[2 * g + 1])[0] == bits(ph[g][(call + 1) * n])[0], (call, g)


def test_chirp_writes_what_is_left_of_the_sweep(G):
    """first + n beyond total: *out_n samples are written, the rest of dst keeps the sentinel."""
    from rodio_amd import _lib

    lib = _lib.lib
    total, first, n = 48000, 47000, 1500
    dst = arena.dst_arena(n)
    m = C.c_uint64(0)
    _lib.check(lib.rh_chirp(vp(dst.ptr()), first, n, total, 48000, 20.0, 20000.0, C.byref(m), _st()), "rh_chirp")
    assert m.value == total - first
    row = dst.check(written=m.value)[: m.value]
    err = float(np.max(np.abs(row.astype(np.float64) - chirp_ref(48000, 20.0, 20000.0, total, first, m.value))))
    assert err <= SINE_TOL, err
    pd, pdp = arena.plain_dst(n)
    _lib.check(lib.rh_chirp(vp(pdp), first, n, total, 48000, 20.0, 20000.0, C.byref(m), _st()), "rh_chirp")
    assert same(host(pd)[: m.value], row)
    for f0, cnt in [(total, 10), (0, 999)]:  # nothing left; a whole block that ends inside a vector
        dst = arena.dst_arena(cnt)
        _lib.check(lib.rh_chirp(vp(dst.ptr()), f0, cnt, total, 48000, 20.0, 20000.0, C.byref(m), _st()), "rh_chirp")
        assert m.value == (0 if f0 == total else cnt)
        dst.check(written=m.value)


# ---- the two streaming handles --------------------------------------------------------------------------------------------------------
def test_resampler_blocks_with_exact_capacities(G, O):
    """3 channels, 96 -> 44.1 kHz, blocks of 1, 7 and 5000 frames, then an empty flush: dst_capacity_frames exactly what
    rh_resampler_pending_frames says; the frames rh_resampler_process reports are written and no others."""
    from rodio_amd import _lib

    lib = _lib.lib
    ch, frm, to = 3, 96000, 44100
    blocks = [1, 7, 5000, 0]
    x = np.random.default_rng(8).uniform(-1, 1, sum(blocks) * ch).astype(f32)
    ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()

    def run(plain):
        h = C.c_void_p()
        _lib.check(lib.rh_resampler_create(C.byref(h), frm, to, ch), "rh_resampler_create")
        parts, a = [], 0
        try:
            for k, b in enumerate(blocks):
                flush = int(k == len(blocks) - 1)
                blk = x[a * ch: (a + b) * ch]
                a += b
                cap, m = C.c_uint64(0), C.c_uint64(0)
                _lib.check(lib.rh_resampler_pending_frames(h, b, flush, C.byref(cap)), "rh_resampler_pending_frames")
                if plain:
                    (st, sp), (dt, dp) = arena.plain(blk if b else np.zeros(1, f32)), arena.plain_dst(cap.value * ch)
                    _lib.check(lib.rh_resampler_process(h, vp(dp), cap.value, vp(sp) if b else None, b, flush, C.byref(m), _st()), "rh_resampler_process")
                    parts.append(host(dt)[: m.value * ch])
                else:
                    src, dst = arena.src_arena(blk), arena.dst_arena(cap.value * ch)
                    _lib.check(lib.rh_resampler_process(h, vp(dst.ptr()), cap.value, vp(src.ptr()) if b else None, b, flush, C.byref(m), _st()), "rh_resampler_process")
                    assert m.value <= cap.value
                    parts.append(dst.check(written=m.value * ch)[: m.value * ch])
                    src.unchanged()
        finally:
            lib.rh_resampler_destroy(h)
        return np.concatenate(parts)

    got = run(False)
    assert same(got, ref)
    assert same(run(True), got)


@pytest.mark.parametrize("ch,delay,blocks", [(2, 2000, [14, 1998, 2002, 6010]), (1, 37, [7, 36, 38, 1]), (2, 4801, [300, 9602])])
def test_echo_blocks_shorter_and_longer_than_the_delay(G, O, ch, delay, blocks):
    from rodio_amd import _lib

    lib = _lib.lib
    ns = None
    for cand in range((delay * 10**9) // (48000 * ch) - 2, (delay * 10**9) // (48000 * ch) + 3):
        if int(lib.rh_delay_samples(cand, 48000, ch)) == delay:
            ns = cand
    assert ns is not None
    x = np.random.default_rng(delay).uniform(-0.25, 0.25, sum(blocks)).astype(f32)
    ref = O.TestSource(x, ch, 48000).reverb(ns, 0.3).collect()

    def run(plain):
        h = C.c_void_p()
        _lib.check(lib.rh_echo_create(C.byref(h), delay, 0.3), "rh_echo_create")
        parts, a = [], 0
        try:
            for b in blocks + [None]:
                n = delay if b is None else b
                if plain:
                    dt, dp = arena.plain_dst(n)
                else:
                    dst = arena.dst_arena(n)
                    dp = dst.ptr()
                if b is None:
                    _lib.check(lib.rh_echo_flush(h, vp(dp), _st()), "rh_echo_flush")
                else:
                    blk = x[a: a + b]
                    a += b
                    src = arena.plain(blk) if plain else arena.src_arena(blk)
                    _lib.check(lib.rh_echo_process(h, vp(dp), vp(src[1] if plain else src.ptr()), b, _st()), "rh_echo_process")
                    if not plain:
                        src.unchanged()
                parts.append(host(dt)[:n] if plain else dst.check())
        finally:
            lib.rh_echo_destroy(h)
        return np.concatenate(parts)

    got = run(False)
    assert same(got, ref)
    assert same(run(True), got)
