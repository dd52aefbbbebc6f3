"""rodio_hip.h's first contract -- "every function enqueues on `stream`", and for host tables "read before the call returns" -- on a
non-blocking side stream that is backed up behind a gate (tests/stream_gate.py, which spells out the six steps and what each catches).
Every other GPU test passes the legacy null stream, which serialises with everything: a helper launch on stream 0, a host table read late
or a staging slot rewritten too early cannot fail there.

A  the compute entries that take a stream (CASES and ALIGNED), each once, gated, through the C ABI, at the smallest shape that reaches the vector route and a ragged tail
   (4099 samples at the leads (0, 0) and (3, 2); two whole tiles plus 3 frames for the tile kernels), against the reference and the
   tolerance of the entry's own arena / parity test (imported, not restated): the one-row effects, one rh_convert_* per kernel template
   either way, rh_wav_decode(_channels), rh_resample_linear, rh_channels_convert, rh_uniform_row / _segments / _segments_dev, rh_mix_sum,
   rh_mix_pair, rh_crossfade, rh_chirp, rh_signal_generate, rh_noise_generate, the three *_steps entries, rh_biquad modes 0 and 1,
   rh_limit and rh_agc with and without a carried state, rh_reverb_spatial, rh_echo_process / _flush, rh_resampler_process, the wide,
   filtered and spatial mixer blocks (33 sources), rh_rlm_run / _run_subset / _run_batch, rh_rlm_set_sources_pcm16 + run on its native
   and its converted route, rh_rlm_stream_block(_v) with the overlap off, and the copies (rh_memset, rh_memcpy_h2d, _h2d_rows, _d2h, _d2h_async,
   _d2d); three of them also on a stream of rh_stream_create.  Not here: rh_rlm_stream_overlap (it declares the opposite contract);
   rh_allreduce_sum_f32, rh_reduce_sum_f32 and rh_comm_* (multi-GPU); rh_stream_synchronize, rh_rlm_autotune, handle creation and the
   rh_rlm_* setters other than rh_rlm_set_sources_pcm16 (they wait by contract and compute nothing); the event entries.
B  nine calls behind one gate, each with its own host table and destination: rh_mix_sum, rh_amplify_steps, rh_biquad_steps,
   rh_uniform_segments, rh_wide_mix_block_filtered, rh_spatial_mix_block, and the two entries that stage their tables in rings of four
   page-locked slots, rh_crossfade and rh_rlm_stream_block_v: calls 1-4 return while the gate is pending, call 5 waits for slot 1's copy.
C  40 rh_biquad mode-1 calls with 40 cutoffs behind one gate: the plan cache (32 plans) evicts plans whose launches are still queued.
D  the shared per-stream scratch: limiter, noise, biquad, AGC and crossfade interleaved on one gated stream with a call that makes the
   scratch grow in their middle; the same on two gated streams call by call; and two host threads on one gated stream.
E  the control: a test-side copy issued on the null stream instead of the gated one fails the checker; on the gated one it passes.

The gate: GATE_FACTOR times SLOWEST_HOST_MS per call (profiles/stream_order.txt holds the measurement behind both).  `pending` is
asserted for every call of A, B and D but those WAITS names, each with the header line that says it waits."""
import ctypes as C
import threading
import time

import numpy as np
import pytest
from conftest import knobs

import arena
import fallback_cases as FC
import stream_gate
import test_gpu_arena_formats as AFo
import test_gpu_arena_fused as AF
import test_gpu_arena_mixers as AM
import test_gpu_live_filter as LF
import test_gpu_pcm16 as P16
import test_gpu_spatial_mix as SM
from filter_signals import RATE as FS_RATE
from filter_signals import criteria, l1_gain, scan_ok, truth
from test_gpu_arena_rows import (LEADS, TAKE_RATE, _elementwise_ops, _entries, _first, _noise_states, _table, _take_cases,
                                 held, layout_frames, resample_tile_frames, signal)
from test_gpu_arena_scan import AGC_KW, LIMIT_KW, TOL_EFFECTS, TOL_LIMIT, _agc_state, _biquad, _biquad_state_ok, _delay_ns, _limit, _reverb_spatial, close
from test_gpu_effects import _programme, rnd
from test_gpu_limit import _signal as limit_signal
from test_gpu_live import amplify_ref, channel_volume_ref
from test_mix_cpu import MS, crossfade_restated, mix_rows
from test_mix_cpu import signal as mix_signal
from test_noise_cpu import EXACT, GAUSS_TOL, INTEGRATOR_TOL, INTEGRATORS, KINDS, hash_, idx, integrator_consts, recurrence_f64, reference, u1

pytestmark = pytest.mark.gpu
f32 = np.float32
bits = arena.bits

N = 4099  # the row entries: 1024 whole vectors and a ragged one, more than one workgroup
GATED_LEADS = [LEADS[0], LEADS[3]]  # (0, 0): the 16-byte routes; (3, 2): neither side on a boundary
assert GATED_LEADS == [(0, 0), (3, 2)]

# profiles/stream_order.txt: SLOWEST_HOST_MS is the longest host time of a warmed call of the case lists that does not wait, rounded up
# with room for the scatter of a host time (the report at the end of the file prints the one of the run: rh_rlm_set_sources_pcm16 with its
# run on the converted route, or rh_uniform_segments, whose 35-segment table the case builds inside the timed call); a gate
# lasts GATE_FACTOR times that for every call queued behind it, plus the restores and the snapshots of the case.
SLOWEST_HOST_MS = 0.3
GATE_FACTOR = 70  # 21 ms a call

# Entries that wait for the stream by contract, each with the line of rodio_hip.h that says so: `pending` is not asserted for them.
WAITS = {
    "rh_rlm_set_sources_pcm16 on a handle that has run": "On a handle that has run, rh_rlm_set_sources and rh_rlm_set_sources_pcm16 wait until everything the handle has queued on its stream has completed.",
    "rh_memcpy_d2h": "Waits until `stream` has run the copy: the host block holds the data when the call returns.",
    "rh_memcpy_h2d_rows": "From a pageable block this call waits until `stream` has run everything queued before it (the runtime's pitched copy does).",
}


def gate_ms(calls=1):
    return GATE_FACTOR * SLOWEST_HOST_MS * max(1, calls)


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


@pytest.fixture(scope="module")
def delay(G):
    return stream_gate.Delay()


@pytest.fixture(scope="module")
def side(G):
    import torch

    return torch.cuda.Stream()  # non-blocking (test_gpu_race.py): it does not wait for the null stream, nor the null stream for it


FILE_LIMIT_S = 120.0  # the whole file takes about 10 s; a machine on which it takes twelve times that is not measuring what the gate assumes


@pytest.fixture(scope="module")
def started():
    return time.monotonic()


@pytest.fixture(autouse=True)
def within_the_files_time_limit(started):
    """The file's budget: once it is spent every remaining case fails at once instead of queueing more gates.  It is checked between
    cases, so it cannot end a call that hangs: that takes a limit from outside, `timeout -k 10 300 python -m pytest ...` as
    profiles/README.md runs the file."""
    spent = time.monotonic() - started
    assert spent < FILE_LIMIT_S, f"test_gpu_stream_order.py has run for {spent:.0f} s, its limit is {FILE_LIMIT_S:.0f} s"


RAN = {}  # group -> gated cases that ran (profiles/stream_order.txt)
SLOWEST = [0.0, ""]  # the longest host time of a call that returned while its gate was pending, and the case it belongs to


def gated(build, stream, delay, group, name, calls=1, exempt=()):
    """One gated case: run, report, assert `pending` for every call whose index is not in `exempt`, then the case's own check."""
    r = stream_gate.run(build, stream, delay, gate_ms(calls))  # (a case of several calls under A: the handles' block sequences, a few calls)
    RAN[group] = RAN.get(group, 0) + 1
    print(f"[stream_order {group} {name}] gate {r.reps} x {delay.fill_ms:.3f} ms, pending {''.join('1' if p else '0' for p in r.pending)}"
          f" queued {int(r.queued)}, host ms max {max(r.host_ms):.3f}")
    for ms, p in zip(r.host_ms, r.pending):
        if p and ms > SLOWEST[0]:
            SLOWEST[:] = [ms, f"{group} {name}"]
    if name not in WAITS:
        late = [i for i, p in enumerate(r.pending) if not p and i not in exempt]
        assert not late, (name, "returned after the gate had opened: the call waited for the stream, or the gate is too short", late, r.host_ms)
    r.check()
    return r


def _st():
    from rodio_amd import source

    return source._stream()  # the current stream: the gated one while a case's calls run


def L():
    from rodio_amd import _lib

    return _lib.lib


def vp(a):
    return C.c_void_p(a) if a is not None else None


def ok(status, tag):
    assert status == 0, (tag, status)


# ================================================================================================================ A: the cases ====
def row_case(k, x, out_len, ref, ls, ld, fn, tol=0.0, written=None):
    """fn(dst, src) -> the count the entry reports (None: all out_len): x between poison, dst between sentinels, as test_gpu_arena_rows.one_row"""
    src, dst, seen = k.src(x, ls), k.dst(out_len, ld), {}

    def call():
        m = fn(dst.ptr(), src.ptr())
        seen["m"] = out_len if m is None else m

    def check():
        m = seen["m"]
        assert written is None or m == written, (m, written)
        got = dst.check_snapshot(m)[:m]
        src.snapshot_unchanged()
        good, why = held(got, ref, tol)
        assert good, why

    return stream_gate.case([call], check)


def elementwise(name):
    def build(k, O, G, ls, ld):
        x = signal(N, N)
        fn, ref, tol = _elementwise_ops(O, x)[name]
        return row_case(k, x, N, ref, ls, ld, fn, tol)

    return build


def delay_like(name):
    def build(k, O, G, ls, ld):
        lib, D = L(), 37
        x = signal(100 + N, N, 0.25)
        ns = D * 1_000_000
        if name == "delay":
            return row_case(k, x, N + D, O.TestSource(x, 1, 1000).delay(ns).collect(), ls, ld, lambda d, s: ok(lib.rh_delay(vp(d), vp(s), N, D, _st()), name))
        return row_case(k, x, N + D, O.TestSource(x, 1, 1000).reverb(ns, 0.7).collect(), ls, ld, lambda d, s: ok(lib.rh_echo_mix(vp(d), vp(s), N, D, 0.7, _st()), name))

    return build


def take_duration(k, O, G, ls, ld):
    """the duration ends inside a frame: the pad store of workgroup 0 behind the samples"""
    lib, ch = L(), 3
    x = signal(200 + N + ch, N)
    _, cases = _take_cases(N, ch)
    K, ns = cases[0]
    ref = O.TestSource(x, ch, TAKE_RATE).take_duration(ns, True).collect()

    def fn(d, s):
        m, e = C.c_uint64(0), C.c_int32(-1)
        ok(lib.rh_take_duration(vp(d), vp(s), N, 0, ch, TAKE_RATE, ns, 1, C.byref(m), C.byref(e), _st()), "take")
        assert e.value == 1
        return m.value

    return row_case(k, x, N + ch, ref, ls, ld, fn, written=ref.size)


def take_duration_from(k, O, G, ls, ld):
    """the same from the state try_seek leaves (test_take_duration_rows: two frames of the duration gone, frame position 0)"""
    lib, ch = L(), 3
    x = signal(200 + N + ch, N)
    dps, cases = _take_cases(N, ch)
    K, ns = cases[0]
    pos = 2 * ch * dps
    ref = O.TestSource(x, ch, TAKE_RATE).take_duration_sought(ns, pos, True).collect()

    def fn(d, s):
        m, e, r = C.c_uint64(0), C.c_int32(-1), C.c_uint64(0)
        ok(lib.rh_take_duration_from(vp(d), vp(s), N, ns - pos, ns, 0, ch, TAKE_RATE, 1, C.byref(m), C.byref(e), C.byref(r), _st()), "take_from")
        assert r.value == ns - pos - min(N, (ns - pos) // dps) * dps
        return m.value

    return row_case(k, x, N + ch, ref, ls, ld, fn, written=ref.size)


def channels(name):
    def build(k, O, G, ls, ld):
        from rodio_amd import _lib

        lib, (in_ch, out_ch) = L(), (6, 2)
        frames = layout_frames(in_ch, out_ch)[-1]  # two whole tiles plus 3 frames
        x = signal(in_ch * 1000 + frames, frames * in_ch)
        gains = np.linspace(0.2, 1.1, out_ch).astype(f32)
        if name == "channels_convert":
            ref = O.ChannelCountConverter(O.TestSource(x, in_ch, 48000), in_ch, out_ch).collect()
            return row_case(k, x, frames * out_ch, ref, ls, ld, lambda d, s: ok(lib.rh_channels_convert(vp(d), vp(s), frames, in_ch, out_ch, _st()), name))
        ref = O.ChannelVolume(O.TestSource(x, in_ch, 48000), gains).collect()

        def fn(d, s):
            g = k.host(gains.copy())  # a host array: garbage as soon as the call has returned
            ok(lib.rh_channel_volume(vp(d), vp(s), frames, in_ch, g.ctypes.data_as(_lib.f32p), out_ch, _st()), name)

        return row_case(k, x, frames * out_ch, ref, ls, ld, fn)

    return build


def amplify_steps(k, O, G, ls, ld, seed=0, n=N):
    lib, period = L(), 441
    first = _first(period)
    x = signal(period + n + seed, n)
    kk = _entries(first, period, n)
    fac = _table(period * 7 + n + seed, kk)
    tab = k.src(fac, 1)
    c = row_case(k, x, n, amplify_ref(x, first, period, fac), ls, ld, lambda d, s: ok(lib.rh_amplify_steps(vp(d), vp(s), n, first, period, vp(tab.ptr()), kk, _st()), "amplify_steps"))
    inner = c.check

    def check():
        inner()
        tab.snapshot_unchanged()

    c.check = check
    return c


def channel_volume_steps(k, O, G, ls, ld):
    lib, (in_ch, out_ch), (gp, fp) = L(), (6, 2), (441, 480)
    first, ff = _first(gp), _first(fp) + 1
    frames = layout_frames(in_ch, out_ch)[-1]
    total = frames * out_ch
    x = signal(in_ch + frames + gp, frames * in_ch)
    kg, kf = _entries(first, gp, total), _entries(ff, fp, total)
    g, fac = _table(gp + frames, kg, out_ch), _table(fp + frames, kf)
    gt, ft = k.src(g, 1), k.src(fac, 3)
    ref = channel_volume_ref(x, in_ch, out_ch, first, gp, g, ff, fp, fac)
    return row_case(k, x, total, ref, ls, ld,
                    lambda d, s: ok(lib.rh_channel_volume_steps(vp(d), vp(s), frames, in_ch, out_ch, first, gp, vp(gt.ptr()), kg, ff, fp, vp(ft.ptr()), kf, _st()), "cvs"))


def resample_linear(k, O, G, ls, ld):
    lib, (frm, to, ch, span) = L(), (44100, 48000, 2, 0)
    tf, F, T = resample_tile_frames(frm, to, ch, span)
    frames = -(-(2 * tf + 3) * F // T) + 1  # two whole tiles of output plus 3 frames
    m = C.c_uint64(0)
    ok(lib.rh_resample_out_frames(frames, frm, to, ch, span, C.byref(m)), "out_frames")
    assert 2 * tf < m.value <= 3 * tf
    x = signal(frames + ch, frames * ch)
    ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
    assert ref.size == m.value * ch
    return row_case(k, x, m.value * ch, ref, ls, ld, lambda d, s: ok(lib.rh_resample_linear(vp(d), vp(s), frames, frm, to, ch, span, _st()), "resample"))


def mix_sum(k, O, G, ls, ld, seed=0, out_len=N):
    """test_mix_sum_rows_anywhere's sources (k_mix_sum_any) at leads (3, 2), test_mix_sum_aligned_starts' (k_mix_sum_v4) at (0, 0); `seed`
    moves the starts and the lengths (B: nine different tables)"""
    lib = L()
    if (ls, ld) == (0, 0):
        srcs = [signal(1 + seed, out_len), signal(2 + seed, out_len // 4 + 3 + 4 * seed), signal(3 + seed, out_len - 1), signal(4 + seed, 5 + seed), signal(5 + seed, out_len // 2 - 50)]
        starts, leads = [0, 4 + 4 * seed, 0, out_len - 7 - (out_len - 7) % 4 - 4 * seed, (out_len // 4) & ~3], [0]
    else:
        srcs = [signal(1 + seed, out_len), signal(2 + seed, out_len - 2 - seed), signal(3 + seed, out_len // 2 + 1 + seed), signal(4 + seed, 3), signal(5 + seed, out_len - 6)]
        starts, leads = [0, 2 + seed, 1, out_len - 3, 6], [1, 0, 3, 2, 1]
    n = len(srcs)
    ars = [k.src(x, leads[i % len(leads)]) for i, x in enumerate(srcs)]
    dst = k.dst(out_len, ld)
    ref = FC.ref_mix(srcs, starts, out_len)

    def call():
        ptrs = k.host((C.c_void_p * n)(*[a.ptr() for a in ars]), k.pit())  # late readers: NaN from the pit, never another row
        st = k.host((C.c_uint64 * n)(*starts), 0)
        ln = k.host((C.c_uint64 * n)(*[len(x) for x in srcs]), 4)
        ok(lib.rh_mix_sum(vp(dst.ptr()), out_len, ptrs, st, ln, n, _st()), "mix_sum")

    def check():
        got = dst.check_snapshot()
        for a in ars:
            a.snapshot_unchanged()
        good, why = held(got, ref)
        assert good, why

    return stream_gate.case([call], check)


def mix_pair(k, O, G, ls, ld):
    lib, na, nb = L(), 1027, N
    a, b = signal(na + 1, na), signal(nb + 2, nb)
    aa, bb, dst = k.src(a, ls), k.src(b, (ls + 1) % 4), k.dst(nb, ld)

    def check():
        good, why = held(dst.check_snapshot(), mix_rows(a, b))
        assert good, why
        aa.snapshot_unchanged()
        bb.snapshot_unchanged()

    return stream_gate.case([lambda: ok(lib.rh_mix_pair(vp(dst.ptr()), vp(aa.ptr()), na, vp(bb.ptr()), nb, _st()), "mix_pair")], check)


def noise_generate(k, O, G, ls, ld):
    """every kind in one call plus WhiteGaussian of Brownian's seed, as test_noise_generate_rows; the states in a state arena"""
    lib, n = L(), N
    kinds = KINDS + ["white_gaussian"]
    rates = [44100, 48000, 8000, 192000, 22050, 44100, 48000, 96000, 44100, 48000]
    seeds = list(range(40, 49)) + [40 + KINDS.index("brownian")]
    ldim = n + 13
    init = _noise_states(kinds, rates, seeds, 3000)
    states, dst = k.state(init.size, init.view(f32)), k.dst_rows(len(kinds), n, ldim, ld)

    def check():
        y = dst.check_snapshot().reshape(len(kinds), n)
        after = states.check_snapshot(dtype=np.uint32).reshape(len(kinds), 8)
        assert np.all((after[:, 2].astype(np.uint64) | (after[:, 3].astype(np.uint64) << np.uint64(32))) == np.uint64(n))
        assert np.array_equal(after[:, [0, 1, 4, 5, 6]], init[:, [0, 1, 4, 5, 6]])
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
            assert good, (kind, why)

    return stream_gate.case([lambda: ok(lib.rh_noise_generate(vp(dst.ptr()), ldim, n, vp(states.ptr()), len(kinds), _st()), "noise_generate")], check)


def limit(with_state, frames=N, ch=1, kw=LIMIT_KW[1], seed=0):
    def build(k, O, G, ls, ld):
        from rodio_amd import _lib

        x = limit_signal(100 * ch + seed, frames, ch)
        src, dst = k.src(x, ls), k.dst(frames * ch, ld)
        st = k.state(2 * ch) if with_state else None
        ref = O.TestSource(x, ch, 48000).limit(**kw).collect()

        def check():
            good, err = close(dst.check_snapshot(), ref, TOL_LIMIT)
            assert good, err
            src.snapshot_unchanged()
            if st:
                state = st.check_snapshot()
                assert np.all(np.isfinite(state)) and np.all(state >= 0.0), state

        def call():  # _limit's call with params_host in the case's hands: garbage as soon as the call has returned
            p = k.host(_lib.LimitParams(kw.get("threshold", -1.0), kw.get("knee_width", 4.0), kw.get("attack_ns", 5_000_000), kw.get("release_ns", 100_000_000)))
            _lib.check(_lib.lib.rh_limit(vp(dst.ptr()), vp(src.ptr()), frames, ch, 48000, 1, C.byref(p), vp(st.ptr() if st else None), _st()), "rh_limit")

        return stream_gate.case([call], check)

    return build


def biquad(mode, with_state, frames=N, ch=2, freq=200, seed=0):
    def build(k, O, G, ls, ld):
        x = rnd(200 + 7 * ch + seed, frames * ch, 0.4)
        co = G.biquad_coeffs("low_pass", freq, 0.5, 48000)
        src, dst = k.src(x, ls), k.dst(frames * ch, ld)
        st = k.state(4 * ch) if with_state else None
        ref = O.TestSource(x, ch, 48000).low_pass(freq).collect()

        def call():
            _biquad(dst.ptr(), src.ptr(), frames, ch, 1, k.host(co.copy()), mode, st.ptr() if st else None)

        def check():
            got = dst.check_snapshot()
            src.snapshot_unchanged()
            if mode == 0:
                assert np.array_equal(bits(got), bits(ref))
            else:
                good, err = close(got, ref, TOL_EFFECTS)
                assert good, err
            if st:
                _biquad_state_ok(st.check_snapshot(), [x], [ref], ch, 0.0 if mode == 0 else TOL_EFFECTS)

        return stream_gate.case([call], check)

    return build


def agc(with_state, n=N, kw=AGC_KW[1], seed=0):
    def build(k, O, G, ls, ld):
        from rodio_amd import _lib

        x = _programme(700 + seed, n + 8)[:n]
        src, dst = k.src(x, ls), k.dst(n, ld)
        st = None
        if with_state:
            st = k.state(_agc_state())
            _lib.check(_lib.lib.rh_agc_state_init(vp(st.ptr()), 1, _st()), "rh_agc_state_init")  # before the case is staged: the initial state
        ref = O.TestSource(x, 1, 48000).automatic_gain_control(**kw).collect()

        def check():
            got = dst.check_snapshot()
            src.snapshot_unchanged()
            good, err = close(got, ref, TOL_EFFECTS)
            assert good and arena.same(got, ref), err  # test_agc_rows_and_states: on these rows every sample is the reference's
            if st:
                assert np.all(np.isfinite(st.check_snapshot()))

        def call():  # _agc's call with params_host in the case's hands
            p = k.host(_lib.AgcParams(kw.get("target_level", 1.0), kw.get("attack_ns", 4_000_000_000), kw.get("release_ns", 0), kw.get("absolute_max_gain", 7.0), kw.get("floor", 0.0)))
            _lib.check(_lib.lib.rh_agc(vp(dst.ptr()), vp(src.ptr()), n, 48000, 1, C.byref(p), vp(st.ptr() if st else None), _st()), "rh_agc")

        return stream_gate.case([call], check)

    return build


def reverb_spatial(k, O, G, ls, ld):
    from rodio_amd import _lib

    S, n, d = 3, 2000, 37
    ns = _delay_ns(d)
    xs = [rnd(40 + s, n, 0.25) for s in range(S)]
    em = [[0.5 + 0.01 * s, 0, 1] for s in range(S)]
    gains = np.stack([G.spatial_gains(e, [-1, 0, 0], [1, 0, 0]) for e in em]).astype(f32)
    n_out = 2 * ((n + d) // 2)
    ss, ds = (n + 3) // 4 * 4 + 8, (n_out + 3) // 4 * 4 + 8
    src, dst, g = k.src_rows(xs, ss), k.dst_rows(S, n_out, ds), k.state(2 * S, gains)

    def check():
        rows = dst.check_snapshot().reshape(S, n_out)
        src.snapshot_unchanged()
        g.snapshot_unchanged()
        for s in range(S):
            ref = O.Spatial(O.TestSource(xs[s], 2, 48000).reverb(ns, 0.3), em[s], [-1, 0, 0], [1, 0, 0]).collect()
            assert len(ref) == n_out and np.array_equal(bits(rows[s]), bits(ref)), s

    return stream_gate.case([lambda: _lib.check(_reverb_spatial(dst.ptr(), src.ptr(), n, d, 0.3, g.ptr(), S, ss, ds), "rh_reverb_spatial")], check)


CF_D = 50 * MS + 10_416  # test_crossfade_three_pairs_one_call's duration: 4801 samples of a stereo 48 kHz `a`
CF_FUSED = lambda s: ((mix_signal(6000, 41 + s), 1, 44100), (mix_signal(3000, 42 + s), 1, 48000))  # noqa: E731
CF_COMPOSED = lambda s: ((mix_signal(6000, 43 + s), 2, 48000), (mix_signal(18000, 44 + s), 6, 48000))  # noqa: E731  a 6-channel b: the composed route
CF_CUT = lambda s: ((mix_signal(6000, 45 + s), 2, 48000), (mix_signal(3000, 46 + s), 1, 44100))  # noqa: E731  the duration ends inside a frame


def crossfade_call(k, O, shapes, d=CF_D):
    """One rh_crossfade call over `shapes` -> (call, check): sources between poison, every capacity exactly rh_crossfade_out_samples()."""
    from rodio_amd import _lib

    lib, W, n = _lib.lib, _lib.CROSSFADE_PAIR_WORDS, len(shapes)
    wants = [crossfade_restated(O, O.TestSource(*a), O.TestSource(*b), d) for a, b in shapes]
    ia, ib = [k.src(a) for (a, _, _), _ in shapes], [k.src(b) for _, (b, _, _) in shapes]
    outs = [k.dst(w.size) for w in wants]

    def call():
        pairs = k.host((C.c_uint64 * (W * n))(), 0)  # zeros behind the return: a late reader finds pairs of no channels
        for i, ((a, ca, ra), (b, cb, rb)) in enumerate(shapes):
            pairs[W * i: W * i + W] = [ia[i].ptr(), a.size, ca, ra, ib[i].ptr(), b.size, cb, rb, 0, outs[i].ptr(), wants[i].size]
        got = (C.c_uint64 * n)()
        _lib.check(lib.rh_crossfade(pairs, n, d, got, _st()), "rh_crossfade")
        assert list(got) == [w.size for w in wants]  # written before the call returns

    def check():
        for i in range(n):
            assert arena.same(outs[i].check_snapshot(), wants[i]), i
        for a in ia + ib:
            a.snapshot_unchanged()

    return call, check


def crossfade_of(shapes_of, d=CF_D):
    def build(k, O, G, ls, ld):
        call, check = crossfade_call(k, O, shapes_of(), d)
        return stream_gate.case([call], check)

    return build


crossfade = crossfade_of(lambda: [CF_FUSED(0), CF_COMPOSED(0), CF_CUT(0)])  # test_crossfade_three_pairs_one_call's batch


def copies(name):
    """rh_memset, rh_memcpy_d2d, rh_memcpy_h2d (a pageable host block), rh_memcpy_h2d_rows, rh_memcpy_d2h_async (a page-locked block of rh_host_alloc)"""

    def build(k, O, G, ls, ld):
        lib = L()
        x = signal(7, N)
        if name == "memset":
            dst = k.dst(N, ld)

            def check():
                assert np.all(dst.check_snapshot(dtype=np.uint32) == 0x3C3C3C3C)

            return stream_gate.case([lambda: ok(lib.rh_memset(vp(dst.ptr()), 0x3C, 4 * N, _st()), name)], check)
        if name == "memcpy_d2d":
            return row_case(k, x, N, x, ls, ld, lambda d, s: ok(lib.rh_memcpy_d2d(vp(d), vp(s), 4 * N, _st()), name))
        if name == "memcpy_h2d":
            dst = k.dst(N, ld)

            def check():
                assert arena.same(dst.check_snapshot(), x)

            return stream_gate.case([lambda: ok(lib.rh_memcpy_h2d(vp(dst.ptr()), vp(k.host(x.copy()).ctypes.data), 4 * N, _st()), name)], check)
        if name.startswith("memcpy_h2d_rows"):
            rows, width, pitch = 3, 1001, 1024  # floats: the 23 behind every row keep the sentinel on the device
            data = np.zeros((rows, pitch), f32)
            data[:, :width] = signal(8, rows * width).reshape(rows, width)
            dst = k.dst_rows(rows, width, pitch, ld)
            if name == "memcpy_h2d_rows":  # a pageable block: read before the call returns, garbage behind it
                call, free = (lambda: ok(lib.rh_memcpy_h2d_rows(vp(dst.ptr()), vp(k.host(data.copy()).ctypes.data), 4 * pitch, 4 * width, rows, _st()), name)), None
            else:  # a page-locked block, as the pull shim's staging ring: the caller's until the stream has reached the copy
                hp = C.c_void_p()
                ok(lib.rh_host_alloc(C.byref(hp), data.nbytes), "rh_host_alloc")
                np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_float)), data.shape)[:] = data
                call, free = (lambda: ok(lib.rh_memcpy_h2d_rows(vp(dst.ptr()), hp, 4 * pitch, 4 * width, rows, _st()), name)), (lambda: ok(lib.rh_host_free(hp), "rh_host_free"))

            def check():
                try:
                    assert arena.same(dst.check_snapshot(), data[:, :width])
                finally:
                    if free:
                        free()

            return stream_gate.case([call], check)
        if name == "memcpy_d2h":  # it waits (WAITS): the block is whole when the call returns, whatever is queued in front of it
            src, block = k.src(x, ls), np.full(N, np.nan, f32)

            def call():
                ok(lib.rh_memcpy_d2h(vp(block.ctypes.data), vp(src.ptr()), 4 * N, _st()), name)
                assert arena.same(block, x)

            return stream_gate.case([call], src.snapshot_unchanged)
        assert name == "memcpy_d2h_async"
        src = k.src(x, ls)
        hp = C.c_void_p()
        ok(lib.rh_host_alloc(C.byref(hp), 4 * N), "rh_host_alloc")
        block = np.ctypeslib.as_array(C.cast(hp, C.POINTER(C.c_float)), (N,))

        def call():
            block[:] = np.nan
            ok(lib.rh_memcpy_d2h_async(hp, vp(src.ptr()), 4 * N, _st()), name)

        def check():
            try:
                assert arena.same(block, x)  # the stream is synchronised: the block holds the row as it was behind the gate
                src.snapshot_unchanged()
            finally:
                ok(lib.rh_host_free(hp), "rh_host_free")

        return stream_gate.case([call], check)

    return build


# ---- the mixers' host tables ----
def wide_mix_block(filtered_mode=None):
    """test_wide_mix_block / test_wide_mix_block_filtered at M = 1000: the WideSrc table, and for the filtered entry the kinds, the
    coefficients and the table of state addresses, are host arrays"""

    def build(k, O, G, ls, ld, seed=0):
        from rodio_amd import _lib

        to_ch, to_rate, M = 6, 48000, 1000 - 4 * seed
        if filtered_mode is None:
            specs = [(6, 44100, 1.0, "live"), (2, 44100, 0.5, "live"), (1, 48000, -1.5, "ended"), (to_ch, to_rate, 1.0, "live"), (3, 11025, 2.0, "silent")]
            srcs = AM._wide_sources(to_rate, M, specs, 600 + to_ch + M)
            want = AM.wide_oracle([(x, ch, rate, gain) for x, ch, rate, gain, _, _ in srcs], to_ch, to_rate)[: M * to_ch]
        else:
            specs = [(6, 44100, 1.0, "live"), (2, 44100, 0.5, "live"), (1, 48000, -1.5, "ended"), (6, 48000, 0.25, "live")]
            filts = [("lp", 1000, 0.5), None, ("hp", 2000, 0.5), None]
            srcs = AM._wide_sources(to_rate, M, specs, 4200 + M + seed)
            want = AM.filtered_oracle([(x, ch, rate, gain, f) for (x, ch, rate, gain, _, _), f in zip(srcs, filts)], to_ch, to_rate)[: M * to_ch]
            need = C.c_uint64(0)
            _lib.check(_lib.lib.rh_wide_mix_filtered_scratch_bytes(to_ch, M, 2, C.byref(need)), "rh_wide_mix_filtered_scratch_bytes")
            sts = [None if f is None else k.state(4 * to_ch) for f in filts]
            scr = k.dst(need.value // 4)
        assert want.size == M * to_ch
        n = len(srcs)
        ins, dst = [k.src(x) for x, *_ in srcs], k.dst(M * to_ch)

        def call():
            table = k.host(AM._wide_table(srcs, [a.ptr() for a in ins]), 0)  # zeros: sources of no frames
            if filtered_mode is None:
                _lib.check(_lib.lib.rh_wide_mix_block(vp(dst.ptr()), to_ch, to_rate, M, table, n, _st()), "rh_wide_mix_block")
                return
            kinds = k.host((C.c_int32 * n)(*[-1 if f is None else {"lp": 0, "hp": 1}[f[0]] for f in filts]), -1)
            co = np.zeros((n, 5), f32)
            for i, f in enumerate(filts):
                if f is not None:
                    co[i] = G.biquad_coeffs(kinds[i], f[1], f[2], to_rate)
            st = k.host((C.c_void_p * n)(*[s.ptr() if s else None for s in sts]), k.pit())
            _lib.check(_lib.lib.rh_wide_mix_block_filtered(vp(dst.ptr()), to_ch, to_rate, M, table, n, kinds, k.host(co).ctypes.data_as(_lib.f32p), st, filtered_mode, vp(scr.ptr()),
                                                           need.value, _st()), "rh_wide_mix_block_filtered")

        def check():
            row = dst.check_snapshot()
            for a in ins:
                a.snapshot_unchanged()
            if filtered_mode is None or filtered_mode == 0:
                assert arena.same(row, want)
            else:  # test_wide_mix_block_filtered: 1e-5 |gain| a filtered source of |x| <= 1
                bound = 1e-5 * sum(abs(g) for (_, _, _, g, _, _), f in zip(srcs, filts) if f is not None)
                err = float(np.max(np.abs(row.astype(np.float64) - want.astype(np.float64))))
                assert err <= bound, (err, bound)
            if filtered_mode is not None:
                arena.check_guards(scr.snapshot(), scr.layout)
                assert all(np.all(np.isfinite(s.check_snapshot())) for s in sts if s)

        return stream_gate.case([call], check)

    return build


def uniform_segments(k, O, G, ls, ld, seed=0):
    """test_uniform_segments, case 4 (22.05 kHz stereo -> 48 kHz mono in spans of 512 samples, every span cut once): a host table"""
    from rodio_amd import _lib

    lib = _lib.lib
    ch, rate, to_ch, to_rate, frames, span = AM.UNIFORM_CASES[4]
    frames -= 16 * seed
    x = (np.random.default_rng(900 + 4 + seed).uniform(-1, 1, frames * ch)).astype(f32)
    ref = O.UniformSourceIterator(O.SpanSource(x, ch, rate, span), to_ch, to_rate).collect()
    src, dst = k.src(x), k.dst(ref.size)

    def call():
        table, total = AM._segments(lib, x, ch, rate, to_ch, to_rate, span, 0.5, src.ptr(), dst.ptr())
        assert total * to_ch == ref.size
        _lib.check(lib.rh_uniform_segments(k.host(table, 0), len(table), _st()), "rh_uniform_segments")  # zeros: segments of no frames

    def check():
        assert arena.same(dst.check_snapshot(), ref)
        src.snapshot_unchanged()

    return stream_gate.case([call], check)


def uniform_segments_dev(k, O, G, ls, ld):
    """the same table on the device (test_gpu_uniform._convert's dev_table): between two byte fills, arriving behind the gate like a source"""
    from rodio_amd import _lib

    lib = _lib.lib
    ch, rate, to_ch, to_rate, frames, span = AM.UNIFORM_CASES[4]
    x = (np.random.default_rng(904).uniform(-1, 1, frames * ch)).astype(f32)
    ref = O.UniformSourceIterator(O.SpanSource(x, ch, rate, span), to_ch, to_rate).collect()
    src, dst = k.src(x), k.dst(ref.size)
    table, total = AM._segments(lib, x, ch, rate, to_ch, to_rate, span, 0.5, src.ptr(), dst.ptr())
    assert total * to_ch == ref.size
    tab = k.add(arena.src_bytes_arena(np.frombuffer(bytes(table), np.uint8).copy()))
    most = max(t.m1 - t.m0 for t in table)

    def check():
        assert arena.same(dst.check_snapshot(), ref)
        src.snapshot_unchanged()
        tab.snapshot_unchanged()

    return stream_gate.case([lambda: _lib.check(lib.rh_uniform_segments_dev(vp(tab.ptr()), len(table), most, _st()), "rh_uniform_segments_dev")], check)


def uniform_row(k, O, G, ls, ld):
    from rodio_amd import _lib

    n, fc, fr, tc, tr, span = 30000, 6, 48000, 1, 8000, 1000  # test_uniform_row: every chain ends inside a frame
    x = mix_signal(n, 57)
    ref = O.UniformSourceIterator(O.SpanSource(x, fc, fr, span), tc, tr).collect()

    def fn(d, s):
        got = C.c_uint64(0)
        _lib.check(_lib.lib.rh_uniform_row(vp(d), ref.size, vp(s), n, fc, fr, tc, tr, span, C.byref(got), _st()), "rh_uniform_row")
        return got.value

    return row_case(k, x, ref.size, ref, 0, 0, fn, written=ref.size)


# ---- generators, the two streaming handles, the spatial block, the live filter ----
def chirp(k, O, G, ls, ld):
    """test_chirp_writes_what_is_left_of_the_sweep: *out_n samples are written, the rest of dst keeps the sentinel"""
    from rodio_amd import _lib

    total, first, n = 48000, 47000, 1500
    dst, seen = k.dst(n, ld), {}

    def call():
        m = C.c_uint64(0)
        _lib.check(_lib.lib.rh_chirp(vp(dst.ptr()), first, n, total, 48000, 20.0, 20000.0, C.byref(m), _st()), "rh_chirp")
        seen["m"] = m.value

    def check():
        assert seen["m"] == total - first
        row = dst.check_snapshot(written=seen["m"])[: seen["m"]]
        err = float(np.max(np.abs(row.astype(np.float64) - AM.chirp_ref(48000, 20.0, 20000.0, total, first, seen["m"]))))
        assert err <= AM.SINE_TOL, err

    return stream_gate.case([call], check)


def signal_generate(k, O, G, ls, ld):
    """test_signal_generate_rows_states_and_functions' first call: the states and the function codes in arenas"""
    from rodio_amd import _lib

    lib = _lib.lib
    rates, freqs, fns = [44100, 48000, 8000, 192000, 22050], [440.0, 20.0, 3999.0, 17.25, 30000.0], ["sine", "square", "sawtooth", "triangle", "square"]
    codes = np.array([{"sine": 0, "triangle": 1, "square": 2, "sawtooth": 3}[f] for f in fns], np.int32)
    n, ldim, Sg = 1001, 1001 + 13, 5
    init = np.zeros(2 * Sg, f32)
    for g in range(Sg):
        _lib.check(lib.rh_signal_generator_init(init[2 * g:].ctypes.data_as(_lib.f32p), rates[g], freqs[g]), "rh_signal_generator_init")
    st, fn, dst = k.state(2 * Sg, init), k.src(codes), k.dst_rows(Sg, n, ldim, ld)
    ph = [AM._phases(init[2 * g], 0.0, n) for g in range(Sg)]

    def check():
        rows, state = dst.check_snapshot(), st.check_snapshot()
        fn.snapshot_unchanged()
        for g in range(Sg):
            want = AM.wave_ref(fns[g], ph[g][:n])
            if fns[g] == "sine":
                err = float(np.max(np.abs(rows[g].astype(np.float64) - want)))
                assert err <= AM.SINE_TOL, (g, err)
            else:
                assert arena.same(rows[g], want), g
            assert bits(state[2 * g])[0] == bits(init[2 * g])[0] and bits(state[2 * g + 1])[0] == bits(ph[g][n])[0], g

    return stream_gate.case([lambda: _lib.check(lib.rh_signal_generate(vp(dst.ptr()), ldim, n, vp(st.ptr()), vp(fn.ptr()), Sg, _st()), "rh_signal_generate")], check)


def echo(k, O, G, ls, ld):
    """rh_echo_process over blocks shorter and longer than the delay, then rh_echo_flush, all behind one gate.  The handle's history cannot
    be wound back: the gated run has a handle of its own, created on the gated stream once the warming run is over."""
    from rodio_amd import _lib

    lib, ch, D, blocks = _lib.lib, 2, 2000, [14, 1998, 2002]
    ns = _delay_ns(D, 48000, ch)
    x = np.random.default_rng(D).uniform(-0.25, 0.25, sum(blocks)).astype(f32)
    ref = O.TestSource(x, ch, 48000).reverb(ns, 0.3).collect()
    h = [C.c_void_p()]
    _lib.check(lib.rh_echo_create(C.byref(h[0]), D, 0.3), "rh_echo_create")
    at = np.cumsum([0] + blocks)
    ins = [k.src(x[at[i]: at[i + 1]]) for i in range(len(blocks))]
    outs = [k.dst(b) for b in blocks] + [k.dst(D)]
    calls = [lambda i=i: _lib.check(lib.rh_echo_process(h[0], vp(outs[i].ptr()), vp(ins[i].ptr()), blocks[i], _st()), "rh_echo_process") for i in range(len(blocks))]
    calls.append(lambda: _lib.check(lib.rh_echo_flush(h[0], vp(outs[-1].ptr()), _st()), "rh_echo_flush"))

    def rewind():
        lib.rh_echo_destroy(h[0])
        _lib.check(lib.rh_echo_create(C.byref(h[0]), D, 0.3), "rh_echo_create")

    def check():
        try:
            assert arena.same(np.concatenate([o.check_snapshot() for o in outs]), ref)
            for a in ins:
                a.snapshot_unchanged()
        finally:
            lib.rh_echo_destroy(h[0])

    return stream_gate.case(calls, check, rewind)


def resampler(k, O, G, ls, ld):
    """rh_resampler_process: blocks of 1, 7 and 5000 frames and an empty flush (test_resampler_blocks_with_exact_capacities), one gate"""
    from rodio_amd import _lib

    lib, ch, frm, to, blocks = _lib.lib, 3, 96000, 44100, [1, 7, 5000, 0]
    x = np.random.default_rng(8).uniform(-1, 1, sum(blocks) * ch).astype(f32)
    ref = O.SampleRateConverter(O.TestSource(x, ch, frm), frm, to, ch).collect()
    h = [C.c_void_p()]
    _lib.check(lib.rh_resampler_create(C.byref(h[0]), frm, to, ch), "rh_resampler_create")
    at, laid, got = np.cumsum([0] + blocks), [], {}

    def call_of(i):
        def call():
            b, flush = blocks[i], int(i == len(blocks) - 1)
            cap, m = C.c_uint64(0), C.c_uint64(0)
            _lib.check(lib.rh_resampler_pending_frames(h[0], b, flush, C.byref(cap)), "rh_resampler_pending_frames")
            assert cap.value * ch <= laid[i][1].layout.n
            _lib.check(lib.rh_resampler_process(h[0], vp(laid[i][1].ptr()), cap.value, vp(laid[i][0].ptr()) if b else None, b, flush, C.byref(m), _st()), "rh_resampler_process")
            got[i] = m.value

        return call

    for i, b in enumerate(blocks):  # a block's capacity: what the converter can have pending for it (one frame more than the ratio gives, and the flush's last)
        laid.append((k.src(x[at[i] * ch: at[i + 1] * ch]), k.dst((b * to // frm + 3) * ch)))

    def rewind():
        lib.rh_resampler_destroy(h[0])
        _lib.check(lib.rh_resampler_create(C.byref(h[0]), frm, to, ch), "rh_resampler_create")

    def check():
        try:
            assert arena.same(np.concatenate([laid[i][1].check_snapshot(written=got[i] * ch)[: got[i] * ch] for i in range(len(blocks))]), ref)
        finally:
            lib.rh_resampler_destroy(h[0])

    return stream_gate.case([call_of(i) for i in range(len(blocks))], check, rewind)


def spatial_mix_block(k, O, G, ls, ld, seed=0):
    """test_gpu_spatial_mix.py's (65 frames, 33 sources): the second launch continues from the stored partial sum.  Five host arrays: the
    WideSrc table, the two tables of device addresses (gains, factors) and the two step tables, each overwritten behind the call."""
    from rodio_amd import _lib

    rate, to_rate, in_ch, M, S, m0 = 44100, 48000, 1, 65, 33, 12345
    rng = np.random.default_rng(1000 * in_ch + rate % 89 + seed)
    F, T = SM.R.reduced(rate, to_rate)
    first = (m0 * F // T) * 2
    srcs = [SM.make(rng, in_ch, rate, to_rate, M, m0, gp=882 + i, gf=first, fp=(441 if i % 3 else None), ff=first + i) for i in range(S)]
    want = SM.R.spatial_mix(2, to_rate, M, srcs)
    devs = [SM.Dev(s) for s in srcs]
    for d in devs:
        for a in d.keep:
            k.add(a)
    dst = k.dst(M * 2, ld)

    def call():  # test_gpu_spatial_mix.call's tables, all five in the case's hands
        arr = k.host((_lib.WideSrc * S)(), 0)  # zeros behind the return: sources of no frames
        gains, factors = k.host((C.c_void_p * S)(), k.pit()), k.host((C.c_void_p * S)(), k.pit())  # late readers: gains and factors of NaN
        gsteps, fsteps = k.host((C.c_uint64 * (3 * S))(), 0), k.host((C.c_uint64 * (3 * S))(), 0)
        for i, (s, d) in enumerate(zip(srcs, devs)):
            arr[i].data, arr[i].channels, arr[i].from_rate, arr[i].phase, arr[i].frames, arr[i].last, arr[i].gain = d.ptr["x"], s.in_ch, s.from_rate, s.phase, s.frames, s.last, 1.0
            gains[i], factors[i] = d.ptr["gains"], d.ptr["factors"]
            gsteps[3 * i: 3 * i + 3] = [s.gain_first, s.gain_period, s.gains.shape[0]]
            fsteps[3 * i: 3 * i + 3] = [s.factor_first, s.factor_period, 0 if s.factors is None else s.factors.size]
        _lib.check(_lib.lib.rh_spatial_mix_block(vp(dst.ptr()), 2, to_rate, M, arr, S, gains, gsteps, factors, fsteps, _st()), "rh_spatial_mix_block")

    def check():
        assert arena.same(dst.check_snapshot(), want)
        for d in devs:
            for a in d.keep:
                a.snapshot_unchanged()

    return stream_gate.case([call], check)


def biquad_steps(k, O, G, ls, ld, seed=0, mode=0):
    """test_mode0_bits_against_the_reference: stereo, a change every 441 samples (inside frames), `first` in the middle of a period, a
    carried state; the table of coefficients on the device"""
    from rodio_amd import _lib

    ch, period, frames = 2, 441, 1027
    n = frames * ch
    first = 5 * period + period // 2
    table = LF.filters_table(O, LF.R.steps_needed(first, period, n), 7 * ch + period + seed)
    x = LF.R.noise(ch * 31 + period % 97 + seed, n)
    st0 = LF.R.noise(5 + seed, ch * 4).reshape(ch, 4) * f32(0.25)
    want, want_st = LF.R.biquad_steps_ref(x, ch, first, period, table, st0)
    src, dst, tab, st = k.src(x, ls), k.dst(n, ld), k.src(table.reshape(-1)), k.state(4 * ch, st0)

    def check():
        assert arena.same(dst.check_snapshot(), want) and arena.same(st.check_snapshot(), want_st)
        src.snapshot_unchanged()
        tab.snapshot_unchanged()

    return stream_gate.case([lambda: _lib.check(LF.steps_call(dst.ptr(), src.ptr(), frames, ch, 1, first, period, tab.ptr(), table.shape[0], 0, st.ptr(), mode), "rh_biquad_steps")], check)


# ---- SampleTypeConverter: one case per kernel template, either way ----
CONVERTERS = ["u8_to_f32", "i16_to_f32", "i24_to_f32", "i64_to_f32", "f64_to_f32", "f32_to_u8", "f32_to_i16", "f32_to_i24", "f32_to_i64", "f32_to_f64"]


def convert(name):
    """test_gpu_arena_formats.convert_case's arenas, both FILLS behind one gate: integers between the fill, f64 between bytes of 0xff, a
    byte dst between the fill (an element never written equals the reference under at most one of the two)"""

    def build(k, O, G, ls, ld):
        fn = getattr(L(), "rh_convert_" + name)
        src_t, dst_t = name.split("_to_")
        if src_t == "f32":
            x = AFo.floats(N, 7 + N)
        else:
            x = AFo.floats(N, 5).astype(np.float64) * (1.0 + 2.0 ** -30) if src_t == "f64" else AFo.ints(src_t, N, 11 + N)
        ref = O.convert(name, x)
        ssz, dsz = x.dtype.itemsize, np.dtype(AFo.NP[dst_t]).itemsize
        ls, ld = ls % (16 // ssz), ld % (16 // dsz)  # leads in elements, below a 16-byte line
        int_src, byte_dst = src_t not in ("f32", "f64"), dst_t != "f32"
        laid = []
        for fill in arena.FILLS:
            src = k.src(x, ls) if src_t == "f32" else k.add(arena.src_bytes_arena(x, ls * ssz, fill if int_src else arena.NAN_FILL))
            dst = k.add(arena.dst_bytes_arena(N, AFo.NP[dst_t], ld * dsz, fill)) if byte_dst else k.dst(N, ld)
            laid.append((src, dst))

        def check():
            outs = []
            for src, dst in laid:
                got = dst.check_snapshot(ref, dtype=AFo.NP[dst_t]) if byte_dst else dst.check_snapshot()
                src.snapshot_unchanged()
                assert np.array_equal(arena.as_bytes(got), arena.as_bytes(ref)), name
                outs.append(got)
            if int_src:
                arena.same_under_fills(outs, ref)

        return stream_gate.case([lambda src=src, dst=dst: ok(fn(vp(dst.ptr()), vp(src.ptr()), N, _st()), name) for src, dst in laid], check)

    return build


def wav_decode(fmt, to):
    """test_wav_decode_rows at two whole tiles plus 3 frames, n_samples one short of the last frame (k_fill_zero completes it); to ==
    channels: rh_wav_decode, else rh_wav_decode_channels.  The sample bytes `ls` bytes behind a 16-byte boundary, both surroundings."""
    fmt, bits, is_float, bps = next(w for w in AFo.WAV if w[0] == fmt)

    def build(k, O, G, ls, ld):
        lib, ch = L(), AFo.WAV_CH
        frames = 2 * AFo.wav_tile_frames(bps, ch, to) + 3
        n = frames * ch - 1
        raw, vals = AFo.wav_samples(fmt, n, frames + bits)
        dec = vals if fmt == "f32" else O.convert(fmt + "_to_f32", vals)
        dec = np.concatenate([dec, np.zeros(frames * ch - n, f32)])
        ref = dec if to == ch else O.ChannelCountConverter(O.TestSource(dec, ch, 48000), ch, to).collect()
        total = frames * to
        fills = (arena.NAN_FILL, arena.FILLS[0]) if fmt == "f32" else arena.FILLS
        laid = [(k.add(arena.src_bytes_arena(raw, ls, fill)), k.dst(total, ls % 4)) for fill in fills]

        def call_of(src, dst):
            def call():
                m = C.c_uint64(0)
                if to == ch:
                    st = lib.rh_wav_decode(vp(dst.ptr()), vp(src.ptr()), n, ch, bits, is_float, C.byref(m), _st())
                else:
                    st = lib.rh_wav_decode_channels(vp(dst.ptr()), vp(src.ptr()), n, ch, bits, is_float, to, C.byref(m), _st())
                assert st == 0 and m.value == total, (fmt, to, st, m.value)

            return call

        def check():
            outs = [dst.check_snapshot() for _, dst in laid]
            for src, _ in laid:
                src.snapshot_unchanged()
            arena.same_under_fills(outs, ref, fills=fills)

        return stream_gate.case([call_of(src, dst) for src, dst in laid], check)

    return build


# ---- the fused handle ----
RLM = dict(frm=44100, to=48000, lens=[4099, 2500, 3001], filt="low_pass", freq=200)


def rlm_run(k, O, G, ls, ld, ch=2):
    """test_one_shot_runs: three ragged sources through one rh_rlm_run"""
    frm, to, lens, filt, freq = RLM["frm"], RLM["to"], RLM["lens"], RLM["filt"], RLM["freq"]
    xs = [rnd(6100 + s, n * ch, 0.3) for s, n in enumerate(lens)]
    M = AF._out_frames(lens, frm, to, ch, 0)
    ref = AF._reference(O, xs, frm, to, ch, 0, filt, freq, None)
    ins, dst = [k.src(x) for x in xs], k.dst(M * ch)
    p = G.ResampleLowpassMix(frm, to, ch, 0, filt, freq, 0.5, max_sources=3, max_in_frames=max(lens), frames_per_lane=4)
    AF._set_sources(p, [a.ptr() for a in ins], lens)

    def call():
        assert AF._run(p, dst.ptr(), M) == M

    def check():
        try:
            p.check_status()
            AF._meets(dst.check_snapshot(), ref, filt)
            for a in ins:
                a.snapshot_unchanged()
        finally:
            p.close()

    return stream_gate.case([call], check)


def rlm_stream(his, equal=False, ch=2):
    """rh_rlm_stream_block_v (equal: rh_rlm_stream_block over sources of one length) with rh_rlm_stream_overlap off, block k up to input
    frame his[k].  What a block is given depends on what the blocks before it consumed -- host outputs of the calls -- so a dry run on a
    handle of its own lays the blocks out before anything is staged."""

    def build(k, O, G, ls, ld):
        from rodio_amd import _lib

        lib, frm, to, filt, freq = _lib.lib, RLM["frm"], RLM["to"], RLM["filt"], RLM["freq"]
        ns = [max(his)] * 3 if equal else RLM["lens"]
        S = len(ns)
        xs = [rnd(6800 + s, n * ch, 0.3) for s, n in enumerate(ns)]
        ref = AF._reference(O, xs, frm, to, ch, None, filt, freq, None)

        def handle():
            p = G.ResampleLowpassMix(frm, to, ch, None, filt, freq, 0.5, max_sources=S, max_in_frames=max(his) + 4096)
            p.stream_begin()
            _lib.check(lib.rh_rlm_stream_overlap(p._h, 0), "rh_rlm_stream_overlap")
            return p

        def block(p, ptrs, avail, hi, dp, cap, host):
            o, c = C.c_uint64(0), C.c_uint64(0)
            if equal:
                _lib.check(lib.rh_rlm_stream_block(p._h, host((C.c_void_p * S)(*ptrs), k.pit()), S, avail[0], int(hi == his[-1]), C.c_void_p(dp), cap, C.byref(o), C.byref(c), _st()), "rh_rlm_stream_block")
            else:
                _lib.check(lib.rh_rlm_stream_block_v(p._h, host((C.c_void_p * S)(*ptrs), k.pit()), host((C.c_uint64 * S)(*avail), 0), host((C.c_uint8 * S)(*[1 if hi >= n else 0 for n in ns]), 1), S,
                                                     C.c_void_p(dp), cap, C.byref(o), C.byref(c), _st()), "rh_rlm_stream_block_v")
            return o.value, c.value

        # the dry run: rows on plain buffers, the consumed counts kept
        dry, plan, g0 = handle(), [], 0
        for hi in his:
            rows = [x[min(g0, n) * ch: min(hi, n) * ch] for x, n in zip(xs, ns)]
            avail = [len(r) // ch for r in rows]
            cap = AF._mirror_capacity(max(avail), frm, to)
            ins, (dt, dp) = [arena.plain(r if r.size else np.zeros(4, f32)) for r in rows], arena.plain_dst(cap * ch)
            o, c = block(dry, [q for _, q in ins], avail, hi, dp, cap, lambda a, v=None: a)
            plan.append((rows, avail, cap, o, c))
            g0 += c
        dry.check_status()
        dry.close()
        p = handle()
        laid = [([k.src(r) for r in rows], k.dst(cap * ch)) for rows, _, cap, _, _ in plan]

        def call_of(i):
            def call():
                _, avail, cap, o, c = plan[i]
                assert block(p, [a.ptr() for a in laid[i][0]], avail, his[i], laid[i][1].ptr(), cap, k.host) == (o, c)

            return call

        def rewind():
            p.stream_begin()
            _lib.check(lib.rh_rlm_stream_overlap(p._h, 0), "rh_rlm_stream_overlap")

        def check():
            try:
                p.check_status()
                parts = [laid[i][1].check_snapshot(written=plan[i][3] * ch)[: plan[i][3] * ch] for i in range(len(his))]
                for ins, _ in laid:
                    for a in ins:
                        a.snapshot_unchanged()
                AF._meets(np.concatenate(parts), ref, filt)
            finally:
                p.close()

        return stream_gate.case([call_of(i) for i in range(len(his))], check, rewind)

    return build


def rlm_subset(k, O, G, ls, ld, ch=2):
    """rh_rlm_run_subset(1, 1): one converted, filtered stream in a dst of the batch's length, silence behind the source's end"""
    frm, to, lens, filt, freq = RLM["frm"], RLM["to"], RLM["lens"], RLM["filt"], RLM["freq"]
    xs = [rnd(6200 + s, n * ch, 0.3) for s, n in enumerate(lens)]
    M, M1 = AF._out_frames(lens, frm, to, ch, 0), AF._out_frames(lens[1:2], frm, to, ch, 0)
    ref = AF._reference(O, xs[1:2], frm, to, ch, None, filt, freq, None)
    ins, dst = [k.src(x) for x in xs], k.dst(M * ch)
    p = G.ResampleLowpassMix(frm, to, ch, None, filt, freq, 0.5, max_sources=3, max_in_frames=max(lens), frames_per_lane=4)
    AF._set_sources(p, [a.ptr() for a in ins], lens)

    def call():
        assert AF._run(p, dst.ptr(), M, subset=(1, 1)) == M

    def check():
        try:
            p.check_status()
            row = dst.check_snapshot()
            AF._meets(row[: M1 * ch], ref, filt)
            assert M1 < M and not np.any(row[M1 * ch:])
        finally:
            p.close()

    return stream_gate.case([call], check)


def rlm_batch(k, O, G, ls, ld):
    """rh_rlm_run_batch: three stereo rows, out_frames rounded up to even plus 2 frames apart: the gaps keep the sentinel"""
    from rodio_amd import _lib

    frm, to, filt, freq, ch, n = RLM["frm"], RLM["to"], RLM["filt"], RLM["freq"], 2, 4099
    xs = [rnd(6300 + s, n * ch, 0.3) for s in range(3)]
    M = AF._out_frames([n], frm, to, ch, 0)
    stride = (M + 1) // 2 * 2 + 2
    refs = [AF._reference(O, xs[s: s + 1], frm, to, ch, None, filt, freq, None) for s in range(3)]
    ins, dst = [k.src(x) for x in xs], k.dst_rows(3, M * ch, stride * ch)
    p = G.ResampleLowpassMix(frm, to, ch, None, filt, freq, 0.5, max_sources=3, max_in_frames=n, frames_per_lane=4)
    AF._set_sources(p, [a.ptr() for a in ins], [n] * 3)

    def call():
        m = C.c_uint64(0)
        _lib.check(_lib.lib.rh_rlm_run_batch(p._h, C.c_void_p(dst.ptr()), stride, C.byref(m), _st()), "rh_rlm_run_batch")
        assert m.value == M

    def check():
        try:
            p.check_status()
            rows = dst.check_snapshot()
            for s in range(3):
                AF._meets(rows[s], refs[s], filt)
        finally:
            p.close()

    return stream_gate.case([call], check)


def rlm_pcm16(native, fresh=True):
    """rh_rlm_set_sources_pcm16 and the run behind it, both inside the gated window: on a handle that has not run yet (created between the
    warming run and the gated one), where the setter has nothing to wait for; fresh=False: on the handle of the warming run, where it
    waits for what the handle has queued (WAITS).  native: test_gpu_pcm16.py's test_mix_rows (nine stereo
    rows of 1537 frames with gains: k_mix_rows_pcm16 reads the int16 rows); else its converted route (four ragged rows, a filter per
    source first).  The reference is that file's: the bits of the same handle on the f32 twins, run here on a quiet stream."""

    def build(k, O, G, ls, ld):
        import torch

        from rodio_amd import _lib

        ch = 2
        if native:
            rows, gains = [P16.pcm(6100 + s, 1537 * ch, 0.1) for s in range(9)], P16.GAINS9
        else:
            rows, gains = [P16.pcm(6300 + s, 20000 * 2, 0.2)[: 2 * (4099 - 100 * s)] for s in range(4)], None
        q = P16._handle(G, rows, ch, gains=gains)
        q.set_sources([torch.from_numpy(P16.twin(r)).cuda() for r in rows])
        want = q.run().cpu().numpy().copy()
        q.check_status()
        q.close()
        h = [P16._handle(G, rows, ch, gains=gains)]
        ins, dst = [k.add(arena.src_bytes_arena(np.array(r), 0, arena.FILLS[s % 2])) for s, r in enumerate(rows)], k.dst(want.size)
        S = len(rows)

        def rewind():
            h[0].close()
            h[0] = P16._handle(G, rows, ch, gains=gains)

        def call():
            ptrs = k.host((C.c_void_p * S)(*[a.ptr() for a in ins]), k.pit())
            frames = k.host((C.c_uint64 * S)(*[len(r) // ch for r in rows]), 0)
            _lib.check(_lib.lib.rh_rlm_set_sources_pcm16(h[0]._h, ptrs, frames, S), "rh_rlm_set_sources_pcm16")
            assert AF._run(h[0], dst.ptr(), want.size // ch) == want.size // ch

        def check():
            try:
                h[0].check_status()
                assert h[0].source_format() == {"format": 1, "native": 1 if native else 0}
                assert arena.same(dst.check_snapshot(), want)
                for a in ins:
                    a.snapshot_unchanged()
            finally:
                h[0].close()

        return stream_gate.case([call], check, rewind if fresh else None)

    return build


STREAM_NINE = [500, 1000, 1600, 2100, 2600, 3024, 3500, 4048, 4099]  # the sources of 2500 and 3001 frames end in blocks 5 and 6


CASES = {
    "rh_amplify": elementwise("amplify"), "rh_distortion": elementwise("distortion"), "rh_dither GPDF": elementwise("dither GPDF"),
    "rh_dither HighPass": elementwise("dither HighPass"), "rh_linear_gain_ramp": elementwise("ramp"),
    "rh_delay": delay_like("delay"), "rh_echo_mix": delay_like("echo_mix"), "rh_take_duration": take_duration, "rh_take_duration_from": take_duration_from,
    "rh_channels_convert": channels("channels_convert"), "rh_channel_volume": channels("channel_volume"),
    "rh_amplify_steps": amplify_steps, "rh_channel_volume_steps": channel_volume_steps, "rh_resample_linear": resample_linear,
    "rh_mix_sum": mix_sum, "rh_mix_pair": mix_pair, "rh_noise_generate": noise_generate,
    "rh_limit": limit(False), "rh_limit state": limit(True),
    "rh_biquad mode 0": biquad(0, False), "rh_biquad mode 0 state": biquad(0, True),
    "rh_agc": agc(False), "rh_agc state": agc(True),
    "rh_memset": copies("memset"), "rh_memcpy_h2d": copies("memcpy_h2d"), "rh_memcpy_h2d_rows": copies("memcpy_h2d_rows"),
    "rh_memcpy_h2d_rows page-locked": copies("memcpy_h2d_rows page-locked"),
    "rh_memcpy_d2h_async": copies("memcpy_d2h_async"), "rh_memcpy_d2h": copies("memcpy_d2h"), "rh_memcpy_d2d": copies("memcpy_d2d"),
    **{"rh_convert_" + c: convert(c) for c in CONVERTERS},
    "rh_wav_decode i16": wav_decode("i16", 3), "rh_wav_decode i24": wav_decode("i24", 3), "rh_wav_decode_channels i16": wav_decode("i16", 2),
    "rh_wav_decode_channels f32": wav_decode("f32", 5),
    "rh_chirp": chirp, "rh_signal_generate": signal_generate, "rh_spatial_mix_block": spatial_mix_block, "rh_biquad_steps": biquad_steps,
}
# rows on 16-byte boundaries only (the entry refuses, or has no other route to take): one case each
ALIGNED = {"rh_biquad mode 1": biquad(1, False), "rh_biquad mode 1 state": biquad(1, True), "rh_reverb_spatial": reverb_spatial, "rh_crossfade": crossfade,
           "rh_wide_mix_block": wide_mix_block(), "rh_wide_mix_block_filtered mode 0": wide_mix_block(0), "rh_wide_mix_block_filtered mode 1": wide_mix_block(1),
           "rh_uniform_segments": uniform_segments, "rh_uniform_segments_dev": uniform_segments_dev, "rh_uniform_row": uniform_row, "rh_rlm_run": rlm_run,
           "rh_rlm_run_subset": rlm_subset, "rh_rlm_run_batch": rlm_batch, "rh_rlm_set_sources_pcm16 native": rlm_pcm16(True),
           "rh_rlm_set_sources_pcm16 converted": rlm_pcm16(False), "rh_rlm_set_sources_pcm16 on a handle that has run": rlm_pcm16(True, fresh=False),
           "rh_echo_process / rh_echo_flush": echo, "rh_resampler_process": resampler,
           "rh_rlm_stream_block": rlm_stream([4099], equal=True), "rh_rlm_stream_block_v": rlm_stream([4099])}


@pytest.mark.parametrize("ls,ld", GATED_LEADS)
@pytest.mark.parametrize("name", list(CASES))
def test_entry_behind_a_gate(G, O, side, delay, name, ls, ld):
    gated(lambda k: CASES[name](k, O, G, ls, ld), side, delay, "A", name)


@pytest.mark.parametrize("name", list(ALIGNED))
def test_aligned_entry_behind_a_gate(G, O, side, delay, name):
    with knobs(RH_BIQUAD_NO_FALLBACK="1"):  # mode 1: k_biquad_scan or an error
        gated(lambda k: ALIGNED[name](k, O, G, 0, 0), side, delay, "A", name)
        G.async_status()


@pytest.mark.parametrize("name", ["rh_amplify", "rh_limit", "rh_mix_sum"])
def test_entry_behind_a_gate_on_a_stream_of_rh_stream_create(G, O, delay, name):
    import torch

    lib, h = L(), C.c_void_p()
    ok(lib.rh_stream_create(C.byref(h)), "rh_stream_create")
    try:
        gated(lambda k: CASES[name](k, O, G, 0, 0), torch.cuda.ExternalStream(h.value), delay, "A rh_stream_create", name)
    finally:
        ok(lib.rh_stream_destroy(h), "rh_stream_destroy")


# ================================================================================================================ B: depth ====
DEPTH = 9  # more than twice either four-slot ring


def depth_of(builder, O, G, ls, ld, **kw):
    """DEPTH cases of one builder (seeds 0..8: different tables, own destinations) as ONE case: their calls in a row, every check"""

    def build(k):
        cs = [builder(k, O, G, ls, ld, seed=s, **kw) for s in range(DEPTH)]

        def check():
            for s, c in enumerate(cs):
                try:
                    c.check()
                except AssertionError as e:
                    raise AssertionError(f"call {s + 1} of {DEPTH}: {e}") from e

        return stream_gate.case([c.calls[0] for c in cs], check)

    return build


@pytest.mark.parametrize("ls,ld", GATED_LEADS)
def test_nine_mix_sums_behind_one_gate(G, O, side, delay, ls, ld):
    gated(depth_of(mix_sum, O, G, ls, ld, out_len=1027), side, delay, "B", "rh_mix_sum", DEPTH)


def test_nine_amplify_steps_behind_one_gate(G, O, side, delay):
    gated(depth_of(amplify_steps, O, G, 3, 2, n=1027), side, delay, "B", "rh_amplify_steps", DEPTH)


def test_nine_filtered_wide_blocks_behind_one_gate(G, O, side, delay):
    gated(depth_of(wide_mix_block(0), O, G, 0, 0), side, delay, "B", "rh_wide_mix_block_filtered", DEPTH)


def test_nine_spatial_blocks_behind_one_gate(G, O, side, delay):
    gated(depth_of(spatial_mix_block, O, G, 0, 0), side, delay, "B", "rh_spatial_mix_block", DEPTH)


def test_nine_biquad_steps_behind_one_gate(G, O, side, delay):
    gated(depth_of(biquad_steps, O, G, 0, 0), side, delay, "B", "rh_biquad_steps", DEPTH)


def test_nine_uniform_segment_tables_behind_one_gate(G, O, side, delay):
    gated(depth_of(uniform_segments, O, G, 0, 0), side, delay, "B", "rh_uniform_segments", DEPTH)


def test_nine_stream_blocks_behind_one_gate_and_the_fifth_waits_for_a_ring_slot(G, O, side, delay):
    """rh_rlm_stream_block_v drives the fused handle's descriptor ring (upload_descriptors, four page-locked tables): nine blocks of
    differing lengths and end flags; calls 1-4 return while the gate is pending, call 5 waits for the copy of call 1's table."""
    r = gated(lambda k: rlm_stream(STREAM_NINE)(k, O, G, 0, 0), side, delay, "B", "rh_rlm_stream_block_v", DEPTH, exempt=range(4, DEPTH))
    assert r.pending[:4] == [True] * 4 and not r.pending[4], ("the four-slot ring: calls 1-4 return at once, call 5 waits", r.pending)


def test_nine_crossfades_behind_one_gate_and_the_fifth_waits_for_a_ring_slot(G, O, side, delay):
    """Eight fused batches and a composed one.  The stream's pinned table ring (rh::table_stage) has four slots: calls 1-4 return while the gate is pending, call 5
    waits for the copy that call 1 queued (behind the gate), so it and what follows return after it.  Every destination is its own."""

    def build(k):
        both = [crossfade_call(k, O, [CF_FUSED(10 * s), CF_CUT(10 * s)][: 1 + s % 2]) for s in range(DEPTH - 1)] + [crossfade_call(k, O, [CF_COMPOSED(7)])]

        def check():
            for s, (_, chk) in enumerate(both):
                try:
                    chk()
                except AssertionError as e:
                    raise AssertionError(f"call {s + 1} of {DEPTH}: {e}") from e

        return stream_gate.case([c for c, _ in both], check)

    r = gated(build, side, delay, "B", "rh_crossfade", DEPTH, exempt=range(4, DEPTH))
    assert r.pending[:4] == [True] * 4 and not r.pending[4], ("the four-slot ring: calls 1-4 return at once, call 5 waits", r.pending)


# ================================================================================================================ C: swept cutoff ====
def test_forty_cutoffs_behind_one_gate_evict_plans_that_are_still_queued(G, O, side, delay):
    """rh_biquad mode 1 keeps 32 plans; a call that adds a 33rd evicts the oldest, whose device table ~BqPlan frees on the spot, trusting
    that "hipFree waits for the device" while launches that read such tables are still queued behind the gate.  `pending` is not
    asserted: a free may wait.  Every destination at test_gpu_filter_signals.py's mode-1 criteria for its coefficients.

    On the runtime of profiles/stream_order.txt the calls return at once until the cache is full, and the first call that evicts returns
    only after the gate has opened: the free does wait, and no table goes while a launch may read it.  A runtime whose hipFree returned
    early would leave the gate pending through all 40 calls and free tables under queued launches: the values are what would tell."""
    frames, ch, n_cut = 4099, 1, 40
    cutoffs = [300 + 97 * i for i in range(n_cut)]
    x = rnd(900, frames * ch, 0.4)
    xp = float(np.abs(x).max())

    def build(k):
        src = k.src(x)
        dsts = [k.dst(frames * ch) for _ in cutoffs]
        cos = [G.biquad_coeffs("low_pass", f, 0.5, FS_RATE) for f in cutoffs]

        def call_of(i):
            return lambda: _biquad(dsts[i].ptr(), src.ptr(), frames, ch, 1, k.host(cos[i].copy()), 1, None)

        def check():
            src.snapshot_unchanged()
            for i, f in enumerate(cutoffs):
                ref = O.TestSource(x, ch, FS_RATE).low_pass(f, 0.5).collect()
                criteria(dsts[i].check_snapshot(), ref, truth(cos[i], x, ch), xp, l1_gain(cos[i]), f"swept cutoff {f} Hz", scan_ok("low_pass", cos[i]), show=False)

        return stream_gate.case([call_of(i) for i in range(n_cut)], check, warm=[call_of(0)])  # one filter warmed: the kernel is loaded

    with knobs(RH_BIQUAD_NO_FALLBACK="1"):
        gated(build, side, delay, "C", "rh_biquad mode 1 x 40", n_cut, exempt=range(n_cut))
        G.async_status()


# ================================================================================================================ D: the scratch ====
# a composed pair whose rows need more than the 1 MiB a stream's scratch starts with: a second of a stereo `a` and of a 6-channel b
grown_crossfade = crossfade_of(lambda: [((mix_signal(2 * 50000, 91), 2, 48000), (mix_signal(6 * 50000, 92), 6, 48000))], 1000 * MS)


def scratch_sequence(O, G, shift, grow):
    """the issue's order: limit A, noise, limit A with a state, biquad mode 1 B, AGC, crossfade composed, limit A, [growth], limit A"""
    fa, fb = 3001 + 16 * shift, 2049 + 8 * shift
    seq = [("rh_limit", limit(False, fa, 2, seed=1 + shift)), ("rh_noise_generate", noise_generate), ("rh_limit state", limit(True, fa, 2, seed=2 + shift)),
           ("rh_biquad mode 1", biquad(1, False, fb, 2, 200 + 50 * shift, seed=shift)), ("rh_agc", agc(False, 4099 + shift, seed=shift)),
           ("rh_crossfade composed", crossfade_of(lambda: [CF_COMPOSED(shift)])),
           ("rh_limit", limit(False, fa, 2, seed=3 + shift))]
    if grow:
        seq.append(("growth", grown_crossfade))
    seq.append(("rh_limit", limit(False, fa, 2, seed=4 + shift)))
    return seq


def sequence_case(seq, O, G, rewind=None):
    def build(k):
        cs = [(name, b(k, O, G, 0, 0)) for name, b in seq]

        def check():
            for i, (name, c) in enumerate(cs):
                try:
                    c.check()
                except AssertionError as e:
                    raise AssertionError(f"step {i + 1} ({name}): {e}") from e

        return stream_gate.case([c.calls[0] for _, c in cs], check, rewind)

    return build


def test_scratch_users_and_a_growth_on_one_gated_stream(G, O, delay):
    """A stream of its own, so that its scratch holds the initial 1 MiB when the gated run begins: the warming run grows it, the rewind
    releases it and one small limiter call allocates it afresh.  Step 8 then synchronises the stream (the header: the scratch is "grown
    on demand"), frees and reallocates -- exempt from `pending`, and so is step 9 behind it; steps 1-7 keep their results."""
    import torch

    from rodio_amd import _lib

    s = torch.cuda.Stream()
    seq = scratch_sequence(O, G, 0, True)
    small = arena.src_arena(limit_signal(5, 257, 2)), arena.dst_arena(514)

    def rewind():
        s.synchronize()
        _lib.check(_lib.lib.rh_stream_release_scratch(_st()), "rh_stream_release_scratch")
        _limit(small[1].ptr(), small[0].ptr(), 257, 2, 1, {}, None)

    try:
        with knobs(RH_BIQUAD_NO_FALLBACK="1"):
            r = gated(sequence_case(seq, O, G, rewind), s, delay, "D", "one stream", len(seq), exempt=(7, 8))
            assert not r.pending[7], "step 8 was to make the scratch grow: it returned without waiting for the stream"
            G.async_status()
    finally:
        s.synchronize()
        _lib.check(_lib.lib.rh_stream_release_scratch(C.c_void_p(s.cuda_stream)), "rh_stream_release_scratch")


def test_scratch_users_interleaved_on_two_gated_streams(G, O, side, delay):
    """Two streams from one host thread, the same entries call by call, other shapes on each: a scratch is a stream's own.  (The six
    steps by hand: stream_gate.run drives one stream.)"""
    import torch

    from rodio_amd import _lib

    other = torch.cuda.Stream()
    streams = [side, other]
    kits, cs = [stream_gate.Kit(), stream_gate.Kit()], []
    for j, k in enumerate(kits):
        cs.append(sequence_case(scratch_sequence(O, G, 1 + j, False), O, G)(k))
    torch.cuda.synchronize()
    for k in kits:
        k.stage()
    torch.cuda.synchronize()
    try:
        with knobs(RH_BIQUAD_NO_FALLBACK="1"):
            gates, pending = [], []
            for warm in (True, False):
                if not warm:
                    gates = [stream_gate.Gate(delay, s, gate_ms(2 * len(cs[0].calls))) for s in streams]
                for k, s in zip(kits, streams):
                    k.restore(s)
                for i in range(len(cs[0].calls)):
                    for j, s in enumerate(streams):
                        with torch.cuda.stream(s):
                            cs[j].calls[i]()
                            if not warm:
                                pending.append(gates[j].pending())
                            kits[j].spoil_hosts()
                for k, s in zip(kits, streams):
                    if not warm:
                        k.snapshot(s)
                    k.spoil(s)
                for s in streams:
                    s.synchronize()
            RAN["D"] = RAN.get("D", 0) + 1
            print(f"[stream_order D two streams] pending {''.join('1' if p else '0' for p in pending)}")
            assert all(pending), pending
            for c in cs:
                c.check()
            G.async_status()
    finally:
        other.synchronize()
        _lib.check(_lib.lib.rh_stream_release_scratch(C.c_void_p(other.cuda_stream)), "rh_stream_release_scratch")


def test_two_host_threads_on_one_gated_stream(G, O, side, delay):
    """ctypes releases the GIL: each thread makes 8 calls, rh_limit and rh_biquad mode 1 in turn, on rows of its own, all on one gated
    stream -- stream_scratch's lock (`hold`) is what keeps one thread's pre-kernel and scan together.  Every row equals its reference."""
    import torch

    per = 8
    k = stream_gate.Kit()
    jobs = [[(limit(False, 1025 + 32 * t, 2, seed=10 * t + i) if i % 2 == 0 else biquad(1, False, 1027 + 16 * t, 2, 300, seed=10 * t + i))(k, O, G, 0, 0) for i in range(per)] for t in range(2)]
    torch.cuda.synchronize()
    k.stage()
    torch.cuda.synchronize()
    errors = []

    def worker(t):
        try:
            with torch.cuda.stream(side):
                for c in jobs[t]:
                    c.calls[0]()
        except BaseException as e:  # noqa: BLE001
            errors.append((t, repr(e)))

    with knobs(RH_BIQUAD_NO_FALLBACK="1"):
        for warm in (True, False):
            gate = None if warm else stream_gate.Gate(delay, side, gate_ms(2 * per))
            k.restore(side)
            ts = [threading.Thread(target=worker, args=(t,)) for t in range(2)]
            for t in ts:
                t.start()
            for t in ts:
                t.join()
            assert not errors, errors
            k.spoil_hosts()  # (the threads' coefficient arrays: every call has returned)
            pending = None if warm else gate.pending()
            if not warm:
                k.snapshot(side)
            k.spoil(side)
            side.synchronize()
        RAN["D"] = RAN.get("D", 0) + 1
        assert pending, "the gate opened before the sixteen calls had returned"
        for t in range(2):
            for i, c in enumerate(jobs[t]):
                try:
                    c.check()
                except AssertionError as e:
                    raise AssertionError(f"thread {t}, call {i + 1}: {e}") from e
        G.async_status()


# ================================================================================================================ E: the control ====
def _copy_case(k, x, on):
    """a stand-in for an entry made of torch alone: dst row = src row, queued on the stream `on` (None: the current, gated one)"""
    import torch

    src, dst = k.src(x), k.dst(x.size)
    a, b = arena.GUARD, arena.GUARD + x.size

    def call():
        with torch.cuda.stream(on if on is not None else torch.cuda.current_stream()):
            dst.buf[a:b].copy_(src.buf[a:b], non_blocking=True)

    def check():
        assert arena.same(dst.check_snapshot(), x)

    return stream_gate.case([call], check)


def test_the_gate_sees_a_copy_on_the_null_stream(G, side, delay):
    """Nothing of the library: the same sequence around a torch copy.  On the gated stream it passes; issued on the null stream it runs
    before the inputs arrive, copies garbage, and the restore wipes it -- the checker must say so."""
    import torch

    x = signal(3, N)
    r = stream_gate.run(lambda k: _copy_case(k, x, None), side, delay, gate_ms())
    assert r.pending == [True]
    r.check()
    r = stream_gate.run(lambda k: _copy_case(k, x, torch.cuda.default_stream()), side, delay, gate_ms())
    assert r.pending == [True]
    with pytest.raises(AssertionError, match="never written"):
        r.check()
    RAN["E"] = RAN.get("E", 0) + 2
    torch.cuda.synchronize()


def test_every_wait_is_a_line_of_the_header():
    import os

    text = " ".join(open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "rodio_hip.h")).read().replace(" * ", " ").split())
    for name, line in WAITS.items():
        assert name.split()[0] in text and line in text, name


def test_report_the_gated_cases_that_ran(delay):
    """the per-group counts of profiles/stream_order.txt (a run of the whole file)"""
    print(f"[stream_order] fill {delay.fill_ms:.3f} ms, gate {GATE_FACTOR} x {SLOWEST_HOST_MS} ms a call, slowest call that did not wait {SLOWEST[0]:.3f} ms ({SLOWEST[1]}); gated cases: "
          + ", ".join(f"{g} {n}" for g, n in sorted(RAN.items())))
