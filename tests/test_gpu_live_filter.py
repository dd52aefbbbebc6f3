"""rh_biquad_steps on the device: a low_pass / high_pass whose coefficients change by steps while the filter's memory stays
(BltFilter::to_low_pass / to_high_pass under periodic_access, blt.rs:68-91, 234-252).  Mode 0 bit for bit against the numpy-f32
restatement of blt.rs:559 with an entry per sample (tests/live_filter_ref.py) and against rh_biquad mode 0 called once per step; mode 1
against the f64 evaluation of the same recurrence; batches, carried state, fallbacks, guard zones (tests/arena.py), and the chains of the
C++ host mirror (tests/cpp/live_filter_test.cpp) over the real library against its CPU stand-in."""
import ctypes as C
import os

import numpy as np
import pytest

import arena
import live_filter_ref as R
from test_live_filter_cpu import CASES, FAKE_EXE, LIVE_EXE, run_case

pytestmark = pytest.mark.gpu
f32 = np.float32
bits, same = arena.bits, arena.same
TOL = 1e-5  # the project's filter contract (rodio_hip.h)


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


def dev(a):
    import torch

    return torch.from_numpy(np.array(a, order="C")).cuda()  # (a copy: the shared reference inputs are read-only)


def steps_call(dst, src, frames, ch, S, first, period, tab, n_steps, stride, state, mode):
    from rodio_amd import _lib

    return _lib.lib.rh_biquad_steps(vp(dst), vp(src), frames, ch, S, first, period, vp(tab), n_steps, stride, vp(state), mode, _st())


def run(x, ch, first, period, table, S=1, state=None, mode=0, lead=0, in_place=False):
    """rh_biquad_steps over the rows x ([S * frames * ch] floats): (y, state') as numpy.  lead: the rows start `lead` floats behind a 16-byte
    boundary (src and dst); in_place: dst == src."""
    import torch

    from rodio_amd import _lib

    x = np.ascontiguousarray(x, f32).reshape(-1)
    frames = x.size // (ch * S)
    xd = torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    xd[lead: lead + x.size] = dev(x)
    yd = xd if in_place else torch.zeros(x.size + 8, dtype=torch.float32, device="cuda")
    t = dev(np.asarray(table, f32).reshape(-1))
    table = np.asarray(table, f32)
    n_steps, stride = (table.shape[1], table.shape[1] * 5) if table.ndim == 3 else (table.shape[0], 0)
    sd = dev(np.asarray(state, f32).reshape(-1)) if state is not None else None
    _lib.check(steps_call(yd.data_ptr() + 4 * lead, xd.data_ptr() + 4 * lead, frames, ch, S, first, period, t.data_ptr(), n_steps, stride, sd.data_ptr() if sd is not None else None, mode),
               "rh_biquad_steps")
    torch.cuda.synchronize()
    return yd.cpu().numpy()[lead: lead + x.size].copy(), (sd.cpu().numpy().reshape(S * ch, 4) if sd is not None else None)


def filters_table(O, n, seed):
    """n stable filters, far apart from step to step: what the exact mode must follow bit for bit."""
    rng = np.random.default_rng(seed)
    return np.array([O.blt_coeffs(("low_pass", "high_pass")[int(rng.integers(2))], int(rng.integers(100, 8000)), (0.5, 0.707, 2.0)[int(rng.integers(3))], R.RATE)
                     for _ in range(n)], f32)


# ---- mode 0 -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("period", [1, 2, 441, 480, 1323, 10**7])  # 441 with stereo: changes fall inside frames; 10**7: longer than the block
@pytest.mark.parametrize("ch", [1, 2, 3, 6])
def test_mode0_bits_against_the_reference(G, O, ch, period):
    """Rows aligned, at src + 4 B and in place; `first` in the middle of a period; a carried state."""
    frames = 1000
    n = frames * ch
    first = 5 * period + period // 2
    table = filters_table(O, R.steps_needed(first, period, n), 7 * ch + period % 1000)
    x = R.noise(ch * 31 + period % 97, n)
    st0 = R.noise(5, ch * 4).reshape(ch, 4) * f32(0.25)
    want, want_st = R.biquad_steps_ref(x, ch, first, period, table, st0)
    for lead, in_place in ((0, False), (1, False), (0, True), (3, True)):
        got, st = run(x, ch, first, period, table, state=st0, lead=lead, in_place=in_place)
        assert same(got, want), (lead, in_place, int(np.flatnonzero(bits(got) != bits(want))[0]))
        assert same(st, want_st), (lead, in_place)


@pytest.mark.parametrize("frames", [1, 5, 20_011])
@pytest.mark.parametrize("ch,period", [(2, 441), (3, 1323), (1, 7)])
def test_mode0_lengths_and_a_first_sample_beyond_2_to_32(G, O, ch, period, frames):
    n = frames * ch
    first = 2**32 + 3 * period + period // 3
    table = filters_table(O, R.steps_needed(first, period, n), frames + ch)
    x = R.noise(frames + ch, n)
    want, want_st = R.biquad_steps_ref(x, ch, first, period, table)
    got, st = run(x, ch, first, period, table, state=np.zeros((ch, 4), f32))
    assert same(got, want) and same(st, want_st)
    got, _ = run(x, ch, first, period, table)  # no state: a zero one that is not kept
    assert same(got, want)


@pytest.mark.parametrize("ch,period,frames", [(2, 480, 5000), (1, 240, 2049), (6, 1320, 1001), (3, 3, 100)])
def test_mode0_equals_rh_biquad_called_once_per_step(G, O, ch, period, frames):
    """Frame-aligned periods: one rh_biquad mode 0 launch per step with the state carried (all there was before) gives the same bits and state."""
    import torch

    from rodio_amd import _lib

    n = frames * ch
    table = filters_table(O, R.steps_needed(0, period, n), period)
    x = R.noise(period, n)
    got, st = run(x, ch, 0, period, table, state=np.zeros((ch, 4), f32))
    xd, yd, sd = dev(x), torch.zeros(n, dtype=torch.float32, device="cuda"), torch.zeros(ch * 4, dtype=torch.float32, device="cuda")
    fp = period // ch
    for k, f0 in enumerate(range(0, frames, fp)):
        nf = min(fp, frames - f0)
        _lib.check(_lib.lib.rh_biquad(vp(yd.data_ptr() + 4 * f0 * ch), vp(xd.data_ptr() + 4 * f0 * ch), nf, ch, 1, table[k].ctypes.data_as(_lib.f32p), vp(sd.data_ptr()), 0, _st()), "rh_biquad")
    torch.cuda.synchronize()
    assert same(got, yd.cpu().numpy())
    assert same(st, sd.cpu().numpy())


# ---- batches ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("S", [1, 3, 70])  # 70: the lane-per-stream grid of mode 0 spans two workgroups
@pytest.mark.parametrize("ch,frames", [(2, 1000), (2, 333), (3, 333)])  # rows of a multiple of 4 floats (the 16-byte kernel of mode 0), and not
def test_batches_row_by_row(G, O, S, ch, frames, mode):
    n = frames * ch
    period, first = 96, 40
    k = R.steps_needed(first, period, n)
    xs = R.noise(S * 1000 + ch, S * n)
    st0 = (R.noise(9, S * ch * 4) * f32(0.1)).reshape(S * ch, 4)
    shared = R.sweep_table(O, "low_pass", 300, 6000, k)
    per_stream = np.stack([R.sweep_table(O, ("low_pass", "high_pass")[s % 2], 700 + 10 * s, 5000 - 20 * s, k) for s in range(S)])
    for table in (shared, per_stream):
        got, st = run(xs, ch, first, period, table, S=S, state=st0, mode=mode)
        for s in (range(S) if S <= 3 else (0, 1, 63, 64, 69)):
            one, one_st = run(xs[s * n: (s + 1) * n], ch, first, period, table if table.ndim == 2 else table[s], state=st0[s * ch: (s + 1) * ch], mode=mode)
            assert same(got[s * n: (s + 1) * n], one), (s, table.ndim)
            assert same(st[s * ch: (s + 1) * ch], one_st), (s, table.ndim)
            if mode == 0:
                want, _ = R.biquad_steps_ref(xs[s * n: (s + 1) * n], ch, first, period, table if table.ndim == 2 else table[s], st0[s * ch: (s + 1) * ch])
                assert same(one, want), s


# ---- state --------------------------------------------------------------------------------------------------------------------------------
BLOCKS = R.BLOCKS


def _blockwise(G, x, ch, period, table, how):
    """The stream cut into BLOCKS frames; block b runs through how[b % len(how)]: "b" rh_biquad mode 0, 0 / 1 rh_biquad_steps in that mode."""
    import torch

    from rodio_amd import _lib

    sd = torch.zeros(ch * 4, dtype=torch.float32, device="cuda")
    xd, yd, td = dev(x), torch.zeros(x.size, dtype=torch.float32, device="cuda"), dev(table.reshape(-1))
    f0 = 0
    for b, nf in enumerate(BLOCKS):
        h = how[b % len(how)]
        at = f0 * ch
        k0 = at // period
        if h == "b":
            _lib.check(_lib.lib.rh_biquad(vp(yd.data_ptr() + 4 * at), vp(xd.data_ptr() + 4 * at), nf, ch, 1, table[k0].ctypes.data_as(_lib.f32p), vp(sd.data_ptr()), 0, _st()), "rh_biquad")
        else:
            _lib.check(steps_call(yd.data_ptr() + 4 * at, xd.data_ptr() + 4 * at, nf, ch, 1, at, period, td.data_ptr() + 20 * k0, table.shape[0] - k0, 0, sd.data_ptr(), h), "rh_biquad_steps")
        f0 += nf
    torch.cuda.synchronize()
    return yd.cpu().numpy(), sd.cpu().numpy().reshape(ch, 4)


@pytest.mark.parametrize("ch,period", R.STATE_LAYOUTS)
def test_blocks_give_the_bits_of_one_pass_in_mode0(G, O, ch, period):
    frames = sum(BLOCKS)
    x = R.noise(77 + ch, frames * ch)
    for how in ((0,), ("b", 0)):
        table = R.plateau_table(O, ch, period, x.size, how)
        want, want_st = R.biquad_steps_ref(x, ch, 0, period, table)
        got, st = _blockwise(G, x, ch, period, table, how)
        assert same(got, want) and same(st, want_st), how


@pytest.mark.parametrize("how", R.STATE_HOWS)
@pytest.mark.parametrize("ch,period", R.STATE_LAYOUTS)
def test_a_stream_changes_between_rh_biquad_mode0_and_mode1_from_block_to_block(G, ch, period, how):
    x, table, want, want_st, _ = R.state_case(ch, period, how)
    got, st = _blockwise(G, x, ch, period, table, how)
    d = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"blocks {how}: max |got - f32 reference| = {d:.3e}")
    assert d <= TOL, (how, d)
    assert same(st[:, :2], want_st[:, :2]) and float(np.max(np.abs(st - want_st))) <= TOL, how


# ---- mode 1 -------------------------------------------------------------------------------------------------------------------------------
def test_the_tests_geometry_is_the_kernels(G):
    assert (G.BIQUAD_STEPS_RUN, G.BIQUAD_STEPS_TILE) == (8, 2048)  # kRun, kScanBlock * kRun of csrc/rh_live.hip (held against the source in test_live_filter_cpu.py)


@pytest.mark.parametrize("name", sorted(R.mode1_cases(8, 2048)))
def test_mode1_is_the_f64_recurrence_rounded_once(G, name):
    """One block, no state.  |got - ref64| <= 2^-23 max(1, peak of ref64): one rounding to f32 is at most 2^-24 |y|, the factor 2 covers the f64
    evaluation's own error, amplified by the filter.  And the project's filter contract against rodio's f32 recurrence on the same inputs:
    1e-5 (of which the reference itself keeps <= 5e-6: test_live_filter_cpu.py)."""
    x, ch, first, period, table, y32, y64 = R.mode1_case(name, G.BIQUAD_STEPS_RUN, G.BIQUAD_STEPS_TILE)
    got, _ = run(x, ch, first, period, table, mode=1)
    peak = float(np.max(np.abs(y64)))
    d64, d32 = float(np.max(np.abs(got.astype(np.float64) - y64))), float(np.max(np.abs(got.astype(np.float64) - y32.astype(np.float64))))
    print(f"{name}: |got - f64| = {d64:.3e} (bound {2.0**-23 * max(1.0, peak):.3e}, peak {peak:.3f}), |got - f32| = {d32:.3e}")
    assert d64 <= 2.0**-23 * max(1.0, peak), (name, d64, peak)
    assert d32 <= TOL, (name, d32)
    # ... and a row that starts 4 bytes behind a 16-byte boundary computes the same
    off, _ = run(x, ch, first, period, table, mode=1, lead=1)
    assert same(off, got)


def test_mode1_state_leaves_in_mode0s_layout(G):
    x, ch, first, period, table, y32, y64 = R.mode1_case("lp_up_in_run", G.BIQUAD_STEPS_RUN, G.BIQUAD_STEPS_TILE)
    got, st = run(x, ch, first, period, table, mode=1, state=np.zeros((ch, 4), f32))
    xs, ys = x.reshape(-1, ch), got.reshape(-1, ch)
    assert same(st[:, 0], xs[-1]) and same(st[:, 1], xs[-2])
    assert same(st[:, 2], ys[-1]) and same(st[:, 3], ys[-2])  # the f64 state, rounded as the samples were


@pytest.mark.parametrize("what", ["nine_channels", "in_place"])
def test_mode1_falls_back_to_the_bits_of_mode0(G, O, what):
    ch = 9 if what == "nine_channels" else 2
    frames, period, first = 3000, 441, 100
    x = R.noise(9, frames * ch)
    table = R.sweep_table(O, "low_pass", 300, 6000, R.steps_needed(first, period, x.size))
    want, want_st = R.biquad_steps_ref(x, ch, first, period, table)
    got, st = run(x, ch, first, period, table, state=np.zeros((ch, 4), f32), mode=1, in_place=what == "in_place")
    assert same(got, want) and same(st, want_st)


# ---- guard zones --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", [0, 1])
@pytest.mark.parametrize("S,ch,frames,lead", R.GUARD_SHAPES)
def test_nothing_is_written_outside_dst_and_state(G, S, ch, frames, lead, mode):
    """A short block, odd row addresses and the largest batch: dst and state between sentinel guards, the sources between poison."""
    from rodio_amd import _lib

    n = frames * ch
    period, first = R.GUARD_PERIOD, R.GUARD_FIRST
    k = R.steps_needed(first, period, n)
    cases = {s: R.guard_case(S, ch, frames, s) for s in R.guard_rows(S)}
    filler = cases[0]
    xs = [cases.get(s, filler)[0] for s in range(S)]
    table = np.stack([cases.get(s, filler)[1] for s in range(S)])
    src, dst, st = arena.src_arena_rows(xs, n, lead), arena.dst_arena_rows(S, n, n, lead), arena.state_arena(S * 4 * ch)
    tab = arena.src_arena(table.reshape(-1))
    _lib.check(steps_call(dst.ptr(), src.ptr(), frames, ch, S, first, period, tab.ptr(), k, 5 * k, st.ptr(), mode), "rh_biquad_steps")
    rows = dst.check().reshape(S, n)
    state = st.check().reshape(S, ch, 4)
    src.unchanged()
    tab.unchanged()
    for s, (_, _, want, want_st, _) in cases.items():
        if mode == 0:
            assert same(rows[s], want) and same(state[s], want_st), s
        else:
            assert float(np.max(np.abs(rows[s] - want))) <= TOL and float(np.max(np.abs(state[s] - want_st))) <= TOL, s
    # in place
    both = arena.inplace_arena_rows(xs, n, lead)
    st2 = arena.state_arena(S * 4 * ch)
    _lib.check(steps_call(both.ptr(), both.ptr(), frames, ch, S, first, period, tab.ptr(), k, 5 * k, st2.ptr(), mode), "rh_biquad_steps")
    rows2 = both.check().reshape(S, n)
    st2.check()
    last = max(cases)
    assert same(rows2[last], cases[last][2])  # (mode 1 in place is mode 0)


def test_bad_arguments_are_refused_and_an_empty_block_leaves_the_state(G):
    import torch

    x = torch.zeros(64, device="cuda")
    st = dev(np.arange(8, dtype=f32))
    p = x.data_ptr()
    for mode in (0, 1):
        assert steps_call(p, p, 8, 2, 1, 0, 0, p, 8, 0, None, mode) == 1  # period 0
        assert steps_call(p, p, 8, 0, 1, 0, 4, p, 8, 0, None, mode) == 1  # no channels
        assert steps_call(p, p, 8, 2, 1, 5, 10, p, 2, 0, None, mode) == 1  # 16 samples from 5 at period 10 reach 3 entries
        assert steps_call(p, p, 8, 2, 1, 5, 10, p, 3, 0, None, mode) == 0
        assert steps_call(p, p, 8, 2, 2, 5, 10, p, 3, 14, None, mode) == 1  # a stride below 5 * n_steps
        assert steps_call(p, p, 8, 2, 2, 5, 10, p, 3, 15, None, mode) == 0
        assert steps_call(p, p, 0, 2, 1, 0, 4, p, 0, 0, st.data_ptr(), mode) == 0  # nothing to do
    assert steps_call(p, p, 8, 2, 1, 0, 4, p, 8, 0, None, 2) == 1  # no such mode
    torch.cuda.synchronize()
    assert st.cpu().numpy().tolist() == list(range(8))


# ---- the chains of the host mirror ----------------------------------------------------------------------------------------------------------
def _need(exe):
    if not os.path.exists(exe):
        pytest.fail(f"{exe} is missing: run python rodio_amd/build.py")


@pytest.mark.parametrize("case", CASES)
def test_chains_over_the_library_are_the_stand_ins_bits(G, tmp_path, case):
    """Mode 0 (the default of live_low_pass / live_high_pass): the real kernels give what the CPU stand-in gives, which test_live_filter_cpu.py
    holds against the reference; and the same for two block sizes."""
    _need(LIVE_EXE), _need(FAKE_EXE)
    want, want_calls = run_case(tmp_path / "fake", case, 4096, exe=FAKE_EXE)
    for block in (256, 4096):
        got, calls = run_case(tmp_path / f"dev{block}", case, block, exe=LIVE_EXE)
        assert same(got, want), (case, block)
        if case != "seek":
            assert calls == want_calls


def test_the_sweep_chain_time_parallel_stays_within_the_contract(G, tmp_path):
    _need(LIVE_EXE), _need(FAKE_EXE)
    want, _ = run_case(tmp_path / "fake", "sweep", 4096, exe=FAKE_EXE)
    got, _ = run_case(tmp_path / "dev", "sweep_tp", 4096, exe=LIVE_EXE)
    d = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"sweep chain, live_filters_time_parallel: max |got - mode 0| = {d:.3e}")
    assert got.shape == want.shape and d <= TOL
