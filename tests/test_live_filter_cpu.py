"""Live filters (live_low_pass / live_high_pass retuned by periodic_access closures: BltFilter::to_low_pass / to_high_pass, blt.rs:68-91,
234-252), host logic: the reference of the filter tests pinned to the oracle, the chains of the C++ host mirror through
tests/cpp/live_filter_test_fake (the mirror over the CPU stand-ins fake_device.cpp + fake_live.cpp + fake_live_filter.cpp) against that
reference bit for bit, and the stated conditions of the mode 1 tests of tests/test_gpu_live_filter.py.  The helpers here restate the
chains for that file too."""
import functools
import os
import re
import subprocess

import numpy as np
import pytest

import live_filter_ref as R
from test_live_params_cpu import expected_calls

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIVE_EXE = os.path.join(ROOT, "tests", "cpp", "live_filter_test")
FAKE_EXE = os.path.join(ROOT, "tests", "cpp", "live_filter_test_fake")
f32 = np.float32
CASES = ["sweep", "switch", "two_access", "behind_amplify", "fixed", "seek"]
FRAMES = 40_003
SEEK_AT = 30_001     # samples served before try_seek(500 ms): inside a frame and inside an access period
SEEK_FRAME = 24_000  # 500 ms at 48 kHz
U5, U7 = 480, 672    # rh_periodic_update_samples(5 ms / 7 ms, 48000, 2)


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def source():
    return R.noise(2024, 2 * FRAMES)


def sweep_freq(k):
    """live_filter_test.cpp's sweep_freq(): 100 Hz, about 6 % up per access, to 8 kHz."""
    f = 100
    for _ in range(k):
        if f >= 8000:
            break
        f = min(8000, f + f // 16 + 1)
    return f


def run_case(d, case, block, exe=FAKE_EXE, pull=0):
    d.mkdir(parents=True, exist_ok=True)
    source().tofile(d / "src_0.f32")
    (d / "seek.txt").write_text(f"{SEEK_AT}\n")
    r = subprocess.run([exe, "run", str(d), case, str(block)] + ([str(pull)] if pull else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    calls = [tuple(int(v) for v in ln.split()) for ln in (d / "calls.txt").read_text().split("\n") if ln.strip()]
    return np.fromfile(d / "out.f32", dtype=f32), calls


def _sweep_table(O, n_steps):
    return np.array([O.blt_coeffs("low_pass", sweep_freq(k), 0.5, R.RATE) for k in range(n_steps)], f32)


@functools.lru_cache(maxsize=None)
def expected(case):
    """(samples, calls) rodio's chain gives for live_filter_test.cpp's case: the closures' schedule restated, the filter by the reference."""
    from oracle import rodio_oracle as O

    x = source()
    n = x.size
    if case == "sweep":
        return R.biquad_steps_ref(x, 2, 0, U5, _sweep_table(O, n // U5 + 1))[0], expected_calls([(5, U5)], n)
    if case == "switch":
        table = np.array([O.blt_coeffs("low_pass", 1000 + 50 * k, 0.5, R.RATE) if k < 30 else O.blt_coeffs("high_pass", 1000 + 20 * min(k - 30, 200), 0.5, R.RATE)
                          for k in range(n // U5 + 1)], f32)
        return R.biquad_steps_ref(x, 2, 0, U5, table)[0], expected_calls([(5, U5)], n)
    if case == "two_access":
        # the 7 ms access is further down the chain: at one sample it runs first, so the 5 ms one has the last word there; what holds at a
        # sample is what the last call at or before it set -- a table with the period gcd(480, 672) = 96
        g = int(np.gcd(U5, U7))
        calls = expected_calls([(7, U7), (5, U5)], n)
        ev = sorted([(k * U7, 0, O.blt_coeffs("low_pass", 8000 - sweep_freq(k) // 2, 0.5, R.RATE)) for k in range(n // U7 + 1)] +
                    [(k * U5, 1, O.blt_coeffs("low_pass", sweep_freq(k), 0.707, R.RATE)) for k in range(n // U5 + 1)], key=lambda e: e[:2])
        table, i, cur = [], 0, None
        for s in range(0, n, g):
            while i < len(ev) and ev[i][0] <= s:
                cur = ev[i][2]
                i += 1
            table.append(cur)
        return R.biquad_steps_ref(x, 2, 0, g, np.array(table, f32))[0], calls
    if case == "behind_amplify":
        vol = np.array([f32(0.5) + f32(0.125) * f32(k % 5) for k in range(n // U5 + 1)], f32)
        y = (x * vol[np.arange(n) // U5]).astype(f32)
        return R.biquad_steps_ref(y, 2, 0, U5, _sweep_table(O, n // U5 + 1))[0], expected_calls([(5, U5)], n)
    if case == "fixed":
        return O.TestSource(x, 2, R.RATE).low_pass(200).collect(), []
    if case == "seek":
        # in front of the seek: the stream from its start.  Behind it: the upstream from 500 ms on through a filter that starts from zero
        # (blt.rs:350-377) while the access count goes on from the consumer's frame (periodic.rs keeps its phase); the sample that
        # completes the consumer's open frame is dropped
        table = _sweep_table(O, 2 * n // U5 + 2)
        pre = R.biquad_steps_ref(x[: SEEK_AT + 1], 2, 0, U5, table)[0][:SEEK_AT]
        at = SEEK_AT - SEEK_AT % 2
        post = R.biquad_steps_ref(x[2 * SEEK_FRAME:], 2, at, U5, table[at // U5:])[0][SEEK_AT % 2:]
        return np.concatenate([pre, post]), None
    raise ValueError(case)


def _need_fake():
    if not os.path.exists(FAKE_EXE):
        pytest.fail(f"{FAKE_EXE} is missing: run python rodio_amd/build.py")


# ------------------------------------------------------------------------------------------------------------------ tests
@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("kind,freq", [("low_pass", 200), ("high_pass", 1000), ("low_pass", 5000)])
def test_the_reference_with_one_entry_is_the_oracles_filter(O, ch, kind, freq):
    x = R.noise(ch * 10 + freq, 3001 * ch)
    want = getattr(O.TestSource(x, ch, R.RATE), kind)(freq).collect()
    got, st = R.biquad_steps_ref(x, ch, 12345, 10**9, [O.blt_coeffs(kind, freq, 0.5, R.RATE)])
    assert np.array_equal(bits(got), bits(want))
    xs, ys = x.reshape(-1, ch), want.reshape(-1, ch)
    assert np.array_equal(bits(st), bits(np.stack([xs[-1], xs[-2], ys[-1], ys[-2]], axis=1)))
    # ... and a table of equal entries, cut into two blocks with the state carried, is the same filter
    a, sa = R.biquad_steps_ref(x[: 1000 * ch], ch, 0, 7, [O.blt_coeffs(kind, freq, 0.5, R.RATE)] * (3001 * ch // 7 + 1))
    b, _ = R.biquad_steps_ref(x[1000 * ch:], ch, 1000 * ch, 7, [O.blt_coeffs(kind, freq, 0.5, R.RATE)] * (3001 * ch // 7 + 1), sa)
    assert np.array_equal(bits(np.concatenate([a, b])), bits(want))


def test_the_python_mirror_states_the_kernels_geometry(rh):
    src = open(os.path.join(ROOT, "rodio_amd", "csrc", "rh_live.hip")).read()
    block = int(re.search(r"constexpr int kScanBlock = (\d+);", src).group(1))
    run = int(re.search(r"constexpr int kRun = (\d+);", src).group(1))
    assert (rh.BIQUAD_STEPS_RUN, rh.BIQUAD_STEPS_TILE) == (run, block * run)


@pytest.mark.parametrize("case", CASES)
@pytest.mark.parametrize("block", [256, 32768])
def test_chains_bit_exact_on_the_stand_in(tmp_path, case, block):
    """A low_pass sweep under periodic_access(5 ms); the kind switched to high_pass in mid-stream; two access points with different periods
    reaching one filter; a live filter behind a live_amplify; a chain with no access point; try_seek."""
    _need_fake()
    got, calls = run_case(tmp_path, case, block)
    want, want_calls = expected(case)
    assert got.shape == want.shape
    assert np.array_equal(bits(got), bits(want)), int(np.flatnonzero(bits(got) != bits(want))[0])
    if case == "seek":  # the count goes on over the samples served: what was computed ahead of the seek is not called again
        assert calls == [(5, k) for k in range(max(k for _, k in calls) + 1)] and max(k for _, k in calls) >= got.size // U5
    else:
        assert calls == want_calls
    if case == "fixed":  # ... the bits of the fixed low_pass in the reference's order
        assert np.array_equal(bits(got), bits(np.fromfile(tmp_path / "plain.f32", dtype=f32)))


@pytest.mark.parametrize("block,pull", [(256, 1), (256, 7), (4096, 7), (1000, 2000), (4096, 8192)])
def test_any_pull_size_gives_the_same_stream(tmp_path, block, pull):
    """Pulls of 1 sample, 7 samples and whole blocks."""
    _need_fake()
    got, calls = run_case(tmp_path, "sweep", block, pull=pull)
    want, want_calls = expected("sweep")
    assert np.array_equal(bits(got), bits(want)) and calls == want_calls


def test_time_parallel_chain_runs_the_same_schedule(tmp_path):
    """On the stand-in both modes compute the reference's order: live_filters_time_parallel() changes nothing but the mode that is passed."""
    _need_fake()
    got, calls = run_case(tmp_path, "sweep_tp", 4096)
    want, want_calls = expected("sweep")
    assert np.array_equal(bits(got), bits(want)) and calls == want_calls


def test_argument_errors_through_the_stand_in():
    _need_fake()
    r = subprocess.run([FAKE_EXE, "args"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    lines = r.stdout.strip().split("\n")
    assert lines[:6] == ["1", "1", "1", "1", "1", "0"]  # period 0, a short table, a bad stride, no channels, no such mode: RH_ERR_INVALID; an empty block: RH_OK
    assert lines[6].split() == [str(v) for v in range(1, 9)]  # ... which leaves the state as it was


def test_a_format_change_in_front_of_a_live_filter_is_refused():
    _need_fake()
    r = subprocess.run([FAKE_EXE, "refuse"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 3, (r.stdout, r.stderr)
    assert r.stdout.split()[0] == "3" and "uniform" in r.stdout  # RH_ERR_UNSUPPORTED, and what to do about it


# ---- the stated conditions of the mode 1 tests: on each of their inputs rodio's f32 recurrence alone is within 5e-6 of the f64 one -------------
COND = 5e-6


@pytest.mark.parametrize("name", sorted(R.mode1_cases(8, 2048)))
def test_condition_of_the_mode1_cases(rh, name):
    x, ch, first, period, table, y32, y64 = R.mode1_case(name, rh.BIQUAD_STEPS_RUN, rh.BIQUAD_STEPS_TILE)
    d = float(np.max(np.abs(y32.astype(np.float64) - y64)))
    print(f"{name}: |f32 - f64| = {d:.3e}, peak {float(np.max(np.abs(y64))):.3f}")
    assert d <= COND


@pytest.mark.parametrize("how", R.STATE_HOWS)
@pytest.mark.parametrize("ch,period", R.STATE_LAYOUTS)
def test_condition_of_the_carried_state_cases(ch, period, how):
    _, _, y32, _, y64 = R.state_case(ch, period, how)
    assert float(np.max(np.abs(y32.astype(np.float64) - y64))) <= COND


@pytest.mark.parametrize("S,ch,frames,lead", R.GUARD_SHAPES)
def test_condition_of_the_guard_zone_cases(S, ch, frames, lead):
    for s in R.guard_rows(S):
        _, _, y32, _, y64 = R.guard_case(S, ch, frames, s)
        assert float(np.max(np.abs(y32.astype(np.float64) - y64))) <= COND


def test_condition_of_the_sweep_chain(O):
    x = source()
    y64, _ = R.biquad_steps_ref(x, 2, 0, U5, _sweep_table(O, x.size // U5 + 1), dtype=np.float64)
    assert float(np.max(np.abs(expected("sweep")[0].astype(np.float64) - y64))) <= COND
