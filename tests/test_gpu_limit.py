"""The time-parallel limiter (rodio_amd/csrc/rh_limit.hip) against the oracle's per-sample Limit (limit.rs:853-988).

<= 1e-5 abs (device log2f / exp2f, re-associated scans), every channel layout the reference has a struct for (LimitMono,
LimitStereo, LimitMulti), tile and lane boundaries, many streams per launch, state carried across blocks, coefficients that
make the look-back walk several windows, and the reference's own behavioural tests (tests/limit.rs:7-155) on the GPU path.
"""
import os

import numpy as np
import pytest
from conftest import knobs  # noqa: E402
from dynamics_signals import limit_f64 as _limit_f64  # limit.rs:853-988 in float64: the ground truth of the ill-conditioned setting

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _signal(seed, n, ch, loud=2.0):
    """Programme-like material that crosses the threshold often: a few tones with a slow envelope + noise bursts."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((n, ch))
    for c in range(ch):
        env = 0.15 + 0.85 * np.abs(np.sin(2 * np.pi * t / (3000.0 + 977.0 * c) + rng.uniform(0, 6)))
        x[:, c] = loud * env * np.sin(2 * np.pi * t * (0.01 + 0.003 * c)) + 0.1 * rng.standard_normal(n)
    if n > 64:
        k = int(rng.integers(0, n - 32))
        x[k: k + 32] *= 3.0  # a transient
    return x.astype(np.float32).reshape(-1)


def _oracle(O, x, ch, sr, **kw):
    return O.TestSource(x, ch, sr).limit(**kw).collect()


@pytest.mark.parametrize("ch", [1, 2, 3, 4, 6])
@pytest.mark.parametrize("frames", [1, 7, 255, 256, 257, 511, 512, 513, 1023, 1024, 1025, 5000, 70001])
def test_limiter_matches_oracle_at_tile_and_lane_boundaries(G, O, ch, frames):
    x = _signal(100 * ch + frames % 97, frames, ch)
    for kw in (dict(), dict(threshold=-6.0, knee_width=0.5, attack_ns=3_000_000, release_ns=12_000_000)):
        ref = _oracle(O, x, ch, 48000, **kw)
        out = G.TestSource(x, ch, 48000).limit(**kw).collect()
        assert out.shape == ref.shape
        assert float(np.max(np.abs(out - ref))) <= TOL, (ch, frames, kw)


def test_limiter_is_actually_limiting_in_these_tests(G, O):
    x = _signal(5, 20000, 2)
    out = G.TestSource(x, 2, 48000).limit().collect()
    # (transients pass an attack of 5 ms; the sustained level is what comes down)
    assert float(np.max(np.abs(x))) > 2.0 and float(np.sqrt(np.mean(out[4000:] ** 2))) < 0.6 * float(np.sqrt(np.mean(x[4000:] ** 2)))
    assert float(np.max(np.abs(out - x))) > 0.5


# (2, 300, 16384) and (2, 1100, 2100): more streams than resident workgroups on the 8-wave and the 4-wave geometry -- the
# variant that walks the next tile's integrator look-back at the current tile's poll point (k_limit_scan<.., SKEW>)
@pytest.mark.parametrize("ch,S,frames", [(2, 5, 40000), (1, 33, 9001), (2, 64, 16384), (3, 7, 12000), (2, 300, 2048), (2, 300, 16384), (2, 1100, 2100), (1, 520, 9000)])
def test_limiter_many_streams_one_launch(G, O, ch, S, frames):
    import torch

    xs = [_signal(900 + s, frames, ch, loud=0.5 + 0.05 * (s % 40)) for s in range(S)]
    x = torch.from_numpy(np.stack(xs)).cuda()
    out = G.limit_batch(x, ch, 44100, threshold=-3.0).cpu().numpy()
    for s in range(S):
        ref = _oracle(O, xs[s], ch, 44100, threshold=-3.0)
        assert float(np.max(np.abs(out[s] - ref))) <= TOL, s


def test_limiter_one_poll_point_variant_with_few_streams(G, O):
    """RH_LIMIT_SKEW=1 forces the one-poll-point variant where the host would not choose it (few streams: the predecessors of a
    workgroup's next tile are other workgroups' next tiles, so the workgroups wait for each other in a chain): slow, still right."""
    import torch

    S, frames, ch = 6, 200000, 2
    xs = [_signal(1200 + s, frames, ch, loud=1.2) for s in range(S)]
    x = torch.from_numpy(np.stack(xs)).cuda()
    outs = {}
    for skew in ("0", "1"):
        with knobs(RH_LIMIT_SKEW=skew):
            outs[skew] = G.limit_batch(x, ch, 48000).cpu().numpy()
    for s in range(S):
        ref = _oracle(O, xs[s], ch, 48000)
        assert float(np.max(np.abs(outs["1"][s] - ref))) <= TOL, s
    assert np.array_equal(outs["0"], outs["1"])  # the same compositions in the same order: the same bits
    G.async_status()


@pytest.mark.parametrize("S,frames", [(5, 40000), (70, 16384), (300, 13000), (3, 6144 * 3), (3, 6144 * 3 + 1)])
def test_limiter_io_wave_variant(G, O, S, frames):
    """RH_LIMIT_NIO=1: the variant with two I/O waves behind six computing waves (tiles of 6144 frames; the computing waves' polls
    then travel alone in vmcnt).  Measured slower than the shipped geometry, kept selectable so that the measurement
    can be repeated -- and right: short last tiles, streams that end on a tile boundary, more streams than workgroups (one poll
    point), state carried across two blocks."""
    import torch

    ch = 2
    xs = [_signal(3100 + s, frames, ch, loud=0.6 + 0.07 * (s % 30)) for s in range(S)]
    x = torch.from_numpy(np.stack(xs)).cuda()
    with knobs(RH_LIMIT_NIO="1"):
        out = G.limit_batch(x, ch, 48000).cpu().numpy()
        half = (frames // 2) * ch
        st = torch.zeros((S, ch * 2), device="cuda")
        a = G.limit_batch(x[:, :half].contiguous(), ch, 48000, state=st).cpu().numpy()
        b = G.limit_batch(x[:, half:].contiguous(), ch, 48000, state=st).cpu().numpy()
    shipped = G.limit_batch(x, ch, 48000).cpu().numpy()
    for s in range(min(S, 12)):
        ref = _oracle(O, xs[s], ch, 48000)
        assert float(np.max(np.abs(out[s] - ref))) <= TOL, s
        assert float(np.max(np.abs(np.concatenate([a[s], b[s]]) - ref))) <= TOL, s
    assert float(np.max(np.abs(out - shipped))) <= 2e-6
    G.async_status()


@pytest.mark.parametrize("ch", [1, 2, 5])
def test_limiter_state_carried_across_blocks_equals_one_pass(G, O, ch):
    import torch

    S, frames = 3, 50000
    xs = [_signal(40 + s, frames, ch) for s in range(S)]
    refs = [_oracle(O, x, ch, 48000) for x in xs]
    x = torch.from_numpy(np.stack(xs)).cuda()
    state = torch.zeros((S, 2 * ch), device="cuda")
    rng = np.random.default_rng(ch)
    outs, a = [], 0
    while a < frames:
        b = min(frames, a + int(rng.choice([1, 3, 64, 500, 511, 4096, 20000])))
        blk = x[:, a * ch: b * ch].contiguous()
        # (rows that are not 16-byte multiples make the library take the reference-order kernel for that block: same state)
        outs.append(G.limit_batch(blk, ch, 48000, state=state))
        a = b
    got = torch.cat(outs, dim=1).cpu().numpy()
    for s in range(S):
        assert float(np.max(np.abs(got[s] - refs[s]))) <= TOL, s
    # and the state itself is the reference's {integrator, peak}: continuing with silence decays like the oracle does
    tail = np.zeros(4000 * ch, np.float32)
    ref_tail = _oracle(O, np.concatenate([xs[0], tail + 1e-3]), ch, 48000)[frames * ch:]
    st0 = state[:1].clone()
    got_tail = G.limit_batch(torch.from_numpy(tail + 1e-3).cuda()[None, :], ch, 48000, state=st0).cpu().numpy()[0]
    assert float(np.max(np.abs(got_tail - ref_tail))) <= TOL


@pytest.mark.parametrize("attack_ms,release_ms,tol", [(5, 100, TOL), (20, 1000, TOL), (800, 3000, None)])
def test_limiter_lookback_walks_several_windows(G, O, attack_ms, release_ms, tol):
    """r^(64 tiles) is not negligible for any of these (64 tiles = 1.4 s at most): a tile composes several windows of
    aggregates, or meets an inclusive state, before it knows its start state.  The last setting (attack 0.8 s, release 3 s) is
    outside what a limiter is used with and ill-conditioned in f32 -- the reference's own recurrence I = r*I + (1-r)*g then
    carries ~1e-4 dB of accumulated rounding that depends on the evaluation order; it is here for the control flow, with the
    bound that conditioning allows."""
    ch, frames = 2, 400000
    x = _signal(77, frames, ch)
    kw = dict(threshold=-9.0, knee_width=2.0, attack_ns=attack_ms * 1_000_000, release_ns=release_ms * 1_000_000)
    ref = _oracle(O, x, ch, 48000, **kw)
    out = G.TestSource(x, ch, 48000).limit(**kw).collect()
    err = float(np.max(np.abs(out - ref)))
    print(f"[limit attack {attack_ms} ms release {release_ms} ms] err={err:.3e}")
    if tol is not None:
        assert err <= tol
        return
    # the ill-conditioned setting: no fixed bound against the reference's f32 recurrence, whose own accumulated rounding depends on
    # the evaluation order -- the GPU result must be no further from the float64 truth than the reference itself is (x2 + 1e-7)
    n64 = 120000  # frames: the python loop below costs a second per 100 000 samples
    truth = _limit_f64(x[: n64 * ch], ch, 48000, **kw)
    e_ref = float(np.max(np.abs(ref[: n64 * ch] - truth)))
    e_gpu = float(np.max(np.abs(out[: n64 * ch] - truth)))
    print(f"[limit attack {attack_ms} ms release {release_ms} ms] |reference - f64| = {e_ref:.3e}, |gpu - f64| = {e_gpu:.3e}")
    assert e_gpu <= 2.0 * e_ref + 1e-7
    assert err <= 5e-4  # and the two f32 evaluations stay together over the whole stream


def test_limiter_full_block_every_sample(G, O):
    # one full-size stream of the benchmark shape (1 Mi stereo frames), every sample compared
    ch, frames = 2, 1 << 20
    x = _signal(3, frames, ch, loud=1.5)
    ref = _oracle(O, x, ch, 48000)
    out = G.TestSource(x, ch, 48000).limit().collect()
    err = float(np.max(np.abs(out - ref)))
    print(f"[limit 1 Mi frames] err={err:.3e}")
    assert err <= TOL
    G.async_status()  # rh_async_status: no hand-off inside the scan expired in anything launched so far


def test_limiter_reference_order_kernel_agrees(G, O):
    # RH_LIMIT_SEQ=1 forces the one-lane-per-stream kernel (what unaligned batches take)
    x = _signal(9, 30000, 2)
    ref = _oracle(O, x, 2, 48000)
    with knobs(RH_LIMIT_SEQ="1"):
        seq = G.TestSource(x, 2, 48000).limit().collect()
    par = G.TestSource(x, 2, 48000).limit().collect()
    assert float(np.max(np.abs(seq - ref))) <= TOL and float(np.max(np.abs(par - seq))) <= TOL


def test_limiter_unaligned_rows_and_partial_frames(G, O):
    import torch

    # rows of 3*1001 floats are not 16-byte multiples: the batch goes through the reference-order kernel
    xs = [_signal(60 + s, 1001, 3) for s in range(4)]
    out = G.limit_batch(torch.from_numpy(np.stack(xs)).cuda(), 3, 48000).cpu().numpy()
    for s in range(4):
        assert float(np.max(np.abs(out[s] - _oracle(O, xs[s], 3, 48000)))) <= TOL
    # a stream that ends inside a frame: every sample is limited, none dropped
    x = _signal(8, 5000, 2)[:-1]
    ref = _oracle(O, x, 2, 48000)
    got = G.TestSource(x, 2, 48000).limit().collect()
    assert got.shape == ref.shape and float(np.max(np.abs(got - ref))) <= TOL


# ---- the reference's behavioural tests (tests/limit.rs) on the GPU path ---------------------------------------------
def _sine(freq, amp, n, sr=48000):  # SineWave::new(f).amplify(a): 48 kHz mono (sine.rs:23-27)
    from conftest import sine_generator

    return (sine_generator(sr, freq, n) * np.float32(amp)).astype(np.float32)


def test_reference_limiting_works(G):  # tests/limit.rs:7-40
    x = _sine(440.0, 3.0, 2600)
    y = G.TestSource(x, 1, 48000).limit(threshold=-6.0, knee_width=0.5, attack_ns=3_000_000, release_ns=12_000_000).collect()
    settled = float(np.max(np.abs(y[1500:])))
    assert 0.4 <= settled <= 0.6 and settled < 0.8


def test_reference_passthrough_below_threshold(G):  # tests/limit.rs:43-63
    x = _sine(1000.0, 0.2, 880)
    y = G.TestSource(x, 1, 48000).limit(threshold=-6.0).collect()
    assert float(np.max(np.abs(y - x))) < 0.01


@pytest.mark.parametrize("thr,peak", [(-1.0, 0.89), (-3.0, 0.71), (-6.0, 0.50)])
def test_reference_limiter_with_different_settings(G, thr, peak):  # tests/limit.rs:66-108
    x = _sine(440.0, 2.0, 2000)
    y = G.TestSource(x, 1, 48000).limit(threshold=thr, knee_width=1.0, attack_ns=2_000_000, release_ns=10_000_000).collect()
    p = float(np.max(np.abs(y[1000:])))
    assert peak - 0.1 <= p <= peak + 0.1


def test_reference_limiter_stereo_processing(G, O):  # tests/limit.rs:111-155
    i = np.arange(1000, dtype=np.float32)
    st = np.stack([np.sin(i * np.float32(0.01)) * np.float32(1.5), np.sin(i * np.float32(0.01)) * np.float32(0.8)], axis=1).astype(np.float32).reshape(-1)
    y = G.SamplesBuffer(2, 44100, st).limit(threshold=-3.0).collect()
    assert float(np.max(np.abs(y[0::2]))) <= 1.5 and float(np.max(np.abs(y[1::2]))) <= 1.5
    assert float(np.max(np.abs(y - O.SamplesBuffer(2, 44100, st).limit(threshold=-3.0).collect()))) <= TOL


def test_an_expired_hand_off_is_reported_and_poisons_the_output(G, O):
    """The failure path of the handle-less scan kernels (never seen on a healthy device): with the poll budget forced to zero
    (RH_SCAN_SPIN_LIMIT=0: a hand-off that is not there at the first look counts as lost) tiles give up, their output is NaN --
    never plausible audio -- and rh_async_status reports RH_ERR_TIMEOUT once."""
    import torch

    from rodio_amd import _lib

    G.async_status()  # clean slate
    x = torch.from_numpy(np.stack([_signal(70 + s, 1 << 18, 2) for s in range(64)])).cuda()
    good = G.limit_batch(x, 2, 48000).clone()
    good_b = G.biquad_batch(x, G.biquad_coeffs("low_pass", 200, 0.5, 48000), mode=1).clone()
    torch.cuda.synchronize()
    with knobs(RH_SCAN_SPIN_LIMIT="0"):
        bad = 0
        for _ in range(12):  # tiles of one stream run side by side: some first looks come too early
            out = G.limit_batch(x, 2, 48000)
            torch.cuda.synchronize()
            bad += int(torch.isnan(out).sum())
            if bad:
                break
        co = G.biquad_coeffs("low_pass", 200, 0.5, 48000)
        outb = G.biquad_batch(x, co, mode=1)
        torch.cuda.synchronize()
        bad += int(torch.isnan(outb).sum())
    assert bad > 0, "no hand-off was late in thirteen launches of 64 x 32 tiles: the test lost its premise"
    with pytest.raises(_lib.RhError) as e:
        G.async_status()
    assert e.value.status == 5  # RH_ERR_TIMEOUT
    G.async_status()  # sticky once, then clear
    # ... and the next launches are whole again, bit for bit what they were before the failure: a reported failure makes every stream's
    # next launch write its hand-off tables afresh instead of trusting what the failed launch left
    for _ in range(3):
        out = G.limit_batch(x, 2, 48000)
        outb = G.biquad_batch(x, co, mode=1)
        torch.cuda.synchronize()
        assert not bool(torch.isnan(out).any()) and torch.equal(out, good)
        assert torch.equal(outb, good_b)
    G.async_status()
