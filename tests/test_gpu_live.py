"""Parameters that change while a source plays, on the device: the stepped kernels (rh_amplify_steps, rh_channel_volume_steps)
bit for bit against a numpy-f32 restatement, and the live chains of the C++ host mirror (tests/cpp/live_test.cpp) against that
restatement plus the oracle for the fixed stages around it."""
import os

import numpy as np
import pytest

from test_live_params_cpu import LIVE_EXE, run_live

pytestmark = pytest.mark.gpu
f32 = np.float32


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def steps(first, period, n):
    j = np.arange(n, dtype=np.uint64) + np.uint64(first)
    return (j // np.uint64(period) - np.uint64(first // period)).astype(np.int64)


def amplify_ref(x, first, period, factors):
    return (x.astype(f32) * factors.astype(f32)[steps(first, period, x.size)]).astype(f32)


def channel_volume_ref(x, in_ch, out_ch, first, gp, gains, ff=0, fp=1, factors=None):
    fr = x.size // in_ch
    xf = x[: fr * in_ch].reshape(fr, in_ch).astype(f32)
    m = np.zeros(fr, f32)
    for c in range(in_ch):  # ((0 + s0) + s1 + ..) / C_in, in f32 (channel_volume.rs:71-88)
        m = (m + xf[:, c]).astype(f32)
    m = (m / f32(in_ch)).astype(f32)
    j = np.arange(fr * out_ch)
    y = (m[j // out_ch] * np.asarray(gains, f32).reshape(-1, out_ch)[steps(first, gp, j.size), j % out_ch]).astype(f32)
    if factors is not None:
        y = (y * np.asarray(factors, f32)[steps(ff, fp, j.size)]).astype(f32)
    return y


@pytest.fixture(scope="module")
def dev(rh):
    import torch

    rh.init(0)
    return torch


def table(rng, k, w=1):
    t = rng.uniform(-2, 2, (k, w)).astype(f32)
    t[::7] = 0.0
    t[3::11] = -0.5
    return t.reshape(-1) if w == 1 else t


@pytest.mark.parametrize("period", [1, 2, 3, 441, 480, 960, 1323, 250_000])
@pytest.mark.parametrize("where", ["aligned", "src+4B", "in_place"])
def test_amplify_steps_bits(rh, dev, period, where):
    rng = np.random.default_rng(period)
    n = 100_003
    first = 5 * period + period // 2  # in the middle of a period
    k = (first + n - 1) // period - first // period + 1
    fac = table(rng, k)
    x = rng.uniform(-1, 1, n + 1).astype(f32)
    xd = dev.from_numpy(x).cuda()
    if where == "aligned":
        got = rh.amplify_steps(xd[:n], first, period, fac).cpu().numpy()
        want = amplify_ref(x[:n], first, period, fac)
    elif where == "src+4B":
        out = dev.empty(n + 1, device="cuda")
        got = rh.amplify_steps(xd[1:], first, period, fac, out=out[1:]).cpu().numpy()
        want = amplify_ref(x[1:], first, period, fac)
    else:
        got = rh.amplify_steps(xd[1:], first, period, fac, out=xd[1:]).cpu().numpy()
        want = amplify_ref(x[1:], first, period, fac)
    assert np.array_equal(bits(got), bits(want))


@pytest.mark.parametrize("period,first", [(2**31 - 1, 2**31 - 1000), (2**31, 3 * 2**31 - 77), (2**31 + 5, 2**31 + 5 - 4096), (3 * 2**32 + 1, 3 * 2**32 - 3),
                                          (7, 2**40 + 3), (441, 2**35 * 441 - 1)])
def test_amplify_steps_index_at_every_boundary(rh, dev, period, first):
    """The 32-bit index of the kernel against the 64-bit quotient: large periods, a first sample far into the stream, a boundary
    inside the block."""
    n = 65_537
    x = np.ones(n, f32)
    k = (first + n - 1) // period - first // period + 1
    fac = np.arange(1, k + 1, dtype=f32)
    got = rh.amplify_steps(dev.from_numpy(x).cuda(), first, period, fac).cpu().numpy()
    assert np.array_equal(got, amplify_ref(x, first, period, fac))


def test_amplify_steps_equals_amplify_with_one_step(rh, dev):
    x = np.random.default_rng(1).uniform(-1, 1, 4099).astype(f32)
    xd = dev.from_numpy(x).cuda()
    a = rh.GpuSource(xd, 1, 44100).amplify(0.37).collect()
    b = rh.amplify_steps(xd, 123, 10**9, [0.37]).cpu().numpy()
    assert np.array_equal(bits(a), bits(b))


@pytest.mark.parametrize("in_ch,out_ch", [(1, 2), (2, 2), (6, 2), (2, 6), (3, 5), (1000, 2)])
@pytest.mark.parametrize("gp,first", [(1, 0), (441, 220), (480, 0), (3, 1), (100_000, 99_999)])
def test_channel_volume_steps_bits(rh, dev, in_ch, out_ch, gp, first):
    rng = np.random.default_rng(in_ch * 100 + out_ch + gp)
    frames = 20_011 if in_ch < 300 else 401
    x = rng.uniform(-1, 1, frames * in_ch + 1).astype(f32)
    k = (first + frames * out_ch - 1) // gp - first // gp + 1
    g = table(rng, k, out_ch)
    xd = dev.from_numpy(x).cuda()
    got = rh.channel_volume_steps(xd[: frames * in_ch], in_ch, out_ch, first, gp, g).cpu().numpy()
    assert np.array_equal(bits(got), bits(channel_volume_ref(x[: frames * in_ch], in_ch, out_ch, first, gp, g)))
    # a row that starts 4 bytes into its buffer
    got = rh.channel_volume_steps(xd[1:], in_ch, out_ch, first, gp, g).cpu().numpy()
    assert np.array_equal(bits(got), bits(channel_volume_ref(x[1:], in_ch, out_ch, first, gp, g)))


@pytest.mark.parametrize("in_ch,out_ch", [(2, 2), (1, 2), (6, 2), (2, 6)])
@pytest.mark.parametrize("gp,fp,first,ff", [(960, 480, 0, 0), (441, 441, 17, 17), (3, 2, 5, 1), (960, 480, 1000, 100_480)])
def test_fused_channel_volume_and_factor_equals_two_calls(rh, dev, in_ch, out_ch, gp, fp, first, ff):
    rng = np.random.default_rng(gp + fp + in_ch)
    frames = 30_001
    x = rng.uniform(-1, 1, frames * in_ch).astype(f32)
    n = frames * out_ch
    g = table(rng, (first + n - 1) // gp - first // gp + 1, out_ch)
    fac = table(rng, (ff + n - 1) // fp - ff // fp + 1)
    xd = dev.from_numpy(x).cuda()
    fused = rh.channel_volume_steps(xd, in_ch, out_ch, first, gp, g, ff, fp, fac).cpu().numpy()
    two = rh.amplify_steps(rh.channel_volume_steps(xd, in_ch, out_ch, first, gp, g), ff, fp, fac).cpu().numpy()
    assert np.array_equal(bits(fused), bits(two))
    assert np.array_equal(bits(fused), bits(channel_volume_ref(x, in_ch, out_ch, first, gp, g, ff, fp, fac)))
    # one step everywhere: rh_channel_volume, then rh_amplify
    one = rh.channel_volume_steps(xd, in_ch, out_ch, 0, 1 << 40, g[:1], 0, 1 << 40, fac[:1]).cpu().numpy()
    ref = rh.GpuSource(xd, in_ch, 48000)
    ref = rh.ChannelVolume(ref, g[0]).amplify(float(fac[0])).collect()
    assert np.array_equal(bits(one), bits(ref))


def test_bad_arguments_are_refused(rh, dev):
    from rodio_amd import _lib

    lib = _lib.lib
    x = dev.zeros(64, device="cuda")
    p = x.data_ptr()
    assert lib.rh_amplify_steps(p, p, 64, 0, 0, p, 64, None) == 1  # period 0
    assert lib.rh_amplify_steps(p, p, 64, 5, 10, p, 6, None) == 1  # 64 samples from 5 at period 10 reach 7 steps
    assert lib.rh_amplify_steps(p, p, 64, 5, 10, p, 7, None) == 0
    assert lib.rh_channel_volume_steps(p, p, 4, 2, 17, 0, 1, p, 64, 0, 1, None, 0, None) == 1  # out_ch > 16
    assert lib.rh_channel_volume_steps(p, p, 4, 2, 2, 0, 0, p, 64, 0, 1, None, 0, None) == 1
    assert lib.rh_channel_volume_steps(p, p, 4, 2, 2, 0, 2, p, 3, 0, 1, None, 0, None) == 1  # 8 outputs at period 2: 4 steps
    assert lib.rh_channel_volume_steps(p, p, 4, 2, 2, 0, 2, p, 4, 0, 3, p, 2, None) == 1    # ... and 3 factor steps
    assert lib.rh_channel_volume_steps(p, p, 4, 2, 2, 0, 2, p, 4, 0, 3, p, 3, None) == 0
    dev.cuda.synchronize()


# ---------------------------------------------------------------------------------------------- chains through the host mirror
def _need_driver():
    if not os.path.exists(LIVE_EXE):
        pytest.fail(f"{LIVE_EXE} is missing: run python rodio_amd/build.py")


@pytest.mark.parametrize("case", ["player", "lowpass", "seek"])
def test_live_chain_through_the_host_mirror(O, dev, tmp_path, case):
    """1. Player-like: 44.1 kHz stereo -> live_amplify(1.0) -> periodic_access(5 ms) with a volume schedule that is a function of the
    access index (0, a negative value, a dB step); 2. live_amplify -> low_pass(200) -> access point; 4. try_seek in mid-stream.
    The output is the same for block_frames 256 and 32768, and equals the restatement (+ the oracle's filter)."""
    _need_driver()
    from test_live_params_cpu import expected_chain

    outs = []
    for block in (256, 32768):
        got, calls = run_live(tmp_path, case, block, exe=LIVE_EXE)
        outs.append(got)
        want, want_calls = expected_chain(O, case)
        if case == "seek":  # the count goes on over the samples served; what was computed ahead of the seek is not called again
            top = max(k for _, k in calls)
            assert calls == [(5, k) for k in range(top + 1)] and top >= got.size // 441
        else:
            assert calls == want_calls
        assert got.shape == want.shape, (got.shape, want.shape)
        if case == "lowpass":
            assert np.max(np.abs(got - want)) <= 1e-5
        else:
            assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


def test_spatial_player_chain_through_the_mixer(O, dev, tmp_path):
    """3. SpatialPlayer-like: a moving emitter every 10 ms inside a 5 ms volume, handed to GpuMixer(2, 48000) on the device
    together with two plain sources; against O.Mixer over the expected chains."""
    _need_driver()
    from test_live_params_cpu import expected_chain

    outs = []
    for block in (256, 32768):
        got, _ = run_live(tmp_path, "spatial_mixer", block, exe=LIVE_EXE)
        outs.append(got)
    want, _ = expected_chain(O, "spatial_mixer")
    assert outs[0].shape == want.shape
    assert np.max(np.abs(outs[0] - want)) <= 1e-6
    assert np.array_equal(bits(outs[0]), bits(outs[1]))


@pytest.mark.parametrize("block", [256, 32768])
def test_spatial_player_chain_alone(O, dev, tmp_path, block):
    """The SpatialPlayer-like chain without the mixer: the fused tail (one rh_channel_volume_steps launch a block) is the restatement's bits."""
    _need_driver()
    from test_live_params_cpu import expected_chain

    got, calls = run_live(tmp_path, "spatial", block, exe=LIVE_EXE)
    want, want_calls = expected_chain(O, "spatial")
    assert calls == want_calls
    assert np.array_equal(bits(got), bits(want))
