"""tests/spatial_mix_ref.py -- the numpy restatement the GPU tests of rh_spatial_mix_block compare with -- held against the oracle.
Constant tables: the bits of `mixer::mixer(2, rate)` fed `Spatial(src, ..).amplify(f)` / `ChannelVolume(src, gains)`.  Stepped tables: the
oracle run PIECEWISE -- every stretch of the adapter's output between two changes comes from ChannelVolume (and Amplify) with that
stretch's values, the stretches are concatenated, and the oracle's mixer converts and sums the result."""
import numpy as np
import pytest

import spatial_mix_ref as R

RATES = [(44100, 48000), (48000, 48000), (96000, 44100), (22050, 48000)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def whole(x, in_ch, rate, to_rate, **tables):
    """A whole ended stream as one block's source."""
    n = len(x) // in_ch
    F, T = R.reduced(rate, to_rate)
    return R.Src(x, in_ch, rate, R.stream_out_frames(n, F, T), last=n - 1, **tables)


@pytest.mark.parametrize("in_ch", [1, 2, 6])
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_constant_tables_are_the_oracles_mixer(O, in_ch, rate, to_rate):
    rng = np.random.default_rng(100 * in_ch + rate % 97)
    xs = [rng.uniform(-1, 1, n * in_ch).astype(np.float32) for n in (301, 157, 1, 2)]
    pos = [rng.uniform(-2, 2, (3, 3)).astype(np.float32) for _ in xs]
    fac = [np.float32(v) for v in (0.7, 1.0, -1.3, 0.25)]
    vols = rng.uniform(-1, 1, 2).astype(np.float32)
    # Amplify(Spatial(..)): SpatialPlayer's chain
    mx = O.Mixer(2, to_rate)
    srcs = []
    for x, p, f in zip(xs, pos, fac):
        mx.add(O.Spatial(O.TestSource(x, in_ch, rate), p[0], p[1], p[2]).amplify(float(f)))
        srcs.append(whole(x, in_ch, rate, to_rate, gains=O.spatial_gains(p[0], p[1], p[2])[None, :], gain_period=1 << 40, factors=[f], factor_period=1 << 40))
    # ChannelVolume(src, gains) on its own, no Amplify
    mx.add(O.ChannelVolume(O.TestSource(xs[0], in_ch, rate), vols))
    srcs.append(whole(xs[0], in_ch, rate, to_rate, gains=vols[None, :], gain_period=1 << 40))
    want = mx.collect()
    M = max(s.frames for s in srcs)
    got = R.spatial_mix(2, to_rate, M, srcs)
    assert got.size == want.size
    assert np.array_equal(bits(got), bits(want))


def piecewise(O, x, in_ch, rate, channels, gains, gain_first, gain_period, factors, factor_first, factor_period):
    """Amplify(ChannelVolume(x)) with stepped tables, from the oracle's adapters with CONSTANT values: sample k of the output lies in gain step
    (gain_first + k) / gain_period - gain_first / gain_period (and likewise for the factor); every run of samples with one pair of entries
    is cut out of the oracle's output for the frames that hold it."""
    n = len(x) // in_ch
    total = n * channels
    k = np.arange(total, dtype=np.int64)
    ge = (gain_first + k) // gain_period - gain_first // gain_period
    fe = (factor_first + k) // factor_period - factor_first // factor_period if factors is not None else np.zeros(total, np.int64)
    cuts = [0] + [int(i) for i in np.flatnonzero((np.diff(ge) != 0) | (np.diff(fe) != 0)) + 1] + [total]
    parts = []
    for lo, hi in zip(cuts[:-1], cuts[1:]):
        f_lo, f_hi = lo // channels, (hi + channels - 1) // channels
        s = O.ChannelVolume(O.TestSource(x[f_lo * in_ch: f_hi * in_ch], in_ch, rate), gains[ge[lo]])
        if factors is not None:
            s = s.amplify(float(factors[fe[lo]]))
        parts.append(s.collect()[lo - f_lo * channels: hi - f_lo * channels])
    return np.concatenate(parts)


@pytest.mark.parametrize("gain_period,gain_first,factor_period,factor_first", [(3, 0, None, 0), (3, 2, 5, 1), (2, 1, 4, 0), (882, 871, 441, 5), (64, (1 << 33) + 17, 96, (1 << 40) + 3)])
@pytest.mark.parametrize("in_ch,rate,to_rate", [(1, 44100, 48000), (2, 96000, 44100), (6, 22050, 48000), (1, 48000, 48000)])
def test_stepped_tables_are_the_oracle_run_piecewise(O, in_ch, rate, to_rate, gain_period, gain_first, factor_period, factor_first):
    rng = np.random.default_rng(gain_period * 7 + in_ch)
    srcs, mx = [], O.Mixer(2, to_rate)
    for n in (500, 223):
        x = rng.uniform(-1, 1, n * in_ch).astype(np.float32)
        ng = R.entries_needed(gain_first, gain_period, 2 * n)
        gains = rng.uniform(-1, 1, (ng, 2)).astype(np.float32)  # every entry differs from its neighbours
        factors = None
        if factor_period:
            factors = rng.uniform(0.1, 2, R.entries_needed(factor_first, factor_period, 2 * n)).astype(np.float32)
        v = piecewise(O, x, in_ch, rate, 2, gains, gain_first, gain_period, factors, factor_first, factor_period or 1)
        assert v.size == 2 * n
        mx.add(O.TestSource(v, 2, rate))
        srcs.append(whole(x, in_ch, rate, to_rate, gains=gains, gain_period=gain_period, gain_first=gain_first, factors=factors, factor_period=factor_period or 1, factor_first=factor_first))
    want = mx.collect()
    got = R.spatial_mix(2, to_rate, max(s.frames for s in srcs), srcs)
    assert got.size == want.size
    assert np.array_equal(bits(got), bits(want))


def test_the_restatement_counts_what_a_block_touches():
    """touched_frames / entries_needed: what the entry's table check counts."""
    s = R.Src(np.zeros(64, np.float32), 1, 44100, 10, np.zeros((1, 2), np.float32), 1 << 40)
    assert R.touched_frames(s, 48000) == 9 * 147 // 160 + 2  # both taps of the last frame
    s.last = 8
    assert R.touched_frames(s, 48000) == 9  # frame 9's first tap is the last frame: verbatim, no second tap
    s2 = R.Src(np.zeros(64, np.float32), 1, 48000, 10, np.zeros((1, 2), np.float32), 1 << 40)
    assert R.touched_frames(s2, 48000) == 10
    assert R.entries_needed(5, 3, 1) == 1 and R.entries_needed(5, 3, 2) == 2 and R.entries_needed((1 << 33) + 2, 3, 4) == 2
