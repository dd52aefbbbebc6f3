"""The premises of tests/test_gpu_wide_positions.py, checked with the oracle alone (no GPU): the bank's arithmetic; the integer-position
restatement of the mixer (tests/wide_positions.py) against `O.Mixer` at every pair of the bank; tests/spatial_mix_ref.py and
tests/player_mix_ref.py against the oracle's mixer at the two large-F pairs, the way test_spatial_mix_cpu.py and test_player_mix_cpu.py
hold them at audio rates (their int64 positions do not depend on a small F); the restatement of rh_uniform_segments against
`O.UniformSourceIterator` for open and closed spans at positions the oracle can reach -- only then may the GPU tests use it beyond 2^31."""
import numpy as np
import pytest

import player_mix_ref as PR
import spatial_mix_ref as SR
import wide_positions as W
from test_player_mix_cpu import oracle_source
from test_spatial_mix_cpu import piecewise, whole

PAIRS = pytest.mark.parametrize("pair", W.BANK, ids=[p.id for p in W.BANK])
LARGE = pytest.mark.parametrize("pair", W.LARGE_F, ids=[p.id for p in W.LARGE_F])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


# ---- the bank -------------------------------------------------------------------------------------------------------------------------------
def test_the_bank_holds_the_pairs_of_the_issue():
    ids = [p.id for p in W.BANK]
    for want in ("65521-48000", "65521-65519", "48000-65521", "100-16777259", "44100-48000"):
        assert want in ids
    assert W.BY_ID["65521-48000"].fit == 65550 and W.BY_ID["65521-48000"].block == 70000
    assert W.BY_ID["65521-65519"].block == W.BY_ID["65521-65519"].fit + 4000
    assert 93000 < W.BY_ID["48000-65521"].block == W.BY_ID["48000-65521"].fit + 4000 < 94000
    assert W.BY_ID["100-16777259"].T > 1 << 24 and W.BY_ID["100-16777259"].block == 300000
    assert int(np.float32(W.BY_ID["100-16777259"].T)) != W.BY_ID["100-16777259"].T  # (float)T rounds


@PAIRS
def test_bank_arithmetic(pair):
    """F T < 2^32; the block is longer than fit exactly where the table says so; the last position a launch of fit frames can form,
    T - 1 + (fit - 1) F, fits 32 bits.  The host's fit = (2^32 - 1 - T) / F keeps T + fit F inside 32 bits, one position more than a
    launch forms, so frame `fit` itself would still fit (T - 1 + fit F <= 2^32 - 2 at every pair) and the first position that does not is
    T - 1 + (fit + 1) F: fit is safe, and short of the longest launch by exactly one frame.  Every other rate of the pair is one the mixer
    takes, and leaves the cut to the pair."""
    F, T, fit = pair.F, pair.T, pair.fit
    assert F * T < W.U32
    assert (pair.block > fit) == pair.cuts
    assert T - 1 + (fit - 1) * F < W.U32
    assert T - 1 + fit * F <= W.U32 - 2 and T - 1 + (fit + 1) * F >= W.U32
    assert fit == W.fit_of(pair.from_rate, pair.to_rate)
    assert (pair.block * F // T + 8) * 6 * 4 < 3 << 20  # the largest source row of a test: six channels, under 3 MB
    for rate in pair.others:
        f, t = W.reduced(rate, pair.to_rate)
        assert f * t < W.U32 and W.fit_of(rate, pair.to_rate) > pair.block, rate
    assert len({W.reduced(r, pair.to_rate) for r in (pair.from_rate,) + pair.others}) == 5  # five different rates: a fifth one starts a launch


def test_a_fit_without_t_differs_in_what_fits_only_where_t_is_large():
    """(2^32 - 1) / F against (2^32 - 1 - T) / F: the looser number is one to three frames more at every pair with a cut, but with T < 2 F a
    launch of that many frames still fits for every phase (only the refusals of fit + 1 frames tell the two apart); 40 000 -> 100 003 alone
    has a phase (above 47 296) from which it wraps, and the blocks of the tests start above it."""
    bites = []
    for p in W.CUT_PAIRS:
        loose = (W.U32 - 1) // p.F
        assert p.fit < loose <= p.fit + 3
        if p.T - 1 + (loose - 1) * p.F >= W.U32:
            bites.append(p.id)
            assert W.U32 - (loose - 1) * p.F <= p.phase_min  # ... and the blocks of the tests start above it
    assert bites == ["40000-100003"]


@PAIRS
def test_the_cases_are_what_they_claim(pair):
    """mixed_case / alike_case: a nonzero phase, one source ending ON the cut frame, one in front, one behind, the rest live."""
    c = W.mixed_case(pair, 2)
    m0, M, cut = c["m0"], c["M"], c["cut"]
    assert M == pair.block and (cut == pair.fit) == pair.cuts and 0 < cut < M
    assert m0 * pair.F % pair.T >= pair.phase_min > 0
    fr = c["frames"]
    assert fr[0] == cut + 1 and 0 < fr[2] <= cut - 777 and cut + 1500 <= fr[3] <= M and all(f == M for f in fr[4:])
    if pair.T < 1 << 24:
        assert fr[1] == cut and fr[3] < M
    else:
        assert 0 < fr[1] < cut  # (a source frame is 114 131 mix frames: no stream of the second rate ends with frame cut - 1)
    x, ch, rate, _ = c["srcs"][0]
    p = W.plan(len(x) // ch, rate, pair.to_rate, m0, M)
    assert p["frames"] == cut + 1 and p["last"] != W.LIVE and p["phase"] == m0 * pair.F % pair.T
    x, ch, rate, _ = c["srcs"][4]
    p = W.plan(len(x) // ch, rate, pair.to_rate, m0, M)
    assert p["frames"] == M and p["last"] == W.LIVE and p["hi"] <= len(x) // ch - 3
    a = W.alike_case(pair)
    assert 1024 <= cut < a["end"] == cut + 1501 < M


# ---- the mixer --------------------------------------------------------------------------------------------------------------------------------
@PAIRS
@pytest.mark.parametrize("to_ch", [1, 2, 6])
def test_the_mixer_restatement_is_the_oracles_mixer(O, pair, to_ch):
    """Sources of 1, 2 and 6 channels at the pair's rate and its second one, gains other than 1, sources that end inside the block, one
    that ended in front of it: the whole mix from frame 0, and the block [m0, m0 + M) out of it."""
    c = W.mixed_case(pair, to_ch, seed=to_ch)
    m0, M = c["m0"], c["M"]
    srcs = c["srcs"] + [(W.signal(np.random.default_rng(9), 40 * 2), 2, pair.from_rate, -0.5)]
    assert {s[1] for s in srcs} >= {1, 2, 6} and all(s[3] != 1.0 for s in srcs)
    mx = O.Mixer(to_ch, pair.to_rate)
    for x, ch, rate, gain in srcs:
        mx.add(O.TestSource(x, ch, rate).amplify(gain))
    want = mx.collect()
    total = max(W.out_frames(len(x) // ch, *W.reduced(rate, pair.to_rate)) for x, ch, rate, _ in srcs)
    assert want.size == total * to_ch and total > m0 + M
    got = W.mix(srcs, to_ch, pair.to_rate, 0, total)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, (int(bad[0]), got[bad[0]], want[bad[0]])
    assert np.array_equal(bits(W.mix(srcs, to_ch, pair.to_rate, m0, M)), bits(want[m0 * to_ch: (m0 + M) * to_ch]))


# ---- the spatial and the player restatement at large F ----------------------------------------------------------------------------------------
@LARGE
@pytest.mark.parametrize("in_ch", [1, 6])
def test_spatial_ref_with_constant_tables_at_large_f(O, pair, in_ch):
    rate, to_rate = pair.from_rate, pair.to_rate
    rng = np.random.default_rng(in_ch)
    xs = [rng.uniform(-1, 1, n * in_ch).astype(np.float32) for n in (3001, 1570, 1, 2)]
    mx, srcs = O.Mixer(2, to_rate), []
    for x, f in zip(xs, (0.7, 1.0, -1.3, 0.25)):
        p = rng.uniform(-2, 2, (3, 3)).astype(np.float32)
        mx.add(O.Spatial(O.TestSource(x, in_ch, rate), p[0], p[1], p[2]).amplify(f))
        srcs.append(whole(x, in_ch, rate, to_rate, gains=O.spatial_gains(p[0], p[1], p[2])[None, :], gain_period=1 << 40, factors=[np.float32(f)], factor_period=1 << 40))
    want = mx.collect()
    got = SR.spatial_mix(2, to_rate, max(s.frames for s in srcs), srcs)
    assert got.size == want.size and np.array_equal(bits(got), bits(want))


@LARGE
@pytest.mark.parametrize("gain_period,gain_first,factor_period,factor_first", [(3, 2, 5, 1), (882, 871, 441, 5), (64, (1 << 35) + 17, 96, (1 << 40) + 3)])
def test_spatial_ref_with_stepped_tables_at_large_f(O, pair, gain_period, gain_first, factor_period, factor_first):
    rate, to_rate = pair.from_rate, pair.to_rate
    rng = np.random.default_rng(gain_period)
    srcs, mx = [], O.Mixer(2, to_rate)
    for n, in_ch in ((900, 1), (423, 6)):
        x = rng.uniform(-1, 1, n * in_ch).astype(np.float32)
        gains = rng.uniform(-1, 1, (SR.entries_needed(gain_first, gain_period, 2 * n), 2)).astype(np.float32)
        factors = rng.uniform(0.1, 2, SR.entries_needed(factor_first, factor_period, 2 * n)).astype(np.float32)
        v = piecewise(O, x, in_ch, rate, 2, gains, gain_first, gain_period, factors, factor_first, factor_period)
        mx.add(O.TestSource(v, 2, rate))
        srcs.append(whole(x, in_ch, rate, to_rate, gains=gains, gain_period=gain_period, gain_first=gain_first, factors=factors, factor_period=factor_period, factor_first=factor_first))
    want = mx.collect()
    got = SR.spatial_mix(2, to_rate, max(s.frames for s in srcs), srcs)
    assert got.size == want.size and np.array_equal(bits(got), bits(want))


@LARGE
@pytest.mark.parametrize("ch,to_ch", [(1, 2), (2, 2), (2, 1), (6, 2), (2, 6)])
def test_player_ref_at_large_f(O, pair, ch, to_ch):
    rate, to_rate = pair.from_rate, pair.to_rate
    rng = np.random.default_rng(10 * ch + to_ch)
    MS = 1_000_000
    for ns in (5 * MS, 1000 * MS):
        for kind, start, end in ((PR.RAMP, 0.0, 1.0), (PR.CLAMP, 1.4, 0.6)):
            mx, srcs = O.Mixer(to_ch, to_rate), []
            for n, g, f, period, first in ((1700, 0.7, 1.3, 7, 5), (633, -1.1, 0.25, 882, (1 << 35) + 871), (1, 1.0, None, 1, 0), (2, 0.5, 2.0, 1, 3)):
                x = rng.uniform(-1, 1, n * ch).astype(np.float32)
                mx.add(oracle_source(O, x, ch, rate, g, kind, ns, start, end, f))
                table = None if f is None else np.full(PR.entries_needed(first, period, n * ch), f, np.float32)
                srcs.append(PR.block_of(x, ch, rate, to_rate, 0, PR.stream_out_frames(n, pair.F, pair.T), gain=g, kind=kind, ramp_ns=ns, start=start, end=end,
                                        factors=table, factor_period=period, factor_first=first))
            want = mx.collect()
            got = PR.player_mix(to_ch, to_rate, max(s.frames for s in srcs), srcs)
            assert got.size == want.size, (ns, kind)
            assert np.array_equal(bits(got), bits(want)), (ns, kind)


@LARGE
def test_player_ref_blocks_in_mid_stream_are_the_one_pass_at_large_f(pair):
    """block_of: phase, first_frame and the factor table's first carried to a block that starts at a large phase."""
    rng = np.random.default_rng(3)
    to_rate, to_ch = pair.to_rate, 2
    x = rng.uniform(-1, 1, 2 * 4000).astype(np.float32)
    a = dict(gain=0.8, kind=PR.RAMP, ramp_ns=30_000_000, start=0.2, end=1.1, factors=rng.uniform(0.2, 1.5, PR.entries_needed(5, 441, 8000)).astype(np.float32), factor_period=441, factor_first=5)
    total = PR.stream_out_frames(4000, pair.F, pair.T)
    one = PR.player_mix(to_ch, to_rate, total, [PR.block_of(x, 2, pair.from_rate, to_rate, 0, total, **a)])
    m = W.largest_phase(pair, 1000, 1000)
    parts = [PR.player_mix(to_ch, to_rate, hi - lo, [PR.block_of(x, 2, pair.from_rate, to_rate, lo, hi, **a)]) for lo, hi in ((0, m), (m, total))]
    assert np.array_equal(bits(np.concatenate(parts)), bits(one))


# ---- rh_uniform_segments ------------------------------------------------------------------------------------------------------------------------
UNIFORM = [(2, 44100, 2, 48000), (1, 65521, 2, 48000), (6, 65521, 2, 65519), (2, 48000, 6, 65521), (1, 100, 1, 16777259), (2, 48000, 2, 48000), (1, 44100, 1, 48000)]


@pytest.mark.parametrize("ch,rate,to_ch,to_rate", UNIFORM)
def test_the_uniform_restatement_is_the_oracles_iterator(O, ch, rate, to_ch, to_rate):
    """A closed span (a SamplesBuffer: one span, its last frame verbatim), spans of 700 samples each closed on its own, and an open one
    (a continuous source: every frame in front of the stream's end) -- with a gain in front, in pieces that start in mid-span."""
    F, T = W.reduced(rate, to_rate)
    n = 7 if T > 1 << 20 else 2300
    x = W.signal(np.random.default_rng(rate % 97 + ch), n * ch)
    g = 0.37
    # closed: the whole span, in two pieces
    want = O.UniformSourceIterator(O.SamplesBuffer(ch, rate, x).amplify(g), to_ch, to_rate).collect()
    total = W.out_frames(n, F, T)
    assert want.size == total * to_ch
    cut = total // 3
    i0 = cut * F // T
    got = np.concatenate([W.uniform_segment(x, 0, ch, rate, to_ch, to_rate, 0, cut, n, g), W.uniform_segment(x[i0 * ch:], i0, ch, rate, to_ch, to_rate, cut, total, n, g)])
    assert np.array_equal(bits(got), bits(want))
    # open: what a continuous source gives in front of its end
    ready = W.lerp_ready(n, F, T) if F != T else n
    want = O.UniformSourceIterator(O.TestSource(x, ch, rate).amplify(g), to_ch, to_rate).collect()
    got = W.uniform_segment(x, 0, ch, rate, to_ch, to_rate, 0, ready, W.U64_MAX, g)
    assert np.array_equal(bits(got), bits(want[: ready * to_ch]))
    # spans of 100 frames, each a converter of its own
    span = 100
    if n > span:
        want = O.UniformSourceIterator(O.SpanSource(x, ch, rate, span * ch), to_ch, to_rate).collect()
        parts = []
        for f0 in range(0, n, span):
            k = min(span, n - f0)
            parts.append(W.uniform_segment(x[f0 * ch: (f0 + k) * ch], 0, ch, rate, to_ch, to_rate, 0, W.out_frames(k, F, T), k))
        assert np.array_equal(bits(np.concatenate(parts)), bits(want))


def test_the_positions_of_the_gpu_cases_leave_32_and_64_bits():
    """What the GPU cases beyond 2^31 claim of their positions, and that a 64-bit product is another number there."""
    m = (1 << 50) + 1
    assert m * 65521 >= 1 << 64 and ((m * 65521) % (1 << 64)) // 48000 != (m * 65521) // 48000
    assert ((1 << 40) + 3) * 147 < 1 << 64 and ((1 << 31) + 700) * 147 < 1 << 64
