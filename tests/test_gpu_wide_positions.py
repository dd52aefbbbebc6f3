"""The one-launch block mixers where tap positions reach 32 bits and blocks are cut into launches, and rh_uniform_segments where positions
leave 32 and 64 bits.  rh_wide_mix_block, rh_wide_mix_block_filtered, rh_wide_mix_batch, rh_spatial_mix_block and rh_player_mix_block all
form `p = r0 + j F` in a u32 and keep it there with `fit = (2^32 - 1 - T) / F`; the first and the fourth cut a longer block into launches
and re-base i0, r0, `last` and the step tables for every later one, the others refuse it.  At audio rates none of that is ever computed.
The rate pairs of tests/wide_positions.py reach it with blocks of a few hundred KiB (their premises: tests/test_wide_positions_cpu.py).

Every comparison is on 32-bit patterns, no tolerance.  The reference is the oracle's mixer (`O.Mixer` fed `TestSource(..).amplify(g)`, run
from frame 0 of the mix: the block is a slice of it) for the three wide entries, tests/spatial_mix_ref.py and tests/player_mix_ref.py for
the spatial and the player entry (their chains of existing entries go through rh_wide_mix_block, which is itself under test here), the
oracle's UniformSourceIterator and the Python-int restatement of tests/wide_positions.py for rh_uniform_segments.  Destinations lie
between sentinel guards, and a source holds exactly the frames its header lets the block read, between NaN (tests/arena.py): a position
that is wrong by one reads a neighbouring frame, and the frame behind the last one is NaN.

Every case that claims a cut, a 128-bit position or the 2048-frame tile asserts that premise itself.  Out of scope: (e) at T > 2^24 and
in the control, whose fit of 4 10^7 frames is no block a test can hold; the step rule's own bound of rh_spatial_mix_block (`fit_steps`:
2^30 emitter samples a launch), which needs gigabytes of source."""
import ctypes as C

import numpy as np
import pytest

import arena
import player_mix_ref as PR
import spatial_mix_ref as SR
import test_gpu_player_mix as PL
import test_gpu_spatial_mix as SP
import wide_positions as W

pytestmark = pytest.mark.gpu
f32 = np.float32
UNSUPPORTED = 3
MS = 1_000_000
PAIRS = pytest.mark.parametrize("pair", W.BANK, ids=[p.id for p in W.BANK])
CUTS = pytest.mark.parametrize("pair", W.CUT_PAIRS, ids=[p.id for p in W.CUT_PAIRS])
SCENES = pytest.mark.parametrize("pair", W.LARGE_F + [W.CONTROL], ids=[p.id for p in W.LARGE_F + [W.CONTROL]])


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same_bits(got, want, ch, what):
    got, want = np.asarray(got, f32).reshape(-1), np.asarray(want, f32).reshape(-1)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.flatnonzero(bits(got) != bits(want))
    assert bad.size == 0, f"{what}: {bad.size} sample(s) differ from the reference, the first at {int(bad[0])} (frame {int(bad[0]) // ch}): {got[bad[0]]!r} != {want[bad[0]]!r}"


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _st():
    from rodio_amd import source

    return source._stream()


# ---- the reference: the oracle's mixer over the whole streams, computed once per case --------------------------------------------------------
_ORACLE = {}


def oracle_mix(key, srcs, to_ch, to_rate, filters=None):
    """mixer::mixer(to_ch, to_rate) fed TestSource(x, ch, rate).amplify(gain) -- behind UniformSourceIterator and a low_pass / high_pass
    where filters[k] = (name, freq, q) -- from frame 0 to the end of the longest stream.  Shared by the tests of a case, never written to."""
    if key not in _ORACLE:
        from oracle import rodio_oracle as O

        mx = O.Mixer(to_ch, to_rate)
        for k, (x, ch, rate, gain) in enumerate(srcs):
            s = O.TestSource(x, ch, rate).amplify(gain)
            if filters and filters[k]:
                u = O.UniformSourceIterator(s, to_ch, to_rate)
                s = u.low_pass(filters[k][1], filters[k][2]) if filters[k][0] == "lp" else u.high_pass(filters[k][1], filters[k][2])
            mx.add(s)
        want = mx.collect()
        want.setflags(write=False)
        _ORACLE[key] = want
    return _ORACLE[key]


def block_of(want, to_ch, m0, M):
    assert want.size >= (m0 + M) * to_ch, "the oracle's mix ends inside the block"
    return want[m0 * to_ch: (m0 + M) * to_ch]


class Block:
    """The table of a block [m0, m0 + M) over resident streams srcs = [(x, ch, rate, gain)]: every source on the device from the frame of
    its first tap to the last frame the header lets the block read, between NaN, at 4-byte offsets 0 .. 3 behind a 16-byte boundary."""

    def __init__(self, srcs, to_rate, m0, M):
        from rodio_amd import _lib

        self.n, self.keep, self.plans = len(srcs), [], []
        self.arr = (_lib.WideSrc * max(self.n, 1))()
        for k, (x, ch, rate, gain) in enumerate(srcs):
            p = W.plan(len(x) // ch, rate, to_rate, m0, M)
            a = None
            if p["frames"]:
                a = arena.src_arena(x[p["lo"] * ch: p["hi"] * ch], lead=k % 4)
                self.keep.append(a)
            W.fill(self.arr[k], p, a.ptr() if a is not None else None, ch, rate, gain)
            self.plans.append(p)

    def unchanged(self):
        for a in self.keep:
            a.unchanged()


def wide_block(blk, to_ch, to_rate, M, lead=1):
    """rh_wide_mix_block into a guarded dst `lead` floats behind a 16-byte boundary: nothing stored outside, every word written."""
    from rodio_amd import _lib

    dst = arena.dst_arena(M * to_ch, lead)
    _lib.check(_lib.lib.rh_wide_mix_block(C.c_void_p(dst.ptr()), to_ch, to_rate, M, blk.arr, blk.n, _st()), "rh_wide_mix_block")
    return dst.check()


def cut_premise(pair, M, blk=None):
    """A case that claims the cut has it: the block is longer than fit exactly where the bank says so, and fit is the least over the table."""
    assert (M > pair.fit) == pair.cuts, "the case no longer crosses the cut it is about"
    if blk is not None:
        fits = [W.fit_of(blk.arr[k].from_rate, pair.to_rate) for k in range(blk.n) if blk.arr[k].frames]
        assert (min(fits) == pair.fit < M) if pair.cuts else (min(fits) >= M)


# ---- rh_wide_mix_block ------------------------------------------------------------------------------------------------------------------------
@PAIRS
@pytest.mark.parametrize("to_ch", [1, 2, 6])
def test_mixed_sources_across_the_cut(G, pair, to_ch):
    """(a) Eight sources of layouts 1, 2, 6 and the mixer's own, half at the pair's rate and half at its second one (44 100 where the mixer
    takes it: cut at a frame that is nothing special for them), from a frame m0 with a large phase.  One source ends in front of the cut,
    one with the frame in front of it (the second launch skips it), one ON the cut frame (the second launch reaches one frame of it: its
    last one, `last` re-based by i0) and one behind it."""
    c = W.mixed_case(pair, to_ch, seed=to_ch)
    m0, M, cut = c["m0"], c["M"], c["cut"]
    blk = Block(c["srcs"], pair.to_rate, m0, M)
    cut_premise(pair, M, blk)
    fr = [p["frames"] for p in blk.plans]
    assert fr[0] == cut + 1 and fr[1] <= cut and fr[2] < cut < fr[3] and fr[4:] == [M] * 4 and blk.plans[0]["phase"] >= pair.phase_min > 0
    tap = (blk.plans[0]["phase"] + cut * pair.F) // pair.T  # the cut frame's first tap: the stream's last frame (verbatim), or the one in front of it
    assert blk.plans[0]["last"] - tap in (0, 1) and blk.plans[0]["last"] > 0
    want = block_of(oracle_mix(("mixed", pair.id, to_ch), c["srcs"], to_ch, pair.to_rate), to_ch, m0, M)
    same_bits(wide_block(blk, to_ch, pair.to_rate, M), want, to_ch, "rh_wide_mix_block")
    blk.unchanged()


@PAIRS
def test_forty_sources_across_the_cut(G, pair):
    """(b) Forty such sources into a stereo mix: every launch behind the first continues from the stored partial sum, on both sides of the cut."""
    c = W.mixed_case(pair, 2, n_sources=40, seed=40)
    blk = Block(c["srcs"], pair.to_rate, c["m0"], c["M"])
    cut_premise(pair, c["M"], blk)
    assert blk.n == 40 > 32
    want = block_of(oracle_mix(("forty", pair.id), c["srcs"], 2, pair.to_rate), 2, c["m0"], c["M"])
    same_bits(wide_block(blk, 2, pair.to_rate, c["M"]), want, 2, "rh_wide_mix_block")
    blk.unchanged()


@PAIRS
def test_five_rates_across_the_cut(G, pair):
    """(c) Ten sources of five (rate, phase) pairs in one block with the cut: the fifth starts a launch of its own, and every later launch
    of the block re-bases all five."""
    c = W.mixed_case(pair, 2, n_sources=10, rates=(pair.from_rate,) + pair.others, seed=5)
    blk = Block(c["srcs"], pair.to_rate, c["m0"], c["M"])
    cut_premise(pair, c["M"], blk)
    assert len({(blk.arr[k].from_rate, blk.arr[k].phase) for k in range(blk.n)}) == 5
    want = block_of(oracle_mix(("five", pair.id), c["srcs"], 2, pair.to_rate), 2, c["m0"], c["M"])
    same_bits(wide_block(blk, 2, pair.to_rate, c["M"]), want, 2, "rh_wide_mix_block")
    blk.unchanged()


@PAIRS
def test_alike_sources_with_one_ending_behind_the_cut(G, pair):
    """(d) Sources of the mixer's layout, one rate and phase, the last one ending 1500 frames behind the cut: the frames in front of its end
    are the uniform kernel's (`j_uni`), cut once more at `fit` -- a uniform launch with j0 > 0 --, the rest the general kernel's.  Once as
    it is and once with RH_WIDE_GENERAL=1: the oracle's bits both times."""
    from conftest import knobs

    c = W.alike_case(pair)
    m0, M = c["m0"], c["M"]
    blk = Block(c["srcs"], pair.to_rate, m0, M)
    cut_premise(pair, M, blk)
    assert 1024 <= c["cut"] < c["end"] < M and blk.plans[-1]["frames"] == c["end"] and all(p["frames"] == M for p in blk.plans[:-1])
    assert len({(blk.arr[k].from_rate, blk.arr[k].phase, blk.arr[k].channels) for k in range(blk.n)}) == 1
    want = block_of(oracle_mix(("alike", pair.id), c["srcs"], 2, pair.to_rate), 2, m0, M)
    uniform = wide_block(blk, 2, pair.to_rate, M)
    with knobs(RH_WIDE_GENERAL="1"):
        general = wide_block(blk, 2, pair.to_rate, M)
    same_bits(uniform, want, 2, "the uniform kernel")
    same_bits(general, want, 2, "RH_WIDE_GENERAL=1")
    blk.unchanged()


@CUTS
def test_blocks_of_fit_minus_one_fit_and_fit_plus_one_frames(G, pair):
    """(e) One launch of fit - 1 and of fit frames, and fit + 1 frames: a launch of fit and one of a single frame.  The block starts where
    the pair's phase is the largest of 40 000 frames, so the last position of the full launch is the largest the entry ever forms."""
    rng = np.random.default_rng(11)
    m0 = W.largest_phase(pair)
    assert m0 * pair.F % pair.T >= pair.T - pair.T // 100
    srcs = []
    for ch, rate, gain in ((1, pair.from_rate, 0.5), (2, pair.from_rate, -1.5), (2, pair.others[0], 0.75)):
        F, T = W.reduced(rate, pair.to_rate)
        srcs.append((W.signal(rng, W.live_frames(F, T, m0 + pair.fit + 1) * ch), ch, rate, gain))
    want = oracle_mix(("edge", pair.id), srcs, 2, pair.to_rate)
    for M in (pair.fit - 1, pair.fit, pair.fit + 1):
        blk = Block(srcs, pair.to_rate, m0, M)
        assert all(p["frames"] == M and p["last"] == W.LIVE for p in blk.plans)
        assert min(W.fit_of(s[2], pair.to_rate) for s in srcs) == pair.fit and (M > pair.fit) == (M == pair.fit + 1)
        same_bits(wide_block(blk, 2, pair.to_rate, M), block_of(want, 2, m0, M), 2, f"{M} frames")
        blk.unchanged()


# ---- rh_wide_mix_block_filtered, mode 0 -------------------------------------------------------------------------------------------------------
def filtered(blk, to_ch, to_rate, M, kinds, states, scratch=None, dst=None):
    """The raw entry in mode 0 with a low_pass(1000, 0.5) / high_pass(2000, 0.5) where kinds[k] is 0 / 1: (status, dst arena, scratch arena)."""
    from rodio_amd import _lib

    co = np.zeros((blk.n, 5), f32)
    for k, kind in enumerate(kinds):
        if kind >= 0:
            assert _lib.lib.rh_biquad_coeffs(kind, 2000 if kind else 1000, 0.5, to_rate, co[k].ctypes.data_as(_lib.f32p)) == 0
    need = C.c_uint64(0)
    assert _lib.lib.rh_wide_mix_filtered_scratch_bytes(to_ch, M, sum(k >= 0 for k in kinds), C.byref(need)) == 0
    scratch = scratch or arena.dst_arena(need.value // 4, 0)
    dst = dst or arena.dst_arena(M * to_ch, 1)
    assert scratch.ptr() % 16 == 0
    st = (C.c_void_p * blk.n)(*[s.ptr() if s is not None else None for s in states])
    status = _lib.lib.rh_wide_mix_block_filtered(C.c_void_p(dst.ptr()), to_ch, to_rate, M, blk.arr, blk.n, (C.c_int32 * blk.n)(*kinds), co.ctypes.data_as(_lib.f32p), st, 0,
                                                 C.c_void_p(scratch.ptr()), need.value, _st())
    return status, dst, scratch


def filtered_case(pair, M, filtered_end=None):
    """A low-passed stereo source at the pair's rate and a high-passed mono one at the second rate (live, or ending about block frame
    filtered_end and just inside fit), and an unfiltered one at the pair's rate that spans the block; the block starts at the frame of the pair's largest phase."""
    rng = np.random.default_rng(21)
    m0 = W.largest_phase(pair)
    F2, T2 = W.reduced(pair.others[0], pair.to_rate)
    n0, n1 = W.live_frames(pair.F, pair.T, m0 + M), W.live_frames(F2, T2, m0 + M)
    if filtered_end is not None:  # the first ends there, the second with the last frame its rate can end with inside fit
        n0 = W.frames_for_total(pair.F, pair.T, m0 + filtered_end)
        n1 = W.frames_for_total(F2, T2, m0 + pair.fit)
        n1 -= 1 if W.out_frames(n1, F2, T2) > m0 + pair.fit else 0
    srcs = [(W.signal(rng, n0 * 2), 2, pair.from_rate, 0.75), (W.signal(rng, n1), 1, pair.others[0], -0.5),
            (W.signal(rng, W.live_frames(pair.F, pair.T, m0 + M) * 6), 6, pair.from_rate, 1.25)]
    return m0, srcs, [0, 1, -1], [("lp", 1000, 0.5), ("hp", 2000, 0.5), None]


def two_blocks(pair, m0, M, srcs, kinds, what):
    """Blocks [0, m0) and [m0, m0 + M) with the filter states carried on the device: (bits of both, the second block's table)."""
    states = [arena.state_arena(4 * 2) if k >= 0 else None for k in kinds]
    parts = []
    for lo, n in ((0, m0), (m0, M)):
        blk = Block(srcs, pair.to_rate, lo, n)
        status, dst, scratch = filtered(blk, 2, pair.to_rate, n, kinds, states)
        assert status == 0, (what, lo, status)
        parts.append(dst.check())
        scratch.check_guards()
        blk.unchanged()
    for s in states:
        if s is not None:
            s.check()  # (guards intact, every word of the state written)
    return np.concatenate(parts), blk


@CUTS
def test_a_filtered_source_of_exactly_fit_frames(G, pair):
    """k_wide_rows at its last legal position: filtered sources that reach exactly fit frames of a block that starts at a large phase, the
    filter states carried over from the block in front of it.  The oracle's bits."""
    M = pair.fit
    m0, srcs, kinds, filters = filtered_case(pair, M)
    got, blk = two_blocks(pair, m0, M, srcs, kinds, "fit")
    assert blk.arr[0].frames == blk.arr[1].frames == pair.fit and blk.arr[0].phase >= pair.T - pair.T // 50
    want = oracle_mix(("filtered", pair.id), srcs, 2, pair.to_rate, filters)
    same_bits(got, want[: (m0 + M) * 2], 2, "rh_wide_mix_block_filtered at fit frames")


@CUTS
def test_a_filtered_source_of_fit_plus_one_frames_is_refused(G, pair):
    """RH_ERR_UNSUPPORTED, and neither a sample nor a carried state nor the scratch is touched (a scratch large enough for the block)."""
    M = pair.fit + 1
    m0, srcs, kinds, _ = filtered_case(pair, M)
    blk = Block(srcs, pair.to_rate, m0, M)
    assert blk.arr[0].frames == pair.fit + 1 > W.fit_of(pair.from_rate, pair.to_rate)
    states = [arena.state_arena(8, np.random.default_rng(2).uniform(-1, 1, 8).astype(f32)) if k >= 0 else None for k in kinds]
    status, dst, scratch = filtered(blk, 2, pair.to_rate, M, kinds, states)
    assert status == UNSUPPORTED
    dst.check(written=0)
    scratch.check(written=0)
    for s in states:
        if s is not None:
            s.unchanged()
    blk.unchanged()


@CUTS
def test_a_block_longer_than_fit_with_its_filtered_sources_inside_fit(G, pair):
    """An unfiltered source of the pair's rate spans a block longer than fit (the mix behind the filters is cut), a filtered one ends 3000
    frames in front of fit and another with the last frame inside fit its rate can end with: accepted, and the oracle's bits."""
    M = pair.block
    m0, srcs, kinds, filters = filtered_case(pair, M, filtered_end=pair.fit - 3000)
    got, blk = two_blocks(pair, m0, M, srcs, kinds, "longer than fit")
    cut_premise(pair, M, blk)
    assert pair.fit - 3000 <= blk.arr[0].frames <= pair.fit - 2990 and pair.fit - 4 <= blk.arr[1].frames <= pair.fit < blk.arr[2].frames == M
    want = oracle_mix(("filtered-long", pair.id), srcs, 2, pair.to_rate, filters)
    same_bits(got, want[: (m0 + M) * 2], 2, "rh_wide_mix_block_filtered beyond fit")


# ---- rh_wide_mix_batch --------------------------------------------------------------------------------------------------------------------------
def test_two_batched_mixers_of_exactly_fit_frames_equal_the_oracle(G):
    """A mono mixer at 48 000 and a stereo one at 65 519, each with sources at 65 521 and 44 100 (some ending inside the block) and a block
    of exactly its fit = 65 550 frames from a frame with a large phase: the longest block the batch takes, against the oracle's mixer."""
    mixers = []
    for pair, to_ch in zip(W.LARGE_F, (1, 2)):
        c = W.mixed_case(pair, to_ch, n_sources=6, M=pair.fit, seed=60 + to_ch)
        blk = Block(c["srcs"], pair.to_rate, c["m0"], pair.fit)
        assert c["M"] == pair.fit == min(W.fit_of(blk.arr[k].from_rate, pair.to_rate) for k in range(blk.n)) and blk.plans[0]["phase"] >= pair.phase_min
        mixers.append((pair, to_ch, c, blk, arena.dst_arena(pair.fit * to_ch, 1)))
    G.wide_mix_batch([m[4].ptr() for m in mixers], [m[1] for m in mixers], [m[0].to_rate for m in mixers], [m[0].fit for m in mixers], [[m[3].arr[k] for k in range(m[3].n)] for m in mixers])
    for pair, to_ch, c, blk, dst in mixers:
        want = block_of(oracle_mix(("batch", pair.id), c["srcs"], to_ch, pair.to_rate), to_ch, c["m0"], pair.fit)
        same_bits(dst.check(), want, to_ch, f"rh_wide_mix_batch, the mixer at {pair.to_rate}")
        blk.unchanged()


# ---- rh_spatial_mix_block -----------------------------------------------------------------------------------------------------------------------
def entry(first, period, k):
    """The table entry of sample k, counted from data (periodic.rs:63-77)."""
    return (first + k) // period - first // period


def spatial_scene(pair, ch, in_chs, seed):
    """Seven emitters of a block longer than fit whose step tables make the cut matter.  With K0 the first sample of the emitter's output the
    second launch reads: a gain boundary at K0 - 1, one at K0 (gain_first above 2^35, the factors in step with the gains) and one at K0 + 1
    (factors on a period of 5); a gain period above 2^31 whose only boundary lies 5001 samples inside the second launch (factors on 441,
    their first above 2^35); gains on a period of 7 under a factor period above 2^31 of the same kind; an emitter that ends 700 source
    frames behind the cut; one without any change."""
    rng = np.random.default_rng(seed)
    rate, to_rate, M, cut = pair.from_rate, pair.to_rate, pair.block, pair.cut
    m0 = W.largest_phase(pair)
    i_cut = (m0 * pair.F % pair.T + cut * pair.F) // pair.T
    K0 = i_cut * ch
    GP, BIG = 50021, (1 << 31) + 11
    at = lambda k, period: (-k) % period                                   # noqa: E731  a first that puts a boundary on sample k
    far = lambda first, period: first + period * ((1 << 35) // period + 1)  # noqa: E731  ... the same boundaries, from beyond 2^35
    specs = [dict(gp=GP, gf=at(K0 - 1, GP)), dict(gp=GP, gf=far(at(K0, GP), GP), fp=GP, ff=far(at(K0, GP), GP)), dict(gp=GP, gf=at(K0 + 1, GP), fp=5, ff=7),
             dict(gp=BIG, gf=at(K0 + 5001, BIG), fp=441, ff=(1 << 35) + 6), dict(gp=7, gf=2, fp=BIG, ff=at(K0 + 5001, BIG)), dict(gp=882, gf=871, fp=441, ff=5, n=i_cut + 700),
             dict(gp=1 << 40, gf=0)]
    srcs = [SP.make(rng, in_chs[k % len(in_chs)], rate, to_rate, M, m0, s.get("n"), ch, gp=s["gp"], gf=s["gf"], fp=s.get("fp"), ff=s.get("ff", 0)) for k, s in enumerate(specs)]
    # the premises, in the restatement's own terms
    assert srcs[0].phase == m0 * pair.F % pair.T >= pair.T - pair.T // 100 and K0 > 2
    for k, d in ((0, -1), (1, 0), (2, 1)):
        s = srcs[k]
        assert entry(s.gain_first, s.gain_period, K0 + d) == entry(s.gain_first, s.gain_period, K0 + d - 1) + 1, "a gain boundary beside the second launch's first sample"
    assert srcs[1].gain_first > 1 << 35 and srcs[3].factor_first > 1 << 35
    for s, first, period, table in ((srcs[3], srcs[3].gain_first, srcs[3].gain_period, srcs[3].gains), (srcs[4], srcs[4].factor_first, srcs[4].factor_period, srcs[4].factors)):
        e = [entry(first, period, k) for k in (0, K0, K0 + 5000, K0 + 5001, SR.touched_frames(s, to_rate) * ch - 1)]
        assert period > 1 << 31 and e == [0, 0, 0, 1, 1] and len(table) == 2, "one boundary, inside the second launch"
    assert cut < srcs[5].frames < M and srcs[5].last != SP.LIVE and all(s.frames == M for k, s in enumerate(srcs) if k != 5)
    return srcs, M


@SCENES
@pytest.mark.parametrize("ch,in_chs", [(2, (1,)), (2, (1, 6)), (5, (6, 1))], ids=["mono-into-stereo", "mono-and-5.1-into-stereo", "into-five-channels"])
def test_spatial_blocks_longer_than_fit(rh, pair, ch, in_chs):
    """Blocks longer than fit against tests/spatial_mix_ref.py, dst on and off an 8-byte boundary: mono emitters into a stereo mix take the
    fast kernel on it -- in front of the ending emitter's last frame, in launches cut at fit -- and the general one off it; mono and
    six-channel emitters into stereo and five channels take the general one.  In the control nothing is cut: the same tables, one launch."""
    srcs, M = spatial_scene(pair, ch, in_chs, 7 * ch + len(in_chs))
    assert (M > pair.fit) == pair.cuts and (pair.cuts or pair is W.CONTROL)
    SP.hold(rh, srcs, pair.to_rate, M, ch, leads=(0, 1), chain=False)


# ---- rh_player_mix_block ------------------------------------------------------------------------------------------------------------------------
def player_scene(pair, M, seed=0):
    """Five live stereo sources of the pair's rate for a block of M frames that starts at a large phase: no adapter; a LinearGainRamp that
    is still running beyond frame 2^33 of its stream; a ramp that ran out long ago under a factor table whose first is above 2^35; factors
    on a period of 3 from beyond 2^35; a running ramp under a factor period above 2^31."""
    rng = np.random.default_rng(seed)
    rate, to_rate = pair.from_rate, pair.to_rate
    m0 = W.largest_phase(pair)
    step_ns, far = 1_000_000_000 // rate, (1 << 33) + 12345
    mk = lambda **kw: PL.make(rng, 2, rate, to_rate, M, m0, **kw)  # noqa: E731
    srcs = [mk(), mk(kind=PR.RAMP, ramp_ns=((1 << 33) + (1 << 22)) * step_ns, start=0.2, end=1.4, first_frame=far), mk(kind=PR.CLAMP, ramp_ns=5 * MS, start=1.0, end=0.37, fp=441, ff=(1 << 35) + 6),
            mk(fp=3, ff=(1 << 35) + 2), mk(kind=PR.RAMP, ramp_ns=3000 * MS, start=0.0, end=1.0, fp=(1 << 33) + 1, ff=(1 << 33) - 200)]
    assert srcs[0].phase >= pair.T - pair.T // 100 and all(s.frames == M and s.last == PR.LIVE for s in srcs)
    top = PR.touched_frames(srcs[1], to_rate)
    assert srcs[1].first_frame > 1 << 33 and (srcs[1].first_frame + top) * step_ns < srcs[1].ramp_ns, "the ramp runs through the block"
    f = PR.ramp_factors(PR.RAMP, srcs[1].ramp_ns, 0.2, 1.4, rate, np.array([far, far + top - 1]))
    assert f[0] != f[1] and 1.0 < f[0] < 1.4
    assert srcs[2].first_frame * step_ns >= 5 * MS and srcs[2].factor_first > 1 << 35
    return srcs


@CUTS
def test_player_blocks_of_exactly_fit_frames(rh, pair):
    """The longest block the entry takes, against tests/player_mix_ref.py: stereo sources on an 8-byte boundary into dst on one (the
    specialised kernel) and off it, and the sources off the boundary (the general kernel both times)."""
    M = pair.fit
    srcs = player_scene(pair, M)
    assert M == W.fit_of(pair.from_rate, pair.to_rate)
    PL.hold(rh, srcs, pair.to_rate, M, 2, leads=(0, 1), chain=False, src_lead=2)
    PL.hold(rh, srcs, pair.to_rate, M, 2, leads=(0,), chain=False, src_lead=1)


@CUTS
def test_a_player_block_of_fit_plus_one_frames_is_refused(rh, pair):
    """RH_ERR_UNSUPPORTED, and dst is as it was -- with sources and tables that cover the longer block."""
    M = pair.fit + 1
    srcs = player_scene(pair, M)
    devs = [PL.Dev(s) for s in srcs]
    for lead in (0, 1):
        dst = arena.dst_arena(M * 2, lead)
        assert PL.call(dst.ptr(), 2, pair.to_rate, M, srcs, devs) == UNSUPPORTED
        dst.check(written=0)
    for d in devs:
        d.unchanged()


# ---- rh_uniform_segments(_dev) ------------------------------------------------------------------------------------------------------------------
class Segments:
    """Segments over ONE resident window of a span (x: its frames from frame `base` on, between NaN), each into a guarded dst of its own."""

    def __init__(self, x, base, ch, rate, to_ch, to_rate, gain=0.37):
        self.x, self.base, self.ch, self.rate, self.to_ch, self.to_rate, self.gain = x, base, ch, rate, to_ch, to_rate, gain
        self.F, self.T = W.reduced(rate, to_rate)
        self.src = arena.src_arena(x, lead=1)
        self.segs, self.dsts = [], []

    def add(self, m0, m1, span, dst_ptr=None):
        """[m0, m1) of a span of `span` frames (U64_MAX: open): src at the first tap's frame, src_frames exactly up to the last tap."""
        from rodio_amd import _lib

        first = m0 * self.F // self.T
        i_last = (m1 - 1) * self.F // self.T
        top = i_last if (self.F == self.T or i_last + 1 >= span) else i_last + 1
        assert self.base <= first and (top + 1 - self.base) * self.ch <= self.x.size
        s = _lib.UniformSeg()
        if dst_ptr is None:
            self.dsts.append(arena.dst_arena((m1 - m0) * self.to_ch, 1))
            dst_ptr = self.dsts[-1].ptr()
        s.src, s.dst = self.src.ptr() + 4 * (first - self.base) * self.ch, dst_ptr
        s.src_frame0, s.src_frames, s.m0, s.m1, s.span_frames = first, top + 1 - first, m0, m1, span
        s.from_rate, s.to_rate, s.from_ch, s.to_ch, s.gain, s.reserved = self.rate, self.to_rate, self.ch, self.to_ch, self.gain, 0
        self.segs.append(s)
        return s

    def ref(self, k):
        s = self.segs[k]
        return W.uniform_segment(self.x[(s.src_frame0 - self.base) * self.ch:], s.src_frame0, self.ch, self.rate, self.to_ch, self.to_rate, s.m0, s.m1, s.span_frames, self.gain)

    def run(self, dev_table):
        import torch

        from rodio_amd import _lib

        arr = (_lib.UniformSeg * len(self.segs))(*self.segs)
        most = max(s.m1 - s.m0 for s in self.segs)
        if dev_table:
            self.table = torch.from_numpy(np.frombuffer(bytes(arr), dtype=np.uint8).copy()).cuda()
            _lib.check(_lib.lib.rh_uniform_segments_dev(C.c_void_p(self.table.data_ptr()), len(self.segs), most, _st()), "rh_uniform_segments_dev")
        else:
            _lib.check(_lib.lib.rh_uniform_segments(arr, len(self.segs), _st()), "rh_uniform_segments")
        torch.cuda.synchronize()
        return most


def window(rng, F, T, ch, m_lo, m_hi, n_frames=None):
    """The frames the taps of [m_lo, m_hi) touch -- or up to frame n_frames - 1 of a span that ends there: (samples, first frame)."""
    base = m_lo * F // T
    top = (m_hi - 1) * F // T + (0 if F == T else 1) if n_frames is None else n_frames - 1
    return W.signal(rng, (top + 1 - base) * ch), base


@pytest.mark.parametrize("dev_table", [False, True], ids=["host-table", "device-table"])
@pytest.mark.parametrize("ch,rate,to_ch,to_rate", [(2, 44100, 2, 48000), (1, 65521, 2, 48000), (2, 48000, 6, 65521)])
def test_uniform_segments_at_the_2_31_boundary(G, ch, rate, to_ch, to_rate, dev_table):
    """[2^31 - 700, 2^31 + 700) ends beyond 2^31: its positions are 128-bit products.  [2^31 - 700, 2^31) over the same window takes the
    64-bit path.  Both equal the integer restatement, and each other where they overlap."""
    lo, mid, hi = (1 << 31) - 700, 1 << 31, (1 << 31) + 700
    sg = Segments(*window(np.random.default_rng(rate % 89), *W.reduced(rate, to_rate), ch, lo, hi), ch, rate, to_ch, to_rate)
    a, b = sg.add(lo, hi, W.U64_MAX), sg.add(lo, mid, W.U64_MAX)
    assert a.m1 > 1 << 31 >= b.m1, "the first segment takes the 128-bit path, the second the 64-bit one"
    sg.run(dev_table)
    long, short = sg.dsts[0].check(), sg.dsts[1].check()
    same_bits(long, sg.ref(0), to_ch, "the 128-bit path")
    same_bits(short, sg.ref(1), to_ch, "the 64-bit path")
    same_bits(long[: 700 * to_ch], short, to_ch, "the two paths over the same frames")
    sg.src.unchanged()


@pytest.mark.parametrize("dev_table", [False, True], ids=["host-table", "device-table"])
@pytest.mark.parametrize("ch,rate,to_ch,to_rate,m0", [(2, 44100, 2, 48000, (1 << 40) + 3), (1, 65521, 2, 48000, (1 << 50) + 1), (2, 65521, 1, 65519, (1 << 50) + 1)])
def test_uniform_segments_at_huge_positions(G, ch, rate, to_ch, to_rate, m0, dev_table):
    """1500 frames from m0 = 2^40 + 3 and from 2^50 + 1, where m F leaves 64 bits at F = 65 521: as an open span, and as a closed one whose
    last frame -- verbatim -- is the segment's last frame.  src points at frame floor(m0 F / T): the window is a few thousand frames."""
    F, T = W.reduced(rate, to_rate)
    assert m0 > 1 << 31 and (F != 65521 or m0 * F >= 1 << 64), "128-bit positions"
    rng = np.random.default_rng(rate % 83 + ch)
    # the closed span: the shortest one of at least 1000 frames past m0 whose last frame an output frame lands on
    m_v = m0 + 1000
    while W.out_frames(m_v * F // T + 1, F, T) != m_v + 1:
        m_v += 1
    n = m_v * F // T + 1
    assert m_v < m0 + 1500 and (m_v * F) // T == n - 1
    opened = Segments(*window(rng, F, T, ch, m0, m0 + 1500), ch, rate, to_ch, to_rate)
    opened.add(m0, m0 + 1500, W.U64_MAX)
    closed = Segments(*window(rng, F, T, ch, m0, m_v + 1, n), ch, rate, to_ch, to_rate)
    closed.add(m0, m_v + 1, n)
    assert closed.segs[0].src_frame0 + closed.segs[0].src_frames == n
    for what, sg in (("open", opened), ("closed", closed)):
        sg.run(dev_table)
        same_bits(sg.dsts[0].check(), sg.ref(0), to_ch, what)
        sg.src.unchanged()
    last = closed.dsts[0].check().reshape(-1, to_ch)[-1]
    want = closed.x.reshape(-1, ch)[-1] * f32(0.37)
    assert last[0] == want[0] and (to_ch == 1 or last[1] == want[1 if ch > 1 else 0]), "the span's last frame comes out verbatim"


def test_uniform_host_table_takes_the_2048_frame_tile(G, O):
    """One mono segment of 2.2 million output frames (8.8 MB) through the host table: ceil(frames / 2048) >= 1024 selects the large tile.
    Against the oracle's UniformSourceIterator over the continuous stream."""
    n = 2_021_300
    x = W.signal(np.random.default_rng(2048), n)
    total = W.out_frames(n, 147, 160)
    assert total >= 2_200_000 and -(-total // 2048) * 1 >= 1024, "tiles * n_segs >= 1024"
    sg = Segments(x, 0, 1, 44100, 1, 48000)
    sg.add(0, total, n)
    sg.run(False)
    want = O.UniformSourceIterator(O.TestSource(x, 1, 44100).amplify(0.37), 1, 48000).collect()
    same_bits(sg.dsts[0].check(), want, 1, "rh_uniform_segments, 2048-frame tiles")
    sg.src.unchanged()


def test_uniform_device_table_takes_the_2048_frame_tile_for_short_segments(G, O):
    """1100 segments of 300 frames of one continuous mono stream at 65 521 into stereo at 48 000, through the device table: a tile per
    segment, 1100 >= 1024 selects the 2048-frame tile for segments shorter than a tile.  Against the oracle."""
    F, T = W.reduced(65521, 48000)
    total = 1100 * 300
    n = W.ending_with(F, T, total)
    assert n is not None
    x = W.signal(np.random.default_rng(300), n)
    sg = Segments(x, 0, 1, 65521, 2, 48000)
    dst = arena.dst_arena(total * 2, 1)
    for k in range(1100):
        sg.add(300 * k, 300 * (k + 1), n if k == 1099 else W.U64_MAX, dst.ptr() + 4 * 2 * 300 * k)
    most = sg.run(True)
    assert most == 300 < 2048 and -(-most // 2048) * len(sg.segs) >= 1024, "tiles * n_segs >= 1024 with segments shorter than a tile"
    want = O.UniformSourceIterator(O.TestSource(x, 1, 65521).amplify(0.37), 2, 48000).collect()
    same_bits(dst.check(), want, 2, "rh_uniform_segments_dev, 2048-frame tiles")
    sg.src.unchanged()
