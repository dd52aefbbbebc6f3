"""rh_spatial_mix_block: a block of a mixer of spatial emitters in ONE launch -- per source SampleRateConverter(Amplify(ChannelVolume(x)))
with the volumes and the factor changing by steps, and the ordered sum.  Two references, both bit for bit (uint32 views, no tolerance:
everything is integer-indexed or IEEE-exact): tests/spatial_mix_ref.py (held against the oracle by tests/test_spatial_mix_cpu.py) and the
chain of existing entries the launch replaces -- rh_channel_volume_steps per source into stereo rows, rh_wide_mix_block over the rows.
dst lies in a guarded arena, sources and tables in arenas whose surroundings are NaN (tests/arena.py); a table holds exactly the entries
the block reaches, so an index one too far comes out as NaN."""
import ctypes as C

import numpy as np
import pytest

import arena
import spatial_mix_ref as R

pytestmark = pytest.mark.gpu

RATES = [(44100, 48000), (48000, 48000), (96000, 44100), (22050, 48000)]
LIVE = 0xFFFFFFFF
INVALID, UNSUPPORTED = 1, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(rng, in_ch, rate, to_rate, M, m0=0, n=None, ch=2, gp=1 << 40, gf=0, fp=None, ff=0, x=None):
    """A source of a block of M output frames that starts at frame m0 of the mix: live (n None: it reaches every frame with both taps) or
    ENDED with n frames left from `data` on.  Its samples are exactly the frames the block's taps touch and its tables exactly the entries
    those reach; gf / ff: the index, in the adapter's output, of the first sample of `data`."""
    F, T = R.reduced(rate, to_rate)
    phase = (m0 * F) % T
    frames, last = M, LIVE
    if n is not None:
        last = n - 1
        i = (phase + np.arange(M, dtype=np.int64) * F) // T
        hit = np.flatnonzero(i >= last)
        # the frame whose first tap is the last frame is emitted verbatim, and the source is over (a converter that steps over the last frame ends without it)
        frames = 0 if n == 0 else (M if hit.size == 0 else int(hit[0]) + (1 if i[hit[0]] == last else 0))
        if n == 0:
            last = 0
    s = R.Src(np.zeros(0, np.float32), in_ch, rate, frames, np.zeros((0, ch), np.float32), gp, gf, None, fp or 1, ff, phase, last)
    nt = R.touched_frames(s, to_rate)
    s.x = rng.uniform(-1, 1, nt * in_ch).astype(np.float32) if x is None else np.ascontiguousarray(x[: nt * in_ch], np.float32)
    s.gains = rng.uniform(-1, 1, (R.entries_needed(gf, gp, nt * ch), ch)).astype(np.float32)
    if fp:
        s.factors = rng.uniform(0.2, 1.5, R.entries_needed(ff, fp, nt * ch)).astype(np.float32)
    return s


class Dev:
    """A source's samples and tables on the device, each a row of an arena of its own at an odd 4-byte offset: between NaN (poison=True) or
    between zeros."""

    def __init__(self, s, poison=True, lead=1):
        import torch

        self.keep, self.ptr, self.view = [], {}, {}
        for name, a in (("x", s.x), ("gains", s.gains), ("factors", s.factors)):
            if a is None or a.size == 0:
                self.ptr[name], self.view[name] = None, None
                continue
            a = np.ascontiguousarray(a, np.float32).reshape(-1)
            if poison:
                ar = arena.src_arena(a, lead)
                self.keep.append(ar)
                st = ar.layout.starts[0]
                self.ptr[name], self.view[name] = ar.ptr(), ar.buf.view(torch.float32)[st: st + a.size]
            else:
                t, p = arena.plain(a, lead=lead)
                self.keep.append(t)
                self.ptr[name], self.view[name] = p, t[arena.GUARD + lead: arena.GUARD + lead + a.size]

    def unchanged(self):
        for k in self.keep:
            if isinstance(k, arena.Arena):
                k.unchanged()


def spatial_srcs(rh, srcs, devs, ch=2):
    return [rh.SpatialSrc(d.ptr["x"], s.in_ch, s.from_rate, s.frames, d.ptr["gains"], s.gain_period, s.gain_first, d.ptr["factors"], s.factor_period, s.factor_first, s.phase, s.last,
                          n_gains=s.gains.size // ch, n_factors=None if s.factors is None else s.factors.size) for s, d in zip(srcs, devs)]


def run_new(rh, srcs, devs, to_rate, M, ch=2, lead=0):
    """The entry into a guarded dst `lead` floats behind a 16-byte boundary: nothing stored outside, every word written."""
    dst = arena.dst_arena(M * ch, lead)
    rh.spatial_mix_block(dst.ptr(), ch, to_rate, M, spatial_srcs(rh, srcs, devs, ch))
    return dst.check()


def run_chain(rh, srcs, devs, to_rate, M, ch=2):
    """rh_channel_volume_steps per source into rows of the mixer's layout, then rh_wide_mix_block over the rows with gain 1."""
    import torch

    from rodio_amd import _lib, source

    arr = (_lib.WideSrc * max(len(srcs), 1))()
    rows = []
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].frames = s.frames
        if s.frames == 0:
            continue
        row = rh.channel_volume_steps(d.view["x"], s.in_ch, ch, s.gain_first, s.gain_period, d.view["gains"], s.factor_first, s.factor_period, d.view["factors"])
        rows.append(row)
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr(), ch, s.from_rate, s.phase, s.last, 1.0
    dst = torch.full((M * ch,), float("nan"), device="cuda")
    _lib.check(_lib.lib.rh_wide_mix_block(C.c_void_p(dst.data_ptr()), ch, to_rate, M, arr, len(srcs), source._stream()), "rh_wide_mix_block")
    return dst.cpu().numpy()


def hold(rh, srcs, to_rate, M, ch=2, leads=(0, 1), chain=True, fills=False):
    """The entry against the restatement (and the chain), dst on and off an 8-byte boundary (off it: the general kernel, whatever the
    sources are); fills: once more with the sources between zeros instead of NaN -- the same bits.  Inputs unchanged.  Returns the bits."""
    want = R.spatial_mix(ch, to_rate, M, srcs)
    devs = [Dev(s) for s in srcs]
    got = None
    for lead in leads:
        got = run_new(rh, srcs, devs, to_rate, M, ch, lead)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, f"lead {lead}: {bad.size} sample(s) differ from the restatement, the first at {int(bad[0])} (frame {int(bad[0]) // ch}): {got[bad[0]]!r} != {want[bad[0]]!r}"
    if chain:
        assert np.array_equal(bits(run_chain(rh, srcs, devs, to_rate, M, ch)), bits(want)), "the chain of existing entries differs from the restatement"
    if fills:
        plain = [Dev(s, poison=False) for s in srcs]
        for lead in leads:
            assert np.array_equal(bits(run_new(rh, srcs, plain, to_rate, M, ch, lead)), bits(want)), "the result depends on what surrounds the sources"
    for d in devs:
        d.unchanged()
    return bits(want)


# ---- parity ---------------------------------------------------------------------------------------------------------------------------------
SIZES = [(1, 1), (63, 3), (64, 32), (65, 33), (1000, 65), (1000, 1), (1, 65)]  # (out_frames, n_sources): 33 and 65 continue from the stored partial sum


@pytest.mark.parametrize("in_ch", [1, 2, 6])
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_parity_with_the_restatement_and_the_chain(rh, rate, to_rate, in_ch):
    """Live sources of one layout and rate in mid-stream (m0 = 12345: a nonzero phase, tables that start inside a step): with mono sources
    and dst on an 8-byte boundary the fast kernel, else the general one."""
    rng = np.random.default_rng(1000 * in_ch + rate % 89)
    m0 = 12345
    F, T = R.reduced(rate, to_rate)
    first = (m0 * F // T) * 2  # the first sample of `data` in the adapter's output
    for M, S in SIZES:
        srcs = [make(rng, in_ch, rate, to_rate, M, m0, gp=882 + k, gf=first, fp=(441 if k % 3 else None), ff=first + k) for k in range(S)]
        hold(rh, srcs, to_rate, M, fills=(M, S) == (65, 33))


def test_parity_of_a_mix_of_layouts_rates_and_ends(rh):
    """Everything side by side in one block of a stereo mixer at 48 kHz: layouts 1, 2, 6, five rates (a fifth one starts a launch), live and
    ended sources, one that reaches nothing; and a mixer of five channels (a ChannelVolume of five volumes)."""
    rng = np.random.default_rng(31)
    M, m0 = 700, 4001
    rates = [44100, 48000, 96000, 22050, 32000]
    for ch in (2, 5):
        srcs = []
        for k in range(41):
            rate, in_ch = rates[k % 5], (1, 2, 6)[k % 3]
            F, T = R.reduced(rate, 48000)
            n = None if k % 4 else int(rng.integers(0, M * F // T))
            srcs.append(make(rng, in_ch, rate, 48000, M, m0, n, ch, gp=(3, 2, 882, 1 << 40)[k % 4], gf=(m0 * F // T) * ch + k, fp=(None, 5, 441)[k % 3], ff=7 * k))
        hold(rh, srcs, 48000, M, ch, fills=True)


# ---- steps ----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gp,gf", [(3, 0), (3, (1 << 32) + 2), (2, 0), (2, 1), (882, 0), (882, 871), (882, (1 << 35) + 880), (1, 0), ((1 << 33) + 1, (1 << 33) - 200)])
@pytest.mark.parametrize("in_ch,rate,to_rate", [(1, 44100, 48000), (1, 48000, 48000), (2, 96000, 44100), (1, 22050, 48000)])
def test_steps(rh, in_ch, rate, to_rate, gp, gf):
    """Periods of 3 (a change in mid-frame) and 2 (every frame), 882 with firsts that put a boundary between the two taps of an output frame
    and between the channels of a frame, 1, and one beyond 2^31 with its single boundary inside the block; firsts beyond 2^32 (the host
    reduces them); the factor table absent, in step with the gains, and on a period of its own."""
    rng = np.random.default_rng(gp % 1000 + in_ch)
    M = 1000
    for fp, ff in ((None, 0), (gp, gf), (5, (1 << 40) + 3), (960, 957)):
        srcs = [make(rng, in_ch, rate, to_rate, M, gp=gp, gf=gf, fp=fp, ff=ff) for _ in range(3)]
        hold(rh, srcs, to_rate, M)


def test_a_boundary_between_the_two_taps_of_one_frame(rh):
    """44.1 -> 48 kHz, mono, period 882 = 441 frames: output frame 480 takes source frames 440 and 441, one from each side of the change.
    Held as a number: gains 1 and 0 on the two sides, a source of ones -- the frame is 1 - num / T, not 1 and not 0."""
    M = 600
    s = R.Src(np.ones(M, np.float32), 1, 44100, M, np.float32([[1, 1], [0, 0]]), 882)
    s.x = s.x[: R.touched_frames(s, 48000)]
    got = hold(rh, [s], 48000, M).view(np.float32).reshape(M, 2)
    assert (480 * 147) // 160 == 441 and (479 * 147) // 160 == 440
    j = 479  # first tap 440 (gain 1), second tap 441 (gain 0)
    num = (j * 147) % 160
    assert got[j, 0] == np.float32(1) + (np.float32(0) - np.float32(1)) * np.float32(num) / np.float32(160)
    assert got[j - 1, 0] == 1.0 and got[j + 1, 0] == 0.0


def call(rh, dst_ptr, ch, to_rate, M, srcs, devs, n_gains=None, n_factors=None, gain=1.0, tweak=None, null=()):
    """The raw entry: its status.  tweak(arr, gsteps, fsteps) edits the tables before the call; null: arrays passed as NULL."""
    from rodio_amd import _lib, source

    source._ensure()
    n = len(srcs)
    arr = (_lib.WideSrc * max(n, 1))()
    gains, factors = (C.c_void_p * max(n, 1))(), (C.c_void_p * max(n, 1))()
    gsteps, fsteps = (C.c_uint64 * (3 * max(n, 1)))(), (C.c_uint64 * (3 * max(n, 1)))()
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = d.ptr["x"], s.in_ch, s.from_rate, s.phase, s.frames, s.last, gain
        gains[k], factors[k] = d.ptr["gains"], d.ptr["factors"]
        gsteps[3 * k], gsteps[3 * k + 1], gsteps[3 * k + 2] = s.gain_first, s.gain_period, s.gains.shape[0] if n_gains is None else n_gains
        fsteps[3 * k], fsteps[3 * k + 1], fsteps[3 * k + 2] = s.factor_first, s.factor_period, (0 if s.factors is None else s.factors.size) if n_factors is None else n_factors
    if tweak:
        tweak(arr, gsteps, fsteps)
    a = dict(srcs=arr, gains=gains, gsteps=gsteps, factors=factors, fsteps=fsteps)
    for name in null:
        a[name] = None
    return _lib.lib.rh_spatial_mix_block(C.c_void_p(dst_ptr) if dst_ptr else None, ch, to_rate, M, a["srcs"], n, a["gains"], a["gsteps"], a["factors"], a["fsteps"], source._stream())


@pytest.mark.parametrize("rate,to_rate,n", [(44100, 48000, None), (48000, 48000, None), (44100, 48000, 300), (22050, 48000, 100)])
def test_a_table_one_entry_short_is_refused(rh, rate, to_rate, n):
    """The tables of make() reach exactly the last sample touched (every other test runs on such tables, between NaN); one entry fewer of
    either is RH_ERR_INVALID and dst is as it was -- for a live source (both taps of the last frame) and an ended one (the verbatim frame has
    one tap)."""
    rng = np.random.default_rng(3)
    M = 500
    # the last sample touched is the first one of its step, for the gains and for the factors
    probe = make(rng, 1, rate, to_rate, M, n=n)
    total = 2 * R.touched_frames(probe, to_rate)
    gp, fp = 100, 64
    gf, ff = (-(total - 1)) % gp, (-(total - 1)) % fp
    srcs = [make(rng, 1, rate, to_rate, M), make(rng, 1, rate, to_rate, M, n=n, gp=gp, gf=gf, fp=fp, ff=ff)]
    assert (gf + total - 1) % gp == 0 and (ff + total - 1) % fp == 0
    devs = [Dev(s) for s in srcs]
    hold(rh, srcs, to_rate, M, chain=False)
    for short in ("gains", "factors"):
        dst = arena.dst_arena(M * 2, 0)

        def tweak(arr, gsteps, fsteps, short=short):
            (gsteps if short == "gains" else fsteps)[3 * 1 + 2] -= 1

        assert call(rh, dst.ptr(), 2, to_rate, M, srcs, devs, tweak=tweak) == INVALID
        dst.check(written=0)
    dst = arena.dst_arena(M * 2, 0)
    assert call(rh, dst.ptr(), 2, to_rate, M, srcs, devs) == 0
    assert np.array_equal(bits(dst.check()), bits(R.spatial_mix(2, to_rate, M, srcs)))


# ---- ends -----------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("in_ch", [1, 2])
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_ends(rh, rate, to_rate, in_ch):
    """A source whose last frame lies inside the block (verbatim, silence behind it), one with frames == 0 and data == NULL, one that is
    live; then all sources ended before the block's end (zeros behind the last one); then a block long enough for the launcher's cut: the
    frames in front of the first end to the fast kernel, the rest to the general one."""
    rng = np.random.default_rng(rate % 1000 + in_ch)
    M = 1000
    F, T = R.reduced(rate, to_rate)
    n = 400 * F // T
    srcs = [make(rng, in_ch, rate, to_rate, M, gp=3, fp=7), make(rng, in_ch, rate, to_rate, M, n=n, gp=2, gf=1), make(rng, in_ch, rate, to_rate, M, n=0),
            make(rng, in_ch, rate, to_rate, M, n=n + 1, fp=882), make(rng, in_ch, rate, to_rate, M, n=1), make(rng, in_ch, rate, to_rate, M, n=2)]
    assert srcs[2].frames == 0 and srcs[2].x.size == 0 and 0 < srcs[1].frames < M
    hold(rh, srcs, to_rate, M)
    got = hold(rh, srcs[1:], to_rate, M)  # everything has ended by frame srcs[3].frames
    end = max(s.frames for s in srcs[1:])
    assert end < M and not got.reshape(M, 2)[end:].any() and got.reshape(M, 2)[:end].any()
    M = 3000
    n = 2000 * F // T
    srcs = [make(rng, in_ch, rate, to_rate, M, gp=882, fp=441) for _ in range(34)] + [make(rng, in_ch, rate, to_rate, M, n=n, gp=882)]
    assert 1024 <= srcs[-1].frames < M
    hold(rh, srcs, to_rate, M, chain=False)


# ---- zeros and specials ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,to_rate", [(48000, 48000), (44100, 48000)])
def test_zeros(rh, rate, to_rate):
    """A mono source of -0.0: the mean's `0 + s` makes +0.0 of it; with gain -1 it is -0.0 again, into a sum that started at +0.0.  Either
    way the mix is +0.0, bit for bit."""
    rng = np.random.default_rng(0)
    M = 200
    for g in (1.0, -1.0):
        s = make(rng, 1, rate, to_rate, M, x=np.full(M + 2, -0.0, np.float32))
        s.gains[:] = g
        assert np.all(bits(s.x) == 0x80000000)
        one = R.converted(s, 2, to_rate)
        if rate == to_rate:
            assert np.all(bits(one) == (0x80000000 if g < 0 else 0))  # the source's own contribution keeps the sign ...
        got = hold(rh, [s], to_rate, M)
        assert not got.any()  # ... the mix does not
        hold(rh, [s, make(rng, 1, rate, to_rate, M)], to_rate, M)


@pytest.mark.parametrize("in_ch,rate,to_rate", [(1, 44100, 48000), (2, 44100, 48000), (1, 48000, 48000), (1, 96000, 44100)])
def test_inf_and_nan_stay_where_their_taps_are(rh, in_ch, rate, to_rate):
    """Inf and NaN in ONE source: the frames whose taps touch them are not finite, every other frame is -- and is what the mix holds without
    them (a source is never multiplied by something that is not its own)."""
    rng = np.random.default_rng(17)
    M = 600
    srcs = [make(rng, in_ch, rate, to_rate, M, gp=3, fp=5) for _ in range(5)]
    clean = R.spatial_mix(2, to_rate, M, srcs)
    i, _, two, _ = R.taps(srcs[2], to_rate)
    spoiled = {int(i[60]): np.inf, int(i[61]) + 1: -np.inf, int(i[300]): np.nan, int(i[500]): np.inf}  # (frames that taps touch: a converter that goes down steps over some)
    for f, v in spoiled.items():
        srcs[2].x[f * in_ch + in_ch - 1] = v
    touched = np.zeros(M, bool)
    for f in spoiled:
        touched |= (i == f) | (two & (i + 1 == f))
    assert 4 <= touched.sum() < 20
    got = hold(rh, srcs, to_rate, M).view(np.float32).reshape(M, 2)
    assert np.array_equal(~np.isfinite(got).all(axis=1), touched)
    assert np.array_equal(bits(got[~touched]), bits(clean.reshape(M, 2)[~touched]))


# ---- kernel choice --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_the_fast_and_the_general_kernel_give_the_same_bits(rh, rate, to_rate):
    """A launch that qualifies for the fast kernel (mono, live, one rate, stereo dst on an 8-byte boundary), and the same launch with one
    source ENDING in the block's last frame -- its last frame is the first tap of that output frame, emitted verbatim -- which sends it to the
    general kernel: the frames in front of the last one hold the same bits, and so does the launch itself off the boundary."""
    rng = np.random.default_rng(rate % 777)
    M = 777
    srcs = [make(rng, 1, rate, to_rate, M, m0=999, gp=(3, 882, 2)[k % 3], gf=5 * k, fp=(None, 441, 1)[k % 3], ff=k) for k in range(37)]
    devs = [Dev(s) for s in srcs]
    want = R.spatial_mix(2, to_rate, M, srcs)
    fast = run_new(rh, srcs, devs, to_rate, M, 2, lead=0)
    assert np.array_equal(bits(fast), bits(want))
    assert np.array_equal(bits(run_new(rh, srcs, devs, to_rate, M, 2, lead=1)), bits(want))  # off the boundary: the general kernel
    F, T = R.reduced(rate, to_rate)
    s = srcs[20]
    s.last = int((s.phase + (M - 1) * F) // T)  # the same samples and tables, but the stream ends on the last frame's first tap
    want2 = R.spatial_mix(2, to_rate, M, srcs)
    general = run_new(rh, srcs, devs, to_rate, M, 2, lead=0)
    assert np.array_equal(bits(general), bits(want2))
    assert np.array_equal(bits(general[: 2 * (M - 1)]), bits(fast[: 2 * (M - 1)]))


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def test_arguments(rh):
    """Every refusal writes nothing (dst still holds the arena's sentinel); n_sources == 0 and sources that reach nothing write zeros."""
    rng = np.random.default_rng(8)
    M = 64
    srcs = [make(rng, 2, 44100, 48000, M, gp=3, fp=5), make(rng, 1, 44100, 48000, M)]
    devs = [Dev(s) for s in srcs]
    dst = arena.dst_arena(M * 2, 0)

    def refused(status=INVALID, ch=2, to_rate=48000, **kw):
        assert call(rh, dst.ptr(), ch, to_rate, M, srcs, devs, **kw) == status, kw
        dst.check(written=0)

    def field(k, name, value):
        return lambda arr, g, f: setattr(arr[k], name, value)

    assert call(rh, None, 2, 48000, M, srcs, devs) == INVALID
    refused(ch=0)
    refused(ch=17)
    refused(to_rate=0)
    refused(null=("srcs",))
    refused(null=("gains",))
    refused(null=("gsteps",))
    refused(null=("fsteps",))  # ... with a source that has factors
    # what rh_wide_mix_block refuses of the shared fields
    refused(tweak=field(1, "data", None))
    refused(tweak=field(1, "from_rate", 0))
    refused(tweak=field(1, "frames", M + 1))
    refused(tweak=field(1, "phase", 160))
    refused(UNSUPPORTED, tweak=field(1, "from_rate", 4294967291))
    # the emitter's own
    refused(tweak=field(0, "channels", 0))
    refused(gain=0.5)
    refused(tweak=lambda arr, g, f: g.__setitem__(3 * 1 + 1, 0))  # a gain period of 0
    refused(tweak=lambda arr, g, f: f.__setitem__(1, 0))          # a factor period of 0
    refused(n_gains=0)

    d2 = [Dev(s) for s in srcs]
    d2[1].ptr["gains"] = None
    assert call(rh, dst.ptr(), 2, 48000, M, srcs, d2) == INVALID  # gains NULL for a source with frames > 0
    dst.check(written=0)
    # out_frames == 0: nothing to do
    assert call(rh, dst.ptr(), 2, 48000, 0, srcs, devs) == 0
    dst.check(written=0)
    # no source, and sources that reach nothing (NULL everywhere): zeros
    for lead in (0, 1):
        z = arena.dst_arena(M * 2, lead)
        assert call(rh, z.ptr(), 2, 48000, M, [], []) == 0
        assert not bits(z.check()).any()
        z = arena.dst_arena(M * 2, lead)
        none = [make(rng, 1, 44100, 48000, M, n=0) for _ in range(3)]
        assert call(rh, z.ptr(), 2, 48000, M, none, [Dev(s) for s in none], tweak=lambda arr, g, f: [g.__setitem__(3 * k + 1, 0) for k in range(3)]) == 0
        assert not bits(z.check()).any()
    # a source without factors does not need the factor arrays
    assert call(rh, dst.ptr(), 2, 48000, M, srcs[1:], devs[1:], null=("factors", "fsteps")) == 0
    assert np.array_equal(bits(dst.check()), bits(R.spatial_mix(2, 48000, M, srcs[1:])))


def test_the_wrapper_takes_tensors(rh):
    """rodio_amd.spatial_mix_block with device tensors for the rows and tables (the tests above hand it addresses)."""
    import torch

    rng = np.random.default_rng(4)
    M = 300
    srcs = [make(rng, 1, 44100, 48000, M, gp=882, fp=441) for _ in range(3)]
    dst = torch.full((2 * M,), float("nan"), device="cuda")
    up = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    rh.spatial_mix_block(dst, 2, 48000, M, [rh.SpatialSrc(up(s.x), 1, 44100, M, up(s.gains), 882, factors=up(s.factors), factor_period=441) for s in srcs])
    assert np.array_equal(bits(dst.cpu().numpy()), bits(R.spatial_mix(2, 48000, M, srcs)))
    with pytest.raises(ValueError):
        rh.spatial_mix_block(dst, 2, 48000, M, [rh.SpatialSrc(up(srcs[0].x), 1, 44100, M, up(srcs[0].gains).double(), 882)])
