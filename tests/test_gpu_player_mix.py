"""rh_player_mix_block: a block of a mixer of Players in ONE launch -- per source the gain, the LinearGainRamp, the Amplify whose factor
changes by steps, the converter to the mixer's rate and layout, and the ordered sum.  Two references, both bit for bit (uint32 views, no
tolerance: everything is integer-indexed or IEEE-exact): tests/player_mix_ref.py (held against the oracle by tests/test_player_mix_cpu.py)
and the chain of existing entries the launch replaces -- rh_amplify -> rh_linear_gain_ramp -> rh_amplify_steps per source into a row,
rh_wide_mix_block over the rows with gain 1.  dst lies in a guarded arena, sources and tables in arenas whose surroundings are NaN
(tests/arena.py); a source holds exactly the samples the block's taps read and a table exactly the entries those reach, so an index one
too far comes out as NaN.  Inputs are finite floats, +0.0 and -0.0 among them."""
import ctypes as C

import numpy as np
import pytest

import arena
import player_mix_ref as R
import stream_gate

pytestmark = pytest.mark.gpu

RATES = [(44100, 48000), (48000, 44100), (48000, 48000), (8000, 48000)]
LAYOUTS = [(1, 2), (2, 2), (2, 1), (6, 2), (2, 6)]
GRID = [(r, t, c, tc) for r, t in RATES for c, tc in LAYOUTS]
MS = 1_000_000
LIVE = R.LIVE
INVALID, UNSUPPORTED = 1, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def make(rng, ch, rate, to_rate, M, m0=0, n=None, to_ch=2, gain=None, kind=R.NONE, ramp_ns=5 * MS, start=0.0, end=1.0, first_frame=None, ramp_rate=None, fp=None, ff=None):
    """A source of a block of M output frames that starts at frame m0 of the mix: live (n None: it reaches every frame with both taps) or
    ENDED with n frames left from `data` on.  Its samples are exactly the ones the block's taps read and its table exactly the entries those
    reach; first_frame / ff: the index, in the adapter's stream, of the first frame / sample of `data` (None: what lies in front of m0)."""
    F, T = R.reduced(rate, to_rate)
    phase, i0 = (m0 * F) % T, (m0 * F) // T
    frames, last = M, LIVE
    if n is not None:
        last = n - 1
        i = (phase + np.arange(M, dtype=np.int64) * F) // T
        hit = np.flatnonzero(i >= last)
        # the frame whose first tap is the last frame is emitted verbatim, and the source is over (a converter that steps over the last frame ends without it)
        frames = 0 if n == 0 else (M if hit.size == 0 else int(hit[0]) + (1 if i[hit[0]] == last else 0))
        if n == 0:
            last = 0
    s = R.Src(np.zeros(0, np.float32), ch, rate, frames, float(rng.uniform(0.3, 1.2)) if gain is None else gain, kind, ramp_ns, start, end, i0 if first_frame is None else first_frame,
              ramp_rate, None, fp or 1, (i0 * ch if ff is None else ff), phase, last)
    ns = R.reached_samples(s, to_ch, to_rate)
    s.x = rng.uniform(-1, 1, ns).astype(np.float32)
    if ns > 8:  # zeros of both signs among the samples
        z = rng.integers(0, ns, 4)
        s.x[z[:2]], s.x[z[2:]] = 0.0, -0.0
    if fp:
        s.factors = rng.uniform(0.2, 1.5, R.entries_needed(s.factor_first, fp, ns)).astype(np.float32)
    return s


class Dev:
    """A source's samples and table on the device, each a row of an arena of its own `lead` floats behind a 16-byte boundary, between NaN."""

    def __init__(self, s, lead=2):
        self.keep, self.ptr = [], {}
        for name, a in (("x", s.x), ("factors", s.factors)):
            if a is None or a.size == 0:
                self.ptr[name] = None
                continue
            ar = arena.src_arena(np.ascontiguousarray(a, np.float32).reshape(-1), lead)
            self.keep.append(ar)
            self.ptr[name] = ar.ptr()

    def unchanged(self):
        for k in self.keep:
            k.unchanged()


def player_srcs(rh, srcs, devs):
    return [rh.PlayerSrc(d.ptr["x"], s.ch, s.from_rate, s.frames, gain=float(s.gain), ramp=s.kind, ramp_ns=s.ramp_ns, start_gain=float(s.start), end_gain=float(s.end),
                         first_frame=s.first_frame, ramp_rate=s.ramp_rate, factors=d.ptr["factors"], factor_period=s.factor_period, factor_first=s.factor_first, phase=s.phase,
                         last=s.last, n_factors=None if s.factors is None else s.factors.size) for s, d in zip(srcs, devs)]


def run_new(rh, srcs, devs, to_rate, M, ch=2, lead=0):
    """The entry into a guarded dst `lead` floats behind a 16-byte boundary: nothing stored outside, every word written."""
    dst = arena.dst_arena(M * ch, lead)
    rh.player_mix_block(dst.ptr(), ch, to_rate, M, player_srcs(rh, srcs, devs))
    return dst.check()


def run_chain(rh, srcs, devs, to_rate, M, ch=2):
    """Per source rh_amplify -> rh_linear_gain_ramp (sample_offset = first_frame * channels) -> rh_amplify_steps into a row, then
    rh_wide_mix_block over the rows with gain 1."""
    import torch

    from rodio_amd import _lib, source

    source._ensure()
    lib, st, vp = _lib.lib, source._stream(), C.c_void_p
    arr = (_lib.WideSrc * max(len(srcs), 1))()
    rows = []
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].frames = s.frames
        if s.frames == 0:
            continue
        n = s.x.size
        row = torch.full((n,), float("nan"), device="cuda")
        rows.append(row)
        p = vp(row.data_ptr())
        _lib.check(lib.rh_amplify(p, vp(d.ptr["x"]), n, float(s.gain), st), "rh_amplify")
        if s.kind != R.NONE:
            _lib.check(lib.rh_linear_gain_ramp(p, p, n, s.first_frame * s.ch, s.ch, s.ramp_rate, s.ramp_ns, float(s.start), float(s.end), int(s.kind == R.CLAMP), st), "rh_linear_gain_ramp")
        if s.factors is not None:
            _lib.check(lib.rh_amplify_steps(p, p, n, s.factor_first, s.factor_period, vp(d.ptr["factors"]), s.factors.size, st), "rh_amplify_steps")
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr(), s.ch, s.from_rate, s.phase, s.last, 1.0
    dst = torch.full((M * ch,), float("nan"), device="cuda")
    _lib.check(lib.rh_wide_mix_block(vp(dst.data_ptr()), ch, to_rate, M, arr, len(srcs), st), "rh_wide_mix_block")
    return dst.cpu().numpy()


def hold(rh, srcs, to_rate, M, ch=2, leads=(0, 1), chain=True, src_lead=2):
    """The entry against the restatement (and the chain), dst on and off an 8-byte boundary (off it: the general kernel, whatever the
    sources are).  Inputs unchanged.  Returns the restatement's bits."""
    want = R.player_mix(ch, to_rate, M, srcs)
    assert np.isfinite(want).all()
    devs = [Dev(s, src_lead) for s in srcs]
    for lead in leads:
        got = run_new(rh, srcs, devs, to_rate, M, ch, lead)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, f"lead {lead}: {bad.size} sample(s) differ from the restatement, the first at {int(bad[0])} (frame {int(bad[0]) // ch}): {got[bad[0]]!r} != {want[bad[0]]!r}"
    if chain:
        assert np.array_equal(bits(run_chain(rh, srcs, devs, to_rate, M, ch)), bits(want)), "the chain of existing entries differs from the restatement"
    for d in devs:
        d.unchanged()
    return bits(want)


# ---- one source -----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,to_rate,ch,to_ch", GRID)
def test_one_source_without_and_with_each_adapter(rh, rate, to_rate, ch, to_ch):
    """No ramp, a ramp only, factors only, both -- in mid-stream (m0 = 12345: a nonzero phase, a table that starts inside a step), the ramp
    running through the whole block."""
    rng = np.random.default_rng(rate % 89 + 10 * ch + to_ch)
    M, m0 = 300, 12345
    for kind, fp in ((R.NONE, None), (R.RAMP, None), (R.NONE, 7), (R.CLAMP, 441)):
        s = make(rng, ch, rate, to_rate, M, m0, to_ch=to_ch, kind=kind, ramp_ns=2000 * MS, start=0.2, end=-1.5, fp=fp)
        hold(rh, [s], to_rate, M, to_ch)


@pytest.mark.parametrize("rate,to_rate,ch,to_ch", GRID)
def test_a_ramp_that_ends_inside_the_block(rh, rate, to_rate, ch, to_ch):
    """A fade_in and a clamped ramp of 5 ms from the block's first frame: done_frame lies inside the block, and where the converter has two
    taps there is an output frame that takes one from each side of it."""
    rng = np.random.default_rng(rate % 83 + 10 * ch + to_ch)
    M = 400
    step_ns = 1_000_000_000 // rate
    done = -(-5 * MS // step_ns)
    F, T = R.reduced(rate, to_rate)
    i = (np.arange(M) * F) // T
    assert 0 < done < i[-1]
    if F != T:
        assert np.any(i == done - 1), "an output frame whose taps are frames done - 1 and done"
    srcs = [make(rng, ch, rate, to_rate, M, to_ch=to_ch, kind=R.RAMP, fp=5), make(rng, ch, rate, to_rate, M, to_ch=to_ch, kind=R.CLAMP, start=1.3, end=0.4)]
    got = hold(rh, srcs, to_rate, M, to_ch)
    # the factor on the two sides, as numbers: the last frame of the ramp is not yet `after`
    f = R.ramp_factors(R.CLAMP, 5 * MS, 1.3, 0.4, rate, np.arange(done - 1, done + 1))
    assert f[0] != np.float32(0.4) and f[1] == np.float32(0.4) and got.any()


@pytest.mark.parametrize("rate,to_rate,ch,to_ch", GRID)
def test_a_second_block(rh, rate, to_rate, ch, to_ch):
    """first_frame > 0: a block that starts inside the ramp (it ends in this block), and one that starts past done_frame, for both clamp
    settings -- the ramp is then ONE constant on the host, 1 or end_gain."""
    rng = np.random.default_rng(rate % 79 + 10 * ch + to_ch)
    M = 350
    F, T = R.reduced(rate, to_rate)
    done = -(-20 * MS // (1_000_000_000 // rate))
    inside = ((done - 40) * T) // F  # the mix frame whose first tap lies 40 frames in front of done_frame
    assert inside > 0
    for m0 in (inside, ((done + 3) * T + F - 1) // F, 10**7):
        srcs = [make(rng, ch, rate, to_rate, M, m0, to_ch=to_ch, kind=R.RAMP, ramp_ns=20 * MS, fp=11), make(rng, ch, rate, to_rate, M, m0, to_ch=to_ch, kind=R.CLAMP, ramp_ns=20 * MS, start=1.0, end=0.37)]
        assert (srcs[0].first_frame >= done) == (m0 != inside) and srcs[0].first_frame > 0
        hold(rh, srcs, to_rate, M, to_ch)
    # past the ramp the clamped source IS its end gain, as a number: the same block from a source without a ramp and gain * 0.37 per tap
    s = make(rng, ch, rate, to_rate, M, 10**7, to_ch=to_ch, gain=0.8, kind=R.CLAMP, ramp_ns=20 * MS, start=1.0, end=0.37)
    got = hold(rh, [s], to_rate, M, to_ch, chain=False)
    plain = R.Src(s.x, ch, rate, s.frames, 0.8, factors=np.float32([0.37]), factor_period=1 << 40, phase=s.phase)
    assert np.array_equal(got, bits(R.player_mix(to_ch, to_rate, M, [plain])))


@pytest.mark.parametrize("to_ch", [2, 1, 6])
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_a_step_boundary_in_mid_frame(rh, rate, to_rate, to_ch):
    """A stereo source and odd periods: 3 (a change inside every other frame, and between the two taps of most lerps), 441 with a first that
    puts boundaries on odd samples, 1 (every sample); firsts beyond 2^32 (the host reduces them); a period beyond 2^31 with its one
    boundary inside the block."""
    rng = np.random.default_rng(rate % 71 + to_ch)
    M = 1000
    for fp, ff in ((3, 0), (3, (1 << 32) + 2), (441, 440), (441, (1 << 35) + 6), (1, 0), ((1 << 33) + 1, (1 << 33) - 200)):
        srcs = [make(rng, 2, rate, to_rate, M, to_ch=to_ch, kind=(R.NONE, R.RAMP)[k], fp=fp, ff=ff) for k in range(2)]
        k = np.arange(srcs[0].x.size, dtype=np.int64)
        e = (ff + k) // fp - ff // fp
        assert np.any(e[1::2] != e[0::2][: e[1::2].size]), "a boundary between the two channels of a frame"
        hold(rh, srcs, to_rate, M, to_ch)


def test_a_boundary_between_the_two_taps_of_one_frame_as_a_number(rh):
    """44.1 -> 48 kHz, mono, period 441: output frame 479 takes source frames 440 and 441, one from each side of the change.  Factors 1 and
    0, a source of ones: the frame is 1 - num / T, not 1 and not 0."""
    M = 600
    s = R.Src(np.ones(M, np.float32), 1, 44100, M, factors=np.float32([1, 0]), factor_period=441)
    s.x = s.x[: R.reached_samples(s, 2, 48000)]
    got = hold(rh, [s], 48000, M).view(np.float32).reshape(M, 2)
    assert (480 * 147) // 160 == 441 and (479 * 147) // 160 == 440
    num = (479 * 147) % 160
    assert got[479, 0] == np.float32(1) + (np.float32(0) - np.float32(1)) * np.float32(num) / np.float32(160)
    assert got[478, 0] == 1.0 and got[480, 0] == 0.0 and np.array_equal(got[:, 0], got[:, 1])


# ---- more than one launch -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", [33, 37])
def test_more_sources_than_a_launch_holds(rh, S):
    """33 and 37 sources of five rates and three layouts in one call: launches continue from the stored partial sum, a fifth rate starts one
    early; live sources beside ones that end inside the block (`last` set, frames < out_frames), one of frames == 0 with NULL pointers; ramps
    that run, that end in the block and that ran out long ago; into a stereo mix and a mix of five channels."""
    rng = np.random.default_rng(S)
    M, m0 = 700, 4001
    rates = [44100, 48000, 96000, 22050, 8000]
    for ch in (2, 5):
        srcs = []
        for k in range(S):
            rate, in_ch = rates[k % 5], (2, 1, 6)[k % 3]
            F, T = R.reduced(rate, 48000)
            n = None if k % 4 else int(rng.integers(0 if k == 8 else 1, M * F // T))
            if k == 8:
                n = 0
            srcs.append(make(rng, in_ch, rate, 48000, M, m0, n, ch, kind=(R.NONE, R.RAMP, R.CLAMP)[k % 3], ramp_ns=(90 * MS, 1 * MS)[k % 2], start=0.1 * k, end=1.0 - 0.05 * k,
                             fp=(None, 5, 441)[(k // 2) % 3], ff=7 * k))
        assert srcs[8].frames == 0 and srcs[8].x.size == 0 and any(0 < s.frames < M for s in srcs)
        hold(rh, srcs, 48000, M, ch)


def test_no_sources_and_sources_that_reach_nothing(rh):
    """n_sources == 0 writes zeros (on and off the boundary), and so do sources of frames == 0 whose every pointer is NULL."""
    rng = np.random.default_rng(2)
    M = 300
    for lead in (0, 1):
        assert not bits(run_new(rh, [], [], 48000, M, 2, lead)).any()
        none = [make(rng, 2, 44100, 48000, M, n=0) for _ in range(3)]
        assert not bits(run_new(rh, none, [Dev(s) for s in none], 48000, M, 2, lead)).any()


def test_the_ramp_counts_time_at_the_rate_in_front_of_speed(rh):
    """A source at 44100 relabelled 66150 by speed 1.5 (speed.rs), inside a fade_in: from_rate is what the mixer sees, the ramp's rate
    stays 44100.  The chain's rh_linear_gain_ramp runs at 44100 too; a ramp at 66150 is another block."""
    rng = np.random.default_rng(9)
    M = 900
    s = make(rng, 2, 66150, 48000, M, kind=R.RAMP, ramp_ns=10 * MS, ramp_rate=44100, fp=441)
    got = hold(rh, [s], 48000, M)
    s.ramp_rate = 66150
    assert not np.array_equal(bits(R.player_mix(2, 48000, M, [s])), got)


# ---- kernel choice --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,to_rate", RATES)
def test_the_specialised_and_the_general_kernel_give_the_same_bits(rh, rate, to_rate):
    """A scene the specialised kernel takes -- stereo live sources of one rate on 8-byte boundaries into a stereo dst on one: 37 of them, a
    full launch and one of five --, the same with dst moved by 4 bytes and with the ROWS moved by 4 bytes, which it must not take, and with
    one source ENDING on the block's last frame (that frame verbatim), which sends its launch to the general kernel: the frames in front
    of the last one hold the same bits."""
    rng = np.random.default_rng(rate % 777)
    M = 777
    srcs = [make(rng, 2, rate, to_rate, M, m0=999, kind=(R.NONE, R.RAMP, R.CLAMP)[k % 3], ramp_ns=(2000 * MS, 1 * MS)[k % 2], first_frame=(0, 10, 10**6)[k % 3], start=0.3, end=1.2,
                 fp=(None, 441, 3)[(k // 3) % 3], ff=k) for k in range(37)]
    want = R.player_mix(2, to_rate, M, srcs)
    devs = [Dev(s, 2) for s in srcs]
    fast = run_new(rh, srcs, devs, to_rate, M, 2, lead=0)
    assert np.array_equal(bits(fast), bits(want))
    assert np.array_equal(bits(run_new(rh, srcs, devs, to_rate, M, 2, lead=2)), bits(want))  # 8 bytes behind a 16-byte boundary: still taken
    assert np.array_equal(bits(run_new(rh, srcs, devs, to_rate, M, 2, lead=1)), bits(want))  # dst off the boundary: the general kernel
    assert np.array_equal(bits(run_new(rh, srcs, [Dev(s, 1) for s in srcs], to_rate, M, 2, lead=0)), bits(want))  # the rows off it
    F, T = R.reduced(rate, to_rate)
    s = srcs[20]
    s.last = int((s.phase + (M - 1) * F) // T)  # the same samples and table, but the stream ends on the last frame's first tap
    want2 = R.player_mix(2, to_rate, M, srcs)
    general = run_new(rh, srcs, devs, to_rate, M, 2, lead=0)
    assert np.array_equal(bits(general), bits(want2))
    same = int(np.flatnonzero((s.phase + np.arange(M, dtype=np.int64) * F) // T >= s.last)[0])  # the frames in front of the first one on the last frame
    assert M - 6 <= same < M and np.array_equal(bits(general[: 2 * same]), bits(fast[: 2 * same]))
    for d in devs:
        d.unchanged()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def tables(srcs, devs, host=lambda a, value=None: a, pit=0):
    """The entry's five host arrays; host(array, value): what a gated case registers them with."""
    from rodio_amd import _lib

    n = max(len(srcs), 1)
    arr = host((_lib.WideSrc * n)(), 0)
    ramps, gains = host((C.c_uint64 * (4 * n))(), 0), host((C.c_float * (2 * n))(), 0)
    factors, fsteps = host((C.c_void_p * n)(), pit), host((C.c_uint64 * (3 * n))(), 0)
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = d.ptr["x"], s.ch, s.from_rate, s.phase, s.frames, s.last, float(s.gain)
        ramps[4 * k: 4 * k + 4] = [s.kind, s.ramp_ns, s.first_frame, s.ramp_rate]
        gains[2 * k: 2 * k + 2] = [float(s.start), float(s.end)]
        factors[k] = d.ptr["factors"]
        fsteps[3 * k: 3 * k + 3] = [s.factor_first, s.factor_period, 0 if s.factors is None else s.factors.size]
    return dict(srcs=arr, ramps=ramps, gains=gains, factors=factors, fsteps=fsteps)


def call(dst_ptr, ch, to_rate, M, srcs, devs, tweak=None, null=(), n=None):
    """The raw entry: its status.  tweak(arr, ramps, gains, factors, fsteps) edits the tables before the call; null: arrays passed as NULL."""
    from rodio_amd import _lib, source

    source._ensure()
    a = tables(srcs, devs)
    if tweak:
        tweak(a["srcs"], a["ramps"], a["gains"], a["factors"], a["fsteps"])
    for name in null:
        a[name] = None
    return _lib.lib.rh_player_mix_block(C.c_void_p(dst_ptr) if dst_ptr else None, ch, to_rate, M, a["srcs"], len(srcs) if n is None else n, a["ramps"], a["gains"], a["factors"],
                                        a["fsteps"], source._stream())


def test_every_refusal_writes_nothing(rh):
    """Each refusal of rodio_hip.h returns its status and leaves dst as it was (the arena's sentinel in every word)."""
    rng = np.random.default_rng(8)
    M = 300
    srcs = [make(rng, 2, 44100, 48000, M, kind=R.RAMP, fp=5), make(rng, 1, 44100, 48000, M)]
    devs = [Dev(s) for s in srcs]
    dst = arena.dst_arena(M * 2, 0)

    def refused(status=INVALID, ch=2, to_rate=48000, frames=M, **kw):
        assert call(dst.ptr(), ch, to_rate, frames, srcs, devs, **kw) == status, kw
        dst.check(written=0)

    def field(k, name, value):
        return lambda arr, r, g, f, fs: setattr(arr[k], name, value)

    def word(which, i, value):
        return lambda arr, r, g, f, fs: (r if which == "ramps" else fs).__setitem__(i, value)

    assert call(None, 2, 48000, M, srcs, devs) == INVALID
    refused(ch=0)
    refused(to_rate=0)
    refused(null=("srcs",))
    # what rh_wide_mix_block refuses of the shared fields
    refused(tweak=field(1, "data", None))
    refused(tweak=field(1, "channels", 0))
    refused(tweak=field(1, "from_rate", 0))
    refused(tweak=field(1, "frames", M + 1))
    refused(tweak=field(1, "phase", 160))
    refused(UNSUPPORTED, tweak=field(1, "from_rate", 4294967291))  # F T beyond 32 bits
    # the adapters
    refused(tweak=word("ramps", 0, 3))              # a kind above 2
    refused(tweak=word("ramps", 3, 0))              # a ramp rate of 0
    refused(null=("gains",))                        # a ramp without its gains
    refused(null=("fsteps",))                       # factors without their steps
    refused(tweak=word("fsteps", 1, 0))             # a factor period of 0
    refused(tweak=word("fsteps", 2, srcs[0].factors.size - 1))  # a table one entry short
    # blocks that are refused, not cut: phase + j F leaves 32 bits; the step rule's sample index leaves 2^30
    refused(UNSUPPORTED, frames=0x7FFFFFFF)
    refused(UNSUPPORTED, frames=0x80000000)
    refused(UNSUPPORTED, to_rate=44100, frames=0x7FFFFFFF, tweak=lambda arr, r, g, f, fs: (setattr(arr[0], "frames", (1 << 29) + 1), fs.__setitem__(1, 1 << 40)))
    # out_frames == 0: nothing to do, whatever the rest says
    assert call(dst.ptr(), 0, 0, 0, srcs, devs, null=("srcs",)) == 0
    dst.check(written=0)
    # kind 0 reads neither the ramp's rate nor the gains; no factors: the steps are not read
    assert call(dst.ptr(), 2, 48000, M, srcs[1:], devs[1:], null=("gains", "factors", "fsteps"), tweak=word("ramps", 3, 0)) == 0
    assert np.array_equal(bits(dst.check()), bits(R.player_mix(2, 48000, M, srcs[1:])))
    dst = arena.dst_arena(M * 2, 0)
    assert call(dst.ptr(), 2, 48000, M, srcs[1:], devs[1:], null=("ramps", "gains", "factors", "fsteps")) == 0
    assert np.array_equal(bits(dst.check()), bits(R.player_mix(2, 48000, M, srcs[1:])))
    dst = arena.dst_arena(M * 2, 0)
    assert call(dst.ptr(), 2, 48000, M, srcs, devs) == 0
    assert np.array_equal(bits(dst.check()), bits(R.player_mix(2, 48000, M, srcs)))


@pytest.mark.parametrize("rate,to_rate,n", [(44100, 48000, None), (48000, 48000, None), (44100, 48000, 200), (8000, 48000, 40)])
def test_a_table_one_entry_short_is_refused(rh, rate, to_rate, n):
    """The last sample a tap reads is the first one of its step: the table make() gives holds exactly the entries reached, one fewer is
    RH_ERR_INVALID and dst is as it was -- for a live source (both taps of the last frame) and an ended one (the verbatim frame has one
    tap), stereo into stereo and six channels into two (the last frame's channels 2 .. 5 are not reached)."""
    rng = np.random.default_rng(3)
    M = 300
    for ch in (2, 6):
        probe = make(rng, ch, rate, to_rate, M, n=n)
        total = R.reached_samples(probe, 2, to_rate)
        fp = 64
        ff = (-(total - 1)) % fp
        srcs = [make(rng, ch, rate, to_rate, M), make(rng, ch, rate, to_rate, M, n=n, kind=R.RAMP, fp=fp, ff=ff)]
        assert (ff + total - 1) % fp == 0 and srcs[1].x.size == total
        devs = [Dev(s) for s in srcs]
        hold(rh, srcs, to_rate, M, chain=False)
        dst = arena.dst_arena(M * 2, 0)
        assert call(dst.ptr(), 2, to_rate, M, srcs, devs, tweak=lambda arr, r, g, f, fs: fs.__setitem__(3 * 1 + 2, fs[3 * 1 + 2] - 1)) == INVALID
        dst.check(written=0)


# ---- a side stream --------------------------------------------------------------------------------------------------------------------------
class DelayOn(stream_gate.Delay):
    """stream_gate.Delay with its fill time measured on the stream under test instead of on a new stream of torch's."""

    def __init__(self, s):
        import torch

        self.big = torch.empty(stream_gate.GIB, dtype=torch.uint8, device="cuda")
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            self.big.zero_()
            e0.record()
            for _ in range(8):
                self.big.zero_()
            e1.record()
        e1.synchronize()
        self.fill_ms = e0.elapsed_time(e1) / 8.0
        assert self.fill_ms > 0.0


def test_behind_a_gate_on_a_side_stream(rh):
    """Every launch of the call goes to the stream it is given (tests/stream_gate.py): 33 sources -- two launches, the second continuing the
    stored sum -- queued behind a gate on a side stream while their inputs still hold garbage, the five host arrays overwritten as soon as
    the call has returned.  The call returns while the gate is pending, and the snapshot holds the restatement's bits.
    The side stream is one of rh_stream_create, destroyed when the case is over, and nothing here takes a stream from torch's pool: which
    streams share a hardware queue decides what a gate holds back in tests/test_gpu_stream_order.py, which runs after this file in the same
    process, and a pool stream taken here moved every stream that file takes to another queue (two of its cases then saw a call wait for
    the gate, and a copy on the null stream wait with it)."""
    import torch

    from rodio_amd import _lib, source

    source._ensure()
    h = C.c_void_p()
    assert _lib.lib.rh_stream_create(C.byref(h)) == 0
    try:
        _behind_a_gate(torch.cuda.ExternalStream(h.value))
    finally:
        assert _lib.lib.rh_stream_destroy(h) == 0


def _behind_a_gate(side):
    from rodio_amd import _lib, source

    delay = DelayOn(side)
    rng = np.random.default_rng(0)
    M, S, to_rate = 300, 33, 48000
    srcs = [make(rng, (2, 1)[k % 2], 44100, to_rate, M, 12345, kind=(R.NONE, R.RAMP, R.CLAMP)[k % 3], ramp_ns=(2000 * MS, 1 * MS)[k % 2], fp=(441 if k % 3 else None), ff=k) for k in range(S)]
    want = R.player_mix(2, to_rate, M, srcs)

    def build(k):
        devs = [Dev(s) for s in srcs]
        for d in devs:
            for a in d.keep:
                k.add(a)
        dst = k.dst(M * 2, 0)

        def one():
            a = tables(srcs, devs, k.host, k.pit())
            _lib.check(_lib.lib.rh_player_mix_block(C.c_void_p(dst.ptr()), 2, to_rate, M, a["srcs"], S, a["ramps"], a["gains"], a["factors"], a["fsteps"], source._stream()), "rh_player_mix_block")

        def check():
            assert arena.same(dst.check_snapshot(), want)
            for d in devs:
                for a in d.keep:
                    a.snapshot_unchanged()

        return stream_gate.case([one], check)

    r = stream_gate.run(build, side, delay, 63.0)  # ms: three times the 21 ms a call that test_gpu_stream_order.py's gates last, for a host busy with others' work
    assert all(r.pending), ("the call waited for the stream, or the gate is too short", r.pending, r.host_ms)
    r.check()


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_takes_tensors(rh):
    """rodio_amd.player_mix_block with device tensors for the rows and tables (the tests above hand it addresses), the ramp by name."""
    import torch

    rng = np.random.default_rng(4)
    M = 300
    srcs = [make(rng, 2, 44100, 48000, M, kind=(R.RAMP, R.CLAMP, R.NONE)[k], ramp_ns=3 * MS, start=(0.0, 1.0, 1.0)[k], end=(1.0, 0.0, 1.0)[k], fp=441) for k in range(3)]
    dst = torch.full((2 * M,), float("nan"), device="cuda")
    up = lambda a: torch.from_numpy(a).cuda()  # noqa: E731
    rh.player_mix_block(dst, 2, 48000, M, [rh.PlayerSrc(up(s.x), 2, 44100, M, gain=float(s.gain), ramp=("fade_in", "fade_out", None)[k], ramp_ns=3 * MS, factors=up(s.factors), factor_period=441)
                                           for k, s in enumerate(srcs)])
    assert np.array_equal(bits(dst.cpu().numpy()), bits(R.player_mix(2, 48000, M, srcs)))
    with pytest.raises(ValueError):
        rh.player_mix_block(dst, 2, 48000, M, [rh.PlayerSrc(up(srcs[0].x), 2, 44100, M, factors=up(srcs[0].factors).double(), factor_period=441)])
