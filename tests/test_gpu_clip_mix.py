"""rh_clip_mix_block: a block of a mixer whose sources may be clips on a timeline -- sound.amplify(g).take_duration(len)[.set_filter_fadeout()]
.delay(at) over a resident sound.  Two references, both bit for bit (uint32 views; NaN positions where a duration under a millisecond makes
x * 0 / 0): tests/clip_mix_ref.py (held against the oracle by tests/test_clip_mix_cpu.py, whose CASES run here) and the chain the launch
replaces -- rh_amplify, rh_take_duration (fade_out), rh_delay into one row of Z + N samples, rh_uniform_row over the row (span_len = its
length under rule G, 0 under rule C), then rh_wide_mix_block over the rows.  dst lies in a guarded arena (tests/arena.py); every sound holds
exactly its N admitted samples and is followed directly by NaN poison, so a tap behind the take poisons the mix; the sounds lie at
4-byte-aligned, not 16-byte-aligned, addresses."""
import ctypes as C

import numpy as np
import pytest

import arena
import clip_mix_ref as R
import player_mix_ref as PR
import stream_gate
from test_clip_mix_cpu import CASES, IDS, Case, bits, same

pytestmark = pytest.mark.gpu

LIVE = PR.LIVE
INVALID, UNSUPPORTED = 1, 3
W = 7  # RH_CLIP_WORDS
BY = {c.name: c for c in CASES}
M_CHAIN = 17833  # output frames of a whole chain, stereo 44.1 -> 48 kHz: rh_uniform_span_frames(16384, ..)


def sound(rng, n):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if n > 8:
        z = rng.integers(0, n, 4)
        x[z[:2]], x[z[2:]] = 0.0, -0.0
    return x


class Dev:
    """A source's samples on the device: a row of an arena of its own, `lead` floats behind a 16-byte boundary, between NaN.  A clip holds
    its N admitted samples and no more (an empty one: a single NaN that nothing may read)."""

    def __init__(self, s, lead=1):
        x = s.x if s.words is None else s.x[: s.words[2]]
        self.arena = arena.src_arena(x if x.size else np.full(1, np.nan, np.float32), lead) if (x.size or s.words is not None) else None
        self.ptr = self.arena.ptr() if self.arena else None

    def unchanged(self):
        if self.arena:
            self.arena.unchanged()


def clip_srcs(rh, srcs, devs):
    return [rh.ClipSrc(d.ptr, s.ch, s.from_rate, s.frames, gain=float(s.gain), words=s.words, phase=s.phase, last=s.last) for s, d in zip(srcs, devs)]


def run_new(rh, srcs, devs, to_rate, M, ch=2, lead=0):
    """The entry into a guarded dst `lead` floats behind a 16-byte boundary: nothing stored outside, every word written."""
    dst = arena.dst_arena(M * ch, lead)
    rh.clip_mix_block(dst.ptr(), ch, to_rate, M, clip_srcs(rh, srcs, devs))
    return dst.check()


def run_chain(rh, srcs, to_rate, M, ch=2):
    """Per clip rh_amplify, rh_take_duration, rh_delay into one row of Z + N samples and rh_uniform_row over it into a row of the mixer's
    layout and rate, then rh_wide_mix_block over the rows (gain 1, one rate: its converter passes through)."""
    import torch

    from rodio_amd import _lib, source

    source._ensure()
    lib, st, vp = _lib.lib, source._stream(), C.c_void_p
    arr = (_lib.WideSrc * max(len(srcs), 1))()
    keep = []
    for k, s in enumerate(srcs):
        arr[k].frames = s.frames
        if s.frames == 0:
            continue
        if s.words is None:  # a plain source: its Amplify into a row, the rest is rh_wide_mix_block's
            row = torch.from_numpy(s.x).cuda()
            _lib.check(lib.rh_amplify(vp(row.data_ptr()), vp(row.data_ptr()), s.x.size, float(s.gain), st), "rh_amplify")
            keep.append(row)
            arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr(), s.ch, s.from_rate, s.phase, s.last, 1.0
            continue
        kind, Z, N, take_ns, flags, done, _ = s.words
        x = torch.from_numpy(np.ascontiguousarray(s.x[:N] if N else np.zeros(1, np.float32))).cuda()
        _lib.check(lib.rh_amplify(vp(x.data_ptr()), vp(x.data_ptr()), N, float(s.gain), st), "rh_amplify")
        if flags & R.TAKE:
            taken = torch.full((N + s.ch,), float("nan"), device="cuda")
            n_out, ended = C.c_uint64(0), C.c_int32(0)
            _lib.check(lib.rh_take_duration(vp(taken.data_ptr()), vp(x.data_ptr()), N, 0, s.ch, s.from_rate, take_ns, 1 if flags & R.FADE else 0, C.byref(n_out), C.byref(ended), st),
                       "rh_take_duration")
            assert N <= n_out.value < N + s.ch  # (behind the N samples: the silence that completes a cut frame, which the last chain never draws)
            x = taken
        row_in = torch.full((Z + N + 1,), float("nan"), device="cuda")
        _lib.check(lib.rh_delay(vp(row_in.data_ptr()), vp(x.data_ptr()), N, Z, st), "rh_delay")
        span_len = Z + N if kind == R.RULE_G else 0
        n_out = C.c_uint64(0)
        _lib.check(lib.rh_uniform_row_out_samples(Z + N, s.ch, s.from_rate, ch, to_rate, span_len, C.byref(n_out)), "rh_uniform_row_out_samples")
        total = R.clip_out_frames(s.words, s.ch, s.from_rate, to_rate)
        assert n_out.value == total * ch
        row = torch.full((n_out.value + 1,), float("nan"), device="cuda")
        got = C.c_uint64(0)
        _lib.check(lib.rh_uniform_row(vp(row.data_ptr()), n_out.value, vp(row_in.data_ptr()), Z + N, s.ch, s.from_rate, ch, to_rate, span_len, C.byref(got), st), "rh_uniform_row")
        assert got.value == n_out.value and done + s.frames <= total
        keep += [x, row_in, row]
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr() + 4 * done * ch, ch, to_rate, 0, LIVE, 1.0
    dst = torch.full((M * ch,), float("nan"), device="cuda")
    _lib.check(lib.rh_wide_mix_block(vp(dst.data_ptr()), ch, to_rate, M, arr, len(srcs), st), "rh_wide_mix_block")
    return dst.cpu().numpy()


def differ(got, want, ch, what):
    if same(got, want):
        return
    nan = np.isnan(want)
    bad = np.flatnonzero((np.isnan(got) != nan) | ((bits(got) != bits(want)) & ~nan))
    raise AssertionError(f"{what}: {bad.size} sample(s) differ, the first at {int(bad[0])} (frame {int(bad[0]) // ch}): {got[bad[0]]!r} != {want[bad[0]]!r}")


def hold(rh, srcs, to_rate, M, ch=2, leads=(0, 1), chain=True, src_lead=1, devs=None):
    """The entry against the restatement (and the chain), dst on and off a 16-byte boundary.  Inputs unchanged.  Returns the restatement."""
    want = R.clip_mix(ch, to_rate, M, srcs)
    devs = [Dev(s, src_lead) for s in srcs] if devs is None else devs
    for lead in leads:
        differ(run_new(rh, srcs, devs, to_rate, M, ch, lead), want, ch, f"the entry, lead {lead}, against the restatement")
    if chain:
        differ(run_chain(rh, srcs, to_rate, M, ch), want, ch, "the chain of existing entries against the restatement")
    for d in devs:
        d.unchanged()
    return want


# ---- the case list: every clip whole, in one block ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_a_whole_clip_in_one_block(rh, case):
    s = case.src()
    assert rh.clip_plan(case.x.size, case.ch, case.rate, case.span_len, case.delay_ns, case.take_ns, case.fade) == case.words()
    M = s.frames + 3  # the clip ends inside the block: silence behind it
    want = hold(rh, [s], case.to_rate, M, case.to_ch)
    assert not bits(want[s.frames * case.to_ch:]).any()


def mixed(rng, names, M, to_rate=48000, every=1):
    """The named cases as clips with cursors anywhere (every third one fresh), a plain source behind every `every`-th: the sources."""
    srcs = []
    for k, name in enumerate(names):
        c = BY[name]
        assert c.to_rate == to_rate
        total = R.clip_out_frames(c.words(), c.ch, c.rate, to_rate)
        done = int(rng.integers(0, max(total - 1, 1))) if k % 3 else 0
        srcs.append(c.src(min(M, total - done), done))
        if k % every == 0:
            ch, rate, n = (2, 1)[k % 2], (44100, 48000, 96000)[k % 3], M + 40
            b = PR.block_of(sound(rng, 3 * n * ch), ch, rate, to_rate, 5 * k, 5 * k + M)
            srcs.append(R.Src(b.x, ch, rate, b.frames, gain=0.4 + 0.03 * k, phase=b.phase, last=b.last))
    return srcs


STEREO_48 = [c.name for c in CASES if (c.to_ch, c.to_rate) == (2, 48000) and R.clip_out_frames(c.words(), c.ch, c.rate, 48000) > 0]


@pytest.mark.parametrize("S", [33, 65])
def test_clips_and_plain_sources_alternating_across_the_launch_table(rh, S):
    """Clip, plain, clip, plain ...: 33 sources are two launches, 65 three; later launches continue from the stored sum.  Clips that end inside
    the block, clips still in their delay and clips in mid-fade among them."""
    rng = np.random.default_rng(S)
    M = 300
    names = [STEREO_48[k % len(STEREO_48)] for k in range((S + 1) // 2)]
    srcs = mixed(rng, names, M)[:S]
    assert len(srcs) == S and sum(1 for s in srcs if s.words) >= S // 2 and all(s.frames for s in srcs)
    assert any(s.words and s.frames < M for s in srcs) and any(s.words and s.words[1] > (s.words[5] + M) * 2 for s in srcs)
    hold(rh, srcs, 48000, M, 2)


@pytest.mark.parametrize("M", [1, 7, 1024, 40000])
def test_blocks_of_several_sizes(rh, M):
    rng = np.random.default_rng(M)
    names = ["take expiring in a later chain, fading across grid lines", "rule C across grid lines: ONE chain", "a short SamplesBuffer pushed across a grid line",
             "odd delay beyond two grid lines", "mono into stereo", "six into stereo, one chain", "an in-point, rule G"]
    srcs = mixed(rng, names, M, every=3)
    hold(rh, srcs, 48000, M, 2)


@pytest.mark.parametrize("name", ["take expiring in a later chain, fading across grid lines", "rule C across grid lines: ONE chain", "odd delay beyond two grid lines",
                                  "the sound ends before the take, in the second chain", "48 -> 44.1 kHz", "T near 2^16"])
def test_a_stream_cut_at_random_points_is_the_one_pass(rh, name):
    c = BY[name]
    rng = np.random.default_rng(len(name))
    whole = c.src()
    want = R.clip_mix(c.to_ch, c.to_rate, whole.frames, [whole])
    dev = Dev(whole)
    cuts = sorted({int(v) for v in rng.integers(0, whole.frames + 1, 5)})
    words = rh.clip_advance(rh.clip_plan(c.x.size, c.ch, c.rate, c.span_len, c.delay_ns, c.take_ns, c.fade), c.ch, c.rate, c.to_rate, 0)
    assert words == whole.words
    parts = []
    for m0, m1 in zip([0] + cuts, cuts + [whole.frames]):
        assert words[5] == m0
        if m1 > m0:
            part = R.Src(c.x, c.ch, c.rate, m1 - m0, gain=c.gain, words=words)
            parts.append(run_new(rh, [part], [dev], c.to_rate, m1 - m0, c.to_ch, lead=m0 % 2))
        before, words = words, rh.clip_advance(words, c.ch, c.rate, c.to_rate, m1 - m0)
        assert words == R.clip_advance(before, c.ch, c.rate, c.to_rate, m1 - m0)
    assert words[5] == words[6] == whole.frames
    differ(np.concatenate(parts), want, c.to_ch, "the cut stream against the one pass")
    dev.unchanged()


def test_blocks_that_start_and_end_on_a_grid_line(rh):
    """Stereo 44.1 -> 48 kHz: a whole chain emits 17833 frames, the last of them verbatim.  A block that ends with that frame, one that starts
    behind it, and one frame either side."""
    c = BY["take expiring in a later chain, fading across grid lines"]
    assert R.span_out(16384, 147, 160) == M_CHAIN
    for done, frames in [(M_CHAIN - 200, 200), (M_CHAIN, 200), (M_CHAIN - 1, 1), (M_CHAIN, 1), (M_CHAIN - 100, 200), (2 * M_CHAIN - 50, 50), (2 * M_CHAIN, 64)]:
        hold(rh, [c.src(frames, done)], 48000, frames, 2, leads=(1,))


def test_a_clip_that_ends_inside_the_block_and_one_still_in_its_delay(rh):
    rng = np.random.default_rng(5)
    M = 500
    ending = BY["take expiring in the first chain"]
    total = R.clip_out_frames(ending.words(), 2, 44100, 48000)
    waiting = BY["odd delay beyond two grid lines"]  # 70001 zeros: 38096 output frames of delay
    plain = R.Src(sound(rng, 2000), 2, 44100, M, gain=0.5)
    srcs = [ending.src(200, total - 200), plain, waiting.src(M, 1000), waiting.src(M, 2 * M_CHAIN - 250)]
    want = hold(rh, srcs, 48000, M, 2)
    assert np.array_equal(bits(want), bits(R.clip_mix(2, 48000, M, srcs[:2])))  # the clips in their delay add +0.0: nothing
    # ... whatever their gain is: rodio's zeros are not multiplied
    hot = waiting.src(M, 1000)
    hot.gain = np.float32("nan")
    differ(run_new(rh, [plain, hot], [Dev(plain), Dev(hot)], 48000, M), R.clip_mix(2, 48000, M, [plain]), 2, "a NaN gain on a clip in its delay")


def test_no_sources_and_no_frames(rh):
    dst = arena.dst_arena(64, 1)
    rh.clip_mix_block(dst.ptr(), 2, 48000, 32, [])
    assert not bits(dst.check()).any()  # n_sources == 0 writes +0.0
    dst = arena.dst_arena(64, 0)
    rh.clip_mix_block(dst.ptr(), 2, 48000, 32, [rh.ClipSrc(None, 2, 44100, 0, words=[1, 10, 10, 0, 0, 0, 0])])
    assert not bits(dst.check()).any()
    dst = arena.dst_arena(64, 0)
    rh.clip_mix_block(dst.ptr(), 2, 48000, 0, [rh.ClipSrc(None, 0, 0, 5, words=[9, 9, 9, 9, 9, 9, 9])])  # out_frames == 0: nothing is looked at
    dst.check(written=0)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def tables(srcs, devs, host=lambda a, value=None: a):
    from rodio_amd import _lib

    n = max(len(srcs), 1)
    arr, words = host((_lib.WideSrc * n)(), 0), host((C.c_uint64 * (W * n))(), 0)
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = d.ptr, s.ch, s.from_rate, s.phase, s.frames, s.last, float(s.gain)
        words[W * k: W * k + W] = s.words or [0] * W
    return arr, words


def call(dst_ptr, ch, to_rate, M, srcs, devs, tweak=None, null=(), n=None):
    """The raw entry: its status.  tweak(arr, words) edits the tables before the call; null: arrays passed as NULL."""
    from rodio_amd import _lib, source

    source._ensure()
    arr, words = tables(srcs, devs)
    if tweak:
        tweak(arr, words)
    return _lib.lib.rh_clip_mix_block(C.c_void_p(dst_ptr) if dst_ptr else None, ch, to_rate, M, None if "srcs" in null else arr, len(srcs) if n is None else n,
                                      None if "words" in null else words, source._stream())


def test_every_refusal_writes_nothing(rh):
    """Each refusal of rodio_hip.h returns its status and leaves dst as it was (the arena's sentinel in every word).  Source 0 is a plain
    source, 1 a fading clip under rule G (Z 1000, N 3000: 2000 frames, 2177 output frames), 2 a clip under rule C (Z 1000, N 6000: 3810)."""
    rng = np.random.default_rng(8)
    M = 300
    g = Case("refusals, rule G", 6000, 1000, take=3000, fade=True)
    c = Case("refusals, rule C", 6000, 1000, kind="test")
    srcs = [R.Src(sound(rng, 800), 2, 44100, M, gain=0.5), g.src(M, 100), c.src(M, 100)]
    devs = [Dev(s) for s in srcs]
    dst = arena.dst_arena(M * 2, 0)

    def refused(status=INVALID, ch=2, to_rate=48000, frames=M, **kw):
        assert call(dst.ptr(), ch, to_rate, frames, srcs, devs, **kw) == status, kw
        dst.check(written=0)

    def field(k, name, value):
        return lambda arr, w: setattr(arr[k], name, value)

    def word(k, i, value, also=None):
        return lambda arr, w: (w.__setitem__(W * k + i, value), also and also(arr, w))

    assert call(None, 2, 48000, M, srcs, devs) == INVALID
    refused(ch=0)
    refused(to_rate=0)
    refused(null=("srcs",))
    refused(null=("words",))  # clips_host == NULL with clips present
    # what rh_wide_mix_block refuses of the shared fields, of a plain source and of a clip
    for k in (0, 1, 2):
        refused(tweak=field(k, "data", None))
        refused(tweak=field(k, "channels", 0))
        refused(tweak=field(k, "from_rate", 0))
        refused(tweak=field(k, "frames", M + 1))
        refused(UNSUPPORTED, tweak=field(k, "from_rate", 4294967291))  # F T beyond 32 bits
    refused(tweak=field(0, "phase", 160))
    # words out of bounds
    refused(tweak=word(1, 0, 3))                     # a kind above 2
    refused(tweak=word(1, 4, 4))                     # flags above 3
    refused(tweak=word(1, 4, 2))                     # the fade-out without a take
    refused(tweak=word(2, 4, 2))
    refused(tweak=word(1, 0, 2))                     # rule C with a take
    refused(tweak=word(1, 2, 3002, word(1, 1, 1002)))  # more samples than the duration admits
    refused(tweak=word(1, 5, 2178))                  # done > total
    refused(tweak=word(1, 5, 2000))                  # frames > total - done
    refused(tweak=word(2, 5, 3700))
    # a chain that would end inside a frame
    refused(UNSUPPORTED, tweak=word(1, 1, 1001))     # (Z + N) mod ch != 0
    refused(UNSUPPORTED, tweak=word(2, 2, 5999))
    refused(UNSUPPORTED, tweak=word(1, 1, 60000, field(1, "channels", 6)))  # Z + N > 32768 with 6 channels under rule G
    # positions beyond 32 bits
    refused(UNSUPPORTED, frames=0x80000000)
    refused(UNSUPPORTED, frames=0x7FFFFFFF)          # the plain source: out_frames > (2^32 - 1 - T) / F
    refused(UNSUPPORTED, to_rate=4294967291, tweak=lambda arr, w: (setattr(arr[0], "frames", 0), setattr(arr[1], "from_rate", 1), setattr(arr[2], "frames", 0),
                                                                   w.__setitem__(W + 1, 40000), w.__setitem__(W + 3, 10**18)))  # M F of rule G
    refused(UNSUPPORTED, tweak=word(2, 1, (1 << 62) + 2))
    # the bounds are met by the last valid value: done + frames == total
    for tw in (word(1, 5, 2177 - M), word(2, 5, 3810 - M)):
        d2 = arena.dst_arena(M * 2, 0)
        assert call(d2.ptr(), 2, 48000, M, srcs, devs, tweak=tw) == 0
        d2.check()
    # a clip's phase and last are not read, nor its word 6
    d2 = arena.dst_arena(M * 2, 0)
    assert call(d2.ptr(), 2, 48000, M, srcs, devs, tweak=lambda arr, w: (setattr(arr[1], "phase", 4000000000), setattr(arr[1], "last", 0), w.__setitem__(W + 6, 5))) == 0
    assert np.array_equal(bits(d2.check()), bits(R.clip_mix(2, 48000, M, srcs)))
    # out_frames == 0: nothing to do, whatever the rest says
    assert call(dst.ptr(), 0, 0, 0, srcs, devs, null=("srcs", "words")) == 0
    dst.check(written=0)
    assert call(dst.ptr(), 2, 48000, M, srcs, devs) == 0
    assert np.array_equal(bits(dst.check()), bits(R.clip_mix(2, 48000, M, srcs)))
    for d in devs:
        d.unchanged()


# ---- a side stream --------------------------------------------------------------------------------------------------------------------------
def test_behind_a_gate_on_a_side_stream(rh):
    """Every launch of the call goes to the stream it is given (tests/stream_gate.py): 33 sources -- two launches, the second continuing the
    stored sum -- queued behind a gate on a side stream while their inputs still hold garbage, both host tables overwritten as soon as the
    call has returned.  The call returns while the gate is pending, and the snapshot holds the restatement's bits.  The side stream is one
    of rh_stream_create, as in tests/test_gpu_player_mix.py (whose reasons hold here)."""
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
    from test_gpu_player_mix import DelayOn

    delay = DelayOn(side)
    rng = np.random.default_rng(0)
    M, S, to_rate = 300, 33, 48000
    srcs = mixed(rng, [STEREO_48[k % len(STEREO_48)] for k in range(17)], M)[:S]
    assert len(srcs) == S
    want = R.clip_mix(2, to_rate, M, srcs)

    def build(k):
        devs = [Dev(s) for s in srcs]
        for d in devs:
            k.add(d.arena)
        dst = k.dst(M * 2, 0)

        def one():
            arr, words = tables(srcs, devs, k.host)
            _lib.check(_lib.lib.rh_clip_mix_block(C.c_void_p(dst.ptr()), 2, to_rate, M, arr, S, words, source._stream()), "rh_clip_mix_block")

        def check():
            assert arena.same(dst.check_snapshot(), want)
            for d in devs:
                d.arena.snapshot_unchanged()

        return stream_gate.case([one], check)

    r = stream_gate.run(build, side, delay, 63.0)  # (ms: test_gpu_player_mix.py's gate)
    assert all(r.pending), ("the call waited for the stream, or the gate is too short", r.pending, r.host_ms)
    r.check()


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_takes_tensors_and_the_helpers_are_the_restatements(rh):
    import torch

    M = 300
    cases = [BY[n] for n in STEREO_48[:8]]
    srcs = [c.src(min(M, c.src().frames)) for c in cases]
    dst = torch.full((2 * M,), float("nan"), device="cuda")
    rh.clip_mix_block(dst, 2, 48000, M, [rh.ClipSrc(torch.from_numpy(np.ascontiguousarray(s.x)).cuda(), s.ch, s.from_rate, s.frames, gain=float(s.gain), words=s.words) for s in srcs])
    assert np.array_equal(bits(dst.cpu().numpy()), bits(R.clip_mix(2, 48000, M, srcs)))
    for c in CASES:
        w = rh.clip_plan(c.x.size, c.ch, c.rate, c.span_len, c.delay_ns, c.take_ns, c.fade)
        assert w == c.words()
        for n in (0, 63, 4097, 10**7):
            assert rh.clip_advance(w, c.ch, c.rate, c.to_rate, n) == R.clip_advance(w, c.ch, c.rate, c.to_rate, n)
            w = R.clip_advance(w, c.ch, c.rate, c.to_rate, n)
    for n, ch, span_len, delay_ns, take_ns, fade in [(40000, 2, 1152, 0, None, False), (4001, 2, 4001, 0, None, False), (60000, 6, 60000, 0, None, False), (4000, 2, 0, 0, None, True)]:
        assert R.clip_plan(n, ch, 44100, span_len, delay_ns, take_ns, fade) in (R.UNSUPPORTED, R.INVALID)
        with pytest.raises(rh.RhError):
            rh.clip_plan(n, ch, 44100, span_len, delay_ns, take_ns, fade)
    with pytest.raises(ValueError):
        rh.ClipSrc(None, 2, 44100, M, words=[1, 2, 3])
