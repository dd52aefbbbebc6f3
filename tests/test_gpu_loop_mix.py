"""rh_loop_mix_block: a block of a mixer whose sources may be loops (source.repeat_infinite()), each read from ONE resident pass.  Two
references, both bit for bit (uint32 views, no tolerance: everything is integer-indexed or IEEE-exact): tests/loop_mix_ref.py (held against
the oracle by tests/test_loop_mix_cpu.py) and the chain the launch replaces -- rh_amplify, then rh_uniform_row over an unrolled copy on the
device (rule 1: span_len = c * channels over the unrolled stream from the cursor's chain on; rule 0: over one pass, the rows of the passes
back to back), then rh_wide_mix_block over the rows.  Sounds are a handful of frames: that is where seams are dense.  dst lies in a guarded
arena (tests/arena.py); every sound holds exactly its L frames and is followed directly by NaN poison, so a tap at frame L instead of frame
0 poisons the mix; the sounds lie at 4-byte-aligned, not 16-byte-aligned, addresses."""
import ctypes as C

import numpy as np
import pytest

import arena
import loop_mix_ref as R
import player_mix_ref as PR
import stream_gate
import wide_positions as WP

pytestmark = pytest.mark.gpu

RATES = [(44100, 48000), (48000, 44100), (48000, 48000), (8000, 48000)]
LAYOUTS = [(1, 2), (2, 2), (2, 1), (6, 2), (2, 6)]
GRID = [(r, t, c, tc) for r, t in RATES for c, tc in LAYOUTS]
# (L, c, rule): every output frame verbatim; one chain a pass; chains 4, 4, 2; a tail chain of ONE frame; the grid meets the seam every time;
# drifts by one frame a chain; 4 against 10
SHAPES = [(1, 1, 0), (5, 5, 0), (10, 4, 0), (9, 4, 0), (4, 4, 1), (5, 4, 1), (10, 4, 1)]
GAINS = [0.7, -1.1, 1.0, 0.5, -0.3, 1.9, -0.25]
LIVE = PR.LIVE
INVALID, UNSUPPORTED = 1, 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sound(rng, n):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if n > 8:  # zeros of both signs among the samples
        z = rng.integers(0, n, 4)
        x[z[:2]], x[z[2:]] = 0.0, -0.0
    return x


def loop(rng, L, c, rule, ch, rate, to_rate, frames, gain, played=0):
    """A loop that has been playing for `played` output frames."""
    return R.Src(sound(rng, L * ch), ch, rate, frames, gain=gain, words=R.loop_advance([L, c, rule, 0, 0], rate, to_rate, played))


class Dev:
    """A source's samples on the device: a row of an arena of its own, `lead` floats behind a 16-byte boundary, between NaN."""

    def __init__(self, s, lead=1):
        self.arena = arena.src_arena(s.x, lead) if s.x.size else None
        self.ptr = self.arena.ptr() if self.arena else None

    def unchanged(self):
        if self.arena:
            self.arena.unchanged()


def loop_srcs(rh, srcs, devs):
    return [rh.LoopSrc(d.ptr, s.ch, s.from_rate, s.frames, gain=float(s.gain), words=s.words, phase=s.phase, last=s.last) for s, d in zip(srcs, devs)]


def run_new(rh, srcs, devs, to_rate, M, ch=2, lead=0):
    """The entry into a guarded dst `lead` floats behind a 16-byte boundary: nothing stored outside, every word written."""
    dst = arena.dst_arena(M * ch, lead)
    rh.loop_mix_block(dst.ptr(), ch, to_rate, M, loop_srcs(rh, srcs, devs))
    return dst.check()


def run_chain(rh, srcs, to_rate, M, ch=2):
    """Per source rh_amplify and rh_uniform_row over an unrolled copy into a row of the mixer's layout and rate, then rh_wide_mix_block over
    the rows (gain 1, one rate: its converter passes through)."""
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
        F, T = R.reduced(s.from_rate, to_rate)
        if s.words is None:  # a plain source: its Amplify into a row, the rest is rh_wide_mix_block's
            row = torch.from_numpy(s.x).cuda()
            _lib.check(lib.rh_amplify(vp(row.data_ptr()), vp(row.data_ptr()), s.x.size, float(s.gain), st), "rh_amplify")
            keep.append(row)
            arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr(), s.ch, s.from_rate, s.phase, s.last, 1.0
            continue
        L, c, rule, start, out = s.words
        x = s.x.reshape(L, s.ch)
        Mc = R.span_out(c, F, T)
        if rule == 1:  # the unrolled stream from the cursor's chain on, in whole chains
            n_chains = (out + s.frames + Mc - 1) // Mc
            src = x[(start + np.arange(n_chains * c)) % L]
            skip, passes = out, 1
        else:  # one pass; its row repeats
            src = x
            P = sum(R.span_out(n, F, T) for _, n in R.chains_of_pass(L, c))
            skip = (start // c) * Mc + out
            passes = (skip + s.frames + P - 1) // P
        src = torch.from_numpy(np.ascontiguousarray(src).reshape(-1)).cuda()
        _lib.check(lib.rh_amplify(vp(src.data_ptr()), vp(src.data_ptr()), src.numel(), float(s.gain), st), "rh_amplify")
        n_out = C.c_uint64(0)
        _lib.check(lib.rh_uniform_row_out_samples(src.numel(), s.ch, s.from_rate, ch, to_rate, c * s.ch, C.byref(n_out)), "rh_uniform_row_out_samples")
        row = torch.full((n_out.value,), float("nan"), device="cuda")
        got = C.c_uint64(0)
        _lib.check(lib.rh_uniform_row(vp(row.data_ptr()), n_out.value, vp(src.data_ptr()), src.numel(), s.ch, s.from_rate, ch, to_rate, c * s.ch, C.byref(got), st), "rh_uniform_row")
        assert got.value == n_out.value == (n_chains * Mc if rule == 1 else P) * ch
        row = row.repeat(passes)
        assert row.numel() >= (skip + s.frames) * ch
        keep.append(row)
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr() + 4 * skip * ch, ch, to_rate, 0, LIVE, 1.0
    dst = torch.full((M * ch,), float("nan"), device="cuda")
    _lib.check(lib.rh_wide_mix_block(vp(dst.data_ptr()), ch, to_rate, M, arr, len(srcs), st), "rh_wide_mix_block")
    return dst.cpu().numpy()


def hold(rh, srcs, to_rate, M, ch=2, leads=(0, 1), chain=True, src_lead=1):
    """The entry against the restatement (and the chain), dst on and off a 16-byte boundary.  Inputs unchanged.  Returns the restatement."""
    want = R.loop_mix(ch, to_rate, M, srcs)
    assert np.isfinite(want).all()
    devs = [Dev(s, src_lead) for s in srcs]
    for lead in leads:
        got = run_new(rh, srcs, devs, to_rate, M, ch, lead)
        bad = np.flatnonzero(bits(got) != bits(want))
        assert bad.size == 0, f"lead {lead}: {bad.size} sample(s) differ from the restatement, the first at {int(bad[0])} (frame {int(bad[0]) // ch}): {got[bad[0]]!r} != {want[bad[0]]!r}"
    if chain:
        assert np.array_equal(bits(run_chain(rh, srcs, to_rate, M, ch)), bits(want)), "the chain of existing entries differs from the restatement"
    for d in devs:
        d.unchanged()
    return want


# ---- small loops: every shape, rate and layout ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,to_rate,ch,to_ch", GRID)
def test_small_loops_of_both_rules(rh, rate, to_rate, ch, to_ch):
    """The seven shapes in one mixer, fresh and with cursors anywhere, in blocks of 64 .. 300 frames: dozens of passes a block."""
    rng = np.random.default_rng(rate % 89 + 10 * ch + to_ch)
    for M, played in ((64, 0), (300, None), (137, None)):
        srcs = [loop(rng, L, c, rule, ch, rate, to_rate, M, g, int(rng.integers(0, 5000)) if played is None else 0) for (L, c, rule), g in zip(SHAPES, GAINS)]
        hold(rh, srcs, to_rate, M, to_ch)


@pytest.mark.parametrize("L,c,rule", SHAPES)
def test_a_pair_with_t_beyond_2_to_the_24(rh, L, c, rule):
    """100 -> 16 777 259 Hz: (float)num and (float)T round.  A chain of c frames emits hundreds of thousands of frames; the cursor stands 150
    frames in front of a chain's end, so the block crosses it."""
    pair = WP.BY_ID["100-16777259"]
    assert pair.T > 1 << 24
    rng = np.random.default_rng(L)
    F, T = pair.F, pair.T
    M = 300
    first = R.span_out(min(c, L), F, T)  # the first chain of a fresh loop
    played = (first if first > 150 else 3 * first + 150) - 150
    srcs = [loop(rng, L, c, rule, ch, pair.from_rate, pair.to_rate, M, g, played + 7 * k) for k, (ch, g) in enumerate(((2, -0.8), (1, 1.3)))]
    assert srcs[0].words[4] + M > R.span_out(c if rule == 1 else min(c, L - srcs[0].words[3]), F, T) or L == 1
    hold(rh, srcs, pair.to_rate, M, 2)


def test_negative_gains_and_minus_zero_on_silence(rh):
    """Negative gains, and a gain of -0.0 on an all-zero loop: every term is -0.0 and the sum, which starts at +0.0, stays +0.0."""
    rng = np.random.default_rng(2)
    M = 200
    srcs = [loop(rng, 10, 4, k % 2, 2, 44100, 48000, M, g, 33) for k, g in enumerate((-1.0, -0.37, -2.5))]
    hold(rh, srcs, 48000, M, 2)
    quiet = [R.Src(np.zeros(20, np.float32), 2, 44100, M, gain=-0.0, words=[10, 4, rule, 0, 0]) for rule in (0, 1)]
    want = hold(rh, quiet, 48000, M, 2)
    assert not bits(want).any()


@pytest.mark.parametrize("span", ["samples_buffer", "none"])
def test_rodio_sized_sounds_in_three_blocks(rh, span):
    """20 000 stereo frames through rh_loop_plan -- as a SamplesBuffer rule 1 with c = 16384, as a None-span source rule 0 with chains of
    16384 + 3616 -- in a block of 70 000 output frames and in three unequal ones with rh_loop_advance's cursor: the same bits."""
    rng = np.random.default_rng(6)
    L, ch, rate, to_rate, M = 20000, 2, 44100, 48000, 70000
    span_len = L * ch if span == "samples_buffer" else 0
    words = rh.loop_plan(L * ch, ch, span_len)
    assert words == R.loop_plan(L * ch, ch, span_len) == [L, 16384, 1 if span_len else 0, 0, 0]
    s = R.Src(sound(rng, L * ch), ch, rate, M, gain=0.8, words=words)
    want = hold(rh, [s], to_rate, M, 2, leads=(0,))
    dev, parts = Dev(s), []
    for n in (17832, 1, M - 17833):  # (the first chain emits 17833 frames under either rule: the second block is its verbatim last frame alone)
        part = R.Src(s.x, ch, rate, n, gain=0.8, words=words)
        parts.append(run_new(rh, [part], [dev], to_rate, n, 2, lead=1))
        assert np.array_equal(bits(parts[-1]), bits(R.loop_mix(2, to_rate, n, [part])))
        words = rh.loop_advance(words, rate, to_rate, n)
        assert words == R.loop_advance(part.words, rate, to_rate, n)
    assert np.array_equal(bits(np.concatenate(parts)), bits(want))
    dev.unchanged()


# ---- loops and plain sources ----------------------------------------------------------------------------------------------------------------
def test_loops_and_plain_sources_interleaved_are_the_oracles_mixer(rh, O):
    """Loops and one-shots (L == 0) in insertion order, a one-shot ending inside the block: the oracle's mixer fed the unrolled loops."""
    from test_loop_mix_cpu import oracle_loop

    rng = np.random.default_rng(12)
    rate, to_rate, ch, M = 44100, 48000, 2, 90
    F, T = R.reduced(rate, to_rate)
    mx, srcs = O.Mixer(2, to_rate), []
    for k, (L, c, rule) in enumerate(SHAPES):
        s = loop(rng, L, c, rule, ch, rate, to_rate, M, GAINS[k])
        mx.add(oracle_loop(O, s.x, ch, rate, s.words, 200 // L + 9).amplify(float(s.gain)))
        srcs.append(s)
        if k % 2 == 0:  # one-shots of 17, 200 (it outlasts the block), 40 and 5 frames
            n = (17, 0, 200, 0, 40, 0, 5)[k]
            y = sound(rng, n * ch)
            mx.add(O.TestSource(y, ch, rate).amplify(0.9))
            srcs.append(R.Src(y, ch, rate, min(M, R.span_out(n, F, T)), gain=0.9, last=n - 1))
    want = mx.pull(M * 2)
    assert want.size == M * 2 and any(s.words is None and 0 < s.frames < M for s in srcs)
    got = hold(rh, srcs, to_rate, M, 2)
    assert np.array_equal(bits(got), bits(want))


def test_without_a_loop_it_is_rh_wide_mix_block(rh):
    """All L == 0: the bits rh_wide_mix_block writes for the same table, sources that end inside the block and a mid-stream phase among them."""
    import torch

    from rodio_amd import _lib, source

    rng = np.random.default_rng(9)
    to_rate, M = 48000, 300
    srcs = []
    for k, (ch, rate, n) in enumerate([(2, 44100, 400), (1, 48000, 120), (6, 8000, 30), (2, 96000, 700), (2, 44100, 90)]):
        F, T = R.reduced(rate, to_rate)
        b = PR.block_of(sound(rng, n * ch), ch, rate, to_rate, 5 * k, 5 * k + M)
        srcs.append(R.Src(b.x, ch, rate, b.frames, gain=0.4 + 0.3 * k, phase=b.phase, last=b.last))
    want = hold(rh, srcs, to_rate, M, 2, chain=False)
    devs = [Dev(s) for s in srcs]
    arr = (_lib.WideSrc * len(srcs))()
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = d.ptr, s.ch, s.from_rate, s.phase, s.frames, s.last, float(s.gain)
    dst = torch.full((M * 2,), float("nan"), device="cuda")
    _lib.check(_lib.lib.rh_wide_mix_block(C.c_void_p(dst.data_ptr()), 2, to_rate, M, arr, len(srcs), source._stream()), "rh_wide_mix_block")
    assert np.array_equal(bits(dst.cpu().numpy()), bits(want))


@pytest.mark.parametrize("S", [33, 40])
def test_more_than_32_sources_continue_from_the_partial_sum(rh, S):
    """Two launches; sources that reach nothing (frames == 0, data NULL) between them do not count, a loop the caller stops inside the block
    (frames < out_frames) is silent behind its frames, and plain sources sit among the loops."""
    rng = np.random.default_rng(S)
    rate, to_rate, M = 44100, 48000, 150
    srcs = []
    for k in range(S):
        L, c, rule = SHAPES[k % len(SHAPES)]
        ch = (2, 1, 6)[k % 3]
        if k % 11 == 5:
            srcs.append(R.Src(np.zeros(0, np.float32), ch, rate, 0, words=[L, c, rule, 0, 0]))
        elif k % 11 == 7:
            srcs.append(R.Src(sound(rng, 400 * ch), ch, rate, M, gain=0.6))
        else:
            srcs.append(loop(rng, L, c, rule, ch, rate, to_rate, M if k % 4 else 40 + k, 0.3 + 0.05 * k, 11 * k))
    live = sum(1 for s in srcs if s.frames)
    assert live > 32 if S == 40 else live <= 32  # (33 entries of which three reach nothing: one launch; 40: two)
    if S == 33:
        srcs += [loop(rng, 5, 4, 1, 2, rate, to_rate, M, -0.5, 3) for _ in range(3)]  # ... and exactly 33 that do: the second launch holds one source
        assert sum(1 for s in srcs if s.frames) == 33
    hold(rh, srcs, to_rate, M, 2)


def test_no_sources_and_no_frames(rh):
    dst = arena.dst_arena(64, 1)
    rh.loop_mix_block(dst.ptr(), 2, 48000, 32, [])
    assert not bits(dst.check()).any()  # n_sources == 0 writes +0.0
    dst = arena.dst_arena(64, 0)
    rh.loop_mix_block(dst.ptr(), 2, 48000, 32, [rh.LoopSrc(None, 2, 44100, 0, words=[10, 4, 0, 0, 0])])
    assert not bits(dst.check()).any()
    dst = arena.dst_arena(64, 0)
    rh.loop_mix_block(dst.ptr(), 2, 48000, 0, [rh.LoopSrc(None, 0, 0, 5, words=[0, 0, 9, 9, 9])])  # out_frames == 0: nothing is looked at
    dst.check(written=0)


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def tables(srcs, devs, host=lambda a, value=None: a):
    from rodio_amd import _lib

    n = max(len(srcs), 1)
    arr, words = host((_lib.WideSrc * n)(), 0), host((C.c_uint64 * (5 * n))(), 0)
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = d.ptr, s.ch, s.from_rate, s.phase, s.frames, s.last, float(s.gain)
        words[5 * k: 5 * k + 5] = s.words or [0] * 5
    return arr, words


def call(dst_ptr, ch, to_rate, M, srcs, devs, tweak=None, null=(), n=None):
    """The raw entry: its status.  tweak(arr, words) edits the tables before the call; null: arrays passed as NULL."""
    from rodio_amd import _lib, source

    source._ensure()
    arr, words = tables(srcs, devs)
    if tweak:
        tweak(arr, words)
    return _lib.lib.rh_loop_mix_block(C.c_void_p(dst_ptr) if dst_ptr else None, ch, to_rate, M, None if "srcs" in null else arr, len(srcs) if n is None else n,
                                      None if "words" in null else words, source._stream())


def test_every_refusal_writes_nothing(rh):
    """Each refusal of rodio_hip.h returns its status and leaves dst as it was (the arena's sentinel in every word).  Source 0 is a plain
    source, 1 a loop under rule 0 (L 10, c 4: chains of 5, 5 and 3 output frames), 2 one under rule 1."""
    rng = np.random.default_rng(8)
    M = 300
    srcs = [R.Src(sound(rng, 800), 2, 44100, M, gain=0.5), loop(rng, 10, 4, 0, 2, 44100, 48000, M, 0.7), loop(rng, 10, 4, 1, 1, 44100, 48000, M, 0.9)]
    devs = [Dev(s) for s in srcs]
    dst = arena.dst_arena(M * 2, 0)

    def refused(status=INVALID, ch=2, to_rate=48000, frames=M, **kw):
        assert call(dst.ptr(), ch, to_rate, frames, srcs, devs, **kw) == status, kw
        dst.check(written=0)

    def field(k, name, value):
        return lambda arr, w: setattr(arr[k], name, value)

    def word(k, i, value, also=None):
        return lambda arr, w: (w.__setitem__(5 * k + i, value), also and also(arr, w))

    assert call(None, 2, 48000, M, srcs, devs) == INVALID
    refused(ch=0)
    refused(to_rate=0)
    refused(null=("srcs",))
    refused(null=("words",))
    # what rh_wide_mix_block refuses of the shared fields, of a loop and of a plain source
    for k in (0, 1):
        refused(tweak=field(k, "data", None))
        refused(tweak=field(k, "channels", 0))
        refused(tweak=field(k, "from_rate", 0))
        refused(tweak=field(k, "frames", M + 1))
        refused(UNSUPPORTED, tweak=field(k, "from_rate", 4294967291))  # F T beyond 32 bits
    refused(tweak=field(0, "phase", 160))
    # the words
    refused(tweak=word(1, 2, 2))                    # a rule above 1
    refused(tweak=word(1, 1, 0))                    # c == 0
    refused(tweak=word(1, 1, 16385))                # c * channels > 32768 (stereo)
    refused(tweak=word(2, 1, 32769, word(2, 0, 40000)))  # ... mono
    refused(tweak=word(2, 1, 11))                   # rule 1 with L < c
    refused(tweak=word(1, 3, 10))                   # chain_start == L
    refused(tweak=word(2, 3, 10))
    refused(tweak=word(1, 3, 5))                    # rule 0: chain_start no multiple of c
    refused(tweak=word(1, 4, 5))                    # chain_out == the chain's output count
    refused(tweak=word(1, 4, 3, word(1, 3, 8)))     # ... the tail chain's
    refused(tweak=word(2, 4, 5))
    # positions beyond 32 bits
    refused(UNSUPPORTED, frames=0x80000000)
    refused(UNSUPPORTED, frames=0x7FFFFFFF)         # the plain source: out_frames > (2^32 - 1 - T) / F
    refused(UNSUPPORTED, tweak=word(2, 0, (1 << 31) + 1))  # L > 2^31
    refused(UNSUPPORTED, to_rate=4294967291, tweak=lambda arr, w: (setattr(arr[0], "frames", 0), setattr(arr[1], "from_rate", 1), setattr(arr[2], "from_rate", 1)))  # M(c) F
    # the cursor's bounds are met by the last valid value
    for tw in (word(1, 4, 4), word(1, 4, 2, word(1, 3, 8)), word(2, 4, 4, word(2, 3, 9))):
        d2 = arena.dst_arena(M * 2, 0)
        assert call(d2.ptr(), 2, 48000, M, srcs, devs, tweak=tw) == 0
        d2.check()
    # a loop's phase and last are not read
    d2 = arena.dst_arena(M * 2, 0)
    assert call(d2.ptr(), 2, 48000, M, srcs, devs, tweak=lambda arr, w: (setattr(arr[1], "phase", 4000000000), setattr(arr[1], "last", 0))) == 0
    assert np.array_equal(bits(d2.check()), bits(R.loop_mix(2, 48000, M, srcs)))
    # out_frames == 0: nothing to do, whatever the rest says
    assert call(dst.ptr(), 0, 0, 0, srcs, devs, null=("srcs", "words")) == 0
    dst.check(written=0)
    assert call(dst.ptr(), 2, 48000, M, srcs, devs) == 0
    assert np.array_equal(bits(dst.check()), bits(R.loop_mix(2, 48000, M, srcs)))


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
    srcs = [loop(rng, *SHAPES[k % len(SHAPES)], (2, 1)[k % 2], 44100, to_rate, M, 0.2 + 0.04 * k, 13 * k) if k % 5 else R.Src(sound(rng, 700), 2, 44100, M, gain=0.5) for k in range(S)]
    want = R.loop_mix(2, to_rate, M, srcs)

    def build(k):
        devs = [Dev(s) for s in srcs]
        for d in devs:
            k.add(d.arena)
        dst = k.dst(M * 2, 0)

        def one():
            arr, words = tables(srcs, devs, k.host)
            _lib.check(_lib.lib.rh_loop_mix_block(C.c_void_p(dst.ptr()), 2, to_rate, M, arr, S, words, source._stream()), "rh_loop_mix_block")

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

    rng = np.random.default_rng(4)
    M = 300
    srcs = [loop(rng, L, c, rule, 2, 44100, 48000, M, g, 77) for (L, c, rule), g in zip(SHAPES, GAINS)]
    dst = torch.full((2 * M,), float("nan"), device="cuda")
    rh.loop_mix_block(dst, 2, 48000, M, [rh.LoopSrc(torch.from_numpy(s.x).cuda(), 2, 44100, M, gain=float(s.gain), words=s.words) for s in srcs])
    assert np.array_equal(bits(dst.cpu().numpy()), bits(R.loop_mix(2, 48000, M, srcs)))
    for n, ch, span_len in [(20000, 2, 0), (40000, 2, 0), (40000, 2, 40000), (88200, 2, 88200), (40000, 2, 1152), (1000, 2, 1152), (30000, 6, 0)]:
        assert rh.loop_plan(n, ch, span_len) == R.loop_plan(n, ch, span_len)
    for n, ch, span_len in [(60000, 6, 0), (60000, 3, 60000), (39999, 2, 0), (40000, 2, 50000), (40000, 2, 1001)]:
        assert R.loop_plan(n, ch, span_len) == R.UNSUPPORTED
        with pytest.raises(rh.RhError):
            rh.loop_plan(n, ch, span_len)
    for (L, c, rule), (rate, to_rate) in zip(SHAPES, RATES + RATES):
        w = [L, c, rule, 0, 0]
        for n in (1, 63, 0, 4097):
            assert rh.loop_advance(w, rate, to_rate, n) == R.loop_advance(w, rate, to_rate, n)
            w = R.loop_advance(w, rate, to_rate, n)
    with pytest.raises(ValueError):
        rh.LoopSrc(None, 2, 44100, M, words=[1, 2, 3])
