"""rh_queue_mix_block: a block of a mixer whose sources may be queues of resident sounds played back to back.  Two references, both bit for
bit (uint32 views, no tolerance: everything is integer-indexed or IEEE-exact): tests/queue_mix_ref.py (held against the oracle by
tests/test_queue_mix_cpu.py) and the chain of entries the launch replaces -- rh_amplify per sound into one concatenated row (zeros behind it
for a keep-alive tail), rh_uniform_row per converter chain over its slice with the chain's format, the rows back to back, rh_wide_mix_block
over the rows with gain 1 at the mix's rate.  Sounds are a handful of frames: that is where seams are dense; the one exception is a sound of
32776 samples, the smallest that makes a chain cross a seam.  dst lies in a guarded arena (tests/arena.py); every sound lies at a
4-byte-aligned, not 16-byte-aligned, address and is followed directly by NaN poison, so a tap one sample past a piece poisons the mix."""
import ctypes as C

import numpy as np
import pytest

import arena
import player_mix_ref as PR
import queue_mix_ref as R
import stream_gate

pytestmark = pytest.mark.gpu

RATES = [(44100, 48000), (48000, 44100), (48000, 48000), (8000, 48000)]
LAYOUTS = [(1, 2), (2, 2), (2, 1), (6, 2), (2, 6)]
GRID = [(r, t, c, tc) for r, t in RATES for c, tc in LAYOUTS]
GAINS = [0.7, -1.1, 1.0, 0.5, -0.3, 1.9, -0.25]
LIVE = PR.LIVE
INVALID, UNSUPPORTED = 1, 3
FORMATS = [(1, 48000), (2, 44100), (1, 44100), (2, 22050), (6, 8000), (2, 96000), (1, 8000)]


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def sound(rng, n, ch, rate, gain=1.0):
    x = rng.uniform(-1, 1, n).astype(np.float32)
    if n > 8:  # zeros of both signs among the samples
        z = rng.integers(0, n, 4)
        x[z[:2]], x[z[2:]] = 0.0, -0.0
    return R.Sound(x, ch, rate, gain)


def abc(rng):
    """A = 32776 samples stereo at 44.1 kHz, B = 6 mono at 8 kHz, C = 10 stereo at 22.05 kHz: the second chain starts at sample 32768 of A and
    reads B and C as stereo frames at 44.1 kHz."""
    return [sound(rng, 32776, 2, 44100, 0.8), sound(rng, 6, 1, 8000, -1.25), sound(rng, 10, 2, 22050, 0.5)]


def tiny_queue(rng, n_sounds, first=0):
    """1 to 5 tiny sounds of mixed formats, every length a whole number of frames of every format a chain could read it in (multiples of 6)."""
    return [sound(rng, 6 * int(rng.integers(1, 4)), *FORMATS[(first + k) % len(FORMATS)], GAINS[(first + k) % len(GAINS)]) for k in range(n_sounds)]


def queue(frames, sounds, keep=True, played=0, to_rate=48000):
    """A queue that has been playing for `played` output frames: the sounds still listed and the cursor."""
    played = min(played, R.stream_frames(sounds, keep, to_rate) - 1)  # (its last chain at least is still to play)
    words, dropped = R.queue_advance([0, 0, 0, 1 if keep else 0], sounds, to_rate, played)
    return R.Src(frames, sounds[dropped:], words)


def plain(rng, ch, rate, to_rate, m0, M, n, gain):
    b = PR.block_of(rng.uniform(-1, 1, n * ch).astype(np.float32), ch, rate, to_rate, m0, m0 + M)
    return R.Src(b.frames, x=b.x, ch=ch, from_rate=rate, gain=gain, phase=b.phase, last=b.last)


class Dev:
    """A source's samples on the device: every sound (or the plain source's row) in an arena of its own, `lead` floats behind a 16-byte
    boundary, between NaN."""

    def __init__(self, s, lead=1):
        rows = [q.x for q in s.sounds] if s.sounds else [s.x]
        self.arenas = [arena.src_arena(x, lead) if x.size else None for x in rows]

    def ptr(self, k=0):
        return self.arenas[k].ptr() if self.arenas[k] else None

    def unchanged(self):
        for a in self.arenas:
            if a:
                a.unchanged()


def queue_srcs(rh, srcs, devs):
    out = []
    for s, d in zip(srcs, devs):
        if s.sounds:
            out.append(rh.QueueSrc(s.frames, [rh.QueueSound(d.ptr(k), q.ch, q.rate, float(q.gain), samples=q.samples) for k, q in enumerate(s.sounds)], s.words))
        else:
            out.append(rh.QueueSrc(s.frames, data=d.ptr(), channels=s.ch, from_rate=s.from_rate, gain=float(s.gain), phase=s.phase, last=s.last))
    return out


def run_new(rh, srcs, devs, to_rate, M, ch=2, lead=0):
    """The entry into a guarded dst `lead` floats behind a 16-byte boundary: nothing stored outside, every word written."""
    dst = arena.dst_arena(M * ch, lead)
    rh.queue_mix_block(dst.ptr(), ch, to_rate, M, queue_srcs(rh, srcs, devs))
    return dst.check()


def run_chain(rh, srcs, to_rate, M, ch=2):
    """Per queue: rh_amplify per sound into one concatenated row (32768 zeros behind it: a keep-alive chain reads on into them),
    rh_uniform_row per converter chain over its slice, the rows back to back; then rh_wide_mix_block over the rows (gain 1, one rate: its
    converter passes through)."""
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
        if not s.sounds:  # a plain source: its Amplify into a row, the rest is rh_wide_mix_block's
            row = torch.from_numpy(s.x).cuda()
            _lib.check(lib.rh_amplify(vp(row.data_ptr()), vp(row.data_ptr()), s.x.size, float(s.gain), st), "rh_amplify")
            keep.append(row)
            arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr(), s.ch, s.from_rate, s.phase, s.last, 1.0
            continue
        at = np.concatenate([[0], np.cumsum([q.samples for q in s.sounds])]).astype(np.int64)
        cat = torch.zeros(int(at[-1]) + R.CHAIN_SAMPLES, device="cuda")
        for q, a in zip(s.sounds, at):
            if q.samples:
                x = torch.from_numpy(q.x).cuda()
                _lib.check(lib.rh_amplify(vp(cat.data_ptr() + 4 * int(a)), vp(x.data_ptr()), q.samples, float(q.gain), st), "rh_amplify")
                keep.append(x)
        segs = R.walk(s.sounds, s.words, to_rate, s.frames)[0]
        arr[k].frames = sum(cnt for _, _, cnt, _ in segs)  # (behind its last chain the queue adds nothing)
        if not segs:
            continue
        rows = []
        for c, _, _, _ in segs:
            n_out = C.c_uint64(0)
            _lib.check(lib.rh_uniform_row_out_samples(c.n, c.ch, c.rate, ch, to_rate, c.n, C.byref(n_out)), "rh_uniform_row_out_samples")
            row = torch.full((n_out.value,), float("nan"), device="cuda")
            got = C.c_uint64(0)
            _lib.check(lib.rh_uniform_row(vp(row.data_ptr()), n_out.value, vp(cat.data_ptr() + 4 * int(at[c.k] + c.off)), c.n, c.ch, c.rate, ch, to_rate, c.n, C.byref(got), st),
                       "rh_uniform_row")
            assert got.value == n_out.value == c.conv(to_rate)[3] * ch
            rows.append(row)
        row = torch.cat(rows)
        keep += [cat, row]
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = row.data_ptr() + 4 * segs[0][3] * ch, ch, to_rate, 0, LIVE, 1.0
    dst = torch.full((M * ch,), float("nan"), device="cuda")
    _lib.check(lib.rh_wide_mix_block(vp(dst.data_ptr()), ch, to_rate, M, arr, len(srcs), st), "rh_wide_mix_block")
    return dst.cpu().numpy()


def hold(rh, srcs, to_rate, M, ch=2, leads=(0, 1, 2, 3), chain=True, src_lead=1):
    """The entry against the restatement (and the chain), dst at every lead off a 16-byte boundary.  Inputs unchanged.  Returns the restatement."""
    want = R.queue_mix(ch, to_rate, M, srcs)
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


# ---- tiny queues: every rate and layout -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rate,to_rate,ch,to_ch", GRID)
def test_queues_of_one_to_five_tiny_sounds(rh, rate, to_rate, ch, to_ch):
    """Five queues of 1 .. 5 sounds, the first sound of each in the grid's format and the rest of mixed formats, fresh and with cursors
    anywhere, with and without keep_alive, in blocks that outlast them: a seam every few frames."""
    rng = np.random.default_rng(rate % 89 + 10 * ch + to_ch)
    for M, played in ((64, 0), (150, None)):
        srcs = []
        for n in range(1, 6):
            sounds = [sound(rng, 6 * int(rng.integers(1, 4)), ch, rate, GAINS[n])] + tiny_queue(rng, n - 1, n)
            total = R.stream_frames(sounds, False, to_rate)
            srcs.append(queue(M, sounds, keep=bool(n % 2), played=0 if played == 0 else int(rng.integers(0, total)), to_rate=to_rate))
        hold(rh, srcs, to_rate, M, to_ch)


def test_the_crossing_chain_three_pieces_mono_read_as_stereo(rh):
    """A / B / C: the block starts 40 frames in front of the first chain's end and outlasts the queue, which ends inside it (no keep_alive)."""
    rng = np.random.default_rng(5)
    for to_ch, to_rate in ((2, 48000), (1, 44100), (6, 48000)):
        sounds = abc(rng)
        F, T = R.reduced(44100, to_rate)
        M1, M2 = R.span_out(16384, F, T), R.span_out(12, F, T)
        s = queue(100, sounds, keep=False, played=M1 - 40, to_rate=to_rate)
        assert s.words == [0, M1 - 40, 0, 0] and len(s.sounds) == 3
        segs = R.walk(s.sounds, s.words, to_rate, 100)[0]
        assert [(m0, cnt, len(c.runs)) for c, m0, cnt, _ in segs] == [(0, 40, 1), (40, M2, 3)]
        want = hold(rh, [s], to_rate, 100, to_ch, leads=(0, 3))
        assert not bits(want.reshape(100, to_ch)[40 + M2:]).any()


def test_the_keep_alive_tail(rh):
    """A and B with keep_alive: the second chain takes 32768 samples, 8 of A, 6 of B and silence; the block starts in front of it, and a
    later one lies wholly in the silence of that chain.  A queue of tiny sounds is silent behind its last sound."""
    rng = np.random.default_rng(6)
    sounds = abc(rng)[:2]
    M1 = R.span_out(16384, 147, 160)
    s = queue(120, sounds, keep=True, played=M1 - 30)
    want = hold(rh, [s, queue(120, tiny_queue(rng, 3), keep=True)], 48000, 120, 2, leads=(0, 1))
    assert len(R.walk(s.sounds, s.words, 48000, 120)[0][1][0].runs) == 3
    late = queue(50, sounds, keep=True, played=M1 + 5000)
    assert late.words == [32768, 5000, 0, 1] and not bits(hold(rh, [late], 48000, 50, 2, leads=(2,))).any()
    done = R.queue_advance([0, 0, 0, 1], sounds, 48000, M1 + R.span_out(16384, 147, 160))
    assert done == ([0, 0, R.SILENT, 1], 2)
    assert want.size == 240


def test_a_queue_stopped_by_its_frames_and_a_source_with_no_frames(rh):
    rng = np.random.default_rng(8)
    M = 90
    srcs = [queue(37, tiny_queue(rng, 5)), queue(0, tiny_queue(rng, 2)), queue(M, tiny_queue(rng, 4, 2), played=11), R.Src(0, x=np.zeros(0, np.float32), ch=2, from_rate=44100)]
    want = hold(rh, srcs, 48000, M, 2)
    assert np.array_equal(bits(want.reshape(M, 2)[37:]), bits(R.queue_mix(2, 48000, M, srcs[2:3]).reshape(M, 2)[37:]))


def test_queues_and_plain_sources_interleaved_are_the_oracles_mixer(rh, O):
    """Queues and one-shots in insertion order, a one-shot ending inside the block: the oracle's mixer fed SeqSources and SamplesBuffers."""
    from test_queue_mix_cpu import oracle_queue

    rng = np.random.default_rng(12)
    to_rate, M = 48000, 80
    mx, srcs = O.Mixer(2, to_rate), []
    for k in range(6):
        if k % 2 == 0:
            sounds = tiny_queue(rng, 2 + k // 2, k)
            mx.add(oracle_queue(O, sounds))
            srcs.append(queue(M, sounds, keep=False))
        else:
            n, ch, rate = (17, 2, 44100) if k == 1 else (200, 1, 22050) if k == 3 else (9, 2, 48000)
            y = rng.uniform(-1, 1, n * ch).astype(np.float32)
            mx.add(O.SamplesBuffer(ch, rate, y).amplify(0.9))
            F, T = R.reduced(rate, to_rate)
            srcs.append(R.Src(min(M, R.span_out(n, F, T)), x=y, ch=ch, from_rate=rate, gain=0.9, last=n - 1))
    want = mx.pull(M * 2)
    assert want.size == M * 2 and any(not s.sounds and 0 < s.frames < M for s in srcs)
    got = hold(rh, srcs, to_rate, M, 2)
    assert np.array_equal(bits(got), bits(want))


def test_without_a_queue_it_is_rh_wide_mix_block(rh):
    import torch

    from rodio_amd import _lib, source

    rng = np.random.default_rng(9)
    to_rate, M = 48000, 300
    srcs = [plain(rng, ch, rate, to_rate, 5 * k, M, n, 0.4 + 0.3 * k) for k, (ch, rate, n) in enumerate([(2, 44100, 400), (1, 48000, 120), (6, 8000, 30), (2, 96000, 700), (2, 44100, 90)])]
    want = hold(rh, srcs, to_rate, M, 2, chain=False)
    devs = [Dev(s) for s in srcs]
    arr = (_lib.WideSrc * len(srcs))()
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = d.ptr(), s.ch, s.from_rate, s.phase, s.frames, s.last, float(s.gain)
    dst = torch.full((M * 2,), float("nan"), device="cuda")
    _lib.check(_lib.lib.rh_wide_mix_block(C.c_void_p(dst.data_ptr()), 2, to_rate, M, arr, len(srcs), source._stream()), "rh_wide_mix_block")
    assert np.array_equal(bits(dst.cpu().numpy()), bits(want))


def forty(rng, M, to_rate=48000):
    srcs = []
    for k in range(40):
        if k % 7 == 3:
            srcs.append(plain(rng, (2, 1)[k % 2], 44100, to_rate, k, M, 400, 0.6))
        elif k % 11 == 5:
            srcs.append(queue(0, tiny_queue(rng, 2)))
        else:
            sounds = tiny_queue(rng, 1 + k % 5, k)
            srcs.append(queue(M if k % 4 else 30 + k, sounds, keep=bool(k % 3), played=int(rng.integers(0, 20))))
    return srcs


def test_forty_sources_in_one_call(rh):
    rng = np.random.default_rng(40)
    hold(rh, forty(rng, 120), 48000, 120, 2, leads=(0, 1))


def test_no_sources_and_no_frames(rh):
    dst = arena.dst_arena(64, 1)
    rh.queue_mix_block(dst.ptr(), 2, 48000, 32, [])
    assert not bits(dst.check()).any()  # n_sources == 0 writes +0.0
    dst = arena.dst_arena(64, 0)
    rh.queue_mix_block(dst.ptr(), 2, 48000, 32, [rh.QueueSrc(0, [rh.QueueSound(None, 2, 44100, samples=0)], [0, 0, 0, 1])])
    assert not bits(dst.check()).any()
    dst = arena.dst_arena(64, 3)
    rh.queue_mix_block(dst.ptr(), 2, 48000, 32, [rh.QueueSrc(32, [rh.QueueSound(None, 2, 44100, samples=0)], [0, 0, 0, 1]), rh.QueueSrc(32, [rh.QueueSound(None, 2, 44100, samples=0)], [0, 0, 2, 0])])
    assert not bits(dst.check()).any()  # a queue of an empty sound, and one that has ended
    dst = arena.dst_arena(64, 0)
    rh.queue_mix_block(dst.ptr(), 2, 48000, 0, [rh.QueueSrc(5, [rh.QueueSound(None, 0, 0, samples=9)], [9, 9, 9, 9])])  # out_frames == 0: nothing is looked at
    dst.check(written=0)


def test_a_stream_in_three_unequal_blocks(rh):
    """A / B / C with keep_alive and two tiny queues through rh_queue_advance: three blocks -- the second one the first chain's verbatim last
    frame alone -- hold the bits of the one pass, and the entry's cursor is the restatement's."""
    rng = np.random.default_rng(13)
    to_rate = 48000
    M1 = R.span_out(16384, 147, 160)
    queues = [(abc(rng), True), (tiny_queue(rng, 5), False), (tiny_queue(rng, 3, 3), True)]
    first, M = M1 - 60, 200
    state = []
    for sounds, keep in queues:
        words, dropped = R.queue_advance([0, 0, 0, 1 if keep else 0], sounds, to_rate, first if len(sounds[0].x) > 100 else 0)
        state.append((sounds[dropped:], words))
    whole = R.queue_mix(2, to_rate, M, [R.Src(M, s, w) for s, w in state]).reshape(M, 2)
    devs = {id(q): arena.src_arena(q.x, 1) for sounds, _ in queues for q in sounds}
    at = 0
    for n in (59, 1, M - 60):
        srcs = [rh.QueueSrc(n, [rh.QueueSound(devs[id(q)].ptr(), q.ch, q.rate, float(q.gain), samples=q.samples) for q in s], w) for s, w in state if s]
        dst = arena.dst_arena(n * 2, 1)
        rh.queue_mix_block(dst.ptr(), 2, to_rate, n, srcs)
        assert np.array_equal(bits(dst.check()), bits(whole[at:at + n].reshape(-1))), at
        nxt = []
        for s, w in state:
            if not s:
                nxt.append((s, w))
                continue
            got, dropped = rh.queue_advance(w, [rh.QueueSound(devs[id(q)].ptr(), q.ch, q.rate, samples=q.samples) for q in s], to_rate, n)
            assert (got, dropped) == R.queue_advance(w, s, to_rate, n)
            nxt.append((s[dropped:], got))
        state, at = nxt, at + n
    assert [w[2] for _, w in state] == [R.PLAYING, R.ENDED, R.SILENT]
    for a in devs.values():
        a.unchanged()


# ---- arguments ------------------------------------------------------------------------------------------------------------------------------
def tables(srcs, devs, host=lambda a, value=None: a):
    from rodio_amd import _lib

    n = max(len(srcs), 1)
    ns = max(sum(len(s.sounds or []) for s in srcs), 1)
    arr, counts, cursors = host((_lib.WideSrc * n)(), 0), host((C.c_uint32 * n)(), 0), host((C.c_uint64 * (4 * n))(), 0)
    sounds, gains = host((C.c_uint64 * (4 * ns))(), 0), host((C.c_float * ns)(), 0)
    at = 0
    for k, (s, d) in enumerate(zip(srcs, devs)):
        arr[k].frames = s.frames
        cursors[4 * k: 4 * k + 4] = s.words
        if s.sounds:
            counts[k] = len(s.sounds)
            for j, q in enumerate(s.sounds):
                sounds[4 * at: 4 * at + 4] = [d.ptr(j) or 0, q.samples, q.ch, q.rate]
                gains[at] = float(q.gain)
                at += 1
        else:
            arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].last, arr[k].gain = d.ptr(), s.ch, s.from_rate, s.phase, s.last, float(s.gain)
    return arr, sounds, gains, counts, cursors


def call(dst_ptr, ch, to_rate, M, srcs, devs, tweak=None, null=(), n=None):
    """The raw entry: its status.  tweak(arr, sounds, cursors) edits the tables before the call; null: arrays passed as NULL."""
    from rodio_amd import _lib, source

    source._ensure()
    arr, sounds, gains, counts, cursors = tables(srcs, devs)
    if tweak:
        tweak(arr, sounds, cursors)
    return _lib.lib.rh_queue_mix_block(C.c_void_p(dst_ptr) if dst_ptr else None, ch, to_rate, M, None if "srcs" in null else arr, len(srcs) if n is None else n,
                                       None if "sounds" in null else sounds, None if "gains" in null else gains, None if "counts" in null else counts,
                                       None if "cursors" in null else cursors, source._stream())


def test_every_refusal_writes_nothing(rh):
    """Each refusal of rodio_hip.h returns its status and leaves dst as it was (the arena's sentinel in every word).  Source 0 is a plain
    source, 1 a queue of 8 mono samples at 48 kHz (a chain of 8 output frames), 12 stereo at 44.1 kHz and 5 mono at 44.1 kHz."""
    rng = np.random.default_rng(8)
    M = 60
    sounds = [sound(rng, 8, 1, 48000, 0.7), sound(rng, 12, 2, 44100, -1.1), sound(rng, 5, 1, 44100, 1.9)]
    srcs = [R.Src(M, x=rng.uniform(-1, 1, 200).astype(np.float32), ch=2, from_rate=44100, gain=0.5), R.Src(M, sounds, [0, 0, 0, 1])]
    devs = [Dev(s) for s in srcs]
    dst = arena.dst_arena(M * 2, 0)

    def refused(status=INVALID, ch=2, to_rate=48000, frames=M, **kw):
        assert call(dst.ptr(), ch, to_rate, frames, srcs, devs, **kw) == status, kw
        dst.check(written=0)

    def field(k, name, value):
        return lambda arr, s, w: setattr(arr[k], name, value)

    def word(i, value):
        return lambda arr, s, w: w.__setitem__(4 + i, value)

    def snd(k, i, value):
        return lambda arr, s, w: s.__setitem__(4 * k + i, value)

    assert call(None, 2, 48000, M, srcs, devs) == INVALID
    refused(ch=0)
    refused(to_rate=0)
    for name in ("srcs", "sounds", "counts", "cursors"):
        refused(null=(name,))
    # what rh_wide_mix_block refuses of a plain source
    refused(tweak=field(0, "data", None))
    refused(tweak=field(0, "channels", 0))
    refused(tweak=field(0, "from_rate", 0))
    refused(tweak=field(0, "frames", M + 1))
    refused(tweak=field(0, "phase", 160))
    refused(UNSUPPORTED, tweak=field(0, "from_rate", 4294967291))  # F T beyond 32 bits
    # the queue
    refused(tweak=field(1, "frames", M + 1))
    refused(tweak=snd(1, 0, 0))             # data 0 with samples > 0
    refused(tweak=snd(1, 2, 0))             # channels 0
    refused(tweak=snd(2, 3, 0))             # rate 0
    refused(tweak=snd(0, 2, 1 << 32))       # channels beyond 32 bits
    refused(tweak=word(2, 3))               # a state above 2
    refused(tweak=word(3, 2))               # flags above 1
    refused(tweak=word(0, 8))               # chain_start == sounds[0].samples
    refused(tweak=word(1, 8))               # chain_out == the chain's output count
    refused(tweak=lambda arr, s, w: (w.__setitem__(6, 1), w.__setitem__(4, 1)))  # a silent queue with a chain_start
    refused(UNSUPPORTED, tweak=snd(1, 3, 4294967291))  # F T beyond 32 bits of a chain
    refused(UNSUPPORTED, tweak=snd(1, 1, 11))          # the stereo chain takes 11 samples: it ends inside a frame
    refused(UNSUPPORTED, tweak=snd(1, 2, 5))           # 12 samples read as frames of five channels
    refused(UNSUPPORTED, to_rate=4294967295, tweak=lambda arr, s, w: (setattr(arr[0], "frames", 0), s.__setitem__(3, 1)))  # M F: 7 * (2^32 - 1) + 1 positions
    # positions beyond 32 bits
    refused(UNSUPPORTED, frames=0x80000000)
    refused(UNSUPPORTED, frames=0x7FFFFFFF)  # the plain source: out_frames > (2^32 - 1 - T) / F
    # the cursor's bounds are met by the last valid value; without gains every gain is 1
    for tw in (word(0, 7), word(1, 7)):
        d2 = arena.dst_arena(M * 2, 0)
        assert call(d2.ptr(), 2, 48000, M, srcs, devs, tweak=tw) == 0
        d2.check()
    d2 = arena.dst_arena(M * 2, 0)
    assert call(d2.ptr(), 2, 48000, M, srcs, devs, null=("gains",)) == 0
    ones = [srcs[0], R.Src(M, [R.Sound(q.x, q.ch, q.rate) for q in sounds], [0, 0, 0, 1])]
    assert np.array_equal(bits(d2.check()), bits(R.queue_mix(2, 48000, M, ones)))
    # a queue's other rh_wide_src fields are not read
    d2 = arena.dst_arena(M * 2, 0)
    assert call(d2.ptr(), 2, 48000, M, srcs, devs, tweak=lambda arr, s, w: (setattr(arr[1], "phase", 4000000000), setattr(arr[1], "last", 0), setattr(arr[1], "channels", 0))) == 0
    assert np.array_equal(bits(d2.check()), bits(R.queue_mix(2, 48000, M, srcs)))
    # out_frames == 0: nothing to do, whatever the rest says
    assert call(dst.ptr(), 0, 0, 0, srcs, devs, null=("srcs", "sounds", "counts", "cursors")) == 0
    dst.check(written=0)
    assert call(dst.ptr(), 2, 48000, M, srcs, devs) == 0
    assert np.array_equal(bits(dst.check()), bits(R.queue_mix(2, 48000, M, srcs)))
    for d in devs:
        d.unchanged()


# ---- a side stream --------------------------------------------------------------------------------------------------------------------------
def test_behind_a_gate_on_a_side_stream(rh):
    """The copy of the tables and the launch go to the stream the call is given (tests/stream_gate.py): 40 sources queued behind a gate on a
    side stream while their inputs still hold garbage, all five host tables overwritten as soon as the call has returned.  The call returns
    while the gate is pending, and the snapshot holds the restatement's bits.  The side stream is one of rh_stream_create, as in
    tests/test_gpu_player_mix.py (whose reasons hold here)."""
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
    M, to_rate = 120, 48000
    srcs = forty(rng, M)
    want = R.queue_mix(2, to_rate, M, srcs)

    def build(k):
        devs = [Dev(s) for s in srcs]
        for d in devs:
            for a in d.arenas:
                if a:
                    k.add(a)
        dst = k.dst(M * 2, 0)

        def one():
            arr, sounds, gains, counts, cursors = tables(srcs, devs, k.host)
            _lib.check(_lib.lib.rh_queue_mix_block(C.c_void_p(dst.ptr()), 2, to_rate, M, arr, len(srcs), sounds, gains, counts, cursors, source._stream()), "rh_queue_mix_block")

        def check():
            assert arena.same(dst.check_snapshot(), want)
            for d in devs:
                for a in d.arenas:
                    if a:
                        a.snapshot_unchanged()

        return stream_gate.case([one], check)

    r = stream_gate.run(build, side, delay, 63.0)  # (ms: test_gpu_player_mix.py's gate)
    assert all(r.pending), ("the call waited for the stream, or the gate is too short", r.pending, r.host_ms)
    r.check()


# ---- the wrapper ----------------------------------------------------------------------------------------------------------------------------
def test_the_wrapper_takes_tensors_and_the_helpers_are_the_restatements(rh):
    import torch

    rng = np.random.default_rng(4)
    M = 100
    queues = [tiny_queue(rng, n, n) for n in range(1, 6)]
    srcs = [queue(M, sounds, keep=bool(k % 2)) for k, sounds in enumerate(queues)]
    dst = torch.full((2 * M,), float("nan"), device="cuda")
    rh.queue_mix_block(dst, 2, 48000, M, [rh.QueueSrc(M, [rh.QueueSound(torch.from_numpy(q.x).cuda(), q.ch, q.rate, float(q.gain)) for q in s.sounds], s.words) for s in srcs])
    assert np.array_equal(bits(dst.cpu().numpy()), bits(R.queue_mix(2, 48000, M, srcs)))
    assert rh.queue_plan() == [0, 0, 0, 1] and rh.queue_plan(keep_alive=False) == [0, 0, 0, 0]
    for sounds in queues:
        w, mine = [0, 0, 0, 1], [rh.QueueSound(1 << 20, q.ch, q.rate, samples=q.samples) for q in sounds]
        for n in (1, 7, 0, 30, 4097):
            got = rh.queue_advance(w, mine, 48000, n)
            assert got == R.queue_advance(w, sounds, 48000, n)
            w, mine, sounds = got[0], mine[got[1]:], sounds[got[1]:]
    with pytest.raises(rh.RhError):
        rh.queue_advance([0, 0, 0, 1], [rh.QueueSound(1 << 20, 6, 48000, samples=32772)], 48000, 10)  # a chain that cuts a frame
    with pytest.raises(ValueError):
        rh.QueueSrc(M, [], words=[1, 2, 3])
    with pytest.raises(ValueError):
        rh.QueueSound(1 << 20, 2, 44100)
