"""The block mixers where their grid-stride loops run a second and a third time, and rh_loop_mix_block, rh_queue_mix_block and
rh_clip_mix_block where their 32-bit positions lie in the upper half of 32 bits, where the clip's fade leaves 32 bits, and where a clip's
cursor lies far from the start of its stream (tests/test_mix_edges_cpu.py holds the premises, tests/test_gpu_mix_edges.py runs the cases;
a plain helper module like wide_positions.py: no fixtures, numpy and Python ints only).

A  Every per-sample mixer kernel is launched with at most 4096 workgroups of 256 lanes and walks the rest of a block with `o += stride`;
   the two fast kernels sweep 64 frames a workgroup.  The sweep sizes below restate those launch lines; the cases are blocks of more
   than two and less than three sweeps that are no multiple of 256 samples, with chain ends, seams and source ends behind the first one.
B  loopmix::locate, clipmix::locate and queuemix::locate keep x0 + m, p and j F in a u32 and divide by multiply-high reciprocals; the
   plans refuse what leaves 32 bits.  The cases put those numbers at and above 2^31 -- where div_u32's `(x - t) >> s1` has its top bit
   set -- and within 1443 of 2^32 - 1, every one of them worked out here with Python ints.
C  clipmix::fade_ms has a 32-bit and a 64-bit form; fade_mode() restates describe()'s choice between them.
D  Clips whose delay or cursor lies beyond 2^32, 2^40 and 2^50 samples: only clip_mix_ref.clip_window() reaches there."""
import numpy as np

import clip_mix_ref as CR
import loop_mix_ref as LR
import player_mix_ref as PR
import queue_mix_ref as QR
import wide_positions as W

f32 = np.float32
U32 = 1 << 32
HALF = 1 << 31

# ---- A: the sweeps ----------------------------------------------------------------------------------------------------------------------------
# `rh::grid_for(total, kBlock, 256u * 16u)` with kBlock = 256 in rh_widemix.hip (k_wide_mix, the alike-sources kernel, k_wide_rows),
# rh_playermix.hip, rh_spatialmix.hip, rh_loopmix.hip, rh_queuemix.hip and rh_clipmix.hip: 4096 workgroups of 256 output SAMPLES
SWEEP_SAMPLES = 4096 * 256
# `rh::grid_for(nf, kFastFrames, 256u * 16u)` in rh_playermix.hip and `rh::grid_for(nf, kSpFastFrames, 256u * 16u)` in
# rh_spatialmix.hip: 4096 workgroups of 64 output FRAMES
SWEEP_FAST_FRAMES = 4096 * 64
LONG_SAMPLES = 2 * SWEEP_SAMPLES + 4099         # rounded down to whole frames by long_frames()
LONG_FAST_FRAMES = 2 * SWEEP_FAST_FRAMES + 77
RATES_A = [(44100, 48000), (48000, 48000)]      # and once at equal rates: F == T, every frame verbatim


def long_frames(ch):
    return LONG_SAMPLES // ch


def sweeps_of(frames, ch):
    """The premise of every case of part A, as numbers: (sweeps the block takes, its samples mod 256)."""
    return frames * ch / SWEEP_SAMPLES, frames * ch % 256


def behind_first_sweep(frame, ch):
    return frame * ch >= SWEEP_SAMPLES


def third_sweep_frame(ch):
    """A block frame in the middle of what the block has of the third sweep."""
    return (2 * SWEEP_SAMPLES + 2048) // ch


def signal(rng, n):
    return W.signal(rng, n)


def plain_ending(rng, ch, rate, to_rate, M, end_frame, gain, src=LR.Src):
    """A plain source of a block [0, M) whose stream ends about block frame end_frame: (the source, the frames it reaches)."""
    F, T = W.reduced(rate, to_rate)
    n = W.frames_for_total(F, T, end_frame)
    b = PR.block_of(signal(rng, n * ch), ch, rate, to_rate, 0, M)
    assert b.frames == W.out_frames(n, F, T) < M
    if src is QR.Src:
        return QR.Src(b.frames, x=b.x, ch=ch, from_rate=rate, gain=gain, phase=b.phase, last=b.last)
    return src(b.x, ch, rate, b.frames, gain=gain, phase=b.phase, last=b.last)


# -- loops
def loop_long(rate, to_rate, many=False, seed=0):
    """A rule-1 loop of 20 000 stereo frames (chains of 16 384 frames of the unrolled stream), a rule-0 loop of 9 frames with c = 4 and a
    plain source that ends inside the third sweep, in a stereo block of long_frames(2); many: 30 loops of 300 frames between them, so
    that the second launch -- it continues from the stored sum -- holds a source that reaches the whole block."""
    rng = np.random.default_rng(100 + seed + rate % 7)
    M = long_frames(2)
    big = LR.Src(signal(rng, 40000), 2, rate, M, gain=0.8, words=LR.loop_advance(LR.loop_plan(40000, 2, 40000), rate, to_rate, 12345))
    small = LR.Src(signal(rng, 18), 2, rate, M, gain=-0.6, words=LR.loop_advance([9, 4, 0, 0, 0], rate, to_rate, 7))
    plain = plain_ending(rng, 2, rate, to_rate, M, third_sweep_frame(2), 0.5)
    srcs = [big, plain]
    if many:
        for k in range(30):
            L, c, rule = [(5, 5, 0), (10, 4, 0), (9, 4, 0), (5, 4, 1), (10, 4, 1)][k % 5]
            ch = (2, 1)[k % 2]
            srcs.append(LR.Src(signal(rng, L * ch), ch, rate, 300, gain=0.3 + 0.01 * k, words=LR.loop_advance([L, c, rule, 0, 0], rate, to_rate, 11 * k)))
    srcs.append(small)  # (many: source 32, alone in the second launch)
    return dict(srcs=srcs, M=M, ch=2, to_rate=to_rate, big=big, small=small, plain=plain)


# -- queues
QUEUE_FORMATS = [(1, 44100), (2, 48000), (6, 22050)]


def queue_sounds(rng, n_sounds, most=50000):
    """Sounds of mono 44.1 kHz, stereo 48 kHz and 6-channel 22.05 kHz in turn, 3 .. `most` samples, every length a whole number of frames
    of all three formats but the seventh, a mono one of 3 samples, and the 50 000-sample ones; six-channel sounds stay below a chain's 32 768
    samples, which six does not divide."""
    out = []
    for k in range(n_sounds):
        ch, rate = QUEUE_FORMATS[k % 3]
        if k == 6:
            n = 3
        elif k % 9 == 3:
            n = 50000  # (mono: two chains, the second one reads on into the sounds behind)
        elif k % 9 == 4:
            n = most   # (stereo)
        else:
            n = 6 * int(rng.integers(1, (32766 if ch == 6 else most) // 6 + 1))
        out.append(QR.Sound(signal(rng, n), ch, rate, (0.7, -1.1, 0.5, 0.9)[k % 4]))
    return out


def queue_at(frames, sounds, keep, played, to_rate):
    words, dropped = QR.queue_advance([0, 0, 0, 1 if keep else 0], sounds, to_rate, played)
    return QR.Src(frames, sounds[dropped:], words)


def queue_long(to_rate, seed=0):
    """A queue of 100 sounds of mixed formats that outlasts a stereo block of long_frames(2), a queue with keep_alive that goes silent
    inside the second sweep and a plain source that ends in the third."""
    rng = np.random.default_rng(200 + seed + to_rate % 7)
    M = long_frames(2)
    sounds = queue_sounds(rng, 100)
    short = queue_sounds(rng, 50)
    total = 0
    while True:  # the longest head of `short` whose stream -- its keep-alive chain included -- ends inside the second sweep
        total = QR.stream_frames(short, True, to_rate)
        if total * 2 < 2 * SWEEP_SAMPLES - 4096:
            break
        short = short[:-1]
    plain_rate = 44100 if to_rate == 48000 else 48000
    # the cursor: where a chain of the stream starts 1000 frames inside the block's share of the third sweep
    at = next(m0 for _, m0, _, _ in QR.walk(sounds, [0, 0, 0, 1], to_rate, 1 << 30)[0] if m0 >= SWEEP_SAMPLES + 3000)
    srcs = [queue_at(M, sounds, True, at - (SWEEP_SAMPLES + 1000), to_rate), plain_ending(rng, 2, plain_rate, to_rate, M, third_sweep_frame(2), 0.5, src=QR.Src), queue_at(M, short, True, 0, to_rate)]
    return dict(srcs=srcs, M=M, ch=2, to_rate=to_rate, silent_from=total)


def queue_seams(s, to_rate):
    """(block frames at which a chain of the queue starts, ... at which a chain's taps pass from one sound to the next)."""
    starts, seams = [], []
    for c, m0, cnt, prior in QR.walk(s.sounds, s.words, to_rate, s.frames)[0]:
        starts.append(m0)
        F, T, n, _ = c.conv(to_rate)
        for _, _, at, _ in c.runs[1:]:  # the first output frame of the chain whose first tap lies at or behind the run's first frame
            j = -(-(at // c.ch) * T // F)
            if prior <= j < prior + cnt:
                seams.append(m0 + j - prior)
    return starts, seams


# -- clips
def case(*a, **kw):
    from test_clip_mix_cpu import Case  # (the clip cases' builder: numpy only)

    return Case(*a, **kw)


def clip_long(rate, to_rate, many=False, seed=0):
    """A fading rule-G clip with an odd delay that ends inside the second sweep, a rule-C clip that spans the block, a clip still in its
    delay for the whole block and a plain source that ends in the third sweep, in a stereo block of long_frames(2); many: 29 clips of
    300 frames between them."""
    rng = np.random.default_rng(300 + seed + rate % 7)
    M = long_frames(2)
    F, T = W.reduced(rate, to_rate)
    n_in = M * F // T + 10  # source frames the block spans
    fading = case("A: rule G, odd delay, fading, ends in the second sweep", 1_400_001, 70001, take=1_300_001, fade=True, rate=rate, to_rate=to_rate, gain=-1.1)
    whole = case("A: rule C, spans the block", 2 * n_in, 40000, kind="test", rate=rate, to_rate=to_rate)
    waiting = case("A: in its delay for the whole block", 3001, 2 * n_in + 1001, kind="test", take=5000, rate=rate, to_rate=to_rate)
    f = fading.src()
    f.frames = min(f.frames, M)
    srcs = [f, plain_ending(rng, 2, rate, to_rate, M, third_sweep_frame(2), 0.5, src=CR.Src)]
    if many:
        from test_clip_mix_cpu import CASES

        short = [c for c in CASES if (c.to_ch, c.to_rate, c.rate) == (2, to_rate, rate) and CR.clip_out_frames(c.words(), c.ch, c.rate, to_rate) > 0]
        for k in range(29):
            c = short[k % len(short)]
            total = CR.clip_out_frames(c.words(), c.ch, c.rate, to_rate)
            done = (37 * k) % max(total - 1, 1)
            srcs.append(c.src(min(300, total - done), done))
    srcs += [waiting.src(M, 0), whole.src(M, 0)]  # (many: the rule-C clip is source 32, alone in the second launch)
    return dict(srcs=srcs, M=M, ch=2, to_rate=to_rate, fading=f, whole=srcs[-1], waiting=srcs[-2])


# -- the wide entries
def wide_long(rate, to_rate, to_ch=2, alike=False, seed=0):
    """Five sources [(x, ch, rate, gain)] of a block [0, long_frames(to_ch)): layouts 1, 2, 6 and the mixer's own, the last one ending
    inside the third sweep (the fifth: a second group of four); alike: the mixer's layout and one rate, all live but the last."""
    rng = np.random.default_rng(400 + seed + rate % 7 + to_ch)
    M = long_frames(to_ch)
    F, T = W.reduced(rate, to_rate)
    srcs = []
    for k in range(5):
        ch = to_ch if alike else (1, 2, 6, to_ch, 2)[k]
        n = W.live_frames(F, T, M) if k < 4 else W.frames_for_total(F, T, third_sweep_frame(to_ch))
        srcs.append((signal(rng, n * ch), ch, rate, W.GAINS[k]))
    end = W.out_frames(len(srcs[-1][0]) // srcs[-1][1], F, T)
    return dict(srcs=srcs, M=M, ch=to_ch, to_rate=to_rate, end=end)


def batch_long(rate, to_rate, seed=0):
    """Two mixers of one batch: a mono one of 1000 frames -- shorter than a sweep -- and a stereo one of long_frames(2)."""
    rng = np.random.default_rng(500 + seed + rate % 7)
    F, T = W.reduced(rate, to_rate)
    mixers = []
    for to_ch, M in ((1, 1000), (2, long_frames(2))):
        srcs = [(signal(rng, W.live_frames(F, T, M) * ch), ch, rate, W.GAINS[k]) for k, ch in enumerate((2, 1, to_ch))]
        mixers.append(dict(srcs=srcs, M=M, ch=to_ch, to_rate=to_rate))
    return mixers


# -- the player and the spatial entry (their source builders live beside their GPU tests; both are numpy only)
def player_long(rate, to_rate, fast, seed=0):
    """Four live stereo sources: no adapter; a fade-in ramp that ends at three quarters of the block, behind the first sweep; a fade-out
    that ended long ago under factors on a period of 441; factors on a period of 3.  fast: a block of LONG_FAST_FRAMES for the
    specialised kernel (the host gate sends it there with sources and dst on 8-byte boundaries), otherwise long_frames(2)."""
    import test_gpu_player_mix as PL

    rng = np.random.default_rng(800 + seed + rate % 7 + fast)
    M = LONG_FAST_FRAMES if fast else long_frames(2)
    F, T = W.reduced(rate, to_rate)
    ramp_ns = (3 * M // 4) * F // T * (1_000_000_000 // rate)
    mk = lambda **kw: PL.make(rng, 2, rate, to_rate, M, 0, **kw)  # noqa: E731
    srcs = [mk(), mk(kind=PR.RAMP, ramp_ns=ramp_ns, start=0.1, end=1.3), mk(kind=PR.CLAMP, ramp_ns=5_000_000, start=1.0, end=0.4, first_frame=10**6, fp=441, ff=5), mk(fp=3, ff=2)]
    return dict(srcs=srcs, M=M, ch=2, to_rate=to_rate, ramp_end=ramp_ns // (1_000_000_000 // rate) * T // F)


def spatial_long(rate, to_rate, fast, seed=0):
    """fast: three mono emitters into stereo, a block of LONG_FAST_FRAMES; otherwise a six-channel and a mono source into five channels, a
    block of long_frames(5).  Gains step every 50 021 samples of the emitter's output (one of them every 7), factors every 441: steps all
    over the block, behind the first sweep as in front of it."""
    import test_gpu_spatial_mix as SP

    rng = np.random.default_rng(900 + seed + rate % 7 + fast)
    ch = 2 if fast else 5
    M = LONG_FAST_FRAMES if fast else long_frames(5)
    ins = (1, 1, 1) if fast else (6, 1)
    srcs = [SP.make(rng, in_ch, rate, to_rate, M, 0, None, ch, gp=(50021, 7, 50021)[k], gf=3 * k, fp=(None, 441, 5)[k], ff=k) for k, in_ch in enumerate(ins)]
    return dict(srcs=srcs, M=M, ch=ch, to_rate=to_rate)


# ---- B: positions in the upper half of 32 bits ----------------------------------------------------------------------------------------------
T24 = W.BY_ID["100-16777259"]  # F = 100, T = 16 777 259: a chain of 255 frames emits 42 614 239 frames, j F reaches 4 261 423 900
EDGE = (32749, 131074)         # a mono chain of 32 768 frames: M F is 1443 below 2^32 - 1
OVER = (32749, 131075)         # ... and its neighbour, which every plan refuses
FIT_C = W.BY_ID["65521-65519"]
# div_u32's correction `(x - t) >> s1` has its top bit set only where t = mulhi(x, m) is small beside x >= 2^31: for a divisor just BELOW a
# power of two (m = floor(2^32 (2^l - d) / d) + 1 is small then).  T = 16 777 259 and T = 131 074 lie just ABOVE one -- there m is next to
# 2^32 and x - t stays small however large x is -- so the pairs above put j F high without ever setting that bit.  This pair does both:
# T = 2^17 - 1, and a mono chain of 32 768 frames emits M = 131 145 frames with M F = 4 294 867 605, 99 690 below 2^32 - 1
BELOW = (32749, 131071)
EDGE_PAIRS = [EDGE, BELOW]


def chain_numbers(rate, to_rate, c):
    """(F, T, M, M F) of a whole chain of c frames."""
    F, T = W.reduced(rate, to_rate)
    M = PR.stream_out_frames(c, F, T)
    return F, T, M, M * F


BIG_LOOP = dict(L=14032, c=255)  # mono: 55 chains of 255 frames and one of 7; P = 2 344 789 782


def big_loop_numbers():
    F, T, M, _ = chain_numbers(T24.from_rate, T24.to_rate, BIG_LOOP["c"])
    L, c = BIG_LOOP["L"], BIG_LOOP["c"]
    tail = PR.stream_out_frames(L % c, F, T)
    return dict(F=F, T=T, M=M, tail=tail, P=(L // c) * M + tail, chains=L // c)


def big_loop_words(which):
    """The cursor of the 14 032-frame loop: "chain": 150 frames in front of the end of chain 51 (x0 >= 2^31); "pass": 150 frames in front
    of the end of the pass's tail chain, so that x passes P inside the block and p wraps to 0."""
    n = big_loop_numbers()
    k, out = (51, n["M"] - 150) if which == "chain" else (n["chains"], n["tail"] - 150)
    return [BIG_LOOP["L"], BIG_LOOP["c"], 0, k * BIG_LOOP["c"], out], k * n["M"] + out


def edge_plain(rng, rate, to_rate, M, gain=0.5, src=LR.Src):
    """A plain mono source at the pair's from_rate from a frame with a large phase: playermix::check_src's source beside the others."""
    F, T = W.reduced(rate, to_rate)
    m0 = max(range(1000, 3000), key=lambda m: m * F % T)
    b = PR.block_of(signal(rng, W.live_frames(F, T, m0 + M)), 1, rate, to_rate, m0, m0 + M)
    assert b.frames == M
    if src is QR.Src:
        return QR.Src(M, x=b.x, ch=1, from_rate=rate, gain=gain, phase=b.phase, last=b.last)
    return src(b.x, 1, rate, M, gain=gain, phase=b.phase, last=b.last)


def big_loop_case(which, M=300):
    rng = np.random.default_rng(600)
    words, x0 = big_loop_words(which)
    s = LR.Src(signal(rng, BIG_LOOP["L"]), 1, T24.from_rate, M, gain=0.9, words=words)
    return dict(srcs=[s, edge_plain(rng, T24.from_rate, T24.to_rate, M)], M=M, ch=2, to_rate=T24.to_rate, x0=x0)


def edge_loops(c, rule, M=300):
    """A stereo and a mono loop of 300 frames with chains of c frames at 100 -> 16 777 259 Hz, the cursor 150 output frames in front of
    the end of a whole chain: pos = j F lies above 2^31 (c = 256: within 2 10^7 of 2^32)."""
    rng = np.random.default_rng(610 + c + rule)
    F, T, Mc, _ = chain_numbers(T24.from_rate, T24.to_rate, c)
    srcs = []
    for k, ch in enumerate((2, 1)):
        words = [300, c, rule, 0, Mc - 150 - 7 * k]
        srcs.append(LR.Src(signal(rng, 300 * ch), ch, T24.from_rate, M, gain=(-0.8, 1.3)[k], words=words))
    srcs.append(edge_plain(rng, T24.from_rate, T24.to_rate, M))
    return dict(srcs=srcs, M=M, ch=2, to_rate=T24.to_rate, j=Mc - 150, F=F, Mc=Mc)


def below_loops(rule, M=300):
    """A mono loop of 33 000 frames at BELOW as rh_loop_plan cuts it -- rule 1: a SamplesBuffer, chains of 32 768 frames of the unrolled
    stream; rule 0: a None-span source, chains of 32 768 and 232 frames -- with the cursor 150 frames in front of the first chain's end:
    j F > 2^31 under a divisor whose reciprocal is small."""
    rng = np.random.default_rng(640 + rule)
    F, T, Mc, _ = chain_numbers(*BELOW, 32768)
    words = LR.loop_plan(33000, 1, 33000 if rule else 0)[:3] + [0, Mc - 150]
    s = LR.Src(signal(rng, 33000), 1, BELOW[0], M, gain=0.9, words=words)
    return dict(srcs=[s, edge_plain(rng, *BELOW, M)], M=M, ch=2, to_rate=BELOW[1], j=Mc - 150, F=F, Mc=Mc)


EDGE_BLOCKS = ["ends with the chain's last frame", "starts behind it", "straddles it"]


def edge_dones(M=300, pair=EDGE):
    """The cursors of three blocks of M frames around the end of the first chain at EDGE (or at `pair`)."""
    _, _, Mc, _ = chain_numbers(*pair, 32768)
    return dict(zip(EDGE_BLOCKS, (Mc - M, Mc, Mc - M // 2)))


def edge_clip(to_rate=EDGE[1]):
    """A mono sound of 40 000 samples behind a delay of 101 samples, fading over a take of 39 000: its first chain has 32 768 frames."""
    return case("B: rule G at the 32-bit bound", 40000, 101, take=39000, fade=True, ch=1, rate=EDGE[0], to_rate=to_rate, gain=0.9)


def edge_clip_case(which, M=300, to_rate=EDGE[1], pair=EDGE):
    """pair: the pair the cursors are worked out at (to_rate differs from its rate only for the refused neighbour)."""
    rng = np.random.default_rng(620)
    to_rate = pair[1] if pair is not EDGE else to_rate
    done = edge_dones(M, pair)[which]
    c = edge_clip(to_rate)
    return dict(srcs=[c.src(M, done), edge_plain(rng, EDGE[0], to_rate, M, src=CR.Src)], M=M, ch=2, to_rate=to_rate, done=done)


def edge_queue_sounds():
    rng = np.random.default_rng(630)
    return [QR.Sound(signal(rng, 40000), 1, EDGE[0], 0.9), QR.Sound(signal(rng, 600), 2, 44100, -0.7)]


def edge_queue_case(which, M=300, pair=EDGE):
    rng = np.random.default_rng(631)
    to_rate = pair[1]
    done = edge_dones(M, pair)[which]
    return dict(srcs=[queue_at(M, edge_queue_sounds(), True, done, to_rate), edge_plain(rng, EDGE[0], to_rate, M, src=QR.Src)], M=M, ch=2, to_rate=to_rate, done=done)


def fit_c():
    """Rule C at 65 521 -> 65 519 Hz from the cursor with the largest phase of 40 000: (done, r0, fit), fit the largest block with
    r0 + (fit - 1) F <= 2^32 - 1."""
    done = W.largest_phase(FIT_C)
    r0 = done * FIT_C.F % FIT_C.T
    return done, r0, (U32 - 1 - r0) // FIT_C.F + 1


def fit_c_clip():
    done, _, fit = fit_c()
    n = 2 * ((done + fit + 10) * FIT_C.F // FIT_C.T + 4)
    return case("B: rule C at its fit", n, 1000, kind="test", rate=FIT_C.from_rate, to_rate=FIT_C.to_rate, gain=0.7)


# ---- C: the fade in 32 and in 64 bits -------------------------------------------------------------------------------------------------------
M_CHAIN = 17833  # output frames of a whole stereo chain at 44.1 -> 48 kHz
NO_FADE, FADE32, FADE64 = 0, 1, 2


def fade_mode(s, to_rate):
    """clipmix::describe()'s choice restated: the 32-bit form while ms0 and reach * dps + ns_pad fit 32 bits, with `reach` the stream
    samples from the first sample of the chain in progress (rule C: of the first tap's frame) up to the end of the last chain (the frame
    behind the last tap) the block touches."""
    kind, Z, N, take_ns, flags, done = s.words[:6]
    if not flags & CR.FADE:
        return NO_FADE
    F, T = W.reduced(s.from_rate, to_rate)
    Ls, ch = Z + N, s.ch
    if kind == CR.RULE_G:
        c = CR.CHAIN_SAMPLES // ch if Ls > CR.CHAIN_SAMPLES else Ls // ch
        Mc = PR.stream_out_frames(c, F, T)
        q0, j0 = done // Mc, done % Mc
        base, reach = q0 * c * ch, ((j0 + s.frames - 1) // Mc + 1) * c * ch
    else:
        i0, r0 = done * F // T, done * F % T
        base, reach = i0 * ch, ((r0 + (s.frames - 1) * F) // T + 2) * ch
    reach = min(reach, Ls - base)
    kbase = max(base - Z, 0)
    rem0 = take_ns - kbase * CR.ns_per_sample(ch, s.from_rate)
    ms0, ns_pad = rem0 // CR.NS_PER_MS, CR.NS_PER_MS - 1 - rem0 % CR.NS_PER_MS
    return FADE32 if ms0 <= U32 - 1 and reach * CR.ns_per_sample(ch, s.from_rate) + ns_pad <= U32 - 1 else FADE64


def fade_clip():
    """A fading rule-G clip of 14 chains, stereo 44.1 -> 48 kHz, behind an odd delay."""
    return case("C: fading over fourteen chains", 450_001, 101, take=440_001, fade=True, gain=-1.1)


# Eleven chains: the 32-bit form.  One frame more: describe() chooses the 64-bit one, since `reach` covers the twelfth chain whole -- but
# that frame reads the chain's first samples only, whose products krel dps + ns_pad still fit 32 bits: the two forms give the same number
# there.  Twelve whole chains: the taps of the twelfth chain's last 7 000 frames have products beyond 2^32 - 1 (fade_overflows()).
FADE_BLOCKS = [M_CHAIN * 11, M_CHAIN * 11 + 1, M_CHAIN * 12]


def fade_overflows(s, to_rate):
    """Whether a tap of the block has krel dps + ns_pad > 2^32 - 1, krel counted as describe() counts it: where the 32-bit form is wrong."""
    kind, Z, N, take_ns, flags, done = s.words[:6]
    assert kind == CR.RULE_G and flags & CR.FADE
    F, T = W.reduced(s.from_rate, to_rate)
    c = CR.CHAIN_SAMPLES // s.ch
    Mc = PR.stream_out_frames(c, F, T)
    base = done // Mc * c * s.ch
    kbase = max(base - Z, 0)
    dps = CR.ns_per_sample(s.ch, s.from_rate)
    ns_pad = CR.NS_PER_MS - 1 - (take_ns - kbase * dps) % CR.NS_PER_MS
    fr, two, _ = CR.tap_of(s.words, s.ch, s.from_rate, to_rate, done + s.frames - 1)  # the block's last frame has its largest samples
    k_last = (fr + (1 if two else 0)) * s.ch + s.ch - 1 - Z - kbase
    return k_last * dps + ns_pad > U32 - 1


def long_take_clip():
    """A take of 58 days on 401 samples: more than 2^32 ms remain, ms0 alone forces the 64-bit form."""
    return case("C: a take beyond 2^32 ms", 401, 31, take=("ns", 5 * 10**15), fade=True, kind="test")


def short_take_clip():
    """A take under a millisecond: x * 0 / 0, NaN by position."""
    return case("C: a take under a millisecond", 3000, 11, take=("ns", 900_000), fade=True)


# ---- D: cursors far from the stream's start -------------------------------------------------------------------------------------------------
def far_words(kind, Z, N, ch, rate, to_rate, take_ns=0, flags=0, done=0):
    w = [kind, Z, N, take_ns, flags, 0, 0]
    total = CR.clip_out_frames_wide(w, ch, rate, to_rate)
    assert done <= total
    return w[:5] + [done, total]


FAR_G = dict(Z=(1 << 40) + 1, N=4001, ch=2, rate=44100, to_rate=48000)  # an odd delay: the stereo sound is shifted by one channel


def far_g():
    """Rule G behind 2^40 + 1 zeros: (the sound, the words at cursor 0, the cursors of the three blocks of 300 frames -- deep in the
    delay, the one in which the delay ends, the next one)."""
    rng = np.random.default_rng(700)
    Z, N = FAR_G["Z"], FAR_G["N"]
    take_ns = N * CR.ns_per_sample(2, 44100) + 37
    words = far_words(CR.RULE_G, Z, N, 2, 44100, 48000, take_ns, CR.TAKE | CR.FADE)
    q = Z // CR.CHAIN_SAMPLES  # the chain in which the sound starts
    first = q * M_CHAIN  # its first output frame: every chain in front of it is a whole one
    return signal(rng, N), words, [12345, first - 100, first + 200]


def far_c():
    """Rule C behind 2^45 + 2 zeros, stereo 44.1 -> 48 kHz: (the sound, the words, the cursor of the block in which the sound starts)."""
    rng = np.random.default_rng(710)
    Z, N = (1 << 45) + 2, 4000
    words = far_words(CR.RULE_C, Z, N, 2, 44100, 48000)
    first = -(-(Z // 2) * 160 // 147)  # the first output frame whose first tap lies in the sound
    return signal(rng, N), words, first - 100


def far_c_128():
    """Rule C at 65 521 -> 65 519 Hz with done = 2^50 + 12345: done * F leaves 64 bits.  The sound starts 50 frames behind the block's
    first tap."""
    rng = np.random.default_rng(720)
    done = (1 << 50) + 12345
    i0 = done * FIT_C.F // FIT_C.T
    Z, N = 2 * (i0 + 50), 1000
    words = far_words(CR.RULE_C, Z, N, 2, FIT_C.from_rate, FIT_C.to_rate, done=done)
    return signal(rng, N), words, done


def far_queue():
    """A queue whose first sound has 50 000 mono samples: its second chain starts at sample 32 768 of it and reads on into the sounds
    behind.  (the sounds, the output frames of the first chain)."""
    rng = np.random.default_rng(730)
    sounds = [QR.Sound(signal(rng, 50000), 1, 44100, 0.8), QR.Sound(signal(rng, 9000), 2, 48000, -1.1), QR.Sound(signal(rng, 12000), 6, 22050, 0.6), QR.Sound(signal(rng, 30000), 1, 44100, 0.9)]
    return sounds, PR.stream_out_frames(32768, 147, 160)
