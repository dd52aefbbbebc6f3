"""The block mixers beyond one sweep of their grid-stride loops, and rh_loop_mix_block, rh_queue_mix_block and rh_clip_mix_block where
their positions lie in the upper half of 32 bits, where the clip's fade takes its 64-bit form and where a clip's cursor lies 2^40 and 2^50
samples from the start of its stream.  The cases and their numbers are tests/mix_edges.py's (premises: tests/test_mix_edges_cpu.py).

Every comparison is bit for bit on uint32 views, NaN equal to NaN by position (test_gpu_clip_mix.differ), no tolerance.  The references
are loop_mix_ref, queue_mix_ref, clip_mix_ref (beyond what the whole stream can be built for: its windowed form), player_mix_ref,
spatial_mix_ref and wide_positions.mix.  dst lies in a guarded arena, 0 and 1 floats behind a 16-byte boundary: nothing stored outside
it, every word written.  Every source holds exactly the samples the block may read, between NaN, and is unchanged afterwards."""
import numpy as np
import pytest

import arena
import clip_mix_ref as CR
import loop_mix_ref as LR
import mix_edges as E
import queue_mix_ref as QR
import test_gpu_clip_mix as TC
import test_gpu_loop_mix as TL
import test_gpu_player_mix as PL
import test_gpu_queue_mix as TQ
import test_gpu_spatial_mix as SP
import test_gpu_wide_positions as WG
import wide_positions as W
from test_gpu_wide_positions import G  # noqa: F401  (the module fixture of the wide entries' tests: the package, initialised)

pytestmark = pytest.mark.gpu

UNSUPPORTED = 3
RATES = pytest.mark.parametrize("rate,to_rate", E.RATES_A, ids=[f"{a}-{b}" for a, b in E.RATES_A])
differ = TC.differ


def hold(run, mod, rh, c, want, leads=(0, 1), devs=None):
    """A case of mix_edges through `run` (a run_new of the entry's GPU file) at both leads against `want`; the sources unchanged."""
    devs = [mod.Dev(s) for s in c["srcs"]] if devs is None else devs
    for lead in leads:
        differ(run(rh, c["srcs"], devs, c["to_rate"], c["M"], c["ch"], lead), want, c["ch"], f"lead {lead}")
    for d in devs:
        d.unchanged()


def hold_loops(rh, c):
    hold(TL.run_new, TL, rh, c, LR.loop_mix(c["ch"], c["to_rate"], c["M"], c["srcs"]))


def hold_queues(rh, c):
    hold(TQ.run_new, TQ, rh, c, QR.queue_mix(c["ch"], c["to_rate"], c["M"], c["srcs"]))


def hold_clips(rh, c, windowed=False, leads=(0, 1)):
    hold(TC.run_new, TC, rh, c, CR.clip_mix(c["ch"], c["to_rate"], c["M"], c["srcs"], windowed), leads)


# ---- A: blocks longer than one sweep ------------------------------------------------------------------------------------------------------------
@RATES
@pytest.mark.parametrize("to_ch,alike", [(2, False), (5, False), (2, True)], ids=["into-stereo", "into-five", "alike-sources"])
def test_wide_mix_block_beyond_one_sweep(G, rate, to_rate, to_ch, alike):
    """Five sources, so a second group of four is entered, the fifth ending inside the third sweep; alike: the mixer's layout and one rate,
    the alike-sources kernel in front of the fifth one's end."""
    c = E.wide_long(rate, to_rate, to_ch, alike)
    blk = WG.Block(c["srcs"], to_rate, 0, c["M"])
    assert blk.plans[-1]["frames"] == c["end"] and all(p["frames"] == c["M"] for p in blk.plans[:-1])
    want = W.mix(c["srcs"], to_ch, to_rate, 0, c["M"])
    for lead in (0, 1):
        differ(WG.wide_block(blk, to_ch, to_rate, c["M"], lead), want, to_ch, f"rh_wide_mix_block, lead {lead}")
    blk.unchanged()


@RATES
def test_wide_mix_batch_with_a_mixer_shorter_than_a_sweep_and_one_longer_than_two(G, rate, to_rate):
    mixers = []
    for k, c in enumerate(E.batch_long(rate, to_rate)):
        mixers.append((c, WG.Block(c["srcs"], to_rate, 0, c["M"]), arena.dst_arena(c["M"] * c["ch"], k)))
    G.wide_mix_batch([m[2].ptr() for m in mixers], [m[0]["ch"] for m in mixers], [to_rate] * 2, [m[0]["M"] for m in mixers], [[m[1].arr[k] for k in range(m[1].n)] for m in mixers])
    for c, blk, dst in mixers:
        differ(dst.check(), W.mix(c["srcs"], c["ch"], to_rate, 0, c["M"]), c["ch"], f"rh_wide_mix_batch, the mixer of {c['M']} frames")
        blk.unchanged()


@RATES
@pytest.mark.parametrize("fast", [True, False], ids=["specialised", "general"])
def test_player_mix_block_beyond_one_sweep(rh, rate, to_rate, fast):
    """Stereo live sources of one rate on 8-byte boundaries into a stereo dst on one: the specialised kernel, 64 frames a workgroup; dst
    moved by 4 bytes: the general one, a lane a sample.  A ramp ends behind the first sweep of either."""
    c = E.player_long(rate, to_rate, fast)
    PL.hold(rh, c["srcs"], to_rate, c["M"], 2, leads=(0,) if fast else (1,), chain=False, src_lead=2)


@RATES
@pytest.mark.parametrize("fast", [True, False], ids=["mono-into-stereo", "six-into-five"])
def test_spatial_mix_block_beyond_one_sweep(rh, rate, to_rate, fast):
    """Mono emitters into stereo on an 8-byte boundary take the fast kernel; a six-channel source into five channels the general one."""
    c = E.spatial_long(rate, to_rate, fast)
    SP.hold(rh, c["srcs"], to_rate, c["M"], c["ch"], leads=(0,) if fast else (0, 1), chain=False)


@pytest.mark.parametrize("rate,to_rate,many", [(44100, 48000, False), (44100, 48000, True), (48000, 48000, False)], ids=["44100-48000", "44100-48000-33-sources", "48000-48000"])
def test_loop_mix_block_beyond_one_sweep(rh, rate, to_rate, many):
    """A rule-1 loop of 20 000 frames, a rule-0 loop of 9 and a plain source that ends in the third sweep; 33 sources: the second launch
    re-reads the sum the first one stored, behind the first sweep as in front of it."""
    hold_loops(rh, E.loop_long(rate, to_rate, many))


@pytest.mark.parametrize("to_rate", [48000, 44100])
def test_queue_mix_block_beyond_one_sweep(rh, to_rate):
    """A queue of 100 sounds of three formats with chain starts in every sweep, a plain source, and a queue that goes silent inside the
    second sweep: k_queue_mix's per-wave walk of the segments, re-entered at o >= 2^20."""
    hold_queues(rh, E.queue_long(to_rate))


@pytest.mark.parametrize("rate,to_rate,many", [(44100, 48000, False), (44100, 48000, True), (48000, 48000, False)], ids=["44100-48000", "44100-48000-33-sources", "48000-48000"])
def test_clip_mix_block_beyond_one_sweep(rh, rate, to_rate, many):
    """A fading rule-G clip behind an odd delay that ends inside the second sweep (its block spans 40 chains: the 64-bit fade), a rule-C
    clip, a clip still in its delay for the whole block and a plain source; 33 sources: two launches."""
    hold_clips(rh, E.clip_long(rate, to_rate, many))


# ---- B: positions in the upper half of 32 bits ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["chain", "pass"])
def test_a_loop_whose_pass_emits_more_than_2_31_frames(rh, which):
    """14 032 mono frames in chains of 255 at 100 -> 16 777 259 Hz: P = 2 344 789 782.  x0 >= 2^31 in chain 51, the block crossing its
    end; and the block in which x passes P and p wraps to 0."""
    c = E.big_loop_case(which)
    assert rh.loop_plan(E.BIG_LOOP["L"], 1, E.BIG_LOOP["c"]) == c["srcs"][0].words[:3] + [0, 0]
    hold_loops(rh, c)


@pytest.mark.parametrize("rule", [0, 1])
@pytest.mark.parametrize("c_frames", [255, 256])
def test_loops_with_j_f_above_2_31(rh, c_frames, rule):
    hold_loops(rh, E.edge_loops(c_frames, rule))


@pytest.mark.parametrize("rule", [0, 1])
def test_loops_with_j_f_above_2_31_under_a_small_reciprocal(rh, rule):
    """32 749 -> 131 071 Hz, T = 2^17 - 1: the only loops here whose division has the top bit of `x - t` set."""
    hold_loops(rh, E.below_loops(rule))


PAIRS = pytest.mark.parametrize("pair", E.EDGE_PAIRS, ids=["131074", "131071"])


@PAIRS
@pytest.mark.parametrize("which", E.EDGE_BLOCKS)
def test_a_clip_whose_chain_ends_next_to_the_bound(rh, which, pair):
    """32 749 -> 131 074 Hz, a mono chain of 32 768 frames: M F is 1443 below 2^32 - 1, j F of its last frames exceeds 2^32 - 2^16.  And
    -> 131 071 Hz, where T lies just below a power of two: the same heights with the top bit of div_u32's correction set."""
    hold_clips(rh, E.edge_clip_case(which, pair=pair))


@PAIRS
@pytest.mark.parametrize("which", E.EDGE_BLOCKS)
def test_a_queue_whose_chain_ends_next_to_the_bound(rh, which, pair):
    hold_queues(rh, E.edge_queue_case(which, pair=pair))


def test_the_neighbouring_rate_is_refused_and_nothing_is_written(rh):
    """The same clip and queue at 131 075 Hz: M F leaves 32 bits, RH_ERR_UNSUPPORTED, dst as it was."""
    for which in E.EDGE_BLOCKS:
        c = E.edge_clip_case(which, to_rate=E.OVER[1])
        devs = [TC.Dev(s) for s in c["srcs"]]
        dst = arena.dst_arena(c["M"] * 2, 0)
        assert TC.call(dst.ptr(), 2, E.OVER[1], c["M"], c["srcs"], devs) == UNSUPPORTED
        dst.check(written=0)
        # (the queue's cursor at the neighbouring rate cannot be worked out -- the chain is refused --: a fresh one)
        q = [QR.Src(c["M"], E.edge_queue_sounds(), [0, 0, 0, 1]), E.edge_plain(np.random.default_rng(1), E.EDGE[0], E.OVER[1], c["M"], src=QR.Src)]
        qdevs = [TQ.Dev(s) for s in q]
        assert TQ.call(dst.ptr(), 2, E.OVER[1], c["M"], q, qdevs) == UNSUPPORTED
        dst.check(written=0)
        for d in devs + qdevs:
            d.unchanged()


def test_rule_c_blocks_of_fit_minus_one_and_fit_frames(rh):
    """65 521 -> 65 519 Hz from the cursor with the largest phase: r0 + (frames - 1) F reaches 2^32 - 1 within F.  (fit + 1 frames are
    refused on the host: tests/cpp/clip_mix_plan_test.cpp and tests/test_mix_edges_cpu.py.)"""
    done, _, fit = E.fit_c()
    case = E.fit_c_clip()
    for frames in (fit - 1, fit):
        hold_clips(rh, dict(srcs=[case.src(frames, done)], M=frames, ch=2, to_rate=E.FIT_C.to_rate), leads=(frames % 2,))


# ---- C: the fade in 32 and in 64 bits -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frames", E.FADE_BLOCKS, ids=["eleven-chains-fade32", "a-frame-more-fade64", "twelve-chains-fade64"])
def test_the_fade_across_eleven_chains_a_frame_more_and_twelve(rh, frames):
    """describe() takes the 64-bit form from eleven chains and a frame on; the 32-bit one would be wrong from the twelfth chain's last
    7 000 frames on, which only the third block reads."""
    s = E.fade_clip().src(frames, 0)
    assert E.fade_mode(s, 48000) == (E.FADE32 if frames == E.FADE_BLOCKS[0] else E.FADE64) and E.fade_overflows(s, 48000) == (frames == E.FADE_BLOCKS[2])
    hold_clips(rh, dict(srcs=[s], M=frames, ch=2, to_rate=48000))


def test_a_take_beyond_2_32_ms_and_one_under_a_millisecond(rh):
    """ms0 alone forces the 64-bit form; under a millisecond x * 0 / 0: NaN by position."""
    for case in (E.long_take_clip(), E.short_take_clip()):
        s = case.src()
        want = CR.clip_mix(2, 48000, s.frames + 3, [s])
        assert np.isnan(want).any() == (case.take_ns < CR.NS_PER_MS)
        hold_clips(rh, dict(srcs=[s], M=s.frames + 3, ch=2, to_rate=48000))


# ---- D: cursors far from the stream's start -------------------------------------------------------------------------------------------------------
def test_a_rule_g_clip_behind_2_40_zeros(rh):
    """Deep in the delay (zrel saturates; the sound is a single NaN that nothing may read), the block in which the delay ends, the next
    one; the cursors are rh_clip_advance's."""
    x, words, dones = E.far_g()
    delay_ns = -(-words[1] * 10**9 // 88200)
    assert rh.clip_plan(x.size, 2, 44100, 0, delay_ns, words[3], True) == words[:5] + [0, 0]
    w = rh.clip_advance(words[:5] + [0, 0], 2, 44100, 48000, dones[0])
    assert w == CR.clip_advance_wide(words, 2, 44100, 48000, dones[0]) == words[:5] + [dones[0], words[6]]
    for k, done in enumerate(dones):
        assert w[5] == done
        s = CR.Src(x if k else np.zeros(0, np.float32), 2, 44100, 300, gain=0.8, words=w)
        want = CR.clip_mix_window(2, 48000, 300, [s])
        assert bool(want.any()) == (k > 0)
        hold_clips(rh, dict(srcs=[s], M=300, ch=2, to_rate=48000), windowed=True)
        step = (dones[k + 1] - done) if k + 1 < len(dones) else 300
        w = rh.clip_advance(w, 2, 44100, 48000, step)
        assert w == CR.clip_advance_wide(s.words, 2, 44100, 48000, step)


def test_rule_c_clips_behind_2_45_zeros_and_with_done_f_beyond_64_bits(rh):
    for (x, words, done), (rate, to_rate) in ((E.far_c(), (44100, 48000)), (E.far_c_128(), (E.FIT_C.from_rate, E.FIT_C.to_rate))):
        w = rh.clip_advance(words[:5] + [0, 0], 2, rate, to_rate, done)
        assert w == words[:5] + [done, words[6]]
        s = CR.Src(x, 2, rate, 300, gain=0.8, words=w)
        want = CR.clip_mix_window(2, to_rate, 300, [s])
        assert want[400:].any() and not want[:80].any(), "the sound starts inside the block"
        hold_clips(rh, dict(srcs=[s], M=300, ch=2, to_rate=to_rate), windowed=True)


def test_a_queue_cursor_inside_a_sound_of_50000_samples_in_three_unequal_blocks(rh):
    """chain_start = 32 768 inside the first sound, chain_out anywhere: the second chain reads on into the sounds behind.  Three blocks
    with rh_queue_advance's cursor hold the bits of the one pass."""
    sounds, M1 = E.far_queue()
    to_rate, M = 48000, 40000
    s = E.queue_at(M, sounds, True, M1 + 777, to_rate)
    whole = QR.queue_mix(2, to_rate, M, [s]).reshape(M, 2)
    devs = {id(q): arena.src_arena(q.x, 1) for q in sounds}
    state, w, at = s.sounds, s.words, 0
    left = E.PR.stream_out_frames(32768, 147, 160) - 777  # frames the chain in progress still emits: the second block is its verbatim last one
    for n in (left - 1, 1, M - left):
        assert w[2] == QR.PLAYING
        mine = [rh.QueueSound(devs[id(q)].ptr(), q.ch, q.rate, float(q.gain), samples=q.samples) for q in state]
        dst = arena.dst_arena(n * 2, at % 2)
        rh.queue_mix_block(dst.ptr(), 2, to_rate, n, [rh.QueueSrc(n, mine, w)])
        differ(dst.check(), whole[at:at + n].reshape(-1), 2, f"the block at {at}")
        got, dropped = rh.queue_advance(w, [rh.QueueSound(devs[id(q)].ptr(), q.ch, q.rate, samples=q.samples) for q in state], to_rate, n)
        assert (got, dropped) == QR.queue_advance(w, state, to_rate, n)
        state, w, at = state[dropped:], got, at + n
    for a in devs.values():
        a.unchanged()
