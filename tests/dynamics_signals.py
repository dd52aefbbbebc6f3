"""Signals and settings for the time-parallel limiter (rh_limit.hip) and the AGC (rh_agc.hip) beyond noise-like programme material, the f64
limiter they are measured against, and the criteria they are held to.  No HIP and no GPU: test_dynamics_signals_cpu.py holds the banks,
the restated variant pick, the residue signs, the twin of the AGC's default path and the premise of criterion C against the oracle and the
sources; test_gpu_dynamics_signals.py runs the kernels.

The limiter bank.  One channel each (the two pair_* streams are the exception: two channels that never occur on one), float64 rounded once to
float32.  The main event sits at frame 8192, a tile boundary of every k_limit_scan variant (tiles are 256 .. 8192 frames); a second event at
12287, the last frame of a 4096-frame tile; a burst ends at 6000, mid-tile.  "Quiet" is 1e-3, never 0: the gain stays observable on every
sample.  On these signals the reference's own f32 recurrences stall below their fixed points (P = a P + (1 - a) I on DC 2.0: 2.6e-6
relative, 5.1e-6 absolute, from the f64 evaluation of the same f32 coefficients; 1.0e-5 after a step to 4.0; 4e-7 on noise), which a
time-parallel evaluation -- a zero-state run plus a^k * start -- does not reproduce.  So, as for the filters (filter_signals.py), two criteria.

Errors are measured in the GAIN: with x_peak = max|x|, peak = max(1, x_peak),
    e = max |out - truth| / max(|x|, 1e-3 x_peak)        (e_gpu for the kernel, e_ref for the oracle)
    d = max |out - oracle| / peak
  B  e_gpu <= 2 e_ref + F, every case: no further from the exact response than rodio's own recurrence, give or take the roundings a
     time-parallel evaluation adds (F: limit_slack below, a derivation).
  C  d <= 1e-5 (the suite's TOL, scaled by peak like the filter contract's), every case but the ill-conditioned setting.  Its premise --
     rodio itself within 5e-6 * peak of the exact response, so that half of the tolerance is the kernel's -- is PROVED for every pair of
     the bank at every setting C is asserted on by test_dynamics_signals_cpu.py; C leaves out no case.

The AGC bank.  Each row is one AGC (all interleaved channels of a row share it).  Events at 8192 = one RMS window; the window sum of the
reference is sum = (sum - old) + new in f32, so after a fall to silence longer than the window it is a rounding RESIDUE:
    dc03_tail   0.3 (its square is inexact), silence from 8192:     residue > 0 (+3.9e-5): rms tiny, target / rms huge, clipped to the ceiling
    noise_tail  uniform noise (seed 0), silence from 8192:          residue < 0 (-1.85e-3): sqrt is NaN, `rms > 0` false, the ceiling again
    step_tail, tail_then_dc: exact squares, residue 0 (`rms > 0` false); tail_then_dc refills the emptied window from 3 * 8192 (sum 512)
    tone_tail   a tone, silence from 6000:                          residue > 0 (+3.3e-5)
RESIDUE_SIGN states the sign per signal; the CPU test proves it with a numpy-f32 window sum."""
import re

import numpy as np

RATE = 48000
EVENT = 8192      # a tile boundary of every k_limit_scan variant; one RMS window of the AGC
SECOND = 12287    # the last frame of a 4096-frame tile
BURST_END = 6000  # mid-tile
QUIET = 1e-3
TOL = 1e-5        # the suite's bound against the oracle


def _events(event):
    return event, SECOND * event // EVENT, BURST_END * event // EVENT


# ================================================================================================ the limiter ====
LIMIT_SIGNALS = ("noise", "dc", "dc_flip", "step_down", "step_up", "impulses", "tone", "burst", "nyquist", "knee_lo", "knee_hi")
PAIRS = ("pair_loud_quiet", "pair_swap")  # channel 0, channel 1: (dc, quiet), (step_down, step_up)

DEFAULT = dict(threshold=-1.0, knee_width=4.0, attack_ns=5_000_000, release_ns=100_000_000)  # rodio's (limit.rs:94-130)
SECOND_SETTING = dict(threshold=-6.0, knee_width=0.5, attack_ns=3_000_000, release_ns=12_000_000)
# name -> (parameters, held to C, cap).  The last one is outside what a limiter is used with and ill-conditioned in f32 (see
# test_limiter_lookback_walks_several_windows): criterion B only.
# cap: the bank is clipped to +-cap for that setting.  With a 20 ms attack 1 - a is 1.04e-3, and the reference's P = a P + (1 - a) I stops
# moving once (1 - a)(I - P) falls below half an ulp of P, 480 ulps under its fixed point: for P in [4, 8) dB (DC 2.0) that is 2.6e-5 of
# the gain, and the oracle alone is 1.08e-5 * peak from the exact response -- measured, 40 000 frames -- so it does not leave half of TOL to
# the kernel.  The premise of C is a statement about the INPUT; the condition stays, the level comes down: clipped to 0.98 every signal asks
# for at most 1 dB of reduction (inside the knee), P stays below 1 dB where an ulp is 6e-8, and the oracle is within 1.8e-6 * peak.
LIMIT_SETTINGS = {
    "default": (DEFAULT, True, None),
    "second": (SECOND_SETTING, True, None),
    "attack0": (dict(DEFAULT, attack_ns=0), True, None),
    "release0": (dict(DEFAULT, release_ns=0), True, None),
    "both0": (dict(DEFAULT, attack_ns=0, release_ns=0), True, None),        # memoryless: out = x * 10^(-g(x) / 20)
    "1ms-1ms": (dict(DEFAULT, attack_ns=1_000_000, release_ns=1_000_000), True, None),       # r^tile is negligible: the look-back ends at once
    "20ms-1s": (dict(DEFAULT, attack_ns=20_000_000, release_ns=1_000_000_000), True, 0.98),  # the look-back walks several tiles
    "800ms-3s": (dict(threshold=-9.0, knee_width=2.0, attack_ns=800_000_000, release_ns=3_000_000_000), False, None),
}


def limit_bank(frames, threshold=-1.0, knee_width=4.0, seed=0, event=EVENT, rate=RATE, cap=None):
    """name -> float32[frames], in the order of LIMIT_SIGNALS.  knee_lo / knee_hi: DC exactly at threshold -/+ knee / 2 dB, the two edges of
    the soft knee of the setting under test.  event: where the steps stand (8192; a shorter batch passes its own, the other events move
    with it).  cap: every signal clipped to +-cap (LIMIT_SETTINGS says where and why)."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames, dtype=np.float64)
    ev, second, burst_end = _events(event)
    tone = 2.0 * np.sin(2.0 * np.pi * 1000.0 * t / float(rate))
    out = {
        "noise": 2.0 * rng.uniform(-1.0, 1.0, frames),
        "dc": np.full(frames, 2.0),
        "dc_flip": np.where(t < ev, -2.0, 2.0),
        "step_down": np.where(t < ev, 4.0, QUIET),
        "step_up": np.where(t < ev, QUIET, 4.0),
        "impulses": np.where((t == 0) | (t == second), 8.0, QUIET),
        "tone": tone,
        "burst": np.where(t < burst_end, tone, QUIET),
        "nyquist": np.where(t % 2 == 0, 2.0, -2.0),
        "knee_lo": np.full(frames, 10.0 ** ((threshold - 0.5 * knee_width) / 20.0)),
        "knee_hi": np.full(frames, 10.0 ** ((threshold + 0.5 * knee_width) / 20.0)),
    }
    assert tuple(out) == LIMIT_SIGNALS
    if cap is not None:
        out = {k: np.clip(v, -float(cap), float(cap)) for k, v in out.items()}
    return {k: v.astype(np.float32) for k, v in out.items()}


def limit_stream_names(ch):
    """The streams of a launch: channel c of stream s carries signal (s + c) mod 11, as filter_signals.streams interleaves; with two
    channels the two pairs follow."""
    n = len(LIMIT_SIGNALS)
    names = []
    for s in range(n):
        part = [LIMIT_SIGNALS[(s + c) % n] for c in range(ch)]
        names.append("+".join(part) if ch <= 2 else f"{part[0]}..{part[-1]}")
    return names + (list(PAIRS) if ch == 2 else [])


def limit_streams(frames, ch, threshold=-1.0, knee_width=4.0, seed=0, event=EVENT, cap=None):
    """float32[S, frames * ch], interleaved; S = 11, or 13 with two channels (the pairs)."""
    b = limit_bank(frames, threshold, knee_width, seed, event, cap=cap)
    n = len(LIMIT_SIGNALS)
    rows = [[b[LIMIT_SIGNALS[(s + c) % n]] for c in range(ch)] for s in range(n)]
    if ch == 2:
        quiet = np.full(frames, QUIET, np.float32)
        rows += [[b["dc"], quiet], [b["step_down"], b["step_up"]]]
    x = np.empty((len(rows), frames, ch), np.float32)
    for s, row in enumerate(rows):
        for c in range(ch):
            x[s, :, c] = row[c]
    return x.reshape(len(rows), frames * ch)


# ---- the truth: limit.rs:853-988 in float64 on the f32 coefficients ---------------------------------------------------------------------------
def _coefficient(ns, rate):
    from rodio_amd import _lib  # (host arithmetic only: math.rs:110-113 in f32, as the kernels and the oracle get it)

    return float(_lib.lib.rh_duration_to_coefficient(int(ns), int(rate)))


def gain_computer_f64(x, threshold, knee_width):
    """limit.rs:853-873: the gain reduction in dB (>= 0) the level of x asks for."""
    bias = np.log2(np.abs(np.asarray(x, np.float64)) + 1.17549435e-38) * 0.30102999566398119521 * 20.0 - threshold
    kb = bias * 2.0
    return np.where(kb < -knee_width, 0.0, np.where(np.abs(kb) <= knee_width, (kb + knee_width) ** 2 / (8.0 * knee_width), bias))


def limit_truth(x, ch, rate, threshold=-1.0, knee_width=4.0, attack_ns=5_000_000, release_ns=100_000_000, state=None):
    """The limiter of every row of x [S, frames * ch] in float64 -> (out [S, frames * ch], final state [S, ch, 2] {integrator, peak}).
    One loop over the frames, vectorised over streams and channels: the integrator I = max(g, r I + (1 - r) g) per channel; the peak
    P = a P + (1 - a) I is linear in I (lfilter); the gain of channel c at frame n reads the channels' peaks as they stand when that sample
    is processed (limit.rs:946-960): this frame's for the channels up to c, the previous frame's for the others.  state: the start state."""
    from scipy.signal import lfilter

    att, rel = _coefficient(attack_ns, rate), _coefficient(release_ns, rate)
    x = np.asarray(x)
    S = x.shape[0]
    xv = x.astype(np.float64).reshape(S, -1, ch)
    n = xv.shape[1]
    g = gain_computer_f64(xv, threshold, knee_width)
    st = np.zeros((S, ch, 2)) if state is None else np.asarray(state, np.float64).reshape(S, ch, 2)
    integ = np.empty_like(g)
    cur = st[:, :, 0].copy()
    omr = 1.0 - rel
    for i in range(n):
        cur = np.maximum(g[:, i], rel * cur + omr * g[:, i])
        integ[:, i] = cur
    if n:
        peak, _ = lfilter([1.0 - att], [1.0, -att], integ, axis=1, zi=(att * st[:, :, 1])[:, None, :])
    else:
        peak = integ
    prev = np.concatenate([st[:, None, :, 1], peak[:, :-1]], axis=1)  # the previous frame's peaks
    seen = np.empty_like(peak)
    for c in range(ch):
        m = peak[:, :, : c + 1].max(axis=2)
        seen[:, :, c] = np.maximum(m, prev[:, :, c + 1:].max(axis=2)) if c + 1 < ch else m
    out = xv * 2.0 ** (-seen * 0.05 * 3.32192809488736234787)
    end = np.stack([cur, peak[:, -1] if n else st[:, :, 1]], axis=2)
    return out.reshape(S, -1), end


def limit_state_f32(x, ch, rate, threshold=-1.0, knee_width=4.0, attack_ns=5_000_000, release_ns=100_000_000):
    """The {integrator, peak} the reference's own recurrences leave behind, restated in numpy f32 in the reference's order (limit.rs:
    853-873, :909-913; the products rounded one by one) -> [S, ch, 2].  The oracle does not show its state; this is what the state a
    kernel leaves is measured against, beside the f64 one: the integrator is NOT observable in the output (with a 3 s release it carries
    ten times the rounding the gain shows), so the state's criterion B takes its e_ref from here.  (numpy's log2 is not bit for bit
    Rust's: the difference is one rounding of g, far inside what the recurrences accumulate.)"""
    f32 = np.float32
    att, rel = f32(_coefficient(attack_ns, rate)), f32(_coefficient(release_ns, rate))
    oma, omr = f32(1.0) - att, f32(1.0) - rel
    x = np.asarray(x, f32)
    S = x.shape[0]
    xv = x.reshape(S, -1, ch)
    thr, knee = f32(threshold), f32(knee_width)
    bias = np.log2(np.abs(xv) + f32(1.17549435e-38)) * f32(0.30102999566398119521) * f32(20.0) - thr
    kb = bias * f32(2.0)
    soft = (kb + knee) * (kb + knee) * (f32(1.0) / (f32(8.0) * knee))
    g = np.where(kb < -knee, f32(0.0), np.where(np.abs(kb) <= knee, soft, bias)).astype(f32)
    integ, peak = np.zeros((S, ch), f32), np.zeros((S, ch), f32)
    for i in range(xv.shape[1]):
        integ = np.maximum(g[:, i], rel * integ + omr * g[:, i])
        peak = att * peak + oma * integ
    return np.stack([integ, peak], axis=2)


def limit_f64(x, ch, rate, threshold=-1.0, knee_width=4.0, attack_ns=5_000_000, release_ns=100_000_000):
    """One stream: the ground truth an ill-conditioned setting is measured against (test_gpu_limit.py)."""
    return limit_truth(np.asarray(x)[None, :], ch, rate, threshold, knee_width, attack_ns, release_ns)[0][0]


def limit_memoryless(x, threshold=-1.0, knee_width=4.0):
    """Both durations 0 (both coefficients 0): I = g and P = I, the limiter has no memory -- one channel: out = x * 10^(-g(x) / 20) per
    sample, in f64.  (With more channels a sample still reads the previous frame's peaks of the channels behind it: limit_truth.)"""
    return np.asarray(x, np.float64) * 10.0 ** (-gain_computer_f64(x, threshold, knee_width) / 20.0)


# ---- the criteria -------------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -24          # the unit roundoff of f32
C_REF_SHARE = 5e-6      # rodio's own distance from the exact response that leaves half of TOL to the kernel
DB = np.log(10.0) / 20.0  # relative change of a gain per dB


def limit_roundings(R, NW, windows=1):
    """How many f32 roundings at the magnitude of the state (I or P, in dB) lie between a sample and the state its lane starts from in
    k_limit_scan, beyond those of the reference's own per-sample steps (which the lane-local runs repeat).  Every FMA `c * v + w` of the
    list rounds once and carries a table constant c = r^k that was rounded once: two units each.
        sub-wave, wave   the DPP scan: 4 row_shr steps + 2 broadcasts                                 6 FMAs, for I and for P
        workgroup        the prefix over the waves in front: at most NW - 1 compositions               NW - 1, for I and for P
        look-back        per window of 64 tiles: weight * aggregate, a 6-step wave sum, the fold       9 for I (candidate and fold), 8 for P
        correction       the wave's start state, the lane's start state                                2, for I and for P
        lane             P only: a^(r+1) Ps + Pz per sample, a^(r+1) by repeated multiplication        1 FMA + R roundings of the weight
        exp              the exponent max P * (-0.05 log2 10)                                          1
    All terms are non-negative and the weights at most 1, so every intermediate is at most the state's magnitude."""
    fma_i = 6 + (NW - 1) + 9 * windows + 2
    fma_p = 6 + (NW - 1) + 8 * windows + 2 + 1
    return 2 * (fma_i + fma_p) + R + 1


def limit_slack(x, threshold, knee_width, R=16, NW=8, windows=1):
    """F of criterion B, in the gain.  With G = max g(x) (the largest reduction in dB any sample asks for: I and P never exceed it),
    Gk = max(G, knee / 2) and L = max(|20 log10 x_peak|, |threshold| + knee / 2) (the levels of the samples that are not simply below
    the knee):
        states      limit_roundings(R, NW, windows) * U * G                                          dB
        gain comp.  v_log_f32 is 1 ulp = 2 U of |20 log10 |x||; the FMA onto the bias, 2 bias + knee, the square and its scale: 4 U of
                    Gk; d soft / d bias <= 1, and I and P are averages of g:  U (2 L + 4 Gk)           dB
        output      v_exp_f32 1 ulp = 2 U, the product x * gain U:  3 U                                relative
    F = U * (ln(10) / 20 * (N G + 2 L + 4 Gk) + 3).  Nothing in it is read off a GPU."""
    x = np.asarray(x, np.float64)
    x_peak = float(np.max(np.abs(x)))
    G = float(np.max(gain_computer_f64(x, threshold, knee_width)))
    Gk = max(G, 0.5 * knee_width)
    L = max(abs(20.0 * np.log10(x_peak)), abs(threshold) + 0.5 * knee_width)
    return U * (DB * (limit_roundings(R, NW, windows) * G + 2.0 * L + 4.0 * Gk) + 3.0)


def limit_state_slack(x, threshold, knee_width, R=16, NW=8, windows=1):
    """The same count for the {integrator, peak} a launch leaves behind, in dB: the states' roundings and the gain computer's of
    limit_slack, without what only the output has (the exponent's rounding, v_exp_f32, the product)."""
    x = np.asarray(x, np.float64)
    G = float(np.max(gain_computer_f64(x, threshold, knee_width)))
    Gk = max(G, 0.5 * knee_width)
    L = max(abs(20.0 * np.log10(float(np.max(np.abs(x))))), abs(threshold) + 0.5 * knee_width)
    return U * ((limit_roundings(R, NW, windows) - 1) * G + 2.0 * L + 4.0 * Gk)


def limit_measure(out, oracle, tru, x, F):
    """The figures of one stream: e_gpu, e_ref (gain), d (per unit of peak), a_ref = max|oracle - truth| / peak (the premise of C)."""
    out, oracle, tru, x = (np.asarray(a) for a in (out, oracle, tru, x))
    assert out.shape == oracle.shape == tru.shape == x.shape, (out.shape, oracle.shape, tru.shape, x.shape)
    assert np.isfinite(out).all(), "the kernel's output is not finite"
    x_peak = float(np.max(np.abs(x)))
    peak = max(1.0, x_peak)
    den = np.maximum(np.abs(x.astype(np.float64)), 1e-3 * x_peak)
    z = lambda a: float(np.max(np.abs(a))) if a.size else 0.0  # noqa: E731
    return {"d": z(out.astype(np.float64) - oracle) / peak, "e_gpu": z((out - tru) / den), "e_ref": z((oracle - tru) / den),
            "a_ref": z(oracle - tru) / peak, "peak": peak, "F": float(F)}


def limit_line(tag, m):
    return (f"[{tag}] |gpu-oracle|={m['d']:.3e} |gpu-f64|={m['e_gpu']:.3e} |oracle-f64|={m['e_ref']:.3e} peak={m['peak']:.3e} F={m['F']:.3e} "
            f"used={m['B_used']:+.2f} C={'yes' if m['C'] else 'no'}")


def limit_criteria(out, oracle, tru, x, F, tag="", contract=True, show=True):
    """Prints `|gpu-oracle| |gpu-f64| |oracle-f64| peak F` and the share of F the case uses, then asserts B (every case) and C (every setting
    but the ill-conditioned one: contract=False).  Returns the figures."""
    m = limit_measure(out, oracle, tru, x, F)
    m["C"] = bool(contract)
    m["B_used"] = (m["e_gpu"] - 2.0 * m["e_ref"]) / m["F"]  # (<= 0: inside 2 e_ref)
    if show:
        print(limit_line(tag, m))
    assert m["e_gpu"] <= 2.0 * m["e_ref"] + m["F"], ("B", tag, limit_line(tag, m))
    if contract:
        assert m["a_ref"] <= C_REF_SHARE, ("the premise of C", tag, limit_line(tag, m))
        assert m["d"] <= TOL, ("C", tag, limit_line(tag, m))
    return m


# ---- which k_limit_scan variant a call takes: rh::scan::pick_variant (rh_scan_launch.h) over kVariants (rh_limit.hip), restated ----------------
LV_VARIANTS = [(1, 8, 8), (1, 16, 8), (1, 16, 16), (1, 8, 1), (2, 8, 8), (2, 8, 16), (2, 8, 4), (2, 8, 1), (2, 16, 8), (2, 16, 4),
               (3, 4, 8), (3, 4, 1), (4, 4, 8), (4, 4, 1), (5, 4, 8), (5, 4, 1), (6, 4, 8), (6, 4, 1), (7, 4, 8), (7, 4, 1), (8, 4, 8), (8, 4, 1)]  # (C, R, NW)
LV_NIO = (2, 16, 6, 2)  # RH_LVIO: 6 computing + 2 I/O waves, tiles of 6144 frames


def lv_variants_in_source(text):
    return [tuple(int(v) for v in m) for m in re.findall(r"RH_LV\((\d+),\s*(\d+),\s*(\d+)\)", text)]


def lv_variant(ch, frames):
    """(R, NW) without a request, among the rows rh_limit allows (`!NIO && NW <= 8`): the longest tile (64 R NW frames) the stream fills
    at least half of; among equals more frames per lane; nothing fits: the shortest."""
    best = None
    for c, r, nw in LV_VARIANTS:
        if c != ch or nw > 8:
            continue
        if best is None:
            best = (r, nw)
            continue
        tc, tv = 64 * r * nw, 64 * best[0] * best[1]
        fc, fv = tc <= 2 * frames, tv <= 2 * frames
        better = fc if fc != fv else ((tc > tv or (tc == tv and r > best[0])) if fc else tc < tv)
        if better:
            best = (r, nw)
    return best


def lv_tile(ch, frames):
    r, nw = lv_variant(ch, frames)
    return 64 * r * nw


def lv_nio_gate(ch, frames):
    """RH_LIMIT_NIO=1 takes the I/O-wave variant where its 6144-frame tile is at least half full (and the layout has one: stereo)."""
    c, r, nw, _ = LV_NIO
    return ch == c and 64 * r * nw <= 2 * frames


def lv_skew_gate(ch, frames):
    """RH_LIMIT_SKEW=1 has a one-poll-point instantiation to force only for variants of at least four waves."""
    return lv_variant(ch, frames)[1] >= 4


# ---- the lengths the GPU test runs, the event each one places (a shorter batch scales the events down) and the variant it names ----------------
LIMIT_EVENTS = {700: 256, 2048: 1024, 3000: 1024, 20000: EVENT, 40000: EVENT}
# (channels, frames) -> (R, NW): 700 frames take the smallest tile of the layout, 3000 a mid tile, 20 000 three 8192-frame tiles (mono,
# stereo) or ten of 2048 (3 and 6 channels) with the events on and off their boundaries
LIMIT_NAMED = {(1, 700): (8, 1), (2, 700): (8, 1), (3, 700): (4, 1), (6, 700): (4, 1),
               (1, 3000): (8, 8), (2, 3000): (16, 4), (3, 3000): (4, 8), (6, 3000): (4, 8),
               (1, 20000): (16, 8), (2, 20000): (16, 8), (3, 20000): (4, 8), (6, 20000): (4, 8),
               (1, 40000): (16, 8), (2, 40000): (16, 8), (3, 40000): (4, 8), (6, 40000): (4, 8),
               (2, 2048): (16, 4)}


def limit_case(setting, ch, frames):
    """(parameters, held to C, input [S, frames * ch]) of one launch."""
    kw, contract, cap = LIMIT_SETTINGS[setting]
    return kw, contract, limit_streams(frames, ch, kw["threshold"], kw["knee_width"], event=LIMIT_EVENTS[frames], cap=cap)


def limit_F(x_row, kw, ch, lengths, variant=None, state=False):
    """F for one stream run in launches of the given lengths (one pass: its own; in blocks: the blocks' too): the largest count.
    variant: (R, NW) where the call does not take the pick (RH_LIMIT_NIO=1: LV_NIO's six computing waves, tiles of 6144 frames).
    state: the slack of the STATE left behind, in dB (limit_state_slack)."""
    worst = 0.0
    for n in lengths:
        r, nw = variant or lv_variant(ch, n)
        tiles = -(-n // (64 * r * nw))
        f = limit_state_slack if state else limit_slack
        worst = max(worst, f(x_row, kw["threshold"], kw["knee_width"], r, nw, -(-tiles // 64)))
    return worst


# ==================================================================================================== the AGC ====
AGC_SIGNALS = ("noise", "silence", "dc", "dc_quiet", "dc_loud", "step_tail", "tail_then_dc", "loud_step", "impulses", "tone", "tone_tail", "nyquist",
               "dc03_tail", "noise_tail")
WINDOW = 8192
NOISE_TAIL_SEED = 0
# the window sum once the window holds nothing but silence (samples 2 * 8192 on): > 0, < 0, or exactly 0
RESIDUE_SIGN = {"step_tail": 0, "tail_then_dc": 0, "tone_tail": +1, "dc03_tail": +1, "noise_tail": -1}

AGC_DEFAULT = dict(target_level=1.0, attack_ns=4_000_000_000, release_ns=0, absolute_max_gain=7.0, floor=0.0)
# name -> (parameters, the default path (release 0, floor <= ceiling: GainOp0)?)
AGC_SETTINGS = {
    "default": (AGC_DEFAULT, True),                                   # k_agc_fused0
    "attack5ms": (dict(AGC_DEFAULT, attack_ns=5_000_000), True),      # the gain reaches the ceiling and stalls under it: 6.999943
    "attack0": (dict(AGC_DEFAULT, attack_ns=0), True),                # gain = clamp(desired): the ceiling exactly
    "general": (dict(target_level=0.5, attack_ns=10_000_000, release_ns=5_000_000, absolute_max_gain=5.0, floor=0.2), False),  # the peak follower: a third chain
    "floor-above": (dict(target_level=0.7, attack_ns=4_000_000_000, release_ns=0, absolute_max_gain=5.0, floor=6.0), False),   # the host must leave GainOp0
}
AGC_ULPS = 2.0 ** -22  # |out - oracle| <= 2^-22 |oracle|: one ulp (2^-23) for the tie rh_agc.hip documents at GainOp0, one for the output
#                        product, times two; division and square root are correctly rounded under the build's flags (-fno-fast-math)


def agc_bank(n, seed=NOISE_TAIL_SEED, rate=RATE):
    """name -> float32[n], in the order of AGC_SIGNALS."""
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    noise_tail = np.where(t < WINDOW, rng.uniform(-1.0, 1.0, n), 0.0)  # (the first 8192 draws of seed 0: the residue the docstring states)
    tone = 0.5 * np.sin(2.0 * np.pi * 1000.0 * t / float(rate))
    out = {
        "noise": 0.5 * np.random.default_rng(seed + 1).uniform(-1.0, 1.0, n),
        "silence": np.zeros(n),
        "dc": np.full(n, 0.5),
        "dc_quiet": np.full(n, 0.01),
        "dc_loud": np.full(n, 20.0),  # target / 20 = 0.05: the floor clamp 0.1
        "step_tail": np.where(t < EVENT, 1.0, 0.0),
        "tail_then_dc": np.where(t < EVENT, 1.0, np.where(t < 3 * EVENT, 0.0, 0.25)),  # the window empties completely, then refills
        "loud_step": np.where(t < EVENT, 0.05, 20.0),
        "impulses": np.where((t == 0) | (t == SECOND), 1.0, 0.0),
        "tone": tone,
        "tone_tail": np.where(t < BURST_END, tone, 0.0),
        "nyquist": np.where(t % 2 == 0, 0.5, -0.5),
        "dc03_tail": np.where(t < EVENT, 0.3, 0.0),
        "noise_tail": noise_tail,
    }
    assert tuple(out) == AGC_SIGNALS
    return {k: v.astype(np.float32) for k, v in out.items()}


def agc_rows(n, seed=NOISE_TAIL_SEED):
    """float32[14, n]: one AGC per row."""
    b = agc_bank(n, seed)
    return np.stack([b[k] for k in AGC_SIGNALS])


def window_sums(x):
    """The reference's window sum (CircularBuffer::push, agc.rs:152-163) in numpy f32: sum = (sum - old) + sq, per row of x [S, n]."""
    x = np.asarray(x, np.float32)
    sq = x * x
    old = np.concatenate([np.zeros((x.shape[0], WINDOW), np.float32), sq[:, :-WINDOW]], axis=1)[:, : x.shape[1]] if x.shape[1] > WINDOW else np.zeros_like(sq)
    out = np.empty_like(sq)
    s = np.zeros(x.shape[0], np.float32)
    for i in range(x.shape[1]):
        s = (s - old[:, i]) + sq[:, i]
        out[:, i] = s
    return out


def agc_default_twin(x, rate, target_level=1.0, attack_ns=4_000_000_000, release_ns=0, absolute_max_gain=7.0, floor=0.0, wrong=None):
    """rh_agc.hip's default path restated in numpy f32, row by row of x [S, n]: agc_peak0 (the level is |x|, NaN with the sum),
    agc_desired1 (ONE division, by max(rms, peak); a level that is zero or NaN drops out of v_max_f32) and GainOp0 (select and both clamps
    as one median: gain' = med3(gain * attack + desired * (1 - attack), 0.1, clamp(desired, 0.1, max))).  For the CPU test only: it shows
    that the algebra of the shortcuts has the oracle's bits on this bank, so what the GPU test finds is the kernels'; the GPU test holds the
    gain word a run leaves behind to the gains returned here.  wrong: a deliberately wrong residue branch, for the CPU test that shows what
    sees it -- "nan": a NaN rms (negative residue) asks for gain 0 instead of the ceiling; "tiny": so does a positive residue."""
    assert release_ns == 0 and floor <= absolute_max_gain and absolute_max_gain >= 0.1
    f32 = np.float32
    x = np.asarray(x, f32)
    att = f32(_coefficient(min(attack_ns, 10_000_000_000), rate))
    oma = f32(1.0) - att
    target, maxg, lo, fl = f32(target_level), f32(absolute_max_gain), f32(0.1), f32(floor)
    sums = window_sums(x)
    with np.errstate(invalid="ignore", divide="ignore", over="ignore"):
        rms = np.sqrt(sums / f32(WINDOW))
        p = np.where(np.isnan(sums), sums, np.abs(x))
        m = np.fmax(rms, p)  # (v_max_f32: the operand that is a number)
        g = np.where(m > 0, np.fmin(target / np.where(m > 0, m, f32(1.0)), maxg), maxg)
        desired = np.fmax(g, fl)
        if wrong == "nan":
            desired = np.where(np.isnan(rms), fl, desired)
        if wrong == "tiny":
            desired = np.where((rms > 0) & (rms < f32(1e-3)) & (p == 0), fl, desired)
    dc = np.minimum(np.maximum(desired, lo), maxg)
    da = desired * oma
    gain = np.ones(x.shape[0], f32)
    gains = np.empty_like(x)
    for i in range(x.shape[1]):
        a = gain * att + da[:, i]
        gain = np.maximum(lo, np.minimum(a, dc[:, i]))  # med3(a, 0.1, dc) with 0.1 <= dc
        gains[:, i] = gain
    return x * gains, gains


def agc_check(out, oracle, x, tag="", show=True):
    """The suite's bound, and the sharper one in the gain on every sample.  Returns d = max|out - oracle| and the worst distance in ulps
    (2^-23) of the oracle's value."""
    out, oracle, x = np.asarray(out), np.asarray(oracle), np.asarray(x)
    assert out.shape == oracle.shape == x.shape and np.isfinite(out).all(), tag
    peak = max(1.0, float(np.max(np.abs(x)))) if x.size else 1.0
    ref = np.abs(oracle.astype(np.float64))
    d = np.abs(out.astype(np.float64) - oracle)
    m = {"d": float(d.max()) if d.size else 0.0, "peak": peak, "ulps": float(np.max(np.where(d > 0, d / np.maximum(ref, 1e-300), 0.0))) / 2.0 ** -23 if d.size else 0.0}
    if show:
        print(f"[{tag}] |gpu-oracle|={m['d']:.3e} peak={peak:.3e} ulps of the oracle's value={m['ulps']:.2f}")
    assert m["d"] <= TOL * peak, (tag, m)
    bad = np.flatnonzero(d > AGC_ULPS * ref)
    assert bad.size == 0, (tag, int(bad[0]), float(out.flat[bad[0]]), float(oracle.flat[bad[0]]), m)
    return m
