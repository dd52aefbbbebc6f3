"""Signals and filters for the time-parallel low_pass / high_pass (rh_biquad mode 1, the fused rh_rlm_* kernels, the streamed blocks) beyond
white noise and q = 0.5, and the two criteria they are held to.  No HIP and no GPU: test_filter_signals_cpu.py holds the bank, the table, the
restated predicates and the variant pick against the oracle and the sources; test_gpu_filter_signals.py runs the kernels.

The bank.  One channel each; every event sits at frame 8192 (a tile boundary of every variant of k_biquad_scan: tiles are 256 .. 8192 frames)
or in the middle of a tile.  On these signals the filter's state is coherent instead of averaging out, the zero-state response of a tile and
its look-back correction cancel at full size, and the tails behind a fall to silence run through thousands of subnormal samples that the
reference-order kernel has to reproduce bit for bit.

The table.  scan_basis() (rh_pipeline_internal.h, a copy in rh_biquad_scan.hip) has two branches: a complex pole pair where disc < 0 and
sqrt(-disc) / 2 > 1e-3, real (or numerically double) poles otherwise.  rodio's f32 coefficients for q = 0.5 have |disc| ~ 1e-7: the real
branch.  FILTERS covers distinct real poles (q < 0.5), the double pole, complex pairs up to q = 5, and a pair of rows either side of the
1e-3 edge.

The criteria, with peak = max(1, max|truth|), e_gpu = max|out - truth|, e_ref = max|oracle - truth| (truth: the f64 evaluation of the same
f32 coefficients):
  B  e_gpu <= 2 e_ref + F, F = 8 * 2^-24 * x_peak * gain: no further from the exact response than rodio's own recurrence, give or take a
     handful of f32 roundings (lane, sub-wave, wave, workgroup, look-back, correction, output) at the magnitude of the terms a time-parallel
     evaluation adds up -- at most x_peak * sum|h[k]|.  A derivation, not a measurement.
  C  max|out - oracle| <= 1e-5 * peak, asserted where the filter passes the gate (scan_ok) and rodio itself is within 5e-6 * peak of the
     exact response: half of the tolerance is then the kernel's.  Which pairs that leaves out is computed, never listed by hand."""
import re

import numpy as np

RATE = 48000
EVENT = 8192  # a tile boundary of every k_biquad_scan variant
SIGNALS = ("noise", "dc", "dc_flip", "dc_noise", "step_tail", "impulses", "tone", "tone_tail", "nyquist")


def bank(frames, freq, rate=RATE, seed=0, event=EVENT):
    """name -> float32[frames], one channel each, in the order of SIGNALS.  event: where the steps stand (8192; a batch shorter than that --
    the fused kernels' few tiles -- passes its own, and the other events move with it: 6000 and 12287 are for 8192)."""
    rng = np.random.default_rng(seed)
    t = np.arange(frames, dtype=np.float64)
    second, silent = 12287 * event // EVENT, 6000 * event // EVENT
    noise = rng.uniform(-1.0, 1.0, frames)
    tone = np.sin(2.0 * np.pi * float(freq) * t / float(rate))  # f64, rounded once below
    out = {
        "noise": noise,
        "dc": np.ones(frames),
        "dc_flip": np.where(t < event, -1.0, 1.0),
        "dc_noise": 0.9 + 0.1 * rng.uniform(-1.0, 1.0, frames),
        "step_tail": np.where(t < event, 1.0, 0.0),
        "impulses": np.where((t == 0) | (t == second), 1.0, 0.0),
        "tone": tone,
        "tone_tail": np.where(t < silent, tone, 0.0),
        "nyquist": np.where(t % 2 == 0, 1.0, -1.0),
    }
    assert tuple(out) == SIGNALS
    return {k: v.astype(np.float32) for k, v in out.items()}


def streams(frames, ch, freq, rate=RATE, seed=0, event=EVENT, names=SIGNALS):
    """float32[len(names), frames * ch], interleaved: channel c of stream s carries signal (s + c) mod len(names), so the channels of a frame
    differ."""
    b = bank(frames, freq, rate, seed, event)
    x = np.empty((len(names), frames, ch), np.float32)
    for s in range(len(names)):
        for c in range(ch):
            x[s, :, c] = b[names[(s + c) % len(names)]]
    return x.reshape(len(names), frames * ch)


def stream_name(s, ch, names=SIGNALS):
    part = [names[(s + c) % len(names)] for c in range(ch)]
    return "+".join(part) if ch <= 2 else f"{part[0]}..{part[-1]}"


# ---- the filters: (kind, freq, q, pole geometry, branch of scan_basis), at 48 kHz; every row passes the gate -------------------------------------
FILTERS = [
    ("low_pass", 1000, 0.3, "distinct", "real"),
    ("low_pass", 300, 0.35, "distinct", "real"),
    ("low_pass", 200, 0.5, "double", "real"),
    ("low_pass", 1000, 0.5, "double", "real"),
    ("high_pass", 600, 0.5, "double", "real"),
    ("high_pass", 20000, 0.5, "double", "real"),
    ("low_pass", 1000, 0.7071, "complex", "complex"),
    ("high_pass", 1000, 0.7071, "complex", "complex"),
    ("high_pass", 2000, 0.7071, "complex", "complex"),
    ("low_pass", 800, 2.0, "complex", "complex"),
    ("low_pass", 5000, 5.0, "complex", "complex"),
    ("high_pass", 5000, 3.0, "complex", "complex"),
    ("low_pass", 20000, 0.7071, "complex", "complex"),
    ("low_pass", 1000, 0.50001, "edge", "real"),      # nu = 7.2e-4
    ("low_pass", 1000, 0.50003, "edge", "complex"),   # nu = 1.25e-3
]
EDGE_NU = 1e-3


def filter_id(row):
    return f"{row[0]}{row[1]}-q{row[2]}"


def discriminant(coeffs):
    a1, a2 = float(coeffs[3]), float(coeffs[4])
    return a1 * a1 - 4.0 * a2


def scan_nu(coeffs):
    """rho sin(theta) of a complex pair (0 for real poles): what scan_basis compares with 1e-3."""
    d = discriminant(coeffs)
    return float(np.sqrt(-d)) * 0.5 if d < 0.0 else 0.0


def scan_branch(coeffs):
    """scan_basis's predicate (rh_pipeline_internal.h): "complex" or "real"."""
    d = discriminant(coeffs)
    return "complex" if d < 0.0 and float(np.sqrt(-d)) * 0.5 > EDGE_NU else "real"


def pole_radius(coeffs):
    a1, a2 = float(coeffs[3]), float(coeffs[4])
    d = a1 * a1 - 4.0 * a2
    if d >= 0.0:
        sq = float(np.sqrt(d))
        return max(abs((-a1 + sq) / 2.0), abs((-a1 - sq) / 2.0))
    return float(np.sqrt(a2)) if a2 > 0.0 else 0.0


def scan_ok(kind, coeffs):
    """filter_scan_ok_coeffs (rh_recurrence.hip): low_pass 1 - r >= 0.0125, high_pass 1 - r >= 0.075."""
    return (1.0 - pole_radius(coeffs)) >= (0.0125 if kind in (0, "low_pass") else 0.075)


# ---- the reference values -------------------------------------------------------------------------------------------------------------------
def truth(coeffs, x, ch):
    """scipy.signal.lfilter in f64 on the f32 coefficients, per channel of the interleaved x."""
    from scipy.signal import lfilter

    co = np.asarray(coeffs, np.float32).astype(np.float64)
    r = np.asarray(x).astype(np.float64).reshape(-1, ch)
    y = lfilter(co[:3], [1.0, co[3], co[4]], r, axis=0) if len(r) else r
    return y.reshape(-1)


def l1_gain(coeffs):
    """sum |h[k]| of the f64 impulse response, summed until the terms fall below 1e-18."""
    n = 1 << 12
    while True:
        imp = np.zeros(n)
        imp[0] = 1.0
        h = np.abs(truth(coeffs, imp, 1))
        if float(np.max(h[-64:])) < 1e-18 or n >= 1 << 24:
            return float(np.sum(h[h >= 1e-18]))
        n *= 4


# ---- the criteria -----------------------------------------------------------------------------------------------------------------------------
F_FACTOR = 8.0
C_TOL = 1e-5       # the contract against rodio, per unit of peak
C_REF_SHARE = 5e-6  # rodio's own distance from the exact response that leaves half of C_TOL to the kernel


def slack(x_peak, gain):
    return F_FACTOR * 2.0 ** -24 * float(x_peak) * float(gain)


def measure(out, oracle, tru, x_peak, gain):
    out, oracle, tru = np.asarray(out), np.asarray(oracle), np.asarray(tru)
    assert out.shape == oracle.shape == tru.shape, (out.shape, oracle.shape, tru.shape)
    assert np.isfinite(out).all(), "the kernel's output is not finite"
    z = lambda a: float(np.max(np.abs(a))) if a.size else 0.0  # noqa: E731
    peak = max(1.0, z(tru))
    return {"d": z(out.astype(np.float64) - oracle), "e_gpu": z(out - tru), "e_ref": z(oracle - tru), "peak": peak, "F": slack(x_peak, gain)}


def contract_applies(e_ref, peak, gate):
    return bool(gate) and e_ref <= C_REF_SHARE * peak


def line(tag, m):
    return (f"[{tag}] |gpu-oracle|={m['d']:.3e} |gpu-f64|={m['e_gpu']:.3e} |oracle-f64|={m['e_ref']:.3e} peak={m['peak']:.3e} F={m['F']:.3e} "
            f"C={'yes' if m['C'] else 'no'}")


def criteria(out, oracle, tru, x_peak, gain, tag="", gate=True, show=True):
    """Prints `|gpu-oracle| |gpu-f64| |oracle-f64| peak F` (show=False: the caller prints, e.g. the worst of a group), then asserts B (every
    case) and C (where it applies).  Returns the figures."""
    m = measure(out, oracle, tru, x_peak, gain)
    m["C"] = contract_applies(m["e_ref"], m["peak"], gate)
    m["B_used"] = (m["e_gpu"] - 2.0 * m["e_ref"]) / m["F"]  # share of F the case uses (<= 0: inside 2 e_ref)
    if show:
        print(line(tag, m))
    assert m["e_gpu"] <= 2.0 * m["e_ref"] + m["F"], ("B", tag, line(tag, m))
    if m["C"]:
        assert m["d"] <= C_TOL * m["peak"], ("C", tag, line(tag, m))
    return m


# ---- which k_biquad_scan variant a call takes: rh::scan::pick_variant (rh_scan_launch.h) over kVariants (rh_biquad_scan.hip), restated -------
BQ_VARIANTS = [(1, 16, 8), (1, 16, 1), (2, 8, 8), (2, 16, 8), (2, 8, 4), (2, 8, 1), (3, 4, 8), (3, 4, 1), (4, 4, 8), (4, 4, 1), (5, 4, 8), (5, 4, 1),
               (6, 4, 8), (6, 4, 1), (7, 4, 8), (7, 4, 1), (8, 4, 8), (8, 4, 1)]  # (C, R, NW)


def bq_variants_in_source(text):
    return [tuple(int(v) for v in m) for m in re.findall(r"RH_BV\((\d+),\s*(\d+),\s*(\d+)\)", text)]


def bq_variant(ch, frames):
    """(R, NW) without a request: the longest tile (64 R NW frames) the stream fills at least half of; among equals more frames per lane;
    nothing fits: the shortest."""
    best = None
    for c, r, nw in BQ_VARIANTS:
        if c != ch:
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


def bq_tile(ch, frames):
    r, nw = bq_variant(ch, frames)
    return 64 * r * nw
