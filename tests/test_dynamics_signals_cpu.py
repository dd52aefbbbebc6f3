"""What test_gpu_dynamics_signals.py rests on (dynamics_signals.py), pinned on the CPU with the oracle alone, so that the banks cannot quietly
stop testing anything: the signals are what the module says (event frames, no exact zero in the limiter bank, both signs of the window-sum
residue), the restated RH_LV rows and the pick are rh_limit.hip's, the premise of criterion C holds for EVERY pair of the limiter bank at
every setting C is asserted on, the oracle's AGC reaches the floor clamp and stalls under the ceiling where the module says, and the
numpy-f32 twin of the AGC's default path (agc_peak0 + agc_desired1 + GainOp0) has the oracle's bits on the whole bank.  The printed
table of e_ref is the CPU half of profiles/dynamics_signals.txt."""
import os

import numpy as np
import pytest
from dynamics_signals import (AGC_SETTINGS, AGC_SIGNALS, AGC_ULPS, C_REF_SHARE, LIMIT_EVENTS, LIMIT_NAMED, LIMIT_SETTINGS, LIMIT_SIGNALS, LV_NIO, LV_VARIANTS, PAIRS,
                              QUIET, RATE, RESIDUE_SIGN, TOL, WINDOW, agc_bank, agc_check, agc_default_twin, agc_rows, gain_computer_f64, limit_bank, limit_case,
                              limit_criteria, limit_F, limit_f64, limit_measure, limit_memoryless, limit_roundings, limit_stream_names, limit_streams,
                              limit_truth, lv_nio_gate, lv_skew_gate, lv_tile, lv_variant, lv_variants_in_source, window_sums)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_AGC = 40000


def _limit_oracle(O, x, ch, kw):
    return np.stack([O.TestSource(x[s], ch, RATE).limit(**kw).collect() for s in range(x.shape[0])])


def _agc_oracle(O, x, kw):
    return np.stack([O.TestSource(x[s], 1, RATE).automatic_gain_control(**kw).collect() for s in range(x.shape[0])])


@pytest.fixture(scope="module")
def agc_refs(O):
    """setting -> (input [14, 40 000], oracle [14, 40 000]), computed once, read-only."""
    x = agc_rows(N_AGC)
    x.setflags(write=False)
    out = {}
    for name, (kw, _) in AGC_SETTINGS.items():
        ref = _agc_oracle(O, x, kw)
        ref.setflags(write=False)
        out[name] = (x, ref)
    return out


# ================================================================================================ the banks ====
def test_the_limiter_bank_is_what_it_says():
    n = 20000
    b = limit_bank(n)
    assert tuple(b) == LIMIT_SIGNALS and all(v.dtype == np.float32 and v.shape == (n,) for v in b.values())
    for name, v in b.items():
        assert np.all(v != 0) or name in ("tone", "burst", "noise"), name  # quiet is 1e-3, never 0 ...
    assert b["tone"][0] == 0 and np.count_nonzero(b["tone"] == 0) <= n // 24 + 1 and np.all(b["noise"] != 0)  # ... but a sine crosses zero
    q = np.float32(QUIET)
    assert np.all(b["dc"] == 2.0) and np.all(b["dc_flip"][:8192] == -2.0) and np.all(b["dc_flip"][8192:] == 2.0)
    assert np.all(b["step_down"][:8192] == 4.0) and np.all(b["step_down"][8192:] == q)
    assert np.all(b["step_up"][:8192] == q) and np.all(b["step_up"][8192:] == 4.0)
    assert np.flatnonzero(b["impulses"] == 8.0).tolist() == [0, 12287] and np.all(np.delete(b["impulses"], [0, 12287]) == q)
    assert np.array_equal(b["burst"][:6000], b["tone"][:6000]) and np.all(b["burst"][6000:] == q) and b["tone"][12] == np.float32(2.0)
    assert np.array_equal(b["nyquist"][:4], np.float32([2, -2, 2, -2])) and 1.999 < float(np.abs(b["noise"]).max()) <= 2.0
    # the knee's two edges, for the setting under test: g = 0 at the lower one, knee / 2 at the upper one
    for thr, knee in ((-1.0, 4.0), (-6.0, 0.5), (-9.0, 2.0)):
        k = limit_bank(64, thr, knee)
        assert abs(float(gain_computer_f64(k["knee_lo"], thr, knee)[0])) < 1e-6 and abs(float(gain_computer_f64(k["knee_hi"], thr, knee)[0]) - knee / 2) < 1e-5
        assert np.all(k["knee_lo"] == k["knee_lo"][0]) and k["knee_lo"][0] < k["knee_hi"][0]
    # the events of a shorter batch move with its own
    s = limit_bank(700, event=256)
    assert np.flatnonzero(s["impulses"] == 8.0).tolist() == [0, 383] and np.all(s["step_up"][:256] == q) and s["step_up"][256] == 4.0 and s["burst"][187] == q != s["burst"][186]
    # the streams: channel c of stream s carries signal (s + c) mod 11; two channels add the pairs
    for ch in (1, 2, 3, 6):
        x = limit_streams(100, ch)
        assert x.shape == (11 + 2 * (ch == 2), 100 * ch) and len(limit_stream_names(ch)) == x.shape[0]
        for st in range(11):
            for c in range(ch):
                assert np.array_equal(x[st].reshape(100, ch)[:, c], limit_bank(100)[LIMIT_SIGNALS[(st + c) % 11]])
    x = limit_streams(n, 2).reshape(13, n, 2)
    assert limit_stream_names(2)[-2:] == list(PAIRS) and limit_stream_names(2)[10] == "knee_hi+noise"
    assert np.array_equal(x[11, :, 0], b["dc"]) and np.all(x[11, :, 1] == q) and np.array_equal(x[12, :, 0], b["step_down"]) and np.array_equal(x[12, :, 1], b["step_up"])
    # the capped bank of the 20 ms / 1 s setting: nothing above 0.98, at most 1 dB of reduction, still never 0 where it was not
    kw, contract, xc = limit_case("20ms-1s", 2, 700)
    assert contract and float(np.abs(xc).max()) == float(np.float32(0.98)) and 0.9 < float(gain_computer_f64(xc, kw["threshold"], kw["knee_width"]).max()) < 1.0


def test_the_agc_bank_is_what_it_says_and_the_residues_have_both_signs():
    n = N_AGC
    b = agc_bank(n)
    assert tuple(b) == AGC_SIGNALS and all(v.dtype == np.float32 and v.shape == (n,) for v in b.values())
    assert not b["silence"].any() and np.all(b["dc"] == 0.5) and np.all(b["dc_quiet"] == np.float32(0.01)) and np.all(b["dc_loud"] == 20.0)
    assert np.all(b["step_tail"][:8192] == 1.0) and not b["step_tail"][8192:].any()
    t = b["tail_then_dc"]
    assert np.all(t[:8192] == 1.0) and not t[8192:3 * 8192].any() and np.all(t[3 * 8192:] == 0.25)
    assert np.all(b["loud_step"][:8192] == np.float32(0.05)) and np.all(b["loud_step"][8192:] == 20.0)
    assert np.flatnonzero(b["impulses"]).tolist() == [0, 12287]
    assert not b["tone_tail"][6000:].any() and np.array_equal(b["tone_tail"][:6000], b["tone"][:6000]) and b["tone"][12] == 0.5
    assert np.all(b["dc03_tail"][:8192] == np.float32(0.3)) and not b["dc03_tail"][8192:].any()
    assert not b["noise_tail"][8192:].any() and np.all(b["noise_tail"][:8192] != 0) and 0.999 < float(np.abs(b["noise_tail"]).max()) <= 1.0
    assert np.all(b["noise"] != 0) and 0.499 < float(np.abs(b["noise"]).max()) <= 0.5  # (never an exactly silent sample: what the noise tests have)
    # the window sums, sum = (sum - old) + sq in f32: once the window holds nothing but silence they are the residues the module states
    names = list(RESIDUE_SIGN)
    ws = window_sums(np.stack([b[k] for k in names]))
    for i, k in enumerate(names):
        hi = 3 * WINDOW if k == "tail_then_dc" else n
        res = ws[i, 2 * WINDOW: hi]
        assert np.all(res == res[0]), k  # silence in, silence out: the sum no longer moves
        print(f"[residue] {k}: {float(res[0]):+.4e}")
        assert np.sign(res[0]) == RESIDUE_SIGN[k], (k, float(res[0]))
    assert set(RESIDUE_SIGN.values()) == {-1, 0, 1}
    assert 3.5e-5 < float(ws[names.index("dc03_tail"), -1]) < 4.5e-5 and -2.0e-3 < float(ws[names.index("noise_tail"), -1]) < -1.7e-3
    assert float(ws[names.index("tail_then_dc"), -1]) == 512.0  # the emptied window, refilled: 8192 * 0.25^2, exact


# ==================================================================================== the variant pick, restated ====
def test_the_restated_variants_are_the_sources():
    src = open(os.path.join(ROOT, "rodio_amd", "csrc", "rh_limit.hip")).read()
    assert lv_variants_in_source(src) == LV_VARIANTS  # (the macro's own definition has no digits: the regex skips it)
    assert f"RH_LVIO({LV_NIO[0]}, {LV_NIO[1]}, {LV_NIO[2]}, {LV_NIO[3]})" in src
    assert "[](const LimitVariant &c) { return !c.NIO && c.NW <= 8; }" in src                       # the predicate of a call without a request
    assert "c.NIO && c.C == (int)channels && (uint64_t)64 * c.R * c.NW <= 2 * frames" in src          # RH_LIMIT_NIO=1: the 6144-frame tile half full
    assert "(nw) >= 4 ? &k_limit_scan<c, r, nw, ((nw) >= 4)> : nullptr" in src                       # RH_LIMIT_SKEW=1: at least four waves
    assert "tile_of(c) <= 2 * frames" in open(os.path.join(ROOT, "rodio_amd", "csrc", "rh_scan_launch.h")).read()
    # the variants the GPU test names
    for (ch, frames), want in LIMIT_NAMED.items():
        assert lv_variant(ch, frames) == want and frames in LIMIT_EVENTS, (ch, frames, lv_variant(ch, frames))
    assert [lv_tile(c, 700) for c in (1, 2, 3, 6)] == [512, 512, 256, 256] and [lv_tile(c, 3000) for c in (1, 2, 3, 6)] == [4096, 4096, 2048, 2048]
    assert [lv_tile(c, 20000) for c in (1, 2, 3, 6)] == [8192, 8192, 2048, 2048]
    # the blocks of the state test: whole 8192-frame tiles in front of the cut, and what is left behind it
    assert [lv_variant(2, n) for n in (8191, 8192, 8193, 12288, 20000 - 8191, 20000 - 12288, 3807)] == [(16, 8)] * 6 + [(16, 4)]
    assert lv_nio_gate(2, 20000) and lv_nio_gate(2, 3072) and not lv_nio_gate(2, 3071) and not lv_nio_gate(1, 20000)
    assert lv_skew_gate(2, 20000) and lv_skew_gate(2, 3000) and not lv_skew_gate(2, 700)
    assert limit_roundings(16, 8) == 2 * (24 + 24) + 16 + 1 and limit_roundings(4, 1) < limit_roundings(16, 8) < limit_roundings(16, 8, 2)


# ================================================================================== the limiter's truth and criteria ====
def test_the_f64_limiter_is_the_one_the_suite_had_and_the_memoryless_form(O):
    """limit_truth (one loop over the frames, vectorised over streams and channels, the channels' peaks read in the reference's order)
    against the per-sample, per-channel loop test_gpu_limit.py carried; a state handed from one block to the next; both durations 0."""
    from rodio_amd import _lib

    kw = dict(threshold=-9.0, knee_width=2.0, attack_ns=800_000_000, release_ns=3_000_000_000)
    att = float(_lib.lib.rh_duration_to_coefficient(kw["attack_ns"], RATE))
    rel = float(_lib.lib.rh_duration_to_coefficient(kw["release_ns"], RATE))
    for ch in (1, 2, 3):
        x = limit_streams(1500, ch, kw["threshold"], kw["knee_width"], event=1024)
        tru, end = limit_truth(x, ch, RATE, **kw)
        for s in (0, 3, x.shape[0] - 1):
            xv = x[s].astype(np.float64).reshape(-1, ch)
            g = gain_computer_f64(xv, kw["threshold"], kw["knee_width"])
            integ, peak, out = np.zeros(ch), np.zeros(ch), np.empty_like(xv)
            for n in range(xv.shape[0]):
                for c in range(ch):
                    integ[c] = max(g[n, c], rel * integ[c] + (1.0 - rel) * g[n, c])
                    peak[c] = att * peak[c] + (1.0 - att) * integ[c]
                    out[n, c] = xv[n, c] * 2.0 ** (-peak.max() * 0.05 * 3.32192809488736234787)
            assert float(np.max(np.abs(out.reshape(-1) - tru[s]))) <= 1e-13 and np.allclose(end[s], np.stack([integ, peak], axis=1), rtol=0, atol=1e-12)
            assert np.array_equal(limit_f64(x[s], ch, RATE, **kw), tru[s])
        a, st = limit_truth(x[:, : 700 * ch], ch, RATE, **kw)
        b, st2 = limit_truth(x[:, 700 * ch:], ch, RATE, state=st, **kw)
        assert float(np.max(np.abs(np.concatenate([a, b], axis=1) - tru))) <= 1e-13 and np.allclose(st2, end, rtol=0, atol=1e-12)
    kw0 = LIMIT_SETTINGS["both0"][0]
    x = limit_streams(3000, 1, event=1024)
    assert float(np.max(np.abs(limit_truth(x, 1, RATE, **kw0)[0] - limit_memoryless(x)))) <= 1e-15
    ref = _limit_oracle(O, x, 1, kw0)
    assert float(np.max(np.abs(ref - limit_memoryless(x)))) <= 2e-6  # the oracle has no memory either


@pytest.mark.parametrize("setting", list(LIMIT_SETTINGS))
def test_criterion_c_applies_to_every_pair_it_is_asserted_on(O, setting):
    """e_ref = max|oracle - truth| per (signal, setting): mono at 30 000 frames (every signal on its own), stereo at 20 000 (the pairs, and
    the channel coupling), 40 000 for the setting that runs that long.  The premise of C -- e_ref <= 5e-6 * peak -- holds for every one of
    them at every setting but the ill-conditioned one, which is why C may leave out no case."""
    kw, contract, cap = LIMIT_SETTINGS[setting]
    worst = 0.0
    for ch, frames in ((1, 30000), (2, 20000)) + (((1, 40000), (2, 40000)) if setting == "20ms-1s" else ()):
        x = limit_streams(frames, ch, kw["threshold"], kw["knee_width"], cap=cap)
        tru, _ = limit_truth(x, ch, RATE, **kw)
        ref = _limit_oracle(O, x, ch, kw)
        assert np.isfinite(ref).all() and np.isfinite(tru).all()
        for s, name in enumerate(limit_stream_names(ch)):
            m = limit_measure(ref[s], ref[s], tru[s], x[s], limit_F(x[s], kw, ch, [frames]))
            print(f"[e_ref] {setting:9s} ch{ch} n{frames} {name:22s} |oracle-f64|={m['a_ref'] * m['peak']:.3e} per peak={m['a_ref']:.3e} in the gain={m['e_ref']:.3e} F={m['F']:.3e}")
            worst = max(worst, m["a_ref"])
            if contract:
                assert m["a_ref"] <= C_REF_SHARE, (setting, ch, name, m)
                limit_criteria(ref[s], ref[s], tru[s], x[s], m["F"], show=False)  # (the oracle against itself: B and C hold trivially)
    if not contract:
        assert worst > 2.0 * TOL, worst  # ill-conditioned: the reference alone is further from the exact response than the whole tolerance
    if setting == "second":
        assert 2.5e-6 < worst < 3.5e-6, worst  # the worst of the settings C is asserted on: dc, 2.9e-6 * peak


def test_what_the_limiter_criteria_are_worth(O):
    """A release tail 0.5 % off in the gain passes the flat 1e-5 the noise tests use and fails B; the exact response, rounded once, is inside F."""
    kw = LIMIT_SETTINGS["default"][0]
    x = limit_streams(20000, 1)
    tru, _ = limit_truth(x, 1, RATE, **kw)
    s = LIMIT_SIGNALS.index("step_down")
    ref = _limit_oracle(O, x[s: s + 1], 1, kw)[0]
    F = limit_F(x[s], kw, 1, [20000])
    ok = limit_criteria(tru[s].astype(np.float32), ref, tru[s], x[s], F, show=False)
    assert ok["e_gpu"] <= 2.0 ** -24 * 1.01 < F
    bad = tru[s].copy()
    bad[8192:] *= 1.005
    bad = bad.astype(np.float32)
    assert float(np.max(np.abs(bad - ref)[8192:])) <= 0.6 * TOL  # invisible to |gpu - oracle| <= 1e-5 ...
    with pytest.raises(AssertionError):
        limit_criteria(bad, ref, tru[s], x[s], F, show=False)  # ... and a thousand times F to criterion B


# ==================================================================================================== the AGC ====
def _gain(ref, x, i):
    return float(ref[i]) / float(x[i])


def test_the_oracles_agc_reaches_the_floor_clamp_and_stalls_under_the_ceiling(O, agc_refs):
    for name, (x, ref) in agc_refs.items():
        assert np.isfinite(ref).all(), name
    loud, step, quiet = (AGC_SIGNALS.index(k) for k in ("dc_loud", "loud_step", "dc_quiet"))
    for name in ("default", "attack5ms", "attack0"):
        x, ref = agc_refs[name]
        for i in (loud, step):  # the floor clamp 0.1: target / 20 = 0.05
            assert ref[i, -1] == np.float32(20.0) * np.float32(0.1), (name, i, float(ref[i, -1]))
    # the gain on silence is not in the output (0 * gain): a last sample of 0.01 behind the silence shows it
    probe = np.zeros(20000, np.float32)
    probe[-1] = 0.01
    q = np.float32(0.01)
    g5 = O.TestSource(probe, 1, RATE).automatic_gain_control(**AGC_SETTINGS["attack5ms"][0]).collect()[-1]
    g0 = O.TestSource(probe, 1, RATE).automatic_gain_control(**AGC_SETTINGS["attack0"][0]).collect()[-1]
    assert q * np.float32(6.9999) < g5 < q * np.float32(7.0), float(g5)  # stalled under the ceiling: f32 rounding that is part of rodio's output
    assert g0 == q * np.float32(7.0)
    # ... and dc_quiet (target / 0.01 = 100: the ceiling) shows the same on every sample
    x, ref = agc_refs["attack5ms"]
    tail = ref[quiet, 8192:].astype(np.float64) / 0.01
    assert np.all(ref[quiet, 8192:] == ref[quiet, -1]) and 6.9999 < float(tail[-1]) < 6.99999, float(tail[-1])
    x, ref = agc_refs["attack0"]
    assert np.all(ref[quiet] == q * np.float32(7.0))
    # both residue branches end at the ceiling: a sample behind the tail comes out times 7 with attack 0
    for k in ("dc03_tail", "noise_tail"):
        xs = agc_bank(3 * WINDOW)[k].copy()
        xs[-1] = 0.01
        assert O.TestSource(xs, 1, RATE).automatic_gain_control(**AGC_SETTINGS["attack0"][0]).collect()[-1] == q * np.float32(7.0), k
    # what the sharper bound sees and the suite's does not: a kernel that reached the ceiling exactly
    x, ref = agc_refs["attack5ms"]
    reached = ref[quiet].copy()
    reached[8192:] = x[quiet, 8192:] * np.float32(7.0)
    assert float(np.max(np.abs(reached[8192:] - ref[quiet, 8192:]))) < 1e-6 < TOL
    assert np.all(np.abs(reached[8192:].astype(np.float64) - ref[quiet, 8192:]) > AGC_ULPS * np.abs(ref[quiet, 8192:]))
    with pytest.raises(AssertionError):
        agc_check(reached, ref[quiet], x[quiet], "a gain of exactly 7.0")
    agc_check(ref[quiet], ref[quiet], x[quiet], "the oracle against itself")


@pytest.mark.parametrize("setting", [k for k, v in AGC_SETTINGS.items() if v[1]])
def test_the_twin_of_the_default_path_has_the_oracles_bits(O, agc_refs, setting):
    """agc_peak0 + agc_desired1 + GainOp0 restated in numpy f32 against the oracle, all 14 signals, 40 000 samples: the shortcuts' premises
    (0.1 <= gain <= max, a zero or NaN level drops out, one division for two) hold on this bank and the documented tie does not occur."""
    x, ref = agc_refs[setting]
    out, gains = agc_default_twin(x, RATE, **AGC_SETTINGS[setting][0])
    for i, k in enumerate(AGC_SIGNALS):
        assert np.array_equal(out[i].view(np.uint32), ref[i].view(np.uint32)), (setting, k, int(np.argmax(out[i].view(np.uint32) != ref[i].view(np.uint32))))
    assert float(gains.min()) == float(np.float32(0.1)) and float(gains.max()) <= 7.0
    sil = AGC_SIGNALS.index("silence")
    if setting == "attack5ms":
        assert 6.9999 < float(gains[sil, -1]) < 7.0 and gains[sil, -1] == gains[sil, -2]  # the stall, in the gain itself
    if setting == "attack0":
        assert np.all(gains[sil] == 7.0)
        for k in ("dc03_tail", "noise_tail", "step_tail"):  # positive residue, negative residue (NaN rms), exact zero: the ceiling
            assert np.all(gains[AGC_SIGNALS.index(k), 2 * WINDOW:] == 7.0), k


@pytest.mark.parametrize("setting", [k for k, v in AGC_SETTINGS.items() if v[1]])
def test_what_sees_a_wrong_residue_branch(setting):
    """The residue rows are exactly silent behind their fall, so the OUTPUT of a run cannot show what the residue branches decide: a twin
    whose NaN rms (or tiny positive rms) asks for gain 0 instead of the ceiling has every output bit of the bank.  What shows it is the gain
    the run leaves behind -- which is why the GPU test holds the carried gain word to the twin's -- and, unless the attack is 0 (the gain is
    then its own sample's desired: nothing of the past is left in it), a probe of 0.01 played behind the run."""
    kw = AGC_SETTINGS[setting][0]
    n, probe = 20000, 8
    x = np.concatenate([agc_rows(n), np.full((len(AGC_SIGNALS), probe), 0.01, np.float32)], axis=1)
    out, gains = agc_default_twin(x, RATE, **kw)
    for wrong, rows in (("nan", {"noise_tail"}), ("tiny", {"dc03_tail", "tone_tail"})):
        bad, bad_gains = agc_default_twin(x, RATE, wrong=wrong, **kw)
        assert np.array_equal(bad[:, :n].view(np.uint32), out[:, :n].view(np.uint32)), wrong  # invisible in the run's output
        differ = {AGC_SIGNALS[i] for i in np.flatnonzero(np.abs(bad_gains[:, n - 1].astype(np.float64) - gains[:, n - 1]) > AGC_ULPS * gains[:, n - 1])}
        assert differ == rows, (wrong, differ)  # the gain word sees it, at every setting
        seen = {AGC_SIGNALS[i] for i in np.flatnonzero(np.any(np.abs(bad[:, n:].astype(np.float64) - out[:, n:]) > AGC_ULPS * np.abs(out[:, n:]), axis=1))}
        # (with attack 0 the probe shows only a branch it takes itself: the window sum behind noise_tail is still negative under it)
        assert seen == (rows if setting != "attack0" or wrong == "nan" else set()), (wrong, setting, seen)
