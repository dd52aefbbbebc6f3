"""What test_gpu_filter_signals.py rests on (filter_signals.py), pinned on the CPU with the oracle alone, so that the bank cannot quietly
stop testing anything: every row of FILTERS takes the branch of scan_basis and the side of the gate the table states, the library's gate
agrees with the restated one, the tails behind a fall to silence run through subnormals, the oracle stays finite on the whole bank, and the
pairs that criterion C leaves out are the ones the rule gives -- never a noise pair, at most a quarter, the DC pairs at low cutoffs among them."""
import os

import numpy as np
import pytest
from filter_signals import (BQ_VARIANTS, FILTERS, RATE, SIGNALS, bank, bq_tile, bq_variant, bq_variants_in_source, contract_applies, filter_id, l1_gain,
                            measure, scan_branch, scan_nu, scan_ok, stream_name, streams, truth)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FRAMES = 20012


def _oracle(O, x, ch, kind, freq, q):
    src = O.TestSource(x, ch, RATE)
    return (src.low_pass(freq, q) if kind == "low_pass" else src.high_pass(freq, q)).collect()


@pytest.fixture(scope="module")
def runs(O):
    """(row, coefficients, gain, input [9, frames], oracle [9, frames], truth [9, frames]) per row of FILTERS, mono, computed once, read-only."""
    out = []
    for row in FILTERS:
        kind, freq, q = row[:3]
        co = O.blt_coeffs(kind, freq, q, RATE)
        x = streams(FRAMES, 1, freq)
        ref = np.stack([_oracle(O, x[s], 1, kind, freq, q) for s in range(len(SIGNALS))])
        tru = np.stack([truth(co, x[s], 1) for s in range(len(SIGNALS))])
        for a in (x, ref, tru):
            a.setflags(write=False)
        out.append((row, co, l1_gain(co), x, ref, tru))
    return out


def test_the_bank_is_what_it_says():
    b = bank(FRAMES, 1000)
    assert tuple(b) == SIGNALS and all(v.dtype == np.float32 and v.shape == (FRAMES,) for v in b.values())
    assert np.all(b["dc"] == 1.0) and np.all(b["dc_flip"][:8192] == -1.0) and np.all(b["dc_flip"][8192:] == 1.0)
    assert np.all(b["step_tail"][:8192] == 1.0) and not b["step_tail"][8192:].any()
    assert np.flatnonzero(b["impulses"]).tolist() == [0, 12287]
    assert 0.8 <= b["dc_noise"].min() < 0.81 and 0.99 < b["dc_noise"].max() <= 1.0
    assert not b["tone_tail"][6000:].any() and np.array_equal(b["tone_tail"][:6000], b["tone"][:6000]) and b["tone"][12] == np.float32(1.0)  # 48 samples a period
    assert np.array_equal(b["nyquist"][:4], np.float32([1, -1, 1, -1])) and abs(float(b["noise"].mean())) < 0.02 and float(np.abs(b["noise"]).max()) > 0.999
    x = streams(100, 6, 1000)
    assert x.shape == (9, 600)
    for s in range(9):
        for c in range(6):
            assert np.array_equal(x[s].reshape(100, 6)[:, c], bank(100, 1000)[SIGNALS[(s + c) % 9]])
    assert stream_name(8, 2) == "nyquist+noise"


def test_every_row_takes_the_branch_and_the_side_of_the_gate_the_table_states(O, rh):
    wrong = []
    for row in FILTERS:
        kind, freq, q, geo, branch = row
        co = O.blt_coeffs(kind, freq, q, RATE)
        if scan_branch(co) != branch:
            wrong.append((filter_id(row), "branch", scan_branch(co), scan_nu(co)))
        if not scan_ok(kind, co):
            wrong.append((filter_id(row), "no longer passes the gate"))
        if bool(rh.filter_scan_ok(kind, freq, q, RATE)) != scan_ok(kind, co):  # (host arithmetic only: needs no device, like test_host_logic.py)
            wrong.append((filter_id(row), "rh_filter_scan_ok disagrees with the restated gate"))
        disc = float(co[3]) ** 2 - 4.0 * float(co[4])
        if geo == "distinct" and not disc > 1e-3 or geo == "double" and not abs(disc) < 1e-6 or geo == "complex" and not disc < -1e-2:
            wrong.append((filter_id(row), "pole geometry", disc))
    assert not wrong, wrong
    assert {r[3] for r in FILTERS} == {"distinct", "double", "complex", "edge"} and {r[4] for r in FILTERS} == {"real", "complex"}
    # the pair either side of scan_basis's 1e-3
    lo, hi = (O.blt_coeffs("low_pass", 1000, q, RATE) for q in (0.50001, 0.50003))
    assert 5e-4 < scan_nu(lo) < 1e-3 < scan_nu(hi) < 1.5e-3, (scan_nu(lo), scan_nu(hi))
    # the restated gate at the contract's documented edges
    for kind, inside, outside in (("low_pass", 100, 50), ("high_pass", 600, 500)):
        assert scan_ok(kind, O.blt_coeffs(kind, inside, 0.5, RATE)) and not scan_ok(kind, O.blt_coeffs(kind, outside, 0.5, RATE))
        assert rh.filter_scan_ok(kind, inside, 0.5, RATE) and not rh.filter_scan_ok(kind, outside, 0.5, RATE)


def test_the_predicates_restate_the_sources():
    src = lambda name: open(os.path.join(ROOT, "rodio_amd", "csrc", name)).read()  # noqa: E731
    for name in ("rh_pipeline_internal.h", "rh_biquad_scan.hip"):
        assert "disc < 0.0 && std::sqrt(-disc) * 0.5 > 1e-3" in src(name), name
    assert "(1.0 - r) >= (kind == 0 ? 0.0125 : 0.075)" in src("rh_recurrence.hip")
    assert bq_variants_in_source(src("rh_biquad_scan.hip")) == BQ_VARIANTS
    assert "tile_of(c) <= 2 * frames" in src("rh_scan_launch.h")
    # the variants the GPU test names
    assert [bq_variant(c, 20012) for c in (1, 2, 6)] == [(16, 8), (16, 8), (4, 8)] and [bq_tile(c, 20012) for c in (1, 2, 6)] == [8192, 8192, 2048]
    assert [bq_variant(c, 1500) for c in (1, 2, 6)] == [(16, 1), (8, 4), (4, 8)] and [bq_tile(c, 1500) for c in (1, 2, 6)] == [1024, 2048, 2048]
    assert [bq_variant(c, 1000) for c in (1, 2, 6)] == [(16, 1), (8, 1), (4, 1)] and [bq_tile(c, 1000) for c in (1, 2, 6)] == [1024, 512, 256]
    assert [bq_variant(c, 500) for c in (1, 2, 6)] == [(16, 1), (8, 1), (4, 1)]
    assert [bq_variant(2, n) for n in (8192, 5000, 3628)] == [(16, 8), (16, 8), (8, 8)]


def test_the_oracle_stays_finite_and_the_tails_run_through_subnormals(runs):
    few = []
    for row, co, gain, x, ref, tru in runs:
        assert np.isfinite(ref).all() and np.isfinite(tru).all(), filter_id(row)
        assert 0.999 <= gain < 10.0, (filter_id(row), gain)  # (a low-pass of unit DC gain in f32 coefficients: 1 - 4e-5 at the least)
        if row[0] != "low_pass":
            continue
        for name in ("step_tail", "tone_tail", "impulses"):
            y = ref[SIGNALS.index(name)]
            sub = int(np.count_nonzero((np.abs(y) < np.float32(2.0 ** -126)) & (y != 0)))
            if sub < 1000:
                few.append((filter_id(row), name, sub))
    assert not few, few


def test_the_pairs_criterion_c_leaves_out(runs):
    excluded, passing = [], 0
    for row, co, gain, x, ref, tru in runs:
        gate = scan_ok(row[0], co)
        for s, name in enumerate(SIGNALS):
            m = measure(ref[s], ref[s], tru[s], float(np.abs(x[s]).max()), gain)
            passing += gate
            if gate and not contract_applies(m["e_ref"], m["peak"], gate):
                excluded.append((filter_id(row), name))
                print(f"[C left out] {filter_id(row)} {name}: |oracle-f64|={m['e_ref']:.3e} peak={m['peak']:.3e}")
    assert passing == len(FILTERS) * len(SIGNALS)  # every row passes the gate today
    assert not [e for e in excluded if e[1] == "noise"], excluded
    assert 4 * len(excluded) <= passing, (len(excluded), passing)
    assert ("low_pass200-q0.5", "dc") in excluded and ("low_pass300-q0.35", "dc") in excluded, excluded
    # what was observed: the dc family, and the tone at the lowest cutoff
    assert {e[1] for e in excluded} <= {"dc", "dc_flip", "dc_noise", "step_tail", "tone", "tone_tail"}, excluded


def test_criterion_b_notices_one_unit_in_the_last_place_of_a_coefficient(runs):
    """What the criteria are worth: a kernel whose a1 is one f32 unit in the last place off (a wrong table entry; evaluated exactly otherwise)
    fails B on some signal of the bank for most rows -- and on DC where noise lets it through."""
    caught = {}
    for row, co, gain, x, ref, tru in runs:
        bad = co.copy()
        bad[3] = np.nextafter(bad[3], np.float32(0))
        used = {}
        for s, name in enumerate(SIGNALS):
            m = measure(truth(bad, x[s], 1).astype(np.float32), ref[s], tru[s], float(np.abs(x[s]).max()), gain)
            used[name] = (m["e_gpu"] - 2.0 * m["e_ref"]) / m["F"]
            ok = measure(tru[s].astype(np.float32), ref[s], tru[s], float(np.abs(x[s]).max()), gain)  # the exact response, rounded once: inside F alone
            assert ok["e_gpu"] <= ok["F"], (filter_id(row), name, ok)
        caught[filter_id(row)] = used
    noticed = [f for f, used in caught.items() if max(used.values()) > 1.0]
    assert len(noticed) >= 10, noticed
    u = caught["low_pass1000-q0.7071"]
    assert u["noise"] < 1.0 < 4.0 < u["dc"], u
    u = caught["low_pass800-q2.0"]
    assert u["tone"] > 2.0 * max(u["noise"], 1.0), u
