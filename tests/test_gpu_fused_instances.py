"""Every shipped instance of the fused kernels against the oracle: the 134 rows of the six tables (fused_instances.py), both kernels of each
row.  The cost model, the geometry overrides of rh_rlm_config and the tuner can each put any row into production; the other suites pin
geometries at 44.1 -> 48 kHz only, which selects the smallest stage of every tile size.  Here a case is one (row, kernel): the rate pair that
makes find_variant select the row (fused_instances.case_of), frames_per_lane / ring_stages pinned, S = 5 sources (more than any ring has
stages) of max(6, look-back + 2) whole tiles and a partial one.

  fast, fast1   equal lengths, set_mix_first(False): every source through the instance's own source loop
  wave, wave1   a ragged batch (three longest sources, one that ends in the middle of a tile near the end, one of half the length); the
                filtered kernel with force_general=1, the plain one by itself
  rag, rag1     the ragged batch, filtered: k_rlm_fast<RAG> with the pairs of the ending sources inside it ("rag"), and -- stereo, with
                RH_RAG_TWO_KERNELS=1 -- without them and k_rlm_resid behind it ("resid": the same operations in the same order, the same bits)

Every case first asserts from geometry() that the row it names is the one that runs (a refused rh_rlm_create raises: the case fails), then
compares: without a filter the oracle's converter + ordered sum bit for bit; with low_pass(200) the checks and tolerances of
test_fused_filtered_pipeline (test_gpu_parity.py)."""
import numpy as np
import pytest
from conftest import knobs
from fused_instances import TABLES, case_of, equal_frames, out_frames, ragged_frames, whole_tiles
from test_gpu_parity import _check_filtered, _oracle_pipeline, _same_bits, _truth_pipeline, rnd

pytestmark = pytest.mark.gpu
FILT, FREQ = "low_pass", 200  # at the output rate: a tile of 64 * 3 frames looks back at ~8 tiles, one of 64 * 20 at 2
RAN = {t: set() for t in TABLES}  # (row, kernel) of the cases that ran on the instance they name
_REFS = {}


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _cases(table):
    rows, _, _, kernels = TABLES[table]
    cases = [(case_of(table, row), k) for row in rows for k in kernels]
    assert len(cases) == len(rows) * len(kernels) and len(set((c.row, k) for c, k in cases)) == len(cases)
    return cases


def _matrix(table):
    cases = _cases(table)
    return pytest.mark.parametrize("case,kernel", cases, ids=[f"{c!r}-{k}" for c, k in cases])


def _inputs(c, ns):
    """rnd(seed, ., 1 / S) per source: the same samples for every case of one channel count, cut to the case's lengths."""
    return [rnd(7100 + 10 * c.ch + s, c.ch * n, 1.0 / c.S) for s, n in enumerate(ns)]


def _refs(O, c, ns, filt):
    """The oracle's mix and, with a filter, the f64 evaluation: computed once per (channels, rates, lengths, filter), shared by the cases with
    that batch (a row's kernels, the same tile size in the wave and rag tables), read-only."""
    key = (c.ch, c.frm, c.to, tuple(ns), filt)
    if key not in _REFS:
        xs = _inputs(c, ns)
        ref = _oracle_pipeline(O, xs, c.frm, c.to, None, filt, FREQ if filt else 0, c.ch)
        truth = _truth_pipeline(O, xs, c.frm, c.to, None, filt, FREQ, c.ch) if filt else None
        for a in (ref, truth):
            if a is not None:
                a.setflags(write=False)
        _REFS[key] = (ref, truth)
    return _REFS[key]


def _run(G, c, filt, general):
    """One handle pinned to the case's (R, NS) at its rates -> (output, lengths, geometry with the batch set).  The handle first (sized for the
    longest look-back there is): the shape follows the look-back it reports."""
    import torch

    p = G.ResampleLowpassMix(c.frm, c.to, c.ch, None, filt, FREQ, 0.5, max_sources=c.S, max_in_frames=equal_frames(c, 32),
                             frames_per_lane=c.R, ring_stages=c.NS, force_general=general)
    try:
        J = p.geometry()["lookback_tiles"]
        assert (1 <= J <= 32) if filt else J == 0, J
        ns = [equal_frames(c, J)] * c.S if c.family == "fast" else ragged_frames(c, J)
        if c.family == "fast":
            p.set_mix_first(False)
        p.set_sources([torch.from_numpy(x).cuda() for x in _inputs(c, ns)])
        geo = p.geometry()
        # ---- the instance, before anything is compared
        assert (geo["frames_per_lane"], geo["stage_kib"], geo["ring_stages"]) == c.row, (c, geo)
        assert geo["general_kernel"] == (0 if c.family == "fast" else 1) and geo["ragged_pair"] == (1 if c.family == "rag" else 0), (c, geo)
        assert geo["mix_first"] == 0 and geo["lookback_tiles"] == J, (c, geo)
        L, M = 64 * c.R, out_frames(max(ns), c.frm, c.to)
        assert p.out_frames == M and geo["n_tiles"] == M // L + 1 >= whole_tiles(J) + 1 and M % 4 != 0, (c, M, geo)
        out = p.run().cpu().numpy().copy()
        p.check_status()
    finally:
        p.close()
    assert len(out) == c.ch * M, (len(out), M)
    return out, ns, geo


def _filtered_checks(O, c, tag, out, ns):
    ref, truth = _refs(O, c, ns, FILT)
    err, peak = _check_filtered(tag, out, ref, truth)
    assert err <= 2e-5 * peak + 1e-7, (tag, err, peak)  # and not merely because the inputs were scaled down


def _case(G, O, c, kernel):
    assert kernel in c.kernels
    tag = f"{c!r} {kernel}"
    if kernel == "plain":  # no filter: the converter + the ordered sum, bit for bit
        out, ns, _ = _run(G, c, None, 0)
        RAN[c.table].add((c.row, kernel))
        ref, _ = _refs(O, c, ns, None)
        assert _same_bits(out, ref), (tag, int(np.argmax(out.view(np.uint32) != ref.view(np.uint32))) if out.shape == ref.shape else (out.shape, ref.shape))
    elif kernel in ("filt", "rag"):  # k_rlm_wave runs a filtered ragged batch only where the ragged pair is switched off
        out, ns, geo = _run(G, c, FILT, 1 if c.family == "wave" else 0)
        RAN[c.table].add((c.row, kernel))
        _filtered_checks(O, c, f"{tag} J{geo['lookback_tiles']}", out, ns)
    else:  # "resid"
        with knobs(RH_RAG_TWO_KERNELS="1"):
            out, ns, geo = _run(G, c, FILT, 0)
        RAN[c.table].add((c.row, kernel))
        _filtered_checks(O, c, f"{tag} J{geo['lookback_tiles']}", out, ns)
        merged, ns2, _ = _run(G, c, FILT, 0)
        assert ns2 == ns and np.array_equal(out, merged), (tag, float(np.max(np.abs(out - merged))))


@_matrix("fast")
def test_fast_stereo(G, O, case, kernel):
    _case(G, O, case, kernel)


@_matrix("fast1")
def test_fast_mono(G, O, case, kernel):
    _case(G, O, case, kernel)


@_matrix("wave")
def test_wave_stereo(G, O, case, kernel):
    _case(G, O, case, kernel)


@_matrix("wave1")
def test_wave_mono(G, O, case, kernel):
    _case(G, O, case, kernel)


@_matrix("rag")
def test_rag_stereo(G, O, case, kernel):
    _case(G, O, case, kernel)


@_matrix("rag1")
def test_rag_mono(G, O, case, kernel):
    _case(G, O, case, kernel)


@pytest.mark.parametrize("table", list(TABLES))
def test_every_row_of_the_table_ran(request, table):
    """Behind the matrix: every case of the table that this session selected ran on the instance it names -- in a whole run of the module
    that is every row of the table times the kernels of a row."""
    rows, _, _, kernels = TABLES[table]
    here = [i for i in request.session.items if i.module is request.module and hasattr(i, "callspec") and "case" in i.callspec.params]
    selected = {(i.callspec.params["case"].row, i.callspec.params["kernel"]) for i in here if i.callspec.params["case"].table == table}
    assert RAN[table] == selected, ("selected, but not run on its instance", sorted(selected - RAN[table]))
    if len(here) == sum(len(v[0]) * len(v[3]) for v in TABLES.values()):  # nothing deselected
        assert len(RAN[table]) == len(rows) * len(kernels) and {r for r, _ in RAN[table]} == set(rows)
