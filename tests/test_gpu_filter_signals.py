"""The time-parallel low_pass / high_pass on the signals and filters of filter_signals.py: DC, steps, impulses, tones at the cutoff, a Nyquist
alternation and tails that decay into subnormals, through distinct real poles, the double pole of q = 0.5, complex pairs and the two rows
either side of scan_basis's branch edge.  Every case prints `|gpu-oracle| |gpu-f64| |oracle-f64| peak F` and is held to the two criteria
of filter_signals.criteria (B: no further from the f64 response than rodio's recurrence, + F; C: within 1e-5 * peak of rodio where rodio
itself is within 5e-6 * peak of the f64 response); profiles/filter_signals.txt holds the lines of one whole run.

  rh_biquad       the nine signals as nine streams of one call, 1 / 2 / 6 channels (channel c of stream s: signal (s + c) mod 9).  Mode 0 is the
                  oracle bit for bit (subnormals and signed zeros included); mode 1 under RH_BIQUAD_NO_FALLBACK=1 (k_biquad_scan or an error)
                  meets B and C per stream, in one call and with the state carried across blocks; the state words left behind are mode 0's
                  within the same criteria.  The variant is rh::scan::pick_variant's (restated in filter_signals.bq_variant, held against the
                  sources by test_filter_signals_cpu.py), (R, NW) -> tile of 64 R NW frames:
                    20 012 frames  mono (16, 8) 8192, stereo (16, 8) 8192, 5.1 (4, 8) 2048: three to ten tiles; blocks of 8192 (whole tiles)
                                   and of 5000 frames (stereo and mono: one partial 8192-tile; 5.1: 2048-tiles)
                     1 500 frames  mono (16, 1) 1024, two tiles; stereo (8, 4) and 5.1 (4, 8): 2048, one partial tile.  Blocks of 500 frames take
                                   the single-wave variants of every layout: (16, 1) 1024, (8, 1) 512, (4, 1) 256
                     1 000 frames  the single-wave variants in one call: mono (16, 1) one tile, stereo (8, 1) two, 5.1 (4, 1) four -- low_pass(200)
                                   looks back over several of them, so a DC state has to survive a look-back longer than one tile
  fused one-pass  ResampleLowpassMix on five sources (dc_noise, tone, step_tail, impulses, noise; events in the middle of the batch) at four
                  geometries (k_rlm_fast with 3, 8, 16 frames per lane, k_rlm_wave with 8; mono has no instance with 3 frames per lane or with
                  16 and three stages: 4 and (16, 2) stand in), stereo and mono, 44.1 -> 48 kHz and 48 -> 48 kHz, mix first on and off;
                  geometry() names the kernel before anything is compared
  streamed        the same batch in blocks of 3000 input frames through rh_rlm_stream_block_v: k_rlm_sblk, and RH_NO_SBLK=1
  per source      rh_rlm_set_filters: one filter of each pole geometry in one handle, the bank as its sources"""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
from conftest import knobs
from filter_signals import (FILTERS, RATE, SIGNALS, bq_variant, criteria, filter_id, l1_gain, line, scan_branch, scan_ok, stream_name, streams, truth)
from fused_instances import equal_frames, out_frames, select, whole_tiles
from test_gpu_parity import _oracle_pipeline, _truth_pipeline

pytestmark = pytest.mark.gpu
_IDS = [filter_id(r) for r in FILTERS]


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


# ================================================================================================ stand-alone rh_biquad ====
LENGTHS = {20012: ((8192, 5000), {1: (16, 8), 2: (16, 8), 6: (4, 8)}),
           1500: ((500,), {1: (16, 1), 2: (8, 4), 6: (4, 8)}),
           1000: ((), {1: (16, 1), 2: (8, 1), 6: (4, 1)})}
BLOCK_VARIANTS = {(8192, 1): (16, 8), (8192, 2): (16, 8), (8192, 6): (4, 8), (5000, 1): (16, 8), (5000, 2): (16, 8), (5000, 6): (4, 8),
                  (500, 1): (16, 1), (500, 2): (8, 1), (500, 6): (4, 1)}


def _biquad(x, frames, ch, co, mode, state=None):
    import torch
    from rodio_amd import _lib

    S = x.shape[0]
    assert x.is_contiguous() and x.shape[1] == frames * ch and (frames * ch) % 4 == 0 and x.data_ptr() % 16 == 0
    out = torch.empty_like(x)
    _lib.check(_lib.lib.rh_biquad(C.c_void_p(out.data_ptr()), C.c_void_p(x.data_ptr()), frames, ch, S, co.ctypes.data_as(_lib.f32p),
                                  C.c_void_p(state.data_ptr()) if state is not None else None, mode, C.c_void_p(torch.cuda.current_stream().cuda_stream)), "rh_biquad")
    return out


def _in_blocks(x, frames, ch, co, mode, step):
    """The call in blocks of `step` frames with the state carried -> (output, state words [S, 4 ch])."""
    import torch

    st = torch.zeros((x.shape[0], 4 * ch), device="cuda")
    parts = []
    for a in range(0, frames, step):
        b = min(frames, a + step)
        parts.append(_biquad(x[:, a * ch: b * ch].contiguous(), b - a, ch, co, mode, st))
    return torch.cat(parts, dim=1).cpu().numpy(), st.cpu().numpy()


def _same_words(a, b):
    return a.shape == b.shape and np.array_equal(np.ascontiguousarray(a).view(np.uint32), np.ascontiguousarray(b).view(np.uint32))


@pytest.mark.parametrize("frames", list(LENGTHS))
@pytest.mark.parametrize("ch", [1, 2, 6])
@pytest.mark.parametrize("row", FILTERS, ids=_IDS)
def test_filter_signals_biquad(G, O, row, ch, frames):
    import torch

    kind, freq, q, _, branch = row
    steps, variants = LENGTHS[frames]
    assert not os.environ.get("RH_BIQUAD_R") and not os.environ.get("RH_BIQUAD_NW")  # (a request would override the pick)
    assert bq_variant(ch, frames) == variants[ch] and all(bq_variant(ch, s) == BLOCK_VARIANTS[(s, ch)] for s in steps)
    co = G.biquad_coeffs(kind, freq, q, RATE)
    assert _same_words(co, O.blt_coeffs(kind, freq, q, RATE)) and scan_branch(co) == branch
    gate, gain = scan_ok(kind, co), l1_gain(co)
    x = streams(frames, ch, freq)
    xd = torch.from_numpy(x).cuda()
    ref = np.stack([(O.TestSource(x[s], ch, RATE).low_pass(freq, q) if kind == "low_pass" else O.TestSource(x[s], ch, RATE).high_pass(freq, q)).collect()
                    for s in range(len(SIGNALS))])
    tru = np.stack([truth(co, x[s], ch) for s in range(len(SIGNALS))])
    tag = f"biquad {filter_id(row)} ch{ch} n{frames} R{variants[ch][0]}xNW{variants[ch][1]}"
    with knobs(RH_BIQUAD_NO_FALLBACK="1"):  # the scan kernel or an error
        seq = _biquad(xd, frames, ch, co, 0).cpu().numpy()
        par = _biquad(xd, frames, ch, co, 1).cpu().numpy()
        blocks = {step: (_in_blocks(xd, frames, ch, co, 0, step), _in_blocks(xd, frames, ch, co, 1, step)) for step in steps}
        G.async_status()
    # mode 0: rodio's bits, in one call and in blocks
    for s in range(len(SIGNALS)):
        assert _same_words(seq[s], ref[s]), ("mode 0", tag, stream_name(s, ch), int(np.argmax(seq[s].view(np.uint32) != ref[s].view(np.uint32))))
    for step, ((seq_b, st0), _) in blocks.items():
        assert _same_words(seq_b, ref), ("mode 0 in blocks", tag, step)
    # mode 1: the criteria per stream
    left_out, worst = [], {}
    for s in range(len(SIGNALS)):
        xp = float(np.abs(x[s]).max())
        m = criteria(par[s], ref[s], tru[s], xp, gain, f"{tag} {stream_name(s, ch)}", gate)
        if not m["C"]:
            left_out.append(stream_name(s, ch))
        for step, ((_, st0), (par_b, st1)) in blocks.items():
            btag = f"{tag} blocks of {step} {stream_name(s, ch)}"
            mb = criteria(par_b[s], ref[s], tru[s], xp, gain, btag, gate, show=False)
            if step not in worst or mb["B_used"] > worst[step][1]["B_used"]:
                worst[step] = (btag, mb)
            # the state: {x1, x2, y1, y2} per channel.  The inputs are the block's own; the outputs are the last two output frames
            w0, w1 = st0[s].reshape(ch, 4), st1[s].reshape(ch, 4)
            assert _same_words(w1[:, :2], w0[:, :2]), ("state inputs", tag, step, s)
            last = tru[s].reshape(frames, ch)[[frames - 1, frames - 2]].T  # [ch, 2]: y1, y2
            assert _same_words(w0[:, 2:], ref[s].reshape(frames, ch)[[frames - 1, frames - 2]].T)
            assert float(np.max(np.abs(w1[:, 2:] - last))) <= 2.0 * mb["e_ref"] + mb["F"], ("state B", tag, step, s)
            if mb["C"]:
                assert float(np.max(np.abs(w1[:, 2:].astype(np.float64) - w0[:, 2:]))) <= 1e-5 * mb["peak"], ("state C", tag, step, s)
    for btag, mb in worst.values():  # of a run in blocks: the stream that uses most of F
        print(line(btag, mb))
    print(f"[{tag}] C left out by the rule: {', '.join(left_out) or 'none'}")


# ============================================================================================= fused one-pass / streamed ====
FIVE = ("dc_noise", "tone", "step_tail", "impulses", "noise")
# (frames per lane, ring stages, general kernel) stereo -> mono: FAST1 has no row with 3 frames per lane and none with (16, ., 3)
GEOS = [(3, 2, 0), (8, 2, 0), (16, 3, 0), (8, 2, 1)]
GEOS_MONO = {(3, 2, 0): (4, 2, 0), (16, 3, 0): (16, 2, 0)}
LAYOUTS = [(2, 44100), (1, 44100), (2, 48000), (1, 48000)]
FUSED_FILTERS = [r for r in FILTERS if r[2] in (0.3, 0.5, 0.7071, 2.0) or r[3] == "edge"]
STREAM_FILTERS = [r for r in FILTERS if r[2] in (0.5, 0.7071, 2.0)]
_REFS = {}


def _sources(n, ch, freq, frm):
    """Five sources of n input frames: channel c of source k carries FIVE[(k + c) % 5]; the steps stand in the middle of the batch."""
    return list(streams(n, ch, freq, frm, seed=5, event=n // 2, names=FIVE))


def _fused_refs(O, n, ch, frm, row):
    key = (n, ch, frm, row[:3])
    if key not in _REFS:
        kind, freq, q = row[:3]
        xs = _sources(n, ch, freq, frm)
        ref = _oracle_pipeline(O, xs, frm, RATE, None, kind, freq, ch, q)
        tru = _truth_pipeline(O, xs, frm, RATE, None, kind, freq, ch, q)
        x_peak = float(np.max(np.sum(np.abs(np.stack(xs)), axis=0)))  # what the sum of the sources can reach
        for a in (ref, tru):
            a.setflags(write=False)
        _REFS[key] = (ref, tru, x_peak)
        while len(_REFS) > 8:
            _REFS.pop(next(iter(_REFS)))
    return _REFS[key]


def _geo_for(geo, ch):
    return GEOS_MONO.get(geo, geo) if ch == 1 else geo


@pytest.mark.parametrize("mix_first", [True, False], ids=["mixfirst", "persource"])
@pytest.mark.parametrize("geo", GEOS, ids=lambda g: f"R{g[0]}-NS{g[1]}-{'wave' if g[2] else 'fast'}")
@pytest.mark.parametrize("row", FUSED_FILTERS, ids=[filter_id(r) for r in FUSED_FILTERS])
def test_filter_signals_fused(G, O, row, geo, mix_first):
    """One (filter, geometry, mix first) per case; the layout (channels, input rate) rotates with both, so every filter meets the four layouts
    over its four geometries and every geometry meets them over the filters."""
    import torch

    kind, freq, q, _, branch = row
    ch, frm = LAYOUTS[(FUSED_FILTERS.index(row) + GEOS.index(geo)) % 4]
    R, NS, general = _geo_for(geo, ch)
    table = {(2, 0): "fast", (1, 0): "fast1", (2, 1): "wave", (1, 1): "wave1"}[(ch, general)]
    want_row = select(table, R, NS, frm, RATE)
    assert want_row is not None, (table, R, NS, frm)
    c = SimpleNamespace(R=R, frm=frm, to=RATE)
    co = G.biquad_coeffs(kind, freq, q, RATE)
    assert scan_branch(co) == branch
    p = G.ResampleLowpassMix(frm, RATE, ch, None, kind, freq, q, max_sources=len(FIVE), max_in_frames=equal_frames(c, 32), frames_per_lane=R, ring_stages=NS,
                             force_general=general)
    try:
        J = p.geometry()["lookback_tiles"]
        assert 1 <= J <= 32, J
        n = equal_frames(c, J)
        p.set_mix_first(mix_first)
        xs = _sources(n, ch, freq, frm)
        p.set_sources([torch.from_numpy(x).cuda() for x in xs])
        g = p.geometry()
        # ---- the kernel, before anything is compared
        assert (g["frames_per_lane"], g["stage_kib"], g["ring_stages"]) == want_row and g["general_kernel"] == general and g["ragged_pair"] == 0, (want_row, g)
        assert g["mix_first"] == (1 if mix_first and not general else 0) and g["lookback_tiles"] == J, g
        M = out_frames(n, frm, RATE)
        assert p.out_frames == M and g["n_tiles"] == M // (64 * R) + 1 >= whole_tiles(J) + 1, (M, g)
        out = p.run().cpu().numpy().copy()
        p.check_status()
    finally:
        p.close()
    ref, tru, x_peak = _fused_refs(O, n, ch, frm, row)
    tag = f"fused {filter_id(row)} {table} R{R} NS{NS} {'mixfirst' if g['mix_first'] else 'persource'} ch{ch} {frm} J{J} n{n}"
    criteria(out, ref, tru, x_peak, l1_gain(co), tag, scan_ok(kind, co))


@pytest.mark.parametrize("ch,frm", LAYOUTS)
@pytest.mark.parametrize("row", STREAM_FILTERS, ids=[filter_id(r) for r in STREAM_FILTERS])
def test_filter_signals_streamed(G, O, row, ch, frm):
    """The five sources in blocks of 3000 input frames through rh_rlm_stream_block_v: every block one launch of k_rlm_sblk; with RH_NO_SBLK=1
    none.  Both against the one-pass references."""
    import torch
    from rodio_amd import _lib

    lib = _lib.lib
    kind, freq, q, _, branch = row
    N, B, S = 20012, 3000, len(FIVE)
    co = G.biquad_coeffs(kind, freq, q, RATE)
    assert scan_branch(co) == branch
    xs = _sources(N, ch, freq, frm)
    data = torch.from_numpy(np.stack(xs)).cuda()
    M = out_frames(N, frm, RATE)

    def run():
        p = G.ResampleLowpassMix(frm, RATE, ch, None, kind, freq, q, max_sources=S, max_in_frames=B + 4096)
        try:
            p.stream_begin(keep_history=True)
            out = torch.zeros(ch * M + 4096, device="cuda", dtype=torch.float32)
            g0 = m = k = 0
            while True:
                hi = min(N, (k + 1) * B)
                ptrs = (C.c_void_p * S)(*[data[s_].data_ptr() + g0 * 4 * ch for s_ in range(S)])
                avail = (C.c_uint64 * S)(*([hi - g0] * S))
                ended = (C.c_uint8 * S)(*([1 if hi == N else 0] * S))
                o, c_ = C.c_uint64(0), C.c_uint64(0)
                _lib.check(lib.rh_rlm_stream_block_v(p._h, ptrs, avail, ended, S, C.c_void_p(out.data_ptr() + m * 4 * ch), M + 512 - m, C.byref(o), C.byref(c_), None), "rh_rlm_stream_block_v")
                assert o.value <= M - m and c_.value <= hi - g0
                m += o.value
                g0 += c_.value
                k += 1
                if hi == N:
                    break
            p.check_status()
            one = C.c_uint32(0)
            _lib.check(lib.rh_rlm_stream_one_launch_blocks(p._h, C.byref(one)), "rh_rlm_stream_one_launch_blocks")
            return out[: ch * m].cpu().numpy(), one.value, p.stream_stats(), k
        finally:
            p.close()

    a, one_a, st_a, nb = run()
    with knobs(RH_NO_SBLK="1"):
        b, one_b, st_b, _ = run()
    # ---- the kernels, before anything is compared: every block on the summed state; one launch per block, or none
    assert nb == 7 and one_a == nb and one_b == 0 and st_a[0] == nb and st_a[1] == 0, (nb, one_a, one_b, st_a, st_b)
    ref, tru, x_peak = _fused_refs(O, N, ch, frm, row)
    assert len(a) == len(b) == len(ref) == ch * M
    gain, gate = l1_gain(co), scan_ok(kind, co)
    criteria(a, ref, tru, x_peak, gain, f"streamed {filter_id(row)} sblk ch{ch} {frm}", gate)
    criteria(b, ref, tru, x_peak, gain, f"streamed {filter_id(row)} no-sblk ch{ch} {frm}", gate)


PER_SOURCE = [("low_pass", 1000, 0.3), ("low_pass", 200, 0.5), ("low_pass", 1000, 0.7071), ("low_pass", 800, 2.0), ("high_pass", 600, 0.5),
              ("high_pass", 1000, 0.7071), ("low_pass", 1000, 0.50003), ("low_pass", 300, 0.35), ("high_pass", 5000, 3.0)]


@pytest.mark.parametrize("ch,frm", [(2, 44100), (1, 48000)])
def test_filter_signals_a_filter_per_source(G, O, ch, frm):
    """rh_rlm_set_filters: nine sources (the bank; the tones at 1 kHz), each behind a filter of its own -- distinct real poles, the double pole,
    complex pairs, the complex side of the branch edge -- in one handle, against the oracle's mixer of the per-source chains."""
    import torch
    from scipy.signal import lfilter

    assert {f for f in PER_SOURCE} <= {r[:3] for r in FILTERS} and len(PER_SOURCE) == len(SIGNALS)
    n = 20012
    xs = list(streams(n, ch, 1000, frm))
    m = O.Mixer(ch, RATE)
    tru, terms, gate = None, 0.0, True
    for x, (kind, freq, q) in zip(xs, PER_SOURCE):
        u = O.UniformSourceIterator(O.TestSource(x, ch, frm), ch, RATE)
        m.add(u.low_pass(freq, q) if kind == "low_pass" else u.high_pass(freq, q))
        co = O.blt_coeffs(kind, freq, q, RATE)
        r = O.UniformSourceIterator(O.TestSource(x, ch, frm), ch, RATE).collect().astype(np.float64).reshape(-1, ch)
        y = lfilter(co[:3].astype(np.float64), [1.0, float(co[3]), float(co[4])], r, axis=0).reshape(-1)
        tru = y if tru is None else tru + y
        terms += float(np.abs(x).max()) * l1_gain(co)  # what this source's time-parallel evaluation adds up
        gate = gate and scan_ok(kind, co)
    ref = m.collect()
    p = G.ResampleLowpassMix(frm, RATE, ch, None, "low_pass", 200, 0.5, max_sources=len(xs), max_in_frames=n)
    try:
        p.set_filters(PER_SOURCE)
        p.set_sources([torch.from_numpy(x).cuda() for x in xs])
        got = p.run().cpu().numpy().copy()
        again = p.run().cpu().numpy()
        p.check_status()
        g = p.geometry()
    finally:
        p.close()
    assert np.array_equal(got, again), g
    criteria(got, ref, tru, 1.0, terms, f"per source ch{ch} {frm}", gate)
