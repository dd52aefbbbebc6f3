"""The time-parallel limiter (rh_limit.hip) and the AGC (rh_agc.hip) on the signals and settings of dynamics_signals.py: DC, sign flips, steps
up and down, impulses, a tone, a burst, a Nyquist alternation, DC at the two edges of the knee, stereo pairs whose gain-setting channel
changes -- and for the AGC exact silence, the floor clamp, the ceiling, and window sums that are rounding residues of either sign.
profiles/dynamics_signals.txt holds the lines of one whole run.

The limiter.  Every case prints `|gpu-oracle| |gpu-f64| |oracle-f64| peak F` and the share of F it uses (the stream of the launch that uses
most) and holds every stream to dynamics_signals.limit_criteria: B (no further from the f64 limiter than rodio's recurrence, + F) and, at
every setting but the ill-conditioned one, C (within 1e-5 * peak of rodio; its premise is proved on the CPU for every pair).
  the bank      every setting, the whole bank in one launch (limit_batch; with two channels the pairs among the streams), 1 / 2 / 3 / 6
                channels, 700 / 3000 / 20 000 frames (the variants dynamics_signals.LIMIT_NAMED names: the smallest tile, a mid tile, three
                8192-frame tiles or ten of 2048), 20 ms / 1 s also at 40 000.  Both durations 0: the memoryless form beside B and C
  the forms     stereo, 20 000 frames: RH_LIMIT_SEQ=1, RH_LIMIT_SKEW=1 (the same bits as without), RH_LIMIT_NIO=1; and the bank tiled to 300
                streams of 2048 frames, the shape that takes the one-poll-point variant by itself (more streams than resident workgroups)
  the state     two blocks cut at 8191, 8192, 8193, 12288 with four channels (rows of any length are 16-byte multiples: every block is the scan
                kernel's) and at 8192, 12288, 8191 with two (8191 frames of two channels are no 16-byte multiple: the reference-order kernel);
                blocks and one pass each meet B and C, and the {integrator, peak} left behind is the f64 limiter's

The AGC.  Against the oracle at the suite's 1e-5 * max(1, max|x|), and on every sample within 2^-22 of the oracle's value (dynamics_signals.
AGC_ULPS: derived, and the bound that sees a gain that reaches the ceiling where rodio's stalls 8e-6 under it); between the forms what the
suite claims: fused == RH_AGC_SEGMENTS=1, RH_AGC_FUSED_R4=1 == default, RH_AGC_VEC=1 == RH_AGC_SEQ=1, bit for bit, outputs and states; the
default path within 1e-6 of RH_AGC_SEQ=1 and the general path equal to it.  Rows that end in exact silence (the residue rows, silence itself)
put out 0 * gain whatever the residue branches decide, so every run is made from a fresh state, and what it leaves is looked at twice: a
probe of 8 samples of 0.01 played from it is held to the oracle's continuation like the run itself, and on the default path the gain word
of every form is the numpy-f32 twin's within 2^-22 (with attack 0 the probe's gain is its own desired and only the word remembers)."""
import numpy as np
import pytest
from conftest import knobs
from dynamics_signals import (AGC_SETTINGS, AGC_SIGNALS, AGC_ULPS, LIMIT_NAMED, LIMIT_SETTINGS, LIMIT_SIGNALS, LV_NIO, RATE, agc_bank, agc_check, agc_default_twin, agc_rows, limit_case,
                              limit_criteria, limit_F, limit_line, limit_memoryless, limit_stream_names, limit_state_f32, limit_streams, limit_truth, lv_nio_gate, lv_skew_gate, lv_variant)

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


# ================================================================================================ the limiter ====
_REFS = {}


def _refs(O, setting, ch, frames):
    """(parameters, held to C, input, oracle, truth, truth's final state) of one launch, computed once, read-only."""
    key = (setting, ch, frames)
    if key not in _REFS:
        kw, contract, x = limit_case(setting, ch, frames)
        ref = np.stack([O.TestSource(x[s], ch, RATE).limit(**kw).collect() for s in range(x.shape[0])])
        tru, end = limit_truth(x, ch, RATE, **kw)
        for a in (x, ref, tru, end):
            a.setflags(write=False)
        _REFS[key] = (kw, contract, x, ref, tru, end)
        while len(_REFS) > 6:
            _REFS.pop(next(iter(_REFS)))
    return _REFS[key]


def _hold(out, refs, ch, lengths, tag, variant=None):
    """Every stream of a launch against B and C; prints the stream that uses most of F (and the one furthest from the oracle)."""
    kw, contract, x, ref, tru, _ = refs
    names = limit_stream_names(ch)
    assert out.shape == x.shape
    ms = [(f"{tag} {names[s]}", limit_criteria(out[s], ref[s], tru[s], x[s], limit_F(x[s], kw, ch, lengths, variant), f"{tag} {names[s]}", contract, show=False))
          for s in range(x.shape[0])]
    top = max(ms, key=lambda t: t[1]["B_used"])
    far = max(ms, key=lambda t: t[1]["d"])
    print(limit_line(*top))
    if far is not top:
        print(limit_line(*far))
    return ms


def _limit(G, x, ch, kw, state=None):
    import torch

    xd = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.array(x)).cuda()  # (a copy: the shared references are read-only)
    return G.limit_batch(xd, ch, RATE, state=state, **kw).cpu().numpy()


BANK_CASES = [(s, c, n) for s in LIMIT_SETTINGS for c in (1, 2, 3, 6) for n in (700, 3000, 20000)] + [("20ms-1s", c, 40000) for c in (1, 2, 3, 6)]


@pytest.mark.parametrize("setting,ch,frames", BANK_CASES, ids=[f"{s}-ch{c}-n{n}" for s, c, n in BANK_CASES])
def test_dynamics_limiter_bank(G, O, setting, ch, frames):
    refs = _refs(O, setting, ch, frames)
    kw, contract, x = refs[:3]
    assert (frames * ch) % 4 == 0 and lv_variant(ch, frames) == LIMIT_NAMED[(ch, frames)]  # rows are 16-byte multiples: the scan kernel, this variant
    r, nw = LIMIT_NAMED[(ch, frames)]
    out = _limit(G, x, ch, kw)
    G.async_status()
    _hold(out, refs, ch, [frames], f"limit {setting} ch{ch} n{frames} R{r}xNW{nw}")
    if setting == "both0" and ch == 1:  # no memory: every sample by its own gain computer, in f64
        want = limit_memoryless(x, kw["threshold"], kw["knee_width"])
        den = np.maximum(np.abs(x.astype(np.float64)), 1e-3 * np.abs(x).max(axis=1, keepdims=True))
        for s, name in enumerate(LIMIT_SIGNALS):
            assert float(np.max(np.abs(out[s] - want[s]) / den[s])) <= limit_F(x[s], kw, ch, [frames]), ("memoryless", name)


@pytest.mark.parametrize("setting", list(LIMIT_SETTINGS))
def test_dynamics_limiter_forms(G, O, setting):
    """Stereo, 20 000 frames: the reference-order kernel, the one-poll-point variant forced, the I/O-wave variant -- each held like the
    shipped form; SKEW on and off give the same bits (the same compositions in the same order)."""
    ch, frames = 2, 20000
    refs = _refs(O, setting, ch, frames)
    kw, contract, x = refs[:3]
    assert lv_skew_gate(ch, frames) and lv_nio_gate(ch, frames)
    outs = {}
    for form, env in (("seq", dict(RH_LIMIT_SEQ="1")), ("skew", dict(RH_LIMIT_SKEW="1")), ("noskew", dict(RH_LIMIT_SKEW="0")), ("nio", dict(RH_LIMIT_NIO="1"))):
        with knobs(**env):
            outs[form] = _limit(G, x, ch, kw)
            G.async_status()
    for form, variant in (("seq", None), ("skew", None), ("nio", LV_NIO[1:3])):  # (F is counted for the variant the form runs: NIO's (16, 6))
        _hold(outs[form], refs, ch, [frames], f"limit {setting} {form} ch{ch} n{frames}", variant)
    assert np.array_equal(outs["skew"].view(np.uint32), outs["noskew"].view(np.uint32))


@pytest.mark.parametrize("setting", list(LIMIT_SETTINGS))
def test_dynamics_limiter_more_streams_than_workgroups(G, O, setting):
    """The bank tiled to 300 stereo streams of 2048 frames, the shape of test_limiter_many_streams_one_launch that takes the one-poll-point
    variant by itself: every copy of a stream gets the same bits, and every one meets B and C."""
    ch, frames, S = 2, 2048, 300
    refs = _refs(O, setting, ch, frames)
    kw, contract, x = refs[:3]
    assert lv_variant(ch, frames) == LIMIT_NAMED[(ch, frames)]
    big = np.ascontiguousarray(x[np.arange(S) % x.shape[0]])
    out = _limit(G, big, ch, kw)
    G.async_status()
    for s in range(x.shape[0], S):
        assert np.array_equal(out[s].view(np.uint32), out[s % x.shape[0]].view(np.uint32)), s
    _hold(out[: x.shape[0]], refs, ch, [frames], f"limit {setting} 300 streams ch{ch} n{frames}")


STATE_CUTS = [(4, 8191), (4, 8192), (4, 8193), (4, 12288), (2, 8192), (2, 12288), (2, 8191)]


@pytest.mark.parametrize("setting", list(LIMIT_SETTINGS))
def test_dynamics_limiter_state_across_blocks(G, O, setting):
    import torch

    frames = 20000
    for ch in (4, 2):
        if ch == 4:  # (not among LIMIT_NAMED's layouts: four channels only here, for rows that stay 16-byte multiples at any cut)
            kw, contract, cap = LIMIT_SETTINGS[setting]
            x = limit_streams(frames, ch, kw["threshold"], kw["knee_width"], cap=cap)
            ref = np.stack([O.TestSource(x[s], ch, RATE).limit(**kw).collect() for s in range(x.shape[0])])
            tru, end = limit_truth(x, ch, RATE, **kw)
            refs = (kw, contract, x, ref, tru, end)
        else:
            refs = _refs(O, setting, ch, frames)
            kw, contract, x, ref, tru, end = refs
        ref_state = limit_state_f32(x, ch, RATE, **kw).astype(np.float64)
        xd = torch.from_numpy(np.array(x)).cuda()
        S = x.shape[0]
        runs, worst = {}, (-1.0, "")
        st = torch.zeros((S, 2 * ch), device="cuda")
        runs["one pass"] = (_limit(G, xd, ch, kw, st), st.cpu().numpy(), [frames])
        for c, cut in STATE_CUTS:
            if c != ch:
                continue
            scan = (cut * ch) % 4 == 0 and ((frames - cut) * ch) % 4 == 0
            assert scan == (not (ch == 2 and cut == 8191))  # the one cut whose rows are no 16-byte multiples: the reference-order kernel
            st = torch.zeros((S, 2 * ch), device="cuda")
            a = _limit(G, xd[:, : cut * ch].contiguous(), ch, kw, st)
            b = _limit(G, xd[:, cut * ch:].contiguous(), ch, kw, st)
            runs[f"cut {cut}"] = (np.concatenate([a, b], axis=1), st.cpu().numpy(), [cut, frames - cut] if scan else [frames])
        G.async_status()
        for what, (out, state, lengths) in runs.items():
            ms = _hold(out, refs, ch, lengths, f"limit {setting} state ch{ch} n{frames} {what}")
            # the state left behind, {integrator, peak} per channel in dB: criterion B with the e_ref of the STATE (the reference's own f32
            # recurrences, dynamics_signals.limit_state_f32) and the state's own slack (limit_state_slack: no output roundings)
            got = state.reshape(S, ch, 2).astype(np.float64)
            assert np.isfinite(state).all()
            for s in range(S):
                err, e_ref = float(np.max(np.abs(got[s] - end[s]))), float(np.max(np.abs(ref_state[s] - end[s])))
                Fs = limit_F(x[s], kw, ch, lengths, state=True)
                line = f"[{ms[s][0]}] state: |gpu-f64|={err:.3e} dB |f32-f64|={e_ref:.3e} dB F={Fs:.3e} dB"
                worst = max(worst, (err / (2.0 * e_ref + Fs), line))
                assert err <= 2.0 * e_ref + Fs, ("state B", line)
        print(worst[1])


# ==================================================================================================== the AGC ====
def _agc_oracle(O, x, kw):
    return np.stack([O.TestSource(x[s], 1, RATE).automatic_gain_control(**kw).collect() for s in range(x.shape[0])])


def _agc(G, xd, kw, state=None):
    return G.agc_batch(xd, RATE, state=state, **kw)


def _agc_hold(got, ref, x, tag, names=AGC_SIGNALS, show=True):
    """Every row against the oracle (both bounds); prints the row furthest from it."""
    ms = [(agc_check(got[s], ref[s], x[s], f"{tag} {name}", show=False), name) for s, name in enumerate(names)]
    m, name = max(ms, key=lambda t: (t[0]["ulps"], t[0]["d"]))
    if show:
        print(f"[{tag}] worst {name}: |gpu-oracle|={m['d']:.3e} peak={m['peak']:.3e} ulps of the oracle's value={m['ulps']:.2f} (bound 2.00)")


def _same(a, b):
    import torch

    return torch.equal(a.view(torch.int32), b.view(torch.int32))


PROBE = 8  # samples of 0.01 played from the state a run leaves: they show the gain that exact silence in front of them hides


def _with_probe(x):
    return np.concatenate([x, np.full((x.shape[0], PROBE), 0.01, np.float32)], axis=1)


_TWIN = {}


def _twin_gain(setting, x):
    """The gain behind the last sample of every row of x, from the numpy-f32 twin of the default path (the oracle's bits on this bank:
    test_dynamics_signals_cpu.py) -- what the carried gain word is held to where the output is 0 * gain.  One run of 40 004 samples per
    setting serves every shorter length: the bank of n samples is a prefix of it."""
    if setting not in _TWIN:
        full = agc_rows(40004)
        _TWIN[setting] = (full, agc_default_twin(full, RATE, **AGC_SETTINGS[setting][0])[1])
    full, gains = _TWIN[setting]
    n = x.shape[1]
    assert x.shape[0] == full.shape[0] and np.array_equal(x, full[:, :n])
    return gains[:, n - 1]


def _forms(G, xd, kw, default_path, cuts=None, stateless=True):
    """name -> (output, final state, the probe's output, the output of the same call without a state) of every form: one call from a fresh
    state, or blocks at `cuts` with the state carried; then PROBE samples of 0.01 from the state that is left."""
    import torch

    forms = [("fused", {}), ("segments", dict(RH_AGC_SEGMENTS="1")), ("vec", dict(RH_AGC_VEC="1")), ("seq", dict(RH_AGC_SEQ="1"))]
    if default_path:
        forms.append(("r4", dict(RH_AGC_FUSED_R4="1")))
    cuts = (0, xd.shape[1]) if cuts is None else cuts
    probe = torch.full((xd.shape[0], PROBE), 0.01, device="cuda")
    out = {}
    for name, env in forms:
        with knobs(**env):
            st = G.agc_state(xd.shape[0])
            parts = [_agc(G, xd[:, i:j].contiguous(), kw, st) for i, j in zip(cuts[:-1], cuts[1:])]
            left = st.clone()
            out[name] = (torch.cat(parts, dim=1), left, _agc(G, probe, kw, st), _agc(G, xd, kw) if stateless else None)
    return out


def _canonical(state):
    """An AGC state as what it means: {sum, peak, gain} and the window's squares in time order.  The reference-order kernels keep the
    ring where its index stands; the chain and fused kernels hand it back rotated to index 0 (k_agc_window_in): the same state."""
    st = state.cpu().numpy().reshape(-1, 4 + 8192).view(np.uint32)
    rows = []
    for r in st:
        idx = int(r[1])
        assert idx < 8192
        rows.append(np.concatenate([r[[0, 2, 3]], np.roll(r[4:], -idx)]))
    return np.stack(rows)


def _between_forms(out, default_path, tag):
    """What the suite claims between the forms: outputs, the states left behind, and what those states do to the probe."""
    f, q = out["fused"], out["seq"]
    for a, b in [("fused", "segments"), ("vec", "seq")] + ([("r4", "fused")] if default_path else []):
        for k, what in ((0, "outputs"), (1, "states"), (2, "probe"), (3, "without a state")):
            if out[a][k] is not None:
                assert _same(out[a][k], out[b][k]), (tag, a, b, what)
    if not default_path:  # every operation the reference's: the reference-order kernel's bits, and the same state up to where the ring starts
        assert _same(f[0], q[0]) and _same(f[2], q[2]), (tag, "fused", "seq", "outputs")
        assert np.array_equal(_canonical(f[1]), _canonical(q[1])), (tag, "fused", "seq", "states")
    if default_path:  # select and clamps as one median: a rounding apart where two candidates tie
        assert float((f[0] - q[0]).abs().max()) <= 1e-6 and float((f[2] - q[2]).abs().max()) <= 1e-6, tag


def _hold_forms(out, ref_full, x, setting, tag, names=AGC_SIGNALS):
    """fused and seq (the others are one of the two bit for bit) against the oracle: the run, the same call without a state, and the probe
    behind it -- the oracle's continuation.  On the default path the gain word every form leaves is the twin's within 2^-22: where a row
    ends in exact silence (the residue rows, silence itself) nothing else shows what agc_desired1 and GainOp0 made of the window sum, and
    with attack 0 not even the probe does (its gain is its own desired)."""
    n = x.shape[1]
    for form in ("fused", "seq"):
        _agc_hold(out[form][0].cpu().numpy(), ref_full[:, :n], x, f"{tag} {form}", names)
        if out[form][3] is not None:
            _agc_hold(out[form][3].cpu().numpy(), ref_full[:, :n], x, f"{tag} {form} without a state", names, show=False)
        _agc_hold(out[form][2].cpu().numpy(), ref_full[:, n:], _with_probe(x)[:, n:], f"{tag} {form} probe", names)
    if AGC_SETTINGS[setting][1] and len(names) == len(AGC_SIGNALS):
        want = _twin_gain(setting, x).astype(np.float64)
        for form, o in out.items():
            got = o[1].cpu().numpy().reshape(len(names), -1)[:, 3].astype(np.float64)
            bad = np.flatnonzero(~(np.abs(got - want) <= AGC_ULPS * want))
            assert bad.size == 0, (tag, form, "the gain left behind", [(names[i], float(got[i]), float(want[i])) for i in bad])


@pytest.mark.parametrize("n", [127, 8492, 20000, 40004])
@pytest.mark.parametrize("setting", list(AGC_SETTINGS))
def test_dynamics_agc_bank(G, O, setting, n):
    """The whole bank in one launch: 127 (rows of 127 samples are no 16-byte multiples: the reference-order kernel for the launch; each row on
    its own is the fused kernel's epilogue), 8492 (one window wrap), 20 000 (ceiling and floor reached, the window emptied), 40 004 (above the
    segment form's square pass, 32 768)."""
    import torch

    kw, default_path = AGC_SETTINGS[setting]
    x = agc_rows(n)
    ref = _agc_oracle(O, _with_probe(x), kw)
    xd = torch.from_numpy(x).cuda()
    out = _forms(G, xd, kw, default_path)
    tag = f"agc {setting} n{n}"
    _between_forms(out, default_path, tag)
    _hold_forms(out, ref, x, setting, tag)
    if n == 127:  # one row per call: 16-byte aligned whatever its length -- the fused kernels, everything in their epilogue
        for s, name in enumerate(AGC_SIGNALS):
            row = _forms(G, xd[s: s + 1].clone(), kw, default_path)
            _between_forms(row, default_path, f"{tag} {name} alone")
            for k in (0, 3):
                agc_check(row["fused"][k].cpu().numpy()[0], ref[s, :n], x[s], f"{tag} fused {name} alone", show=False)
            agc_check(row["fused"][2].cpu().numpy()[0], ref[s, n:], _with_probe(x)[s, n:], f"{tag} fused {name} alone, probe", show=False)


@pytest.mark.parametrize("setting", list(AGC_SETTINGS))
def test_dynamics_agc_one_odd_stream(G, O, setting):
    """One stream of 40 001 samples of tail_then_dc: the window fills, empties completely and refills; a tail shorter than a chunk."""
    import torch

    kw, default_path = AGC_SETTINGS[setting]
    x = agc_bank(40001)["tail_then_dc"][None, :]
    ref = _agc_oracle(O, _with_probe(x), kw)
    out = _forms(G, torch.from_numpy(x).cuda(), kw, default_path)
    _between_forms(out, default_path, f"agc {setting} 40001")
    _hold_forms(out, ref, x, setting, f"agc {setting} n40001", names=("tail_then_dc",))


@pytest.mark.parametrize("cuts", [(8192, 16384, 24576), (8191, 8192, 8193, 16384, 24576)], ids=["aligned", "all"])
@pytest.mark.parametrize("setting", list(AGC_SETTINGS))
def test_dynamics_agc_state_across_blocks(G, O, setting, cuts):
    """The window empties and refills across block boundaries.  `aligned`: every block is the fused kernel's (or the form's under test); `all`:
    blocks of 8191, 1, 1 and 8191 samples are no 16-byte multiples and take the reference-order kernel -- the state passes between the two."""
    import torch

    kw, default_path = AGC_SETTINGS[setting]
    n = 40000
    x = agc_rows(n)
    ref = _agc_oracle(O, _with_probe(x), kw)
    xd = torch.from_numpy(x).cuda()
    whole = _agc(G, xd, kw)
    out = _forms(G, xd, kw, default_path, cuts=(0,) + tuple(cuts) + (n,), stateless=False)
    tag = f"agc {setting} n{n} blocks {'-'.join(str(c) for c in cuts)}"
    _between_forms(out, default_path, tag)
    blocks = out["fused"][0]
    if default_path:
        assert float((blocks - whole).abs().max()) <= 1e-6, tag  # (a block boundary moves nothing but GainOp0's tie)
    else:
        assert _same(blocks, whole), tag
    _hold_forms(out, ref, x, setting, tag)
    # the state left behind: the window's squares are the input's, the sum is tail_then_dc's refilled window exactly
    st = out["fused"][1].cpu().numpy().reshape(len(AGC_SIGNALS), -1)
    assert np.isfinite(st[:, [0, 2, 3]]).all()
    i = AGC_SIGNALS.index("tail_then_dc")
    assert st[i, 0] == 512.0 and np.all(st[i, 4:] == np.float32(0.0625))


def test_dynamics_agc_silence_from_a_fresh_state_with_attack_0(G, O):
    """rh_agc_state_init, then silence with attack 0: desired is the ceiling (neither level is > 0) and the gain is exactly 7.0 from the first
    sample on -- read from the state (0 * gain says nothing) and from a sample of 0.01 behind the silence."""
    import torch

    kw = AGC_SETTINGS["attack0"][0]
    for S, first in ((1, 1), (3, 4)):
        st = G.agc_state(S)
        assert np.all(st.cpu().numpy().reshape(S, -1)[:, 3] == 1.0)  # a fresh AGC starts at 1.0
        for n in (first, 4096, 8192 + 4):
            out = _agc(G, torch.zeros((S, n), device="cuda"), kw, st)
            assert not out.cpu().numpy().any()
            assert np.all(st.cpu().numpy().reshape(S, -1)[:, 3] == np.float32(7.0)), (S, n)
        probe = torch.full((S, 4), 0.01, device="cuda")
        out = _agc(G, probe, kw, st).cpu().numpy()
        assert np.all(out == np.float32(0.01) * np.float32(7.0)), out
        ref = O.TestSource(np.concatenate([np.zeros(first + 4096 + 8192 + 4, np.float32), np.full(4, 0.01, np.float32)]), 1, RATE).automatic_gain_control(**kw).collect()
        assert np.array_equal(ref[-4:], out[0])
