"""A mixer or player that runs for days: the 32-bit counters that live across launches, taken past their limits.

Every other test runs a handle for at most a few thousand launches.  RH_COUNTER_JUMP=<after>:<tickets_left>:<launches_left>
 moves the counters of a handle (or of the scan kernels' per-stream scratch) forward at its after-th launch, as
though the launches in between had run: the ticket counters to `tickets_left` tickets before they wrap (so the wrap falls inside the
next launch), the epoch tag of the aggregate / halo / sblk tables to `launches_left` tags before its re-base.  Only the words that wait
for the next launch (a per-source stream's states) move with the epoch: the tables keep the low tags of the launches before the jump,
and a re-base that let them pass as fresh words would show as wrong samples (every run below mixes new samples).  Each case runs a
sequence of calls across those marks and checks it three ways: bit for bit against the same sequence without the knob (the counters
must never reach the arithmetic; that sequence first repeats itself bit for bit), against the oracle's chains with the tolerance the
suite uses for that kernel, and for a clean status (no NaN, the handle's and the scan kernels' sticky flags clear).

The elementwise adapters that take a sample offset are checked where it crosses 2^32 samples."""
import ctypes as C

import numpy as np
import pytest
from conftest import knobs

pytestmark = pytest.mark.gpu
TOL = 1e-5


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available()
    rh.init(0)
    return rh


def rnd(seed, n, scale=1.0):
    return (np.random.default_rng(seed).uniform(-1, 1, n) * scale).astype(np.float32)


def _mix_oracle(O, xs, frm, to, ch, filters, gains=None):
    m = O.Mixer(ch, to)
    for i, (x, f) in enumerate(zip(xs, filters)):
        src = O.TestSource(x, ch, frm)
        if gains is not None:
            src = src.amplify(float(gains[i]))
        u = O.UniformSourceIterator(src, ch, to)
        if f is not None:
            u = u.low_pass(f[1]) if f[0] == "low_pass" else u.high_pass(f[1])
        m.add(u)
    return m.collect()


def _three_ways(runs, jumped, refs, tol=TOL):
    """runs: two sequences without the knob, jumped: the sequence with it, refs: the oracle's results (None: not compared)."""
    a, b = runs
    assert len(a) == len(b) == len(jumped)
    for k, (x, y, z) in enumerate(zip(a, b, jumped)):
        assert np.array_equal(x, y), f"call {k}: the sequence does not repeat itself bit for bit"
        assert not np.isnan(z).any(), f"call {k}: NaN"
        assert np.array_equal(x, z), f"call {k}: differs from the sequence without the jump (max {float(np.max(np.abs(x - z))):.3e})"
        if refs is not None and refs[k] is not None:
            assert z.shape == refs[k].shape, (k, z.shape, refs[k].shape)
            err = float(np.max(np.abs(z - refs[k])))
            assert err <= tol, (k, err)


# ---- one-shot runs of the fused path ----------------------------------------------------------------------------------------------
# A sequence of runs of one handle, new samples every time (stale aggregates of an earlier run would then show), the jump at the
# second run: tickets wrap inside the third launch, and the epoch re-bases two runs later.
ONE_SHOT = {
    # name: (sources, frames, filters (None: the handle's one), exclusive, mix first, batch)
    "fast ticketed": (5, 30000, None, False, False, False),
    "fast direct": (5, 30000, None, True, False, False),
    "chunk": (12, 60000, None, False, True, False),
    "chunk direct": (12, 60000, None, True, True, False),
    "chunk classes": (6, 40000, [("low_pass", 200), ("high_pass", 1000), ("low_pass", 200), ("low_pass", 3000), ("high_pass", 1000), ("low_pass", 3000)], True, True, False),
    "batch sharded": (32, 6000, None, False, False, True),
}


def _one_shot_sequence(G, name, calls=6):
    import torch

    S, n, filters, excl, mf, batch = ONE_SHOT[name]
    p = G.ResampleLowpassMix(44100, 48000, 2, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=n)
    if filters is not None:
        p.set_filters(filters)
    p.set_exclusive(excl)
    p.set_mix_first(mf)
    outs = []
    for k in range(calls):
        xs = [rnd(7000 + 100 * k + s, 2 * n, 0.5 / S) for s in range(S)]
        p.set_sources([torch.from_numpy(x).cuda() for x in xs])
        out = p.run_batch() if batch else p.run()
        p.check_status()
        outs.append(out.cpu().numpy())
    p.close()
    return outs


@pytest.mark.parametrize("name", list(ONE_SHOT))
def test_one_shot_runs_across_the_ticket_wrap_and_the_epoch_rebase(G, O, name):
    S, n, filters, _, _, batch = ONE_SHOT[name]
    runs = [_one_shot_sequence(G, name) for _ in range(2)]
    with knobs(RH_COUNTER_JUMP="2:5:2"):
        jumped = _one_shot_sequence(G, name)
    refs = []
    for k in range(len(jumped)):
        xs = [rnd(7000 + 100 * k + s, 2 * n, 0.5 / S) for s in range(S)]
        if batch:
            refs.append(np.stack([_mix_oracle(O, [x], 44100, 48000, 2, [("low_pass", 200)]) for x in xs]) if k in (1, 2, 4) else None)
        else:
            refs.append(_mix_oracle(O, xs, 44100, 48000, 2, filters or [("low_pass", 200)] * S))
    _three_ways(runs, jumped, refs)
    G.async_status()


# ---- block streaming ----------------------------------------------------------------------------------------------------------
def _summed_stream(G, overlap, S=7, N=360_000, B=40_000, ch=2):
    """Resident rows read at `row + consumed`, every block summed in one launch (k_rlm_sblk); test_gpu_mix_first.py's shape."""
    import torch
    from rodio_amd import _lib

    lib = _lib.lib
    xs = [rnd(9900 + s, ch * N, 0.15) for s in range(S)]
    gains = np.linspace(0.4, 1.3, S).astype(np.float32)
    data = torch.from_numpy(np.stack(xs)).cuda()
    mo = C.c_uint64(0)
    _lib.check(lib.rh_resample_out_frames(N, 44100, 48000, ch, 0, C.byref(mo)), "rh_resample_out_frames")
    M = mo.value
    p = G.ResampleLowpassMix(44100, 48000, ch, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=B + 4096)
    p.set_gains(gains)
    p.stream_begin(keep_history=True)
    _lib.check(lib.rh_rlm_stream_overlap(p._h, 1 if overlap else 0), "rh_rlm_stream_overlap")
    out = torch.zeros(ch * M + 4096, device="cuda", dtype=torch.float32)
    g0 = m = k = 0
    chained = []
    while True:
        hi = min(N, (k + 1) * B)
        ptrs = (C.c_void_p * S)(*[data[s_].data_ptr() + g0 * 4 * ch for s_ in range(S)])
        avail = (C.c_uint64 * S)(*([hi - g0] * S))
        ended = (C.c_uint8 * S)(*([1 if hi == N else 0] * S))
        o, c = C.c_uint64(0), C.c_uint64(0)
        _lib.check(lib.rh_rlm_stream_block_v(p._h, ptrs, avail, ended, S, C.c_void_p(out.data_ptr() + m * 4 * ch), M + 512 - m, C.byref(o), C.byref(c), None), "rh_rlm_stream_block_v")
        ovl = C.c_uint32(0)
        _lib.check(lib.rh_rlm_stream_overlapped_blocks(p._h, C.byref(ovl)), "rh_rlm_stream_overlapped_blocks")
        chained.append(ovl.value)
        m += o.value
        g0 += c.value
        k += 1
        if hi == N:
            break
    p.check_status()
    one = C.c_uint32(0)
    _lib.check(lib.rh_rlm_stream_one_launch_blocks(p._h, C.byref(one)), "rh_rlm_stream_one_launch_blocks")
    res = out[: ch * m].cpu().numpy()
    p.close()
    return res, chained, one.value, xs, gains


@pytest.mark.parametrize("overlap", [False, True])
def test_summed_stream_across_the_epoch_rebase(G, O, overlap):
    """k_rlm_sblk's blocks, with and without rh_rlm_stream_overlap, across the re-base of the epoch (in front of block 3 of 0..8): its
    three rotating sets of aggregates and hand-off words keep their tags relative to the epoch, and blocks behind it run side by side
    again."""
    a, ca, one_a, xs, gains = _summed_stream(G, overlap)
    b, _, _, _, _ = _summed_stream(G, overlap)
    with knobs(RH_COUNTER_JUMP="2:5:2"):
        j, cj, one_j, _, _ = _summed_stream(G, overlap)
    ref = _mix_oracle(O, xs, 44100, 48000, 2, [("low_pass", 200)] * len(xs), gains)
    _three_ways([[a], [b]], [j], [ref])
    nb = len(cj)
    assert one_a == one_j == nb, (one_a, one_j, nb)
    # which blocks started without a barrier behind the block in front: as without the jump, except the two blocks that something was
    # queued in front of -- the jump (block 1) and the re-base (block 3)
    fa, fj = np.diff([0] + ca), np.diff([0] + cj)
    want = fa.copy()
    want[[1, 3]] = 0
    assert np.array_equal(fj, want), (ca, cj)
    if overlap:
        assert ca[-1] >= nb - 3 and int(np.sum(fj[4:])) >= 3, (ca, cj)  # the chained path ran behind the re-base
    else:
        assert ca[-1] == 0


def _per_source_stream(G, hist, ns, cuts, S=6, filt="low_pass", freq=200):
    import torch

    gains = np.linspace(0.5, 1.3, S).astype(np.float32)
    xs = [rnd(7100 + i, 2 * n, 0.15) for i, n in enumerate(ns)]
    xd = [torch.from_numpy(x).cuda() for x in xs]
    p = G.ResampleLowpassMix(44100, 48000, 2, None, filt, freq, 0.5, max_sources=S, max_in_frames=max(ns))
    p.set_gains(gains)
    p.stream_begin(keep_history=hist)
    outs = []
    fed = [0] * S
    for k in range(len(cuts) - 1):
        hi = cuts[k + 1]
        blocks, ended = [], []
        for s_, (x, n) in enumerate(zip(xd, ns)):
            a, b = min(fed[s_], n), min(hi, n)
            blocks.append(x[2 * a: 2 * b])
            fed[s_] = b
            ended.append(b >= n)
        outs.append(p.stream_feed_v(blocks, ended))
    p.check_status()
    got = torch.cat(outs).cpu().numpy()
    stats = p.stream_stats()
    p.close()
    return got, stats, xs, gains


# "end apart, together again" of test_gpu_mix_first.py: per-source blocks, then back on the summed state (the rejoin's increment of
# the epoch behind k_rlm_state_sum), then per-source again.  launches_left moves the re-base over the stream's launches: per-source
# blocks (k_rlm_wave with live column-0 states), the rejoin increment, summed blocks, the recovery replay.
REJOIN = ([200000, 60000, 200000, 130000, 200000, 200000], list(range(0, 200001, 25000)))
APART = ([90000, 61000, 90000, 45000, 90000, 40000], [0, 25000, 50000, 75000, 90000])


# The jump comes at the handle's third tag (its tables then hold the tags of two launches) -- the per-source case without history at
# the first, where the states of the stream's first block are the only words that wait.
@pytest.mark.parametrize("case,hist,after,left", [("rejoin", True, 3, left) for left in (1, 2, 3, 4, 5, 6, 7, 8, 9)] + [("apart", False, a, 1) for a in (1, 2, 3)])
def test_per_source_stream_across_the_epoch_rebase(G, O, case, hist, after, left):
    ns, cuts = {"rejoin": REJOIN, "apart": APART}[case]
    a, st_a, xs, gains = _per_source_stream(G, hist, ns, cuts)
    b, _, _, _ = _per_source_stream(G, hist, ns, cuts)
    with knobs(RH_COUNTER_JUMP=f"{after}:3:{left}"):
        j, st_j, _, _ = _per_source_stream(G, hist, ns, cuts)
    ref = _mix_oracle(O, xs, 44100, 48000, 2, [("low_pass", 200)] * len(xs), gains)
    _three_ways([[a], [b]], [j], [ref])
    assert st_a == st_j, (st_a, st_j)
    if case == "rejoin":
        assert st_a == (6, 2, 2), st_a  # the blocks ran the way test_gpu_mix_first.py pins them


# ---- streams that run past 2^31 / 2^32 frames ---------------------------------------------------------------------------------
# RH_STREAM_START=<k>: rh_rlm_stream_begin starts the stream k periods of the converter in -- k * F input and k * T
# output frames of the reduced ratio (44.1 -> 48 kHz: 147 / 160), or k whole spans.  The converter's arithmetic at frame k * T is its
# arithmetic at 0, and the filter starts from a zero state either way, so every block -- the first one included -- must be the bits of
# the same stream started at 0.  k is chosen so that the stream crosses the mark a few blocks in: the kernels then work at global
# positions past 2^31 / 2^32 (Params::st_m0 / st_g0, the cursor, k_rlm_sblk's block-relative offsets).
S_MARK, N_MARK, B_MARK = 4, 60_000, 20_000


def _span_period(ch, span):
    from rodio_amd import _lib

    cin = span // ch
    o = C.c_uint64(0)
    _lib.check(_lib.lib.rh_resample_out_frames(cin, 44100, 48000, ch, 0, C.byref(o)), "rh_resample_out_frames")
    return cin, o.value


def _start_below(mark, ch, span, side):
    """k that puts the stream's start ~half a stream in front of `mark` output (side 'out') or input (side 'in') frames."""
    fi, fo = _span_period(ch, span) if span else (147, 160)
    per = fo if side == "out" else fi
    back = (N_MARK // 2) * (160 if side == "out" else 147) // 147
    return (mark - back) // per


def _mark_stream(G, ch, span, kind):
    import torch

    ns = [N_MARK] * S_MARK if kind == "summed" else [N_MARK, 41_000, N_MARK, 27_000]
    xs = [rnd(5100 + 7 * ch + i, ch * n, 0.2) for i, n in enumerate(ns)]
    xd = [torch.from_numpy(x).cuda() for x in xs]
    p = G.ResampleLowpassMix(44100, 48000, ch, span, "low_pass", 200, 0.5, max_sources=S_MARK, max_in_frames=B_MARK + 8192)
    p.stream_begin()
    cuts = list(range(0, N_MARK + 1, B_MARK))
    outs = []
    if kind == "summed":
        for k in range(len(cuts) - 1):
            outs.append(p.stream_feed([x[ch * cuts[k]: ch * cuts[k + 1]] for x in xd], flush=(k == len(cuts) - 2)).cpu().numpy())
    else:
        fed = [0] * S_MARK
        for k in range(len(cuts) - 1):
            blocks, ended = [], []
            for s_, (x, n) in enumerate(zip(xd, ns)):
                a, b = min(fed[s_], n), min(cuts[k + 1], n)
                blocks.append(x[ch * a: ch * b])
                fed[s_] = b
                ended.append(b >= n)
            outs.append(p.stream_feed_v(blocks, ended).cpu().numpy())
    p.check_status()
    p.close()
    return outs, xs


MARKS = [("out", 1 << 31), ("out", 1 << 32), ("in", 1 << 32)]


@pytest.mark.parametrize("ch,span,kind", [(2, None, "summed"), (1, None, "summed"), (2, None, "per source"), (1, None, "per source"), (2, 4096, "summed"), (1, 4096, "per source")])
def test_streams_started_just_below_2_31_and_2_32_frames(G, O, ch, span, kind):
    base, xs = _mark_stream(G, ch, span, kind)
    again, _ = _mark_stream(G, ch, span, kind)
    assert all(np.array_equal(x, y) for x, y in zip(base, again))
    m = O.Mixer(ch, 48000)
    for x in xs:
        src = O.SpanSource(x, ch, 44100, span) if span else O.TestSource(x, ch, 44100)
        m.add(O.UniformSourceIterator(src, ch, 48000).low_pass(200))
    ref = m.collect()
    got0 = np.concatenate(base)
    assert got0.shape == ref.shape and float(np.max(np.abs(got0 - ref))) <= TOL
    fi, fo = _span_period(ch, span) if span else (147, 160)
    for side, mark in MARKS:
        k = _start_below(mark, ch, span, side)
        m0, g0 = k * fo, k * fi
        end = (m0 + len(got0) // ch) if side == "out" else (g0 + N_MARK)
        assert (m0 if side == "out" else g0) < mark < end, (side, mark, k)  # the stream crosses the mark
        with knobs(RH_STREAM_START=str(k)):
            shifted, _ = _mark_stream(G, ch, span, kind)
        assert len(shifted) == len(base)
        for blk, (x, y) in enumerate(zip(base, shifted)):
            assert not np.isnan(y).any(), (side, mark, blk)
            assert np.array_equal(x, y), (side, mark, blk, x.shape, y.shape)
    G.async_status()


# ---- the scan kernels: the ticket counter of the per-stream scratch ---------------------------------------------------------------
def _limit_signal(seed, n, ch, loud=2.0):
    rng = np.random.default_rng(seed)
    t = np.arange(n, dtype=np.float64)
    x = np.zeros((n, ch))
    for c in range(ch):
        env = 0.15 + 0.85 * np.abs(np.sin(2 * np.pi * t / (3000.0 + 977.0 * c) + rng.uniform(0, 6)))
        x[:, c] = loud * env * np.sin(2 * np.pi * t * (0.01 + 0.003 * c)) + 0.1 * rng.standard_normal(n)
    return x.astype(np.float32).reshape(-1)


LIM_A = (5, 40000)  # streams, frames
BQ_B = (3, 70000)


def _scan_calls(G):
    """The interleaved sequence on one stream: limit shape A, biquad shape B, an AGC, limit A three times, limit A with a carried
    state, limit A -- the scratch's shared ScratchAux, both parity tables and the "clean" shortcut in turn."""
    import torch

    xa = torch.from_numpy(np.stack([_limit_signal(500 + s, LIM_A[1], 2) for s in range(LIM_A[0])])).cuda()
    xb = torch.from_numpy(np.stack([rnd(600 + s, 2 * BQ_B[1], 0.8) for s in range(BQ_B[0])])).cuda()
    co = G.biquad_coeffs("low_pass", 1000, 0.5, 48000)
    st = torch.zeros((LIM_A[0], 4), device="cuda")
    calls = [
        ("limit", lambda: G.limit_batch(xa, 2, 48000)),
        ("biquad", lambda: G.biquad_batch(xb, co, mode=1)),
        ("agc", lambda: G.agc_batch(xb, 48000)),
        ("limit", lambda: G.limit_batch(xa, 2, 48000)),
        ("limit", lambda: G.limit_batch(xa, 2, 48000)),
        ("limit", lambda: G.limit_batch(xa, 2, 48000)),
        ("limit state", lambda: G.limit_batch(xa, 2, 48000, state=st)),
        ("limit", lambda: G.limit_batch(xa, 2, 48000)),
        ("biquad", lambda: G.biquad_batch(xb, co, mode=1)),
    ]
    return calls, xa, xb, co


def _scan_sequence(G):
    calls, _, _, _ = _scan_calls(G)
    outs = [f().cpu().numpy() for _, f in calls]
    G.async_status()
    return outs


@pytest.mark.parametrize("after", [1, 2, 4, 6])  # scan launches: limit, biquad, (agc), limit, limit, limit, limit with state, limit, biquad
def test_scan_kernels_across_the_ticket_wrap(G, O, after):
    """RH_COUNTER_JUMP at the after-th scan launch: the limiter (alone, behind the biquad, with a carried state) or rh_biquad mode 1
    takes tickets across 2^32 inside one launch.  Every result equals the same call made alone (RH_LIMIT_INIT=1: tables written in
    front of every launch) and the oracle."""
    runs = [_scan_sequence(G) for _ in range(2)]
    with knobs(RH_COUNTER_JUMP=f"{after}:7:0"):
        jumped = _scan_sequence(G)
    with knobs(RH_LIMIT_INIT="1"):
        calls, xa, xb, co = _scan_calls(G)
        alone = [f().cpu().numpy() for _, f in calls]
        G.async_status()
    xa_h, xb_h = xa.cpu().numpy(), xb.cpu().numpy()
    refs = []
    for name, _ in calls:
        if name.startswith("limit"):
            refs.append(np.stack([O.TestSource(r, 2, 48000).limit().collect() for r in xa_h]))
        elif name == "biquad":
            refs.append(np.stack([O.TestSource(r, 2, 48000).low_pass(1000).collect() for r in xb_h]))
        else:
            refs.append(None)
    _three_ways(runs, jumped, refs)
    for k, (x, y) in enumerate(zip(jumped, alone)):
        assert np.array_equal(x, y), (k, calls[k][0])


# ---- sample offsets past 2^32 -----------------------------------------------------------------------------------------------
def _ramp_f64(n, offset, ch, rate, dur_ns, a, b, clamp):
    """linear_ramp.rs:79-110 restated: frame f = (offset + i) / ch ramps with elapsed = f * (1e9 / rate) ns until elapsed >= total."""
    k = offset + np.arange(n, dtype=np.uint64)
    f = k // np.uint64(ch)
    step = 1_000_000_000 // rate
    elapsed = f * np.uint64(step)
    p = elapsed.astype(np.float64) / float(dur_ns)
    g = a * (1.0 - p) + b * p
    done = elapsed >= np.uint64(dur_ns)
    g[done] = b if clamp else 1.0
    return g


def test_elementwise_adapters_at_sample_offsets_past_2_32(G):
    import torch
    from rodio_amd import _lib

    lib = _lib.lib
    n = 1 << 16
    x = rnd(77, n, 0.8)
    xd = torch.from_numpy(x).cuda()
    for ch in (1, 2, 6):
        for base in ((1 << 32) - n // 2 - 3, ((1 << 32) * ch) - n // 2 - 1):
            base -= base % ch
            # dither: one call straddling the mark equals its two halves; offset 2^32 + i is not offset i
            one = G.TestSource(x, ch, 48000).dither(16, "TPDF", 5, sample_offset=base).collect()
            cut = n // 2 + 3
            h1 = G.TestSource(x[:cut], ch, 48000).dither(16, "TPDF", 5, sample_offset=base).collect()
            h2 = G.TestSource(x[cut:], ch, 48000).dither(16, "TPDF", 5, sample_offset=base + cut).collect()
            assert np.array_equal(one, np.concatenate([h1, h2])), (ch, base)
            hi = G.TestSource(x, ch, 48000).dither(16, "TPDF", 5, sample_offset=(1 << 32) * ch).collect()
            low = G.TestSource(x, ch, 48000).dither(16, "TPDF", 5, sample_offset=0).collect()
            assert float(np.mean(hi != low)) > 0.5, ch  # the counter is 64-bit: no repeat of the noise after 2^32 samples
            # linear_gain_ramp across the mark: halves, and the f64 restatement of linear_ramp.rs
            rate = 48000
            dur = int((base // ch + n // (2 * ch)) * (1_000_000_000 // rate)) + 123  # ends inside the block
            for clamp in (False, True):
                one = G.TestSource(x, ch, rate).linear_gain_ramp(dur, 0.2, 1.5, clamp, sample_offset=base).collect()
                h1 = G.TestSource(x[:cut], ch, rate).linear_gain_ramp(dur, 0.2, 1.5, clamp, sample_offset=base).collect()
                h2 = G.TestSource(x[cut:], ch, rate).linear_gain_ramp(dur, 0.2, 1.5, clamp, sample_offset=base + cut).collect()
                assert np.array_equal(one, np.concatenate([h1, h2])), (ch, base, clamp)
                want = x.astype(np.float64) * _ramp_f64(n, base, ch, rate, dur, 0.2, 1.5, clamp)
                assert float(np.max(np.abs(one - want))) <= 1e-6 * 1.5 + 1e-7, (ch, base, clamp)
            # take_duration: a duration that expires inside the block, past 2^32 samples of the stream (take.rs:96-148)
            dps = 1_000_000_000 // (rate * ch)
            if dps == 0:
                continue
            expire = base + n // 2 + 1  # samples admitted
            dur = expire * dps + dps // 2
            for fade in (0, 1):
                out = torch.empty(n + ch, device="cuda", dtype=torch.float32)
                m, ended = C.c_uint64(0), C.c_int32(0)
                _lib.check(lib.rh_take_duration(C.c_void_p(out.data_ptr()), C.c_void_p(xd.data_ptr()), n, base, ch, rate, dur, fade, C.byref(m), C.byref(ended), None), "rh_take_duration")
                torch.cuda.synchronize()
                take = expire - base
                pad = (ch - (expire % ch)) % ch
                assert m.value == take + pad and ended.value == 1, (ch, base, m.value, take, pad)
                got = out[: m.value].cpu().numpy()
                rem = dur - (base + np.arange(take, dtype=np.uint64)) * np.uint64(dps)  # remaining_duration in front of sample i
                want = x[:take].astype(np.float64) * ((rem // np.uint64(1_000_000)).astype(np.float64) / float(dur // 1_000_000) if fade else 1.0)
                assert float(np.max(np.abs(got[:take] - want))) <= 3e-7, (ch, base, fade)  # (f32 arithmetic: a few units of the last place)
                assert np.all(got[take:] == 0.0)
