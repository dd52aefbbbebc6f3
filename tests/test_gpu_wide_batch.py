"""rh_wide_mix_batch: the current block of many mixers of any channel count in ONE launch.  Every mixer's block must hold the bits
rh_wide_mix_block writes for it (the entry that exists since round 6), and -- without that entry -- the oracle's mixer (mixer.rs order).
Every comparison is on 32-bit patterns.  The case data is tests/wide_batch_cases.py.

How many launches a call makes is not tested here: the project counts launches with a kernel trace of a tool's run (tools/bench_wide.py),
which a test cannot call; DESIGN.md states the count from the code."""
import ctypes as C

import numpy as np
import pytest

import arena
import stream_gate
import wide_batch_cases as WB

pytestmark = pytest.mark.gpu
f32 = np.float32
INVALID, UNSUPPORTED = 1, 3


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _st():
    from rodio_amd import source

    return source._stream()


def vp(a):
    return C.c_void_p(a) if a is not None else None


def _upload(mixers):
    """Every source's rows in a device tensor of its own (a source without rows: None)"""
    import torch

    return [[torch.from_numpy(s["x"]).cuda() if s["x"].size else None for s in srcs] for _, _, _, srcs in mixers]


def _tables(mixers, ptrs):
    """-> per mixer a WideSrc array (ptrs: per mixer, per source a device address or None)"""
    from rodio_amd import _lib

    out = []
    for (_, _, _, srcs), pp in zip(mixers, ptrs):
        arr = (_lib.WideSrc * max(len(srcs), 1))()
        WB.fill_table(arr, 0, srcs, pp)
        out.append((arr, len(srcs)))
    return out


def _one_by_one(mixers, tables):
    """The existing entry, a call per mixer: what the batch must equal"""
    import torch

    from rodio_amd import _lib

    outs = []
    for (ch, rate, M, _), (arr, n) in zip(mixers, tables):
        dst = torch.full((M * ch,), float("nan"), device="cuda")
        _lib.check(_lib.lib.rh_wide_mix_block(vp(dst.data_ptr()), ch, rate, M, arr, n, _st()), "rh_wide_mix_block")
        outs.append(dst)
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in outs]


def _batched(G, mixers, tables):
    import torch

    dsts = [torch.full((M * ch,), float("nan"), device="cuda") for ch, _, M, _ in mixers]
    G.wide_mix_batch(dsts, [m[0] for m in mixers], [m[1] for m in mixers], [m[2] for m in mixers], [[arr[k] for k in range(n)] for arr, n in tables])
    torch.cuda.synchronize()
    return [d.cpu().numpy() for d in dsts]


@pytest.fixture(scope="module")
def mixed(G):
    """The five mixers of the first test, their rows on the device, and each mixer's block by rh_wide_mix_block (computed once, shared)"""
    mixers = WB.mixed_batch()
    rows = _upload(mixers)
    tables = _tables(mixers, [[r.data_ptr() if r is not None else None for r in rr] for rr in rows])
    return dict(mixers=mixers, rows=rows, tables=tables, want=_one_by_one(mixers, tables))


def test_a_mixed_batch_equals_the_existing_entry_mixer_by_mixer(G, mixed):
    """Five mixers in one call: no sources; one; five; 37 sources of six rates and three layouts (the old entry's chunk of 32 and its four
    (rate, phase) pairs both crossed); four.  Blocks that are not the stream's first, sources that end inside the block, sources of no
    frames with NULL data, F == T, -0.0 samples, zero and negative gains."""
    shapes = [(ch, rate, M, len(s)) for ch, rate, M, s in mixed["mixers"]]
    assert shapes == [(1, 48000, 1, 0), (2, 44100, 257, 1), (6, 48000, 1000, 5), (3, 96000, 4099, 37), (2, 48000, 64, 4)]
    got = _batched(G, mixed["mixers"], mixed["tables"])
    for b, (g, w) in enumerate(zip(got, mixed["want"])):
        assert np.all(np.isfinite(w)) and g.shape == w.shape
        assert np.array_equal(_bits(g), _bits(w)), (b, int(np.flatnonzero(_bits(g) != _bits(w))[0]))
    assert np.array_equal(_bits(got[0]), _bits(np.zeros(1, f32)))  # a mixer without sources: +0.0


def _three_blocks_against_the_oracle(G, specs, seed):
    """specs: per mixer (channels, rate, [(source channels, rate, gain, frames)]).  Every mixer's stream in three consecutive batched blocks
    (phase and data advanced by the caller), against the oracle's mixer over the whole stream."""
    import torch

    from rodio_amd import _lib
    from test_gpu_widemix import _oracle

    assert len(specs) >= 2  # (a call of one mixer may be handed to rh_wide_mix_block)
    rng = np.random.default_rng(seed)
    mixers = []
    for ch, rate, ss in specs:
        srcs = [(WB.signal(rng, n * c), c, r, g) for c, r, g, n in ss]
        total = max(WB.out_frames(len(x) // c, *WB.reduced(r, rate)) for x, c, r, _ in srcs)
        mixers.append(dict(ch=ch, rate=rate, srcs=srcs, dev=[torch.from_numpy(x).cuda() for x, *_ in srcs], total=total, want=_oracle(srcs, ch, rate), parts=[]))
    assert all(m["want"].size == m["total"] * m["ch"] for m in mixers)
    for k in range(3):
        dsts, tables, frames = [], [], []
        for m in mixers:
            cuts = [0, m["total"] // 3 + 1, 2 * m["total"] // 3 + 5, m["total"]]
            lo, hi = cuts[k], cuts[k + 1]
            arr = (_lib.WideSrc * len(m["srcs"]))()
            for e, (x, c, r, g), d in zip(arr, m["srcs"], m["dev"]):
                i0, e.phase, e.frames, e.last = WB.stream_block(len(x) // c, c, r, m["rate"], lo, hi)
                e.data, e.channels, e.from_rate, e.gain = d.data_ptr() + 4 * i0 * c, c, r, g
            dsts.append(torch.full(((hi - lo) * m["ch"],), float("nan"), device="cuda"))
            tables.append(arr)
            frames.append(hi - lo)
        G.wide_mix_batch(dsts, [m["ch"] for m in mixers], [m["rate"] for m in mixers], frames, tables)
        torch.cuda.synchronize()
        for m, d in zip(mixers, dsts):
            m["parts"].append(d.cpu().numpy())
    for b, m in enumerate(mixers):
        got = np.concatenate(m["parts"])
        assert got.shape == m["want"].shape
        assert np.array_equal(_bits(got), _bits(m["want"])), b


def test_three_batched_blocks_of_two_mixers_equal_the_oracle(G):
    """Two mixers of sources of many rates and layouts.  Two mixers a call: nothing here goes through rh_wide_mix_block."""
    _three_blocks_against_the_oracle(G, [(6, 48000, [(6, 44100, 1.0, 2900), (2, 44100, -0.5, 1500), (1, 48000, 2.0, 3100), (3, 11025, 0.0, 600), (6, 96000, 0.25, 5000), (4, 8000, 1.0, 400),
                                                     (2, 22050, -1.5, 1300)]),
                                         (2, 44100, [(2, 48000, 1.0, 2500), (1, 44100, 0.5, 2000), (6, 32000, -1.0, 1200)])], 31)


def test_mixers_of_alike_sources_equal_the_oracle(G):
    """Sources of the mixer's own layout and one rate: while all of them reach a whole block with both taps the tile takes the walk that works
    the tap offset out once per lane (nine and three sources: groups of eight with slots left over); the last block, in which they end, takes
    the general one.  A resampled 5.1 mixer, a stereo one whose sources pass through (F == T), and one of sources of different lengths."""
    _three_blocks_against_the_oracle(G, [(6, 48000, [(6, 44100, g, 2700) for g in (1.0, 0.5, -1.5, 0.0, 2.0, -0.25, 1.0, 0.75, -1.0)]),
                                         (2, 44100, [(2, 44100, g, 2500) for g in (1.0, -0.5, 0.25)]),
                                         (3, 22050, [(3, 48000, 1.0, 5000 + 700 * k) for k in range(5)])], 32)


def test_one_mixer_of_forty_sources_a_call(G):
    """A call of one mixer whose sources do not fit one launch of rh_wide_mix_block, against that entry"""
    rng = np.random.default_rng(33)
    mixers = [(6, 48000, 700, [WB.block_source(rng, 6 if k % 4 else 2, 44100, WB.GAINS[k % 6], 48000, 300, 700, "ended" if k == 17 else "live") for k in range(40)])]
    rows = _upload(mixers)
    tables = _tables(mixers, [[r.data_ptr() for r in rows[0]]])
    want, got = _one_by_one(mixers, tables), _batched(G, mixers, tables)
    assert np.all(np.isfinite(want[0])) and np.array_equal(_bits(got[0]), _bits(want[0]))
    # ... and the first five of them alone: a call that is handed to that entry as it is
    few = [(6, 48000, 700, mixers[0][3][:5])]
    tables = _tables(few, [[r.data_ptr() for r in rows[0][:5]]])
    assert np.array_equal(_bits(_batched(G, few, tables)[0]), _bits(_one_by_one(few, tables)[0]))


def test_more_mixers_than_cus_and_a_ragged_grid(G):
    """300 mixers of 2 sources x 33 frames and one of 3 sources x 70 000 frames in one call; mixer by mixer against the existing entry"""
    import torch

    mixers = WB.ragged_batch()
    assert len(mixers) == 301
    # (one device buffer for all rows: a source's rows start on a 4-byte boundary, whatever lay in front)
    sizes = [s["x"].size for _, _, _, srcs in mixers for s in srcs]
    buf = torch.from_numpy(np.concatenate([s["x"] for _, _, _, srcs in mixers for s in srcs])).cuda()
    offs = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    it = iter(offs)
    ptrs = [[buf.data_ptr() + 4 * int(next(it)) for _ in srcs] for _, _, _, srcs in mixers]
    tables = _tables(mixers, ptrs)
    want = _one_by_one(mixers, tables)
    got = _batched(G, mixers, tables)
    for b, (g, w) in enumerate(zip(got, want)):
        assert np.all(np.isfinite(w)) and np.array_equal(_bits(g), _bits(w)), b


def test_destinations_back_to_back_and_poison_around_every_source(G, mixed):
    """The outputs of the five mixers one behind the other in ONE buffer that starts 4 bytes behind a 16-byte boundary, sentinel guards
    around the whole; every source between zones of poison that begin where the header says reading ends.  Every word of every block is
    written and equals the existing entry's, no guard word changes, no source is written."""
    from rodio_amd import _lib

    mixers = mixed["mixers"]
    ins = [[arena.src_arena(s["x"], lead=(k % 4)) if s["x"].size else None for k, s in enumerate(srcs)] for _, _, _, srcs in mixers]
    sizes = [M * ch for ch, _, M, _ in mixers]
    dst = arena.dst_arena(sum(sizes), lead=1)
    assert dst.ptr() % 16 == 4
    at = np.concatenate([[0], np.cumsum(sizes)])
    B = len(mixers)
    tables = _tables(mixers, [[a.ptr() if a is not None else None for a in aa] for aa in ins])
    flat = (_lib.WideSrc * sum(n for _, n in tables))()
    k = 0
    for arr, n in tables:
        for i in range(n):
            C.memmove(C.byref(flat, k * C.sizeof(_lib.WideSrc)), C.byref(arr[i]), C.sizeof(_lib.WideSrc))
            k += 1
    dsts = (C.c_void_p * B)(*[dst.ptr() + 4 * int(at[b]) for b in range(B)])
    st = _lib.lib.rh_wide_mix_batch(dsts, (C.c_uint32 * B)(*[m[0] for m in mixers]), (C.c_uint32 * B)(*[m[1] for m in mixers]), (C.c_uint64 * B)(*[m[2] for m in mixers]),
                                    (C.c_uint32 * B)(*[n for _, n in tables]), B, flat, _st())
    assert st == 0
    row = dst.check()  # every word written, every guard word intact
    for b in range(B):
        assert np.array_equal(_bits(row[at[b]: at[b + 1]]), _bits(mixed["want"][b])), b
    for aa in ins:
        for a in aa:
            if a is not None:
                a.unchanged()


SENT = np.uint32(arena.SENTINEL)


def test_refusals_write_nothing(G):
    """Every refusal of the header: the status, and both destinations of the call still hold their sentinel (the refused mixer is the first
    of two; the second one is valid)."""
    import torch

    from rodio_amd import _lib

    f = _lib.lib.rh_wide_mix_batch
    rows = torch.zeros(4096, device="cuda")
    sent = torch.from_numpy(np.full(2048, SENT, np.uint32).view(np.int32))

    def attempt(what, want, change=None, null=None):
        d = [sent.clone().cuda(), sent.clone().cuda()]
        a = dict(dsts=(C.c_void_p * 2)(d[0].data_ptr(), d[1].data_ptr()), ch=(C.c_uint32 * 2)(2, 6), rates=(C.c_uint32 * 2)(48000, 48000), frames=(C.c_uint64 * 2)(100, 64),
                 counts=(C.c_uint32 * 2)(2, 1), srcs=(_lib.WideSrc * 3)())
        for e, (ch, rate, phase, frames, last) in zip(a["srcs"], [(2, 44100, 0, 100, WB.NONE), (1, 48000, 0, 50, 49), (6, 44100, 3, 64, WB.NONE)]):
            e.data, e.channels, e.from_rate, e.phase, e.frames, e.last, e.gain = rows.data_ptr(), ch, rate, phase, frames, last, 1.0
        if change:
            change(a)
        if null:
            a[null] = None
        st = f(a["dsts"], a["ch"], a["rates"], a["frames"], a["counts"], 2, a["srcs"], _st())
        torch.cuda.synchronize()
        assert st == want, (what, st)
        if want:
            for t in d:
                assert np.all(t.cpu().numpy().view(np.uint32) == SENT), (what, "a refused call wrote")
        return d

    ok = attempt("the batch itself", 0)
    assert all(np.all(t.cpu().numpy().view(np.uint32)[:n] != SENT) for t, n in zip(ok, (200, 384)))
    assert f(None, None, None, None, None, 0, None, _st()) == 0  # n_mixers == 0: nothing to do
    for name in ("dsts", "ch", "rates", "frames", "counts", "srcs"):
        attempt(f"{name} == NULL", INVALID, null=name)

    def setter(key, i, value):
        def change(a):
            a[key][i] = value
        return change

    def src_setter(i, field, value):
        def change(a):
            setattr(a["srcs"][i], field, value)
        return change

    attempt("a NULL dst with out_frames > 0", INVALID, setter("dsts", 0, None))
    attempt("channels of 0", INVALID, setter("ch", 0, 0))
    attempt("to_rate of 0", INVALID, setter("rates", 0, 0))
    attempt("a source without data", INVALID, src_setter(0, "data", None))
    attempt("a source of 0 channels", INVALID, src_setter(1, "channels", 0))
    attempt("a source of rate 0", INVALID, src_setter(0, "from_rate", 0))
    attempt("a source that reaches more frames than the block has", INVALID, src_setter(1, "frames", 101))
    attempt("a phase that is no remainder mod T", INVALID, src_setter(0, "phase", 160))
    attempt("F * T beyond 32 bits", UNSUPPORTED, src_setter(0, "from_rate", 4294967291))
    attempt("out_frames beyond 2^31 - 1", UNSUPPORTED, setter("frames", 0, 0x80000000))
    # ... and what is no refusal: a mixer with out_frames == 0 is skipped, whatever else it says
    def skipped(a):
        a["frames"][0], a["dsts"][0], a["ch"][0], a["rates"][0] = 0, None, 0, 0
        a["srcs"][0].data, a["srcs"][0].channels = None, 0
    d = attempt("a mixer with out_frames == 0", 0, skipped)
    assert np.all(d[0].cpu().numpy().view(np.uint32) == SENT) and np.all(d[1].cpu().numpy().view(np.uint32)[:384] != SENT)


def test_a_block_too_long_for_32_bit_positions_is_refused(G):
    """from_rate 65521 into 48000 (F = 65521, T = 48000: no common factor), 70 000 mono frames: fit = (2^32 - 1 - 48000) / 65521 = 65 550 is
    below 70 000, so phase + j F would leave 32 bits inside the block.  rh_wide_mix_block cuts such a block into launches; the batch refuses
    it.  Every buffer is allocated in full (0.38 MB of source, 0.28 MB of destination): an implementation that ran it would write."""
    import torch

    from rodio_amd import _lib

    F, T, M = 65521, 48000, 70000
    assert (2**32 - 1 - T) // F == 65550 < M
    n = (M - 1) * F // T + 2
    src = torch.from_numpy(WB.signal(np.random.default_rng(3), n)).cuda()
    dst = torch.from_numpy(np.full(M, SENT, np.uint32).view(np.int32)).cuda()
    other = torch.from_numpy(np.full(64, SENT, np.uint32).view(np.int32)).cuda()
    srcs = (_lib.WideSrc * 2)()
    for e, (frames, rate) in zip(srcs, [(M, F), (64, 44100)]):
        e.data, e.channels, e.from_rate, e.phase, e.frames, e.last, e.gain = src.data_ptr(), 1, rate, 0, frames, WB.NONE, 1.0
    st = _lib.lib.rh_wide_mix_batch((C.c_void_p * 2)(dst.data_ptr(), other.data_ptr()), (C.c_uint32 * 2)(1, 1), (C.c_uint32 * 2)(T, T), (C.c_uint64 * 2)(M, 64), (C.c_uint32 * 2)(1, 1), 2,
                                    srcs, _st())
    torch.cuda.synchronize()
    assert st == UNSUPPORTED
    assert np.all(dst.cpu().numpy().view(np.uint32) == SENT) and np.all(other.cpu().numpy().view(np.uint32) == SENT)
    # a block of exactly `fit` frames is taken, and is the existing entry's block
    ok = 65550
    srcs[0].frames = ok
    st = _lib.lib.rh_wide_mix_batch((C.c_void_p * 2)(dst.data_ptr(), other.data_ptr()), (C.c_uint32 * 2)(1, 1), (C.c_uint32 * 2)(T, T), (C.c_uint64 * 2)(ok, 64), (C.c_uint32 * 2)(1, 1), 2,
                                    srcs, _st())
    assert st == 0
    ref = torch.empty(ok, device="cuda")
    _lib.check(_lib.lib.rh_wide_mix_block(vp(ref.data_ptr()), 1, T, ok, srcs, 1, _st()), "rh_wide_mix_block")
    torch.cuda.synchronize()
    assert np.array_equal(dst.cpu().numpy().view(np.uint32)[:ok], _bits(ref.cpu().numpy()))
    assert np.all(dst.cpu().numpy().view(np.uint32)[ok:] == SENT)


# ---- stream order: the case of tests/test_gpu_stream_order.py for this entry ---------------------------------------------------------------
GATE_MS = 21.0  # test_gpu_stream_order.py: GATE_FACTOR (70) times SLOWEST_HOST_MS (0.3 ms), for the one call queued behind the gate


@pytest.fixture(scope="module")
def delay(G):
    return stream_gate.Delay()


def test_the_batch_behind_a_gate_on_a_side_stream(G, delay, mixed):
    """The five mixers queued on a backed-up side stream while the gate is pending; all five host arrays and srcs_host are overwritten as soon
    as the call returns; the outputs are copied to snapshots and spoiled on the same stream.  The warmed call returns while the gate is
    still pending, and the snapshots hold the existing entry's blocks."""
    import torch

    from rodio_amd import _lib

    mixers = mixed["mixers"]
    B = len(mixers)

    def build(k):
        ins = [[k.src(s["x"]) if s["x"].size else None for s in srcs] for _, _, _, srcs in mixers]
        outs = [k.dst(M * ch) for ch, _, M, _ in mixers]
        total = sum(len(srcs) for _, _, _, srcs in mixers)

        def call():
            flat = k.host((_lib.WideSrc * total)(), 0)  # zeros: sources of no frames
            at = 0
            for (_, _, _, srcs), aa in zip(mixers, ins):
                at = WB.fill_table(flat, at, srcs, [a.ptr() if a is not None else None for a in aa])
            dsts = k.host((C.c_void_p * B)(*[o.ptr() for o in outs]), k.pit())
            ch = k.host((C.c_uint32 * B)(*[m[0] for m in mixers]), 1)
            rates = k.host((C.c_uint32 * B)(*[m[1] for m in mixers]), 1)
            frames = k.host((C.c_uint64 * B)(*[m[2] for m in mixers]), 0)
            counts = k.host((C.c_uint32 * B)(*[len(m[3]) for m in mixers]), 0)
            _lib.check(_lib.lib.rh_wide_mix_batch(dsts, ch, rates, frames, counts, B, flat, _st()), "rh_wide_mix_batch")

        def check():
            for b, o in enumerate(outs):
                assert arena.same(o.check_snapshot(), mixed["want"][b]), b
            for aa in ins:
                for a in aa:
                    if a is not None:
                        a.snapshot_unchanged()

        return stream_gate.case([call], check)

    r = stream_gate.run(build, torch.cuda.Stream(), delay, GATE_MS)
    print(f"[wide_mix_batch behind a gate] gate {r.reps} x {delay.fill_ms:.3f} ms, pending {r.pending} queued {int(r.queued)}, host ms {max(r.host_ms):.3f}")
    assert all(r.pending), ("rh_wide_mix_batch returned after the gate had opened: the call waited for the stream, or the gate is too short", r.host_ms)
    r.check()
