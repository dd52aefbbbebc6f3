"""The fused path (rh_rlm_*) in a hostile memory layout (tests/arena.py): every source in a poison arena of its own on a 16-byte boundary, as
the header requires, exactly in_frames long; dst exactly *out_frames frames between sentinel guards.  The tile loaders read whole vectors and
LDS-DMA tiles around a row by design: nothing of that may reach the mix, and the last (partial) tile may store nothing behind the row.
References and tolerances are those of test_gpu_mix_first.py and the block-streaming tests; every run is also held, bit for bit, against the
same call on plain rows (zeros around the sources, a fresh zeroed dst).  Through the C ABI."""
import ctypes as C

import numpy as np
import pytest
from conftest import knobs

import arena
from test_gpu_mix_first import TOL  # 1e-5: the filtered fused path against the oracle's per-sample chain
from test_gpu_mix_first import _oracle_run, rnd

pytestmark = pytest.mark.gpu
STREAM_TOL = 1e-6  # a stream's concatenated blocks against one rh_rlm_run over the whole stream (rodio_hip.h; test_gpu_parity.py's block-streaming tests)
same = arena.same


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _st():
    from rodio_amd import source

    return source._stream()


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def close(got, ref, tol):
    """max |got - ref| <= tol, written so that a NaN fails it"""
    got, ref = np.asarray(got, np.float32).reshape(-1), np.asarray(ref, np.float32).reshape(-1)
    assert got.shape == ref.shape, (got.shape, ref.shape)
    err = float(np.max(np.abs(got.astype(np.float64) - ref.astype(np.float64)))) if got.size else 0.0
    return err <= tol, err


def _reference(O, xs, frm, to, ch, span, filt, freq, gains):
    """The oracle's Mixer over UniformSourceIterator(src.amplify(g)) [.low_pass / .high_pass]"""
    if filt is not None:
        return _oracle_run(O, xs, frm, to, span, filt, freq, gains, ch)
    m = O.Mixer(ch, to)
    for i, x in enumerate(xs):
        src = O.TestSource(x, ch, frm) if not span else O.SpanSource(x, ch, frm, span)
        if gains is not None:
            src = src.amplify(float(gains[i]))
        m.add(O.UniformSourceIterator(src, ch, to))
    return m.collect()


def _meets(got, ref, filt):
    """no filter: the bit-exact ordered sum; a filter: the 1e-5 of the filtered path"""
    if filt is None:
        assert same(got, ref), int(np.argmax(arena.bits(got) != arena.bits(ref))) if len(got) == len(ref) else (len(got), len(ref))
    else:
        ok, err = close(got, ref, TOL)
        assert ok, err


def _out_frames(lens, frm, to, ch, span):
    from rodio_amd import _lib

    mx = 0
    for n in lens:
        o = C.c_uint64(0)
        _lib.check(_lib.lib.rh_resample_out_frames(n, frm, to, ch, span or 0, C.byref(o)), "rh_resample_out_frames")
        mx = max(mx, o.value)
    return mx


def _set_sources(p, ptrs, lens):
    from rodio_amd import _lib

    n = len(ptrs)
    _lib.check(_lib.lib.rh_rlm_set_sources(p._h, (C.c_void_p * n)(*ptrs), (C.c_uint64 * n)(*lens), n), "rh_rlm_set_sources")


def _run(p, dst_ptr, cap, subset=None):
    from rodio_amd import _lib

    m = C.c_uint64(0)
    if subset is None:
        _lib.check(_lib.lib.rh_rlm_run(p._h, C.c_void_p(dst_ptr), cap, C.byref(m), _st()), "rh_rlm_run")
    else:
        _lib.check(_lib.lib.rh_rlm_run_subset(p._h, subset[0], subset[1], C.c_void_p(dst_ptr), cap, C.byref(m), _st()), "rh_rlm_run_subset")
    return m.value


def _both(G, xs, make, ch, out_frames, subset=None):
    """One run with the sources in poison arenas and dst in a sentinel arena of exactly out_frames frames, one on plain rows: the checked
    row of the first (which has the bits of the second) and the handle's geometry."""
    lens = [len(x) // ch for x in xs]
    ins = [arena.src_arena(x) for x in xs]
    dst = arena.dst_arena(out_frames * ch)
    p = make()
    _set_sources(p, [a.ptr() for a in ins], lens)
    geo = p.geometry()
    assert _run(p, dst.ptr(), out_frames, subset) == out_frames
    p.check_status()
    row = dst.check()
    for a in ins:
        a.unchanged()
    p.close()
    plains = [arena.plain(x) for x in xs]
    pd, pdp = arena.plain_dst(out_frames * ch)
    p = make()
    _set_sources(p, [q for _, q in plains], lens)
    assert _run(p, pdp, out_frames, subset) == out_frames
    p.check_status()
    plain_row = host(pd)[: out_frames * ch]
    differ = np.flatnonzero(arena.bits(plain_row) != arena.bits(row))
    assert differ.size == 0, f"poison around the sources changed the bits of the mix: {differ.size} of {row.size} samples, the first at {int(differ[0])}, {int(np.isnan(row).sum())} NaN"
    p.close()
    return row, geo


FILTERS = [("low_pass", 200), ("high_pass", 300), (None, 0)]


# ---- one-shot runs --------------------------------------------------------------------------------------------------------------------
EQUAL, RAGGED = [4099] * 3, [4099, 2500, 3001]
GAINS3 = np.array([1.0, 0.5, -0.75], dtype=np.float32)
# (from_rate, to_rate, span_len, force_general, in_frames, gains)
ONE_SHOT = [(44100, 48000, span, fg, lens, None) for span in (0, 4096) for fg in (0, 1) for lens in (EQUAL, RAGGED)]
ONE_SHOT += [(48000, 48000, 0, 0, EQUAL, None), (44100, 48000, 0, 0, EQUAL, GAINS3), (44100, 48000, 0, 0, RAGGED, GAINS3)]


@pytest.mark.parametrize("cfg", range(len(ONE_SHOT)), ids=[f"{c[0]}to{c[1]}-span{c[2]}-general{c[3]}-{'equal' if c[4] is EQUAL else 'ragged'}{'-gains' if c[5] is not None else ''}" for c in ONE_SHOT])
@pytest.mark.parametrize("filt,freq", FILTERS, ids=["low_pass", "high_pass", "no_filter"])
@pytest.mark.parametrize("ch", [2, 1])
def test_one_shot_runs(G, O, ch, filt, freq, cfg):
    """frames_per_lane = 4 (tiles of 256 output frames: the last tile is partial), 3 sources of 4099 frames and of [4099, 2500, 3001]; the
    equal-length and the ragged-batch kernel; spans of 4096 samples; 48 -> 48 kHz; gains.

    A row of 4099 frames ends inside a 16-byte vector (2 stereo / 4 mono frames), and the last output frame is the source's last frame
    verbatim (sample_rate.rs:193-200), formed as a + (b - a) * 0 / T: with the frame BEHIND the row as b (k_rlm_fast until this test) the
    last frame of the mix was NaN between poison -- 2 of 8924 samples stereo, 1 of 4462 mono -- and right between zeros."""
    frm, to, span, fg, lens, gains = ONE_SHOT[cfg]
    xs = [rnd(6100 + s, n * ch, 0.3) for s, n in enumerate(lens)]

    def make():
        p = G.ResampleLowpassMix(frm, to, ch, span, filt, freq, 0.5, max_sources=3, max_in_frames=max(lens), frames_per_lane=4, force_general=fg)
        if gains is not None:
            p.set_gains(gains)
        return p

    M = _out_frames(lens, frm, to, ch, span)
    row, geo = _both(G, xs, make, ch, M)
    if filt is not None and lens is RAGGED and not fg:
        assert geo["ragged_pair"] == 1, geo
    ref = _reference(O, xs, frm, to, ch, span, filt, freq, gains)
    assert len(ref) == M * ch, (len(ref), M)
    _meets(row, ref, filt)


@pytest.mark.parametrize("filt,freq", FILTERS, ids=["low_pass", "high_pass", "no_filter"])
@pytest.mark.parametrize("ch", [2, 1])
def test_run_subset_and_run_batch(G, O, ch, filt, freq):
    from rodio_amd import _lib

    frm, to, lens = 44100, 48000, [4099, 2500, 3001]
    xs = [rnd(6200 + s, n * ch, 0.3) for s, n in enumerate(lens)]

    def make():
        return G.ResampleLowpassMix(frm, to, ch, None, filt, freq, 0.5, max_sources=3, max_in_frames=max(lens), frames_per_lane=4)

    # rh_rlm_run_subset(1, 1): one converted, filtered stream in a dst of the BATCH's length (rodio_hip.h): silence behind the source's end
    M, M1 = _out_frames(lens, frm, to, ch, 0), _out_frames(lens[1:2], frm, to, ch, 0)
    row, _ = _both(G, xs, make, ch, M, subset=(1, 1))
    _meets(row[: M1 * ch], _reference(O, xs[1:2], frm, to, ch, None, filt, freq, None), filt)
    assert M1 < M and not np.any(row[M1 * ch:]), "frames behind the subset's last source are not silent"
    # rh_rlm_run_batch: rows out_frames rounded up to even plus 2 frames apart: the gaps stay sentinel
    n = 4099
    xs = [rnd(6300 + s, n * ch, 0.3) for s in range(3)]
    M = _out_frames([n], frm, to, ch, 0)
    stride = (M + 1) // 2 * 2 + 2
    ins = [arena.src_arena(x) for x in xs]
    dst = arena.dst_arena_rows(3, M * ch, stride * ch)
    p = make()
    _set_sources(p, [a.ptr() for a in ins], [n] * 3)
    m = C.c_uint64(0)
    if ch != 2:  # stereo batches only (rodio_hip.h): refused, nothing written
        assert _lib.lib.rh_rlm_run_batch(p._h, C.c_void_p(dst.ptr()), stride, C.byref(m), _st()) == 3  # RH_ERR_UNSUPPORTED
        dst.check(written=0)
        p.close()
        return
    assert _lib.lib.rh_rlm_run_batch(p._h, C.c_void_p(dst.ptr()), stride - 1, C.byref(m), _st()) == 1  # an odd stride: RH_ERR_INVALID
    dst.check(written=0)
    _lib.check(_lib.lib.rh_rlm_run_batch(p._h, C.c_void_p(dst.ptr()), stride, C.byref(m), _st()), "rh_rlm_run_batch")
    assert m.value == M
    p.check_status()
    rows = dst.check()
    p.close()
    for s in range(3):
        _meets(rows[s], _reference(O, xs[s: s + 1], frm, to, ch, None, filt, freq, None), filt)
    plains = [arena.plain(x) for x in xs]
    pd, pdp = arena.plain_dst(3 * stride * ch)
    p = make()
    _set_sources(p, [q for _, q in plains], [n] * 3)
    _lib.check(_lib.lib.rh_rlm_run_batch(p._h, C.c_void_p(pdp), stride, C.byref(m), _st()), "rh_rlm_run_batch")
    p.check_status()
    assert same(host(pd)[: 3 * stride * ch].reshape(3, -1)[:, : M * ch], rows)
    p.close()


# ---- mix first ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("filt,freq", FILTERS[:2], ids=["low_pass", "high_pass"])
def test_mix_first_two_launches(G, O, filt, freq):
    """16 equal sources of 4096 stereo frames: summed at the input rate by k_mix_rows, then the fused kernel on the one row."""
    S, n, ch = 16, 4096, 2
    xs = [rnd(6400 + s, n * ch, 0.05) for s in range(S)]
    gains = np.linspace(0.4, 1.2, S).astype(np.float32)

    def make():
        p = G.ResampleLowpassMix(44100, 48000, ch, None, filt, freq, 0.5, max_sources=S, max_in_frames=n)
        p.set_gains(gains)
        return p

    M = _out_frames([n], 44100, 48000, ch, 0)
    row, geo = _both(G, xs, make, ch, M)
    assert geo["mix_first"] == 1, geo
    _meets(row, _reference(O, xs, 44100, 48000, ch, None, filt, freq, gains), filt)


@pytest.mark.parametrize("span", [None, 3000])
def test_mix_first_chunk_kernel(G, O, span):
    """k_rlm_chunk takes stereo rows from 2 x 256 chunks of 1024 frames on: 3 sources of 524 288 frames (test_chunk_kernel_equals_rodio_chain)."""
    S, n, ch = 3, 524288, 2
    xs = [rnd(6500 + s, n * ch, 0.3) for s in range(S)]
    gains = np.array([1.0, 0.5, -0.75], dtype=np.float32)

    def make():
        p = G.ResampleLowpassMix(44100, 48000, ch, span, "low_pass", 200, 0.5, max_sources=S, max_in_frames=n)
        p.set_gains(gains)
        return p

    M = _out_frames([n], 44100, 48000, ch, span)
    row, geo = _both(G, xs, make, ch, M)
    assert geo["mix_first"] == 2, geo
    _meets(row, _reference(O, xs, 44100, 48000, ch, span, "low_pass", 200, gains), "low_pass")


def test_mix_first_filter_classes_in_one_launch(G, O):
    """Two filter classes of two sources each, rows long enough for k_rlm_chunk: one launch walks the classes (geometry().mix_first == 3,
    test_filter_classes_walked_in_one_launch)."""
    S, n, ch = 4, 524288, 2
    filters = [("low_pass", 200), ("high_pass", 300), ("high_pass", 300), ("low_pass", 200)]
    xs = [rnd(7300 + s, n * ch, 0.1) for s in range(S)]
    gains = np.linspace(0.5, 1.2, S).astype(np.float32)
    how = []

    def make():
        p = G.ResampleLowpassMix(44100, 48000, ch, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=n)
        p.set_filters(filters)
        p.set_gains(gains)
        how.append(p)
        return p

    M = _out_frames([n], 44100, 48000, ch, 0)
    ins = [arena.src_arena(x) for x in xs]
    dst = arena.dst_arena(M * ch)
    p = make()
    _set_sources(p, [a.ptr() for a in ins], [n] * S)
    assert _run(p, dst.ptr(), M) == M
    p.check_status()
    assert p.geometry()["mix_first"] == 3, p.geometry()
    row = dst.check()
    for a in ins:
        a.unchanged()
    p.close()
    plains = [arena.plain(x) for x in xs]
    pd, pdp = arena.plain_dst(M * ch)
    p = make()
    _set_sources(p, [q for _, q in plains], [n] * S)
    assert _run(p, pdp, M) == M
    p.check_status()
    assert same(host(pd)[: M * ch], row)
    p.close()
    m = O.Mixer(ch, 48000)
    for x, f, g in zip(xs, filters, gains):
        u = O.UniformSourceIterator(O.TestSource(x, ch, 44100).amplify(float(g)), ch, 48000)
        m.add(u.low_pass(f[1]) if f[0] == "low_pass" else u.high_pass(f[1]))
    _meets(row, m.collect(), "classes")


# ---- streams --------------------------------------------------------------------------------------------------------------------------
def _mirror_capacity(avail, frm, to):
    """what ResampleLowpassMix.stream_feed gives a block's dst (rodio_amd/source.py)"""
    return int(avail * (to / frm + 1)) + 64


def _stream_equal(G, xs, ch, frm, to, filt, freq, blocks, use_arena):
    """rh_rlm_stream_block: every source passes the frames it kept plus the block's new ones, exactly that many inside poison; the last
    block flushes.  Only *out_frames frames of dst may be touched."""
    from rodio_amd import _lib

    lib, S = _lib.lib, len(xs)
    p = G.ResampleLowpassMix(frm, to, ch, None, filt, freq, 0.5, max_sources=S, max_in_frames=max(blocks) + 4096)
    p.stream_begin()
    parts, g0, fed = [], 0, 0
    for k, b in enumerate(blocks):
        fed += b
        flush = int(k == len(blocks) - 1)
        rows = [x[g0 * ch: fed * ch] for x in xs]
        avail = fed - g0
        cap = _mirror_capacity(avail, frm, to)
        if use_arena:
            ins, dst = [arena.src_arena(r) for r in rows], arena.dst_arena(cap * ch)
            ptrs, dp = [a.ptr() for a in ins], dst.ptr()
        else:
            ins, (dt, dp) = [arena.plain(r if r.size else np.zeros(4, np.float32)) for r in rows], arena.plain_dst(cap * ch)
            ptrs = [q for _, q in ins]
        o, c = C.c_uint64(0), C.c_uint64(0)
        _lib.check(lib.rh_rlm_stream_block(p._h, (C.c_void_p * S)(*ptrs), S, avail, flush, C.c_void_p(dp), cap, C.byref(o), C.byref(c), _st()), "rh_rlm_stream_block")
        p.check_status()
        assert o.value <= cap and c.value <= avail
        if use_arena:
            parts.append(dst.check(written=o.value * ch)[: o.value * ch])
            for a in ins:
                a.unchanged()
        else:
            parts.append(host(dt)[: o.value * ch])
        g0 += c.value
    p.close()
    return np.concatenate(parts)


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("filt,freq", FILTERS, ids=["low_pass", "high_pass", "no_filter"])
def test_stream_block(G, O, ch, filt, freq):
    frm, to, S = 44100, 48000, 3
    blocks = [1000, 1024, 1000, 1024, 51]
    n = sum(blocks)
    xs = [rnd(6700 + s, n * ch, 0.3) for s in range(S)]
    got = _stream_equal(G, xs, ch, frm, to, filt, freq, blocks, True)
    ref = _reference(O, xs, frm, to, ch, None, filt, freq, None)
    _meets(got, ref, filt)
    assert same(_stream_equal(G, xs, ch, frm, to, filt, freq, blocks, False), got)
    # ... and one rh_rlm_run over the whole stream
    import torch

    p = G.ResampleLowpassMix(frm, to, ch, None, filt, freq, 0.5, max_sources=S, max_in_frames=n)
    p.set_sources([torch.from_numpy(x).cuda() for x in xs])
    ok, err = close(got, host(p.run()), STREAM_TOL)
    p.close()
    assert ok, err


def _stream_v(G, xs, ch, frm, to, filt, freq, his, use_arena, keep_history=False, overlap=False, gains=None):
    """rh_rlm_stream_block_v: block k passes, per source, the frames it kept and the new ones up to input frame his[k] (or to the source's
    end, which it then reports).  -> the output and rh_rlm_stream_one_launch_blocks"""
    from rodio_amd import _lib

    lib, S = _lib.lib, len(xs)
    ns = [len(x) // ch for x in xs]
    p = G.ResampleLowpassMix(frm, to, ch, None, filt, freq, 0.5, max_sources=S, max_in_frames=max(his) + 4096)
    if gains is not None:
        p.set_gains(gains)
    p.stream_begin(keep_history=keep_history)
    _lib.check(lib.rh_rlm_stream_overlap(p._h, 1 if overlap else 0), "rh_rlm_stream_overlap")
    parts, g0, prev, cur = [], 0, None, None
    for hi in his:
        rows = [x[min(g0, n) * ch: min(hi, n) * ch] for x, n in zip(xs, ns)]
        avail = [len(r) // ch for r in rows]
        cap = _mirror_capacity(max(avail), frm, to)
        if use_arena:
            ins, dst = [arena.src_arena(r) for r in rows], arena.dst_arena(cap * ch)
            ptrs, dp = [a.ptr() for a in ins], dst.ptr()
        else:
            ins, (dt, dp) = [arena.plain(r if r.size else np.zeros(4, np.float32)) for r in rows], arena.plain_dst(cap * ch)
            ptrs = [q for _, q in ins]
        prev, cur = cur, ins  # (keep_history: the rows of a block stay valid until the next block's work has run)
        o, c = C.c_uint64(0), C.c_uint64(0)
        _lib.check(lib.rh_rlm_stream_block_v(p._h, (C.c_void_p * S)(*ptrs), (C.c_uint64 * S)(*avail), (C.c_uint8 * S)(*[1 if hi >= n else 0 for n in ns]), S, C.c_void_p(dp), cap,
                                             C.byref(o), C.byref(c), _st()), "rh_rlm_stream_block_v")
        p.check_status()
        assert o.value <= cap
        if use_arena:
            parts.append(dst.check(written=o.value * ch)[: o.value * ch])
            for a in ins:
                a.unchanged()
        else:
            parts.append(host(dt)[: o.value * ch])
        g0 += c.value
    one = C.c_uint32(0)
    _lib.check(lib.rh_rlm_stream_one_launch_blocks(p._h, C.byref(one)), "rh_rlm_stream_one_launch_blocks")
    p.close()
    return np.concatenate(parts), one.value


@pytest.mark.parametrize("ch", [2, 1])
@pytest.mark.parametrize("filt,freq", FILTERS, ids=["low_pass", "high_pass", "no_filter"])
def test_stream_block_v_ragged_sources(G, O, ch, filt, freq):
    """The three ragged sources end in different blocks."""
    frm, to, lens = 44100, 48000, [4099, 2500, 3001]
    xs = [rnd(6800 + s, n * ch, 0.3) for s, n in enumerate(lens)]
    his = [1000, 2024, 3024, 4048, 4099]
    got, _ = _stream_v(G, xs, ch, frm, to, filt, freq, his, True)
    _meets(got, _reference(O, xs, frm, to, ch, None, filt, freq, None), filt)
    plain, _ = _stream_v(G, xs, ch, frm, to, filt, freq, his, False)
    assert same(plain, got)


@pytest.mark.parametrize("overlap", [False, True])
def test_stream_block_on_the_summed_state_in_one_launch(G, O, overlap):
    """k_rlm_sblk's smallest block (test_gpu_sblk.py: the instance with 1 KiB windows, 2 stereo sources, a stream of one block of one tile,
    104 frames): rh_rlm_stream_one_launch_blocks counts it."""
    ch, frm, to, n = 2, 48000, 44100, 104
    gains = np.array([1.3, -0.45], dtype=np.float32)
    xs = [rnd(104000 + s, n * ch, 0.98 / 1.75) for s in range(2)]
    with knobs(RH_SBLK_KV="1"):
        got, one = _stream_v(G, xs, ch, frm, to, "low_pass", 200, [n], True, keep_history=True, overlap=overlap, gains=gains)
        plain, one_p = _stream_v(G, xs, ch, frm, to, "low_pass", 200, [n], False, keep_history=True, overlap=overlap, gains=gains)
    assert one == 1 and one_p == 1, (one, one_p)
    _meets(got, _reference(O, xs, frm, to, ch, None, "low_pass", 200, gains), "low_pass")
    assert same(plain, got)
