"""Sources set as 16-bit PCM (rh_rlm_set_sources_pcm16): the fused mixer reads the samples as they lie in a WAV data chunk.  dasp's i16 -> f32 is
`s as f32 / 32768.0`, exact, so every run on PCM16 rows must give the BITS of the same handle configuration on the f32 twins of the rows
(rh_rlm_set_sources) -- whether the kernels read the int16 rows themselves (k_rlm_chunk_pcm16, k_mix_rows_pcm16: source_format()["native"] == 1)
or a converted copy (every other route).  Each run is repeated once on the same handle and must repeat its bits."""
import functools
import os

import numpy as np
import pytest
from conftest import knobs

pytestmark = pytest.mark.gpu
TOL = 1e-5
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GAINS3 = np.array([1.0, 0.5, -0.75], dtype=np.float32)
GAINS9 = np.array([1.0, 0.5, 1.7, 0.0, -0.25, 0.9, 1.0, 0.3, 1.1], dtype=np.float32)


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available()
    rh.init(0)
    return rh


def rnd(seed, n, scale=1.0):
    return (np.random.default_rng(seed).uniform(-1, 1, n) * scale).astype(np.float32)


@functools.lru_cache(maxsize=None)
def pcm(seed, n, scale):
    s = np.round(rnd(seed, n, scale) * 32767).astype(np.int16)
    s.setflags(write=False)
    return s


def twin(s):
    return s.astype(np.float32) / np.float32(32768)


def test_the_twin_is_the_reference_conversion(O):
    s = np.concatenate([pcm(1, 5000, 1.0), np.array([-32768, 32767, 0, -1, 1], dtype=np.int16)])
    assert np.array_equal(twin(s), O.convert("i16_to_f32", s))


def _oracle_run(O, xs, frm, to, span, filt, freq, gains, ch):
    m = O.Mixer(ch, to)
    for i, x in enumerate(xs):
        src = O.TestSource(x, ch, frm) if not span else O.SpanSource(x, ch, frm, span)
        if gains is not None:
            src = src.amplify(float(gains[i]))
        u = O.UniformSourceIterator(src, ch, to)
        m.add(u.low_pass(freq) if filt == "low_pass" else u.high_pass(freq))
    return m.collect()


def _dev_rows(rows, byte_off=0):
    """Every int16 row in an allocation of its own; byte_off: as a view that starts that many bytes behind the allocation's boundary."""
    import torch

    out = []
    for r in rows:
        t = torch.zeros(len(r) + byte_off // 2 + 64, dtype=torch.int16, device="cuda")
        v = t[byte_off // 2: byte_off // 2 + len(r)]
        v.copy_(torch.from_numpy(np.array(r)))  # (a copy: the cached rows are read-only)
        out.append(v)
    return out


def _handle(G, rows, ch, frm=44100, to=48000, span=None, filt="low_pass", freq=200, gains=None, filters=None, **kw):
    S = len(rows)
    p = G.ResampleLowpassMix(frm, to, ch, span, filt, freq, 0.5, max_sources=S, max_in_frames=max(len(r) for r in rows) // ch, **kw)
    if filters is not None:
        p.set_filters(filters)
    if gains is not None:
        p.set_gains(gains)
    return p


def _twice(p, run):
    got = run(p).cpu().numpy().copy()
    again = run(p).cpu().numpy()
    p.check_status()
    assert np.array_equal(got, again)
    return got


def _both(G, rows, ch, run=lambda p: p.run(), dev=None, **cfg):
    """The same handle configuration on the PCM16 rows and on their f32 twins: (PCM16 result, f32 result, geometry, source_format of the PCM16 run)."""
    import torch

    p = _handle(G, rows, ch, **cfg)
    p.set_sources(dev if dev is not None else _dev_rows(rows))
    assert p.source_format() == {"format": 1, "native": 0}  # (nothing has run)
    geo = p.geometry()
    got = _twice(p, run)
    fmt = p.source_format()
    p.close()
    q = _handle(G, rows, ch, **cfg)
    q.set_sources([torch.from_numpy(twin(r)).cuda() for r in rows])
    assert q.geometry() == geo
    want = _twice(q, run)
    assert q.source_format() == {"format": 0, "native": 0}
    q.close()
    assert got.shape == want.shape
    return got, want, geo, fmt


def _same_bits(got, want):
    assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (int(np.argmax(got != want)), float(np.max(np.abs(got - want))))


# ---- 1. k_rlm_chunk_pcm16, stereo -------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frm,to,span", [(44100, 48000, None), (44100, 48000, 32768), (48000, 44100, None), (48000, 48000, None)])
@pytest.mark.parametrize("filt,freq", [("low_pass", 200), ("high_pass", 300)])
def test_chunk_stereo(G, O, frm, to, span, filt, freq):
    S, n, ch = 3, 600000, 2
    rows = [pcm(6500 + s, n * ch, 0.3) for s in range(S)]
    got, want, geo, fmt = _both(G, rows, ch, frm=frm, to=to, span=span, filt=filt, freq=freq, gains=GAINS3)
    assert geo["mix_first"] == 2, geo
    assert fmt == {"format": 1, "native": 1}
    _same_bits(got, want)
    # the f32 path's own bound on this distribution (test_chunk_kernel_equals_rodio_chain): it follows from the bits, and catches a twin built wrongly
    ref = _oracle_run(O, [twin(r) for r in rows], frm, to, span, filt, freq, GAINS3, ch)
    assert len(got) == len(ref)
    err = np.abs(got - ref)
    assert float(np.max(err)) <= TOL, (int(np.argmax(err)), float(np.max(err)))


# ---- 2. the instance with chunks of 512 frames ------------------------------------------------------------------------------------------
def test_chunk_512_frame_instance(G):
    S, n, ch = 3, 600000, 2
    rows = [pcm(6500 + s, n * ch, 0.3) for s in range(S)]
    got, want, geo, fmt = _both(G, rows, ch, frm=22050, to=48000, gains=GAINS3)
    assert geo["mix_first"] == 2, geo
    assert fmt == {"format": 1, "native": 1}
    _same_bits(got, want)


# ---- 3. mono ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("span", [None, 32768])
def test_chunk_mono(G, span):
    S, n, ch = 3, 600000, 1
    rows = [pcm(6700 + s, n * ch, 0.3) for s in range(S)]
    got, want, geo, fmt = _both(G, rows, ch, span=span, gains=GAINS3)
    assert geo["mix_first"] == 2, geo
    assert fmt == {"format": 1, "native": 1}
    _same_bits(got, want)


# ---- 4. more tiles than slots: tiles by ticket ------------------------------------------------------------------------------------------
def test_chunk_more_tiles_than_slots(G):
    S, n, ch = 2, 2_600_000, 2
    rows = [pcm(7000 + s, n * ch, 0.3) for s in range(S)]
    got, want, geo, fmt = _both(G, rows, ch)
    assert geo["mix_first"] == 2, geo
    assert fmt == {"format": 1, "native": 1}
    _same_bits(got, want)


# ---- 5. rows the chunk kernel must refuse -----------------------------------------------------------------------------------------------
def test_chunk_refuses_rows_that_are_no_whole_pcm16_vectors(G):
    S, n, ch = 3, 600002, 2  # whole 16-byte vectors of f32 (k_rlm_chunk takes them), 4 samples over whole vectors of int16
    rows = [pcm(6800 + s, n * ch, 0.3) for s in range(S)]
    got, want, geo, fmt = _both(G, rows, ch, gains=GAINS3)
    assert geo["mix_first"] == 2, geo
    assert fmt == {"format": 1, "native": 0}
    _same_bits(got, want)


@pytest.mark.parametrize("byte_off", [2, 8])
def test_chunk_refuses_rows_off_their_boundary(G, byte_off):
    S, n, ch = 3, 600000, 2
    rows = [pcm(6500 + s, n * ch, 0.3) for s in range(S)]
    dev = _dev_rows(rows, byte_off)
    assert all(d.data_ptr() % 16 == byte_off for d in dev)
    got, want, geo, fmt = _both(G, rows, ch, dev=dev, gains=GAINS3)
    assert geo["mix_first"] == 2, geo
    assert fmt == {"format": 1, "native": 0}  # k_rlm_chunk_pcm16's LDS-DMA needs 16-byte boundaries (rodio_hip.h)
    _same_bits(got, want)


# ---- 6. k_mix_rows_pcm16 ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mix", [None, "1", "2", "4", "12"])
@pytest.mark.parametrize("ch,n", [(2, 30000), (1, 30001), (2, 1537), (1, 4099), (2, 70000)])
def test_mix_rows(G, mix, ch, n):
    rows = [pcm(6100 + s, n * ch, 0.1) for s in range(9)]
    with knobs(**({"RH_MIX_U": mix} if mix else {})):
        got, want, geo, fmt = _both(G, rows, ch, gains=GAINS9)
    assert geo["mix_first"] == 1, geo
    # rows in allocations of their own lie on 8-byte boundaries, which is all k_mix_rows_pcm16 asks (any length: (1, 30001) ends in its guarded
    # tail); "12" is k_mix_ring, which has no PCM16 form
    assert fmt == {"format": 1, "native": 0 if mix == "12" else 1}
    _same_bits(got, want)


@pytest.mark.parametrize("byte_off,native", [(2, 0), (4, 0), (8, 1)])
def test_mix_rows_boundary(G, byte_off, native):
    ch, n = 1, 30001
    rows = [pcm(6100 + s, n * ch, 0.1) for s in range(9)]
    dev = _dev_rows(rows, byte_off)
    assert all(d.data_ptr() % 16 == byte_off for d in dev)
    got, want, geo, fmt = _both(G, rows, ch, dev=dev, gains=GAINS9)
    assert geo["mix_first"] == 1, geo
    assert fmt == {"format": 1, "native": native}
    _same_bits(got, want)


# ---- 7. the routes that run on the converted copy ---------------------------------------------------------------------------------------
def _rows7():
    return [pcm(6300 + s, 20000 * 2, 0.2) for s in range(4)]


def test_converted_no_filter(G, O):
    rows = _rows7()
    got, want, geo, fmt = _both(G, rows, 2, filt=None, freq=0)
    assert geo["mix_first"] == 0 and fmt == {"format": 1, "native": 0}
    _same_bits(got, want)
    m = O.Mixer(2, 48000)  # that path's own contract: rodio's ordered sum of converted samples, bit for bit
    for r in rows:
        m.add(O.UniformSourceIterator(O.TestSource(twin(r), 2, 44100), 2, 48000))
    assert np.array_equal(got, m.collect())


def test_converted_ragged(G):
    rows = [r[: 2 * (20000 - 100 * s)] for s, r in enumerate(_rows7())]
    got, want, geo, fmt = _both(G, rows, 2)
    assert geo["mix_first"] == 0 and fmt == {"format": 1, "native": 0}
    _same_bits(got, want)


def test_converted_general_kernel(G):
    got, want, geo, fmt = _both(G, _rows7(), 2, force_general=1)
    assert geo["general_kernel"] == 1 and fmt == {"format": 1, "native": 0}
    _same_bits(got, want)


def test_converted_filter_first(G):
    got, want, geo, fmt = _both(G, _rows7(), 2, filter_first=True)
    assert fmt == {"format": 1, "native": 0}
    _same_bits(got, want)


def test_converted_run_subset(G):
    got, want, geo, fmt = _both(G, _rows7(), 2, run=lambda p: p.run_subset(1, 2))
    assert fmt == {"format": 1, "native": 0}
    _same_bits(got, want)


def test_converted_run_batch(G):
    got, want, geo, fmt = _both(G, _rows7(), 2, run=lambda p: p.run_batch())
    assert fmt == {"format": 1, "native": 0}
    _same_bits(got, want)


def test_converted_per_source_filters(G):
    filters = [("low_pass", 200), ("high_pass", 300), None, ("low_pass", 200)]
    got, want, geo, fmt = _both(G, _rows7(), 2, filters=filters)
    assert fmt == {"format": 1, "native": 0}
    _same_bits(got, want)


# ---- 8. extremes, and neighbours that must not be read ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n,mix_first", [(600000, 2), (30000, 1)])
def test_extremes_and_packed_rows(G, n, mix_first):
    import torch

    ch = 2
    alt = np.tile(np.array([32767, -32768], dtype=np.int16), n * ch // 2)
    rows = [np.full(n * ch, -32768, dtype=np.int16), np.full(n * ch, 32767, dtype=np.int16), alt]
    got, want, geo, fmt = _both(G, rows, ch, gains=GAINS3)
    assert geo["mix_first"] == mix_first, geo
    assert fmt == {"format": 1, "native": 1}
    _same_bits(got, want)
    # the same rows back to back in one arena, 4 KiB of alternating full-scale samples in front of, between and behind them: a load that strays
    # into a neighbour changes a sample
    guard = np.tile(np.array([32767, -32768], dtype=np.int16), 1024)
    assert (n * ch * 2) % 16 == 0 and guard.nbytes == 4096
    arena = torch.from_numpy(np.concatenate([guard] + [np.concatenate([r, guard]) for r in rows])).cuda()
    dev, at = [], len(guard)
    for r in rows:
        dev.append(arena[at: at + len(r)])
        at += len(r) + len(guard)
    assert all(d.data_ptr() % 16 == 0 for d in dev)
    packed, _, geo2, fmt2 = _both(G, rows, ch, dev=dev, gains=GAINS3)
    assert geo2 == geo and fmt2 == fmt
    _same_bits(packed, got)


# ---- 9. switching between the two entries -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [600000, 30000])
def test_switching_gains_and_autotune(G, n):
    import torch

    S, ch = 3, 2
    rows = [pcm(6900 + s, n * ch, 0.3) for s in range(S)]
    f32 = [torch.from_numpy(twin(r)).cuda() for r in rows]
    i16 = _dev_rows(rows)
    p = _handle(G, rows, ch, gains=GAINS3)
    p.set_sources(f32)
    a = _twice(p, lambda h: h.run())
    assert p.source_format() == {"format": 0, "native": 0}
    p.set_sources(i16)
    b = _twice(p, lambda h: h.run())
    assert p.source_format() == {"format": 1, "native": 1}
    p.set_sources(f32)
    c = _twice(p, lambda h: h.run())
    assert p.source_format() == {"format": 0, "native": 0}
    _same_bits(b, a)
    _same_bits(c, a)
    # new gains behind set_sources_pcm16 reach the table the native kernels read
    g2 = np.array([0.25, -1.5, 0.0], dtype=np.float32)
    p.set_sources(i16)
    p.set_gains(g2)
    d = _twice(p, lambda h: h.run())
    assert p.source_format() == {"format": 1, "native": 1}
    assert not np.array_equal(d, a)
    # ... and the copy a converted run reads (a sub-mix of all three sources' worth: run_subset over the whole list is a whole run, so take two)
    e = _twice(p, lambda h: h.run_subset(0, 2))
    assert p.source_format() == {"format": 1, "native": 0}
    p.set_sources(f32)
    _same_bits(d, _twice(p, lambda h: h.run()))
    _same_bits(e, _twice(p, lambda h: h.run_subset(0, 2)))
    # the tuner runs on PCM16 sources and leaves a handle that still gives the bits of the same handle on f32 rows
    p.set_sources(i16)
    r, ns = p.autotune()
    assert r >= 1 and ns >= 2
    tuned = _twice(p, lambda h: h.run())
    p.set_sources(f32)
    _same_bits(tuned, _twice(p, lambda h: h.run()))
    p.close()


def test_a_stream_in_between_asks_for_the_sources_again(G):
    """The stream entries take f32 rows per block and leave their block in the handle's place: a one-shot run on the PCM16 sources set before it
    must not read the int16 rows by the block's lengths."""
    import torch
    from rodio_amd._lib import RhError

    rows = [pcm(6300 + s, 20000 * 2, 0.2) for s in range(2)]
    i16 = _dev_rows(rows)
    p = _handle(G, rows, 2)
    p.set_sources(i16)
    first = _twice(p, lambda h: h.run())
    assert p.source_format() == {"format": 1, "native": 1}
    p.stream_begin()
    p.stream_feed([torch.from_numpy(twin(r[:10000])).cuda() for r in rows], flush=True)
    with pytest.raises(RhError):
        p.run()
    p.set_sources(i16)
    _same_bits(_twice(p, lambda h: h.run()), first)
    p.close()


# ---- 10. the real asset -----------------------------------------------------------------------------------------------------------------
def test_music_wav(G):
    data = open(os.path.join(ROOT, "tests", "golden", "music.wav"), "rb").read()
    w = G.wav_probe(data)
    assert (w["channels"], w["bits_per_sample"], w["is_float"]) == (2, 16, 0)
    s = np.frombuffer(data, dtype="<i2", count=w["data_bytes"] // 2, offset=w["data_offset"]).reshape(-1, 2)
    assert len(s) == 447327
    n = 894648
    base = np.concatenate([s, s])[:n]
    rows = [np.ascontiguousarray(np.roll(base, k, axis=0)).reshape(-1) for k in (0, 1000, 50001, 200003)]
    got, want, geo, fmt = _both(G, rows, 2, gains=np.full(4, 0.25, dtype=np.float32))
    assert geo["mix_first"] == 2, geo
    assert fmt == {"format": 1, "native": 1}
    _same_bits(got, want)
