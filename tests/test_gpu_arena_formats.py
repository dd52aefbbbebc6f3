"""The sample-format entries in a hostile memory layout (tests/arena.py): all 22 rh_convert_* and rh_wav_decode / rh_wav_decode_channels.
Rows of 1-, 2-, 4- and 8-byte elements and sample bytes at any byte address.  Integers have no NaN, so an integer source lies between two
different byte fills in turn (the output must equal the reference under both, and the two outputs each other), and an integer or f64
destination lies in two different sentinel fills in turn (under each, every guard byte untouched and the row equal to the reference: an
element that was never written equals it under at most one).  Float sources keep the NaN poison, f32 destinations the NaN sentinel.
Every case: (a) the arena checks, sources unchanged; (b) the row against the oracle's restatement of the conversion, bit for bit; (c) the
same bytes as the same call on rows in friendly surroundings (zeros) at the same leads.  Through the C ABI."""
import ctypes as C

import numpy as np
import pytest
from conftest import knobs

import arena

pytestmark = pytest.mark.gpu
f32 = np.float32

NP = {"i8": np.int8, "u8": np.uint8, "i16": np.int16, "u16": np.uint16, "i24": np.int32, "u24": np.int32, "i32": np.int32, "u32": np.uint32,
      "i64": np.int64, "u64": np.uint64, "f32": np.float32, "f64": np.float64}
TO_F32 = ["i8", "u8", "i16", "u16", "i24", "i32", "u24", "u32", "i64", "u64", "f64"]
FROM_F32 = ["i8", "i16", "u16", "i32", "u8", "i24", "u24", "u32", "i64", "u64", "f64"]
# Leads in ELEMENTS behind a 16-byte boundary, per element size, so that the address takes every residue the launchers branch on:
#   1 byte : src % 4 in {0, 1, 2, 3} (k_int_to_f32_lines wants 0), % 16 in {0, 4, 8, ..} (4 and 8: on a 4-byte boundary and off a vector)
#   2 bytes: src % 8 in {0, 2, 4, 6}, % 16 (8: on an 8-byte boundary and off a vector; 14: the last residue)
#   4 bytes: % 16 in {0, 4, 8, 12};  8 bytes: % 16 in {0, 8} (sizeof(Pack<i64, 2>) == 16)
# and the same for a dst of that size: dst % (4 * sizeof(T)) for k_f32_to_int, dst % 16 for the rest.
ELEM_LEADS = {1: [0, 1, 2, 3, 4, 8, 15], 2: [0, 1, 2, 3, 4, 7], 4: [0, 1, 2, 3], 8: [0, 1]}
SIZES = [10007, 3, 1]  # 10007: 40 workgroups of vectors and a ragged one; 3 and 1: below one vector of every converter (E = 4 or 2)


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    return rh


def _st():
    from rodio_amd import source

    return source._stream()


def L():
    from rodio_amd import _lib

    return _lib.lib


def vp(a):
    return C.c_void_p(a) if a is not None else None


def lead_pairs(src_size, dst_size):
    """(src lead, dst lead) in elements: every src lead, every dst lead, both on a boundary, both on their last residue"""
    sl, dl = ELEM_LEADS[src_size], ELEM_LEADS[dst_size]
    pairs = [(s, dl[i % len(dl)]) for i, s in enumerate(sl)] + [(sl[(i + 1) % len(sl)], d) for i, d in enumerate(dl)]
    pairs += [(0, 0), (sl[-1], dl[-1]), (0, dl[1]), (sl[1], 0), (sl[-2], 0)]
    return sorted(set(pairs))


def ints(kind, n, seed):
    """n values over the type's whole range, its extremes and zero in front"""
    info = {"i24": (-2 ** 23, 2 ** 23 - 1), "u24": (0, 2 ** 24 - 1)}.get(kind) or (int(np.iinfo(NP[kind]).min), int(np.iinfo(NP[kind]).max))
    rng = np.random.default_rng(seed)
    if kind in ("i64", "u64"):
        x = rng.integers(0, 2 ** 64, n, dtype=np.uint64).view(NP[kind]).copy()
        odd = 2 ** 62 + 2 ** 38 + 1  # where one rounding and two differ (RH_DASP_I64_VIA_F64); u64 goes through i64 by subtracting 2^63
        head = [info[0], info[1], 0, odd + (2 ** 63 if kind == "u64" else 0), 1]
    else:
        x = rng.integers(info[0], info[1] + 1, n, dtype=np.int64).astype(NP[kind])
        head = [info[0], info[1], 0, 1, (info[0] + info[1]) // 2]
    for k, v in enumerate(head[:n]):
        x[k] = NP[kind](v) if kind != "u64" else np.uint64(v % 2 ** 64)
    return x


def floats(n, seed):
    """n finite f32 in +-1.5 with both zeros, the saturating values of every integer target, a subnormal and 2^-24 in front"""
    x = np.random.default_rng(seed).uniform(-1.5, 1.5, n).astype(f32)
    head = [-0.0, 1.0, -2.0, 0.0, 0.99999994, -1.0, 300.0, -300.0, 1e-40, 2.0 ** -24, -0.99999994, 2.0, 1e-9]
    for k, v in enumerate(head[:n]):
        x[k] = f32(v)
    return x


def convert_case(name, x, ref, ls, ld):
    """rh_convert_<name> over x `ls` elements behind a 16-byte boundary into a row `ld` elements behind one: the three assertions"""
    import torch

    fn = getattr(L(), "rh_convert_" + name)
    src_t, dst_t = name.split("_to_")
    n, ssz, dsz = x.size, x.dtype.itemsize, np.dtype(NP[dst_t]).itemsize
    int_src, byte_dst = src_t not in ("f32", "f64"), dst_t != "f32"
    outs = []
    for fill in (arena.FILLS if (int_src or byte_dst) else arena.FILLS[:1]):
        if src_t == "f32":
            src = arena.src_arena(x, ls)
        else:  # integers between the fill; f64 between bytes of 0xff (a NaN of every size)
            src = arena.src_bytes_arena(x, ls * ssz, fill if int_src else arena.NAN_FILL)
        dst = arena.dst_bytes_arena(n, NP[dst_t], ld * dsz, fill) if byte_dst else arena.dst_arena(n, ld)
        assert fn(vp(dst.ptr()), vp(src.ptr()), n, _st()) == 0, name
        got = dst.check(ref, dtype=NP[dst_t]) if byte_dst else dst.check()  # (a), and (b) for a byte dst: check_filled holds the row against ref
        src.unchanged()
        outs.append(got)
        assert np.array_equal(arena.as_bytes(got), arena.as_bytes(ref)), (name, n, ls, ld, hex(fill))  # (b)
    if int_src:
        arena.same_under_fills(outs, ref)
    pt, pp = arena.plain(x, lead=ls)  # (c)
    pd = torch.zeros(n * dsz + 64, dtype=torch.uint8, device="cuda")
    assert fn(vp(pd.data_ptr() + ld * dsz), vp(pp), n, _st()) == 0
    torch.cuda.synchronize()
    plain = pd.cpu().numpy()[ld * dsz: (ld + n) * dsz]
    assert np.array_equal(plain, arena.as_bytes(outs[0])), (name, n, ls, ld, "the arena run differs from the plain run")


# Routes of launch_int_to_f32 (rh_elementwise.hip), 1- and 2-byte samples:
#   lines   dst on a 16-byte boundary and src on a boundary of four samples: leads (0, 0), and src leads 4 and 8 (1 byte) / 4 (2 bytes) with dst 0
#   vector  (k_int_to_f32: dst and src on 16-byte boundaries) is taken only where `lines` is switched off (RH_PCM_NO_TILE: test_gpu_fallbacks.py);
#           every pair of pointers it would take goes to `lines` first
#   tile    i16 / u8 off those boundaries (rh::pcm_tile_try, one channel): any src lead with dst lead != 0, src leads 1, 2, 3 with dst lead 0
#   scalar  i8 / u16 off those boundaries: the same leads
# i24 / i32 (k_i32_to_f32): vec_ok = both on 16-byte boundaries, (0, 0) only.  The Pack converters (rh_formats.hip): vec_ok = src and dst on
# the boundaries of their packs, (0, 0) only for the 4-byte types, and for i64 / u64 / f64 <-> f32 also src 0 with an even f32 lead.
@pytest.mark.parametrize("kind", TO_F32)
def test_convert_to_f32_rows(G, O, kind):
    name = kind + "_to_f32"
    for n in SIZES:
        x = floats(n, 5).astype(np.float64) * (1.0 + 2.0 ** -30) if kind == "f64" else ints(kind, n, 11 + n)  # (f64 values that are no f32: the conversion rounds)
        ref = O.convert(name, x)
        assert ref.dtype == f32 and np.all(np.isfinite(ref))
        for ls, ld in lead_pairs(x.dtype.itemsize, 4):
            convert_case(name, x, ref, ls, ld)


@pytest.mark.parametrize("kind", ["i8", "u8", "i16", "u16"])
def test_convert_small_ints_vector_route(G, O, kind):
    """launch_int_to_f32's second route, k_int_to_f32 (16 bytes in a lane, two loads in flight): with RH_PCM_NO_TILE=1 rows on 16-byte
    boundaries go there instead of to `lines`, and every other row -- i16 and u8 included, whose tile kernel the knob switches off -- to the
    scalar kernel.  n = 10007: 625 (1-byte) or 1250 (2-byte) whole vectors over several workgroups and a scalar tail of 7 samples; n = 3 and
    1: the tail alone."""
    name = kind + "_to_f32"
    with knobs(RH_PCM_NO_TILE="1"):
        for n in SIZES:
            x = ints(kind, n, 21 + n)
            ref = O.convert(name, x)
            for ls, ld in [(0, 0), (1, 0), (0, 1), (ELEM_LEADS[x.dtype.itemsize][4], 0)]:
                convert_case(name, x, ref, ls, ld)


@pytest.mark.parametrize("kind", FROM_F32)
def test_convert_from_f32_rows(G, O, kind):
    """f32 -> integers: vec_ok of k_f32_to_int is src on a 16-byte boundary and dst on one of four samples (i8: 4 bytes; i16 / u16: 8; i32: 16)
    -- (0, 0), and dst leads 4 and 8 for the 1-byte and 4 for the 2-byte targets; everything else sample by sample.  Saturation on both
    sides, both zeros."""
    name = "f32_to_" + kind
    for n in SIZES:
        x = floats(n, 7 + n)
        ref = O.convert(name, x)
        for ls, ld in lead_pairs(4, np.dtype(NP[kind]).itemsize):
            convert_case(name, x, ref, ls, ld)


@pytest.mark.parametrize("kind", ["i64", "u64"])
def test_convert_64_bit_integers_through_f64(G, O, kind):
    """the other reading of dasp's i64 -> f32 (RH_DASP_I64_VIA_F64=1: two roundings), the same arenas"""
    name = kind + "_to_f32"
    x = ints(kind, 10007, 3)
    once, twice = O.convert(name, x), O.convert(name + "_via_f64", x)
    assert not np.array_equal(once, twice)
    with knobs(RH_DASP_I64_VIA_F64="1"):
        for ls, ld in lead_pairs(8, 4):
            convert_case(name, x, twice, ls, ld)


def test_convert_refusals_write_nothing(G):
    """a NULL pointer with samples to convert: RH_ERR_INVALID, the dst keeps every sentinel"""
    lib = L()
    src = arena.src_bytes_arena(ints("i16", 64, 1), 2)
    for fill in arena.FILLS:
        dst = arena.dst_bytes_arena(64, np.int16, 6, fill)
        assert lib.rh_convert_f32_to_i16(vp(dst.ptr()), None, 64, _st()) == 1
        dst.check(np.zeros(64, np.int16), written=0)
    d32 = arena.dst_arena(64, 1)
    assert lib.rh_convert_i16_to_f32(vp(d32.ptr()), None, 64, _st()) == 1 and lib.rh_convert_i16_to_f32(None, vp(src.ptr()), 64, _st()) == 1
    d32.check(0)
    src.unchanged()


# ---- rh_wav_decode, rh_wav_decode_channels ---------------------------------------------------------------------------------------------------
WAV = [("u8", 8, 0, 1), ("i16", 16, 0, 2), ("i24", 24, 0, 3), ("i32", 32, 0, 4), ("f32", 32, 1, 4)]  # format, bits, is_float, bytes a sample
BYTE_LEADS = [0, 1, 2, 3, 4, 5, 8, 15]  # `file + data_offset`; 4 and 8: on the sample's own boundary and off the vector's (rh_wav_decode's tile route for i32 / u8 / i16)
WAV_CH = 3


def wav_tile_frames(bps, ch, to):
    """Frames a tile of k_pcm_to_channels_tile (rh::pcm_tile_try): ~10 KiB in + out, a multiple of 4"""
    return (10240 // (ch * bps + 4 * to)) & ~3


def wav_samples(fmt, n, seed):
    """(the sample bytes as the file holds them, the samples as f32)"""
    import struct

    if fmt == "f32":
        x = floats(n, seed)
        return x.astype("<f4").view(np.uint8), x
    if fmt == "i24":
        v = ints("i24", n, seed)
        raw = np.frombuffer(b"".join(struct.pack("<i", int(s))[:3] for s in v), np.uint8)
        return raw, v
    v = ints({"u8": "u8", "i16": "i16", "i32": "i32"}[fmt], n, seed)
    return v.astype(v.dtype.newbyteorder("<")).view(np.uint8), v


def test_wav_tile_frames_are_what_the_launcher_derives():
    assert [wav_tile_frames(b, WAV_CH, 2) for _, _, _, b in WAV] == [928, 728, 600, 512, 512]


@pytest.mark.parametrize("fmt,bits,is_float,bps", WAV)
@pytest.mark.parametrize("to", [WAV_CH, 2, 5])
def test_wav_decode_rows(G, O, fmt, bits, is_float, bps, to):
    """to == channels: rh_wav_decode, whose routes are decided by the byte address -- on a vector boundary the converters of
    rh_elementwise.hip (u8, i16, i32), a device copy (f32) or the tile kernel (i24), then k_fill_zero for the cut frame; off the vector's
    boundary and on the sample's the tile kernel; off the sample's own boundary rh_wav_decode_channels.  to != channels:
    rh_wav_decode_channels, the tile kernel in its aligned and its BYTES instantiation (i16 at odd addresses, i32 / f32 off a 4-byte boundary).
    1 and 7 frames and two whole tiles plus 3; n_samples ends one sample inside the last frame: zeros complete it."""
    lib = L()
    ch = WAV_CH
    tf = wav_tile_frames(bps, ch, to)
    assert tf >= 8
    for frames in (1, 7, 2 * tf + 3):
        n = frames * ch - 1
        raw, vals = wav_samples(fmt, n, frames + bits)
        dec = vals if fmt == "f32" else O.convert({"u8": "u8_to_f32", "i16": "i16_to_f32", "i24": "i24_to_f32", "i32": "i32_to_f32"}[fmt], vals)
        dec = np.concatenate([dec, np.zeros(frames * ch - n, f32)])  # wav.rs:161-169
        ref = dec if to == ch else O.ChannelCountConverter(O.TestSource(dec, ch, 48000), ch, to).collect()
        total = frames * to
        assert ref.size == total

        def call(d, s):
            m = C.c_uint64(0)
            if to == ch:
                st = lib.rh_wav_decode(vp(d), vp(s), n, ch, bits, is_float, C.byref(m), _st())
            else:
                st = lib.rh_wav_decode_channels(vp(d), vp(s), n, ch, bits, is_float, to, C.byref(m), _st())
            assert st == 0 and m.value == total, (fmt, to, st, m.value)

        fills = (arena.NAN_FILL, arena.FILLS[0]) if fmt == "f32" else arena.FILLS  # f32 bytes: a NaN at every byte shift, and a second surrounding
        for so in BYTE_LEADS:
            outs = []
            for fill in fills:
                src = arena.src_bytes_arena(raw, so, fill)
                dst = arena.dst_arena(total, so % 4)
                call(dst.ptr(), src.ptr())
                outs.append(dst.check())
                src.unchanged()
            arena.same_under_fills(outs, ref, fills=fills)
            import torch

            pt, pp = arena.plain(raw, lead=so)
            dt, dp = arena.plain_dst(total + 4)
            call(dp + 4 * (so % 4), pp)
            torch.cuda.synchronize()
            assert arena.same(dt.cpu().numpy()[so % 4: so % 4 + total], outs[0]), (fmt, to, frames, so, "the arena run differs from the plain run")


def test_wav_decode_refusals_write_nothing(G):
    """an unofficial depth, a float format that is not 32 bits, no channels, a NULL data pointer: refused, every sentinel intact"""
    lib = L()
    src, dst = arena.src_bytes_arena(ints("i16", 64, 1), 2), arena.dst_arena(80, 1)
    m = C.c_uint64(0)
    assert lib.rh_wav_decode(vp(dst.ptr()), vp(src.ptr()), 64, 2, 12, 0, C.byref(m), _st()) == 3
    assert lib.rh_wav_decode(vp(dst.ptr()), vp(src.ptr()), 32, 2, 16, 1, C.byref(m), _st()) == 3
    assert lib.rh_wav_decode_channels(vp(dst.ptr()), vp(src.ptr()), 64, 2, 12, 0, 2, C.byref(m), _st()) == 3
    assert lib.rh_wav_decode_channels(vp(dst.ptr()), vp(src.ptr()), 64, 0, 16, 0, 2, C.byref(m), _st()) == 1
    assert lib.rh_wav_decode_channels(vp(dst.ptr()), None, 64, 2, 16, 0, 2, C.byref(m), _st()) == 1
    assert lib.rh_wav_decode(vp(dst.ptr()), None, 64, 2, 16, 0, C.byref(m), _st()) == 1
    dst.check(0)
    src.unchanged()
