"""What every block mixer answers about the fields of an rh_wide_src they share -- rh_wide_mix_block(_filtered), rh_wide_mix_batch,
rh_player_mix_block, rh_spatial_mix_block, rh_loop_mix_block, rh_queue_mix_block, rh_clip_mix_block: one rule (check_src of
rodio_amd/csrc/rh_mix_plan.h), so one answer.  Three sources of 64 frames into a stereo mix of 64 frames; source 1 is replaced in turn by
each broken one.  Every output, scratch and source lies in a guarded arena (tests/arena.py): a refused call leaves the poison untouched, a
source that reaches no frame is not looked at.  Through the C ABI."""
import ctypes as C
from math import gcd

import numpy as np
import pytest

import arena

pytestmark = pytest.mark.gpu
OK, INVALID, UNSUPPORTED = 0, 1, 3
NONE = 0xFFFFFFFF
f32 = np.float32
M, TO_CH, TO_RATE, RATE = 64, 2, 48000, 44100  # F / T = 147 / 160: the taps of 64 output frames reach source frames 0 .. 58
PRIME_RATE, PRIME_FROM = 65537, 65539          # both prime: F T = 65538^2 - 1 > 2^32 - 1
GARBAGE_PTR = 0xDEAD0BAD0

# (what source 1 becomes, the status every entry must give); "prime" also moves the mixer to 65537 Hz
CASES = [("data_null", INVALID), ("channels_0", INVALID), ("from_rate_0", INVALID), ("frames_65", INVALID), ("phase_T", INVALID), ("prime", UNSUPPORTED),
         ("frames_0_garbage", OK), ("valid", OK)]
ENTRIES = ["wide", "filtered", "batch", "player", "spatial", "loop", "queue", "clip"]
PLAIN = [e for e in ENTRIES if e not in ("filtered", "spatial")]  # a table of plain sources: rh_wide_mix_block's bits


def vp(a):
    return C.c_void_p(a) if a is not None else None


@pytest.fixture(scope="module")
def K(rh):
    """The sources, once: three stereo ones, three mono ones (the emitters), a one-entry gain table, a second mixer's source."""
    import torch

    assert torch.cuda.is_available(), "gpu tests need a GPU"
    rh.init(0)
    rng = np.random.default_rng(2024)

    class Kit:
        pass

    k = Kit()
    k.rh = rh
    k.stereo = [arena.src_arena(rng.uniform(-1, 1, 2 * M).astype(f32)) for _ in range(3)]
    k.mono = [arena.src_arena(rng.uniform(-1, 1, M).astype(f32)) for _ in range(3)]
    k.other = arena.src_arena(rng.uniform(-1, 1, 2 * M).astype(f32))
    k.gains = arena.src_arena(np.array([0.75, -0.5], f32))  # [1 entry][2 channels]
    return k


def table(K, entry, case, to_rate, keep=(0, 1, 2)):
    """The rh_wide_src table of a call: sources `keep` of the three, source 1 as `case` says."""
    from rodio_amd import _lib

    mono = entry == "spatial"
    ins = K.mono if mono else K.stereo
    gains = (0.5, -1.25, 0.8)
    arr = (_lib.WideSrc * len(keep))()
    for q, s in enumerate(keep):
        x = arr[q]
        x.data, x.channels, x.from_rate, x.phase, x.frames, x.last, x.gain = ins[s].ptr(), 1 if mono else 2, RATE, 0, M, NONE, 1.0 if mono else gains[s]
        if s != 1:
            continue
        if case == "data_null":
            x.data = None
        elif case == "channels_0":
            x.channels = 0
        elif case == "from_rate_0":
            x.from_rate = 0
        elif case == "frames_65":
            x.frames = M + 1
        elif case == "phase_T":
            x.phase = to_rate // gcd(RATE, to_rate)
        elif case == "prime":
            x.from_rate = PRIME_FROM
        elif case == "frames_0_garbage":
            x.data, x.channels, x.from_rate, x.phase, x.frames, x.last, x.gain = GARBAGE_PTR, 0, 0, 0xFFFFFFF0, 0, 7, float("nan")
    return arr


def call(K, entry, arr, n, to_rate):
    """One call of `entry` on a fresh dst arena -> (status, [the arenas the call may write, with the words it must write on success])."""
    from rodio_amd import _lib, source

    lib, st = _lib.lib, source._stream()
    dst = arena.dst_arena(M * TO_CH)
    outs = [(dst, M * TO_CH)]
    u64 = C.c_uint64
    if entry == "wide":
        status = lib.rh_wide_mix_block(vp(dst.ptr()), TO_CH, to_rate, M, arr, n, st)
    elif entry == "filtered":
        kinds = (C.c_int32 * n)(0, *([-1] * (n - 1)))  # source 0 carries a low_pass
        co = np.zeros((n, 5), f32)
        co[0] = K.rh.biquad_coeffs(0, 1000, 0.5, to_rate)
        need = u64(0)
        assert lib.rh_wide_mix_filtered_scratch_bytes(TO_CH, M, 1, C.byref(need)) == OK and need.value % 4 == 0
        scratch = arena.dst_arena(need.value // 4)
        outs.append((scratch, None))
        status = lib.rh_wide_mix_block_filtered(vp(dst.ptr()), TO_CH, to_rate, M, arr, n, kinds, co.ctypes.data_as(_lib.f32p), (C.c_void_p * n)(), 0, vp(scratch.ptr()), need.value, st)
    elif entry == "batch":  # a second mixer of one source, so that the call does not go to rh_wide_mix_block
        dst2 = arena.dst_arena(M * TO_CH)
        outs.append((dst2, M * TO_CH))
        flat = (_lib.WideSrc * (n + 1))()
        for q in range(n):
            C.memmove(C.byref(flat, q * C.sizeof(_lib.WideSrc)), C.byref(arr[q]), C.sizeof(_lib.WideSrc))
        x = flat[n]
        x.data, x.channels, x.from_rate, x.phase, x.frames, x.last, x.gain = K.other.ptr(), 2, RATE, 0, M, NONE, 1.0
        status = lib.rh_wide_mix_batch((C.c_void_p * 2)(dst.ptr(), dst2.ptr()), (C.c_uint32 * 2)(TO_CH, TO_CH), (C.c_uint32 * 2)(to_rate, to_rate), (u64 * 2)(M, M),
                                       (C.c_uint32 * 2)(n, 1), 2, flat, st)
    elif entry == "player":
        status = lib.rh_player_mix_block(vp(dst.ptr()), TO_CH, to_rate, M, arr, n, None, None, None, None, st)
    elif entry == "spatial":
        gains = (C.c_void_p * n)(*[K.gains.ptr()] * n)
        gsteps = (u64 * (3 * n))(*[0, 1 << 20, 1] * n)  # first, period, entries: one entry covers the block
        status = lib.rh_spatial_mix_block(vp(dst.ptr()), TO_CH, to_rate, M, arr, n, gains, gsteps, None, None, st)
    elif entry == "loop":
        status = lib.rh_loop_mix_block(vp(dst.ptr()), TO_CH, to_rate, M, arr, n, (u64 * (source.LOOP_WORDS * n))(), st)
    elif entry == "queue":
        status = lib.rh_queue_mix_block(vp(dst.ptr()), TO_CH, to_rate, M, arr, n, None, None, (C.c_uint32 * n)(), (u64 * (source.QUEUE_WORDS * n))(), st)
    else:
        status = lib.rh_clip_mix_block(vp(dst.ptr()), TO_CH, to_rate, M, arr, n, (u64 * (source.CLIP_WORDS * n))(), st)
    return status, outs


def run(K, entry, case, keep=(0, 1, 2)):
    to_rate = PRIME_RATE if case == "prime" else TO_RATE
    status, outs = call(K, entry, table(K, entry, case, to_rate, keep), len(keep), to_rate)
    rows = []
    for a, n in outs:
        if n is None:
            a.check_guards()  # a scratch: the entry may use as much of it as it likes, and nothing beside it
        else:
            rows.append(a.check(written=n if status == OK else 0))  # refused: every word still holds the sentinel
    for a in K.stereo + K.mono + [K.other, K.gains]:
        a.unchanged()
    return status, rows


@pytest.mark.parametrize("case,want", CASES)
@pytest.mark.parametrize("entry", ENTRIES)
def test_every_entry_gives_the_shared_rules_status(K, entry, case, want):
    status, rows = run(K, entry, case)
    assert status == want, (entry, case, status)
    if case == "frames_0_garbage":  # not looked at: the mix of the two remaining sources
        status2, rows2 = run(K, entry, "valid", keep=(0, 2))
        assert status2 == OK and all(arena.same(a, b) for a, b in zip(rows, rows2))


def test_a_table_of_plain_sources_is_the_same_mix_through_every_entry(K):
    mixes = [run(K, entry, "valid")[1][0] for entry in PLAIN]
    assert all(arena.same(mixes[0], m) for m in mixes[1:])
    assert np.all(np.isfinite(mixes[0])) and np.any(mixes[0] != 0)
