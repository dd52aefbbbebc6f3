"""Source::mix and Source::take_crossfade_with on the MI355X: rh_mix_pair (all four arms, every alignment, in place), GpuSource.mix
and take_crossfade_with against the CPU restatement of tests/test_mix_cpu.py, the fused rh_crossfade against the composed path,
and the C++ mirror's Mix / Crossfade (include/rodio_hip.hpp) against the library.  Every comparison is bit for bit on uint32 views."""
import ctypes as C

import numpy as np
import pytest

from test_mix_cpu import (CROSSFADE_CASES, CROSSFADE_D, MS, bits, check_mirror_generators, check_mirror_host_fed, check_mirror_mixer, crossfade_case, crossfade_restated,
                          mix_restated, mix_rows, same_bits, signal)

pytestmark = pytest.mark.gpu
f32 = np.float32
LENGTHS = [0, 1, 3, 4, 5, 255, 256, 257, 1027]


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def stream():
    import torch

    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def special_rows(na, nb, seed):
    """Two rows with the values whose bits a sum or a copy could lose: -0.0 in front of both (-0.0 + -0.0), and in the LONGER row's tail
    -- where Mix hands it on verbatim -- a -0.0 and a NaN with a payload."""
    a, b = signal(na, seed), signal(nb, seed + 1000)
    for x in (a, b):
        if x.size:
            x[0] = -0.0
    long, short = (a, b) if na > nb else (b, a)
    if long.size > short.size:
        long[-1] = -0.0
    if long.size - 2 >= short.size:
        long.view(np.uint32)[-2] = 0x7FC12345
    return a, b


def mix_pair(rh, a, b, off_a=0, off_b=0, off_d=0, in_place=None):
    """rh_mix_pair over rows at off_* floats from a 16-byte boundary; in_place = "a" / "b": dst is that input."""
    import torch

    rh.source._ensure()
    n = max(a.size, b.size)
    ta, tb = torch.zeros(a.size + 8, device="cuda"), torch.zeros(b.size + 8, device="cuda")
    pad = 7  # canaries behind the row
    if in_place == "a":
        ta = torch.zeros(n + 8 + pad, device="cuda")
    if in_place == "b":
        tb = torch.zeros(n + 8 + pad, device="cuda")
    ta[off_a:off_a + a.size] = torch.from_numpy(a).cuda()
    tb[off_b:off_b + b.size] = torch.from_numpy(b).cuda()
    td = torch.full((n + 8 + pad,), 7.0, device="cuda")
    dst, off = (ta, off_a) if in_place == "a" else (tb, off_b) if in_place == "b" else (td, off_d)
    before = host(dst).copy()
    st = rh.lib.rh_mix_pair(C.c_void_p(dst.data_ptr() + 4 * off), C.c_void_p(ta.data_ptr() + 4 * off_a), a.size, C.c_void_p(tb.data_ptr() + 4 * off_b), b.size, stream())
    assert st == 0
    got = host(dst)
    assert np.array_equal(bits(got[:off]), bits(before[:off])) and np.array_equal(bits(got[off + n:]), bits(before[off + n:])), "wrote outside the row"
    return got[off:off + n]


@pytest.mark.parametrize("na", LENGTHS)
def test_mix_pair_lengths_and_arms(rh, na):
    for nb in LENGTHS:
        a, b = special_rows(na, nb, 100 + na)
        assert same_bits(mix_pair(rh, a, b), mix_rows(a, b)), (na, nb)


def test_mix_pair_zero_signs_and_payloads(rh):
    a, b = special_rows(260, 1027, 1)
    got = mix_pair(rh, a, b)
    assert bits(got)[0] == 0x80000000  # -0.0 + -0.0
    assert bits(got)[-1] == 0x80000000 and bits(got)[-2] == 0x7FC12345  # the verbatim tail
    got = mix_pair(rh, b, a)
    assert bits(got)[0] == 0x80000000 and bits(got)[-1] == 0x80000000 and bits(got)[-2] == 0x7FC12345


@pytest.mark.parametrize("off_a", [0, 1, 2, 3])
def test_mix_pair_alignments(rh, off_a):
    for off_b in range(4):
        for off_d in range(4):
            for na, nb in [(1027, 257), (255, 1027), (5, 5)]:
                a, b = special_rows(na, nb, 3)
                assert same_bits(mix_pair(rh, a, b, off_a, off_b, off_d), mix_rows(a, b)), (off_a, off_b, off_d, na, nb)


@pytest.mark.parametrize("which", ["a", "b"])
def test_mix_pair_in_place(rh, which):
    for na, nb in [(1027, 257), (257, 1027), (256, 256), (0, 5), (5, 0)]:
        for off in (0, 1, 3):
            a, b = special_rows(na, nb, 5)
            assert same_bits(mix_pair(rh, a, b, off, (off + 1) % 4, 0, in_place=which), mix_rows(a, b)), (which, na, nb, off)


# ---- GpuSource.mix against the restatement --------------------------------------------------------------------------------------
def make(mod, x, ch, rate, span):
    return mod.SpanSource(x, ch, rate, span) if span else mod.TestSource(x, ch, rate)


MIX_CASES = [  # (a: channels, rate, samples, span), (b: ...)
    ((2, 48000, 6000, 0), (1, 44100, 3000, 0)),      # b shorter
    ((2, 48000, 6000, 0), (1, 44100, 50000, 0)),     # b longer (and past one chunk of the converter's 32-bit positions)
    ((1, 8000, 3000, 0), (6, 48000, 30000, 0)),      # b shorter: 5000 frames at 48 kHz are 834 at 8 kHz
    ((1, 8000, 1000, 0), (6, 48000, 48000, 0)),      # b longer: 8000 frames are 1334 (a side of 50 000 samples at most cannot outlast 3000 here)
    ((6, 48000, 30000, 0), (2, 44100, 3000, 0)),
    ((6, 48000, 6000, 0), (2, 44100, 40000, 0)),
    ((2, 48000, 6000, 1000), (1, 44100, 5000, 0)),   # spans of 1000 samples on a: the identity all the same
    ((2, 48000, 6000, 0), (1, 44100, 5000, 1000)),   # ... on b: a fresh converter every 1000 samples
    ((1, 8000, 3000, 0), (6, 48000, 30000, 1000)),   # ... of six channels: every chain ends inside a frame
    ((6, 48000, 30000, 1000), (2, 44100, 40000, 1000)),
    ((2, 48000, 50000, 0), (2, 48000, 3001, 0)),     # equal formats, b ends inside a frame
]


@pytest.mark.parametrize("case", range(len(MIX_CASES)))
def test_gpusource_mix_against_restatement(rh, O, case):
    (ca, ra, na, sa), (cb, rb, nb, sb) = MIX_CASES[case]
    a, b = signal(na, 31 + case), signal(nb, 57 + case)
    want = mix_restated(O, make(O, a, ca, ra, sa), make(O, b, cb, rb, sb))
    got = make(rh, a, ca, ra, sa).mix(make(rh, b, cb, rb, sb))
    assert (got.channels(), got.sample_rate(), got.current_span_len()) == (ca, ra, None)
    assert same_bits(got.collect(), want), case


def test_gpusource_mix_of_a_cut_take_duration(rh, O):
    """A first input that is a TakeDuration whose duration expires inside a frame: the identity wrapper in front of it ends before the
    silence that completes the frame (take.rs:109-123,180-196), so the mix is 4801 samples here, not 4802 -- b shorter and b longer."""
    d = 50 * MS + 10_416
    a = signal(6000, 71)
    assert rh.TestSource(a, 2, 48000).take_duration(d).collect().size == 4802
    for nb, n in [(1000, 4801), (3000, 6532)]:  # 3000 frames at 44.1 kHz are 3266 stereo frames at 48 kHz
        b = signal(nb, 72)
        want = mix_restated(O, O.TestSource(a, 2, 48000).take_duration(d), O.TestSource(b, 1, 44100))
        got = rh.TestSource(a, 2, 48000).take_duration(d).mix(rh.TestSource(b, 1, 44100)).collect()
        assert want.size == n and same_bits(got, want), nb


@pytest.mark.parametrize("delay_ns", [7 * MS, 7 * MS + 10_417])
def test_reverb_identity_on_the_device(rh, delay_ns):
    """mix(x, x.amplify(g).delay(d)) has the bits of reverb(d, g) (rh_echo_mix), an odd delay included."""
    x = signal(6000, 11)
    x[5] = -0.0
    want = rh.TestSource(x, 2, 48000).reverb(delay_ns, 0.3).collect()
    got = rh.TestSource(x, 2, 48000).mix(rh.TestSource(x, 2, 48000).amplify(0.3).delay(delay_ns)).collect()
    assert want.size == 6000 + rh.delay_samples(delay_ns, 48000, 2) and same_bits(got, want)


def test_reference_crossfade_tests_on_the_device(rh):  # crossfade.rs:46-80
    ten = np.arange(1, 11, dtype=f32)
    got = rh.SamplesBuffer(1, 1, ten).take_crossfade_with(rh.SamplesBuffer(1, 1, ten), CROSSFADE_D).collect()
    assert got.tolist() == [1.0, 2.0, 3.0, 4.0, 5.0]
    got = rh.SamplesBuffer(1, 1, ten).take_crossfade_with(rh.TestSource(np.zeros(10, f32), 1, 1), CROSSFADE_D).collect()
    assert got.size == 5 and np.all(np.abs(got - np.array([1.0, 2.0 * 0.8, 3.0 * 0.6, 4.0 * 0.4, 5.0 * 0.2])) < 1e-6)


@pytest.mark.parametrize("name", list(CROSSFADE_CASES))
def test_take_crossfade_with_against_restatement(rh, O, name):
    a, b, d, want = crossfade_case(O, name)
    got = rh.TestSource(a, 2, 48000).take_crossfade_with(rh.TestSource(b, 1, 44100), d)
    assert same_bits(got.collect(), want), name
    assert (got.channels(), got.sample_rate(), got.current_span_len()) == (2, 48000, None)


# ---- rh_crossfade: the fused batch against the composed path ---------------------------------------------------------------------
def test_crossfade_batch_equals_composed_pair_by_pair(rh, O):
    """One batch of 50 ms crossfades: pairs the kernel declines (a 6-channel b) next to pairs it takes (equal rates, either side
    shorter than the duration, an 8-channel a, a mono a), each against the restatement and the composed path; twice."""
    extra = [((signal(6000, 41), 2, 48000), (signal(18000, 42), 6, 48000)),  # 6-channel b: composed
             ((signal(6000, 43), 2, 48000), (signal(6000, 44), 2, 48000)),   # a stereo pair at equal rates: fused, the converter passes through
             ((signal(6000, 45), 2, 48000), (signal(3000, 46), 1, 44100)),
             ((signal(1000, 47), 2, 48000), (signal(3000, 48), 1, 44100)),   # a shorter than the duration
             ((signal(6000, 49), 2, 48000), (signal(500, 50), 1, 44100)),    # b shorter
             ((signal(6000, 51), 8, 48000), (signal(3000, 52), 2, 32000)),
             ((signal(6000, 53), 1, 44100), (signal(6000, 54), 2, 48000))]
    d = 50 * MS
    a = [rh.TestSource(*x) for x, _ in extra]
    b = [rh.TestSource(*y) for _, y in extra]
    first = [g.collect() for g in rh.crossfade_batch(a, b, d)]
    for k, (x, y) in enumerate(extra):
        want = crossfade_restated(O, O.TestSource(*x), O.TestSource(*y), d)
        composed = rh.TestSource(*x).take_crossfade_with(rh.TestSource(*y), d).collect()
        assert same_bits(composed, want) and same_bits(first[k], composed), k
    again = [g.collect() for g in rh.crossfade_batch(a, b, d)]  # a second call over the same batch
    assert all(same_bits(p, q) for p, q in zip(first, again))


@pytest.mark.parametrize("name", list(CROSSFADE_CASES))
def test_crossfade_batch_cases(rh, O, name):
    """Each of the seven cases through rh_crossfade, next to a pair the kernel declines (a b whose span cuts frames) in the same call."""
    a, b, d, want = crossfade_case(O, name)
    a6, b6 = signal(6000, 61), signal(18000, 62)
    got = rh.crossfade_batch([rh.TestSource(a, 2, 48000), rh.TestSource(a6, 2, 48000), rh.TestSource(a, 2, 48000)],
                             [rh.TestSource(b, 1, 44100), rh.SpanSource(b6, 6, 48000, 1000), rh.SpanSource(b, 1, 44100, 1000)], d)
    assert same_bits(got[0].collect(), want), name
    assert same_bits(got[1].collect(), crossfade_restated(O, O.TestSource(a6, 2, 48000), O.SpanSource(b6, 6, 48000, 1000), d))
    assert same_bits(got[2].collect(), crossfade_restated(O, O.TestSource(a, 2, 48000), O.SpanSource(b, 1, 44100, 1000), d))
    assert same_bits(got[0].collect(), rh.TestSource(a, 2, 48000).take_crossfade_with(rh.TestSource(b, 1, 44100), d).collect())


def test_crossfade_capacity_too_small_writes_nothing(rh):
    import torch

    rh.source._ensure()
    a, b = rh.TestSource(signal(6000, 1), 2, 48000), rh.TestSource(signal(3000, 2), 1, 44100)
    dst = torch.full((2, 4800), 7.0, device="cuda")
    pairs = (C.c_uint64 * 22)()
    for k, cap in enumerate([4800, 4799]):  # the SECOND pair is the one that does not fit: the first is not written either
        pairs[11 * k: 11 * k + 11] = [a.samples.data_ptr(), 6000, 2, 48000, b.samples.data_ptr(), 3000, 1, 44100, 0, dst[k].data_ptr(), cap]
    assert rh.lib.rh_crossfade(pairs, 2, 50 * MS, None, stream()) == 1  # RH_ERR_INVALID
    assert np.all(host(dst) == 7.0)
    pairs[21] = 4800
    got = (C.c_uint64 * 2)()
    assert rh.lib.rh_crossfade(pairs, 2, 50 * MS, got, stream()) == 0 and list(got) == [4800, 4800]
    out = host(dst)
    assert same_bits(out[0], out[1]) and not np.any(out == 7.0)
    pairs[2] = 0  # a_channels
    assert rh.lib.rh_crossfade(pairs, 2, 50 * MS, None, stream()) == 1


# ---- the C++ mirror on the GPU ---------------------------------------------------------------------------------------------------
def test_cpp_mix_of_generators_stays_on_the_device(tmp_path):
    check_mirror_generators(False, tmp_path)


@pytest.mark.parametrize("block_frames", [1000, 4096])
def test_cpp_mix_of_host_fed_chains(O, block_frames, tmp_path):
    check_mirror_host_fed(False, O, block_frames, tmp_path)


def test_cpp_mixer_add_mix(tmp_path):
    check_mirror_mixer(False, tmp_path)
