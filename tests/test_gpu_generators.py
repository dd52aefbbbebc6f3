"""On-device signal generators on the MI355X: SignalGenerator / *Wave / GeneratorBank (rh_signal_generate) and Chirp (rh_chirp)
against the reference's own unit vectors and a serial f32 restatement (tests/test_generators_cpu.py), across block sizes and
seeks, and feeding the fused mixer and BASELINE config 1's chain with no sample uploaded."""
import numpy as np
import pytest

from test_generators_cpu import TAU, check_mirror_chain, check_mirror_mixer, check_mirror_trait, phase_step, seek_phase_ref, serial_phases, wave_ref

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 1 << 20
SINE_TOL = 2.4e-7  # 2 ulp at 1.0, against an f64 sin of the same f32 argument


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def check(function, got, ph):
    want = wave_ref(function, ph)
    if function == "sine":
        assert np.max(np.abs(got.astype(np.float64) - want)) <= SINE_TOL
    else:
        assert np.array_equal(bits(got), bits(want)), (function, int(np.argmax(bits(got) != bits(want))))


def test_reference_unit_vectors(rh):
    # signal_generator.rs:158-230
    assert host(rh.SignalGenerator(2000, 500.0, "square").take(8)).tolist() == [1, 1, -1, -1, 1, 1, -1, -1]
    assert host(rh.SignalGenerator(8000, 1000.0, "triangle").take(16)).tolist() == [-1, -0.5, 0, 0.5, 1, 0.5, 0, -0.5, -1, -0.5, 0, 0.5, 1, 0.5, 0, -0.5]
    assert host(rh.SignalGenerator(200, 50.0, "sawtooth").take(7)).tolist() == [0, 0.5, -1, -0.5, 0, 0.5, -1]
    s = host(rh.SignalGenerator(1000, 100.0, "sine").take(7))
    assert np.max(np.abs(s - np.array([0.0, 0.58778525, 0.95105652, 0.95105652, 0.58778525, 0.0, -0.58778554]))) <= 1e-4


@pytest.mark.parametrize("freq", [0.01, 20.0, 440.0, 5000.0, 12000.0, 20000.0, 24000.0, 48000.0, 71000.0])
def test_one_mi_samples_against_serial(rh, freq):
    ph = serial_phases(phase_step(48000, freq), 0.0, N)
    for function in ("sine", "triangle", "square", "sawtooth"):
        g = rh.SignalGenerator(48000, freq, function)
        check(function, host(g.take(N)), ph)
        end = serial_phases(phase_step(48000, freq), 0.0, N + 1)[-1]
        assert np.float32(g.phase()).view(np.uint32) == end.view(np.uint32)


def test_wave_helpers_and_trait(rh):
    for make, fn in [(rh.SineWave, "sine"), (rh.SquareWave, "square"), (rh.TriangleWave, "triangle"), (rh.SawtoothWave, "sawtooth")]:
        g = make(440.0)
        assert (g.channels(), g.sample_rate(), g.current_span_len(), g.total_duration(), g.size_hint()) == (1, 48000, None, None, ((1 << 64) - 1, None))
        check(fn, host(g.take(5000)), serial_phases(phase_step(48000, 440.0), 0.0, 5000))
    with pytest.raises(rh.RhError):
        rh.SignalGenerator(48000, 0.0, "sine")
    inf = host(rh.SignalGenerator(48000, float("inf"), "sawtooth").take(3))
    assert inf[0] == 0.0 and np.isnan(inf[1:]).all()  # the first sample is f(0), then the phase is NaN


def test_blocks_and_seek_give_the_same_bits(rh):
    freq, total = 441.7, 300_000
    one = host(rh.SignalGenerator(44100, freq, "triangle").take(total))
    g = rh.SignalGenerator(44100, freq, "triangle")
    parts, k = [], 0
    for b in [1, 63, 64, 65, 1000, 4095, 4096, 4097, 77777]:
        parts.append(host(g.take(b)))
        k += b
    parts.append(host(g.take(total - k)))
    assert np.array_equal(bits(np.concatenate(parts)), bits(one))
    # try_seek in the middle: the stream from the sought phase, block by block, is the serial recurrence from that phase
    pos = 123_456_789
    g.try_seek(pos)
    p0 = seek_phase_ref(44100, freq, pos)
    assert g.phase() == p0
    got = np.concatenate([host(g.take(b)) for b in (10, 5000, 100_000)])
    check("triangle", got, serial_phases(phase_step(44100, freq), p0, got.size))


def test_bank_mixed_functions(rh):
    rates = [44100, 48000, 8000, 192000, 22050]
    freqs = [440.0, 20.0, 3999.0, 17.25, 30000.0]
    fns = ["sine", "square", "sawtooth", "triangle", "square"]
    bank = rh.GeneratorBank(rates, freqs, fns)
    a = host(bank.take(70_001))
    b = host(bank.take(9_999))
    for r, f, fn, row_a, row_b in zip(rates, freqs, fns, a, b):
        ph = serial_phases(phase_step(r, f), 0.0, 80_000)
        check(fn, np.concatenate([row_a, row_b]), ph)


def chirp_ref(rate, f0, f1, total, first, n):
    i = np.arange(first, first + n, dtype=np.uint64)
    ratio = (i.astype(np.float64) / float(total)).astype(f32)
    freq = (f32(f0) * (f32(1.0) - ratio) + f32(f1) * ratio).astype(f32)
    t = ((i.astype(np.float64) / float(rate)).astype(f32) * TAU).astype(f32) * freq
    return np.sin(t.astype(f32).astype(np.float64))


def test_chirp(rh):
    c = rh.chirp(48000, 20.0, 20000.0, 10 * 10**9)
    assert c.size_hint() == (480_000, 480_000) and c.total_duration() == 10 * 10**9
    got = np.concatenate([host(c.take(b)) for b in (1, 4096, 200_000, 400_000)])
    assert got.size == 480_000 and c.size_hint() == (0, 0) and host(c.take(10)).size == 0
    ref = chirp_ref(48000, 20.0, 20000.0, 480_000, 0, 480_000)
    assert np.max(np.abs(got - ref)) <= SINE_TOL
    # arguments near 1e6 rad, and positions past 2^32 samples
    c = rh.chirp(48000, 19000.0, 20000.0, 200_000 * 10**9)
    c.try_seek(9 * 10**9)
    assert c.size_hint()[0] == c.total_samples - 432_000
    got = host(c.take(65536))
    assert np.max(np.abs(got - chirp_ref(48000, 19000.0, 20000.0, c.total_samples, 432_000, 65536))) <= SINE_TOL
    c.seek_sample((1 << 32) + 12345)
    got = host(c.take(65536))
    assert np.max(np.abs(got - chirp_ref(48000, 19000.0, 20000.0, c.total_samples, (1 << 32) + 12345, 65536))) <= SINE_TOL


def test_mixer_of_generated_tones_equals_host_fed(rh):
    import torch

    G, n = 256, 44100
    freqs = [float(f32(55.0 * 1.0145 ** k)) for k in range(G)]
    bank = rh.GeneratorBank(44100, freqs, ["sine", "triangle", "square", "sawtooth"] * (G // 4))
    rows = bank.take(n)
    x = host(rows)
    for k in range(G):  # the rows are the generators' samples (triangle / square / sawtooth bit for bit, sine within 2 ulp)
        fn = ["sine", "triangle", "square", "sawtooth"][k % 4]
        check(fn, x[k], serial_phases(phase_step(44100, freqs[k]), 0.0, n))
    p = rh.ResampleLowpassMix(44100, 48000, 1, None, "low_pass", 200, 0.5, max_sources=G, max_in_frames=n)
    p.set_sources([rows[k] for k in range(G)])  # device rows: nothing crosses PCIe
    a = host(p.run()).copy()
    p.check_status()
    p.set_sources([torch.from_numpy(x[k].copy()).cuda() for k in range(G)])  # the same samples, uploaded
    b = host(p.run()).copy()
    assert np.array_equal(bits(a), bits(b))


def test_baseline_config1_chain_on_device(rh, O):
    # SignalGenerator -> SampleRateConverter -> amplify, against the oracle fed with the generated samples
    g = rh.SignalGenerator(44100, 440.0, "sine")
    src = g.source(44100)
    x = host(src.samples)
    got = rh.SampleRateConverter(src, 44100, 48000, 1).amplify(0.5).collect()
    ref = O.SampleRateConverter(O.TestSource(x, 1, 44100), 44100, 48000, 1).amplify(0.5).collect()
    assert np.array_equal(bits(got), bits(ref))


def test_cpp_mirror_trait():
    check_mirror_trait(False)


@pytest.mark.parametrize("block_frames", [1000, 4096])
def test_cpp_mirror_chain_launches_the_generator(tmp_path, block_frames):
    check_mirror_chain(False, tmp_path, block_frames)  # bit for bit the serial triangle, 0 uploaded samples


def test_cpp_mirror_mixer_of_generators_is_device_resident(tmp_path):
    check_mirror_mixer(False, tmp_path)  # equal to the host-fed mixer bit for bit, 0 uploaded samples


def test_unknown_function_code_gives_nan(rh):
    import torch

    bank = rh.GeneratorBank(48000, [440.0], "sine")
    bank._fns.fill_(7)
    assert np.isnan(host(bank.take(100))).all()
