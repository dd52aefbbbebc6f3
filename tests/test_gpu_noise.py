"""On-device noise sources on the MI355X: NoiseBank / WhiteUniform ... Velvet (rh_noise_generate) against the numpy restatement of the
contract (tests/test_noise_cpu.py) -- bit for bit for the white kinds, blue, violet, pink and velvet, the Gaussian bit for bit against
rh_dither's GPDF noise, the integrators within 4e-5 of the f64 recurrence -- across sample indices past 2^32 and 2^40, block splits and
seeks; the reference's own unit tests (noise.rs:993-1230) on device samples; and generated noise feeding the fused mixer with no sample
uploaded."""
import numpy as np
import pytest

from test_noise_cpu import (EXACT, GAUSS_TOL, INTEGRATOR_TOL, INTEGRATORS, KINDS, bits, check_noise_chain, check_noise_follow,
                            check_noise_mixer, check_noise_trait, hash_, idx, integrator_consts, recurrence_f64, reference, same_values, u1,
                            velvet_grid)

pytestmark = pytest.mark.gpu
f32 = np.float32
N = 1 << 20


def host(t):
    import torch

    torch.cuda.synchronize()
    return t.cpu().numpy()


def set_position(bank, k0):
    st = bank.state.view(-1, 8)
    st[:, 2] = int(np.uint32(k0 & 0xFFFFFFFF).view(np.int32))
    st[:, 3] = int(np.uint32(k0 >> 32).view(np.int32))


def check_row(kind, got, seed, k0, rate=48000, density=2000, gauss=None):
    if kind == "white_gaussian":
        assert np.max(np.abs(got.astype(np.float64) - reference(kind, seed, k0, got.size))) <= GAUSS_TOL
    else:
        want = reference(kind, seed, k0, got.size, rate=rate, density=density)
        assert np.array_equal(bits(got), bits(want)), (kind, seed, k0, int(np.argmax(bits(got) != bits(want))))


def integrator_f64(kind, seed, k0, n, rate, gauss_rows=None, acc=0.0):
    leak, scale = integrator_consts(kind, rate)
    w = u1(hash_(seed, idx(k0, n))).astype(np.float64) if kind == "red" else gauss_rows.astype(np.float64)
    return recurrence_f64(w, leak, scale, acc)


@pytest.mark.parametrize("k0", [0, (1 << 32) - 5, (1 << 40) + 3])
def test_stateless_kinds_match_the_contract(rh, k0):
    kinds = EXACT + ["white_gaussian"]
    seeds = [1, 12345, (1 << 63) + 7]
    ks = [k for k in kinds for _ in seeds]
    ss = [s for _ in kinds for s in seeds]
    bank = rh.NoiseBank(ks, 48000, ss, [2000 if i % 2 else 1000 for i in range(len(ks))])
    set_position(bank, k0)
    y = host(bank.take(N))
    for r, (kind, seed) in enumerate(zip(ks, ss)):
        check_row(kind, y[r], seed, k0, density=2000 if r % 2 else 1000)
    assert np.all(bank.positions() == np.uint64(k0 + N))


def test_mixed_kinds_in_one_call_with_ld_above_n(rh):
    import torch

    n, ld = 100_003, 100_003 + 13  # rows start at every alignment
    rates = [44100, 48000, 8000, 192000, 22050, 44100, 48000, 96000, 44100]
    bank = rh.NoiseBank(KINDS, rates, list(range(40, 49)), [3000] * 9)
    out = torch.full((9, ld), 7.0, dtype=torch.float32, device="cuda")
    y = host(bank.take(n, out=out))
    full = host(out)
    assert np.all(full[:, n:] == 7.0)
    gauss = host(rh.NoiseBank(["white_gaussian"], 48000, [46]).take(n))[0]  # Brownian's white samples: WhiteGaussian of its seed
    for r, kind in enumerate(KINDS):
        if kind in INTEGRATORS:
            ref = integrator_f64(kind, 40 + r, 0, n, rates[r], gauss_rows=gauss)
            assert np.max(np.abs(y[r] - ref)) <= INTEGRATOR_TOL
        else:
            check_row(kind, y[r], 40 + r, 0, rate=rates[r], density=3000)


@pytest.mark.parametrize("algorithm,kind", [("RPDF", "white_uniform"), ("TPDF", "white_triangular"), ("GPDF", "white_gaussian"), ("HighPass", "blue")])
def test_dither_noise_is_the_noise_source(rh, algorithm, kind):
    import torch

    for seed, k0 in [(5, 0), (99, (1 << 32) - 7), ((1 << 64) - 3, (1 << 40) + 1)]:
        n = 200_003
        zeros = rh.GpuSource(torch.zeros(n, device="cuda"), 1, 48000)
        d = -host(zeros.dither(1, algorithm, seed, k0).samples)  # target_bits 1: lsb 1, out = 0 - noise
        bank = rh.NoiseBank([kind], 48000, [seed])
        set_position(bank, k0)
        y = host(bank.take(n))[0]
        assert same_values(y, d)  # (as values: -0.0 against +0.0)


def test_block_splits_and_seek(rh):
    rng = np.random.default_rng(17)
    rates = [48000] * 9
    one = rh.NoiseBank(KINDS, rates, list(range(60, 69)))
    split = rh.NoiseBank(KINDS, rates, list(range(60, 69)))
    total = 300_000
    a = host(one.take(total))
    cuts = np.sort(rng.choice(np.arange(4100, total), 11, replace=False))
    sizes = [1, 3, 4093, 3] + list(np.diff(np.concatenate([[4100], cuts, [total]])))  # one sample, a few, a tile less one, ...
    b = np.concatenate([host(split.take(int(s))) for s in sizes], axis=1)
    gauss = host(rh.NoiseBank(["white_gaussian"], 48000, [66]).take(total))[0]
    for r, kind in enumerate(KINDS):
        if kind in INTEGRATORS:
            ref = integrator_f64(kind, 60 + r, 0, total, 48000, gauss_rows=gauss)
            assert np.max(np.abs(b[r] - ref)) <= INTEGRATOR_TOL and np.max(np.abs(a[r] - ref)) <= INTEGRATOR_TOL
        else:
            assert np.array_equal(bits(a[r]), bits(b[r])), kind
    # try_seek: Ok, and only the integrators' acc moves (to 0); k stays
    before = split.states()
    split.try_seek(10**9)
    after = split.states()
    assert np.array_equal(before[:, :7], after[:, :7])
    for r, kind in enumerate(KINDS):
        assert (after[r, 7] == 0) if kind in INTEGRATORS else (after[r, 7] == before[r, 7])
    c = host(split.take(50_000))
    g2 = host(rh.NoiseBank(["white_gaussian"], 48000, [66]).take(total + 50_000))[0][total:]
    for r, kind in enumerate(KINDS):
        if kind in INTEGRATORS:
            ref = integrator_f64(kind, 60 + r, total, 50_000, 48000, gauss_rows=g2, acc=0.0)
            assert np.max(np.abs(c[r] - ref)) <= INTEGRATOR_TOL
        elif kind != "white_gaussian":
            check_row(kind, c[r], 60 + r, total)


@pytest.mark.parametrize("rate", [8000, 44100, 48000, 192000])
def test_integrators_within_bound_over_2_pow_24(rh, rate):
    n = 1 << 24
    bank = rh.NoiseBank(["red", "brownian", "white_gaussian"], rate, [12345, 777, 777])
    y = bank.take(n)
    red, brown, gauss = host(y[0]), host(y[1]), host(y[2])
    e_red = np.max(np.abs(red - integrator_f64("red", 12345, 0, n, rate)))
    e_brown = np.max(np.abs(brown - integrator_f64("brownian", 777, 0, n, rate, gauss_rows=gauss)))
    assert e_red <= INTEGRATOR_TOL and e_brown <= INTEGRATOR_TOL, (e_red, e_brown)
    # the carry on the device: one more block continues the f64 recurrence
    more = host(bank.take(100_000)[0])
    leak, scale = integrator_consts("red", rate)
    w = u1(hash_(12345, idx(0, n + 100_000))).astype(np.float64)
    assert np.max(np.abs(more - recurrence_f64(w, leak, scale)[n:])) <= INTEGRATOR_TOL


# ---- the reference's own tests (noise.rs:993-1230), on device samples at TEST_SAMPLE_RATE -------------------------------------------
RATE = 44100
MEDIUM = 1000


def samples(rh, kind, n, seed=None, density=2000):
    return host(rh.NoiseBank([kind], RATE, None if seed is None else [seed], [density]).take(n))[0].astype(f32)


def correlation(x):
    return float(np.sum((x[:-1] * x[1:]).astype(f32), dtype=f32) / f32(x.size - 1))


@pytest.mark.parametrize("kind", ["white_uniform", "white_triangular", "pink", "velvet"])
def test_bounded_generators_range(rh, kind):
    for seed in (1, 2, 3, None):
        x = samples(rh, kind, MEDIUM, seed)
        assert np.all((x >= -1.0) & (x <= 1.0))


@pytest.mark.parametrize("kind", ["white_gaussian", "blue", "violet", "brownian", "red"])
def test_unbounded_generators_finite(rh, kind):
    assert np.all(np.isfinite(samples(rh, kind, MEDIUM, 4)))


@pytest.mark.parametrize("cls", ["WhiteUniform", "WhiteTriangular", "WhiteGaussian", "Pink", "Blue", "Violet", "Brownian", "Red", "Velvet"])
def test_source_trait_properties_and_seek(rh, cls):
    src = getattr(rh, cls)(RATE)
    assert src.channels() == 1 and src.sample_rate() == RATE and src.total_duration() is None and src.current_span_len() is None
    assert src.size_hint() == ((1 << 64) - 1, None)
    x = src.take(100)
    src.try_seek(10**9)
    assert src.position() == 100 and host(x).size == 100
    assert len(src.source(64)) == 64
    seeded = getattr(rh, cls).new_with_seed(RATE, 9)
    assert seeded.seed == 9 and np.array_equal(bits(host(seeded.take(500))), bits(host(getattr(rh, cls).new_with_seed(RATE, 9).take(500))))


def test_white_uniform_distribution(rh):
    x = samples(rh, "white_uniform", MEDIUM, 8)
    assert x.min() < -0.9 and x.max() > 0.9
    assert rh.WhiteUniform(RATE).std_dev() == float(np.sqrt(f32(1) / f32(3)))


def test_triangular_distribution(rh):
    x = samples(rh, "white_triangular", MEDIUM, 8)
    assert np.count_nonzero(np.abs(x) < 0.5) > MEDIUM // 2
    assert rh.WhiteTriangular(RATE).std_dev() == float(f32(2) / np.sqrt(f32(6)))


def test_gaussian_noise_properties(rh):
    g = rh.WhiteGaussian(RATE)
    assert g.std_dev() == float(f32(0.6)) and g.mean() == 0.0
    x = samples(rh, "white_gaussian", MEDIUM, 8)
    assert np.count_nonzero(np.abs(x) <= 1.0) / x.size * 100.0 > 85.0


def test_pink_blue_violet_properties(rh):
    assert correlation(samples(rh, "pink", MEDIUM, 8)) > -0.1
    assert correlation(samples(rh, "blue", MEDIUM, 8)) < 0.1
    x = samples(rh, "violet", MEDIUM, 8)
    mean = f32(np.sum(x, dtype=f32) / f32(x.size))
    d = (x[1:] - x[:-1]).astype(f32)
    diff_var = float(np.sum(d * d, dtype=f32)) / (x.size - 1)
    sig_var = float(np.sum(((x[:-1] - mean) ** 2).astype(f32), dtype=f32)) / x.size
    assert diff_var > sig_var * 0.1


@pytest.mark.parametrize("kind", ["brownian", "red"])
def test_integrated_noise_properties(rh, kind):
    x = samples(rh, kind, RATE * 10, 8)  # 10 seconds
    assert abs(float(np.sum(x, dtype=f32)) / x.size) < 0.5
    assert correlation(x) > 0.1


def test_velvet_noise_properties(rh):
    for seed in (8, None):
        x = samples(rh, "velvet", RATE, seed)
        imp = x[x != 0]
        assert np.all((imp == 1.0) | (imp == -1.0))
        assert int(2000 * 0.75) < imp.size < int(2000 * 1.25)


def test_velvet_custom_density(rh):
    v = rh.Velvet.new_with_density(RATE, 1000, 8)
    x = host(v.take(RATE))
    assert 1000 - np.count_nonzero(x) < 200 and velvet_grid(RATE, 1000) == 45
    with pytest.raises(rh.RhError):
        rh.Velvet.new_with_density(RATE, 0, 8)


def test_deprecated_helpers(rh):
    with pytest.warns(DeprecationWarning):
        w = rh.white(RATE)
    with pytest.warns(DeprecationWarning):
        p = rh.pink(RATE)
    assert isinstance(w, rh.WhiteUniform) and isinstance(p, rh.Pink) and host(p.take(10)).size == 10


def test_unknown_kind_gives_nan(rh):
    bank = rh.NoiseBank(["white_uniform"], 48000, [1])
    bank.state.view(-1, 8)[:, 4] = 11
    assert np.isnan(host(bank.take(1001))).all()


# ---- end to end --------------------------------------------------------------------------------------------------------------------
def test_noise_bank_through_the_mixer_equals_uploaded(rh):
    import torch

    G, n = 256, N
    kinds = [KINDS[g % 9] for g in range(G)]
    bank = rh.NoiseBank(kinds, 44100, list(range(1000, 1000 + G)))
    rows = bank.take(n)
    x = host(rows)
    for g in range(0, G, 37):  # the rows are the streams' samples
        if kinds[g] in EXACT:
            check_row(kinds[g], x[g], 1000 + g, 0, rate=44100)
    p = rh.ResampleLowpassMix(44100, 48000, 1, None, "low_pass", 200, 0.5, max_sources=G, max_in_frames=n)
    p.set_sources([rows[g] for g in range(G)])  # device rows: nothing crosses PCIe
    a = host(p.run()).copy()
    p.check_status()
    p.set_sources([torch.from_numpy(x[g].copy()).cuda() for g in range(G)])  # the same samples, uploaded
    b = host(p.run()).copy()
    assert np.array_equal(bits(a), bits(b)) and np.all(np.isfinite(a))


def test_cpp_noise_trait():
    check_noise_trait(False)


@pytest.mark.parametrize("kind", KINDS)
def test_cpp_noise_host_follows_device(kind, tmp_path):
    a, b = check_noise_follow(False, kind, 44100, 31, tmp_path)
    if kind in EXACT:
        assert np.array_equal(bits(a), bits(b)) and np.array_equal(bits(a), bits(reference(kind, 31, 0, 5500, rate=44100)))
    elif kind == "white_gaussian":
        assert np.max(np.abs(a.astype(np.float64) - reference(kind, 31, 0, 5500))) <= GAUSS_TOL
    else:  # the device's scan and the host's serial loop: each within the bound of f64
        assert np.max(np.abs(a - b)) <= 2 * INTEGRATOR_TOL


@pytest.mark.parametrize("kind", EXACT)
def test_cpp_noise_chain_launches_the_source(kind, tmp_path):
    got, k1 = check_noise_chain(False, kind, tmp_path, 4096)
    want = np.concatenate([reference(kind, 77, 0, 100_000), reference(kind, 77, k1, 50_000)])
    assert np.array_equal(bits(got), bits(want))


def test_cpp_noise_mixer_is_device_resident(tmp_path):
    check_noise_mixer(False, tmp_path)  # equal to the host-fed mixer bit for bit, 0 uploaded samples
