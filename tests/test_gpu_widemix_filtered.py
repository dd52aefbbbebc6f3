"""rh_wide_mix_block_filtered: a block of a mixer of any channel count whose sources may carry a low_pass / high_pass -- k_wide_rows converts
the filtered sources into rows (the bits of rh_amplify -> rh_uniform_row), rh_biquad filters the rows batched by coefficient set with a
carried state per source, and rh_wide_mix_block sums the table with the rows in their sources' places.  The oracle is
`mixer::mixer(ch, rate)` + `add(UniformSourceIterator(src.amplify(g), ch, rate).low_pass(f, q))` (mixer.rs:58-66, blt.rs:397-492) over
continuous sources.  Mode 0: bit-exact; mode 1: the filter contract.  The block planner is the one of tests/test_gpu_widemix.py (GpuMixer's)."""
import ctypes as C
import os
from math import gcd

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

NONE = 0xFFFFFFFF


def lerp_ready(n, F, T):  # #m with floor(m F / T) <= n - 2: both taps of the lerp exist
    return 0 if n == 0 else ((n - 1) * T + F - 1) // F


def out_frames(n, F, T):  # ... plus the verbatim last frame, when an output frame lands on it (sample_rate.rs:193-200)
    if n == 0:
        return 0
    if F == T:
        return n
    c1 = lerp_ready(n, F, T)
    return c1 + (1 if c1 * F < n * T else 0)


def _kind(name):
    return {"lp": 0, "hp": 1}[name]


class Pump:
    """Sources arrive block by block (`feed` frames a pull); a block emits what every live source has both taps for.  srcs: (x, ch, rate, gain,
    filt) with filt None, ("lp" | "hp", freq, q) or ("lp" | "hp", coeffs5).  carry: every filtered source has a device state that the blocks
    hand on (False: NULL states)."""

    def __init__(self, rh, srcs, to_ch, to_rate, mode, carry=True):
        import torch

        self.rh, self.torch = rh, torch
        self.to_ch, self.to_rate, self.mode = to_ch, to_rate, mode
        self.s = []
        for x, ch, rate, gain, filt in srcs:
            g = gcd(rate, to_rate)
            co = None
            if filt is not None:
                co = np.asarray(filt[1], np.float32) if np.ndim(filt[1]) else rh.biquad_coeffs(_kind(filt[0]), filt[1], filt[2], to_rate)
            self.s.append(dict(x=x, ch=ch, rate=rate, gain=gain, F=rate // g, T=to_rate // g, n=len(x) // ch, fed=0, dev=torch.from_numpy(x).cuda() if len(x) else torch.zeros(1, device="cuda"),
                               ended=len(x) == 0, kind=None if filt is None else _kind(filt[0]), co=co, state=torch.zeros(4 * to_ch, device="cuda") if filt is not None and carry else None))
        self.m = 0

    def total(self):
        return max([out_frames(s["n"], s["F"], s["T"]) for s in self.s] + [0])

    def block(self, feeds, cap):
        from rodio_amd import _lib

        for s, f in zip(self.s, feeds):
            if not s["ended"]:
                s["fed"] = min(s["n"], s["fed"] + f)
                if s["fed"] == s["n"]:
                    s["ended"] = True
        live = [lerp_ready(s["fed"], s["F"], s["T"]) if s["F"] != s["T"] else s["fed"] for s in self.s if not s["ended"]]
        m_end = min(live) if live else self.total()
        m_end = max(self.m, min(m_end, self.m + cap))
        out = m_end - self.m
        if out == 0:
            return np.zeros(0, np.float32), not live and m_end >= self.total()
        arr = (_lib.WideSrc * len(self.s))()
        for k, s in enumerate(self.s):
            F, T = s["F"], s["T"]
            end = out_frames(s["n"], F, T) if s["ended"] else m_end
            i0 = self.m * F // T
            arr[k].frames = max(0, min(end, m_end) - self.m)
            arr[k].data = s["dev"].data_ptr() + 4 * i0 * s["ch"]
            arr[k].channels, arr[k].from_rate = s["ch"], s["rate"]
            arr[k].phase = self.m * F % T
            arr[k].last = (s["n"] - 1 - i0) if s["ended"] and s["n"] - 1 >= i0 else (0 if s["ended"] else NONE)
            arr[k].gain = s["gain"]
            if arr[k].frames and not s["ended"]:  # what the planner promises: every tap of a live source lies in what has been fed
                assert (m_end - 1) * F // T + (0 if F == T else 1) <= s["fed"] - 1
        dst = self.torch.full((out * self.to_ch,), float("nan"), device="cuda")
        filters = [None if s["kind"] is None else (s["kind"], s["co"], s["state"]) for s in self.s]
        self.rh.wide_mix_block_filtered(dst, self.to_ch, self.to_rate, out, arr, filters, self.mode)
        self.m = m_end
        return dst.cpu().numpy(), not live and m_end >= self.total()


def _run(rh, srcs, to_ch, to_rate, mode, rng, feed=(700, 1400), cap=1 << 20, carry=True):
    p = Pump(rh, srcs, to_ch, to_rate, mode, carry)
    parts = []
    for _ in range(100000):
        o, done = p.block([int(rng.integers(feed[0], feed[1] + 1)) for _ in srcs], cap)
        parts.append(o)
        if done:
            break
    else:
        raise AssertionError("the pump never finished")
    return np.concatenate(parts) if parts else np.zeros(0, np.float32)


def _oracle(srcs, to_ch, to_rate):
    from oracle import rodio_oracle as O

    mx = O.Mixer(to_ch, to_rate)
    for x, ch, rate, gain, filt in srcs:
        s = O.TestSource(x, ch, rate)
        if gain != 1.0:
            s = s.amplify(gain)
        if filt is not None:
            u = O.UniformSourceIterator(s, to_ch, to_rate)
            s = u.low_pass(filt[1], filt[2]) if filt[0] == "lp" else u.high_pass(filt[1], filt[2])
        mx.add(s)
    return mx.collect()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


FORMATS = [(6, 48000), (3, 22050), (8, 96000)]
FILTERS = [("lp", 1000, 0.5), None, ("hp", 2000, 0.5), ("lp", 1000, 0.5), ("lp", 300, 0.9), None, ("hp", 2000, 0.5)]  # interleaved classes
GAINS = [1.0, 0.5, -1.5, 0.25, 0.75, 1.0, 2.0]


def _seven(to_ch, to_rate, filters):
    """Seven sources (not a whole group of four) of seven layouts, 2 000 .. 6 000 frames; the sixth -- unfiltered, 8 kHz -- is made the one
    whose stream ends last, so that the mix has frames behind every filtered source's end."""
    rng = np.random.default_rng(4200 + to_ch)
    layouts = [(6, 44100), (2, 44100), (1, 48000), (to_ch, to_rate), (8, 96000), (4, 8000), (3, 11025)]
    srcs = []
    for k, (ch, rate) in enumerate(layouts):
        n = int(rng.integers(5000, 6001)) if k == 5 else int(rng.integers(2000, 6001))
        srcs.append((rng.uniform(-1, 1, n * ch).astype(np.float32), ch, rate, GAINS[k], filters[k]))
    return srcs


_CACHE = {}


def _case(to_ch, to_rate, filters):
    """The sources of a format and the oracle's mix of them: computed once, shared by the tests, never written to."""
    key = (to_ch, to_rate, tuple(filters))
    if key not in _CACHE:
        srcs = _seven(to_ch, to_rate, filters)
        want = _oracle(srcs, to_ch, to_rate)
        want.setflags(write=False)
        _CACHE[key] = (srcs, want)
    return _CACHE[key]


@pytest.mark.parametrize("to_ch,to_rate", FORMATS)
def test_mode_0_is_the_oracles_mixer_bit_for_bit(rh, to_ch, to_rate):
    """Blocks of 700 .. 1 400 fed frames: every source crosses several seams with its carried state and ends inside a block."""
    srcs, want = _case(to_ch, to_rate, FILTERS)
    got = _run(rh, srcs, to_ch, to_rate, 0, np.random.default_rng(1))
    assert got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want)), int(np.argmax(_bits(got) != _bits(want)))


def _contract_filters(rh, to_rate):
    """FILTERS where the contract holds at to_rate; a cutoff the contract does not cover there (low_pass(300, q 0.9) at 96 kHz: its poles
    lie at 1 - r = 0.011) is doubled until it does -- the contract is a statement about 1 - r, which grows with freq / rate."""
    out = []
    for f in FILTERS:
        while f is not None and not rh.filter_scan_ok(_kind(f[0]), f[1], f[2], to_rate):
            f = (f[0], 2 * f[1], f[2])
        out.append(f)
    return out


@pytest.mark.parametrize("to_ch,to_rate", FORMATS)
def test_mode_1_stays_within_the_filter_contract(rh, to_ch, to_rate):
    """|x| <= 1, every filter inside the contract (asserted): the contract's 1e-5 for a full-scale source scales with the peak, the converter's
    lerp is a convex combination of two samples (its output peaks where its input does), so filtered source s is within 1e-5 |gain_s| of the
    reference and the mix within the sum of those.  The length is exact, and so is every frame behind the last filtered source's end."""
    filters = _contract_filters(rh, to_rate)
    for f in filters:
        assert f is None or rh.filter_scan_ok(_kind(f[0]), f[1], f[2], to_rate)
    srcs, want = _case(to_ch, to_rate, filters)
    assert all(float(np.max(np.abs(x))) <= 1.0 for x, *_ in srcs)
    got = _run(rh, srcs, to_ch, to_rate, 1, np.random.default_rng(2))
    assert got.shape == want.shape
    bound = 1e-5 * sum(abs(g) for _, _, _, g, f in srcs if f is not None)
    err = float(np.max(np.abs(got.astype(np.float64) - want.astype(np.float64))))
    print(f"mode 1, {to_ch} ch at {to_rate} Hz: max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    tail = to_ch * max(out_frames(len(x) // ch, rate // gcd(rate, to_rate), to_rate // gcd(rate, to_rate)) for x, ch, rate, _, f in srcs if f is not None)
    assert tail < len(want)
    assert np.array_equal(_bits(got[tail:]), _bits(want[tail:]))


def test_a_filter_outside_the_contract_runs_in_reference_order_in_mode_1(rh):
    assert not rh.filter_scan_ok(0, 20, 0.5, 48000)
    rng = np.random.default_rng(43)
    srcs = [(rng.uniform(-1, 1, 3000 * 6).astype(np.float32), 6, 44100, 0.8, ("lp", 20, 0.5)), (rng.uniform(-1, 1, 2500 * 2).astype(np.float32), 2, 48000, 1.0, None),
            (rng.uniform(-1, 1, 2000).astype(np.float32), 1, 44100, 0.5, ("lp", 20, 0.5))]
    m0 = _run(rh, srcs, 6, 48000, 0, np.random.default_rng(3))
    m1 = _run(rh, srcs, 6, 48000, 1, np.random.default_rng(3))
    assert np.array_equal(_bits(m0), _bits(m1))
    assert np.array_equal(_bits(m0), _bits(_oracle(srcs, 6, 48000)))


def test_more_sources_than_a_launch_holds(rh):
    """37 sources (32 + 5), all filtered with one filter: two convert launches and two mix launches a block, one filter batch."""
    rng = np.random.default_rng(44)
    srcs = [(rng.uniform(-1, 1, int(rng.integers(1500, 3001)) * ch).astype(np.float32), ch, rate, float(np.float32(rng.uniform(0.1, 1.5))), ("lp", 1000, 0.5))
            for ch, rate in ([(6, 44100), (2, 48000), (1, 22050), (6, 48000)] * 10)[:37]]
    want = _oracle(srcs, 6, 48000)
    got = _run(rh, srcs, 6, 48000, 0, rng)
    assert got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want)), int(np.argmax(_bits(got) != _bits(want)))


def _whole_table(srcs, to_rate):
    """Every source whole and ended: ONE call gives the whole mix."""
    import torch

    from rodio_amd import _lib

    arr = (_lib.WideSrc * len(srcs))()
    keep, total = [], 0
    for k, (x, ch, rate, gain, _) in enumerate(srcs):
        g = gcd(rate, to_rate)
        d = torch.from_numpy(x).cuda()
        keep.append(d)
        arr[k].data, arr[k].channels, arr[k].from_rate, arr[k].phase, arr[k].frames, arr[k].last, arr[k].gain = d.data_ptr(), ch, rate, 0, out_frames(len(x) // ch, rate // g, to_rate // g), len(x) // ch - 1, gain
        total = max(total, arr[k].frames)
    return arr, keep, total


@pytest.mark.parametrize("to_ch", [1, 2])
def test_without_a_filtered_source_it_is_rh_wide_mix_block(rh, to_ch):
    import torch

    from rodio_amd import _lib, source

    rng = np.random.default_rng(45 + to_ch)
    srcs = [(rng.uniform(-1, 1, int(rng.integers(1000, 3000)) * ch).astype(np.float32), ch, rate, gain, None) for ch, rate, gain in [(6, 44100, 0.5), (2, 48000, 1.0), (1, 22050, -0.7), (to_ch, 48000, 1.0), (3, 11025, 2.0)]]
    arr, keep, total = _whole_table(srcs, 48000)
    a = torch.full((total * to_ch,), float("nan"), device="cuda")
    b = torch.full((total * to_ch,), float("nan"), device="cuda")
    rh.wide_mix_block_filtered(a, to_ch, 48000, total, arr, [None] * len(srcs), 1)
    _lib.check(_lib.lib.rh_wide_mix_block(C.c_void_p(b.data_ptr()), to_ch, 48000, total, arr, len(srcs), source._stream()), "rh_wide_mix_block")
    assert np.array_equal(_bits(a.cpu().numpy()), _bits(b.cpu().numpy()))
    assert not bool(torch.isnan(a).any())


def test_more_than_eight_channels_run_in_reference_order_in_mode_1(rh):
    """rh_biquad's documented fallback: the scan kernel takes 1 to 8 channels."""
    rng = np.random.default_rng(47)
    srcs = [(rng.uniform(-1, 1, 2500 * 6).astype(np.float32), 6, 44100, 0.8, ("lp", 1000, 0.5)), (rng.uniform(-1, 1, 2000 * 10).astype(np.float32), 10, 48000, 1.0, None)]
    m0 = _run(rh, srcs, 10, 48000, 0, np.random.default_rng(4))
    m1 = _run(rh, srcs, 10, 48000, 1, np.random.default_rng(4))
    assert np.array_equal(_bits(m0), _bits(m1))
    assert np.array_equal(_bits(m0), _bits(_oracle(srcs, 10, 48000)))


def test_the_state_travels_through_the_pointer(rh):
    rng = np.random.default_rng(48)
    srcs = [(rng.uniform(-1, 1, 3000 * 6).astype(np.float32), 6, 44100, 0.8, ("lp", 1000, 0.5)), (rng.uniform(-1, 1, 2800 * 2).astype(np.float32), 2, 48000, 1.0, ("hp", 2000, 0.5)),
            (rng.uniform(-1, 1, 2000).astype(np.float32), 1, 44100, 0.5, None)]
    whole = 1 << 20
    one = _run(rh, srcs, 6, 48000, 0, rng, feed=(whole, whole))
    p = Pump(rh, srcs, 6, 48000, 0)
    first, done = p.block([whole] * 3, (p.total() + 1) // 2)
    assert not done and len(first) == 6 * ((p.total() + 1) // 2)
    second, done = p.block([0] * 3, whole)
    assert done
    assert np.array_equal(_bits(np.concatenate([first, second])), _bits(one))
    # NULL states: a fresh filter every call, nothing written back -- the same block twice, and the one-block run above
    a = _run(rh, srcs, 6, 48000, 0, rng, feed=(whole, whole), carry=False)
    b = _run(rh, srcs, 6, 48000, 0, rng, feed=(whole, whole), carry=False)
    assert np.array_equal(_bits(a), _bits(b)) and np.array_equal(_bits(a), _bits(one))


def test_arguments(rh):
    import torch

    from rodio_amd import _lib, source

    source._ensure()
    x = torch.zeros(64, device="cuda")
    dst = torch.full((24,), float("nan"), device="cuda")
    scratch = torch.zeros(1024, device="cuda")
    s = (_lib.WideSrc * 1)()
    s[0].data, s[0].channels, s[0].from_rate, s[0].phase, s[0].frames, s[0].last, s[0].gain = x.data_ptr(), 2, 44100, 0, 4, NONE, 1.0
    kinds = (C.c_int32 * 1)(0)
    co = rh.biquad_coeffs(0, 1000, 0.5, 48000)
    cop = co.ctypes.data_as(_lib.f32p)
    f = _lib.lib.rh_wide_mix_block_filtered
    d, sc, nb = C.c_void_p(dst.data_ptr()), C.c_void_p(scratch.data_ptr()), scratch.numel() * 4
    assert f(d, 6, 48000, 0, s, 1, kinds, cop, None, 0, sc, nb, None) == 0  # nothing to do
    assert f(d, 6, 48000, 4, s, 1, None, cop, None, 0, sc, nb, None) == 1  # RH_ERR_INVALID: no filter table
    kinds[0] = 2
    assert f(d, 6, 48000, 4, s, 1, kinds, cop, None, 0, sc, nb, None) == 1  # a kind above 1
    kinds[0] = 0
    assert f(d, 6, 48000, 4, s, 1, kinds, None, None, 0, sc, nb, None) == 1  # a filter without coefficients
    assert f(d, 6, 48000, 4, s, 1, kinds, cop, None, 2, sc, nb, None) == 1  # a mode that does not exist
    assert f(d, 6, 48000, 4, s, 1, kinds, cop, None, 0, None, 0, None) == 1  # no rows to work in
    assert f(d, 6, 48000, 4, s, 1, kinds, cop, None, 0, sc, 64, None) == 7  # RH_ERR_CAPACITY
    s[0].frames = 5  # what rh_wide_mix_block refuses: more frames than the block
    assert f(d, 6, 48000, 4, s, 1, kinds, cop, None, 0, sc, nb, None) == 1
    s[0].frames = 4
    # (rh_biquad_coeffs computes coefficients for any frequency, as blt.rs does: there is no refusal at Nyquist to pass on)
    torch.cuda.synchronize()
    assert bool(torch.isnan(dst).all())
    need = C.c_uint64(0)
    assert _lib.lib.rh_wide_mix_filtered_scratch_bytes(6, 4, 1, C.byref(need)) == 0 and need.value == 4 * (2 * 24 + 24)
    assert f(d, 6, 48000, 4, s, 1, kinds, cop, None, 0, sc, need.value, None) == 0
    torch.cuda.synchronize()
    assert not bool(torch.isnan(dst).any())


@pytest.mark.parametrize("ch,rate,to_ch,to_rate", [(2, 44100, 6, 48000), (8, 96000, 3, 22050), (1, 48000, 6, 48000), (6, 44100, 6, 48000)])
def test_rows_are_amplify_and_uniform_row_bit_for_bit(rh, ch, rate, to_ch, to_rate):
    """k_wide_rows through the entry: one source whose filter is the identity {1,0,0,0,0} (y = x in mode 0's operation order for finite
    samples), so the block is 0.0 + the converted row -- against rh_amplify -> rh_uniform_row on the same source."""
    from rodio_amd import source

    rng = np.random.default_rng(49 + ch)
    x = rng.uniform(-1, 1, 3001 * ch).astype(np.float32)
    gain = 0.7
    srcs = [(x, ch, rate, gain, ("lp", np.float32([1, 0, 0, 0, 0])))]
    got = _run(rh, srcs, to_ch, to_rate, 0, rng, feed=(1 << 20, 1 << 20))
    row = source._uniform_row(rh.TestSource(x, ch, rate).amplify(gain), to_ch, to_rate).cpu().numpy()
    want = np.float32(0.0) + row
    assert got.shape == want.shape
    assert np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("pull_first", [6 * 2500 + 1])
def test_gpu_mixer_with_wide_filters_on_the_device(O, tmp_path, pull_first):
    """GpuMixer(6, 48000) with Options::wide_filters against the library (tests/cpp/wide_filtered_test; its CPU twin is
    tests/test_wide_filtered_cpu.py): filtered and plain sources in one-launch generations, a late join, sources ending inside blocks, the
    states carried on the device.  Every filter lies inside the contract (asserted) and |x| <= 0.25, so the mix stays within
    1e-5 * 0.25 * sum |gain| over the filtered sources of the oracle's; the length and every size_hint() are exact."""
    import test_wide_filtered_cpu as W

    import rodio_amd as rh

    for _, _, _, _, kind, freq, q in W.SPEC:
        assert kind < 0 or rh.filter_scan_ok(kind, freq, q, 48000)
    xs = W._inputs()
    assert all(float(np.max(np.abs(x))) <= 0.25 for x in xs)
    want, want_hints = W._oracle(O, xs, pull_first)
    got, hints, st = W._run(tmp_path, xs, pull_first, True, os.path.join(W.ROOT, "tests", "cpp", "wide_filtered_test"))
    assert st["chains"] == 0 and st["wide_filtered_blocks"] > 0, st
    assert got.shape == want.shape
    bound = 1e-5 * 0.25 * sum(abs(g) for _, _, g, _, kind, _, _ in W.SPEC if kind >= 0)
    err = float(np.max(np.abs(got.astype(np.float64) - want)))
    print(f"GpuMixer, wide_filters: max |got - want| = {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (err, bound)
    assert np.array_equal(hints, want_hints)
