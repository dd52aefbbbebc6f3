"""k_rlm_sblk (rh_pipeline_sblk.hip): a block of a stream on the summed state in one launch -- the sum over the sources, the conversion and
the filter.  Its existing tests run S = 7 sources on the instances that blocks of <= 70 000 frames pick; these pin every instance, wrap the
loader rings (ceil(S / 8) > NS sources per wave), run the ticketed grid, walk the host gate's edges (sblk_try) and change paths inside one
stream.  Every case counts the blocks the kernel took (rh_rlm_stream_one_launch_blocks) and compares with three references: the oracle's
one-pass mix, an f64 evaluation of the filter on the (bit-exact) converted sources, and the same stream with RH_NO_SBLK=1."""
import ctypes as C

import numpy as np
import pytest
from conftest import knobs
from test_gpu_mix_first import _oracle, rnd

pytestmark = pytest.mark.gpu
TOL = 1e-5
NOISE = 2e-6  # |kernel - two launches| and |kernel - truth| beyond the oracle's own distance from it

# (R, C, KV, NS) of k_rlm_sblk's instances, as kInst lists them: a window of KV KiB of every source's row, NS ring stages per loader wave
INST = {"st1": (3, 2, 1, 12), "st2": (5, 2, 2, 6), "st3": (7, 2, 3, 4), "st4": (9, 2, 4, 3), "mo1": (5, 1, 1, 12), "mo2": (9, 1, 2, 6)}


def _wd(inst):  # frames of a window, and the largest stride of the windows (windows overlap by 4 frames)
    _, ch, kv, _ = INST[inst]
    wd = kv * 1024 // (4 * ch)
    return wd, wd - 4


@pytest.fixture(scope="module")
def G(rh):
    import torch

    assert torch.cuda.is_available()
    rh.init(0)
    return rh


@pytest.fixture(scope="module")
def cus():
    import torch

    return torch.cuda.get_device_properties(0).multi_processor_count


def _gains(S, seed, zero=True):
    """Distinct gains of either sign, |g| in [0.45, 1.3]; source 1 silent (zero=True); source S - 2 negative."""
    rng = np.random.default_rng(seed)
    g = rng.permutation(np.linspace(0.45, 1.3, S)).astype(np.float32)
    if S >= 2:
        g[S - 2] = -g[S - 2]
    if zero and S >= 3:
        g[1] = 0.0
    return g


def _case(S, ch, frm, to, filt, freq, sched, seed, ns=None, zero=True):
    """sched: where every block's rows end -- an int is an input frame, ("+", n) is n frames behind the end of the block before (the rows
    also hold the frames the stream kept).  The last entry is the end: every source has ended there.  ns: each source's length (default: all
    end with the last block)."""
    gains = _gains(S, seed, zero)
    amp = 0.98 / float(np.sum(np.abs(gains)))  # sum_s |g_s| amp_s <= 1
    N = max(ns) if ns else None
    xs = None
    if ns is not None:
        xs = [rnd(seed * 1000 + s, ch * n, amp) for s, n in enumerate(ns)]
    return dict(S=S, ch=ch, frm=frm, to=to, filt=filt, freq=freq, sched=sched, gains=gains, amp=amp, ns=ns, N=N, xs=xs, seed=seed)


def _ends(sched):
    his, hi = [], 0
    for e in sched:
        hi = e if isinstance(e, int) else hi + e[1]
        his.append(hi)
    return his


def _resolve(c):
    """Input frames of the stream: the schedule's own end when the sources' lengths were not given."""
    if c["xs"] is None:
        end = _ends(c["sched"])[-1]
        c["N"] = end
        c["ns"] = [end] * c["S"]
        c["xs"] = [rnd(c["seed"] * 1000 + s, c["ch"] * end, c["amp"]) for s in range(c["S"])]
    return c


def _stream(G, c, exclusive=True, overlap=False, env=None):
    """One stream through rh_rlm_stream_block_v on resident rows read at `row + consumed`.  Returns the output, the block count,
    rh_rlm_stream_one_launch_blocks, rh_rlm_stream_overlapped_blocks, stream_stats() and geometry()["n_tiles"] after every block."""
    import contextlib

    import torch
    from rodio_amd import _lib

    lib = _lib.lib
    c = _resolve(c)
    S, ch, N, ns = c["S"], c["ch"], c["N"], c["ns"]
    if "dev" not in c:  # rows padded to the longest: a pointer past a source's end still lies inside its allocation
        rows = np.zeros((S, ch * N), np.float32)
        for s, x in enumerate(c["xs"]):
            rows[s, : len(x)] = x
        c["dev"] = torch.from_numpy(rows).cuda()
    data = c["dev"]
    mo = C.c_uint64(0)
    _lib.check(lib.rh_resample_out_frames(N, c["frm"], c["to"], ch, 0, C.byref(mo)), "rh_resample_out_frames")
    M = mo.value
    his = _ends(c["sched"])
    assert his[-1] == N and all(b > a for a, b in zip([0] + his, his)), his
    biggest = max(b - a for a, b in zip([0] + his, his))  # (+ the frames a block keeps for the next: far fewer than 4096)
    with knobs(**env) if env else contextlib.nullcontext():
        p = G.ResampleLowpassMix(c["frm"], c["to"], ch, None, c["filt"], c["freq"], 0.5, max_sources=S, max_in_frames=biggest + 4096)
        if not exclusive:
            p.set_exclusive(False)
        p.set_gains(c["gains"])
        p.stream_begin(keep_history=True)
        _lib.check(lib.rh_rlm_stream_overlap(p._h, 1 if overlap else 0), "rh_rlm_stream_overlap")
        out = torch.zeros(ch * M + 4096, device="cuda", dtype=torch.float32)
        g0 = m = 0
        tiles = []
        for hi in his:
            ptrs = (C.c_void_p * S)(*[data[s].data_ptr() + g0 * 4 * ch for s in range(S)])
            avail = (C.c_uint64 * S)(*[max(0, min(hi, n) - g0) for n in ns])
            ended = (C.c_uint8 * S)(*[1 if hi >= n else 0 for n in ns])
            o, k = C.c_uint64(0), C.c_uint64(0)
            _lib.check(lib.rh_rlm_stream_block_v(p._h, ptrs, avail, ended, S, C.c_void_p(out.data_ptr() + m * 4 * ch), M + 512 - m, C.byref(o), C.byref(k), None),
                       "rh_rlm_stream_block_v")
            m += o.value
            g0 += k.value
            tiles.append(p.geometry()["n_tiles"])
        p.check_status()
        one, ovl = C.c_uint32(0), C.c_uint32(0)
        _lib.check(lib.rh_rlm_stream_one_launch_blocks(p._h, C.byref(one)), "rh_rlm_stream_one_launch_blocks")
        _lib.check(lib.rh_rlm_stream_overlapped_blocks(p._h, C.byref(ovl)), "rh_rlm_stream_overlapped_blocks")
        res = out[: ch * m].cpu().numpy()
        stats = p.stream_stats()
        p.close()
    return dict(out=res, blocks=len(his), one=one.value, ovl=ovl.value, stats=stats, tiles=tiles)


def _converted(O, c):
    """Every source as the kernel reads it: UniformSourceIterator(TestSource(x_s).amplify(g_s)), f64 (the converter is bit-exact)."""
    if "conv" not in c:
        c["conv"] = [O.UniformSourceIterator(O.TestSource(x, c["ch"], c["frm"]).amplify(float(g)), c["ch"], c["to"]).collect().astype(np.float64).reshape(-1, c["ch"])
                     for x, g in zip(c["xs"], c["gains"])]
    return c["conv"]


def _filtered(O, c):
    """Every converted source through the filter in f64 (scipy.signal.lfilter on the oracle's f32 coefficients): each source's own filter, as
    the oracle's Mixer adds them (a source that ends takes its filter's ring-down with it)."""
    if "filt64" not in c:
        from scipy.signal import lfilter

        co = O.blt_coeffs(c["filt"], c["freq"], 0.5, c["to"]).astype(np.float64)
        c["filt64"] = [lfilter(co[:3], [1.0, co[3], co[4]], r, axis=0) for r in _converted(O, c)]
    return c["filt64"]


def _truth(O, c):
    """f64: the sum over the sources of the filtered converted sources."""
    ys = _filtered(O, c)
    acc = np.zeros((max(len(y) for y in ys), c["ch"]))
    for y in ys:
        acc[: len(y)] += y
    return acc.reshape(-1)


def _ref(O, c):
    key = ("sblk", c["S"], c["ch"], c["frm"], c["to"], c["filt"], c["freq"], c["seed"], tuple(c["ns"]))
    return _oracle(O, c["xs"], c["frm"], c["to"], None, c["filt"], c["freq"], c["gains"], c["ch"], key=key)


def _check(G, O, c, one, exclusive=True, env=None, overlap=True, ovl=None, stats=None, tiles=None):
    """The stream without and with rh_rlm_stream_overlap, and with RH_NO_SBLK=1, against the oracle and the f64 truth.  one: the blocks the kernel
    must take; ovl: the blocks that must start without a barrier behind the block in front (None: not checked); stats: stream_stats() (None: every
    block on the summed state); tiles(list of n_tiles): a check of the grids."""
    a = _stream(G, c, exclusive, False, env)
    nb = a["blocks"]
    assert a["one"] == one, ("blocks on k_rlm_sblk", a["one"], one, a["tiles"])
    assert a["stats"] == (stats if stats is not None else (nb, 0, 0)), a["stats"]
    if tiles is not None:
        tiles(a["tiles"])
    ref = _ref(O, c)
    tru = _truth(O, c)
    assert len(a["out"]) == len(ref) == len(tru), (len(a["out"]), len(ref), len(tru))
    e_ref = float(np.max(np.abs(a["out"] - ref)))
    e_gpu, e_or = float(np.max(np.abs(a["out"] - tru))), float(np.max(np.abs(ref - tru)))
    assert e_ref <= TOL, ("|gpu - oracle|", e_ref)
    assert e_gpu <= e_or + NOISE, ("|gpu - f64| vs |oracle - f64|", e_gpu, e_or)
    if overlap:
        b = _stream(G, c, exclusive, True, env)
        assert b["one"] == one and b["stats"] == a["stats"], (b["one"], b["stats"])
        assert np.array_equal(a["out"], b["out"]), float(np.max(np.abs(a["out"] - b["out"])))  # side by side: the same bits
        if ovl is not None:
            assert b["ovl"] == ovl, ("blocks started beside the block in front", b["ovl"], ovl, b["tiles"])
    r = _stream(G, c, exclusive, False, dict(env or {}, RH_NO_SBLK="1"))
    assert r["one"] == 0 and r["stats"] == a["stats"], (r["one"], r["stats"])
    e_two = float(np.max(np.abs(a["out"] - r["out"])))
    assert e_two <= NOISE, ("|kernel - two launches|", e_two)
    print(f"[sblk S={c['S']} C={c['ch']} {c['frm']}->{c['to']} {c['filt']}({c['freq']}) {env or ''}] blocks {nb} one-launch {a['one']} tiles {a['tiles']} "
          f"|gpu-oracle| {e_ref:.2e} |gpu-f64| {e_gpu:.2e} |oracle-f64| {e_or:.2e} |kernel-two launches| {e_two:.2e}")
    return a


def _mid(inst):
    """A block in the middle of a stream: >= 16 tiles, and enough frames to stay on the summed state (>= the per-source kernel's look-back)."""
    _, pm = _wd(inst)
    return max(16 * pm, 6000)


def _tiles(first, last):
    """The grid check of a stream: tiles of its first and of its last block (an int, or a (lo, hi) range)."""
    def check(t):
        for v, want in ((t[0], first), (t[-1], last)):
            assert (v == want) if isinstance(want, int) else (want[0] <= v <= want[1]), (t, first, last)
    return check


# ---- A. every instance, source counts that wrap the loader rings, one tile / a partial last tile / >= 16 tiles ----------------------------------
def _a_cases():
    out = []
    big = (16, 256)
    for inst, (_, ch, kv, ns) in INST.items():
        wd, pm = _wd(inst)
        vec = 4 // ch  # frames of a 16-byte vector: every block whole vectors (the gate)
        mid = _mid(inst)
        up, down = (44100, 48000), (48000, 44100)
        # wrap: ceil(S / 8) = NS + 1 > NS; three blocks of >= 16 tiles (partial last tiles), then a last block of one tile
        out.append((inst, 8 * ns + 1, up if kv % 2 else down, ("low_pass", 200), [mid + 8 * vec, ("+", mid + 22 * vec), ("+", mid + 36 * vec), ("+", wd // 2)], big, 1))
        # S = 512: 64 sources per wave (64 / NS ring wraps); >= 16 tiles, then one tile
        out.append((inst, 512, down if kv % 2 else up, ("high_pass", 1000), [mid + 6 * vec, ("+", wd // 2)], big, 1))
        # the rings exactly full (NS sources per wave); a last block of a few tiles
        out.append((inst, 8 * ns, up, ("high_pass", 1000), [mid + 2 * vec, ("+", 2 * pm + 40)], big, (3, 4)))
        # few sources: a stream of one block of one tile (the stream's first block: fewer than two frames in front of it)
        out.append((inst, 2 if inst in ("st1", "st4", "mo2") else 9, down, ("low_pass", 200), [wd - 24], 1, 1))
        odd = {"st2": 9, "st3": 21, "mo2": 37}.get(inst)  # an odd count in the middle: the last wave's share is short
        if odd:
            out.append((inst, odd, up, ("low_pass", 200), [mid + 4 * vec, ("+", 3 * pm + 8)], big, (4, 5)))
    return out


A_CASES = _a_cases()


@pytest.mark.parametrize("inst,S,rates,filt,sched,t0,t1", A_CASES,
                         ids=[f"{c[0]}-S{c[1]}-{c[2][0]}to{c[2][1]}-{c[3][0]}{c[3][1]}-{len(c[4])}blk" for c in A_CASES])
def test_every_instance_and_source_count(G, O, inst, S, rates, filt, sched, t0, t1):
    """RH_SBLK_KV pins the instance: every block of the stream is the kernel's, so the one-launch count proves the pinned instance ran."""
    _, ch, kv, _ = INST[inst]
    c = _case(S, ch, rates[0], rates[1], filt[0], filt[1], sched, seed=100 + S + 7 * kv + ch)
    _check(G, O, c, one=len(sched), env={"RH_SBLK_KV": str(kv)}, tiles=_tiles(t0, t1))
    if S == 512:  # every source matters: dropping any one changes the exact mix by more than 10 x the tolerance (a lost source cannot hide)
        for s, (y, g) in enumerate(zip(_filtered(O, c), c["gains"])):
            if g != 0.0:
                assert float(np.max(np.abs(y))) > 10 * TOL, (s, g)


@pytest.mark.parametrize("S", [1, 513])
def test_source_counts_outside_the_kernel(G, O, S):
    """S = 1 never runs on the summed state; S = 513 is more than 8 waves of 64 sources: both fall back, with the right output."""
    c = _case(S, 2, 44100, 48000, "low_pass", 200, [6000, ("+", 6400), ("+", 900)], seed=300 + S)
    _check(G, O, c, one=0, overlap=False, stats=(0, 3, 0) if S == 1 else None)


# ---- B. grids: ticketed (exclusive(0), or more tiles than the chip holds at once), direct, and too many tiles ---------------------------------
def test_ticketed_blocks_under_exclusive_0(G, O):
    """rh_rlm_set_exclusive(0): tiles by ticket from the counters the other fused kernels use, the grid rounded to 8 -- block after block.  A
    block launched beside the block in front needs a direct grid, so none is, though the overlap was asked for."""
    c = _case(17, 2, 44100, 48000, "low_pass", 200, [7000, ("+", 6004), ("+", 9000), ("+", 4100), ("+", 800)], seed=401)
    _check(G, O, c, one=5, exclusive=False, ovl=0)


def test_ticketed_and_direct_blocks_alternate(G, O, cus):
    """exclusive(1), KV 1: blocks of 5 x .. 8 x the CUs in tiles (not a multiple of 8) are ticketed whatever the occupancy, blocks of <= CUs tiles
    direct.  Only a direct block behind a direct block starts beside it: of big, small, big, small, small exactly the last does."""
    _, pm = _wd("st1")
    big = (5 * cus + 3) * pm - 40  # 5 CUs + 3 tiles (the reach lies up to ~50 frames short of the rows' end)
    small = 50 * pm
    c = _case(9, 2, 44100, 48000, "low_pass", 200, [big, ("+", small), ("+", big), ("+", small), ("+", small)], seed=402)

    def grids(t):
        assert all(5 * cus < t[k] <= 8 * cus and t[k] % 8 != 0 for k in (0, 2)), t
        assert all(16 <= t[k] <= cus for k in (1, 3, 4)), t

    _check(G, O, c, one=5, env={"RH_SBLK_KV": "1"}, ovl=1, tiles=grids)


def test_too_many_tiles_fall_back(G, O, cus):
    """Well over 8 x 5 x CUs tiles (more than any occupancy lets the ticketed grid hold): the two-launch form; the kernel takes the next block."""
    _, pm = _wd("st1")
    c = _case(2, 2, 44100, 48000, "low_pass", 200, [(8 * 5 * cus + 300) * pm, ("+", 30 * pm)], seed=403)
    _check(G, O, c, one=1, env={"RH_SBLK_KV": "1"}, overlap=False, tiles=_tiles((1, 1 << 30), (30, 32)))


# ---- C. the ratio and filter edges of the gate ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("frm,to,one", [(96000, 64000, 2), (96000, 63990, 0)], ids=["2F=3T", "2F>3T"])
def test_the_downsampling_bound(G, O, frm, to, one):
    """2F <= 3T: the two frames the filter looks back at start at most 3 input frames in front of a frame's first tap."""
    c = _case(9, 2, frm, to, "low_pass", 200, [8000, ("+", 2000)], seed=501)
    _check(G, O, c, one=one)


# stereo instances: (frm -> 48 kHz) just inside ceil(Wd T / F) + 3 <= 64 R, and just outside
BOUND = {"st1": (32600, 32400), "st2": (38800, 38700), "st3": (41450, 41400), "st4": (42900, 42850)}


@pytest.mark.parametrize("inst", list(BOUND))
@pytest.mark.parametrize("inside", [True, False], ids=["inside", "outside"])
def test_the_frames_per_window_bound(G, O, inst, inside):
    """The output frames of a window must fit 64 runs of R frames: a rate pair just inside the bound runs on the pinned instance, one just
    outside is refused by it."""
    R, ch, kv, _ = INST[inst]
    wd, _ = _wd(inst)
    frm = BOUND[inst][0 if inside else 1]
    need = -(-wd * 48000 // frm) + 3  # ceil(Wd T / F) + 3
    assert need == (64 * R if inside else 64 * R + 1), (need, R)
    c = _case(9, 2, frm, 48000, "low_pass", 200, [_mid(inst) + 10, ("+", wd - 20)], seed=510 + kv)
    _check(G, O, c, one=2 if inside else 0, env={"RH_SBLK_KV": str(kv)})


@pytest.mark.parametrize("filt,freq", [("low_pass", 100), ("high_pass", 600), ("low_pass", 4000)])
def test_filters_across_the_contract(G, O, filt, freq):
    """low_pass(100) at 48 kHz on KV 1: the longest look-back in tiles (J ~ 21 of the gate's 32); high_pass(600); low_pass(4000), J = 1."""
    c = _case(16, 2, 44100, 48000, filt, freq, [7000, ("+", 7002), ("+", 6400), ("+", 3000)], seed=520 + freq)
    _check(G, O, c, one=4, env={"RH_SBLK_KV": "1"})


# ---- D. path changes inside one stream ----------------------------------------------------------------------------------------------------
def test_blocks_the_kernel_refuses_inside_a_stream(G, O):
    """An odd number of stereo frames is not whole vectors: that block runs as two launches on the summed state, the next on the kernel again,
    and a chain of blocks started beside each other starts over behind it (blocks 3 and 6 of 0 .. 6 start beside the block in front)."""
    sched = [6000, ("+", 6001), ("+", 6399), ("+", 7000), ("+", 5001), ("+", 6001), ("+", 6000)]  # blocks 1 and 4: an odd count
    c = _case(8, 2, 48000, 44100, "high_pass", 1000, sched, seed=601)
    _check(G, O, c, one=5, ovl=2)


def test_a_source_ends_after_kernel_blocks(G, O):
    """keep_history: two kernel blocks, then a source ends -- that block recovers the per-source states from the block before and runs with one
    state per source; once the source has given everything the stream is back on the summed state, on the kernel, without it."""
    S, N = 9, 60000
    ns = [N] * S
    ns[3] = 25000
    c = _case(S, 2, 44100, 48000, "low_pass", 200, [10000, 20000, 30000, 40000, 50000, N], seed=602, ns=ns)
    _check(G, O, c, one=5, stats=(5, 1, 1))
