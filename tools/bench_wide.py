"""A block of a 5.1 mixer (mixer::mixer(nz!(6), 48 kHz)): S continuous sources at 44.1 kHz, amplified, converted, summed.
    old: what a wide generation of GpuMixer ran until round 6 -- per source rh_amplify + rh_uniform_segments (one segment), then rh_mix_sum
    new: rh_wide_mix_block, one launch
Rows resident in device memory; HIP events around `steps` blocks.  Prints one JSON line per form.

    python tools/bench_wide.py [--sources 16] [--block 16384] [--channels 6] [--steps 50]

The filtered leg (--filtered K: the first K of the sources carry low_pass(1000) with a carried state, mixer.add(src, gain, filter)):
    chains: what GpuMixer runs for such a generation without Options::wide_filters -- every source a chain, rh_amplify + rh_uniform_segments
            [+ rh_biquad mode 1 with its state] + the device copy into the mixer's row, then rh_mix_sum (K = 0: rh_wide_mix_block, as today)
    entry:  rh_wide_mix_block_filtered, mode 1
`--reps` windows of `--steps` blocks each; the line reports the median window and the spread.  --root DIR takes the package (and its
library) from another checkout: the chains form of the parent commit is timed with the parent's library.  --trace-blocks N runs N blocks
of the form and nothing else, for a `rocprofv3 --kernel-trace` run of its own (launches per block = dispatches / N).

    python tools/bench_wide.py --filtered 16 --form entry [--reps 7] [--steps 200] [--root DIR] [--trace-blocks N]
"""
import argparse
import ctypes as C
import json
import sys
import os

sys.path.insert(0, sys.argv[sys.argv.index("--root") + 1] if "--root" in sys.argv else os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rodio_amd import _lib, source

U64_MAX = (1 << 64) - 1


def measure(S=16, M=16384, Cc=6, from_rate=44100, to_rate=48000, steps=50, check_frames=2048):
    """-> {"old": ms per block, "new": ms per block, "bit_identical_to_chain": bool, "oracle_ok": bool | None, "algorithmic_bytes": int}"""
    source._ensure()
    lib = _lib.lib
    n_in = M * from_rate // to_rate + 8
    rng = np.random.default_rng(1)
    host = [rng.uniform(-1, 1, n_in * Cc).astype(np.float32) for _ in range(S)]
    rows = [torch.from_numpy(h).cuda() for h in host]
    gains = [float(np.float32(0.5 + 0.01 * s)) for s in range(S)]
    st = source._stream()
    # ---- old: amplify -> uniform segment -> rows -> rh_mix_sum
    amp = [torch.empty_like(r) for r in rows]
    conv = [torch.empty(M * Cc, device="cuda") for _ in range(S)]
    dst_old = torch.empty(M * Cc, device="cuda")
    segs = []
    for s in range(S):
        g = _lib.UniformSeg()
        g.src, g.dst = amp[s].data_ptr(), conv[s].data_ptr()
        g.src_frame0, g.src_frames, g.m0, g.m1, g.span_frames = 0, n_in, 0, M, U64_MAX
        g.from_rate, g.to_rate, g.from_ch, g.to_ch, g.gain, g.reserved = from_rate, to_rate, Cc, Cc, 1.0, 0
        segs.append(g)
    ptrs = (C.c_void_p * S)(*[c.data_ptr() for c in conv])
    start = (C.c_uint64 * S)(*([0] * S))
    lens = (C.c_uint64 * S)(*([M * Cc] * S))

    def old():
        for s in range(S):
            _lib.check(lib.rh_amplify(C.c_void_p(amp[s].data_ptr()), C.c_void_p(rows[s].data_ptr()), n_in * Cc, gains[s], st), "rh_amplify")
            _lib.check(lib.rh_uniform_segments(C.byref(segs[s]), 1, st), "rh_uniform_segments")
        _lib.check(lib.rh_mix_sum(C.c_void_p(dst_old.data_ptr()), M * Cc, ptrs, start, lens, S, st), "rh_mix_sum")

    # ---- new: one launch
    dst_new = torch.empty(M * Cc, device="cuda")
    arr = (_lib.WideSrc * S)()
    for s in range(S):
        arr[s].data, arr[s].channels, arr[s].from_rate, arr[s].phase, arr[s].frames, arr[s].last, arr[s].gain = rows[s].data_ptr(), Cc, from_rate, 0, M, 0xFFFFFFFF, gains[s]

    def new():
        _lib.check(lib.rh_wide_mix_block(C.c_void_p(dst_new.data_ptr()), Cc, to_rate, M, arr, S, st), "rh_wide_mix_block")

    res = {}
    for name, fn in (("old", old), ("new", new)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()  # (source._stream() is torch's current stream)
        for _ in range(steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        res[name] = e0.elapsed_time(e1) / steps
    res["bit_identical_to_chain"] = bool(torch.equal(dst_old.view(torch.int32), dst_new.view(torch.int32)))
    res["algorithmic_bytes"] = 4 * S * Cc * (M * from_rate // to_rate) + 4 * Cc * M
    res["oracle_ok"] = None
    if check_frames:  # the first frames against the oracle's mixer (the checker: mixer::mixer(ch, rate) + add(src.amplify(g)) per sample)
        from oracle import rodio_oracle as O

        k = min(check_frames, M)
        need = k * from_rate // to_rate + 4  # frames whose taps the first k outputs read
        mx = O.Mixer(Cc, to_rate)
        for s in range(S):
            mx.add(O.TestSource(host[s][: need * Cc], Cc, from_rate).amplify(gains[s]))
        ref = mx.pull(k * Cc)
        res["oracle_ok"] = bool(len(ref) == k * Cc and np.array_equal(ref.view(np.uint32), dst_new[: k * Cc].cpu().numpy().view(np.uint32)))
    return res


def measure_filtered(form, S=16, K=16, M=16384, Cc=6, from_rate=44100, to_rate=48000, steps=200, reps=7, trace_blocks=0):
    """One block of the mixer with the first K sources filtered, `form` "chains" or "entry" (module docstring) -> (dict, the block's output)"""
    source._ensure()
    lib = _lib.lib
    n_in = M * from_rate // to_rate + 8
    rng = np.random.default_rng(1)
    rows = [torch.from_numpy(rng.uniform(-1, 1, n_in * Cc).astype(np.float32)).cuda() for _ in range(S)]
    gains = [float(np.float32(0.5 + 0.01 * s)) for s in range(S)]
    st = source._stream()
    co = np.zeros(5, np.float32)
    _lib.check(lib.rh_biquad_coeffs(0, 1000, 0.5, to_rate, co.ctypes.data_as(_lib.f32p)), "rh_biquad_coeffs")
    states = [torch.zeros(4 * Cc, device="cuda") for _ in range(K)]
    dst = torch.empty(M * Cc, device="cuda")
    arr = (_lib.WideSrc * S)()
    for s in range(S):
        arr[s].data, arr[s].channels, arr[s].from_rate, arr[s].phase, arr[s].frames, arr[s].last, arr[s].gain = rows[s].data_ptr(), Cc, from_rate, 0, M, 0xFFFFFFFF, gains[s]
    if form == "entry":
        kinds = (C.c_int32 * S)(*([0] * K + [-1] * (S - K)))
        coeffs = np.tile(co, (S, 1))
        sp = (C.c_void_p * S)(*([x.data_ptr() for x in states] + [None] * (S - K)))
        need = C.c_uint64(0)
        _lib.check(lib.rh_wide_mix_filtered_scratch_bytes(Cc, M, K, C.byref(need)), "rh_wide_mix_filtered_scratch_bytes")
        scratch = torch.empty(max(need.value // 4, 4), device="cuda")

        def block():
            _lib.check(lib.rh_wide_mix_block_filtered(C.c_void_p(dst.data_ptr()), Cc, to_rate, M, arr, S, kinds, coeffs.ctypes.data_as(_lib.f32p), sp, 1, C.c_void_p(scratch.data_ptr()),
                                                      scratch.numel() * 4, st), "rh_wide_mix_block_filtered")
    elif K == 0:
        def block():
            _lib.check(lib.rh_wide_mix_block(C.c_void_p(dst.data_ptr()), Cc, to_rate, M, arr, S, st), "rh_wide_mix_block")
    else:
        amp = [torch.empty_like(r) for r in rows]
        conv = [torch.empty(M * Cc, device="cuda") for _ in range(S)]
        filt = [torch.empty(M * Cc, device="cuda") for _ in range(K)]
        mrow = [torch.empty(M * Cc, device="cuda") for _ in range(S)]
        segs = []
        for s in range(S):
            g = _lib.UniformSeg()
            g.src, g.dst = amp[s].data_ptr(), conv[s].data_ptr()
            g.src_frame0, g.src_frames, g.m0, g.m1, g.span_frames = 0, n_in, 0, M, U64_MAX
            g.from_rate, g.to_rate, g.from_ch, g.to_ch, g.gain, g.reserved = from_rate, to_rate, Cc, Cc, 1.0, 0
            segs.append(g)
        ptrs = (C.c_void_p * S)(*[c.data_ptr() for c in mrow])
        start = (C.c_uint64 * S)(*([0] * S))
        lens = (C.c_uint64 * S)(*([M * Cc] * S))
        cop = co.ctypes.data_as(_lib.f32p)

        def block():
            for s in range(S):
                _lib.check(lib.rh_amplify(C.c_void_p(amp[s].data_ptr()), C.c_void_p(rows[s].data_ptr()), n_in * Cc, gains[s], st), "rh_amplify")
                _lib.check(lib.rh_uniform_segments(C.byref(segs[s]), 1, st), "rh_uniform_segments")
                last = conv[s]
                if s < K:
                    _lib.check(lib.rh_biquad(C.c_void_p(filt[s].data_ptr()), C.c_void_p(conv[s].data_ptr()), M, Cc, 1, cop, C.c_void_p(states[s].data_ptr()), 1, st), "rh_biquad")
                    last = filt[s]
                _lib.check(lib.rh_memcpy_d2d(C.c_void_p(mrow[s].data_ptr()), C.c_void_p(last.data_ptr()), M * Cc * 4, st), "rh_memcpy_d2d")
            _lib.check(lib.rh_mix_sum(C.c_void_p(dst.data_ptr()), M * Cc, ptrs, start, lens, S, st), "rh_mix_sum")

    if trace_blocks:
        for _ in range(trace_blocks):
            block()
        torch.cuda.synchronize()
        return {"form": form, "filtered": K, "sources": S, "trace_blocks": trace_blocks}, None
    for _ in range(20):
        block()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            block()
        e1.record()
        torch.cuda.synchronize()
        ms.append(e0.elapsed_time(e1) / steps)
    for x in states:  # the output of ONE block from fresh states, for the comparison between the forms
        x.zero_()
    block()
    torch.cuda.synchronize()
    return {"form": form, "filtered": K, "sources": S, "channels": Cc, "block_frames": M, "ms_per_block_median": float(np.median(ms)), "ms_per_block_min": min(ms), "ms_per_block_max": max(ms),
            "reps": reps, "steps": steps, "library": _lib.LIB_PATH}, dst.cpu().numpy()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--filtered", type=int, default=None, help="the filtered leg: this many of the sources carry low_pass(1000)")
    ap.add_argument("--form", choices=["chains", "entry", "both"], default="both")
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--root", default=None, help="take rodio_amd (and its library) from this checkout")
    ap.add_argument("--trace-blocks", type=int, default=0)
    ap.add_argument("--sources", type=int, default=16)
    ap.add_argument("--block", type=int, default=16384, help="output frames per block")
    ap.add_argument("--channels", type=int, default=6)
    ap.add_argument("--from-rate", type=int, default=44100)
    ap.add_argument("--to-rate", type=int, default=48000)
    ap.add_argument("--steps", type=int, default=50)
    a = ap.parse_args()
    S, M, Cc = a.sources, a.block, a.channels
    if a.filtered is not None:
        outs = {}
        for form in (["chains", "entry"] if a.form == "both" else [a.form]):
            res, outs[form] = measure_filtered(form, S, a.filtered, M, Cc, a.from_rate, a.to_rate, a.steps, a.reps, a.trace_blocks)
            if len(outs) == 2 and outs["chains"] is not None:
                res["max_abs_diff_to_chains"] = float(np.max(np.abs(outs["entry"].astype(np.float64) - outs["chains"])))
            print(json.dumps(res))
        return
    res = measure(S, M, Cc, a.from_rate, a.to_rate, a.steps)
    algo = res["algorithmic_bytes"]
    for name in ("old", "new"):
        ms = res[name]
        print(json.dumps({"form": name, "sources": S, "channels": Cc, "block_frames": M, "ms_per_block": ms, "launches_per_block": (2 * S + (S + 31) // 32) if name == "old" else (S + 31) // 32,
                          "algorithmic_bytes": algo, "GBps": algo / ms / 1e6, "frac_of_8TBps": algo / ms / 1e6 / 8000.0, "bit_identical_to_old": res["bit_identical_to_chain"], "oracle_ok": res["oracle_ok"]}))


if __name__ == "__main__":
    main()
