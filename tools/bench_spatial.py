"""A block of a mixer of spatial emitters -- per source SampleRateConverter(Amplify(ChannelVolume(x))), gains retuned every 10 ms, and the
ordered sum -- as ONE launch (rh_spatial_mix_block) and as the chain it replaces: rh_channel_volume_steps per source into stereo rows,
then rh_wide_mix_block over the rows.  Mono sources at 44.1 kHz, a stereo mix at 48 kHz, inputs resident, HIP events; the two forms
alternate inside one process (`--rounds` windows of `--steps` blocks each; the median window is reported, the spread printed beside it).
One JSON line per shape: ms per block for both forms, the bytes each moves (counted from the shapes), the fraction of the 8 TB/s roofline,
the launches per block, and whether the two forms gave the same bits.

    python tools/bench_spatial.py [--shapes 16x16384,256x65536] [--steps 50] [--rounds 5] [--one-step] [--general]

--one-step: tables of ONE entry (a period that never comes): what is left of the time is not the step lookup's loads or its boundaries.
--general: dst 4 bytes off an 8-byte boundary, which sends the one launch to the general kernel (a lane per output sample).
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import rodio_amd as rh
from rodio_amd import _lib, source

FROM, TO, CH = 44100, 48000, 2
F, T = 147, 160


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def shape(S, N, steps, rounds, one_step, general):
    M = ((N - 1) * T + F - 1) // F  # output frames whose two taps lie in N source frames
    period = (1 << 40) if one_step else int(rh.periodic_update_samples(10_000_000, FROM, CH))  # 10 ms of the emitter's stereo output: 882 samples
    entries = (CH * N - 1) // period + 1
    rng = np.random.default_rng(7)
    xs = [torch.from_numpy((rng.uniform(-1, 1, N) / S).astype(np.float32)).cuda() for _ in range(S)]
    gains = [torch.from_numpy(rng.uniform(0, 1, (entries, CH)).astype(np.float32)).cuda() for _ in range(S)]
    factors = [torch.from_numpy(rng.uniform(0.5, 1, entries).astype(np.float32)).cuda() for _ in range(S)]
    dst_new = torch.empty(M * CH + 4, device="cuda")[(1 if general else 0):][: M * CH]  # (general: off the 8-byte boundary the fast kernel wants)
    rows = torch.empty(S, N * CH, device="cuda")
    dst_old = torch.empty(M * CH, device="cuda")
    # every argument is built once: a timed block is the library's calls and nothing else of Python's
    vp, st, lib = C.c_void_p, source._stream(), _lib.lib
    emit = (_lib.WideSrc * S)()  # the emitters as the one launch reads them ...
    arr = (_lib.WideSrc * S)()   # ... and their stereo rows as the chain's mixer does
    gp, fp = (C.c_void_p * S)(), (C.c_void_p * S)()
    gsteps, fsteps = (C.c_uint64 * (3 * S))(), (C.c_uint64 * (3 * S))()
    for s in range(S):
        emit[s].data, emit[s].channels, emit[s].from_rate, emit[s].phase, emit[s].frames, emit[s].last, emit[s].gain = xs[s].data_ptr(), 1, FROM, 0, M, 0xFFFFFFFF, 1.0
        arr[s].data, arr[s].channels, arr[s].from_rate, arr[s].phase, arr[s].frames, arr[s].last, arr[s].gain = rows[s].data_ptr(), CH, FROM, 0, M, 0xFFFFFFFF, 1.0
        gp[s], fp[s] = gains[s].data_ptr(), factors[s].data_ptr()
        gsteps[3 * s], gsteps[3 * s + 1], gsteps[3 * s + 2] = 0, period, entries
        fsteps[3 * s], fsteps[3 * s + 1], fsteps[3 * s + 2] = 0, period, entries
    a_new = (vp(dst_new.data_ptr()), CH, TO, M, emit, S, gp, gsteps, fp, fsteps, st)
    a_cvs = [(vp(rows[s].data_ptr()), vp(xs[s].data_ptr()), N, 1, CH, 0, period, vp(gains[s].data_ptr()), entries, 0, period, vp(factors[s].data_ptr()), entries, st) for s in range(S)]
    a_mix = (vp(dst_old.data_ptr()), CH, TO, M, arr, S, st)
    f_new, f_cvs, f_mix = lib.rh_spatial_mix_block, lib.rh_channel_volume_steps, lib.rh_wide_mix_block

    def new():
        if f_new(*a_new):
            raise RuntimeError("rh_spatial_mix_block failed")

    def old():
        bad = 0
        for a in a_cvs:
            bad |= f_cvs(*a)
        if bad | f_mix(*a_mix):
            raise RuntimeError("the chain failed")

    for _ in range(3):
        new(), old()
    torch.cuda.synchronize()
    same = bool(torch.equal(dst_new.view(torch.int32), dst_old.view(torch.int32)))
    t_new, t_old = [], []
    for _ in range(rounds):
        t_new.append(window(new, steps))
        t_old.append(window(old, steps))
    ms_new, ms_old = float(np.median(t_new)), float(np.median(t_old))
    b_new = 4 * 1 * N * S + 4 * CH * M                        # every source frame once, the mix once
    b_old = S * (4 * N + 4 * CH * N) + S * 4 * CH * N + 4 * CH * M  # per source: the frame in, the stereo row out; the mixer reads the rows back
    launches = -(-S // 32)
    return {"sources": S, "frames": N, "out_frames": M, "gain_period_samples": period, "steps_per_table": entries,
            "one_launch": {"ms": ms_new, "min": min(t_new), "max": max(t_new), "bytes": b_new, "GBps": b_new / ms_new / 1e6, "frac_of_8TBps": b_new / ms_new / 1e6 / 8000, "launches": launches},
            "chain": {"ms": ms_old, "min": min(t_old), "max": max(t_old), "bytes": b_old, "GBps": b_old / ms_old / 1e6, "frac_of_8TBps": b_old / ms_old / 1e6 / 8000, "launches": S + launches},
            "speedup": ms_old / ms_new, "bytes_ratio": b_old / b_new, "bit_identical": same, "kernel": "k_spatial_mix" if general else "k_spatial_mix_mono2"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x16384,256x65536")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--one-step", action="store_true")
    ap.add_argument("--general", action="store_true")
    a = ap.parse_args()
    source._ensure()
    for sh in a.shapes.split(","):
        S, N = (int(v) for v in sh.split("x"))
        print(json.dumps(shape(S, N, a.steps, a.rounds, a.one_step, a.general)), flush=True)


if __name__ == "__main__":
    main()
