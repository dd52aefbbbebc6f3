"""A block of a mixer of Players -- per source LinearGainRamp, the Amplify whose factor a periodic_access resets every 5 ms, the converter
and the ordered sum -- as ONE call (rh_player_mix_block) and as the chain it replaces: rh_linear_gain_ramp (the sources inside a fade_in)
and rh_amplify_steps per source into rows, then rh_wide_mix_block over the rows.  Stereo sources at 44.1 kHz, a stereo mix at 48 kHz, inputs
resident, HIP events; half of the sources are inside a fade_in of 10 s, the other half have none (their chain skips that launch); every
source has a factor table with a step every 5 ms.  The two forms alternate inside one process (`--rounds` windows of `--steps` blocks each;
the median window is reported, the spread printed beside it).  One JSON line per shape: ms per block for both forms, the bytes each moves
(counted from the shapes), the fraction of the 8 TB/s roofline, the launches per block, and whether the two forms gave the same bits.

    python tools/bench_player_mix.py [--shapes 16x16384,256x65536] [--steps 50] [--rounds 5] [--general]

--general: dst 4 bytes off an 8-byte boundary, which sends the one call to the general kernel (a lane per output sample).
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
FADE_NS = 10_000_000_000


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def shape(S, N, steps, rounds, general):
    M = ((N - 1) * T + F - 1) // F  # output frames whose two taps lie in N source frames
    period = int(rh.periodic_update_samples(5_000_000, FROM, CH))  # 5 ms of the stereo stream: 441 samples
    entries = (CH * N - 1) // period + 1
    rng = np.random.default_rng(7)
    xs = [torch.from_numpy((rng.uniform(-1, 1, N * CH) / S).astype(np.float32)).cuda() for _ in range(S)]
    factors = [torch.from_numpy(rng.uniform(0.5, 1, entries).astype(np.float32)).cuda() for _ in range(S)]
    fading = [s % 2 == 0 for s in range(S)]
    dst_new = torch.empty(M * CH + 4, device="cuda")[(1 if general else 0):][: M * CH]  # (general: off the 8-byte boundary the specialised kernel wants)
    rows = torch.empty(S, N * CH, device="cuda")
    dst_old = torch.empty(M * CH, device="cuda")
    # every argument is built once: a timed block is the library's calls and nothing else of Python's
    vp, st, lib = C.c_void_p, source._stream(), _lib.lib
    play = (_lib.WideSrc * S)()  # the sources as the one call reads them ...
    arr = (_lib.WideSrc * S)()   # ... and their rows as the chain's mixer does
    ramps, gains = (C.c_uint64 * (4 * S))(), (C.c_float * (2 * S))()
    fp, fsteps = (C.c_void_p * S)(), (C.c_uint64 * (3 * S))()
    for s in range(S):
        play[s].data, play[s].channels, play[s].from_rate, play[s].phase, play[s].frames, play[s].last, play[s].gain = xs[s].data_ptr(), CH, FROM, 0, M, 0xFFFFFFFF, 1.0
        arr[s].data, arr[s].channels, arr[s].from_rate, arr[s].phase, arr[s].frames, arr[s].last, arr[s].gain = rows[s].data_ptr(), CH, FROM, 0, M, 0xFFFFFFFF, 1.0
        ramps[4 * s: 4 * s + 4] = [1 if fading[s] else 0, FADE_NS, 1000 * s, FROM]  # fade_in, 1000 s frames of it behind the source already
        gains[2 * s: 2 * s + 2] = [0.0, 1.0]
        fp[s] = factors[s].data_ptr()
        fsteps[3 * s: 3 * s + 3] = [0, period, entries]
    a_new = (vp(dst_new.data_ptr()), CH, TO, M, play, S, ramps, gains, fp, fsteps, st)
    a_ramp = [(vp(rows[s].data_ptr()), vp(xs[s].data_ptr()), N * CH, 1000 * s * CH, CH, FROM, FADE_NS, 0.0, 1.0, 0, st) for s in range(S) if fading[s]]
    a_step = [(vp(rows[s].data_ptr()), vp(rows[s].data_ptr() if fading[s] else xs[s].data_ptr()), N * CH, 0, period, vp(factors[s].data_ptr()), entries, st) for s in range(S)]
    a_mix = (vp(dst_old.data_ptr()), CH, TO, M, arr, S, st)
    f_new, f_ramp, f_step, f_mix = lib.rh_player_mix_block, lib.rh_linear_gain_ramp, lib.rh_amplify_steps, lib.rh_wide_mix_block

    def new():
        if f_new(*a_new):
            raise RuntimeError("rh_player_mix_block failed")

    def old():
        bad = 0
        for a in a_ramp:
            bad |= f_ramp(*a)
        for a in a_step:
            bad |= f_step(*a)
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
    n_fading = sum(fading)
    b_new = 4 * CH * N * S + 4 * CH * M                                   # every source frame once, the mix once
    b_old = (n_fading + S) * 2 * 4 * CH * N + S * 4 * CH * N + 4 * CH * M  # a row in and out per adapter launch; the mixer reads the rows back
    launches = -(-S // 32)
    return {"sources": S, "frames": N, "out_frames": M, "fading": n_fading, "factor_period_samples": period, "steps_per_table": entries,
            "one_call": {"ms": ms_new, "min": min(t_new), "max": max(t_new), "bytes": b_new, "GBps": b_new / ms_new / 1e6, "frac_of_8TBps": b_new / ms_new / 1e6 / 8000, "launches": launches},
            "chain": {"ms": ms_old, "min": min(t_old), "max": max(t_old), "bytes": b_old, "GBps": b_old / ms_old / 1e6, "frac_of_8TBps": b_old / ms_old / 1e6 / 8000, "launches": n_fading + S + launches},
            "speedup": ms_old / ms_new, "bytes_ratio": b_old / b_new, "bit_identical": same, "kernel": "k_player_mix" if general else "k_player_mix_stereo"}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x16384,256x65536")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--general", action="store_true")
    a = ap.parse_args()
    source._ensure()
    for sh in a.shapes.split(","):
        S, N = (int(v) for v in sh.split("x"))
        print(json.dumps(shape(S, N, a.steps, a.rounds, a.general)), flush=True)


if __name__ == "__main__":
    main()
