"""A filter sweep on the device: one stereo stream of 32 Ki frames at 48 kHz whose low_pass is retuned every 5 ms (480 samples, 240
frames), and 256 such streams in one call, three ways:
    per step   one rh_biquad mode 0 launch per step with the state carried (all there was before rh_biquad_steps)
    steps m0   rh_biquad_steps mode 0: one launch, rodio's operation order
    steps m1   rh_biquad_steps mode 1: one launch, time-parallel
HIP events around `reps` repetitions launched back to back on one stream, warmed up, the three ways alternating `rounds` times (the
figure is the median of the rounds, the spread their min .. max); the outputs of the three ways are compared before anything is timed.
    python tools/bench_live_filter.py [--frames 32768] [--streams 256] [--reps 20] [--rounds 5]        (GPU box)
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rodio_amd import _lib, source

PERIOD, RATE, CH = 480, 48000, 2


def timed(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps * 1e3  # microseconds a pass


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=32768)
    ap.add_argument("--streams", type=int, default=256)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    source._ensure()
    lib, st, ck = _lib.lib, source._stream(), _lib.check
    P = lambda t, off=0: C.c_void_p(t.data_ptr() + 4 * off)
    F = a.frames
    n = F * CH
    k = (n + PERIOD - 1) // PERIOD
    freqs = [int(round(100 * 80 ** (i / max(1, k - 1)))) for i in range(k)]  # 100 Hz -> 8 kHz, geometric
    table = np.stack([source.biquad_coeffs("low_pass", f, 0.5, RATE) for f in freqs]).astype(np.float32)
    tab = torch.from_numpy(table.reshape(-1)).cuda()
    fp = PERIOD // CH
    for S in (1, a.streams):
        x = (torch.rand(S * n, device="cuda") * 2 - 1).contiguous()
        outs = [torch.zeros(S * n, device="cuda") for _ in range(3)]
        states = [torch.zeros(S * CH * 4, device="cuda") for _ in range(3)]  # zero for the pass that is compared, carried on by the timed ones

        def per_step(dst=outs[0], state=states[0]):
            # the batch layout of rh_biquad is rows back to back, so a step of every stream is one call only for S = 1; for a batch the
            # parent's way is a call per (stream, step)
            for s in range(S):
                for i, f0 in enumerate(range(0, F, fp)):
                    ck(lib.rh_biquad(P(dst, s * n + f0 * CH), P(x, s * n + f0 * CH), min(fp, F - f0), CH, 1, table[i].ctypes.data_as(_lib.f32p), P(state, s * CH * 4), 0, st), "rh_biquad")

        def steps(mode, dst):
            ck(lib.rh_biquad_steps(P(dst), P(x), F, CH, S, 0, PERIOD, P(tab), k, 0, P(states[1 + mode]), mode, st), "rh_biquad_steps")

        ways = {"per step (rh_biquad mode 0)": per_step, "rh_biquad_steps mode 0": lambda: steps(0, outs[1]), "rh_biquad_steps mode 1": lambda: steps(1, outs[2])}
        reps = {w: (max(1, a.reps // 10) if w.startswith("per step") and S > 1 else a.reps) for w in ways}
        for fn in ways.values():  # warm-up, and the results that are compared
            fn()
        torch.cuda.synchronize()
        same01 = bool(torch.equal(outs[0].view(torch.int32), outs[1].view(torch.int32)))
        d12 = float((outs[1].double() - outs[2].double()).abs().max())
        if not same01 or not d12 <= 1e-5:
            raise SystemExit(f"the three ways disagree: per step == mode 0: {same01}, |mode 0 - mode 1| = {d12:.3e}")
        t = {w: [] for w in ways}
        for _ in range(a.rounds):
            for w, fn in ways.items():
                t[w].append(timed(fn, reps[w]))
        for w in ways:
            print(json.dumps({"row": w, "streams": S, "frames": F, "steps": k, "launches": (S * ((F + fp - 1) // fp) if w.startswith("per step") else 1),
                              "us": round(statistics.median(t[w]), 1), "min_us": round(min(t[w]), 1), "max_us": round(max(t[w]), 1),
                              "mode0_bits_equal": same01, "max_abs_mode1_minus_mode0": float(f"{d12:.3e}")}), flush=True)


if __name__ == "__main__":
    main()
