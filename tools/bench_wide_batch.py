"""The current block of B 5.1 mixers (mixer::mixer(nz!(6), 48 kHz)), each of S continuous sources at 44.1 kHz, amplified, converted, summed:
    loop:  B calls of rh_wide_mix_block on the same tables -- what a host with B mixers ran until now (a launch per 32 sources each)
    batch: rh_wide_mix_batch, one call: one table copy and one launch
Rows of every mixer resident in device memory (no two mixers share a row); HIP events around `--steps` blocks of all B mixers, `--reps`
windows each; a line reports the median window of both forms, the spread of the loop's windows (max - min over the median: what the batch
must beat it by), and whether the two forms gave the same bits.  The roofline figure counts bytes as rh_widemix.hip's header does: every
input byte once, 4 S C N per mixer in, 4 C M out.

    python tools/bench_wide_batch.py [--reps 7] [--steps 50] [--only B,S,M]
"""
import argparse
import ctypes as C
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from rodio_amd import _lib, source

SHAPES = [(B, 16, M) for M in (1024, 16384) for B in (1, 8, 64, 256)] + [(8, 128, 16384)]  # (mixers, sources per mixer, frames per block)


def measure(B, S, M, Cc=6, from_rate=44100, to_rate=48000, steps=50, reps=7):
    source._ensure()
    lib = _lib.lib
    st = source._stream()
    n_in = M * from_rate // to_rate + 8
    torch.manual_seed(B * 1000 + S)
    rows = torch.rand(B * S, n_in * Cc, device="cuda") * 2 - 1
    table = (_lib.WideSrc * (B * S))()
    for k in range(B * S):
        e = table[k]
        e.data, e.channels, e.from_rate, e.phase, e.frames, e.last, e.gain = rows[k].data_ptr(), Cc, from_rate, 0, M, 0xFFFFFFFF, float(np.float32(0.5 + 0.01 * (k % S)))
    out = {name: torch.empty(B, M * Cc, device="cuda") for name in ("loop", "batch")}
    per_mixer = [C.cast(C.byref(table, b * S * C.sizeof(_lib.WideSrc)), C.POINTER(_lib.WideSrc)) for b in range(B)]
    loop_dst = [C.c_void_p(out["loop"][b].data_ptr()) for b in range(B)]
    dsts = (C.c_void_p * B)(*[out["batch"][b].data_ptr() for b in range(B)])
    ch, rates, frames, counts = (C.c_uint32 * B)(*([Cc] * B)), (C.c_uint32 * B)(*([to_rate] * B)), (C.c_uint64 * B)(*([M] * B)), (C.c_uint32 * B)(*([S] * B))

    def loop():
        for b in range(B):
            _lib.check(lib.rh_wide_mix_block(loop_dst[b], Cc, to_rate, M, per_mixer[b], S, st), "rh_wide_mix_block")

    def batch():
        _lib.check(lib.rh_wide_mix_batch(dsts, ch, rates, frames, counts, B, table, st), "rh_wide_mix_batch")

    res = {"mixers": B, "sources": S, "block_frames": M, "channels": Cc, "steps": steps, "reps": reps}
    for name, fn in (("loop", loop), ("batch", batch)):
        for _ in range(5):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(reps):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()  # (source._stream() is torch's current stream)
            for _ in range(steps):
                fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1) / steps)
        res[f"{name}_ms"] = float(np.median(ms))
        res[f"{name}_ms_min"], res[f"{name}_ms_max"] = min(ms), max(ms)
    res["loop_spread"] = (res["loop_ms_max"] - res["loop_ms_min"]) / res["loop_ms"]
    res["speedup"] = res["loop_ms"] / res["batch_ms"]
    res["batch_faster_by_more_than_the_loops_spread"] = bool(res["batch_ms_max"] < res["loop_ms_min"] and res["speedup"] - 1.0 > res["loop_spread"])
    res["batch_ms_per_mixer"] = res["batch_ms"] / B
    res["bit_identical"] = bool(torch.equal(out["loop"].view(torch.int32), out["batch"].view(torch.int32)))
    algo = B * (4 * S * Cc * (M * from_rate // to_rate) + 4 * Cc * M)
    res["algorithmic_bytes"] = algo
    for name in ("loop", "batch"):
        res[f"{name}_frac_of_8TBps"] = algo / res[f"{name}_ms"] / 1e6 / 8000.0
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--only", default=None, help="B,S,M: one shape instead of the list")
    a = ap.parse_args()
    shapes = [tuple(int(v) for v in a.only.split(","))] if a.only else SHAPES
    for B, S, M in shapes:
        steps = max(5, a.steps // 5) if B * S >= 1024 else a.steps  # (the loop of the largest shapes: hundreds of calls a step)
        print(json.dumps(measure(B, S, M, steps=steps, reps=a.reps)), flush=True)
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
