"""A block of a mixer of CLIPS ON A TIMELINE -- sound.amplify(g).take_duration(len)[.set_filter_fadeout()].delay(at), each sound 100 000
stereo frames at 44.1 kHz, a stereo mix at 48 kHz -- three ways in one process, inputs resident, HIP events, warmed, per block:

  (a) entry   rh_clip_mix_block over the resident sounds: ceil(S / 32) launches
  (b) chain   what it replaces on the device, per clip and per block over the stretch of the clip's stream that the block's converter
              chains span: rh_amplify, rh_take_duration (clips with a take), rh_delay into a row, rh_uniform_row with span_len = the row's
              length into a row of the mix's format, then rh_wide_mix_block over the rows
  (c) floor   rh_wide_mix_block over the rows (b) converted, alone: the sum without delay, gain, fade and converter

Every clip has a delay, a cursor and a gain of its own; every block crosses a grid line of its clips (a whole chain emits 17833 frames);
every eighth clip is still in its delay at the block's first frame and every sixteenth for the whole block.  --fade: which clips carry the
fade-out (half: every other one; none; all) -- clips without it have no take either (a SamplesBuffer behind a delay: rule G all the same).
The three alternate (`--rounds` windows of `--steps` blocks each; the median window is reported with the fastest and the slowest beside
it).  The entry's block and the chain's are compared as integers before anything is timed, and a
difference ends the run.  One JSON line per shape; the launches per block and the fraction of the 8 TB/s roofline on (a)'s algorithmic bytes -- every sample
of a sound the block reaches once, the mix written once -- are in it.

    python tools/bench_clip_mix.py [--shapes 16x16384,256x65536] [--fade half] [--steps 50] [--rounds 5]
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
FRAMES = 100000  # of a sound
CHAIN = 32768    # samples
M_CHAIN = 17833  # output frames of a whole chain
DPS = 10**9 // (FROM * CH)


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def shape(S, M, fade, steps, rounds):
    vp, st, lib = C.c_void_p, source._stream(), _lib.lib
    rng = np.random.default_rng(7)
    N = FRAMES * CH
    xs = [torch.from_numpy(rng.uniform(-1, 1, N).astype(np.float32)).cuda() for _ in range(S)]
    srcs, clips = (_lib.WideSrc * S)(), (C.c_uint64 * (rh.source.CLIP_WORDS * S))()
    arr_b, keep, chain_calls = (_lib.WideSrc * S)(), [], []
    got, n_taken, ended = C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
    bytes_a, faded = 4 * CH * M, 0
    for s in range(S):
        fading = fade == "all" or (fade == "half" and s % 2 == 0)
        faded += fading
        if s % 16 == 15:
            Z = 2 * 200000        # the whole block lies in the delay
        elif s % 8 == 7:
            Z = 2 * (30000 + 1000 * (s % 5))  # the sound starts inside the block
        else:
            Z = 2 * (1000 + 37 * s)
        done = 20000 if s % 8 == 7 else M_CHAIN + 2000 + (7919 * s) % 15000
        delay_ns = -(-Z * 10**9 // (CH * FROM))
        take_ns = N * DPS + 5 if fading else None
        gain = 0.9 / S * (1 + s % 3)
        w = rh.clip_advance(rh.clip_plan(N, CH, FROM, N, delay_ns, take_ns, fading), CH, FROM, TO, done)
        assert w[1] == Z and w[2] == N and w[5] == done and w[6] - done >= M and (done % M_CHAIN) + M > M_CHAIN
        srcs[s].data, srcs[s].channels, srcs[s].from_rate, srcs[s].phase, srcs[s].frames, srcs[s].last, srcs[s].gain = xs[s].data_ptr(), CH, FROM, 0, M, 0xFFFFFFFF, gain
        clips[rh.source.CLIP_WORDS * s: rh.source.CLIP_WORDS * (s + 1)] = w
        # (b): the stretch of the stream the block's chains span, [base, end)
        q0, j0 = divmod(done, M_CHAIN)
        base, end = q0 * CHAIN, min(((done + M - 1) // M_CHAIN + 1) * CHAIN, Z + N)
        zeros = min(max(Z - base, 0), end - base)
        k0, k1 = max(base - Z, 0), max(end - Z, 0)  # the sound's samples in the stretch
        n = k1 - k0
        amp, row_in = torch.empty(max(n, 1) + CH, device="cuda"), torch.empty(end - base, device="cuda")
        if n:
            chain_calls.append((lib.rh_amplify, (vp(amp.data_ptr()), vp(xs[s].data_ptr() + 4 * k0), n, gain, st)))
            if fading:
                taken = torch.empty(n + CH, device="cuda")
                chain_calls.append((lib.rh_take_duration, (vp(taken.data_ptr()), vp(amp.data_ptr()), n, k0, CH, FROM, take_ns, 1, C.byref(n_taken), C.byref(ended), st)))
                keep.append(amp)
                amp = taken
            bytes_a += 4 * n
        chain_calls.append((lib.rh_delay, (vp(row_in.data_ptr()), vp(amp.data_ptr()) if n else None, n, zeros, st)))
        n_out = C.c_uint64(0)
        _lib.check(lib.rh_uniform_row_out_samples(end - base, CH, FROM, CH, TO, end - base, C.byref(n_out)), "rh_uniform_row_out_samples")
        row = torch.empty(n_out.value, device="cuda")
        assert n_out.value >= (j0 + M) * CH
        chain_calls.append((lib.rh_uniform_row, (vp(row.data_ptr()), n_out.value, vp(row_in.data_ptr()), end - base, CH, FROM, CH, TO, end - base, C.byref(got), st)))
        keep += [amp, row_in, row]
        arr_b[s].data, arr_b[s].channels, arr_b[s].from_rate, arr_b[s].phase, arr_b[s].frames, arr_b[s].last, arr_b[s].gain = row.data_ptr() + 4 * CH * j0, CH, TO, 0, M, 0xFFFFFFFF, 1.0
    dst_a, dst_b, dst_c = (torch.empty(M * CH, device="cuda") for _ in range(3))
    a_new = (vp(dst_a.data_ptr()), CH, TO, M, srcs, S, clips, st)
    a_mix_b = (vp(dst_b.data_ptr()), CH, TO, M, arr_b, S, st)
    a_mix_c = (vp(dst_c.data_ptr()), CH, TO, M, arr_b, S, st)
    f_new, f_mix = lib.rh_clip_mix_block, lib.rh_wide_mix_block

    def new():
        if f_new(*a_new):
            raise RuntimeError("rh_clip_mix_block failed")

    def chain():
        bad = 0
        for f, a in chain_calls:
            bad |= f(*a)
        if bad | f_mix(*a_mix_b):
            raise RuntimeError("the chain failed")

    def floor():
        if f_mix(*a_mix_c):
            raise RuntimeError("rh_wide_mix_block failed")

    for _ in range(3):
        new(), chain(), floor()
    torch.cuda.synchronize()
    same = bool(torch.equal(dst_a.view(torch.int32), dst_b.view(torch.int32)))
    if not same:  # no timing of wrong output is ever printed
        raise RuntimeError(f"{S} x {M}, fade {fade}: the entry's block and the chain's differ")
    t = {"entry": [], "chain": [], "floor": []}
    for _ in range(rounds):
        t["entry"].append(window(new, steps))
        t["chain"].append(window(chain, steps))
        t["floor"].append(window(floor, steps))
    med = {k: float(np.median(v)) for k, v in t.items()}
    launches = -(-S // 32)
    out = {"sources": S, "out_frames": M, "fade": fade, "fading_clips": int(faded), "bit_identical_to_chain": same}
    for k, n_launch in (("entry", launches), ("chain", len(chain_calls) + launches), ("floor", launches)):
        out[k] = {"ms": med[k], "min": min(t[k]), "max": max(t[k]), "spread": (max(t[k]) - min(t[k])) / med[k], "launches": n_launch}
    out["entry"].update({"bytes": bytes_a, "GBps": bytes_a / med["entry"] / 1e6, "frac_of_8TBps": bytes_a / med["entry"] / 1e6 / 8000})
    out["chain_over_entry"] = med["chain"] / med["entry"]
    out["entry_over_floor"] = med["entry"] / med["floor"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x16384,256x65536")
    ap.add_argument("--fade", default="half", choices=("half", "none", "all"))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    source._ensure()
    for sh in a.shapes.split(","):
        S, M = (int(v) for v in sh.split("x"))
        print(json.dumps(shape(S, M, a.fade, a.steps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
