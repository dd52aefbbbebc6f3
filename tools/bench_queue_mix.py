"""A block of a mixer of QUEUES -- every queue a playlist of one-second stereo sounds at 44.1 kHz, each behind a gain of its own, a stereo mix
at 48 kHz, every block crossing at least one seam between two sounds -- three ways in one process, inputs resident, HIP events, warmed, per
block:

  (a) entry   rh_queue_mix_block over the resident sounds: one copy of the tables and ONE launch
  (b) chain   what it replaces on the device: per sound rh_amplify of the stretch the block's chains read into one concatenated row,
              rh_uniform_row per converter chain (32768 samples of the stream each, whatever sounds they come from) into rows back to back,
              then rh_wide_mix_block over the rows with gain 1 at the mix's rate
  (c) floor   rh_wide_mix_block over the rows (b) converted, alone: the mixer without the queue

Every queue has a cursor of its own; the seam between its first two sounds falls inside the block.  The three alternate (`--rounds` windows of
`--steps` blocks each; the median window is reported with the fastest and the slowest beside it).  One JSON line per shape; the launches per
block and the fraction of the 8 TB/s roofline on (a)'s algorithmic bytes -- every input frame the block reaches read once, the mix written
once -- are in it.  Every shape runs in a child process of its own under a time limit; after one that fails nothing more is started.

    python tools/bench_queue_mix.py [--shapes 16x16384,256x65536] [--steps 50] [--rounds 5] [--limit 300]
"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FROM, TO, CH = 44100, 48000, 2
F, T = 147, 160
N = 88200        # samples of a sound: one second
CHAIN = 32768    # samples of a converter chain
SOUNDS = 4       # a queue's sounds: more than the longest block's chains read


def span_out(n):
    c = ((n - 1) * T + F - 1) // F
    return c + (1 if c * F < n * T else 0)


def window(fn, steps):
    import torch

    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def shape(S, M, steps, rounds):
    import numpy as np
    import torch

    import rodio_amd as rh
    from rodio_amd import _lib, source

    source._ensure()
    vp, st, lib = C.c_void_p, source._stream(), _lib.lib
    rng = np.random.default_rng(7)
    Mc = span_out(CHAIN // CH)
    xs = [[torch.from_numpy((rng.uniform(-1, 1, N) / S).astype(np.float32)).cuda() for _ in range(SOUNDS)] for _ in range(S)]
    gains = [[0.5 + 0.1 * k + 0.001 * s for k in range(SOUNDS)] for s in range(S)]
    srcs, counts, cursors = (_lib.WideSrc * S)(), (C.c_uint32 * S)(), (C.c_uint64 * (4 * S))()
    sounds, sgains = (C.c_uint64 * (4 * SOUNDS * S))(), (C.c_float * (SOUNDS * S))()
    amps, converts, arr_b, keep = [], [], (_lib.WideSrc * S)(), []
    got = C.c_uint64(0)
    seams = 0
    for s in range(S):
        mine = [rh.QueueSound(x, CH, FROM, g) for x, g in zip(xs[s], gains[s])]
        # the first sound ends 2000 + 37 s output frames into the block, give or take a chain's rounding
        words, dropped = rh.queue_advance(rh.queue_plan(True), mine, TO, 48000 - 2000 - 37 * s)
        assert dropped == 0 and words[2] == 0
        srcs[s].frames, counts[s] = M, SOUNDS
        cursors[4 * s: 4 * s + 4] = words
        for k, q in enumerate(mine):
            sounds[4 * (SOUNDS * s + k): 4 * (SOUNDS * s + k) + 4] = [q.address(), q.samples, q.channels, q.rate]
            sgains[SOUNDS * s + k] = q.gain
        # (b): the chains of the block are 32768 samples of the stream each, from the cursor's chain on
        p0, out = words[0], words[1]
        n_chains = -(-(out + M) // Mc)
        p1 = p0 + n_chains * CHAIN
        assert p1 <= SOUNDS * N and p0 < N < p1
        seams += (p1 - 1) // N
        cat = torch.empty(p1 - p0, device="cuda")
        for k in range(p0 // N, (p1 - 1) // N + 1):
            a, b = max(p0, k * N), min(p1, (k + 1) * N)
            amps.append((vp(cat.data_ptr() + 4 * (a - p0)), vp(xs[s][k].data_ptr() + 4 * (a - k * N)), b - a, gains[s][k], st))
        row = torch.empty(n_chains * Mc * CH, device="cuda")
        for k in range(n_chains):
            converts.append((vp(row.data_ptr() + 4 * k * Mc * CH), Mc * CH, vp(cat.data_ptr() + 4 * k * CHAIN), CHAIN, CH, FROM, CH, TO, CHAIN, C.byref(got), st))
        keep += [cat, row]
        arr_b[s].data, arr_b[s].channels, arr_b[s].from_rate, arr_b[s].phase, arr_b[s].frames, arr_b[s].last, arr_b[s].gain = row.data_ptr() + 4 * CH * out, CH, TO, 0, M, 0xFFFFFFFF, 1.0
    dst_a, dst_b = (torch.empty(M * CH, device="cuda") for _ in range(2))
    a_new = (vp(dst_a.data_ptr()), CH, TO, M, srcs, S, sounds, sgains, counts, cursors, st)
    a_mix = (vp(dst_b.data_ptr()), CH, TO, M, arr_b, S, st)
    f_new, f_amp, f_row, f_mix = lib.rh_queue_mix_block, lib.rh_amplify, lib.rh_uniform_row, lib.rh_wide_mix_block

    def new():
        if f_new(*a_new):
            raise RuntimeError("rh_queue_mix_block failed")

    def chain():
        bad = 0
        for a in amps:
            bad |= f_amp(*a)
        for a in converts:
            bad |= f_row(*a)
        if bad | f_mix(*a_mix):
            raise RuntimeError("the chain failed")

    def floor():
        if f_mix(*a_mix):
            raise RuntimeError("rh_wide_mix_block failed")

    for _ in range(3):
        new(), chain(), floor()
    torch.cuda.synchronize()
    same = bool(torch.equal(dst_a.view(torch.int32), dst_b.view(torch.int32)))
    t = {"entry": [], "chain": [], "floor": []}
    for _ in range(rounds):
        t["entry"].append(window(new, steps))
        t["chain"].append(window(chain, steps))
        t["floor"].append(window(floor, steps))
    med = {k: float(np.median(v)) for k, v in t.items()}
    b_a = S * 4 * CH * ((M * F) // T + 2) + 4 * CH * M  # every input frame the block reaches once, the mix once
    launches = -(-S // 32)  # (rh_wide_mix_block: a launch per 32 sources)
    out = {"queues": S, "out_frames": M, "sound_samples": N, "seams_per_block": seams / S, "bit_identical_to_chain": same}
    for k, n_launch in (("entry", 1), ("chain", len(amps) + len(converts) + launches), ("floor", launches)):
        out[k] = {"ms": med[k], "min": min(t[k]), "max": max(t[k]), "spread": (max(t[k]) - min(t[k])) / med[k], "launches": n_launch}
    out["entry"].update({"bytes": b_a, "GBps": b_a / med["entry"] / 1e6, "frac_of_8TBps": b_a / med["entry"] / 1e6 / 8000})
    out["chain_over_entry"] = med["chain"] / med["entry"]
    out["entry_over_floor"] = med["entry"] / med["floor"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x16384,256x65536")
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--limit", type=int, default=300, help="seconds a shape's process may take")
    ap.add_argument("--child", action="store_true", help="run the one shape in this process")
    a = ap.parse_args()
    for sh in a.shapes.split(","):
        S, M = (int(v) for v in sh.split("x"))
        if a.child:
            print(json.dumps(shape(S, M, a.steps, a.rounds)), flush=True)
            continue
        # a fresh process per shape, under its own time limit; this one never opens the GPU
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", "--shapes", sh, "--steps", str(a.steps), "--rounds", str(a.rounds)], timeout=a.limit)
        if r.returncode:
            sys.exit(f"shape {sh} ended with status {r.returncode}: nothing more is started")


if __name__ == "__main__":
    main()
