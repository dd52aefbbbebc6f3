"""A block of a mixer of LOOPS -- source.repeat_infinite(), each one second of stereo at 44.1 kHz, a stereo mix at 48 kHz -- three ways in
one process, inputs resident, HIP events, warmed, per block:

  (a) entry   rh_loop_mix_block over the resident passes: ceil(S / 32) launches
  (b) chain   what it replaces on the device.  Rule 1 (the sounds are SamplesBuffers of 88 200 samples: chains of 16384 frames of the unrolled
              stream): per source the block's stretch of the loop unrolled with rh_memcpy_d2d pieces, from the cursor's chain on, rh_uniform_row
              with span_len = 32768 into a row, then rh_wide_mix_block over the rows.  Rule 0 (--rule 0: the same sounds answering None, chains
              of 16384 + 16384 + 11332 frames): every pass converts alike, so the chain is given the converted pass FOR FREE (one rh_uniform_row
              per source outside the timed blocks) and pays only the rh_memcpy_d2d pieces that unroll it into a row, and the mixer.
  (c) floor   rh_wide_mix_block over the 44.1 kHz stretches unrolled beforehand: the same taps and the same lerp without the loop arithmetic
              and without counting the unrolling (its bits differ at the chains' ends: it is a cost floor, not a reference)

Every loop has a cursor of its own.  The three alternate (`--rounds` windows of `--steps` blocks each; the median window is reported with the
fastest and the slowest beside it).  One JSON line per shape; the launches per block and the fraction of the 8 TB/s roofline on (a)'s
algorithmic bytes -- each pass read once, the mix written once -- are in it.

    python tools/bench_loop_mix.py [--shapes 16x16384,256x65536] [--rule 1] [--steps 50] [--rounds 5]
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
L = 44100  # one second


def window(fn, steps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / steps


def span_out(n):
    c = ((n - 1) * T + F - 1) // F
    return c + (1 if c * F < n * T else 0)


def shape(S, M, rule, steps, rounds):
    vp, st, lib = C.c_void_p, source._stream(), _lib.lib
    rng = np.random.default_rng(7)
    xs = [torch.from_numpy((rng.uniform(-1, 1, L * CH) / S).astype(np.float32)).cuda() for _ in range(S)]
    plan = rh.loop_plan(L * CH, CH, L * CH if rule == 1 else 0)
    assert plan[2] == rule
    c = plan[1]
    Mc = span_out(c)
    P = (L // c) * Mc + span_out(L % c)
    words = [rh.loop_advance(plan, FROM, TO, 7919 * s + 100) for s in range(S)]
    srcs, loops = (_lib.WideSrc * S)(), (C.c_uint64 * (5 * S))()
    for s in range(S):
        srcs[s].data, srcs[s].channels, srcs[s].from_rate, srcs[s].phase, srcs[s].frames, srcs[s].last, srcs[s].gain = xs[s].data_ptr(), CH, FROM, 0, M, 0xFFFFFFFF, 1.0
        loops[5 * s: 5 * s + 5] = words[s]
    dst_a, dst_b, dst_c = (torch.empty(M * CH, device="cuda") for _ in range(3))
    a_new = (vp(dst_a.data_ptr()), CH, TO, M, srcs, S, loops, st)

    # (b): the copies that unroll, the converter, the mixer -- every argument built once
    copies, converts, arr_b, arr_c, keep = [], [], (_lib.WideSrc * S)(), (_lib.WideSrc * S)(), []
    got = C.c_uint64(0)
    for s in range(S):
        _, _, _, start, out = words[s]
        n_chains = -(-(out + M) // Mc)
        if rule == 1:
            n_in = n_chains * c  # whole chains of the unrolled stream from the cursor's chain on
            un = torch.empty(n_in * CH, device="cuda")
            pos, at = start, 0
            while at < n_in:
                n = min(L - pos, n_in - at)
                copies.append((vp(un.data_ptr() + 4 * CH * at), vp(xs[s].data_ptr() + 4 * CH * pos), 4 * CH * n, st))
                pos, at = (pos + n) % L, at + n
            row = torch.empty(n_chains * Mc * CH, device="cuda")
            converts.append((vp(row.data_ptr()), row.numel(), vp(un.data_ptr()), n_in * CH, CH, FROM, CH, TO, c * CH, C.byref(got), st))
            skip = out
        else:
            once = torch.empty(P * CH, device="cuda")  # the converted pass: outside the timed blocks
            _lib.check(lib.rh_uniform_row(vp(once.data_ptr()), once.numel(), vp(xs[s].data_ptr()), L * CH, CH, FROM, CH, TO, c * CH, C.byref(got), st), "rh_uniform_row")
            assert got.value == P * CH
            pos = (start // c) * Mc + out
            row = torch.empty(M * CH, device="cuda")
            at = 0
            while at < M:
                n = min(P - pos, M - at)
                copies.append((vp(row.data_ptr() + 4 * CH * at), vp(once.data_ptr() + 4 * CH * pos), 4 * CH * n, st))
                pos, at = (pos + n) % P, at + n
            skip = 0
            keep.append(once)
            # the floor's stretch: the 44.1 kHz frames from the pass's start on (the cursor's place in the pass does not matter to a floor)
            n_in = (M * F) // T + 2
            un = xs[s].repeat(-(-n_in // L))
        keep += [un, row]
        arr_b[s].data, arr_b[s].channels, arr_b[s].from_rate, arr_b[s].phase, arr_b[s].frames, arr_b[s].last, arr_b[s].gain = row.data_ptr() + 4 * CH * skip, CH, TO, 0, M, 0xFFFFFFFF, 1.0
        arr_c[s].data, arr_c[s].channels, arr_c[s].from_rate, arr_c[s].phase, arr_c[s].frames, arr_c[s].last, arr_c[s].gain = un.data_ptr(), CH, FROM, 0, M, 0xFFFFFFFF, 1.0
    a_mix_b = (vp(dst_b.data_ptr()), CH, TO, M, arr_b, S, st)
    a_mix_c = (vp(dst_c.data_ptr()), CH, TO, M, arr_c, S, st)
    f_new, f_copy, f_row, f_mix = lib.rh_loop_mix_block, lib.rh_memcpy_d2d, lib.rh_uniform_row, lib.rh_wide_mix_block

    def new():
        if f_new(*a_new):
            raise RuntimeError("rh_loop_mix_block failed")

    def chain():
        bad = 0
        for a in copies:
            bad |= f_copy(*a)
        for a in converts:
            bad |= f_row(*a)
        if bad | f_mix(*a_mix_b):
            raise RuntimeError("the chain failed")

    def floor():
        if f_mix(*a_mix_c):
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
    b_a = S * 4 * CH * min(L, (M * F) // T + 2) + 4 * CH * M  # every frame of a pass the block reaches once, the mix once
    launches = -(-S // 32)
    out = {"sources": S, "out_frames": M, "rule": rule, "loop_frames": L, "chain_frames": c, "bit_identical_to_chain": same}
    for k, n_launch in (("entry", launches), ("chain", len(copies) + len(converts) + launches), ("floor", launches)):
        out[k] = {"ms": med[k], "min": min(t[k]), "max": max(t[k]), "spread": (max(t[k]) - min(t[k])) / med[k], "launches": n_launch}
    out["entry"].update({"bytes": b_a, "GBps": b_a / med["entry"] / 1e6, "frac_of_8TBps": b_a / med["entry"] / 1e6 / 8000})
    out["chain_over_entry"] = med["chain"] / med["entry"]
    out["entry_over_floor"] = med["entry"] / med["floor"]
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="16x16384,256x65536")
    ap.add_argument("--rule", type=int, default=1, choices=(0, 1))
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    source._ensure()
    for sh in a.shapes.split(","):
        S, M = (int(v) for v in sh.split("x"))
        print(json.dumps(shape(S, M, a.rule, a.steps, a.rounds)), flush=True)


if __name__ == "__main__":
    main()
