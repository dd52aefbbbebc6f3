"""Source::take_crossfade_with on resident batches: 256 pairs of 2 s, stereo 48 kHz fading out into stereo 44.1 kHz fading in.
Times rh_crossfade (one launch for the batch) and the same pairs through the chain of stand-alone calls it fuses (rh_take_duration
twice, rh_linear_gain_ramp, rh_uniform_row, rh_mix_pair: five calls a pair), alternating the two in rounds so that both see the same
machine; checks that they give the same bits; and expresses both as a fraction of 8 TB/s by ALGORITHMIC bytes -- the admitted samples
of a and b read once, the output written once.

    python tools/bench_crossfade.py [--pairs 256] [--seconds 2.0] [--iters 10] [--rounds 3] [--out profiles/crossfade.txt]
"""
import argparse
import ctypes as C
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import rodio_amd as rh  # noqa: E402
from rodio_amd._lib import CROSSFADE_PAIR_WORDS as W  # noqa: E402
from rodio_amd._lib import check, lib  # noqa: E402


def timed(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, default=256)
    ap.add_argument("--seconds", type=float, default=2.0)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "crossfade.txt"))
    args = ap.parse_args()
    rh.init(0)
    P, d = args.pairs, int(args.seconds * 1e9)
    ca, ra, cb, rb = 2, 48000, 2, 44100
    na, nb = int(args.seconds * ra) * ca, int(args.seconds * rb) * cb
    g = torch.Generator(device="cuda").manual_seed(1)
    a = torch.rand((P, na), generator=g, device="cuda") * 2 - 1
    b = torch.rand((P, nb), generator=g, device="cuda") * 2 - 1
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = C.c_void_p

    pairs = (C.c_uint64 * (W * P))()
    m = C.c_uint64(0)
    pairs[0:9] = [a[0].data_ptr(), na, ca, ra, b[0].data_ptr(), nb, cb, rb, 0]
    check(lib.rh_crossfade_out_samples(pairs, d, C.byref(m)), "rh_crossfade_out_samples")
    n_out = m.value
    ld = (n_out + 3) // 4 * 4  # rows on 16-byte boundaries
    fused_out = torch.zeros((P, ld), device="cuda")
    comp_out = torch.zeros((P, ld), device="cuda")
    for k in range(P):
        pairs[W * k: W * k + W] = [a[k].data_ptr(), na, ca, ra, b[k].data_ptr(), nb, cb, rb, 0, fused_out[k].data_ptr(), n_out]

    def fused():
        check(lib.rh_crossfade(pairs, P, d, None, stream), "rh_crossfade")

    # the stand-alone chain: what TakeDuration admits, and the span its current_span_len() answers (take.rs:180-196)
    ta_n = min(na, d // (1_000_000_000 // (ra * ca)))
    tb_n = min(nb, d // (1_000_000_000 // (rb * cb)))
    span_b = d // (1_000_000_000 // (rb * cb))
    ta = torch.empty(na + ca, device="cuda")
    tb = torch.empty(nb + cb, device="cuda")
    ub = torch.empty(n_out + 64, device="cuda")
    got, ended = C.c_uint64(0), C.c_int32(0)

    def composed():
        for k in range(P):
            check(lib.rh_take_duration(vp(ta.data_ptr()), vp(a[k].data_ptr()), na, 0, ca, ra, d, 1, C.byref(got), C.byref(ended), stream), "rh_take_duration")
            check(lib.rh_take_duration(vp(tb.data_ptr()), vp(b[k].data_ptr()), nb, 0, cb, rb, d, 0, C.byref(got), C.byref(ended), stream), "rh_take_duration")
            check(lib.rh_linear_gain_ramp(vp(tb.data_ptr()), vp(tb.data_ptr()), tb_n, 0, cb, rb, d, 0.0, 1.0, 0, stream), "rh_linear_gain_ramp")
            check(lib.rh_uniform_row(vp(ub.data_ptr()), n_out + 64, vp(tb.data_ptr()), tb_n, cb, rb, ca, ra, span_b, C.byref(got), stream), "rh_uniform_row")
            check(lib.rh_mix_pair(vp(comp_out[k].data_ptr()), vp(ta.data_ptr()), ta_n, vp(ub.data_ptr()), got.value, stream), "rh_mix_pair")

    fused(), composed()  # warm-up: code objects, the stream's scratch
    torch.cuda.synchronize()
    same = bool(torch.equal(fused_out.view(torch.int32), comp_out.view(torch.int32)))
    tf, tc = [], []
    for _ in range(args.rounds):
        tf += timed(fused, args.iters)
        tc += timed(composed, max(2, args.iters // 3))
    nbytes = P * 4 * (ta_n + tb_n + n_out)

    def row(name, ts):
        med = float(np.median(ts))
        gbs = nbytes / (med * 1e-3) / 1e9
        return f"{name:>34} {med:>9.3f} {min(ts):>9.3f} {max(ts):>9.3f} {gbs:>9.1f} {gbs / 8000:>9.3f}"

    lines = [f"device: {torch.cuda.get_device_name(0)}; {P} pairs of {args.seconds} s, stereo 48 kHz (a, fading out) into stereo 44.1 kHz (b, fading in);",
             f"{ta_n} + {tb_n} samples admitted and {n_out} written a pair: {nbytes / 2**20:.1f} MiB of algorithmic traffic a batch;",
             f"{args.rounds} rounds alternating the two, {args.iters} / {max(2, args.iters // 3)} timed calls a round (HIP events around the call); spread = min .. max of all calls",
             f"bits of rh_crossfade == bits of the stand-alone chain: {same}", "",
             f"{'':>34} {'median ms':>9} {'min ms':>9} {'max ms':>9} {'GB/s':>9} {'of 8TB/s':>9}",
             row("rh_crossfade (one launch)", tf), row(f"stand-alone chain ({5 * P} calls)", tc),
             f"ratio of the medians: {float(np.median(tc)) / float(np.median(tf)):.1f}x"]
    text = "\n".join(lines) + "\n"
    print(text)
    if not same:
        raise SystemExit("rh_crossfade and the stand-alone chain differ")
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    shown = [x for i, x in enumerate(sys.argv) if i and x != "--out" and sys.argv[i - 1] != "--out" and not x.startswith("--out=")]  # (where the report goes is no part of it)
    open(args.out, "w").write("command: " + " ".join(["python tools/bench_crossfade.py"] + shown) + "\n" + text)


if __name__ == "__main__":
    main()
