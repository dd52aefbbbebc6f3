"""The headline shape on 16-bit PCM sources: 256 sources x 1 Mi stereo frames, 44.1 -> 48 kHz, low_pass(200), inputs resident.  Three forms in one
process, alternating, timed with device events over windows of launches:

    (a) rh_rlm_run on f32 rows                                   -- the f32 path as it always was
    (b) rh_rlm_run on PCM16 rows, native (k_rlm_chunk_pcm16)     -- rh_rlm_set_sources_pcm16
    (c) rh_convert_i16_to_f32 of all rows, then (a)              -- what a caller with PCM16 assets did before

    python tools/bench_pcm16.py [--sources 256] [--frames 1048576] [--launches 20] [--windows 7] [--only a|b|c]

Prints, per form: ms per step (median over the windows), the windows' spread, the algorithmic bytes ((a), (c): S N C 4 + M C 4; (b): S N C 2 + M C 4)
and that figure over 8 TB/s; then one comparison of (b)'s bits with (a)'s.  --only b: that form alone, for a profiler run of its own
(rocprofv3 --kernel-trace --stats -- python tools/bench_pcm16.py --only b)."""
import argparse
import ctypes as C
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sources", type=int, default=256)
    ap.add_argument("--frames", type=int, default=1 << 20)
    ap.add_argument("--launches", type=int, default=20)
    ap.add_argument("--windows", type=int, default=7)
    ap.add_argument("--only", choices=["a", "b", "c"], default=None)
    args = ap.parse_args()
    import torch

    import rodio_amd as rh
    from rodio_amd import _lib

    rh.init(0)
    S, N, Cn = args.sources, args.frames, 2
    torch.manual_seed(1234)
    i16 = torch.randint(-8192, 8192, (S, N * Cn), dtype=torch.int16, device="cuda")
    f32 = torch.empty((S, N * Cn), dtype=torch.float32, device="cuda")
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    vp = lambda t: C.c_void_p(t.data_ptr())

    def convert():
        _lib.check(_lib.lib.rh_convert_i16_to_f32(vp(f32), vp(i16), S * N * Cn, stream), "rh_convert_i16_to_f32")

    convert()
    gains = [1.0 / S] * S
    pf = rh.ResampleLowpassMix(44100, 48000, Cn, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=N)
    pf.set_gains(gains)
    pf.set_sources([f32[s] for s in range(S)])
    pp = rh.ResampleLowpassMix(44100, 48000, Cn, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=N)
    pp.set_gains(gains)
    pp.set_sources([i16[s] for s in range(S)])
    M = pf.out_frames
    out_a = torch.empty(M * Cn, device="cuda", dtype=torch.float32)
    out_b = torch.empty(M * Cn, device="cuda", dtype=torch.float32)

    def form_a():
        pf.run(out_a)

    def form_b():
        pp.run(out_b)

    def form_c():
        convert()
        pf.run(out_a)

    forms = {"a": form_a, "b": form_b, "c": form_c}
    names = {"a": "(a) rh_rlm_run, f32 rows", "b": "(b) rh_rlm_run, PCM16 rows (native)", "c": "(c) rh_convert_i16_to_f32 of all rows + (a)"}
    algo = {"a": S * N * Cn * 4 + M * Cn * 4, "b": S * N * Cn * 2 + M * Cn * 4, "c": S * N * Cn * 4 + M * Cn * 4}
    which = [args.only] if args.only else ["a", "b", "c"]
    for k in which:  # warm every form
        for _ in range(3):
            forms[k]()
    torch.cuda.synchronize()
    pf.check_status()
    pp.check_status()
    print(f"{S} sources x {N} stereo frames, 44100 -> 48000 Hz, low_pass(200); {M} output frames; windows of {args.launches} launches, {args.windows} per form, alternating")
    print("geometry f32  :", pf.geometry())
    print("geometry pcm16:", pp.geometry(), pp.source_format())
    ms = {k: [] for k in which}
    for _ in range(args.windows):
        for k in which:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(args.launches):
                forms[k]()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1) / args.launches)
    pf.check_status()
    pp.check_status()
    for k in which:
        med, lo, hi = statistics.median(ms[k]), min(ms[k]), max(ms[k])
        print(f"{names[k]:46s} {med:.4f} ms/step  (windows {lo:.4f} .. {hi:.4f}, spread {hi - lo:.4f})  algorithmic {algo[k] / 1e9:.4f} GB -> {algo[k] / (med * 1e-3) / 1e12:.3f} TB/s = "
              f"{algo[k] / (med * 1e-3) / 8e12:.3f} of 8 TB/s")
    if "a" in which and "b" in which:
        a, b = statistics.median(ms["a"]), statistics.median(ms["b"])
        spread_a = max(ms["a"]) - min(ms["a"])
        print(f"(b) / (a) = {b / a:.3f}; (b) - (a) = {b - a:+.4f} ms against (a)'s own spread of {spread_a:.4f} ms: {'within' if b - a <= spread_a else 'SLOWER THAN'} it")
        if "c" in which:
            c = statistics.median(ms["c"])
            print(f"(b) / (c) = {b / c:.3f}: {'faster' if b < c else 'NOT FASTER'} than converting first")
        form_a()
        form_b()
        torch.cuda.synchronize()
        print("bits of (b) equal to (a):", bool(torch.equal(out_a.view(torch.int32), out_b.view(torch.int32))), " native:", pp.source_format()["native"])
    pf.close()
    pp.close()


if __name__ == "__main__":
    main()
