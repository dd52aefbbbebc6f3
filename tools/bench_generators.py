"""On-device signal generators (rh_signal_generate): the kernel pair alone for G generators x 1 Mi samples at 48 kHz, its write
rate against 8 TB/s, next to a pinned rh_memcpy_h2d of the same bytes; and end to end, 256 generated 44.1 kHz tones -> 48 kHz ->
low_pass(200) -> mix (ResampleLowpassMix) against the same samples pulled from the host (pinned upload + the same run).

    python tools/bench_generators.py [--iters 20] [--out profiles/generators.txt]
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
from rodio_amd._lib import check, lib  # noqa: E402


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(iters):
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "generators.txt"))
    args = ap.parse_args()
    rh.init(0)
    n = 1 << 20
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.iters}; 1 Mi samples per generator at 48 kHz", "",
             "generator kernels alone (k_gen_walk + k_gen_fill), sawtooth / sine:",
             f"{'G':>5} {'freq':>7} {'ms saw':>8} {'ms sine':>8} {'GB/s':>8} {'of 8TB/s':>8} {'h2d ms':>8} {'h2d/gen':>8}"]
    for G in (1, 256, 2048):
        out = torch.empty((G, n), dtype=torch.float32, device="cuda")
        hb = min(G * n * 4, 1 << 30)  # pinned staging of at most 1 GiB: larger copies are scaled from it (PCIe time is linear in bytes)
        pinned = C.c_void_p()
        check(lib.rh_host_alloc(C.byref(pinned), hb), "rh_host_alloc")
        C.memset(pinned, 0, hb)
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        h2d = timed(lambda: check(lib.rh_memcpy_h2d(C.c_void_p(out.data_ptr()), pinned, hb, stream), "h2d"), max(3, args.iters // 4)) * (G * n * 4 / hb)
        for freq in (20.0, 440.0, 5000.0, 20000.0):
            ms = {}
            for fn in ("sawtooth", "sine"):
                bank = rh.GeneratorBank(48000, [freq] * G, fn)
                ms[fn] = timed(lambda: bank.take(n, out=out), args.iters)
            gbs = G * n * 4 / (ms["sine"] * 1e-3) / 1e9
            lines.append(f"{G:>5} {freq:>7.0f} {ms['sawtooth']:>8.3f} {ms['sine']:>8.3f} {gbs:>8.1f} {gbs / 8000:>8.3f} {h2d:>8.3f} {h2d / ms['sine']:>8.1f}")
        check(lib.rh_host_free(pinned), "rh_host_free")
        del out
    # end to end
    G, n = 256, 1 << 20
    freqs = [float(np.float32(55.0 * 1.0145 ** k)) for k in range(G)]
    bank = rh.GeneratorBank(44100, freqs, "sine")
    rows = torch.empty((G, n), dtype=torch.float32, device="cuda")
    p = rh.ResampleLowpassMix(44100, 48000, 1, None, "low_pass", 200, 0.5, max_sources=G, max_in_frames=n)
    p.set_sources([rows[k] for k in range(G)])
    mix = torch.empty(p.out_frames + 16, dtype=torch.float32, device="cuda")
    pinned = C.c_void_p()
    check(lib.rh_host_alloc(C.byref(pinned), G * n * 4), "rh_host_alloc")
    C.memset(pinned, 0, G * n * 4)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    gen = timed(lambda: (bank.take(n, out=rows), p.run(out=mix)), args.iters)
    up = timed(lambda: (check(lib.rh_memcpy_h2d(C.c_void_p(rows.data_ptr()), pinned, G * n * 4, stream), "h2d"), p.run(out=mix)), max(3, args.iters // 4))
    run_only = timed(lambda: p.run(out=mix), args.iters)
    p.check_status()
    check(lib.rh_host_free(pinned), "rh_host_free")
    lines += ["", f"end to end: {G} tones x {n} samples, 44.1 kHz -> 48 kHz -> low_pass(200) -> mix (mono)",
              f"  generated on the device + mix: {gen:.3f} ms",
              f"  pulled from pinned host memory (h2d) + mix: {up:.3f} ms",
              f"  mix alone: {run_only:.3f} ms",
              f"  speed-up of generating over uploading: {up / gen:.1f}x"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
