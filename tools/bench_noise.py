"""On-device noise sources (rh_noise_generate): for each of noise.rs's nine kinds, 256 streams x 1 Mi samples at 48 kHz -- the kernel
time (the call's three launches, HIP events), its write rate against 8 TB/s, and a pinned rh_memcpy_h2d of the same 1 GiB; then all nine
kinds mixed in one call, and rh_dither over the same sample count (its noise is rh_noise.h's).

    python tools/bench_noise.py [--iters 20] [--out profiles/noise.txt]
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

KINDS = ["white_uniform", "white_triangular", "white_gaussian", "pink", "blue", "violet", "brownian", "red", "velvet"]


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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "noise.txt"))
    args = ap.parse_args()
    rh.init(0)
    G, n = 256, 1 << 20
    nbytes = G * n * 4
    out = torch.empty((G, n), dtype=torch.float32, device="cuda")
    pinned = C.c_void_p()
    check(lib.rh_host_alloc(C.byref(pinned), nbytes), "rh_host_alloc")
    C.memset(pinned, 0, nbytes)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    h2d = timed(lambda: check(lib.rh_memcpy_h2d(C.c_void_p(out.data_ptr()), pinned, nbytes, stream), "h2d"), max(3, args.iters // 4))
    check(lib.rh_host_free(pinned), "rh_host_free")
    lines = [f"device: {torch.cuda.get_device_name(0)}; median of {args.iters}; {G} streams x {n} samples at 48 kHz (1 GiB written)",
             f"pinned upload of the same 1 GiB (rh_memcpy_h2d): {h2d:.3f} ms; the bar (10x faster than uploading): {h2d / 10:.3f} ms", "",
             f"{'kind':>17} {'ms':>8} {'GB/s':>8} {'of 8TB/s':>8} {'h2d/gen':>8} {'bar':>5}"]
    rows = [(k, [k] * G) for k in KINDS] + [("all nine, mixed", [KINDS[g % 9] for g in range(G)])]
    for name, kinds in rows:
        bank = rh.NoiseBank(kinds, 48000, list(range(G)))
        ms = timed(lambda: bank.take(n, out=out), args.iters)
        gbs = nbytes / (ms * 1e-3) / 1e9
        lines.append(f"{name:>17} {ms:>8.3f} {gbs:>8.1f} {gbs / 8000:>8.3f} {h2d / ms:>8.1f} {'met' if h2d / ms >= 10 else 'MISS':>5}")
    # rh_dither: 256 Mi samples in, 256 Mi out (TPDF, stereo, 16 bits: the shape of tools/bench_rows.py's row)
    x = torch.zeros(G * n, dtype=torch.float32, device="cuda")
    flat = out.view(-1)
    ms = timed(lambda: check(lib.rh_dither(C.c_void_p(flat.data_ptr()), C.c_void_p(x.data_ptr()), G * n, 0, 2, 16, 1, 1234, stream), "rh_dither"), args.iters)
    gbs = 2 * nbytes / (ms * 1e-3) / 1e9
    lines += ["", f"rh_dither (HighPass, 2 channels, 16 bits) over the same {G * n} samples, 8 B a sample moved: {ms:.3f} ms, {gbs:.1f} GB/s, "
              f"{gbs / 8000:.3f} of 8 TB/s"]
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    open(args.out, "w").write(text)


if __name__ == "__main__":
    main()
