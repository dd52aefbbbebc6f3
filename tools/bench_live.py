"""Parameters that change while a source plays: the stepped kernels at a size that fills the chip (fraction of 8 TB/s on their
algorithmic bytes, next to the fixed-parameter entries they extend), and the SpatialPlayer tail (channel volume + factor) at block
sizes, as one launch and as two.  HIP events, rows resident.

    python tools/bench_live.py [--mib 512] [--steps 10]
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
from tools.bench_rows import timed


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mib", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    a = ap.parse_args()
    source._ensure()
    lib, st, ck = _lib.lib, source._stream(), _lib.check
    P = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
    n = (a.mib << 20) // 4
    x = (torch.rand(n, device="cuda") * 2 - 1).contiguous()
    dst = torch.empty(n, device="cuda")

    def row(name, fn, alg, **extra):
        ms = timed(fn, a.steps)
        d = {"row": name, "ms": round(ms, 4), "GBps": round(alg / ms / 1e6, 1), "frac": round(alg / ms / 1e6 / 8000, 3), **extra}
        print(json.dumps(d), flush=True)

    def tab(first, period, m, w=1):
        k = (first + m - 1) // period - first // period + 1
        return torch.rand(k * w, device="cuda") + 0.5, k

    row("amplify", lambda: ck(lib.rh_amplify(P(dst), P(x), n, 0.5, st), "rh_amplify"), 8 * n)
    for label, U in (("5 ms / 441", 441), ("10 ms / 960", 960)):
        f, k = tab(0, U, n)
        row(f"amplify_steps {label}", lambda: ck(lib.rh_amplify_steps(P(dst), P(x), n, 0, U, P(f), k, st), "rh_amplify_steps"), 8 * n + 4 * k)
    f1 = torch.full((1,), 0.5, device="cuda")  # one step for the whole row: what the step index and the table load cost without a boundary
    row("amplify_steps one step", lambda: ck(lib.rh_amplify_steps(P(dst), P(x), n, 0, 1 << 40, P(f1), 1, st), "rh_amplify_steps"), 8 * n)
    xo, f, k = x[1:], *tab(220, 441, n - 1)
    row("amplify_steps 5 ms / 441 src+4B", lambda: ck(lib.rh_amplify_steps(P(dst), P(xo), n - 1, 220, 441, P(f), k, st), "rh_amplify_steps"), 8 * (n - 1) + 4 * k)
    g2 = np.array([0.7, 0.4], np.float32)
    row("channel_volume 2->2", lambda: ck(lib.rh_channel_volume(P(dst), P(x), n // 2, 2, g2.ctypes.data_as(_lib.f32p), 2, st), "rh_channel_volume"), 8 * n)
    for label, U in (("5 ms / 441", 441), ("10 ms / 960", 960)):
        g, k = tab(0, U, n, 2)
        row(f"channel_volume_steps 2->2 {label}", lambda: ck(lib.rh_channel_volume_steps(P(dst), P(x), n // 2, 2, 2, 0, U, P(g), k, 0, 1, None, 0, st), "cv_steps"), 8 * n + 8 * k)
    g1 = torch.tensor([0.7, 0.4], device="cuda")
    row("channel_volume_steps 2->2 one step", lambda: ck(lib.rh_channel_volume_steps(P(dst), P(x), n // 2, 2, 2, 0, 1 << 40, P(g1), 1, 0, 1, None, 0, st), "cv_steps"), 8 * n)
    g, kg = tab(0, 960, n, 2)
    f, kf = tab(0, 480, n)
    row("channel_volume_steps 2->2 + factor 960/480", lambda: ck(lib.rh_channel_volume_steps(P(dst), P(x), n // 2, 2, 2, 0, 960, P(g), kg, 0, 480, P(f), kf, st), "cv_steps"),
        8 * n + 8 * kg + 4 * kf)
    for label, ic, oc in (("6->2", 6, 2), ("2->6", 2, 6)):
        fr = n // max(ic, oc)
        g, k = tab(0, 480, fr * oc, oc)
        row(f"channel_volume_steps {label} 10 ms / 480", lambda: ck(lib.rh_channel_volume_steps(P(dst), P(x), fr, ic, oc, 0, 480, P(g), k, 0, 1, None, 0, st), "cv_steps"),
            4 * fr * (ic + oc))
    # the SpatialPlayer tail at block sizes: one launch (channel volume + factor) against two (channel volume, then amplify)
    for frames in (256, 1024, 4096, 32768):
        m = 2 * frames
        g, kg = tab(0, 960, m, 2)
        f, kf = tab(0, 480, m)
        xs, ds = x[:m], dst[:m]
        one = lambda: ck(lib.rh_channel_volume_steps(P(ds), P(xs), frames, 2, 2, 0, 960, P(g), kg, 0, 480, P(f), kf, st), "cv_steps")  # noqa: E731

        def two():
            ck(lib.rh_channel_volume_steps(P(ds), P(xs), frames, 2, 2, 0, 960, P(g), kg, 0, 1, None, 0, st), "cv_steps")
            ck(lib.rh_amplify_steps(P(ds), P(ds), m, 0, 480, P(f), kf, st), "rh_amplify_steps")

        row(f"spatial tail {frames} frames, one launch", one, 8 * m, us=round(timed(one, 200) * 1e3, 2))
        row(f"spatial tail {frames} frames, two launches", two, 8 * m, us=round(timed(two, 200) * 1e3, 2))


if __name__ == "__main__":
    main()
