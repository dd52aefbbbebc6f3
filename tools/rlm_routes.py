"""One short run over every route rlm_launch / sblk_try / chunk_launch_classes can take (rodio_amd/csrc/rh_rlm_launch.h), at the small sizes the
tests use, for comparing the launches of two builds of the library (RODIO_HIP_LIB) under a kernel trace:

    rocprofv3 --kernel-trace --output-format csv -d <dir> -o kt -- python tools/rlm_routes.py
    python tools/rlm_routes.py --dispatches <dir>/.../kt_kernel_trace.csv      the library's launches: kernel, grid x, y, workgroup, LDS bytes

Not a test: it asserts nothing about the samples (tests/test_gpu_mix_first.py, test_gpu_sblk.py, test_gpu_parity.py do)."""
import contextlib
import csv
import os
import re
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))


def dispatches(path):
    rows = list(csv.DictReader(open(path, newline="")))
    rows.sort(key=lambda r: int(r["Dispatch_Id"]))
    for r in rows:
        m = re.search(r"\bk_\w+(<[^()]*>)?", r["Kernel_Name"])  # the library's kernels, by name and template arguments (not torch's or the runtime's copies)
        if m:
            print(m.group(0).replace(" ", ""), r["Grid_Size_X"], r["Grid_Size_Y"], r["Workgroup_Size_X"], r["LDS_Block_Size"])


def main():
    import numpy as np
    import torch

    import rodio_amd as G

    G.init(0)

    @contextlib.contextmanager
    def knobs(**env):  # the library reads its tuning variables in rh_init()
        old = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        G.init(0)
        try:
            yield
        finally:
            for k, v in old.items():
                os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
            G.init(0)

    def rnd(seed, n, scale=0.1):
        return torch.from_numpy((np.random.default_rng(seed).uniform(-1, 1, n) * scale).astype(np.float32)).cuda()

    def one_shot(what, lens, ch=2, filt="low_pass", frm=44100, to=48000, filters=None, batch=False, **kw):
        p = G.ResampleLowpassMix(frm, to, ch, None, filt, 200, 0.5, max_sources=len(lens), max_in_frames=max(lens), **kw)
        if filters:
            p.set_filters(filters)
        p.set_sources([rnd(100 + i, n * ch) for i, n in enumerate(lens)])
        for _ in range(2):  # (the second run finds the handle's buffers in place)
            p.run_batch() if batch else p.run()
        p.check_status()
        geo = p.geometry()  # (behind the run: mix_first = 3 says that the classes went in one launch)
        p.close()
        print(f"{what}: mix_first {geo['mix_first']} ragged_pair {geo['ragged_pair']} general {geo['general_kernel']} tiles {geo['n_tiles']}", flush=True)

    def stream(what, S, block, blocks, per_source=False, ch=2):
        p = G.ResampleLowpassMix(44100, 48000, ch, None, "low_pass", 200, 0.5, max_sources=S, max_in_frames=4 * block)
        p.stream_begin()
        xs = [rnd(300 + s, block * blocks * ch) for s in range(S)]
        for k in range(blocks):
            part = [x[ch * block * k: ch * block * (k + 1)] for x in xs]
            last = k == blocks - 1
            p.stream_feed_v(part, [last] * S) if per_source else p.stream_feed(part, flush=last)
        p.check_status()
        print(f"{what}: stats {p.stream_stats()}", flush=True)
        p.close()

    ragged = [90000] * 5 + [90000 - 700 * i - 13 for i in range(1, 12)] + [45000, 30000, 7000]
    one_shot("equal filtered batch (chunk)", [600000] * 3)
    one_shot("equal filtered batch, mono (chunk)", [600000] * 3, ch=1)
    one_shot("equal filtered batch, short (mix rows + fused)", [30000] * 9)
    with knobs(RH_NO_MIX_FIRST="1"):
        one_shot("RH_NO_MIX_FIRST", [30000] * 9)
    one_shot("filter_first", [8192] * 16, filter_first=True)
    one_shot("unfiltered", [30000] * 9, filt=None)
    one_shot("ragged stereo", ragged)
    one_shot("ragged mono", ragged, ch=1)
    with knobs(RH_RAG_TWO_KERNELS="1"):
        one_shot("ragged stereo, RH_RAG_TWO_KERNELS", ragged)
        one_shot("ragged mono, RH_RAG_TWO_KERNELS", ragged, ch=1)
    one_shot("batch mode, 16 sources", [8192] * 16, batch=True)
    one_shot("batch mode, 7 sources", [8192] * 7, batch=True)
    kinds = [("low_pass", 200), ("high_pass", 300), ("low_pass", 1000)]
    one_shot("filter classes of one geometry", [300000] * 6, filters=kinds * 2)
    one_shot("filter classes of different geometry", [300000, 280000] * 3, filters=kinds[:2] * 3)
    with knobs(RH_CLASSES_ONE_WAVE="1"):
        one_shot("filter classes, RH_CLASSES_ONE_WAVE", [300000] * 6, filters=kinds * 2)
    with knobs(RH_CLASSES_ONE_BY_ONE="1"):
        one_shot("filter classes, RH_CLASSES_ONE_BY_ONE", [300000] * 6, filters=kinds * 2)
    stream("summed stream, 64 Ki-frame blocks", 16, 65536, 4)
    stream("summed stream, 4 Ki-frame blocks", 16, 4096, 6)
    with knobs(RH_NO_SBLK="1"):
        stream("summed stream, 4 Ki-frame blocks, RH_NO_SBLK", 16, 4096, 4)
    stream("per-source-state stream", 6, 25000, 4, per_source=True)
    torch.cuda.synchronize()


if __name__ == "__main__":
    if len(sys.argv) > 2 and sys.argv[1] == "--dispatches":
        dispatches(sys.argv[2])
    else:
        main()
