"""A gate on a side stream: the entries' first contract, "every function enqueues on `stream`", under test (a plain helper module like
arena.py: no fixtures).  tests/test_gpu_stream_order.py holds the cases.

The gate is device work of torch's own -- zero_() of a 1 GiB buffer, repeated -- queued on the stream under test, with an event behind it:
`pending()` is `not event.query()`.  While it is pending nothing queued behind it on that stream has run.  A gated case (run()):

  1. before the gate  every buffer is allocated and staged (arena.py's gate mode): the real inputs and initial states lie in staging
                      tensors, the live buffers hold GARBAGE.  The calls have run once on the stream with the same shapes (scratch, plans,
                      occupancy queries and ring slots exist), and the stream is idle.
  2. behind the gate  device copies put the staged content in place: inputs, states, and the sentinel of every output arena.
  3. the calls        on the stream; `pending()` is read when each returns (a call that waited for the stream returns after the gate).
  4. host arrays      every host array a call was given is overwritten as soon as it returns (Kit.host registers them).
  5. still queued     the arenas are copied to their snapshots, then the live buffers are spoiled with GARBAGE again.
  6. the check        the stream is synchronised; the case's check reads the snapshots.

A launch or copy that went to another stream ran before step 2: it read garbage, and step 2 wiped what it stored.  A reader of a host
table that came late read step 4's garbage.  A kernel that left the stream and ran late read step 5's garbage, and its store missed the
snapshot.  No host thread, no retry: one gate per case."""
import math
import time
from types import SimpleNamespace

import numpy as np

import arena

GIB = 1 << 30


class Delay:
    """The gate's device work, measured once: the time one zero_() of 1 GiB takes on an otherwise idle GPU (HIP events around eight)."""

    def __init__(self):
        import torch

        self.big = torch.empty(GIB, dtype=torch.uint8, device="cuda")
        s = torch.cuda.Stream()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        with torch.cuda.stream(s):
            self.big.zero_()
            e0.record()
            for _ in range(8):
                self.big.zero_()
            e1.record()
        e1.synchronize()
        self.fill_ms = e0.elapsed_time(e1) / 8.0
        assert self.fill_ms > 0.0

    def reps(self, ms):
        return max(1, math.ceil(ms / self.fill_ms))


class Gate:
    """`ms` milliseconds of the delay's fills queued on `stream`, and the event behind them."""

    def __init__(self, delay, stream, ms):
        import torch

        self.reps = delay.reps(ms)
        with torch.cuda.stream(stream):
            for _ in range(self.reps):
                delay.big.zero_()
            self.ev = torch.cuda.Event()
            self.ev.record(stream)

    def pending(self):
        return not self.ev.query()


class Kit:
    """What a case allocates: arenas (staged by run()) and the host arrays of the call in progress."""

    def __init__(self):
        self.arenas, self.fresh, self._pit = [], [], None

    def add(self, a):
        self.arenas.append(a)
        return a

    def src(self, x, lead=0):
        return self.add(arena.src_arena(x, lead))

    def src_rows(self, xs, stride, lead=0):
        return self.add(arena.src_arena_rows(xs, stride, lead))

    def dst(self, n, lead=0, dtype=np.float32):
        return self.add(arena.dst_arena(n, lead, dtype))

    def dst_rows(self, S, n, stride, lead=0):
        return self.add(arena.dst_arena_rows(S, n, stride, lead))

    def state(self, k, init=None):
        return self.add(arena.state_arena(k, init))

    def host(self, a, value=None):
        """Register a host array of the call being made: overwritten (arena.spoil_host) as soon as the call has returned."""
        self.fresh.append((a, value))
        return a

    def pit(self):
        """The address of 1 MiB of NaN on the device: what a spoiled table of device addresses points to, so that a late reader of the
        table computes NaN instead of leaving its rows."""
        import torch

        if self._pit is None:
            self._pit = torch.full((1 << 18,), float("nan"), dtype=torch.float32, device="cuda")
        return self._pit.data_ptr()

    def spoil_hosts(self):
        for a, value in self.fresh:
            arena.spoil_host(a, value)
        self.fresh = []

    def stage(self):
        for a in self.arenas:
            a.stage()

    def restore(self, stream):
        for a in self.arenas:
            a.restore_on(stream)

    def snapshot(self, stream):
        for a in self.arenas:
            a.snapshot_on(stream)

    def spoil(self, stream):
        for a in self.arenas:
            a.spoil_on(stream)


def case(calls, check, rewind=None, warm=None):
    """calls: the entries, each a callable that makes one call on the current stream (torch.cuda.current_stream() is the gated stream while
    they run) and registers its host arrays with Kit.host; check: reads the snapshots; warm: the calls of the warming run where they are
    not `calls`; rewind: run on the stream between the warming run and the gated one (a handle's reset)."""
    return SimpleNamespace(calls=list(calls), check=check, rewind=rewind, warm=list(calls if warm is None else warm))


def run(build, stream, delay, gate_ms):
    """build(kit) -> case(...).  Runs the six steps; returns the case's kit, whether the gate was pending when each call returned and
    when everything was queued, and each call's host time.  The caller asserts on `pending` and runs `check()`."""
    import torch

    kit = Kit()
    c = build(kit)
    torch.cuda.synchronize()
    kit.stage()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        # 1. warmed, then garbage in every live buffer and an idle stream
        kit.restore(stream)
        for call in c.warm:
            call()
            kit.spoil_hosts()
        stream.synchronize()
        if c.rewind is not None:
            c.rewind()
            stream.synchronize()
        kit.spoil(stream)
        stream.synchronize()
        # 2. - 5.: nothing below synchronises
        gate = Gate(delay, stream, gate_ms)
        kit.restore(stream)
        pending, host_ms = [], []
        for call in c.calls:
            t0 = time.perf_counter()
            call()
            t1 = time.perf_counter()
            pending.append(gate.pending())
            host_ms.append((t1 - t0) * 1e3)
            kit.spoil_hosts()
        kit.snapshot(stream)
        kit.spoil(stream)
        queued = gate.pending()
        stream.synchronize()  # 6.
    return SimpleNamespace(kit=kit, pending=pending, queued=queued, host_ms=host_ms, check=c.check, reps=gate.reps)
