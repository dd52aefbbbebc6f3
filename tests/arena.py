"""Guard zones and poisoned surroundings for the kernels' rows (a plain helper module like fallback_cases.py: no fixtures).

A kernel's `dst`, `state` and `scratch` live in SENTINEL arenas: one device buffer whose every 32-bit word holds a quiet NaN with a payload
(0x7fc5a5a5) before the call, the row(s) `lead` elements behind a 16-byte boundary, at least GUARD words in front and behind, and sentinel
in the gaps between batched rows.  Its sources live in POISON arenas: the samples between two zones of another quiet NaN (0x7fc00bad), so a
read outside a row that reaches the arithmetic comes out as NaN instead of as `junk * 0`.  `check` works on the uint32 words that were copied
back: every guard and gap word must still be the sentinel (nothing stored outside a row) and every row word must differ from it (nothing
left unwritten), except behind the count an entry reports (`*out_n` of rh_chirp, the samples a take admits), where it must still be there.

Rows of 1-, 2- and 8-byte elements, and sample bytes at any byte address (`file + data_offset`), lie in BYTE layouts: the row `lead` bytes
(0..15) behind a 16-byte boundary, GUARD_BYTES of one byte value in front and behind.  Integers have no NaN, so those arenas come in PAIRS,
one per value of FILLS (two bytes that differ in every bit).  A source between fills: the call runs under both, each output equals the
reference and the two outputs equal each other bit for bit (`same_under_fills`) -- a row that takes anything from its surroundings differs
under one of them.  A destination between fills (`check_filled`): under each fill every guard and gap byte is untouched and the row equals
the reference -- an element that was never written still holds the fill, which equals the reference under at most one of the two.

Gate mode (tests/stream_gate.py, test_gpu_stream_order.py): `stage()` keeps an arena's content aside and leaves GARBAGE (a third NaN) in the
live buffer; `restore_on`, `snapshot_on` and `spoil_on` queue copies and fills on the stream under test, and `check_snapshot` /
`snapshot_unchanged` are the checks above on the snapshot.  `spoil_host` is what a host table gets once its call has returned.

The layouts and the checkers are pure numpy (tests/test_arena_cpu.py holds them on arrays spoiled by hand); only `Arena` and `ByteArena`
touch torch."""
import numpy as np

GUARD = 1024  # words in front of the first row and behind the last one: a multiple of 4, wider than any vector or tile tail
SENTINEL = 0x7FC5A5A5  # quiet NaN, payload 0x5a5a5: what an output arena holds before the call
POISON = 0x7FC00BAD  # quiet NaN, another payload: what surrounds a source
INT_SENTINEL = 0x80000001  # for integer rows: a value the tests' data cannot produce (function codes, small counters)
GUARD_BYTES = 4 * GUARD  # the same zones in a byte layout
FILLS = (0x55, 0xAA)  # the two surroundings of an integer row: every bit differs, so no element of any size equals both
NAN_FILL = 0xFF  # a byte whose repetition is a NaN at every byte shift of a float (0xffffffff): around f32 sample bytes at odd addresses


class Layout:
    """Where the rows lie in a buffer of `total` 32-bit words: row r covers words [starts[r], starts[r] + n); everything else is guard or gap
    and holds `fill`."""

    def __init__(self, total, starts, n, fill):
        self.total, self.starts, self.n, self.fill = int(total), [int(s) for s in starts], int(n), int(fill)

    @property
    def rows(self):
        return len(self.starts)


def layout_rows(S, n, stride, lead=0, fill=SENTINEL):
    """S rows of n words, `stride` words apart (stride >= n), the first one `lead` words behind a 16-byte boundary."""
    assert S >= 1 and n >= 0 and stride >= n and 0 <= lead < 4 and GUARD % 4 == 0
    span = (S - 1) * stride + n
    return Layout(GUARD + lead + span + GUARD, [GUARD + lead + r * stride for r in range(S)], n, fill)


def layout(n, lead=0, fill=SENTINEL):
    return layout_rows(1, n, n, lead, fill)


def build(lay, rows=None):
    """The uint32 words of a fresh arena: `fill` everywhere, row r = the 32-bit words of rows[r] where rows are given."""
    w = np.full(lay.total, lay.fill, dtype=np.uint32)
    if rows is not None:
        assert len(rows) == lay.rows
        for s, x in zip(lay.starts, rows):
            x = np.ascontiguousarray(x).reshape(-1)
            assert x.dtype.itemsize == 4 and x.size == lay.n
            w[s: s + lay.n] = x.view(np.uint32)
    return w


def _where(lay, i):
    """Word i of the buffer as an offset relative to a row: the row it lies in or behind, row 0 for the leading guard."""
    r = max([k for k, s in enumerate(lay.starts) if s <= i], default=0)
    return f"offset {i - lay.starts[r]:+d} relative to row {r} (rows of {lay.n} words)"


def check(host_words, lay, written=None):
    """host_words: the arena's words after the call (uint32).  written: words the entry's contract says it writes, one count for every row or
    a count per row; None = all n.  Raises AssertionError that names the first offending offset; returns the rows' words, shape (n,) for
    one row and (rows, n) otherwise (a copy)."""
    w = np.asarray(host_words)
    assert w.dtype == np.uint32 and w.ndim == 1 and w.size == lay.total, "check() wants the arena's uint32 words"
    counts = [lay.n] * lay.rows if written is None else ([int(written)] * lay.rows if np.isscalar(written) else [int(c) for c in written])
    assert len(counts) == lay.rows and all(0 <= c <= lay.n for c in counts)
    must_write = np.zeros(lay.total, dtype=bool)
    for s, c in zip(lay.starts, counts):
        must_write[s: s + c] = True
    stored = np.flatnonzero(~must_write & (w != np.uint32(lay.fill)))
    if stored.size:
        i = int(stored[0])
        raise AssertionError(f"stored outside what the entry may write: {stored.size} word(s), the first at {_where(lay, i)}: 0x{int(w[i]):08x}")
    missed = np.flatnonzero(must_write & (w == np.uint32(lay.fill)))
    if missed.size:
        i = int(missed[0])
        raise AssertionError(f"never written: {missed.size} word(s) still hold the sentinel, the first at {_where(lay, i)}")
    out = np.stack([w[s: s + lay.n] for s in lay.starts]).copy()
    return out[0] if lay.rows == 1 else out


def check_guards(host_words, lay):
    """Only the words outside the rows (a scratch buffer: the entry may use as much of it as it likes, and nothing beside it)."""
    w = np.asarray(host_words)
    assert w.dtype == np.uint32 and w.ndim == 1 and w.size == lay.total, "check_guards() wants the arena's uint32 words"
    inside = np.zeros(lay.total, dtype=bool)
    for s in lay.starts:
        inside[s: s + lay.n] = True
    stored = np.flatnonzero(~inside & (w != np.uint32(lay.fill)))
    if stored.size:
        i = int(stored[0])
        raise AssertionError(f"stored outside what the entry may write: {stored.size} word(s), the first at {_where(lay, i)}: 0x{int(w[i]):08x}")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)


def same(a, b):
    """Two blocks of floats hold the same bits (compared as uint32: a NaN equals itself only bit for bit); shapes are flattened."""
    a, b = np.asarray(a, np.float32).reshape(-1), np.asarray(b, np.float32).reshape(-1)
    return a.shape == b.shape and bool(np.array_equal(bits(a), bits(b)))


GARBAGE = 0x7FC0DEAD  # gate mode: a third quiet NaN, what a live buffer holds outside the gated window
GARBAGE_BYTE = 0xFF  # ... of a byte arena: a NaN at every byte shift of a float, -1 in every integer type
HOST_GARBAGE_BYTE = 0xA5  # ... and a host array after the call it was given to has returned


class _Gated:
    """Gate mode (the section below): stage() / restore_on / snapshot_on / spoil_on for Arena and ByteArena.  Every device operation is
    queued on the given torch stream and none synchronises; snapshot() is read after the caller has synchronised."""

    def stage(self):
        """Keep the buffer's present content as the staged copy (and as `initial`) and fill the live buffer with garbage."""
        self.staged = self.buf.clone()
        self.snap = self.buf.clone()
        self.initial = self.staged.cpu().numpy().view(self.initial.dtype)
        self.buf.fill_(self._garbage)
        self.snap.fill_(self._garbage)
        return self

    def restore_on(self, stream):
        import torch

        with torch.cuda.stream(stream):
            self.buf.copy_(self.staged, non_blocking=True)

    def snapshot_on(self, stream):
        import torch

        with torch.cuda.stream(stream):
            self.snap.copy_(self.buf, non_blocking=True)

    def spoil_on(self, stream):
        import torch

        with torch.cuda.stream(stream):
            self.buf.fill_(self._garbage)

    def snapshot(self):
        """The snapshot's words (bytes for a ByteArena): call after the stream has been synchronised."""
        return self.snap.cpu().numpy().view(self.initial.dtype)


class Arena(_Gated):
    """A layout on the device.  ptr(r) is the address of row r; words() copies the buffer back; check() is check() on that copy;
    unchanged() holds the buffer against what was uploaded (sources, function tables: nothing may write them)."""
    _garbage = GARBAGE

    def __init__(self, lay, rows=None):
        import torch

        self.layout = lay
        self.initial = build(lay, rows)
        self.buf = torch.from_numpy(self.initial.view(np.int32).copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self, r=0):
        return self.buf.data_ptr() + 4 * self.layout.starts[r]

    def words(self):
        import torch

        torch.cuda.synchronize()
        return self.buf.cpu().numpy().view(np.uint32)

    def check(self, written=None, dtype=np.float32):
        return check(self.words(), self.layout, written).view(dtype)

    def check_guards(self):
        check_guards(self.words(), self.layout)

    def unchanged(self):
        w = self.words()
        bad = np.flatnonzero(w != self.initial)
        assert bad.size == 0, f"a read-only arena was written: {bad.size} word(s), the first at {_where(self.layout, int(bad[0]))}"

    # gate mode (below): the same checks on the snapshot
    def check_snapshot(self, written=None, dtype=np.float32):
        return check(self.snapshot(), self.layout, written).view(dtype)

    def snapshot_unchanged(self):
        check_unchanged(self.snapshot(), self.initial, self.layout)


# ---- gate mode (tests/stream_gate.py): an arena whose content arrives on the stream under test ------------------------------------------------
# The live buffer holds GARBAGE until a device copy queued on the gated stream puts the staged content in place; what the entry left is
# copied to a snapshot on the same stream, the live buffer is spoiled again behind it, and the checks read the snapshot.  A launch that ran
# on another stream ran too early (it read garbage, and the restore wiped what it stored) or too late (it read garbage again).


def spoil_host(a, value=None):
    """Overwrite a host array (numpy or ctypes) in place after the call that was given it has returned: every byte HOST_GARBAGE_BYTE, or
    every element `value` -- for tables of device addresses, counts and lengths, where the garbage must be one that cannot send a late
    reader out of bounds (the address of a pit of NaN, a length of 0).  Returns the array."""
    import ctypes

    if isinstance(a, np.ndarray):
        assert a.flags.writeable and a.flags.c_contiguous
        if value is None:
            a.reshape(-1).view(np.uint8)[:] = HOST_GARBAGE_BYTE
        else:
            a[...] = value
    elif value is None or value == 0:  # (zero also for arrays of structures)
        ctypes.memset(ctypes.addressof(a), HOST_GARBAGE_BYTE if value is None else 0, ctypes.sizeof(a))
    else:
        for i in range(len(a)):
            a[i] = value
    return a


def host_bytes(a):
    """The bytes of a host array (numpy or ctypes) as they lie in memory, a copy."""
    import ctypes

    if isinstance(a, np.ndarray):
        return np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()
    return np.frombuffer(ctypes.string_at(ctypes.addressof(a), ctypes.sizeof(a)), np.uint8).copy()


def check_unchanged(words, initial, lay, where=_where):
    """A read-only arena's words (or bytes) against what was staged."""
    w, initial = np.asarray(words), np.asarray(initial)
    assert w.shape == initial.shape and w.dtype == initial.dtype
    bad = np.flatnonzero(w != initial)
    assert bad.size == 0, f"a read-only arena was written: {bad.size} element(s), the first at {where(lay, int(bad[0]))}"


def dst_arena(n, lead=0, dtype=np.float32):
    """n elements of a 32-bit type between sentinel guards, the row `lead` elements behind a 16-byte boundary."""
    return Arena(layout(n, lead, SENTINEL if np.dtype(dtype).kind == "f" else INT_SENTINEL))


def dst_arena_rows(S, n, stride, lead=0):
    return Arena(layout_rows(S, n, stride, lead, SENTINEL))


def src_arena(x, lead=0):
    """x (a 32-bit type) between two poison zones."""
    x = np.ascontiguousarray(x).reshape(-1)
    return Arena(layout(x.size, lead, POISON), [x])


def src_arena_rows(xs, stride, lead=0):
    xs = [np.ascontiguousarray(x).reshape(-1) for x in xs]
    return Arena(layout_rows(len(xs), xs[0].size, stride, lead, POISON), xs)


def inplace_arena(x, lead=0):
    """dst == src: the signal between SENTINEL guards (a signal does not hold the sentinel's payload, so check() still sees the guards)."""
    x = np.ascontiguousarray(x).reshape(-1)
    return Arena(layout(x.size, lead, SENTINEL), [x])


def inplace_arena_rows(xs, stride, lead=0):
    xs = [np.ascontiguousarray(x).reshape(-1) for x in xs]
    return Arena(layout_rows(len(xs), xs[0].size, stride, lead, SENTINEL), xs)


def state_arena(k, init=None):
    """Exactly k 32-bit words of the caller's initial values (zeros by default) between sentinel guards, on a 16-byte boundary: the end is
    usually inside a vector."""
    v = np.zeros(k, np.float32) if init is None else np.ascontiguousarray(init).reshape(-1)
    assert v.size == k
    return Arena(layout(k, 0, SENTINEL), [v])


def plain(x, rows=1, stride=None, lead=0):
    """The same rows in friendly surroundings, for the bit comparisons of arena against plain runs: zeros around and between the sources.
    lead: elements (of x's type) the first row lies behind a 16-byte boundary, as in the arena run it is compared with."""
    import torch

    xs = np.ascontiguousarray(x).reshape(rows, -1)
    stride = stride or xs.shape[1]
    assert (GUARD * xs.dtype.itemsize) % 16 == 0 and 0 <= lead * xs.dtype.itemsize < 16
    buf = np.zeros(GUARD + lead + rows * stride + GUARD, dtype=xs.dtype)
    for r in range(rows):
        buf[GUARD + lead + r * stride: GUARD + lead + r * stride + xs.shape[1]] = xs[r]
    t = torch.from_numpy(buf).cuda()
    assert t.data_ptr() % 16 == 0
    return t, t.data_ptr() + (GUARD + lead) * xs.dtype.itemsize


def plain_dst(n_words):
    """A fresh zeroed dst for the plain run."""
    import torch

    t = torch.zeros(n_words + 8, dtype=torch.float32, device="cuda")
    return t, t.data_ptr()


# ---- rows of any element size: byte layouts, two fills ----------------------------------------------------------------------------------
class ByteLayout:
    """Where the rows lie in a buffer of `total` BYTES: row r covers bytes [starts[r], starts[r] + n); everything else holds the byte `fill`."""

    def __init__(self, total, starts, n, fill):
        self.total, self.starts, self.n, self.fill = int(total), [int(s) for s in starts], int(n), int(fill)
        assert 0 <= self.fill <= 255

    @property
    def rows(self):
        return len(self.starts)


def layout_bytes_rows(S, nbytes, stride, lead=0, fill=FILLS[0]):
    """S rows of nbytes bytes, `stride` bytes apart, the first one `lead` bytes (0..15) behind a 16-byte boundary."""
    assert S >= 1 and nbytes >= 0 and stride >= nbytes and 0 <= lead < 16 and GUARD_BYTES % 16 == 0
    span = (S - 1) * stride + nbytes
    return ByteLayout(GUARD_BYTES + lead + span + GUARD_BYTES, [GUARD_BYTES + lead + r * stride for r in range(S)], nbytes, fill)


def layout_bytes(nbytes, lead=0, fill=FILLS[0]):
    return layout_bytes_rows(1, nbytes, nbytes, lead, fill)


def as_bytes(x):
    """The bytes of an array of any element type, as they lie in memory."""
    return np.ascontiguousarray(x).reshape(-1).view(np.uint8)


def build_bytes(lay, rows=None):
    """The bytes of a fresh arena: `fill` everywhere, row r = the bytes of rows[r] where rows are given."""
    b = np.full(lay.total, lay.fill, dtype=np.uint8)
    if rows is not None:
        assert len(rows) == lay.rows
        for s, x in zip(lay.starts, rows):
            x = as_bytes(x)
            assert x.size == lay.n
            b[s: s + lay.n] = x
    return b


def _where_bytes(lay, i):
    r = max([k for k, s in enumerate(lay.starts) if s <= i], default=0)
    return f"byte offset {i - lay.starts[r]:+d} relative to row {r} (rows of {lay.n} bytes)"


def check_filled(host_bytes, lay, ref_rows, written=None):
    """host_bytes: a byte arena after the call (uint8).  ref_rows: what row r must hold, any element type, lay.n bytes each (one array for
    one row).  written: BYTES of each row the entry's contract says it writes (None = all); behind them the fill must still be there.
    Every guard and gap byte must hold the fill and every row must equal its reference.  An element that was never written holds the fill:
    run the call under both FILLS and it differs from the reference under at least one.  Returns the rows' bytes (a copy)."""
    b = np.asarray(host_bytes)
    assert b.dtype == np.uint8 and b.ndim == 1 and b.size == lay.total, "check_filled() wants the arena's bytes"
    refs = [ref_rows] if lay.rows == 1 and not isinstance(ref_rows, (list, tuple)) else list(ref_rows)
    counts = [lay.n] * lay.rows if written is None else ([int(written)] * lay.rows if np.isscalar(written) else [int(c) for c in written])
    assert len(refs) == lay.rows and len(counts) == lay.rows and all(0 <= c <= lay.n for c in counts)
    may_write = np.zeros(lay.total, dtype=bool)
    for s, c in zip(lay.starts, counts):
        may_write[s: s + c] = True
    stored = np.flatnonzero(~may_write & (b != np.uint8(lay.fill)))
    if stored.size:
        i = int(stored[0])
        raise AssertionError(f"stored outside what the entry may write: {stored.size} byte(s), the first at {_where_bytes(lay, i)}: 0x{int(b[i]):02x} (fill 0x{lay.fill:02x})")
    for r, (s, c, ref) in enumerate(zip(lay.starts, counts, refs)):
        ref = as_bytes(ref)
        assert ref.size >= c, "the reference is shorter than what the entry writes"
        bad = np.flatnonzero(b[s: s + c] != ref[:c])
        if bad.size:
            i = int(bad[0])
            held = "it still holds the fill (never written?)" if b[s + i] == lay.fill else f"0x{int(b[s + i]):02x}"
            raise AssertionError(f"row {r} differs from the reference in {bad.size} byte(s) under fill 0x{lay.fill:02x}, the first at byte {i}: {held}, reference 0x{int(ref[i]):02x}")
    out = np.stack([b[s: s + lay.n] for s in lay.starts]).copy()
    return out[0] if lay.rows == 1 else out


def same_under_fills(outs, ref, tol=0.0, fills=FILLS):
    """outs: the output rows of the same call with its integer source between each of `fills` (any element type).  Each must equal the
    reference -- as bytes (a NaN equals itself only bit for bit), or for an entry that is held by a tolerance within `tol` of it (a NaN
    is outside) -- and they must equal each other as bytes."""
    assert len(outs) == len(fills) == 2
    r = as_bytes(ref)
    bs = [as_bytes(o) for o in outs]
    for fill, o, out in zip(fills, bs, outs):
        assert o.size == r.size, "an output of another length than the reference"
        if tol:
            err = np.abs(np.asarray(out, np.float64).reshape(-1) - np.asarray(ref, np.float64).reshape(-1))
            bad = np.flatnonzero(~(err <= tol))
        else:
            bad = np.flatnonzero(o != r)
        assert bad.size == 0, f"differs from the reference with 0x{fill:02x} around the source: {bad.size} {'value' if tol else 'byte'}(s), the first at {'index' if tol else 'byte'} {int(bad[0])}"
    bad = np.flatnonzero(bs[0] != bs[1])
    assert bad.size == 0, f"the row depends on its surroundings: {bad.size} byte(s) differ between the two fills, the first at byte {int(bad[0])}"


class ByteArena(_Gated):
    """A byte layout on the device; the same calls as Arena.  check(ref_rows) is check_filled on the bytes copied back."""
    _garbage = GARBAGE_BYTE

    def check_snapshot(self, ref_rows, written=None, dtype=np.uint8):
        return check_filled(self.snapshot(), self.layout, ref_rows, written).view(dtype)

    def snapshot_unchanged(self):
        check_unchanged(self.snapshot(), self.initial, self.layout, _where_bytes)

    def __init__(self, lay, rows=None):
        import torch

        self.layout = lay
        self.initial = build_bytes(lay, rows)
        self.buf = torch.from_numpy(self.initial.copy()).cuda()
        assert self.buf.data_ptr() % 16 == 0

    def ptr(self, r=0):
        return self.buf.data_ptr() + self.layout.starts[r]

    def bytes(self):
        import torch

        torch.cuda.synchronize()
        return self.buf.cpu().numpy()

    def check(self, ref_rows, written=None, dtype=np.uint8):
        return check_filled(self.bytes(), self.layout, ref_rows, written).view(dtype)

    def unchanged(self):
        b = self.bytes()
        bad = np.flatnonzero(b != self.initial)
        assert bad.size == 0, f"a read-only arena was written: {bad.size} byte(s), the first at {_where_bytes(self.layout, int(bad[0]))}"


def src_bytes_arena(x, lead=0, fill=FILLS[0]):
    """x (any element type) between two zones of the byte `fill`, `lead` BYTES behind a 16-byte boundary."""
    x = as_bytes(x)
    return ByteArena(layout_bytes(x.size, lead, fill), [x])


def dst_bytes_arena(n, dtype, lead=0, fill=FILLS[0]):
    """n elements of `dtype` between zones of the byte `fill` (the row itself holds it too), `lead` BYTES behind a 16-byte boundary."""
    return ByteArena(layout_bytes(n * np.dtype(dtype).itemsize, lead, fill))
