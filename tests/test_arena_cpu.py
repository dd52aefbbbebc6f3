"""tests/arena.py's checker on arrays spoiled by hand: the evidence that the guard-zone tests (test_gpu_arena_*.py) can fail.  No GPU."""
import numpy as np
import pytest

import arena


def _written(lay, counts=None):
    """An arena after a well-behaved kernel: every row word (or the first counts[r] of row r) holds a finite value."""
    w = arena.build(lay)
    counts = [lay.n] * lay.rows if counts is None else counts
    for r, (s, c) in enumerate(zip(lay.starts, counts)):
        w[s: s + c] = (np.arange(c, dtype=np.float32) * np.float32(0.25) - np.float32(r)).view(np.uint32)
    return w


def test_layouts_put_rows_behind_16_byte_boundaries_between_wide_guards():
    assert arena.GUARD >= 1024 and arena.GUARD % 4 == 0
    assert np.isnan(np.array([arena.SENTINEL, arena.POISON], np.uint32).view(np.float32)).all() and arena.SENTINEL != arena.POISON
    for lead in range(4):
        lay = arena.layout(1001, lead)
        assert lay.starts[0] % 4 == lead and lay.starts[0] >= arena.GUARD and lay.total - (lay.starts[0] + 1001) >= arena.GUARD
    lay = arena.layout_rows(3, 1001, 1014, lead=1)
    assert [s - lay.starts[0] for s in lay.starts] == [0, 1014, 2028] and lay.total == arena.GUARD + 1 + 2 * 1014 + 1001 + arena.GUARD
    w = arena.build(arena.layout(5, 0, arena.POISON), [np.arange(5, dtype=np.float32)])
    assert np.all(w[: arena.GUARD] == arena.POISON) and np.all(w[arena.GUARD + 5:] == arena.POISON)
    assert np.array_equal(w[arena.GUARD: arena.GUARD + 5].view(np.float32), np.arange(5, dtype=np.float32))


def test_clean_layouts_pass_and_return_the_rows():
    lay = arena.layout(1001, lead=3)
    w = _written(lay)
    row = arena.check(w, lay)
    assert row.shape == (1001,) and np.array_equal(row, w[lay.starts[0]: lay.starts[0] + 1001])
    lay = arena.layout_rows(3, 257, 268)
    rows = arena.check(_written(lay), lay)
    assert rows.shape == (3, 257) and rows.view(np.float32)[2, 4] == np.float32(-1.0)
    lay = arena.layout(1000)
    assert arena.check(_written(lay, [640]), lay, written=640).shape == (1000,)
    lay = arena.layout_rows(2, 10, 16)
    arena.check(_written(lay, [10, 3]), lay, written=[10, 3])
    arena.check(arena.build(arena.layout(0)), arena.layout(0))  # an entry that may write nothing at all


def test_a_write_one_word_in_front_of_the_row():
    lay = arena.layout(1001, lead=1)
    w = _written(lay)
    w[lay.starts[0] - 1] = np.float32(0.5).view(np.uint32)
    with pytest.raises(AssertionError, match=r"stored outside.*offset -1 relative to row 0"):
        arena.check(w, lay)


def test_a_write_one_word_behind_the_row():
    lay = arena.layout(1001)
    w = _written(lay)
    w[lay.starts[0] + 1001] = 0  # +0.0: the rest of a 16-byte store
    with pytest.raises(AssertionError, match=r"stored outside.*offset \+1001 relative to row 0"):
        arena.check(w, lay)


def test_a_write_in_a_stride_gap_of_row_1_of_3():
    lay = arena.layout_rows(3, 1001, 1014)
    w = _written(lay)
    w[lay.starts[1] + 1003] = np.float32(1.0).view(np.uint32)
    with pytest.raises(AssertionError, match=r"stored outside.*offset \+1003 relative to row 1"):
        arena.check(w, lay)


def test_a_nan_of_another_payload_in_a_guard_is_a_write_too():
    lay = arena.layout(16)
    w = _written(lay)
    w[-1] = arena.POISON  # (a source's poison copied through: compared as bits, not as floats)
    with pytest.raises(AssertionError, match="stored outside"):
        arena.check(w, lay)


def test_an_untouched_word_in_the_middle_of_a_row():
    lay = arena.layout_rows(3, 1001, 1014)
    w = _written(lay)
    w[lay.starts[2] + 500] = arena.SENTINEL
    with pytest.raises(AssertionError, match=r"never written.*offset \+500 relative to row 2"):
        arena.check(w, lay)


def test_a_touched_word_behind_a_short_count():
    lay = arena.layout(1000)
    w = _written(lay, [641])
    with pytest.raises(AssertionError, match=r"stored outside.*offset \+640 relative to row 0"):
        arena.check(w, lay, written=640)
    with pytest.raises(AssertionError, match=r"never written.*offset \+641 relative to row 0"):
        arena.check(w, lay, written=642)


def test_check_wants_the_words_it_was_built_for():
    lay = arena.layout(8)
    with pytest.raises(AssertionError):
        arena.check(_written(lay).view(np.float32), lay)  # floats: NaN != NaN would hide every guard
    with pytest.raises(AssertionError):
        arena.check(_written(lay)[:-1], lay)


def test_a_scratch_arena_is_held_by_its_guards_alone():
    lay = arena.layout(100)
    w = _written(lay, [37])  # as much of the scratch as the entry liked
    arena.check_guards(w, lay)
    w[lay.starts[0] + 100] = 0
    with pytest.raises(AssertionError, match=r"stored outside.*offset \+100 relative to row 0"):
        arena.check_guards(w, lay)


# ---- byte layouts and the two fills (rows of 1-, 2- and 8-byte elements, sample bytes at any byte address) -----------------------------
def _ref_rows(lay, dtype):
    """What a well-behaved kernel leaves in the rows: values that hold neither fill byte."""
    k = lay.n // np.dtype(dtype).itemsize
    return [(np.arange(k) % 61 + 1 + r).astype(dtype) for r in range(lay.rows)]


def _after(lay, refs):
    return arena.build_bytes(lay, refs)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int32, np.int64, np.float64])
def test_byte_layouts_put_rows_at_every_byte_lead(dtype):
    assert arena.GUARD_BYTES == 4 * arena.GUARD and all(((arena.FILLS[0] ^ arena.FILLS[1]) >> k) & 1 for k in range(8))
    assert all(np.isnan(np.full(7, arena.NAN_FILL, np.uint8)[s: s + 4].copy().view(np.float32)[0]) for s in range(4))
    size = np.dtype(dtype).itemsize
    for lead in range(16):
        for fill in arena.FILLS:
            lay = arena.layout_bytes(1001 * size, lead, fill)
            assert lay.starts[0] % 16 == lead and lay.starts[0] >= arena.GUARD_BYTES and lay.total - (lay.starts[0] + lay.n) >= arena.GUARD_BYTES
            refs = _ref_rows(lay, dtype)
            b = arena.build_bytes(lay, refs)
            assert np.all(b[: lay.starts[0]] == fill) and np.all(b[lay.starts[0] + lay.n:] == fill)
            row = arena.check_filled(b, lay, refs[0])
            assert row.dtype == np.uint8 and np.array_equal(row.view(dtype), refs[0])
    lay = arena.layout_bytes_rows(3, 2002, 2050, lead=7)
    assert [s - lay.starts[0] for s in lay.starts] == [0, 2050, 4100] and lay.starts[0] % 16 == 7
    assert arena.check_filled(_after(lay, _ref_rows(lay, np.int16)), lay, _ref_rows(lay, np.int16)).shape == (3, 2002)


@pytest.mark.parametrize("fill", arena.FILLS)
def test_one_byte_stored_directly_in_front_of_a_byte_row(fill):
    lay = arena.layout_bytes(2 * 1001, lead=5, fill=fill)
    refs = _ref_rows(lay, np.int16)
    b = _after(lay, refs)
    b[lay.starts[0] - 1] = 0
    with pytest.raises(AssertionError, match=r"stored outside.*byte offset -1 relative to row 0"):
        arena.check_filled(b, lay, refs[0])


@pytest.mark.parametrize("fill", arena.FILLS)
def test_one_byte_stored_directly_behind_a_byte_row(fill):
    lay = arena.layout_bytes(8 * 1001, lead=8, fill=fill)
    refs = _ref_rows(lay, np.float64)
    b = _after(lay, refs)
    b[lay.starts[0] + lay.n] ^= 0x01  # one bit of the byte behind the last f64
    with pytest.raises(AssertionError, match=r"stored outside.*byte offset \+8008 relative to row 0"):
        arena.check_filled(b, lay, refs[0])


def test_one_byte_stored_in_the_gap_between_byte_rows():
    lay = arena.layout_bytes_rows(3, 1001, 1024, lead=3)
    refs = _ref_rows(lay, np.uint8)
    b = _after(lay, refs)
    b[lay.starts[1] + 1010] = 0
    with pytest.raises(AssertionError, match=r"stored outside.*byte offset \+1010 relative to row 1"):
        arena.check_filled(b, lay, refs)


def test_a_byte_stored_behind_a_reported_count_of_bytes():
    lay = arena.layout_bytes(4 * 100, lead=4)
    ref = (np.arange(100) + 1).astype(np.int32)
    b = arena.build_bytes(lay)
    b[lay.starts[0]: lay.starts[0] + 4 * 61] = arena.as_bytes(ref[:61])
    arena.check_filled(b, lay, ref, written=4 * 61)
    with pytest.raises(AssertionError, match=r"stored outside.*byte offset \+240 relative to row 0"):
        arena.check_filled(b, lay, ref, written=4 * 60)


@pytest.mark.parametrize("dtype", [np.uint8, np.int16, np.int64])
def test_an_unwritten_element_whose_reference_equals_one_of_the_fills(dtype):
    """The reference of element 500 IS fill 0 repeated: under that fill an element that was never written cannot be told from a written one,
    under the other fill it can -- so a case that runs both fills always notices."""
    size = np.dtype(dtype).itemsize
    failures = 0
    for fill in arena.FILLS:
        lay = arena.layout_bytes(1001 * size, lead=size, fill=fill)
        ref = _ref_rows(lay, dtype)[0]
        ref.view(np.uint8)[500 * size: 501 * size] = arena.FILLS[0]
        b = _after(lay, [ref])
        b[lay.starts[0] + 500 * size: lay.starts[0] + 501 * size] = fill  # the kernel skipped element 500
        if fill == arena.FILLS[0]:
            arena.check_filled(b, lay, ref)  # invisible here ...
        else:
            with pytest.raises(AssertionError, match=rf"row 0 differs from the reference.*first at byte {500 * size}: it still holds the fill"):
                arena.check_filled(b, lay, ref)  # ... and caught here
            failures += 1
    assert failures == 1


def test_a_wrong_value_in_a_byte_row():
    lay = arena.layout_bytes(2 * 1001, lead=2)
    refs = _ref_rows(lay, np.int16)
    b = _after(lay, refs)
    b[lay.starts[0] + 2 * 777] ^= 0x80
    with pytest.raises(AssertionError, match=r"row 0 differs from the reference in 1 byte\(s\).*first at byte 1554"):
        arena.check_filled(b, lay, refs[0])


def test_a_row_that_depends_on_its_surroundings():
    ref = np.linspace(-1, 1, 1001).astype(np.float32)
    arena.same_under_fills([ref.copy(), ref.copy()], ref)
    a, b = ref.copy(), ref.copy()
    a[1000] = np.float32(arena.FILLS[0]) / np.float32(128)  # the last sample took a byte from behind the source, under both fills
    b[1000] = np.float32(arena.FILLS[1]) / np.float32(128)
    with pytest.raises(AssertionError, match="differs from the reference with 0x55 around the source"):
        arena.same_under_fills([a, b], ref)
    with pytest.raises(AssertionError, match="differs from the reference with 0xaa around the source"):
        arena.same_under_fills([ref.copy(), b], ref)
    # an entry that is held to its reference by a tolerance: both outputs are inside it, and only their comparison can tell
    a[1000], b[1000] = ref[1000] + np.float32(2e-6), ref[1000] - np.float32(2e-6)
    with pytest.raises(AssertionError, match=r"depends on its surroundings: \d byte\(s\) differ.*first at byte 4000"):
        arena.same_under_fills([a, b], ref, tol=1e-5)
    arena.same_under_fills([a, a.copy()], ref, tol=1e-5)
    a[3] = np.nan
    with pytest.raises(AssertionError, match="differs from the reference with 0x55"):
        arena.same_under_fills([a, a.copy()], ref, tol=1e-5)  # a NaN is outside every tolerance


def test_check_filled_wants_the_bytes_it_was_built_for():
    lay = arena.layout_bytes(64)
    refs = _ref_rows(lay, np.uint8)
    with pytest.raises(AssertionError):
        arena.check_filled(_after(lay, refs).view(np.uint32), lay, refs[0])
    with pytest.raises(AssertionError):
        arena.check_filled(_after(lay, refs)[:-1], lay, refs[0])
    with pytest.raises(AssertionError):
        arena.same_under_fills([refs[0]], refs[0])


def test_same_compares_bits_and_flattens():
    a = np.array([[0.0, np.nan], [1.0, -0.0]], np.float32)
    assert arena.same(a, a.reshape(-1)) and not arena.same(a, -a) and not arena.same(a[0], a)
    b = a.copy()
    b.view(np.uint32)[0, 1] = arena.SENTINEL
    assert not arena.same(a, b)  # two NaNs of different payloads


# ---- gate mode: the pure parts (the device parts run in test_gpu_stream_order.py, whose control shows that the gate can fail) --------------------
def test_the_three_nans_differ_and_garbage_is_neither_sentinel():
    w = np.array([arena.SENTINEL, arena.POISON, arena.GARBAGE], np.uint32)
    assert np.isnan(w.view(np.float32)).all() and len(set(w.tolist())) == 3
    assert arena.GARBAGE < 2**31  # it fills an int32 tensor
    assert arena.GARBAGE_BYTE not in arena.FILLS and arena.HOST_GARBAGE_BYTE not in arena.FILLS
    # a row that was written with garbage counts as written, one that the restore wiped does not: what the control relies on
    lay = arena.layout(16)
    w = arena.build(lay)
    with pytest.raises(AssertionError, match="never written: 16 word"):
        arena.check(w, lay)
    w[lay.starts[0]: lay.starts[0] + 16] = arena.GARBAGE
    assert np.isnan(arena.check(w, lay).view(np.float32)).all()


def test_spoil_host_overwrites_numpy_and_ctypes_arrays_in_place():
    import ctypes as C

    a = np.arange(6, dtype=np.float32).reshape(2, 3)
    keep = a
    assert arena.spoil_host(a) is keep and np.all(arena.host_bytes(a) == arena.HOST_GARBAGE_BYTE) and not np.any(a == np.arange(6, dtype=np.float32).reshape(2, 3))
    t = (C.c_uint64 * 5)(1, 2, 3, 4, 5)
    arena.spoil_host(t)
    assert list(t) == [0xA5A5A5A5A5A5A5A5] * 5 and arena.host_bytes(t).size == 40
    # tables of addresses and lengths: an element value that cannot send a late reader out of bounds
    p = (C.c_void_p * 3)(0x1000, 0x2000, 0x3000)
    arena.spoil_host(p, 0x7000)
    assert [p[i] for i in range(3)] == [0x7000] * 3
    n = np.array([5, 6, 7], np.uint64)
    arena.spoil_host(n, 0)
    assert not n.any()
    with pytest.raises(AssertionError):
        arena.spoil_host(np.arange(10)[::2])  # not the array the call was given


def test_check_unchanged_names_the_first_word_that_differs():
    lay = arena.layout(100, 1, arena.POISON)
    w = arena.build(lay, [np.arange(100, dtype=np.float32)])
    arena.check_unchanged(w.copy(), w, lay)
    bad = w.copy()
    bad[lay.starts[0] + 7] = arena.GARBAGE
    with pytest.raises(AssertionError, match=r"read-only arena was written: 1 element.*offset \+7 relative to row 0"):
        arena.check_unchanged(bad, w, lay)
    bl = arena.layout_bytes(10, 3)
    b = arena.build_bytes(bl, [np.arange(10, dtype=np.uint8)])
    bad = b.copy()
    bad[bl.starts[0] - 1] = 0
    with pytest.raises(AssertionError, match=r"byte offset -1 relative to row 0"):
        arena.check_unchanged(bad, b, bl, arena._where_bytes)


def test_a_kit_spoils_the_host_arrays_of_the_call_that_returned_and_forgets_them():
    import stream_gate

    k = stream_gate.Kit()
    a, b = k.host(np.ones(4, np.float32)), k.host(np.array([3, 4], np.uint64), 0)
    k.spoil_hosts()
    assert np.all(arena.host_bytes(a) == arena.HOST_GARBAGE_BYTE) and not b.any() and k.fresh == []
    c = stream_gate.case([len], print)
    assert c.warm == c.calls == [len] and c.rewind is None and stream_gate.case([len], print, warm=[id]).warm == [id]
