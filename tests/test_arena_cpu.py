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


def test_same_compares_bits_and_flattens():
    a = np.array([[0.0, np.nan], [1.0, -0.0]], np.float32)
    assert arena.same(a, a.reshape(-1)) and not arena.same(a, -a) and not arena.same(a[0], a)
    b = a.copy()
    b.view(np.uint32)[0, 1] = arena.SENTINEL
    assert not arena.same(a, b)  # two NaNs of different payloads
