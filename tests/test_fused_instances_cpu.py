"""tests/fused_instances.py against the sources, no GPU: its six lists are the instance tables of rodio_amd/csrc/rh_pipeline_fast_lo / _fast_hi /
_fast1 / _wave.hip row for row (a row added to or dropped from a table fails here until the list follows, and test_gpu_fused_instances.py then
runs it), every row is the one its case selects, and the geometry overrides of every ragged case reach the fast plan too."""
import os
import re

import pytest
from fused_instances import RATES, SOURCES, TABLES, case_of, equal_frames, fast_table_of, kv_needed, out_frames, ragged_frames, reduced, select

CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "rodio_amd", "csrc")


def _rows_in(path, macro):
    """The (R, KV, NS) of every use of `macro` with literal arguments, in the branch a shipped build compiles (not RH_DEV_VARIANTS)."""
    with open(os.path.join(CSRC, path)) as f:
        text = f.read()
    text = re.sub(r"#ifdef RH_DEV_VARIANTS.*?#else", "", text, flags=re.S)
    assert "RH_DEV_VARIANTS" not in text, path  # (another form of the switch: this reader has to learn it)
    rows = []
    for m in re.finditer(r"\b" + macro + r"\(([^()]*)\)", text):
        args = [a.strip() for a in m.group(1).split(",")]
        if not all(a.isdigit() for a in args):
            continue  # the macro's own definition: RH_FAST(r, kv, ns)
        v = [int(a) for a in args]
        assert len(v) in (2, 3), (path, m.group(0))
        rows.append((v[0], v[1], v[2] if len(v) == 3 else 2))  # RH_RAG(r, kv), RH_RAG1(r, kv): rings of 2 stages
    return rows


@pytest.mark.parametrize("table", list(TABLES))
def test_the_lists_are_the_tables_of_the_sources(table):
    listed = TABLES[table][0]
    found = [row for path, macro in SOURCES[table] for row in _rows_in(path, macro)]
    assert len(found) == len(set(found)), ("a row twice in the sources", table, sorted(r for r in found if found.count(r) > 1))
    assert len(listed) == len(set(listed)), ("a row twice in the list", table)
    assert sorted(found) == sorted(listed), ("only in the sources", sorted(set(found) - set(listed)), "only in fused_instances.py", sorted(set(listed) - set(found)))


def test_the_tables_have_the_sizes_the_matrix_counts():
    assert {t: len(v[0]) for t, v in TABLES.items()} == {"fast": 53, "fast1": 26, "wave": 16, "wave1": 14, "rag": 16, "rag1": 9}
    assert sum(len(v[0]) * len(v[3]) for v in TABLES.values()) == 259  # kernels the GPU matrix runs


def test_no_other_instance_macro_in_the_four_units():
    """Every RH_<NAME>(digits...) of the four units belongs to one of the six tables: a seventh table would need a list of its own."""
    known = {m for uses in SOURCES.values() for _, m in uses}
    for path in sorted({p for uses in SOURCES.values() for p, _ in uses}):
        with open(os.path.join(CSRC, path)) as f:
            used = set(re.findall(r"\b(RH_[A-Z0-9]+)\(\s*\d+\s*,\s*\d+", f.read()))
        assert used <= known, (path, used - known)


def test_kv_needed_on_known_values():
    """By hand from the formula: a tile of 64 * 8 stereo frames at 44.1 -> 48 kHz spans (513 * 147) / 160 + 5 + 14 = 490 frames = 245 vectors,
    + 2 -> 4 KiB of 64 vectors; at 2 : 1 (513 * 2 + 19 = 1045 frames, 524 vectors) 9 KiB; mono frames are half the bytes."""
    assert kv_needed(512, 147, 160, 2) == 4 and kv_needed(512, 2, 1, 2) == 9
    assert kv_needed(512, 147, 160, 1) == 2 and kv_needed(512, 1, 1, 1) == 3


@pytest.mark.parametrize("table", list(TABLES))
def test_every_row_is_selected_by_its_case(table):
    rows = TABLES[table][0]
    for row in rows:
        c = case_of(table, row)
        assert (c.frm, c.to) in RATES and c.ch == TABLES[table][1]
        assert select(table, c.R, c.NS, c.frm, c.to) == row, (table, row, c)
        F, T = reduced(c.frm, c.to)
        assert 2 * F <= 9 * T, c  # rh_rlm_create refuses ratios above 4.5
        # ... and it is the first pair of the list that does
        first = next((frm, to) for frm, to in RATES
                     if select(table, c.R, c.NS, frm, to) == row and (c.family == "fast" or select(fast_table_of(table), c.R, c.NS, frm, to)))
        assert first == (c.frm, c.to)


@pytest.mark.parametrize("table", ["wave", "wave1", "rag", "rag1"])
def test_the_overrides_of_a_ragged_case_reach_the_fast_plan(table):
    """rh_rlm_create plans k_rlm_fast first, with the same frames_per_lane / ring_stages: without such an instance a stereo handle is refused
    (RH_ERR_INVALID) and a mono one plans again without the overrides."""
    fast = TABLES[fast_table_of(table)][0]
    for row in TABLES[table][0]:
        assert any((r, ns) == (row[0], row[2]) for r, _, ns in fast), (table, row)
        c = case_of(table, row)
        assert select(fast_table_of(table), c.R, c.NS, c.frm, c.to) is not None, c  # ... large enough at the case's rates


@pytest.mark.parametrize("table", list(TABLES))
@pytest.mark.parametrize("J", [0, 1, 9, 32])
def test_the_shapes_cross_every_seam(table, J):
    """Whatever look-back the handle reports: max(6, J + 2) whole tiles and a partial one, no multiple of 4 frames; the ragged shape has its
    longest sources at one length, one that ends inside a tile within two tiles of the end, and one of about half the length."""
    for row in TABLES[table][0]:
        c = case_of(table, row)
        L = 64 * c.R
        ns = [equal_frames(c, J)] * c.S if c.family == "fast" else ragged_frames(c, J)
        assert len(ns) == 5 and max(r[2] for r in TABLES[table][0]) < len(ns)  # the ring wraps
        M = out_frames(max(ns), c.frm, c.to)
        assert M // L >= max(6, J + 2) and M % L != 0 and M % 4 != 0, (c, M)
        assert M < 64 * 20 * 36  # (a few tens of thousands of frames at the most)
        if c.family != "fast":
            ms = [out_frames(n, c.frm, c.to) for n in ns]
            assert sorted(ns)[-3:] == [max(ns)] * 3 and ms.count(M) == 3
            near, half = sorted(ms)[1], sorted(ms)[0]
            assert L < M - near <= 2 * L and near % L not in (0, L - 1), (c, ms)
            assert abs(half - M / 2) <= 0.01 * M + 2, (c, ms)
