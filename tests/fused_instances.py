"""The instance tables of the fused kernels, and the smallest batch that makes the library run one given row of them.  No HIP and no GPU:
test_fused_instances_cpu.py holds the lists against the sources and checks the selection; test_gpu_fused_instances.py runs every row.

A row is (R, KV, NS): R output frames per lane (a tile is 64 R frames), a ring of NS stages of KV KiB each.  rh_rlm_create takes R and NS from
rh_rlm_config (frames_per_lane, ring_stages) and KV from the rates: the smallest KV >= kv_needed(64 R, F, T, channels) the table has with that
R and NS (find_variant, rh_pipeline_internal.h).  So a row is pinned by (R, NS) and a rate pair."""
from math import gcd

# ---- the tables, as the sources list them (the shipped branch, not RH_DEV_VARIANTS) -----------------------------------------------------------
# k_rlm_fast, stereo: rh_pipeline_fast_lo.hip (R <= 9) + rh_pipeline_fast_hi.hip (R >= 10); kernels per row: filt + plain
FAST_LO = [(3, 2, 2), (3, 2, 3), (3, 4, 2), (3, 7, 2),
           (4, 2, 2), (4, 2, 3), (4, 3, 2), (4, 3, 3), (4, 5, 2), (4, 9, 2),
           (5, 3, 2), (5, 3, 3), (5, 6, 2),
           (6, 3, 2), (6, 3, 3), (6, 4, 2), (6, 4, 3), (6, 7, 2), (6, 14, 2),
           (7, 4, 2), (7, 4, 3), (7, 8, 2),
           (8, 4, 2), (8, 4, 3), (8, 4, 4), (8, 5, 2), (8, 5, 3), (8, 9, 2),
           (9, 5, 2), (9, 5, 3), (9, 10, 2)]
FAST_HI = [(10, 5, 2), (10, 5, 3), (10, 6, 2), (10, 6, 3), (10, 11, 2),
           (12, 6, 2), (12, 6, 3), (12, 7, 2), (12, 7, 3), (12, 13, 2),
           (14, 7, 2), (14, 8, 2),
           (16, 8, 2), (16, 8, 3), (16, 9, 2), (16, 9, 3),
           (18, 9, 2), (18, 9, 3), (18, 10, 2),
           (20, 10, 2), (20, 10, 3), (20, 11, 2)]
FAST = FAST_LO + FAST_HI
# k_rlm_fast, mono: rh_pipeline_fast1.hip; filt + plain
FAST1 = [(4, 2, 2), (4, 3, 2), (4, 5, 2), (6, 2, 2), (6, 4, 2), (6, 7, 2), (8, 2, 2), (8, 3, 2),
         (8, 5, 2), (8, 10, 2), (9, 3, 2), (9, 5, 2), (10, 3, 2), (10, 6, 2), (12, 3, 2), (12, 4, 2),
         (12, 7, 2), (16, 4, 2), (16, 5, 2), (16, 9, 2), (18, 5, 2), (18, 5, 3), (18, 10, 2), (20, 5, 2),
         (20, 6, 2), (20, 11, 2)]
# k_rlm_wave, stereo / mono: rh_pipeline_wave.hip (kWave, kWave1); filt + plain
WAVE = [(6, 3, 2), (6, 4, 2), (6, 7, 2), (6, 14, 2), (8, 4, 2), (8, 4, 3), (8, 5, 2), (8, 9, 2),
        (9, 5, 2), (9, 5, 3), (10, 5, 2), (10, 5, 3), (10, 6, 2), (12, 6, 2), (12, 6, 3), (12, 7, 2)]
WAVE1 = [(6, 2, 2), (6, 4, 2), (6, 7, 2), (8, 2, 2), (8, 3, 2), (8, 5, 2), (8, 10, 2),
         (9, 3, 2), (9, 5, 2), (10, 3, 2), (10, 6, 2), (12, 3, 2), (12, 4, 2), (12, 7, 2)]
# k_rlm_fast<RAG> (+ k_rlm_resid<R, KV>, stereo only), rh_pipeline_wave.hip (kRag, kRag1): every ring has 2 stages
RAG = [(6, 3, 2), (6, 4, 2), (6, 7, 2), (6, 14, 2), (8, 4, 2), (8, 5, 2), (8, 9, 2), (9, 5, 2), (10, 5, 2), (10, 6, 2), (12, 6, 2), (12, 7, 2),
       (14, 7, 2), (14, 8, 2), (18, 9, 2), (18, 10, 2)]
RAG1 = [(6, 2, 2), (8, 2, 2), (8, 3, 2), (10, 3, 2), (12, 3, 2), (12, 4, 2), (16, 4, 2), (16, 5, 2), (18, 5, 2)]

# name -> (rows, channels, family, the kernels of a row).  "filt" / "plain": the two members of a Variant; "rag": k_rlm_fast<RAG> with the pairs
# of the ending sources inside it; "resid": the same kernel without them, and k_rlm_resid behind it
TABLES = {
    "fast": (FAST, 2, "fast", ("filt", "plain")),
    "fast1": (FAST1, 1, "fast", ("filt", "plain")),
    "wave": (WAVE, 2, "wave", ("filt", "plain")),
    "wave1": (WAVE1, 1, "wave", ("filt", "plain")),
    "rag": (RAG, 2, "rag", ("rag", "resid")),
    "rag1": (RAG1, 1, "rag", ("rag",)),
}
# where a table's rows stand in the sources: (file under rodio_amd/csrc, instance macro, rows the macro's arguments leave out)
SOURCES = {
    "fast": [("rh_pipeline_fast_lo.hip", "RH_FAST"), ("rh_pipeline_fast_hi.hip", "RH_FAST")],
    "fast1": [("rh_pipeline_fast1.hip", "RH_FAST1")],
    "wave": [("rh_pipeline_wave.hip", "RH_WAVE")],
    "wave1": [("rh_pipeline_wave.hip", "RH_WAVE1")],
    "rag": [("rh_pipeline_wave.hip", "RH_RAG")],  # RH_RAG(r, kv): NS = 2
    "rag1": [("rh_pipeline_wave.hip", "RH_RAG1")],  # RH_RAG1(r, kv): NS = 2
}

# the rate pairs a case is chosen from, in this order
RATES = [(44100, 48000), (48000, 48000), (48000, 44100), (96000, 48000), (192000, 44100), (32000, 48000)]
S = 5  # sources of a case: more than any ring has stages, so every ring wraps


# ---- the selection, mirrored ------------------------------------------------------------------------------------------------------------------
def reduced(frm, to):
    g = gcd(frm, to)
    return frm // g, to // g


def kv_needed(L, F, T, channels):
    """rh_pipeline_internal.h: KiB (64 lanes x 16 bytes) a stage must hold for a tile of L output frames."""
    fb = 4 * channels
    vf = 16 // fb
    span = ((L + 1) * F) // T + 5 + (128 // fb - 2)
    nvec = span // vf + 2
    return (nvec + 63) // 64


def find_variant(rows, R, need, NS):
    """find_variant: the row with this R and NS and the smallest KV >= need, or None."""
    best = None
    for r, kv, ns in rows:
        if r == R and ns == NS and kv >= need and (best is None or kv < best[1]):
            best = (r, kv, ns)
    return best


def select(table, R, NS, frm, to):
    """The row of `table` a handle with frames_per_lane = R, ring_stages = NS takes at these rates."""
    rows, ch = TABLES[table][:2]
    F, T = reduced(frm, to)
    return find_variant(rows, R, kv_needed(64 * R, F, T, ch), NS)


def fast_table_of(table):
    return "fast" if TABLES[table][1] == 2 else "fast1"


class Case:
    """What makes the library run `row` of `table`: the rates, the channel count, the family (fast: S sources of one length; wave, rag: the
    ragged shape) and the kernels of the row."""

    def __init__(self, table, row, frm, to):
        rows, ch, family, kernels = TABLES[table]
        self.table, self.row, self.frm, self.to, self.ch, self.family, self.kernels = table, tuple(row), frm, to, ch, family, kernels
        self.R, self.KV, self.NS = self.row
        self.S = S

    def __repr__(self):
        return f"{self.table}-R{self.R}-KV{self.KV}-NS{self.NS}-{self.frm}to{self.to}"


def case_of(table, row):
    """The first rate pair of RATES at which (R, NS) selects exactly `row` -- and, for the ragged tables, at which the fast plan every handle
    builds first has an instance with that (R, NS) too (rh_rlm_create refuses a stereo handle otherwise, and re-plans a mono one)."""
    R, _, NS = row
    for frm, to in RATES:
        if select(table, R, NS, frm, to) != tuple(row):
            continue
        if TABLES[table][2] != "fast" and select(fast_table_of(table), R, NS, frm, to) is None:
            continue
        return Case(table, row, frm, to)
    raise LookupError(f"no rate pair of {RATES} selects {row} of {table}")


# ---- the shapes -----------------------------------------------------------------------------------------------------------------------------
def out_frames(n, frm, to):
    """Output frames of n input frames (run_out_frames, rh_resample.hip): every m with floor(m F / T) <= n - 2, and the verbatim last frame
    when an output frame lands on it."""
    F, T = reduced(frm, to)
    if n == 0:
        return 0
    if F == T:
        return n
    c1 = ((n - 1) * T + F - 1) // F
    return c1 + (1 if c1 * F < n * T else 0)


def whole_tiles(lookback_tiles):
    return max(6, lookback_tiles + 2)


def _frames_for(m_want, frm, to, ok=lambda m: True):
    """The fewest input frames that give at least m_want output frames with ok(output frames)."""
    F, T = reduced(frm, to)
    n = max(2, m_want * F // T - 2)
    while out_frames(n, frm, to) < m_want or not ok(out_frames(n, frm, to)):
        n += 1
    return n


def equal_frames(case, lookback_tiles):
    """Input frames of every source of an equal-length batch: max(6, lookback_tiles + 2) whole tiles of 64 R output frames, then a partial
    tile (about a third of one), and an output that is no multiple of 4 frames."""
    L = 64 * case.R
    return _frames_for(whole_tiles(lookback_tiles) * L + L // 3, case.frm, case.to, lambda m: m % 4 != 0 and m % L != 0)


def ragged_frames(case, lookback_tiles):
    """Input frames of the S sources of a ragged batch: three of N frames (the longest share one length: pair_ok), one that ends in the
    middle of a tile about 1.5 tiles before the end of the mix (so the tiles around it hold a source that is about to end), and one of
    about half the length."""
    L = 64 * case.R
    N = equal_frames(case, lookback_tiles)
    M = out_frames(N, case.frm, case.to)
    near = _frames_for(M - L - L // 2, case.frm, case.to, lambda m: m % L not in (0, L - 1))
    ns = [N, near, N, N // 2 + 1, N]
    assert out_frames(near, case.frm, case.to) < M - L and out_frames(N // 2 + 1, case.frm, case.to) < M
    return ns
