"""The reference of the live filter tests (test_live_filter_cpu.py, test_gpu_live_filter.py): BltFilter's recurrence (blt.rs:559) with a
coefficient entry per SAMPLE, restated in numpy -- f32 in rodio's operation order, or the same recurrence in f64 -- and the inputs the
mode 1 tests share.  Coefficients come from the oracle (oracle.blt_coeffs).  Test infrastructure only."""
import functools

import numpy as np

f32 = np.float32
RATE = 48000


def step_index(first, period, n):
    """Table entry of sample i < n of a block whose first sample is the stream's sample `first`."""
    j = np.arange(n, dtype=np.uint64) + np.uint64(first)
    return (j // np.uint64(period) - np.uint64(first // period)).astype(np.int64)


def steps_needed(first, period, n):
    return (first + n - 1) // period - first // period + 1 if n else 0


def biquad_steps_ref(x, channels, first, period, table, state=None, dtype=np.float32):
    """y, state' of one stream: x interleaved (whole frames), table [steps, 5] = {b0,b1,b2,a1,a2}, state [channels, 4] =
    {x1,x2,y1,y2} (None: zeros).  Every product and sum is rounded to `dtype`, left to right as blt.rs:559 writes them; the channels
    are independent chains, so a frame is one step of arrays [channels]."""
    x = np.asarray(x, f32)
    C = int(channels)
    frames = x.size // C
    assert x.size == frames * C
    table = np.asarray(table, f32).reshape(-1, 5)
    idx = step_index(first, period, x.size)
    assert idx.size == 0 or idx[-1] < table.shape[0]
    co = table[idx].astype(dtype).reshape(frames, C, 5)
    xs = x.astype(dtype).reshape(frames, C)
    st = np.zeros((C, 4), f32) if state is None else np.asarray(state, f32).reshape(C, 4)
    x1, x2, y1, y2 = (st[:, k].astype(dtype) for k in range(4))
    y = np.empty((frames, C), dtype)
    for n in range(frames):
        k, xn = co[n], xs[n]
        r = k[:, 0] * xn
        r = r + k[:, 1] * x1
        r = r + k[:, 2] * x2
        r = r - k[:, 3] * y1
        r = r - k[:, 4] * y2
        y2, x2, y1, x1 = y1, x1, r, xn
        y[n] = r
    out_state = np.stack([x1, x2, y1, y2], axis=1).astype(f32)
    return y.reshape(-1), out_state


def sweep_table(O, kind, f_from, f_to, n_steps, q=0.5, rate=RATE):
    """A geometric sweep of the cutoff over n_steps entries (whole Hz, as to_low_pass takes them)."""
    if n_steps == 1:
        return np.array([O.blt_coeffs(kind, f_from, q, rate)], f32)
    fr = [int(round(f_from * (f_to / f_from) ** (k / (n_steps - 1)))) for k in range(n_steps)]
    return np.array([O.blt_coeffs(kind, f, q, rate) for f in fr], f32)


def noise(seed, n):
    return np.random.default_rng(seed).uniform(-1, 1, n).astype(f32)  # full scale


def mode1_cases(run, tile):
    """name -> (kind, f_from, f_to, q, channels, period U, first, frames): the inputs of the mode 1 tests.  `run` / `tile`: frames a lane owns
    and frames a tile of the kernel (rodio_amd.BIQUAD_STEPS_RUN / _TILE).  The sweeps of the issue's table, at lengths that end inside
    a lane's run, inside a wave and just past a tile; a step boundary at the first and at the last sample of a lane's run."""
    wave = 64 * run
    return {
        "lp_up_in_run": ("low_pass", 100, 8000, 0.5, 2, 480, 0, 2 * tile + 5 * run + 3),
        "lp_down_in_wave": ("low_pass", 8000, 100, 0.5, 2, 480, 240, tile + wave + 17 * run),
        "hp_1000_past_tile": ("high_pass", 1000, 6000, 0.5, 2, 480, 0, 2 * tile + 1),
        "hp_600": ("high_pass", 600, 6000, 0.5, 1, 240, 100, tile + 1),
        "lp_q0707": ("low_pass", 200, 6000, 0.707, 2, 480, 0, tile - 1),
        "stereo_U441": ("low_pass", 100, 8000, 0.5, 2, 441, 220, tile + 2 * wave + 1),
        "six_U1323": ("low_pass", 300, 5000, 0.5, 6, 1323, 0, tile + 3 * run + 1),
        "U1": ("low_pass", 400, 4000, 0.5, 1, 1, 0, 3 * run + 5),
        # mono: a boundary with the first sample of a lane's run (period = 3 runs) and with its last (first = 1)
        "edge_first_of_run": ("low_pass", 100, 8000, 0.5, 1, 3 * run, 0, tile + wave),
        "edge_last_of_run": ("high_pass", 1000, 6000, 0.707, 1, 3 * run, 1, tile + wave),
        "short": ("low_pass", 1000, 2000, 0.5, 2, 4, 0, 5),
        "one_frame": ("high_pass", 1000, 2000, 0.5, 3, 2, 1, 1),
    }


@functools.lru_cache(maxsize=None)
def mode1_case(name, run, tile):
    """(x, channels, first, period, table, y32, y64) of a case, computed once per process and shared (read-only)."""
    from oracle import rodio_oracle as O

    kind, fa, fb, q, C, U, first, frames = mode1_cases(run, tile)[name]
    n = frames * C
    table = sweep_table(O, kind, fa, fb, steps_needed(first, U, n), q)
    x = noise(sorted(mode1_cases(run, tile)).index(name) + 100, n)
    y32, _ = biquad_steps_ref(x, C, first, U, table, dtype=np.float32)
    y64, _ = biquad_steps_ref(x, C, first, U, table, dtype=np.float64)
    for a in (x, table, y32, y64):
        a.setflags(write=False)
    return x, C, first, U, table, y32, y64


# ---- the other inputs that meet mode 1 (the CPU test holds the f32 reference within 5e-6 of the f64 one on each of them) ----------------------
BLOCKS = (1, 777, 8191, 1, 777, 8191, 777)  # frames: the cuts of the carried-state tests
STATE_LAYOUTS = ((2, 441), (3, 1000))       # (channels, period)
STATE_HOWS = ((1,), (1, 0), ("b", 0, 1), (1, "b", 0))  # block b runs through how[b % len(how)]: "b" rh_biquad mode 0, 0 / 1 rh_biquad_steps in that mode


def plateau_table(O, ch, period, n, how):
    """A smooth low_pass sweep whose entries are equal across every block that rh_biquad (one coefficient set per call) takes."""
    table = sweep_table(O, "low_pass", 300, 6000, steps_needed(0, period, n)).copy()
    f0 = 0
    for b, nf in enumerate(BLOCKS):
        if how[b % len(how)] == "b":
            a, e = f0 * ch // period, ((f0 + nf) * ch - 1) // period
            table[a: e + 1] = table[a]
        f0 += nf
    return table


@functools.lru_cache(maxsize=None)
def state_case(ch, period, how):
    """(x, table, y32, state32, y64) of a carried-state case: one pass over the whole stream from a zero state."""
    from oracle import rodio_oracle as O

    x = noise(78 + ch, sum(BLOCKS) * ch)
    table = plateau_table(O, ch, period, x.size, how)
    y32, st32 = biquad_steps_ref(x, ch, 0, period, table)
    y64, _ = biquad_steps_ref(x, ch, 0, period, table, dtype=np.float64)
    return x, table, y32, st32, y64


GUARD_SHAPES = ((1, 2, 5, 0), (1, 2, 1001, 1), (1, 3, 700, 3), (70, 2, 300, 0), (70, 3, 33, 1))  # (streams, channels, frames, lead)
GUARD_PERIOD, GUARD_FIRST = 50, 7


def guard_rows(S):
    return tuple(range(S)) if S == 1 else (0, 63, 64, 69)  # the rows that are compared with the reference


@functools.lru_cache(maxsize=None)
def guard_case(S, ch, frames, s):
    """(x, table, y32, state32, y64) of row s of a guard-zone case."""
    from oracle import rodio_oracle as O

    n = frames * ch
    x = noise(300 + s, n)
    table = sweep_table(O, "low_pass", 400 + s, 5000, steps_needed(GUARD_FIRST, GUARD_PERIOD, n))
    y32, st32 = biquad_steps_ref(x, ch, GUARD_FIRST, GUARD_PERIOD, table)
    y64, _ = biquad_steps_ref(x, ch, GUARD_FIRST, GUARD_PERIOD, table, dtype=np.float64)
    return x, table, y32, st32, y64
