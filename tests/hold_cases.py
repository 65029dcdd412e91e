"""The frame script of the held-gate suites (include/mbx_hold.h), shared by tests/test_hold_host.py and tests/test_gpu_hold.py: 12
frames of 300 rows whose loudness has PERSISTENCE, a plan of one bus of every size of the levels suite, tie buses (a row twice, a row
beside its negation) and two planted buses of 2 and of 9 inputs whose rows are written by hand; the holds of the suites; numpy's
answer for every (hold, form), frame by frame, made once and shared read-only; and what each bus SEES under a hold (rising, falling,
steady, hysteresis hold, hang hold, expiry), from numpy alone.

Why persistence: with independent draws per frame the N loudest of a bus of 255 inputs and more never keep a member for two frames,
and no steady input is ever summed under a loudest-N gate.  Here a row's class -- far below close_peak, between the two peaks, above
open_peak, near full range -- is redrawn with probability 0.3 per frame and scaled by a fixed factor of the row."""
import numpy as np

from mbelib_neo_amd import hold, levels, mixdown

FRAMES, ROWS = 12, 300
OPEN, CLOSE, HANG = 900, 500, 2
SIZES = [0, 1, 2, 3, 4, 7, 8, 9, 22, 23, 24, 255, 256, 257, 4096]   # those of test_gpu_levels.SIZES
LOUDEST = (0, 1, 3, 8)
RAMPS = (0, 3, 7)
HOLDS = [(OPEN, CLOSE, HANG, n, r) for n in LOUDEST for r in RAMPS]
CLASS_PEAK = (100, 700, 3000, 27000)   # far below CLOSE | between CLOSE and OPEN | above OPEN | near full range (a factor of 1.2 fits int16)
PLANTED = list(range(290, 299))        # rows written by hand; the random rows are 0 .. 289 and 299
Q, M, L = 0, 1, 2
# the planted rows' classes per frame.  Row 290: opens, stays, is held by the hysteresis (M), by the hang (Q, Q), expires, re-opens.
# Row 291 opens while 290 hangs and is louder than a hanging row: under "the loudest 1" it takes the bus from it.
PLANTED_CLASSES = [
    [L, L, M, Q, Q, Q, Q, L, L, L, Q, Q],
    [Q, Q, Q, L, L, Q, Q, Q, Q, Q, Q, Q],
    [Q, L, L, L, M, M, Q, Q, Q, L, Q, Q],
    [M, M, L, Q, Q, Q, L, L, M, Q, Q, Q],
    [Q, Q, L, L, L, L, L, Q, Q, Q, L, L],
    [L, Q, Q, Q, L, M, M, M, Q, Q, Q, L],
    [Q, Q, Q, Q, Q, L, L, L, L, M, Q, Q],
    [L, L, L, L, L, L, L, L, L, L, L, L],
    [Q, Q, Q, Q, Q, Q, Q, Q, Q, Q, Q, Q],
]
PLANTED_SCALE = [1.0, 0.9, 0.6, 0.55, 0.5, 0.45, 0.4, 0.3, 1.0]   # row 290 is the loudest of the planted when it is loud
KINDS = ("rising", "falling", "steady", "hysteresis", "hang", "expiry")

_MADE = {}


def _frame(rng, cls, factor):
    """rows of the classes `cls`: the magnitudes A * m / 160, m = 1 .. 160, A = the class's peak times the row's factor, in an order
    and with signs drawn anew for every row and frame.  So the peak is exactly A, and the energy depends on A alone: the ranking of
    two rows holds for as long as both keep their class, which is what gives a loudest-N gate a member to keep."""
    amp = np.maximum(1, (np.array(CLASS_PEAK)[cls] * factor).astype(np.int64))
    mag = rng.permuted(np.tile(np.arange(1, 161, dtype=np.int64), (cls.size, 1)), axis=1)
    sign = rng.integers(0, 2, size=(cls.size, 160), dtype=np.int64) * 2 - 1
    return (sign * (amp[:, None] * mag // 160)).astype(np.int16)


def script():
    """(x [FRAMES, ROWS, 160] int16, bus_offset, src_row, gain_q12, sizes): read-only"""
    if "script" not in _MADE:
        rng = np.random.default_rng(2025)
        factor = rng.uniform(0.8, 1.2, size=ROWS)
        factor[PLANTED] = PLANTED_SCALE
        cls = rng.integers(0, 4, size=ROWS)
        x = np.zeros((FRAMES, ROWS, 160), dtype=np.int16)
        for f in range(FRAMES):
            redraw = rng.random(ROWS) < 0.3
            cls = np.where(redraw, rng.integers(0, 4, size=ROWS), cls) if f else cls
            now = cls.copy()
            now[PLANTED] = [c[f] for c in PLANTED_CLASSES]
            x[f] = _frame(rng, now, factor)
            x[f, 11] = np.clip(x[f, 11], -32767, 32767)
            x[f, 10] = -x[f, 11]   # a row beside its negation: equal energies in every frame
        free = np.array([r for r in range(ROWS) if r not in PLANTED])
        sizes = list(SIZES)
        rows = [rng.choice(free, size=n).tolist() for n in sizes]
        extra = [[12] * 6, [10, 11], [11, 10, 5],      # a row six times; a row beside its negation, either first
                 PLANTED[:2], PLANTED]                 # the planted buses of 2 and of 9 inputs
        rows += extra
        sizes += [len(e) for e in extra]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        row = np.array([r for bus in rows for r in bus], dtype=np.int32)
        row[off[SIZES.index(4096)] + 4095] = ROWS - 1
        gain = rng.integers(-5000, 5001, size=row.size, dtype=np.int64).astype(np.int16)
        gain[rng.integers(0, row.size, size=200)] = rng.choice(np.array([-32768, 32767, 4096, 0], dtype=np.int16), size=200)
        gain[off[len(SIZES)]:] = 4096   # the tie buses and the planted buses at unity
        for a in (x, off, row, gain):
            a.setflags(write=False)
        _MADE["script"] = (x, off, row, gain, sizes)
    return _MADE["script"]


def planted_buses():
    """the bus numbers of the planted bus of 2 and of 9 inputs"""
    sizes = script()[4]
    return len(sizes) - 2, len(sizes) - 1


def run(holds, form, state=None):
    """numpy over the script, frame f under holds[f] (or the one hold given for all): [(out, state after)] per frame"""
    x, off, row, gain, _ = script()
    if isinstance(holds, tuple):
        holds = [holds] * FRAMES
    st = hold.zero_state(off[-1]) if state is None else state
    steps = []
    for f, h in enumerate(holds):
        out, st = hold.step(x[f], off, row, gain, form, h, st)
        out.setflags(write=False)
        st.setflags(write=False)
        steps.append((out, st))
    return steps


def expected(h, form):
    """run((h,) * FRAMES, form) from zeroed state, made once per (hold, form) and shared read-only"""
    key = (tuple(h), form)
    if key not in _MADE:
        _MADE[key] = run(tuple(h), form)
    return _MADE[key]


def seen(h):
    """what every bus sees under the hold h over the script, from numpy alone: {kind: bool [n_buses]}"""
    x, off, row, _, sizes = script()
    open_peak, close_peak = h[0], h[1]
    got = {kind: np.zeros(len(sizes), dtype=bool) for kind in KINDS}
    st = hold.zero_state(off[-1])
    for f in range(FRAMES):
        lv = levels.measure(x[f])
        new = hold.decide(lv, off, row, h, st)
        code = hold.codes(st, new)
        peak = lv["peak"][row].astype(np.int64)
        was_open = st["open"].astype(bool)
        per_input = {"rising": code == hold.RISING, "falling": code == hold.FALLING, "steady": code == hold.STEADY,
                     "hysteresis": was_open & (peak >= close_peak) & (peak < open_peak),
                     "hang": was_open & (peak < close_peak) & (st["hang_left"] > 0),
                     "expiry": was_open & (peak < close_peak) & (st["hang_left"] == 0)}
        for kind, hit in per_input.items():
            for b in range(len(sizes)):
                got[kind][b] |= bool(hit[off[b]:off[b + 1]].any())
        st = new
    return got


def hold_of(h):
    return hold.Hold(*h)


def out_dtype(form):
    return mixdown.out_dtype(form)
