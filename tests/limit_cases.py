"""The frame script of the limited-buses suites (include/mbx_limit.h), shared by tests/test_limit_host.py and tests/test_gpu_limit.py:
8 buses x 24 frames of scripted int32 sums under two parameter sets, every ramp_log2 0 .. 7 across the parametrisation, and what the
numpy definition (mbelib_neo_amd.limit.step) makes of them -- computed once per (set, ramp_log2) and shared, never changed.

Set "bridge" is what a console would use behind AGC'd talkers: ceiling 24000, a quarter of the distance to unity regained per frame,
two frames of hold.  Set "rails" is the identity's ceiling 32767 with the fastest release and no hold: the only ceiling under which a
sum of -32768 is one LSB too large.

The buses (a row is seeded noise of a background amplitude, with spikes written over it at scripted samples):
  0  digital silence, then quiet speech: all-zero rows, and a limiter that never leaves unity
  1  one spike in sample 0, then speech: an attack with n* = 0, the hold counting to 0, a slewed release
  2  a spike in sample 1, a larger one in the next frame: an attack with 0 < n* < R (R >= 2), an attack on a gain already reduced
  3  spikes in sample 159, then in sample 140: attacks with n* = 159 and with n* >= R at every ramp
  4  a large spike, then a bus that stays hot: the release stopped by need < 32768
  5  sums beyond +-2^22, either sign: the clamp of the limiter's range
  6  full-scale rows with -32768 in them: one LSB above the ceiling 32767
  7  seeded random amplitudes at seeded samples
"""
import functools

import numpy as np

from mbelib_neo_amd import limit

BUSES, FRAMES = 8, 24
SETS = {
    "bridge": dict(ceiling=24000, release_q8=64, hold_frames=2),
    "rails": dict(ceiling=32767, release_q8=255, hold_frames=0),
}
RAMPS = tuple(range(limit.MAX_RAMP_LOG2 + 1))
CASES = [(name, ramp) for ramp in RAMPS for name in SETS]

# what the script must show, each at least once (coverage())
KINDS = ("attack-at-0", "attack-inside-ramp", "attack-beyond-ramp", "attack-at-159", "attack-on-reduced-gain", "hold-to-zero", "release-slewed",
         "release-stopped", "release-reaches-unity", "beyond-range", "minus-32768-under-32767", "all-zero-row")


def params(name, ramp_log2):
    return limit.Limit(ramp_log2=int(ramp_log2), **SETS[name])


def _plan():
    """per bus and frame: (background amplitude, ((sample, value), ...))"""
    quiet = (3000, ())
    p = [[quiet] * FRAMES for _ in range(BUSES)]
    p[0] = [(0, ())] * 2 + [quiet] * 10 + [(0, ())] + [quiet] * 11
    p[1] = [(5000, ((0, 60000),))] + [(5000, ())] * 23
    p[2] = [(4000, ((1, -50000),)), (4000, ((1, 90000),))] + [(4000, ())] * 10 + [(4000, ((1, 70000), (3, -70000)))] + [(4000, ())] * 11
    p[3] = [(6000, ((159, 45000),))] + [quiet] * 2 + [(6000, ((140, -80000), (150, 80000)))] + [quiet] * 8 + [(100, ((159, -32769),))] + [quiet] * 11
    p[4] = [(20000, ((77, 100000),))] + [(40000, ((9, 40000),))] * 15 + [(10000, ())] * 8
    p[5] = [(30000, ((50, 5000000),)), quiet, (30000, ((0, -6000000), (159, 4194304))), quiet, (2000, ((80, -4194305), (81, 4194303)))] + [quiet] * 19
    p[6] = [(20000, ((100, -32768),)), (32767, ((0, -32768), (159, 32767))), (32767, ())] * 8
    return p


@functools.lru_cache(maxsize=None)
def script():
    """int32 [FRAMES, BUSES, 160]"""
    rng = np.random.default_rng(2025)
    x = np.zeros((FRAMES, BUSES, 160), dtype=np.int32)
    plan = _plan()
    for f in range(FRAMES):
        for b in range(BUSES):
            if b == 7:
                bg = int(rng.choice([0, 100, 8000, 23999, 24000, 24001, 32767, 32768, 50000, 300000, 4194304, 9000000]))
                spikes = tuple((int(rng.integers(0, 160)), int(rng.choice([-1, 1])) * bg) for _ in range(2))
                bg = min(bg, 20000)
            else:
                bg, spikes = plan[b][f]
            if bg:
                x[f, b] = rng.integers(-bg, bg + 1, size=160)
            for at, value in spikes:
                x[f, b, at] = value
    x.setflags(write=False)
    return x


def rows(first, T):
    """frames first .. first + T - 1 of every bus as the rows of ONE call: bus-major [BUSES * T, 160]"""
    return np.ascontiguousarray(script()[first:first + T].transpose(1, 0, 2).reshape(BUSES * T, 160))


@functools.lru_cache(maxsize=None)
def expected(name, ramp_log2):
    """frame by frame from a fresh state: a tuple of (out [BUSES, 160] int16, records after, events [BUSES], records before, detail)"""
    p = params(name, ramp_log2)
    st = limit.fresh_state(BUSES)
    steps = []
    for f in range(FRAMES):
        detail = []
        out, after, events = limit.step(script()[f], 1, p, st, detail=detail)
        for v in (out, after, events):
            v.setflags(write=False)
        steps.append((out, after, events, st, tuple(detail)))
        st = after
    return tuple(steps)


def coverage(name, ramp_log2):
    """the KINDS the script shows under one parameter set and ramp, from limit.step's events and details alone"""
    R = 1 << ramp_log2
    got = set()
    x = script()
    for f, (out, after, events, before, detail) in enumerate(expected(name, ramp_log2)):
        for b in range(BUSES):
            d, e = detail[b], int(events[b])
            if e == limit.ATTACK:
                assert d["need"] < d["g0"] and d["g1"] == d["need"] and d["h1"] == SETS[name]["hold_frames"]
                n = d["n_star"]
                got |= {k for k, hit in (("attack-at-0", n == 0), ("attack-inside-ramp", 0 < n < R), ("attack-beyond-ramp", n >= R), ("attack-at-159", n == 159),
                                         ("attack-on-reduced-gain", d["g0"] < limit.UNITY)) if hit}
            else:
                assert d["n_star"] == 160 and d["need"] >= d["g0"]
            if e == limit.HELD and d["h1"] == 0:
                got.add("hold-to-zero")
            if e == limit.RELEASE_SLEWED:
                got.add("release-reaches-unity" if d["g1"] == limit.UNITY else "release-slewed")
            if e == limit.RELEASE_STOPPED:
                assert d["g1"] == d["need"] < limit.UNITY
                got.add("release-stopped")
            if (np.abs(x[f, b].astype(np.int64)) > limit.RANGE).any():
                got.add("beyond-range")
            if SETS[name]["ceiling"] == 32767 and (x[f, b] == -32768).any():
                got.add("minus-32768-under-32767")
            if not x[f, b].any():
                assert out[b].tolist() == [0] * 160
                got.add("all-zero-row")
    return got
