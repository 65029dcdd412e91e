"""The frame script of the levelled-rows suites (include/mbx_agc.h), shared by tests/test_agc_host.py and tests/test_gpu_agc.py: 8
streams x 24 frames of scripted amplitudes under two parameter sets, every ramp_log2 0 .. 7 across the parametrisation, and what the
numpy definition (mbelib_neo_amd.agc.step) makes of them -- computed once per (set, ramp_log2) and shared, never changed.

Set "voice" is what a bridge would use: target 8000, floor 200, gains x 1/2 .. x 8, the envelope released by a quarter and the gain
raised by an eighth per frame.  Set "extreme" has every field at an end of its range: target 32767, floor 1, min = max = 32768 (the
only parameters under which a sample of -32768 can meet the gain 32768: a row of peak 32768 is never frozen, and under any
min_gain below 32768 it makes the gain fall in its first sample), release and rise 255.

The streams:
  0  digital silence, then a quiet talker with one frame of comfort noise: freeze on a fresh state and on a raised gain, a slewed
     rise up to max_gain, the rise that reaches it, hold
  1  a hot mobile that backs off: fall to min_gain, the envelope's decay above the peak, a rise, frozen frames, a rise again
  2  levels round floor_peak: the envelope's decay term falls below floor_peak and the peak takes over
  3  a quiet talker, a burst with a row of -32768 in it, quiet again: the fall from a high gain clips inside the ramp
  4  full scale from the first frame, silence, 32767, then speech level
  5  at the target from the first frame: hold on a fresh state
  6  seeded random amplitudes
  7  speech and pauses alternating
"""
import functools

import numpy as np

from mbelib_neo_amd import agc

STREAMS, FRAMES = 8, 24
SETS = {
    "voice": dict(target_peak=8000, floor_peak=200, min_gain_q10=512, max_gain_q10=8192, release_q8=64, rise_q8=32),
    "extreme": dict(target_peak=32767, floor_peak=1, min_gain_q10=32768, max_gain_q10=32768, release_q8=255, rise_q8=255),
}
RAMPS = tuple(range(agc.MAX_RAMP_LOG2 + 1))
CASES = [(name, ramp) for ramp in RAMPS for name in SETS]

# what the script must show, each at least once (coverage())
KINDS = ("freeze-fresh", "freeze-raised", "hold", "fall", "rise-slewed", "rise-reached", "want-at-min", "want-at-max", "decay-wins", "decay-below-floor",
         "saturated-high", "saturated-low", "full-scale-at-top-gain")


def params(name, ramp_log2):
    return agc.Agc(ramp_log2=int(ramp_log2), zero=0, **SETS[name])


def amplitudes():
    rng = np.random.default_rng(2024)
    a = np.zeros((STREAMS, FRAMES), dtype=np.int64)
    a[0] = [0, 0] + [500] * 8 + [100] + [500] * 13
    a[1] = [30000] * 3 + [1000] * 10 + [100] * 2 + [1000] * 9
    a[2] = [250, 210, 205, 199, 250, 300, 220, 201, 200, 199, 1000, 250] * 2
    a[3] = [400] * 12 + [20000, 32768, 20000] + [400] * 9
    a[4] = [32768] * 4 + [0] * 4 + [32767] * 4 + [3000] * 12
    a[5] = [8000] * 24
    a[6] = rng.choice([0, 40, 150, 199, 200, 700, 2500, 8000, 15000, 32767, 32768], size=FRAMES)
    a[7] = [3000, 50] * 12
    return a


@functools.lru_cache(maxsize=None)
def script():
    """int16 [FRAMES, STREAMS, 160]: row (f, s) has the peak amplitudes()[s, f] exactly, at a seeded position and sign"""
    rng = np.random.default_rng(77)
    amp = amplitudes()
    x = np.zeros((FRAMES, STREAMS, 160), dtype=np.int16)
    for f in range(FRAMES):
        for s in range(STREAMS):
            a = int(amp[s, f])
            if a == 0:
                continue
            row = rng.integers(max(-a, -32768), min(a, 32767) + 1, size=160)
            at = int(rng.integers(2, 160))
            row[at] = -a if a == 32768 or rng.integers(0, 2) else a
            row[0], row[1] = a - 1, -(a - 1)   # both signs near full size in the first samples, where a falling gain is still high
            x[f, s] = row
    x.setflags(write=False)
    return x


def rows(first, T):
    """frames first .. first + T - 1 of every stream as the rows of ONE call: stream-major [STREAMS * T, 160]"""
    return np.ascontiguousarray(script()[first:first + T].transpose(1, 0, 2).reshape(STREAMS * T, 160))


@functools.lru_cache(maxsize=None)
def expected(name, ramp_log2):
    """frame by frame from a fresh state: a tuple of (out [STREAMS, 160], state after, events [STREAMS], state before)"""
    a = params(name, ramp_log2)
    st = agc.fresh_state(STREAMS)
    steps = []
    for f in range(FRAMES):
        out, after, events = agc.step(script()[f], 1, a, st)
        for v in (out, after, events):
            v.setflags(write=False)
        steps.append((out, after, events, st))
        st = after
    return tuple(steps)


def coverage(name, ramp_log2):
    """the KINDS the script shows under one parameter set and ramp, from agc.step's events and a restatement of the envelope"""
    p = SETS[name]
    got = set()
    x = script().astype(np.int64)
    for f, (out, after, events, before) in enumerate(expected(name, ramp_log2)):
        for s in range(STREAMS):
            g0, env0 = int(before["gain_q10"][s]), int(before["env"][s])
            peak = int(np.abs(x[f, s]).max())
            e = int(events[s])
            if e == agc.FREEZE:
                assert peak < p["floor_peak"] and after[s] == before[s]
                got.add("freeze-fresh" if (g0, env0) == (agc.UNITY, 0) else "freeze-raised" if g0 > agc.UNITY else "freeze")
                continue
            got.add({agc.HOLD: "hold", agc.FALL: "fall", agc.RISE_SLEWED: "rise-slewed", agc.RISE_REACHED: "rise-reached"}[e])
            decayed = env0 - ((env0 * p["release_q8"] + 255) >> 8)
            if decayed > peak:
                got.add("decay-wins")
            if env0 >= p["floor_peak"] and decayed < p["floor_peak"]:
                got.add("decay-below-floor")
            raw = (p["target_peak"] << 10) // max(peak, decayed)
            if raw < p["min_gain_q10"]:
                got.add("want-at-min")
            if raw > p["max_gain_q10"]:
                got.add("want-at-max")
            g1 = int(after["gain_q10"][s])
            up = np.minimum(np.arange(160) + 1, 1 << ramp_log2)
            g = g0 + (((g1 - g0) * up) >> ramp_log2)
            wide = (x[f, s] * g + 512) >> 10
            if (wide > 32767).any():
                got.add("saturated-high")
            if (wide < -32768).any():
                got.add("saturated-low")
            if ((x[f, s] == -32768) & (g == agc.MAX_GAIN)).any():
                got.add("full-scale-at-top-gain")
    return got
