"""The script of the filtered-rows suites (include/mbx_filter.h), shared by tests/test_filter_host.py and tests/test_gpu_filter.py: the
filters, the rows and what the numpy definition (mbelib_neo_amd.filters.step) makes of them -- computed once per case and shared, never
changed.

The filters, S sections each (S in 1, 2, 4):
  design  filters.highpass(200, S): what a host runs in front of its gain;
  rail    S integrators {16384, 0, 0 | -16384, 0} over rows at +3000, then -3000, then +3000 by call (a little noise on top): every
          section runs into one rail, crosses to the other and back;
  delay   S sections {0, 0, 16384 | 0, 0}: 2 S samples of delay, read across frames and calls;
  corner  S sections {32767, -32768, 0 | 32767, -32768}, both sums of magnitudes at the bound 65535: under the alternating entry ff
          and fb reach -+2 * 32767 * 32768 and acc leaves int32.

The rows of a call of n entries x T frames, three calls in a row (the records carry from call to call): seeded full-scale random
samples; entry 1 (where there is one) alternates -32768 / 32767 sample by sample; entry 3 is the constant 12345, then -32768, then 0 by
call; the last sample and the first of consecutive frames of every even entry are planted at the extremes, so that a state read from
the wrong row or the wrong end shows.  The `rail` rows are their own (above)."""
import functools

import numpy as np

from mbelib_neo_amd import filters

KINDS = ("design", "rail", "delay", "corner")
SECTIONS = (1, 2, 4)
FRAMES = (1, 3)
CALLS = 3
NMAX = 130   # two workgroups of the lane-per-entry kernel and a bit

_SECTION = {"rail": (16384, 0, 0, -16384, 0), "delay": (0, 0, 16384, 0, 0), "corner": (32767, -32768, 0, 32767, -32768)}


def coeffs(kind, S):
    """int64 [S, 5]"""
    if kind == "design":
        return filters.highpass(200, S).coeffs()[:S]
    return np.array([_SECTION[kind]] * S, dtype=np.int64)


def filt(kind, S):
    return filters.Filter.of(coeffs(kind, S))


@functools.lru_cache(maxsize=None)
def rows(kind, T, call):
    """int16 [NMAX * T, 160] of call `call` for NMAX entries, stream-major: entries do not depend on each other, so the first n * T are the
    rows of a call of n entries"""
    rng = np.random.default_rng(2000 + 10 * T + call + (500 if kind == "rail" else 0))
    if kind == "rail":
        x = (rng.integers(-200, 201, size=(NMAX, T, 160)) + (3000, -3000, 3000)[call]).astype(np.int16)
    else:
        x = rng.integers(-32768, 32768, size=(NMAX, T, 160)).astype(np.int16)
        phase = (call * T * 160) & 1
        x[1] = np.where((np.arange(T * 160) + phase) & 1, 32767, -32768).astype(np.int16).reshape(T, 160)
        x[3] = (12345, -32768, 0)[call]
        x[4::2, :, 159] = 32767
        x[4::2, :, 0] = -32768
    out = x.reshape(NMAX * T, 160)
    out.setflags(write=False)
    return out


def call_rows(kind, n, T, call):
    return np.array(rows(kind, T, call)[:n * T])


@functools.lru_cache(maxsize=None)
def expected(kind, S, T):
    """numpy, once, for NMAX entries on a fresh state: per call (rows int16 [NMAX * T, 160], the records after it [NMAX])"""
    c = coeffs(kind, S)
    st = filters.fresh_state(NMAX)
    calls = []
    for k in range(CALLS):
        out, st = filters.step(c, st, T, rows(kind, T, k))
        out.setflags(write=False)
        st.setflags(write=False)
        calls.append((out, st))
    return tuple(calls)
