"""The frame script of the wide-rows suites (include/mbx_resample.h), shared by tests/test_resample_host.py and
tests/test_gpu_resample.py: the filters, the rows and what the numpy definition (mbelib_neo_amd.resample.step) makes of them --
computed once per case and shared, never changed.

The filters: design(L, K) for every L in 2, 3, 4, 6 and K in 2, 16, 32; the HOLD and the DELAY taps of the header; and the RAIL taps --
the hold taps scaled to the bound of the header: taps[p] = taps[p + L] = 32767 and, where K allows a third, taps[p + 2 L] = 1, so that
a phase sums to 65535 (65534 at K = 2) and a row of -32768 drives acc to -65535 * 32768, the corner of the int32 bound, where the final
clamp fires.

The rows of a call of n entries x T frames, three calls in a row (the records carry from call to call): seeded full-scale random
samples; entry 1 (where there is one) is all -32768 in the first call, all 32767 in the second and alternates the two sample by sample
in the third; the last sample and the first of consecutive frames are planted at the extremes, so that a history read from the wrong
row or the wrong end shows."""
import functools

import numpy as np

from mbelib_neo_amd import resample

FACTORS = resample.FACTORS
KS = (2, 16, 32)
CALLS = 3
NMAX = 9


def rail_taps(L, K):
    h = np.zeros(K * L, dtype=np.int16)
    h[:2 * L] = 32767
    if K >= 4:
        h[2 * L:3 * L] = 1
    return h


@functools.lru_cache(maxsize=None)
def taps(kind, L, K):
    h = {"design": resample.design, "hold": resample.hold_taps, "delay": resample.delay_taps, "rail": rail_taps}[kind](L, K)
    h.setflags(write=False)
    return h


def filt(kind, L, K):
    return resample.Resample.of(L, K, taps(kind, L, K))


@functools.lru_cache(maxsize=None)
def rows(T, call):
    """int16 [NMAX * T, 160] of call `call` for NMAX entries, stream-major: entries do not depend on each other, so the first n of them
    are the rows of a call of n entries"""
    rng = np.random.default_rng(1000 + 10 * T + call)
    x = rng.integers(-32768, 32768, size=(NMAX, T, 160)).astype(np.int16)
    x[1] = (-32768, 32767)[call] if call < 2 else np.where(np.arange(160) & 1, 32767, -32768).astype(np.int16)
    x[2::2, :, 159] = 32767
    x[2::2, :, 0] = -32768
    x[3::2, :, 128] = -32768
    out = x.reshape(NMAX * T, 160)
    out.setflags(write=False)
    return out


def call_rows(n, T, call):
    return np.array(rows(T, call)[:n * T])


@functools.lru_cache(maxsize=None)
def expected(kind, L, K, T):
    """numpy, once, for NMAX entries on a fresh state: per call (wide rows int16 [NMAX * T, 160 L], the records after it [NMAX])"""
    rs = (L, K, taps(kind, L, K))
    st = resample.fresh_state(NMAX)
    calls = []
    for c in range(CALLS):
        out, st = resample.step(rs, st, T, rows(T, c))
        out.setflags(write=False)
        calls.append((out, st))
    return tuple(calls)
