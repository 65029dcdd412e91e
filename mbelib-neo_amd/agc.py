"""Levelled rows (include/mbx_agc.h): the numpy definition of the per-stream automatic gain control -- ``step(pcm16, T, agc, state,
stream_index=None) -> (out, state, events)``: the n * T rows of a call levelled, the state after it and what every row did (freeze,
hold, fall, a slewed rise, a rise that reached the wanted gain), int64 inside --, the constants and structures of the header, and a
small wrapper of the native state object.  The tests hold the library to this module; nothing here runs on the hot path (that is
``pcm_agc_kernel`` on the device: ``BatchDecoder.agc``, ``mbx_session_next_agc``)."""
import ctypes as C

import numpy as np

from . import _native

UNITY = 1024          # MBX_AGC_UNITY_Q10
MAX_GAIN = 32768      # MBX_AGC_MAX_GAIN_Q10
MAX_PEAK = 32768      # the largest peak a row can have, and the largest envelope
MAX_RAMP_LOG2 = 7     # MBX_AGC_MAX_RAMP_LOG2

# mbx_agc_record: 4 bytes; fresh or reset is {1024, 0}
RECORD_DTYPE = np.dtype([("gain_q10", "<u2"), ("env", "<u2")])
assert RECORD_DTYPE.itemsize == 4

FREEZE, HOLD, FALL, RISE_SLEWED, RISE_REACHED = 0, 1, 2, 3, 4   # what a row did to the gain
PASSED = 5                                                       # a row of an entry whose record is outside the state: passed through


class Agc(C.Structure):
    """mbx_agc"""
    _fields_ = [("target_peak", C.c_uint16), ("floor_peak", C.c_uint16), ("min_gain_q10", C.c_uint16), ("max_gain_q10", C.c_uint16),
                ("release_q8", C.c_uint8), ("rise_q8", C.c_uint8), ("ramp_log2", C.c_uint8), ("zero", C.c_uint8)]

    def astuple(self):
        return (self.target_peak, self.floor_peak, self.min_gain_q10, self.max_gain_q10, self.release_q8, self.rise_q8, self.ramp_log2, self.zero)


def _fields(agc):
    t = tuple(int(v) for v in (agc.astuple() if isinstance(agc, Agc) else agc))
    target, floor, gmin, gmax, release, rise, ramp, zero = t if len(t) == 8 else t + (0,)
    if not 1 <= target <= 32767:
        raise ValueError("target_peak is 1 .. 32767")
    if not 1 <= floor <= MAX_PEAK:
        raise ValueError("floor_peak is 1 .. 32768")
    if not (1 <= gmin <= MAX_GAIN and 1 <= gmax <= MAX_GAIN):
        raise ValueError("min_gain_q10 and max_gain_q10 are 1 .. 32768")
    if gmin > gmax:
        raise ValueError("min_gain_q10 is above max_gain_q10")
    if not (0 <= release <= 255 and 0 <= rise <= 255):
        raise ValueError("release_q8 and rise_q8 are uint8")
    if not 0 <= ramp <= MAX_RAMP_LOG2:
        raise ValueError("ramp_log2 is 0 .. MAX_RAMP_LOG2")
    if zero != 0:
        raise ValueError("the zero field is not 0")
    return target, floor, gmin, gmax, release, rise, ramp


def fresh_state(n):
    st = np.zeros(int(n), dtype=RECORD_DTYPE)
    st["gain_q10"] = UNITY
    return st


def check_state(state):
    st = np.asarray(state)
    if st.dtype != RECORD_DTYPE or st.ndim != 1:
        raise TypeError("state is a 1-d array of RECORD_DTYPE")
    if (st["gain_q10"] < 1).any() or (st["gain_q10"] > MAX_GAIN).any() or (st["env"] > MAX_PEAK).any():
        raise ValueError("a state record whose gain_q10 is 0 or above 32768, or whose env is above 32768")
    return st


def step(pcm16, T, agc, state, stream_index=None):
    """int16 rows [n * T, 160], stream-major, and the state before them -> (the levelled rows, the state after them, an event code per
    row [n * T]).  Entry i uses record stream_index[i] (None: i); an entry outside the state is passed through and touches no record.
    Per row: p = max |x| in int64; below floor_peak the state freezes; else env = max(p, env - ((env * release + 255) >> 8)),
    want = clamp((target << 10) // env, min_gain, max_gain), the gain falls at once and rises by at most (g * rise + 255) >> 8;
    g(n) = g0 + (((g1 - g0) * min(n + 1, R)) >> ramp_log2); y = clamp((x * g(n) + 512) >> 10) (floors)."""
    target, floor, gmin, gmax, release, rise, ramp = _fields(agc)
    T = int(T)
    x = np.ascontiguousarray(pcm16)
    if x.dtype != np.int16 or x.ndim != 2 or x.shape[1] != 160 or T < 0 or (T and x.shape[0] % T) or (T == 0 and x.shape[0]):
        raise ValueError("pcm16 is int16 [n * T, 160]")
    n = x.shape[0] // T if T else 0
    st = check_state(state).copy()
    index = np.arange(n, dtype=np.int64) if stream_index is None else np.ascontiguousarray(stream_index, dtype=np.int64).reshape(-1)
    if index.size != n:
        raise ValueError("stream_index has one entry per stream of the call")
    wide = x.astype(np.int64)
    out = np.empty_like(x)
    events = np.empty(n * T, dtype=np.int64)
    up = np.minimum(np.arange(160, dtype=np.int64) + 1, 1 << ramp)
    for i in range(n):
        r = int(index[i])
        owns = 0 <= r < st.size
        g0, env = (int(st["gain_q10"][r]), int(st["env"][r])) if owns else (UNITY, 0)
        for t in range(T):
            row = wide[i * T + t]
            p = int(np.abs(row).max())
            if not owns:
                g1, event = g0, PASSED
            elif p < floor:
                g1, event = g0, FREEZE
            else:
                env = max(p, env - ((env * release + 255) >> 8))
                want = min(max((target << 10) // env, gmin), gmax)
                if want <= g0:
                    g1, event = want, (HOLD if want == g0 else FALL)
                else:
                    slewed = g0 + ((g0 * rise + 255) >> 8)
                    g1, event = (want, RISE_REACHED) if want <= slewed else (slewed, RISE_SLEWED)
            g = g0 + (((g1 - g0) * up) >> ramp)
            out[i * T + t] = np.clip((row * g + 512) >> 10, -32768, 32767).astype(np.int16)
            events[i * T + t] = event
            g0 = g1
        if owns:
            st[r] = (g0, env)
    return out, st, events


class AgcState:
    """A native AGC state (mbx_agc_state_create): `streams` records on the current device, every one {1024, 0}.  Owns the native handle."""

    def __init__(self, streams):
        self.handle = None
        h = C.c_void_p()
        _native.check(_native.lib().mbx_agc_state_create(C.byref(h), int(streams)), "mbx_agc_state_create")
        self.handle = h
        self.streams = _native.lib().mbx_agc_state_streams(h)

    def _range(self, first, count):
        first = int(first)
        return first, self.streams - first if count is None else int(count)

    def get(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        out = fresh_state(max(count, 0))
        _native.check(_native.lib().mbx_agc_state_get(self.handle, first, count, out.ctypes.data if out.size else None, stream), "mbx_agc_state_get")
        return out

    def set(self, state, first=0, stream=None):
        st = np.ascontiguousarray(state, dtype=RECORD_DTYPE).reshape(-1)
        _native.check(_native.lib().mbx_agc_state_set(self.handle, int(first), st.size, st.ctypes.data if st.size else None, stream), "mbx_agc_state_set")

    def reset(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        _native.check(_native.lib().mbx_agc_state_reset(self.handle, first, count, stream), "mbx_agc_state_reset")

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_agc_state_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
