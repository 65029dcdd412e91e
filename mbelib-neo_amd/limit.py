"""Limited buses (include/mbx_limit.h): the numpy definition of the look-ahead peak limiter behind the mix-down sums -- ``step(sums, T,
limit, state, form=PCM16) -> (out, state, events)``: the n * T rows of a call limited, the records after it and what every row did
(where it attacked, a hold, a release slewed, stopped or at unity), int64 inside --, the sums themselves in front of the clamp
(``sums`` / ``sums_gated`` / ``sums_held``: mixdown.mix, levels.mix_gated and hold.step without their last line), the constants and
structures of the header, and a small wrapper of the native state object.  It is the third statement of the arithmetic, beside the
header and mbx_bus_limit_host; the tests hold the library to this module, and nothing here runs on the hot path (that is
``bus_limit_kernel`` and the sums instances of the bus kernels on the device: ``BatchDecoder.bus_limit`` / ``.mixdown_sums`` /
``.mixdown_gated_sums`` / ``.mixdown_held_sums``, ``mbx_session_next_limit``)."""
import ctypes as C

import numpy as np

from . import _native, hold, levels, mixdown, pcm8

UNITY = 32768          # MBX_LIMIT_UNITY_Q15
MIN_CEILING = 1024     # MBX_LIMIT_MIN_CEILING
MAX_CEILING = 32767    # MBX_LIMIT_MAX_CEILING
MAX_HOLD = 255         # the largest hold counter of a record
MAX_RAMP_LOG2 = 7      # MBX_LIMIT_MAX_RAMP_LOG2
RANGE_LOG2 = 22        # MBX_LIMIT_RANGE_LOG2
RANGE = 1 << RANGE_LOG2    # M: the limiter's range, 128 x full scale

# mbx_limit_record: 4 bytes; fresh or reset is {32768, 0}
RECORD_DTYPE = np.dtype([("gain_q15", "<u2"), ("hold_left", "<u2")])
assert RECORD_DTYPE.itemsize == 4

ATTACK, HELD, RELEASE_SLEWED, RELEASE_STOPPED, IDLE = 0, 1, 2, 3, 4   # what a row did to the gain (IDLE: at unity, nothing to do)


class Limit(C.Structure):
    """mbx_limit"""
    _fields_ = [("ceiling", C.c_uint16), ("release_q8", C.c_uint8), ("hold_frames", C.c_uint8), ("ramp_log2", C.c_uint8), ("zero", C.c_uint8 * 3)]

    def astuple(self):
        return (self.ceiling, self.release_q8, self.hold_frames, self.ramp_log2, self.zero[0] | self.zero[1] | self.zero[2])


def _fields(limit):
    t = tuple(int(v) for v in (limit.astuple() if isinstance(limit, Limit) else limit))
    ceiling, release, hold_frames, ramp, zero = t if len(t) == 5 else t + (0,)
    if not MIN_CEILING <= ceiling <= MAX_CEILING:
        raise ValueError("ceiling is 1024 .. 32767")
    if not (0 <= release <= 255 and 0 <= hold_frames <= 255):
        raise ValueError("release_q8 and hold_frames are uint8")
    if not 0 <= ramp <= MAX_RAMP_LOG2:
        raise ValueError("ramp_log2 is 0 .. MAX_RAMP_LOG2")
    if zero != 0:
        raise ValueError("the zero bytes are not 0")
    return ceiling, release, hold_frames, ramp


def fresh_state(n):
    st = np.zeros(int(n), dtype=RECORD_DTYPE)
    st["gain_q15"] = UNITY
    return st


def check_state(state):
    st = np.asarray(state)
    if st.dtype != RECORD_DTYPE or st.ndim != 1:
        raise TypeError("state is a 1-d array of RECORD_DTYPE")
    if (st["gain_q15"] < 1).any() or (st["gain_q15"] > UNITY).any() or (st["hold_left"] > MAX_HOLD).any():
        raise ValueError("a state record whose gain_q15 is 0 or above 32768, or whose hold_left is above 255")
    return st


def step(sums, T, limit, state, form=mixdown.PCM16, detail=None):
    """int32 rows [n * T, 160], bus-major, and the records before them -> (the limited rows in `form`, the records after them, an event
    code per row [n * T]).  Row i * T + t is frame t of bus i and uses record i.  Per row: s' = clamp(s, -M, M), a = |s'|, P = max a;
    need = 32768 if P <= ceiling else (ceiling << 15) // P; thr0 = (ceiling << 15) // g0; n* = the first n with a[n] > thr0, else 160.
    n* < 160 is an ATTACK: g1 = need, h1 = hold_frames, g(n) = g1 + (((g0 - g1) * clamp(n* - n, 0, R)) >> ramp_log2).  Otherwise a
    hold counter above 0 counts down with the gain held, else g1 = min(need, g0 + (((32768 - g0) * release + 255) >> 8)); g(n) = g0 +
    (((g1 - g0) * min(n + 1, R)) >> ramp_log2).  y = (s' * g(n) + 16384) >> 15 (a floor): no clamp behind it.
    detail: a list that receives one dict per row (n_star, need, g0, g1, h0, h1, peak, product: the largest |s' * g(n)|)."""
    ceiling, release, hold_frames, ramp = _fields(limit)
    if form not in mixdown.FORMS:
        raise ValueError("form is PCM16 (0), ULAW (1) or ALAW (2)")
    T = int(T)
    x = np.ascontiguousarray(sums)
    if x.dtype != np.int32 or x.ndim != 2 or x.shape[1] != 160 or T < 0 or (T and x.shape[0] % T) or (T == 0 and x.shape[0]):
        raise ValueError("sums is int32 [n * T, 160]")
    n = x.shape[0] // T if T else 0
    st = check_state(state).copy()
    if st.size < n:
        raise ValueError("n is above the records of the state")
    clamped = np.clip(x.astype(np.int64), -RANGE, RANGE)
    y = np.empty(x.shape, dtype=np.int16)
    events = np.empty(n * T, dtype=np.int64)
    R = 1 << ramp
    at = np.arange(160, dtype=np.int64)
    C15 = ceiling << 15
    for i in range(n):
        g0, h0 = int(st["gain_q15"][i]), int(st["hold_left"][i])
        for t in range(T):
            row = clamped[i * T + t]
            a = np.abs(row)
            P = int(a.max())
            need = UNITY if P <= ceiling else C15 // P
            above = np.flatnonzero(a > C15 // g0)
            n_star = int(above[0]) if above.size else 160
            assert (n_star < 160) == (need < g0), "the attack condition is need < g0"
            if n_star < 160:
                g1, h1, event = need, hold_frames, ATTACK
                g = g1 + (((g0 - g1) * np.clip(n_star - at, 0, R)) >> ramp)
            else:
                if h0 > 0:
                    g1, h1, event = g0, h0 - 1, HELD
                else:
                    risen = g0 + (((UNITY - g0) * release + 255) >> 8)
                    g1, h1 = min(need, risen), 0
                    event = RELEASE_STOPPED if need < risen else (IDLE if g0 == UNITY else RELEASE_SLEWED)
                g = g0 + (((g1 - g0) * np.minimum(at + 1, R)) >> ramp)
            product = row * g
            out = (product + 16384) >> 15
            assert int(np.abs(out).max()) <= ceiling, "|y| <= ceiling"
            y[i * T + t] = out.astype(np.int16)
            events[i * T + t] = event
            if detail is not None:
                detail.append(dict(n_star=n_star, need=need, g0=g0, g1=g1, h0=h0, h1=h1, peak=P, product=int(np.abs(product).max())))
            g0, h0 = g1, h1
        st[i] = (g0, h0)
    out = y if form == mixdown.PCM16 else pcm8.compand(y, pcm8.LAW_ULAW if form == mixdown.ULAW else pcm8.LAW_ALAW)
    return out, st, events


# ---- the sums in front of the clamp: what the sums launches and their host twins deliver, int64 inside, int32 out ------------------------
def sums(pcm16, bus_offset, src_row, gain_q12=None):
    """mixdown.mix without its clamp: int32 [n_buses, 160]"""
    x = np.asarray(pcm16)
    if x.dtype != np.int16 or x.ndim != 2 or x.shape[1] != 160:
        raise TypeError("mix-down takes int16 rows of 160 samples")
    off, row, gain = mixdown._arrays(bus_offset, src_row, gain_q12)
    if off[-1] and int(row[:off[-1]].max()) >= x.shape[0]:
        raise ValueError("a src_row beyond the rows of pcm16")
    x = x.astype(np.int64)
    acc = np.zeros((off.size - 1, 160), dtype=np.int64)
    for b in range(off.size - 1):
        k = slice(int(off[b]), int(off[b + 1]))
        g = np.full(k.stop - k.start, mixdown.UNITY, dtype=np.int64) if gain is None else gain[k].astype(np.int64)
        acc[b] = ((x[row[k]] * g[:, None] + 2048) >> 12).sum(axis=0)
    assert np.abs(acc).max(initial=0) < 2 ** 31
    return acc.astype(np.int32)


def sums_gated(pcm16, bus_offset, src_row, gain_q12=None, open_peak=0, loudest_n=0):
    """levels.mix_gated without its clamp: the gain of every input that is not chosen is 0"""
    off = np.ascontiguousarray(bus_offset, dtype=np.int32).reshape(-1)
    n = int(off[-1])
    gain = np.full(n, mixdown.UNITY, dtype=np.int16) if gain_q12 is None else np.ascontiguousarray(gain_q12, dtype=np.int16).reshape(-1)[:n].copy()
    row = np.ascontiguousarray(src_row, dtype=np.int32).reshape(-1)
    gain[~levels.chosen(levels.measure(pcm16), off, row, open_peak, loudest_n)] = 0
    return sums(pcm16, off, row, gain)


def sums_held(pcm16, bus_offset, src_row, gain_q12, hold_params, state):
    """hold.step without its clamp: (int32 [n_buses, 160], the gate state after the frame)"""
    ramp_log2 = hold._fields(hold_params)[4]
    x = np.asarray(pcm16)
    off, row, gain = mixdown._arrays(bus_offset, src_row, gain_q12)
    n = int(off[-1])
    new = hold.decide(levels.measure(x), off, row, hold_params, state)
    q = hold.weights(hold.codes(state, new), ramp_log2)
    g = np.full(n, mixdown.UNITY, dtype=np.int64) if gain is None else gain[:n].astype(np.int64)
    term = (x.astype(np.int64)[row[:n]] * g[:, None] + 2048) >> 12
    ramped = (term * q + ((1 << ramp_log2) >> 1)) >> ramp_log2
    acc = np.zeros((off.size - 1, 160), dtype=np.int64)
    for b in range(off.size - 1):
        acc[b] = ramped[int(off[b]):int(off[b + 1])].sum(axis=0)
    return acc.astype(np.int32), new


class LimitState:
    """A native limiter state (mbx_limit_state_create): `buses` records on the current device, every one {32768, 0}, and the scratch
    for the sums of as many buses.  Owns the native handle."""

    def __init__(self, buses):
        self.handle = None
        h = C.c_void_p()
        _native.check(_native.lib().mbx_limit_state_create(C.byref(h), int(buses)), "mbx_limit_state_create")
        self.handle = h
        self.buses = _native.lib().mbx_limit_state_buses(h)

    def _range(self, first, count):
        first = int(first)
        return first, self.buses - first if count is None else int(count)

    def sums_ptr(self):
        """the device address of the scratch: buses * 160 int32 (mbx_limit_state_sums)"""
        return _native.lib().mbx_limit_state_sums(self.handle)

    def get(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        out = fresh_state(max(count, 0))
        _native.check(_native.lib().mbx_limit_state_get(self.handle, first, count, out.ctypes.data if out.size else None, stream), "mbx_limit_state_get")
        return out

    def set(self, state, first=0, stream=None):
        st = np.ascontiguousarray(state, dtype=RECORD_DTYPE).reshape(-1)
        _native.check(_native.lib().mbx_limit_state_set(self.handle, int(first), st.size, st.ctypes.data if st.size else None, stream), "mbx_limit_state_set")

    def reset(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        _native.check(_native.lib().mbx_limit_state_reset(self.handle, first, count, stream), "mbx_limit_state_reset")

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_limit_state_destroy(self.handle)
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
