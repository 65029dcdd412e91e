"""The held gate (include/mbx_hold.h): the numpy definition of the gated mix-down with memory -- ``step(pcm16, bus_offset, src_row,
gain_q12, form, hold, state) -> (out, state)``: one frame of the buses under a hold (hysteresis, hang time, the N loudest, ramps of
1 .. 128 samples) and the state after it, int64 inside, on top of ``levels.measure`` --, the constants and structures of the header,
and a small wrapper of the native state object.  The tests hold the library to this module; nothing here runs on the hot path (the
decisions are ``hold_decide_kernel`` / ``hold_long_kernel`` on the device, the sums ``hold_sum_kernel`` / ``hold_long_kernel``:
``BatchDecoder.mixdown_held``, ``mbx_session_next_mixdown_held``)."""
import ctypes as C

import numpy as np

from . import _native, levels, mixdown, pcm8

MAX_RAMP_LOG2 = 7   # MBX_HOLD_MAX_RAMP_LOG2: fades of at most 128 samples

# mbx_gate_input_state: 4 bytes, all zero is closed
STATE_DTYPE = np.dtype([("hang_left", "<u2"), ("open", "u1"), ("on", "u1")])
assert STATE_DTYPE.itemsize == 4

OFF, STEADY, RISING, FALLING = 0, 1, 2, 3   # what an input does in a frame, from (on before, on now)


class Hold(C.Structure):
    """mbx_mixdown_hold"""
    _fields_ = [("open_peak", C.c_uint16), ("close_peak", C.c_uint16), ("hang_frames", C.c_uint16), ("loudest_n", C.c_uint8), ("ramp_log2", C.c_uint8)]

    def astuple(self):
        return (self.open_peak, self.close_peak, self.hang_frames, self.loudest_n, self.ramp_log2)


def _fields(hold):
    open_peak, close_peak, hang_frames, loudest_n, ramp_log2 = (int(v) for v in (hold.astuple() if isinstance(hold, Hold) else hold))
    if not 0 <= open_peak <= levels.MAX_PEAK:
        raise ValueError("open_peak is 0 .. 32768")
    if not 0 <= close_peak <= open_peak:
        raise ValueError("close_peak is 0 .. open_peak")
    if not 0 <= hang_frames <= 0xFFFF:
        raise ValueError("hang_frames is a uint16")
    if not 0 <= loudest_n <= levels.GATE_MAX_LOUDEST:
        raise ValueError("loudest_n is 0 .. GATE_MAX_LOUDEST")
    if not 0 <= ramp_log2 <= MAX_RAMP_LOG2:
        raise ValueError("ramp_log2 is 0 .. MAX_RAMP_LOG2")
    return open_peak, close_peak, hang_frames, loudest_n, ramp_log2


def zero_state(inputs):
    return np.zeros(int(inputs), dtype=STATE_DTYPE)


def check_state(state):
    st = np.asarray(state)
    if st.dtype != STATE_DTYPE or st.ndim != 1:
        raise TypeError("state is a 1-d array of STATE_DTYPE")
    if (st["open"] > 1).any() or (st["on"] > 1).any() or (st["on"] > st["open"]).any():
        raise ValueError("a state record whose open or on is not 0 or 1, or that is on without open")
    return st


def decide(lv, bus_offset, src_row, hold, state):
    """The state after this frame (STATE_DTYPE per input) from the level records of the rows and the state before it."""
    open_peak, close_peak, hang_frames, loudest_n, _ = _fields(hold)
    st = check_state(state)
    off = np.ascontiguousarray(bus_offset, dtype=np.int64).reshape(-1)
    row = np.ascontiguousarray(src_row, dtype=np.int64).reshape(-1)[:int(off[-1])]
    if st.size != int(off[-1]):
        raise ValueError("state holds one record per input")
    peak = lv["peak"][row].astype(np.int64)
    energy = lv["energy"][row].astype(np.int64)
    was_open, hang_was = st["open"].astype(bool), st["hang_left"].astype(np.int64)
    fresh = (peak >= open_peak) | (was_open & (peak >= close_peak))
    hung = ~fresh & was_open & (hang_was > 0)
    new = np.zeros(st.size, dtype=STATE_DTYPE)
    new["open"] = fresh | hung
    new["hang_left"] = np.where(fresh, hang_frames, np.where(hung, hang_was - 1, 0))
    on = new["open"].astype(bool)
    if loudest_n:
        on = np.zeros(st.size, dtype=bool)
        for b in range(off.size - 1):
            lo, hi = int(off[b]), int(off[b + 1])
            is_open = new["open"][lo:hi].astype(bool)
            # the open inputs, loudest first; a stable sort keeps the earlier position in front at equal energy
            order = [k for k in np.argsort(-energy[lo:hi], kind="stable") if is_open[k]][:loudest_n]
            on[lo + np.array(order, dtype=np.int64)] = True
    new["on"] = on
    return new


def codes(before, after):
    """OFF / STEADY / RISING / FALLING per input from the `on` of two states"""
    was, now = np.asarray(before)["on"].astype(bool), np.asarray(after)["on"].astype(bool)
    return np.where(now, np.where(was, STEADY, RISING), np.where(was, FALLING, OFF))


def weights(code, ramp_log2):
    """q(n), n = 0 .. 159, per input: [inputs, 160] int64"""
    R = 1 << int(ramp_log2)
    up = np.minimum(np.arange(160, dtype=np.int64) + 1, R)
    table = np.stack([np.zeros(160, dtype=np.int64), np.full(160, R, dtype=np.int64), up, R - up])
    return table[np.asarray(code, dtype=np.int64)]


def step(pcm16, bus_offset, src_row, gain_q12, form, hold, state):
    """One frame: int16 rows [rows, 160] and the state before it -> (the buses [n_buses, 160] in `form`, the state after it).
    term = (x * gain + 2048) >> 12; ramped = (term * q(n) + R / 2) >> ramp_log2 (floors); the ramped terms of a bus summed, the sum
    clamped to int16 once, then the form."""
    if form not in mixdown.FORMS:
        raise ValueError("form is PCM16 (0), ULAW (1) or ALAW (2)")
    ramp_log2 = _fields(hold)[4]
    x = np.asarray(pcm16)
    off, row, gain = mixdown._arrays(bus_offset, src_row, gain_q12)
    n = int(off[-1])
    if n and int(row[:n].max()) >= x.shape[0]:
        raise ValueError("a src_row beyond the rows of pcm16")
    new = decide(levels.measure(x), off, row, hold, state)
    q = weights(codes(state, new), ramp_log2)
    g = np.full(n, mixdown.UNITY, dtype=np.int64) if gain is None else gain[:n].astype(np.int64)
    term = (x.astype(np.int64)[row[:n]] * g[:, None] + 2048) >> 12
    ramped = (term * q + ((1 << ramp_log2) >> 1)) >> ramp_log2
    acc = np.zeros((off.size - 1, 160), dtype=np.int64)
    for b in range(off.size - 1):
        acc[b] = ramped[int(off[b]):int(off[b + 1])].sum(axis=0)
    y = np.clip(acc, -32768, 32767).astype(np.int16)
    return (y if form == mixdown.PCM16 else pcm8.compand(y, pcm8.LAW_ULAW if form == mixdown.ULAW else pcm8.LAW_ALAW)), new


class GateState:
    """A native gate state (mbx_gate_state_create): one record per input of `plan` (a mixdown.Plan) on the current device, zeroed.
    Owns the native handle; the plan must outlive it."""

    def __init__(self, plan):
        self.handle = None
        h = C.c_void_p()
        _native.check(_native.lib().mbx_gate_state_create(C.byref(h), plan.handle), "mbx_gate_state_create")
        self.handle = h
        self.inputs = _native.lib().mbx_gate_state_inputs(h)

    def get(self, stream=None):
        out = zero_state(self.inputs)
        _native.check(_native.lib().mbx_gate_state_get(self.handle, out.ctypes.data if out.size else None, stream), "mbx_gate_state_get")
        return out

    def set(self, state, stream=None):
        st = np.ascontiguousarray(state, dtype=STATE_DTYPE).reshape(-1)
        if st.size != self.inputs:
            raise ValueError("state holds one record per input of the plan")
        _native.check(_native.lib().mbx_gate_state_set(self.handle, st.ctypes.data if st.size else None, stream), "mbx_gate_state_set")

    def reset(self, stream=None):
        _native.check(_native.lib().mbx_gate_state_reset(self.handle, stream), "mbx_gate_state_reset")

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_gate_state_destroy(self.handle)
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
