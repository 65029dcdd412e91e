"""Mix-down out (include/mbx_mixdown.h): the numpy definition of the talkgroup buses the library delivers -- ``mix(pcm16, bus_offset,
src_row, gain_q12, form)``, int64 inside --, the constants of the header and a small wrapper of the native plan.  The tests hold the
library to this module; nothing here runs on the hot path (the sum is ``mixdown_kernel`` / ``mixdown_long_kernel`` on the device,
``BatchDecoder.mixdown`` / ``mbx_session_next_mixdown``)."""
import ctypes as C

import numpy as np

from . import _native, pcm8

PCM16 = 0   # MBX_MIXDOWN_PCM16: the buses as int16
ULAW = 1    # MBX_MIXDOWN_ULAW: as G.711 mu-law bytes, silence 0xFF
ALAW = 2    # MBX_MIXDOWN_ALAW: as G.711 A-law bytes, silence 0xD5
FORMS = (PCM16, ULAW, ALAW)
UNITY = 4096        # MBX_MIXDOWN_UNITY: the Q12 gain 1.0
MAX_INPUTS = 4096   # MBX_MIXDOWN_MAX_INPUTS: inputs of one bus
SESSION_MIXDOWN = 16   # MBX_SESSION_MIXDOWN: the outputs bit of mbx_session_create[_mixed]
LONG_ABOVE = 22     # the library's default split (kMixdownLongAbove, csrc/mbx_mixdown_plan.h): buses with more inputs take the long kernel form


def _arrays(bus_offset, src_row, gain_q12):
    off = np.ascontiguousarray(bus_offset, dtype=np.int32).reshape(-1)
    row = np.ascontiguousarray(src_row, dtype=np.int32).reshape(-1)
    gain = None if gain_q12 is None else np.ascontiguousarray(gain_q12, dtype=np.int16).reshape(-1)
    if off.size < 2 or off[0] != 0 or (np.diff(off.astype(np.int64)) < 0).any():
        raise ValueError("bus_offset is [n_buses + 1], starts at 0 and does not decrease")
    if (np.diff(off.astype(np.int64)) > MAX_INPUTS).any():
        raise ValueError("a bus has more than MAX_INPUTS inputs")
    if row.size < off[-1] or (gain is not None and gain.size < off[-1]):
        raise ValueError("src_row and gain_q12 hold bus_offset[-1] inputs")
    if (row[:off[-1]] < 0).any():
        raise ValueError("a negative src_row")
    return off, row, gain


def mix(pcm16, bus_offset, src_row, gain_q12=None, form=PCM16):
    """int16 rows [rows, 160] -> the buses [n_buses, 160]: int16 (PCM16) or uint8 (ULAW, ALAW).  Per sample
    term = (x * gain + 2048) >> 12 (a floor), the terms of a bus summed, the sum clamped to int16 once, then the form."""
    if form not in FORMS:
        raise ValueError("form is PCM16 (0), ULAW (1) or ALAW (2)")
    x = np.asarray(pcm16)
    if x.dtype != np.int16 or x.ndim != 2 or x.shape[1] != 160:
        raise TypeError("mix-down takes int16 rows of 160 samples")
    off, row, gain = _arrays(bus_offset, src_row, gain_q12)
    if off[-1] and int(row[:off[-1]].max()) >= x.shape[0]:
        raise ValueError("a src_row beyond the rows of pcm16")
    x = x.astype(np.int64)
    acc = np.zeros((off.size - 1, 160), dtype=np.int64)
    for b in range(off.size - 1):
        k = slice(int(off[b]), int(off[b + 1]))
        g = np.full(k.stop - k.start, UNITY, dtype=np.int64) if gain is None else gain[k].astype(np.int64)
        acc[b] = ((x[row[k]] * g[:, None] + 2048) >> 12).sum(axis=0)
    y = np.clip(acc, -32768, 32767).astype(np.int16)
    return y if form == PCM16 else pcm8.compand(y, pcm8.LAW_ULAW if form == ULAW else pcm8.LAW_ALAW)


def out_dtype(form):
    return np.int16 if form == PCM16 else np.uint8


class Plan:
    """A native mix-down plan (mbx_mixdown_plan_create[_split]): the buses checked on the host, their tables on the current device,
    which must have been initialised (decoder.ensure_init).  Owns the native handle; immutable.  long_above: buses with more inputs
    take the long kernel form; None: the library's default."""

    def __init__(self, bus_offset, src_row, gain_q12=None, long_above=None):
        self.handle = None
        off = np.ascontiguousarray(bus_offset, dtype=np.int32).reshape(-1)
        row = np.ascontiguousarray(src_row, dtype=np.int32).reshape(-1)
        gain = None if gain_q12 is None else np.ascontiguousarray(gain_q12, dtype=np.int16).reshape(-1)
        if off.size < 1 or (off.size > 1 and (row.size < off.max() or (gain is not None and gain.size < off.max()))):
            raise ValueError("bus_offset is [n_buses + 1]; src_row and gain_q12 hold bus_offset[-1] inputs")
        L = _native.lib()
        h = C.c_void_p()
        args = (C.byref(h), off.size - 1, off.ctypes.data, row.ctypes.data if row.size else None, None if gain is None else gain.ctypes.data)
        if long_above is None:
            _native.check(L.mbx_mixdown_plan_create(*args), "mbx_mixdown_plan_create")
        else:
            _native.check(L.mbx_mixdown_plan_create_split(*args, int(long_above)), "mbx_mixdown_plan_create_split")
        self.handle = h
        self.buses = L.mbx_mixdown_plan_buses(h)
        self.rows = L.mbx_mixdown_plan_rows(h)
        self.long_buses = L.mbx_mixdown_plan_long_buses(h)

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_mixdown_plan_destroy(self.handle)
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
