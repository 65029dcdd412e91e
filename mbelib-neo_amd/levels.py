"""Levels out and the gated mix-down (include/mbx_levels.h): the numpy definition of the level records the library delivers --
``measure(pcm16)``, int64 inside --, of the inputs a gate chooses -- ``chosen(levels, bus_offset, src_row, open_peak, loudest_n)`` --
and of the gated buses -- ``mix_gated(...)``: ``mixdown.mix`` with the gains of the inputs that are not chosen set to 0 --, and the
constants of the header.  The tests hold the library to this module; nothing here runs on the hot path (the records are
``pcm_levels_kernel`` on the device, the buses ``mixdown_gated_kernel`` / ``mixdown_gated_long_kernel``: ``BatchDecoder.levels`` /
``BatchDecoder.mixdown_gated``, ``mbx_session_next_levels`` / ``mbx_session_next_mixdown_gated``)."""
import ctypes as C

import numpy as np

from . import mixdown

GATE_MAX_LOUDEST = 8   # MBX_GATE_MAX_LOUDEST: the largest loudest_n
SESSION_LEVELS = 32    # MBX_SESSION_LEVELS: the outputs bit of mbx_session_create[_mixed]
MAX_PEAK = 32768       # the largest peak of a row (|-32768|): an open_peak above it is refused

# mbx_row_level: 16 bytes
LEVEL_DTYPE = np.dtype([("energy", "<u8"), ("peak", "<u2"), ("clipped", "<u2"), ("zero", "<u4")])
assert LEVEL_DTYPE.itemsize == 16


class Gate(C.Structure):
    """mbx_mixdown_gate"""
    _fields_ = [("open_peak", C.c_uint16), ("loudest_n", C.c_uint16)]


def _check_gate(open_peak, loudest_n):
    if not 0 <= int(open_peak) <= MAX_PEAK:
        raise ValueError("open_peak is 0 .. 32768")
    if not 0 <= int(loudest_n) <= GATE_MAX_LOUDEST:
        raise ValueError("loudest_n is 0 .. GATE_MAX_LOUDEST")


def measure(pcm16):
    """int16 rows [rows, 160] -> their level records [rows] (LEVEL_DTYPE): energy = the sum of x^2, peak = the largest |x| (32768 for
    -32768), clipped = how many samples are 32767 or -32768."""
    x = np.asarray(pcm16)
    if x.dtype != np.int16 or x.ndim != 2 or x.shape[1] != 160:
        raise TypeError("levels are of int16 rows of 160 samples")
    out = np.zeros(x.shape[0], dtype=LEVEL_DTYPE)
    w = x.astype(np.int64)
    out["energy"] = (w * w).sum(axis=1).astype(np.uint64)
    out["peak"] = np.abs(w).max(axis=1, initial=0).astype(np.uint16)
    out["clipped"] = ((x == 32767) | (x == -32768)).sum(axis=1).astype(np.uint16)
    return out


def chosen(levels, bus_offset, src_row, open_peak=0, loudest_n=0):
    """bool per input: is it summed?  An input is open iff the peak of its row >= open_peak; with loudest_n = N > 0 only the N loudest
    open inputs of each bus are chosen: the larger energy wins, at equal energy the earlier position in the bus."""
    _check_gate(open_peak, loudest_n)
    lv = np.asarray(levels)
    if lv.dtype != LEVEL_DTYPE or lv.ndim != 1:
        raise TypeError("levels is a 1-d array of LEVEL_DTYPE")
    off = np.ascontiguousarray(bus_offset, dtype=np.int64).reshape(-1)
    row = np.ascontiguousarray(src_row, dtype=np.int64).reshape(-1)
    take = np.zeros(int(off[-1]), dtype=bool)
    for b in range(off.size - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        r = row[lo:hi]
        is_open = lv["peak"][r].astype(np.int64) >= int(open_peak)
        if loudest_n:
            energy = lv["energy"][r].astype(np.int64)
            # the open inputs, loudest first; a stable sort keeps the earlier position in front at equal energy
            order = [k for k in np.argsort(-energy, kind="stable") if is_open[k]][:int(loudest_n)]
            take[lo + np.array(order, dtype=np.int64)] = True
        else:
            take[lo:hi] = is_open
    return take


def mix_gated(pcm16, bus_offset, src_row, gain_q12=None, form=mixdown.PCM16, open_peak=0, loudest_n=0):
    """The gated buses: mixdown.mix with the gain of every input that is not chosen set to 0 (a term at gain 0 is 0)."""
    off = np.ascontiguousarray(bus_offset, dtype=np.int32).reshape(-1)
    n = int(off[-1])
    gain = np.full(n, mixdown.UNITY, dtype=np.int16) if gain_q12 is None else np.ascontiguousarray(gain_q12, dtype=np.int16).reshape(-1)[:n].copy()
    row = np.ascontiguousarray(src_row, dtype=np.int32).reshape(-1)
    if n and (int(row[:n].max()) >= np.asarray(pcm16).shape[0] or int(row[:n].min()) < 0):
        raise ValueError("a src_row outside the rows of pcm16")
    gain[~chosen(measure(pcm16), off, row, open_peak, loudest_n)] = 0
    return mixdown.mix(pcm16, off, row, gain, form)
