"""Companded PCM out (include/mbx_pcm8.h): the numpy definition of the G.711 bytes the library delivers -- ``ulaw(x)`` and
``alaw(x)`` for int16 samples -- and the two standard 256-entry expansion tables.  The tests hold the library to this module;
nothing here runs on the hot path (the conversion is ``pcm_compand_kernel`` on the device, ``BatchDecoder.compand`` /
``mbx_session_next_pcm8``)."""
import numpy as np

LAW_ULAW = 0
LAW_ALAW = 1
SESSION_PCM8 = 8   # MBX_SESSION_PCM8: the outputs bit of mbx_session_create[_mixed]


def _log2(m):
    """floor(log2 m) of positive integers, exactly (the exponent of the float, not a logarithm)."""
    return np.frexp(m.astype(np.float64))[1].astype(np.int32) - 1


def _samples(x):
    x = np.asarray(x)
    if x.dtype != np.int16:
        raise TypeError("companding takes int16 samples")
    return x.astype(np.int32)


def ulaw(x):
    """int16 samples -> mu-law bytes (the classic linear2ulaw on the 14-bit value), any shape."""
    v = _samples(x) >> 2
    neg = v < 0
    m = np.minimum(np.where(neg, -v, v), 8159) + 33
    seg = _log2(m) - 5
    code = np.where(seg == 8, 0x7F, (seg << 4) | ((m >> (seg + 1)) & 15))
    return (code ^ np.where(neg, 0x7F, 0xFF)).astype(np.uint8)


def alaw(x):
    """int16 samples -> A-law bytes (the classic linear2alaw on the 13-bit value), any shape."""
    v = _samples(x) >> 3
    neg = v < 0
    m = np.where(neg, -v - 1, v)
    seg = np.where(m < 32, 0, _log2(np.maximum(m, 1)) - 4)
    code = (seg << 4) | ((m >> np.where(seg < 2, 1, seg)) & 15)
    return (code ^ np.where(neg, 0x55, 0xD5)).astype(np.uint8)


def compand(x, law):
    if law not in (LAW_ULAW, LAW_ALAW):
        raise ValueError("law is LAW_ULAW (0) or LAW_ALAW (1)")
    return alaw(x) if law == LAW_ALAW else ulaw(x)


def _ulaw_expand():
    u = ~np.arange(256, dtype=np.int32) & 0xFF
    t = (((u & 0x0F) << 3) + 0x84) << ((u & 0x70) >> 4)
    return np.where(u & 0x80, 0x84 - t, t - 0x84).astype(np.int16)


def _alaw_expand():
    a = np.arange(256, dtype=np.int32) ^ 0x55
    seg = (a & 0x70) >> 4
    t = (a & 0x0F) << 4
    t = np.where(seg == 0, t + 8, (t + 0x108) << np.maximum(seg - 1, 0))
    return np.where(a & 0x80, t, -t).astype(np.int16)


ULAW_EXPAND = _ulaw_expand()   # the standard expanders (ulaw2linear / alaw2linear): byte -> int16
ALAW_EXPAND = _alaw_expand()
ULAW_EXPAND.setflags(write=False)
ALAW_EXPAND.setflags(write=False)


def fnv1a32(data):
    """FNV-1a-32 of a byte array: what the 65,536-byte tables are pinned by."""
    h = 0x811C9DC5
    for b in bytes(data):
        h = ((h ^ b) * 0x01000193) & 0xFFFFFFFF
    return h
