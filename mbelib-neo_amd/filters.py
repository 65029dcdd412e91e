"""Filtered rows (include/mbx_filter.h): the numpy definition of the per-stream biquad cascade -- ``step(filt, state, T, rows,
index=None) -> (out, state)``: the n * T rows of a call through 1 .. 4 second-order sections, and the state records after it, int64
inside, vectorised over the entries and serial over the samples --, the designers a host needs (the C library ships none and owns no
tables): ``highpass``, ``lowpass``, ``notch`` and ``peaking``, the constants and structures of the header, and a small wrapper of the
native state object.  The tests hold the library to this module; nothing here runs on the hot path (that is ``pcm_filter_kernel`` on
the device: ``BatchDecoder.filter``, ``mbx_session_next_filter``).

THE DESIGNERS are the bilinear (RBJ cookbook) forms at 8 kHz, normalised by a0 and rounded to Q14.  ``highpass(fc, sections)`` is a
Butterworth cascade of order 2 * sections (Q_k = 1 / (2 cos((2 k + 1) pi / (4 sections)))); after the rounding it sets
b1 = -(b0 + b2), so that every section's numerator sums to EXACTLY zero: a constant input then decays to exactly 0 (without that the
200 Hz section of order 2 idles at 90 under a constant -32768).  The float64 response of the quantised cascades against the
unquantised designs, at 25, 50, 100, 200, 300, 500, 1000 and 3000 Hz, for highpass(fc, 2) at fc = 60, 100, 150, 200, 250 and 300 Hz:
within 0.070 dB, the worst at fc = 60 Hz and 25 Hz (tests/test_filter_host.py measures it and holds it to 0.070 + 0.05 dB for the
platform's libm; finer steps of fc read up to 0.11 dB, and four sections at 60-100 Hz up to 0.10 dB).  ``lowpass``, ``notch`` and
``peaking`` round plainly.  Every designer raises ValueError where a coefficient leaves int16 or a section leaves the bounds of the
header."""
import ctypes as C
import math

import numpy as np

from . import _native

MAX_SECTIONS = 4      # MBX_FILTER_MAX_SECTIONS
UNITY = 16384         # MBX_FILTER_UNITY_Q14
COEFF_BOUND = 65535   # MBX_FILTER_COEFF_BOUND: |b0| + |b1| + |b2| and |a1| + |a2| of a section, at most
RATE = 8000.0         # the rows are 8 kHz

# mbx_filter_record: 32 bytes; fresh or reset is zeros
RECORD_DTYPE = np.dtype([("x1", "<i2"), ("x2", "<i2"), ("sec", np.dtype([("y1", "<i2"), ("y2", "<i2"), ("e", "<u2")]), (MAX_SECTIONS,)),
                         ("zero", "<u2", (2,))])
assert RECORD_DTYPE.itemsize == 32


class Section(C.Structure):
    """mbx_filter_section"""
    _fields_ = [("b0", C.c_int16), ("b1", C.c_int16), ("b2", C.c_int16), ("a1", C.c_int16), ("a2", C.c_int16)]


class Filter(C.Structure):
    """mbx_filter"""
    _fields_ = [("sections", C.c_uint8), ("zero", C.c_uint8 * 3), ("sec", Section * MAX_SECTIONS)]

    @classmethod
    def of(cls, coeffs):
        """the structure of 1 .. 4 sections (b0, b1, b2, a1, a2), Q14 integers; ValueError for what the library refuses"""
        c = _fields(coeffs)
        f = cls()
        f.sections = c.shape[0]
        for s, row in enumerate(c.tolist()):
            f.sec[s] = Section(*row)
        return f

    def coeffs(self):
        """int64 [4, 5]: every section of the structure, those beyond `sections` included"""
        return np.array([[x.b0, x.b1, x.b2, x.a1, x.a2] for x in self.sec], dtype=np.int64)


def _fields(filt):
    """int64 [S, 5] of a Filter or of a sequence of sections; ValueError for what the library refuses"""
    if isinstance(filt, Filter):
        S, zero, c = int(filt.sections), int(filt.zero[0]) | int(filt.zero[1]) | int(filt.zero[2]), filt.coeffs()
    else:
        c = np.asarray(filt, dtype=np.int64)
        if c.ndim != 2 or c.shape[1] != 5:
            raise ValueError("a filter is 1 .. 4 sections of (b0, b1, b2, a1, a2)")
        S, zero = c.shape[0], 0
        c = np.concatenate([c[:MAX_SECTIONS], np.zeros((max(MAX_SECTIONS - S, 0), 5), dtype=np.int64)])
    if not 1 <= S <= MAX_SECTIONS:
        raise ValueError("sections is 1 .. MAX_SECTIONS")
    if zero != 0:
        raise ValueError("the zero bytes are not 0")
    if (c < -32768).any() or (c > 32767).any():
        raise ValueError("coefficients are int16")
    if (np.abs(c[:S, :3]).sum(axis=1) > COEFF_BOUND).any() or (np.abs(c[:S, 3:]).sum(axis=1) > COEFF_BOUND).any():
        raise ValueError("a section whose |b0| + |b1| + |b2| or |a1| + |a2| is above 65535")
    if c[S:].any():
        raise ValueError("a non-zero coefficient beyond sections")
    return c[:S]


def fresh_state(n):
    return np.zeros(int(n), dtype=RECORD_DTYPE)


def check_state(state):
    st = np.asarray(state)
    if st.dtype != RECORD_DTYPE or st.ndim != 1:
        raise TypeError("state is a 1-d array of RECORD_DTYPE")
    if (st["sec"]["e"] >= UNITY).any() or st["zero"].any():
        raise ValueError("a state record whose e is above 16383, or whose pad is not 0")
    return st


def step(filt, state, T, rows, index=None):
    """int16 rows [n * T, 160], stream-major, and the state before them -> (the filtered rows, the state after them).  Entry i uses
    record index[i] (None: i); an entry outside the state runs over a zero record and stores none.  Per sample and section:
    ff = b0 x + b1 x1 + b2 x2; fb = a1 y1 + a2 y2; acc = ff - fb + e; q = acc >> 14 (floors); e = acc - (q << 14);
    y = clamp(q, -32768, 32767); the input of section s + 1 is y of section s.  The records of sections >= S stay as they were."""
    c = _fields(filt)
    S, T = c.shape[0], int(T)
    x = np.ascontiguousarray(rows)
    if x.dtype != np.int16 or x.ndim != 2 or x.shape[1] != 160 or T < 0 or (T and x.shape[0] % T) or (T == 0 and x.shape[0]):
        raise ValueError("rows is int16 [n * T, 160]")
    n = x.shape[0] // T if T else 0
    st = check_state(state).copy()
    idx = np.arange(n, dtype=np.int64) if index is None else np.ascontiguousarray(index, dtype=np.int64).reshape(-1)
    if idx.size != n:
        raise ValueError("index has one entry per stream of the call")
    out = np.empty_like(x)
    if n * T == 0:
        return out, st
    owns = (idx >= 0) & (idx < st.size)
    rec = fresh_state(n)
    rec[owns] = st[idx[owns]]
    # line[0], line[1]: x1, x2 of section 0; line[2 s + 2], line[2 s + 3]: y1, y2 of section s, which are x1, x2 of section s + 1
    line = [rec["x1"].astype(np.int64), rec["x2"].astype(np.int64)]
    for s in range(S):
        line += [rec["sec"]["y1"][:, s].astype(np.int64), rec["sec"]["y2"][:, s].astype(np.int64)]
    e = [rec["sec"]["e"][:, s].astype(np.int64) for s in range(S)]
    wide = x.astype(np.int64).reshape(n, T * 160)
    y = np.empty((n, T * 160), dtype=np.int64)
    coef = c.tolist()
    for k in range(T * 160):
        v = wide[:, k]
        for s in range(S):
            b0, b1, b2, a1, a2 = coef[s]
            x1, x2, y1, y2 = line[2 * s], line[2 * s + 1], line[2 * s + 2], line[2 * s + 3]
            acc = b0 * v + b1 * x1 + b2 * x2 - (a1 * y1 + a2 * y2) + e[s]
            q = acc >> 14
            e[s] = acc - (q << 14)
            line[2 * s + 1], line[2 * s] = x1, v   # (the inputs of section s: the outputs of section s - 1, moved when that one ran its next sample)
            v = np.clip(q, -32768, 32767)
        line[2 * S + 1], line[2 * S] = line[2 * S], v
        y[:, k] = v
    out[:] = y.reshape(n * T, 160).astype(np.int16)
    rec["x1"], rec["x2"] = line[0].astype(np.int16), line[1].astype(np.int16)
    for s in range(S):
        rec["sec"]["y1"][:, s], rec["sec"]["y2"][:, s] = line[2 * s + 2].astype(np.int16), line[2 * s + 3].astype(np.int16)
        rec["sec"]["e"][:, s] = e[s].astype(np.uint16)
    st[idx[owns]] = rec[owns]
    return out, st


# ---- designers ---------------------------------------------------------------------------------------------------------------------------
def butterworth_qs(sections):
    """the Q of every second-order section of a Butterworth filter of order 2 * sections"""
    sections = int(sections)
    if not 1 <= sections <= MAX_SECTIONS:
        raise ValueError("sections is 1 .. MAX_SECTIONS")
    return [1.0 / (2.0 * math.cos((2 * k + 1) * math.pi / (4.0 * sections))) for k in range(sections)]


def prototype(kind, f, q, gain_db=0.0, rate=RATE):
    """the unquantised section (b0, b1, b2, a1, a2), normalised by a0: the RBJ forms 'highpass', 'lowpass', 'notch', 'peaking'"""
    f, q, rate = float(f), float(q), float(rate)
    if not (0.0 < f < rate / 2.0) or not q > 0.0:
        raise ValueError("0 < f < rate / 2 and Q > 0")
    w0 = 2.0 * math.pi * f / rate
    cs, alpha = math.cos(w0), math.sin(w0) / (2.0 * q)
    if kind == "highpass":
        b, a = ((1.0 + cs) / 2.0, -(1.0 + cs), (1.0 + cs) / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "lowpass":
        b, a = ((1.0 - cs) / 2.0, 1.0 - cs, (1.0 - cs) / 2.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "notch":
        b, a = (1.0, -2.0 * cs, 1.0), (1.0 + alpha, -2.0 * cs, 1.0 - alpha)
    elif kind == "peaking":
        A = 10.0 ** (float(gain_db) / 40.0)
        b, a = (1.0 + alpha * A, -2.0 * cs, 1.0 - alpha * A), (1.0 + alpha / A, -2.0 * cs, 1.0 - alpha / A)
    else:
        raise ValueError("kind is 'highpass', 'lowpass', 'notch' or 'peaking'")
    return np.array([b[0], b[1], b[2], a[1], a[2]], dtype=np.float64) / a[0]


def quantise(sections, zero_sum=False):
    """float sections [S, 5] -> a Filter: rint(c * 16384); zero_sum: b1 = -(b0 + b2) behind the rounding"""
    c = np.rint(np.asarray(sections, dtype=np.float64).reshape(-1, 5) * UNITY).astype(np.int64)
    if zero_sum:
        c[:, 1] = -(c[:, 0] + c[:, 2])
    return Filter.of(c)


def highpass_prototype(fc, sections=2, rate=RATE):
    return np.stack([prototype("highpass", fc, q, rate=rate) for q in butterworth_qs(sections)])


def highpass(fc, sections=2, rate=RATE):
    """a Butterworth high-pass of order 2 * sections at fc Hz; every section's numerator sums to exactly zero"""
    return quantise(highpass_prototype(fc, sections, rate), zero_sum=True)


def lowpass(fc, sections=2, rate=RATE):
    """a Butterworth low-pass of order 2 * sections at fc Hz"""
    return quantise(np.stack([prototype("lowpass", fc, q, rate=rate) for q in butterworth_qs(sections)]))


def notch(f0, q=8.0, rate=RATE):
    """one section: a notch at f0 Hz, Q = f0 / bandwidth"""
    return quantise(prototype("notch", f0, q, rate=rate))


def peaking(f0, q, gain_db, rate=RATE):
    """one section: gain_db at f0 Hz, Q = f0 / bandwidth, unity far from it"""
    return quantise(prototype("peaking", f0, q, gain_db, rate=rate))


def response_db(sections, freqs, rate=RATE):
    """the magnitude in dB, float64, of a cascade at `freqs` Hz: `sections` is a Filter (its Q14 coefficients / 16384) or float [S, 5]"""
    c = _fields(sections).astype(np.float64) / UNITY if isinstance(sections, Filter) else np.asarray(sections, dtype=np.float64).reshape(-1, 5)
    z = np.exp(-2j * np.pi * np.asarray(freqs, dtype=np.float64) / float(rate))
    h = np.ones_like(z)
    for b0, b1, b2, a1, a2 in c:
        h = h * (b0 + b1 * z + b2 * z * z) / (1.0 + a1 * z + a2 * z * z)
    return 20.0 * np.log10(np.abs(h))


class FilterState:
    """A native filter state (mbx_filter_state_create): `streams` records on the current device, every one zeros.  Owns the native
    handle."""

    def __init__(self, streams):
        self.handle = None
        h = C.c_void_p()
        _native.check(_native.lib().mbx_filter_state_create(C.byref(h), int(streams)), "mbx_filter_state_create")
        self.handle = h
        self.streams = _native.lib().mbx_filter_state_streams(h)

    def _range(self, first, count):
        first = int(first)
        return first, self.streams - first if count is None else int(count)

    def get(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        out = fresh_state(max(count, 0))
        _native.check(_native.lib().mbx_filter_state_get(self.handle, first, count, out.ctypes.data if out.size else None, stream), "mbx_filter_state_get")
        return out

    def set(self, state, first=0, stream=None):
        st = np.ascontiguousarray(state, dtype=RECORD_DTYPE).reshape(-1)
        _native.check(_native.lib().mbx_filter_state_set(self.handle, int(first), st.size, st.ctypes.data if st.size else None, stream), "mbx_filter_state_set")

    def reset(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        _native.check(_native.lib().mbx_filter_state_reset(self.handle, first, count, stream), "mbx_filter_state_reset")

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_filter_state_destroy(self.handle)
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
