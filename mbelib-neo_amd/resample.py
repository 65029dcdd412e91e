"""Wide rows (include/mbx_resample.h): the numpy definition of the polyphase FIR interpolator -- ``step(rs, records, T, x,
stream_index=None) -> (out, records)``: the n * T rows of a call upsampled by L, and the history records after it, int64 inside --,
``design(L, K)``, the one convenience a host needs (the C library ships no designer and owns no tables), the constants and structures of
the header, and a small wrapper of the native state object.  The tests hold the library to this module; nothing here runs on the hot
path (that is ``pcm_resample_kernel`` on the device: ``BatchDecoder.resample``, ``mbx_session_next_resample``)."""
import ctypes as C

import numpy as np

from . import _native

MAX_TAPS = 192        # MBX_RESAMPLE_MAX_TAPS
UNITY = 16384         # MBX_RESAMPLE_UNITY_Q14
HISTORY = 32          # MBX_RESAMPLE_HISTORY
PHASE_BOUND = 65535   # the largest sum of |taps| a phase may have
FACTORS = (2, 3, 4, 6)

# mbx_resample_record: the last 32 input samples of a row, oldest first; fresh or reset is zeros
RECORD_DTYPE = np.dtype([("hist", "<i2", (HISTORY,))])
assert RECORD_DTYPE.itemsize == 64


class Resample(C.Structure):
    """mbx_resample"""
    _fields_ = [("L", C.c_uint8), ("K", C.c_uint8), ("zero", C.c_uint8 * 2), ("taps", C.c_int16 * MAX_TAPS)]

    @classmethod
    def of(cls, L, K, taps):
        """the structure of a prototype filter h[0 .. K*L-1] (any integer sequence of that length)"""
        h = np.asarray(taps).reshape(-1)
        if h.size != int(L) * int(K) or h.size > MAX_TAPS:
            raise ValueError("taps holds K * L values, at most 192")
        if (h < -32768).any() or (h > 32767).any():
            raise ValueError("taps are int16")
        rs = cls()
        rs.L, rs.K = int(L), int(K)
        for i, v in enumerate(h.tolist()):
            rs.taps[i] = int(v)
        return rs

    def prototype(self):
        return np.array(self.taps[:], dtype=np.int16)


def _fields(rs):
    """(L, K, int64 taps h[0 .. K*L-1]) of a Resample or of a tuple (L, K, taps); ValueError for what the library refuses"""
    if isinstance(rs, Resample):
        L, K, zero, taps = int(rs.L), int(rs.K), int(rs.zero[0]) | int(rs.zero[1]), np.array(rs.taps[:], dtype=np.int64)
    else:
        L, K, h = rs
        L, K, zero = int(L), int(K), 0
        h = np.asarray(h, dtype=np.int64).reshape(-1)
        if h.size > MAX_TAPS or (h < -32768).any() or (h > 32767).any():
            raise ValueError("taps are at most 192 int16")
        taps = np.zeros(MAX_TAPS, dtype=np.int64)
        taps[:h.size] = h
    if L not in FACTORS:
        raise ValueError("L is 2, 3, 4 or 6")
    if not (2 <= K <= 32 and K % 2 == 0):
        raise ValueError("K is even, 2 .. 32")
    if zero != 0:
        raise ValueError("the zero bytes are not 0")
    if taps[K * L:].any():
        raise ValueError("a nonzero tap beyond K * L")
    h = taps[:K * L]
    if int(np.abs(h).reshape(K, L).sum(axis=0).max()) > PHASE_BOUND:
        raise ValueError("a phase whose taps sum to more than 65535 in magnitude")
    return L, K, h


def fresh_state(n):
    return np.zeros(int(n), dtype=RECORD_DTYPE)


def check_state(records):
    st = np.asarray(records)
    if st.dtype != RECORD_DTYPE or st.ndim != 1:
        raise TypeError("records is a 1-d array of RECORD_DTYPE")
    return st


def step(rs, records, T, x, stream_index=None):
    """int16 rows [n * T, 160], stream-major, and the records before them -> (the wide rows int16 [n * T, 160 * L], the records after
    them).  Entry i uses record stream_index[i] (None: i); an entry outside the records runs over a zero history and stores none.  Per
    row: x_ext = the record (frame 0) or the last 32 samples of the row in front (frame t > 0), then the row;
    y[n*L+p] = clamp((sum_k taps[p + k*L] * x_ext[n - k] + 8192) >> 14) (the shift floors); the new record is the last 32 samples of the
    entry's last row."""
    L, K, h = _fields(rs)
    T = int(T)
    x = np.ascontiguousarray(x)
    if x.dtype != np.int16 or x.ndim != 2 or x.shape[1] != 160 or T < 0 or (T and x.shape[0] % T) or (T == 0 and x.shape[0]):
        raise ValueError("x is int16 [n * T, 160]")
    n = x.shape[0] // T if T else 0
    st = check_state(records).copy()
    index = np.arange(n, dtype=np.int64) if stream_index is None else np.ascontiguousarray(stream_index, dtype=np.int64).reshape(-1)
    if index.size != n:
        raise ValueError("stream_index has one entry per stream of the call")
    out = np.empty((n * T, 160 * L), dtype=np.int16)
    if n * T == 0:
        return out, st
    owns = (index >= 0) & (index < st.size)
    hist = np.zeros((n, HISTORY), dtype=np.int64)
    hist[owns] = st["hist"][index[owns]]
    rows = x.astype(np.int64).reshape(n, T * 160)
    ext = np.concatenate([hist, rows], axis=1)                  # [n, 32 + T * 160]: frame t > 0 finds the tail of frame t - 1 in front of it
    taps = h.reshape(K, L)                                      # taps[k, p] = h[p + k * L]
    acc = np.zeros((n, T * 160, L), dtype=np.int64)
    for k in range(K):
        acc += ext[:, HISTORY - k:HISTORY - k + T * 160, None] * taps[k][None, None, :]
    assert int(np.abs(acc).max()) <= PHASE_BOUND * 32768
    y = np.clip((acc + 8192) >> 14, -32768, 32767).astype(np.int16)
    out[:] = y.reshape(n * T, 160 * L)
    st["hist"][index[owns]] = ext[owns, -HISTORY:].astype(np.int16)
    return out, st


def design(L, K, cut=0.92, beta=7.0):
    """A Kaiser-windowed sinc prototype for L x interpolation, K taps per phase, as int16 Q14 h[0 .. K*L-1]: N = K * L,
    t = arange(N) - (N - 1) / 2, fc = 0.5 / L * cut, h = 2 fc sinc(2 fc t) L kaiser(N, beta); then every phase p is normalised on its
    own -- f = h[p::L] / sum(h[p::L]), r = rint(f * 16384), and 16384 - sum(r) is added to the tap of largest magnitude -- so that every
    phase has exact DC unity (a constant row comes out as that constant)."""
    L, K = int(L), int(K)
    if L not in FACTORS or not (2 <= K <= 32 and K % 2 == 0):
        raise ValueError("L is 2, 3, 4 or 6 and K is even, 2 .. 32")
    N = K * L
    t = np.arange(N) - (N - 1) / 2.0
    fc = 0.5 / L * float(cut)
    h = 2.0 * fc * np.sinc(2.0 * fc * t) * L * np.kaiser(N, float(beta))
    taps = np.zeros(N, dtype=np.int64)
    for p in range(L):
        f = h[p::L] / h[p::L].sum()
        r = np.rint(f * UNITY).astype(np.int64)
        r[int(np.argmax(np.abs(r)))] += UNITY - int(r.sum())
        taps[p::L] = r
    assert (taps >= -32768).all() and (taps <= 32767).all()
    return taps.astype(np.int16)


def hold_taps(L, K, value=UNITY):
    """the HOLD identity of the header: taps[p] = value for every p, everything else 0"""
    h = np.zeros(int(K) * int(L), dtype=np.int16)
    h[:int(L)] = value
    return h


def delay_taps(L, K):
    """the DELAY identity of the header: taps[p + (K-1)*L] = 16384, everything else 0"""
    h = np.zeros(int(K) * int(L), dtype=np.int16)
    h[(int(K) - 1) * int(L):] = UNITY
    return h


class ResampleState:
    """A native resampler state (mbx_resample_state_create): `streams` records on the current device, every one zeros.  Owns the
    native handle."""

    def __init__(self, streams):
        self.handle = None
        h = C.c_void_p()
        _native.check(_native.lib().mbx_resample_state_create(C.byref(h), int(streams)), "mbx_resample_state_create")
        self.handle = h
        self.streams = _native.lib().mbx_resample_state_streams(h)

    def _range(self, first, count):
        first = int(first)
        return first, self.streams - first if count is None else int(count)

    def get(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        out = fresh_state(max(count, 0))
        _native.check(_native.lib().mbx_resample_state_get(self.handle, first, count, out.ctypes.data if out.size else None, stream), "mbx_resample_state_get")
        return out

    def set(self, records, first=0, stream=None):
        st = np.ascontiguousarray(records, dtype=RECORD_DTYPE).reshape(-1)
        _native.check(_native.lib().mbx_resample_state_set(self.handle, int(first), st.size, st.ctypes.data if st.size else None, stream), "mbx_resample_state_set")

    def reset(self, first=0, count=None, stream=None):
        first, count = self._range(first, count)
        _native.check(_native.lib().mbx_resample_state_reset(self.handle, first, count, stream), "mbx_resample_state_reset")

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_resample_state_destroy(self.handle)
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
