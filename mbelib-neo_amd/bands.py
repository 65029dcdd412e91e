"""Band records (include/mbx_bands.h) in numpy: the definition the host function (mbx_pcm_bands_host) and the kernel (pcm_bands_kernel)
are held to, and the designers -- the C library ships none and owns no table: the caller brings the probes.

A bank is int16 [K, 2, 160]: probe k is the vectors c = probes[k, 0] and s = probes[k, 1], every one with sum |v[n]| <= 65535.  Per row
x and probe k, re = sum x[n] c[n] and im = sum x[n] s[n], exact in int32; COMPLEX records are (re, im), POWER records are
(re^2 + im^2) >> 31 as uint32.  No torch, no native library."""
import numpy as np

MAX_PROBES = 32          # MBX_BANDS_MAX_PROBES
VECTOR_BOUND = 65535     # MBX_BANDS_VECTOR_BOUND
COMPLEX, POWER = 0, 1    # MBX_BANDS_COMPLEX, MBX_BANDS_POWER
FORMS = (COMPLEX, POWER)
RECORD_DTYPE = np.dtype([("re", "<i4"), ("im", "<i4")])   # mbx_band_record
RATE = 8000
DTMF_HZ = (697, 770, 852, 941, 1209, 1336, 1477, 1633)    # the four rows, then the four columns
DTMF_KEYS = "123A456B789C*0#D"                             # key = DTMF_KEYS[4 * row + column]


def out_dtype(form):
    if form not in FORMS:
        raise ValueError("form is MBX_BANDS_COMPLEX or MBX_BANDS_POWER")
    return RECORD_DTYPE if form == COMPLEX else np.dtype("<u4")


def record_bytes(form):
    return out_dtype(form).itemsize


def _bank(probes):
    p = np.asarray(probes)
    if p.dtype != np.int16:
        raise TypeError("probes are int16")
    if p.ndim == 2 and p.shape == (2, 160):
        p = p[None]
    if p.ndim != 3 or p.shape[1:] != (2, 160):
        raise ValueError("probes are [K, 2, 160]: K x { c[160], s[160] }")
    return p


def check(probes):
    """raises ValueError with the library's wording for what mbx_band_bank_create refuses of a bank; returns it as int16 [K, 2, 160]"""
    p = _bank(probes)
    if not 1 <= p.shape[0] <= MAX_PROBES:
        raise ValueError("K is 1 .. MBX_BANDS_MAX_PROBES")
    sums = np.abs(p.astype(np.int64)).sum(axis=2)
    for k, v in zip(*np.nonzero(sums > VECTOR_BOUND)):
        raise ValueError(f"probe {k}: the |{'cs'[v]}[n]| sum to {sums[k, v]}, above MBX_BANDS_VECTOR_BOUND (65535)")
    return p


def measure(pcm16, probes, form=COMPLEX):
    """THE definition: int16 rows [n, 160] and a bank -> records [n, K] of `form`, in int64 throughout"""
    x = np.asarray(pcm16)
    if x.dtype != np.int16:
        raise TypeError("pcm16 is int16")
    x = x.reshape(-1, 160).astype(np.int64)
    p = check(probes).astype(np.int64)
    dtype = out_dtype(form)
    re = x @ p[:, 0].T
    im = x @ p[:, 1].T
    assert np.abs(re).max(initial=0) < 2**31 and np.abs(im).max(initial=0) < 2**31
    if form == COMPLEX:
        out = np.empty(re.shape, dtype=RECORD_DTYPE)
        out["re"], out["im"] = re, im
        return out
    power = (re.astype(np.uint64) * re.astype(np.uint64) + im.astype(np.uint64) * im.astype(np.uint64)) >> np.uint64(31)   # (mod 2^64: a square is the same either sign)
    assert power.max(initial=0) < 2**32
    return power.astype(dtype)


def _window(name):
    n = np.arange(160)
    if name == "rect":
        return np.ones(160)
    if name == "hann":
        return 0.5 - 0.5 * np.cos(2.0 * np.pi * (n + 0.5) / 160.0)
    raise ValueError('window is "rect" or "hann"')


def tone(freq_hz, window="rect"):
    """one probe, int16 [2, 160]: c = w[n] cos(2 pi f n / 8000) and s = -w[n] sin(2 pi f n / 8000), both scaled by ONE factor -- the
    largest for which both vectors meet the bound before rounding -- and truncated toward zero, so the bound holds by construction"""
    w = _window(window)
    n = np.arange(160)
    c = w * np.cos(2.0 * np.pi * float(freq_hz) * n / RATE)
    s = -w * np.sin(2.0 * np.pi * float(freq_hz) * n / RATE)
    scale = VECTOR_BOUND / max(np.abs(c).sum(), np.abs(s).sum())
    scale = min(scale, 32767.0 / max(np.abs(c).max(), np.abs(s).max()))
    probe = np.trunc(np.stack([c, s]) * scale).astype(np.int16)
    return probe


def dtmf(window="rect"):
    """the eight DTMF probes, int16 [8, 2, 160]: 697, 770, 852 and 941 Hz (the rows), then 1209, 1336, 1477 and 1633 Hz (the columns)"""
    return np.stack([tone(f, window) for f in DTMF_HZ])


def dtmf_key(power):
    """the key each row of POWER records of dtmf() decides: the largest row probe and the largest column probe -> str of len(power)"""
    p = np.asarray(power).reshape(-1, 8)
    return "".join(DTMF_KEYS[4 * int(r) + int(c)] for r, c in zip(p[:, :4].argmax(axis=1), p[:, 4:].argmax(axis=1)))
