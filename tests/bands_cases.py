"""Shared cases of the band-record tests (tests/test_bands_host.py on the CPU, tests/test_gpu_bands.py on the device): rows of every
loudness with the rails among them, banks of random probes at exactly the bound with the sign-aligned probe that reaches
+-2,147,450,880, and the synthetic DTMF rows.  numpy only; everything is made once and handed out read-only."""
import numpy as np

from mbelib_neo_amd import bands

BOUND = bands.VECTOR_BOUND


def rows(rng, n):
    """n rows of very different loudness, full-range ones among them; planted at the front (as far as n reaches): all 32767, all
    -32768, alternating rails, zeros"""
    scale = rng.choice(np.array([3, 40, 700, 5000, 32768]), size=n)
    x = (rng.integers(-32768, 32768, size=(n, 160), dtype=np.int64) * scale[:, None] // 32768).astype(np.int16)
    planted = [np.full(160, 32767), np.full(160, -32768), np.where(np.arange(160) & 1, -32768, 32767), np.zeros(160)]
    for r, p in zip(range(min(n, 4)), planted):
        x[r] = p.astype(np.int16)
    return x


def vector_at_bound(rng, total=BOUND, signs=None):
    """160 int16 whose magnitudes sum to exactly `total`, spread at random (no element above 32767); signs random, or those given"""
    assert 0 <= total <= BOUND
    cuts = np.sort(rng.integers(0, total + 1, size=159))
    mag = np.diff(np.concatenate([[0], cuts, [total]]))
    if total == BOUND and rng.integers(0, 2):   # every other one as few elements as the bound allows: 32767 + 32767 + 1
        mag = np.zeros(160, dtype=np.int64)
        mag[rng.permutation(160)[:3]] = [32767, 32767, 1]
    assert mag.sum() == total and mag.max() <= 32767
    s = rng.choice(np.array([-1, 1]), size=160) if signs is None else np.asarray(signs)
    return (mag * s).astype(np.int16)


def bank(rng, K):
    """K probes, every vector at exactly the bound, signs at random; probe 0 is sign-aligned with the rows of rows(): c all positive
    (the all-32767 and all -32768 rows reach -+2,147,418,113 and +-2,147,450,880), s alternating (the alternating rails reach it)"""
    p = np.stack([np.stack([vector_at_bound(rng), vector_at_bound(rng)]) for _ in range(K)])
    p[0, 0] = vector_at_bound(rng, signs=np.ones(160, dtype=np.int64))
    p[0, 1] = vector_at_bound(rng, signs=np.where(np.arange(160) & 1, 1, -1))
    if K > 2:
        p[K - 1] = 0                      # a probe of zeros (ZERO)
    if K > 3:
        p[K - 2, 0] = 0
        p[K - 2, 0, 77] = 16384           # an impulse (IMPULSE)
        p[K - 2, 1] = 0
    assert np.abs(p.astype(np.int64)).sum(axis=2).max() == BOUND
    return p


_DTMF = {}


def dtmf_rows():
    """(rows int16 [2400, 160], keys str of 2400): 16 digits x (-10, -20, -30 dBFS per tone) x 50 rows, two tones with random phases and
    white noise at -50 dBFS rms, default_rng(7)"""
    if not _DTMF:
        rng = np.random.default_rng(7)
        n = np.arange(160)
        out, keys = [], []
        for digit in range(16):
            lo, hi = bands.DTMF_HZ[digit // 4], bands.DTMF_HZ[4 + digit % 4]
            for db in (-10, -20, -30):
                a = 32768.0 * 10.0 ** (db / 20.0)
                phase = rng.uniform(0.0, 2.0 * np.pi, size=(50, 2))
                x = a * np.sin(2.0 * np.pi * lo * n / 8000.0 + phase[:, :1]) + a * np.sin(2.0 * np.pi * hi * n / 8000.0 + phase[:, 1:])
                x = x + rng.normal(0.0, 32768.0 * 10.0 ** (-50 / 20.0), size=x.shape)
                out.append(np.clip(np.rint(x), -32768, 32767).astype(np.int16))
                keys.append(bands.DTMF_KEYS[digit] * 50)
        x = np.concatenate(out)
        x.setflags(write=False)
        _DTMF["it"] = (x, "".join(keys))
    return _DTMF["it"]


_WANT = {}


def case(nrows, K):
    """(rows, bank, {form: numpy's records}) for nrows rows and K probes: made once per shape, read-only"""
    if (nrows, K) not in _WANT:
        rng = np.random.default_rng(1000 * nrows + K)
        x, p = rows(rng, nrows), bank(rng, K)
        want = {form: bands.measure(x, p, form) for form in bands.FORMS}
        for a in (x, p, *want.values()):
            a.setflags(write=False)
        _WANT[nrows, K] = (x, p, want)
    return _WANT[nrows, K]
