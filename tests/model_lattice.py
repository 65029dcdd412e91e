"""Model lattices: caller-made models for the single-stage entry points (mbx_synthesize_speech, mbx_spectral_amp_enhance,
mbx_adaptive_smoothing, mbx_synthesize_tone, mbx_decode_parms and their mbe_* twins).

The batch path only ever meets models the decoder made itself: w0 one of 208 or 120 table values, L a function of w0, voicing in
band-sized blocks, phases what two frames of history produced.  The stage entry points take whatever struct the caller wrote, and
the device functions behind them (synth_core, enhance, smooth, wrap_two_pi, tone_frame) carry statements that hold for decoder-made
models only.  A lattice here is a named, seeded set of (cur, prev, rng) struct arrays -- at most MAX_STRUCTS, one launch per entry
point --, each struct with a class (the unit the float bounds are applied to, in groups of at most GROUP structs) and one line of
text that failure messages print.  `oracle(name, entry)` is the CPU oracle's answer, made once and shared (read it, never write to
it); `composition(name)` asserts, from the oracle's answer alone, that the lattice holds what it claims.

Unless a class says otherwise: Ml[l] = u_l * 3000 / (2 L), u_l uniform in [0, 1), so that the voiced sum 2 sum Ml < 3000 cannot reach
the soft clip at 4,446.9; w0 uniform between the smallest and the largest fundamental of the codec tables (read from the blob), off
the grid; PHIl and PSIl uniform in [-4000, 4000]; noiseSeed and noiseOverlap integer-valued in 0..53,124.

The oracle is the checker; no fixture is written.  Test infrastructure: imported without a GPU; nothing in the package uses it."""
import ctypes as C
import functools
import math
from collections import namedtuple

import numpy as np

from mbelib_neo_amd import framegen
from mbelib_neo_amd.layout import init_parms, rng_seeded

import oracle_lib
import parity

MAX_STRUCTS = 4096
GROUP = 256
F = np.float32
TWO_PI = 2.0 * math.pi
MUTE_IMBE, MUTE_AMBE = F(0.0875), F(0.096)
SHIM_SAMPLE = 32
MIN_SHARE_BELOW_CLIP = 0.90

# name, cur, prev, rng [n]; cls [n] str: the class of each struct; text [n] str: one line per struct; extra: dict of further inputs
Lattice = namedtuple("Lattice", "name cur prev rng cls text extra")

SYNTHESIS = ("pairs", "voicing", "pitch", "phase", "gate", "energy")
# entry point -> the lattices that go through it
ENTRIES = {
    "speech": SYNTHESIS,
    "smoothing": ("energy", "pairs"),
    "enhance": ("weights", "pairs"),
    "noise": ("gate",),
    "tone": ("tones",),
    "tone_dstar": ("tones_dstar",),
    "decode_parms": ("predict0", "predict1", "predict3"),
}
TAGS = {"pairs": 1, "voicing": 2, "pitch": 3, "phase": 4, "gate": 5, "energy": 6, "weights": 7, "tones": 8, "tones_dstar": 9, "predict0": 10,
        "predict1": 11, "predict3": 13}


def w0_span():
    """(smallest, largest) fundamental of the codec tables, from the blob"""
    t = framegen._tables()
    w = np.concatenate([t["imbe_w0"], t["ambe_w0"] * np.float32(2.0 * math.pi)])   # (the AMBE table holds f0 = w0 / 2 pi)
    w = w[w > 0]
    return float(w.min()), float(w.max())


def _next(x, up=True, steps=1):
    x = np.asarray(x, dtype=F)
    for _ in range(steps):
        x = np.nextafter(x, F(np.inf) if up else F(-np.inf))
    return x


def _models(n, rng, L, pL=None, near=None):
    """n free (cur, prev, rng) structs with the given L / prev.L (arrays or scalars); near: bool [n], prev.w0 = cur.w0 * U(0.92, 1.08)"""
    lo, hi = w0_span()
    L = np.broadcast_to(np.asarray(L, dtype=np.int32), (n,)).copy()
    pL = L.copy() if pL is None else np.broadcast_to(np.asarray(pL, dtype=np.int32), (n,)).copy()
    near = np.zeros(n, dtype=bool) if near is None else np.broadcast_to(np.asarray(near, dtype=bool), (n,))
    out = []
    slot = np.arange(57)[None, :]
    w0 = rng.uniform(lo, hi, size=n).astype(F)
    for k, l in enumerate((L, pL)):
        p = np.repeat(init_parms(1), n)
        if k == 0:
            p["w0"] = w0
        else:
            p["w0"] = np.where(near, np.clip(w0 * rng.uniform(0.92, 1.08, size=n), lo, hi), rng.uniform(lo, hi, size=n)).astype(F)
        p["L"] = l
        safe = np.clip(l, 1, 56)
        p["K"] = np.where(safe <= 36, (safe + 2) // 3, 12)
        live = (slot >= 1) & (slot <= safe[:, None])
        p["Vl"] = rng.integers(0, 2, size=(n, 57)) * (live | (slot == 0))
        p["Ml"] = (rng.random((n, 57)) * 3000.0 / (2.0 * safe[:, None]) * live).astype(F)
        p["log2Ml"] = (rng.uniform(-2.0, 8.0, size=(n, 57)) * live).astype(F)
        p["PHIl"] = rng.uniform(-4000.0, 4000.0, size=(n, 57)).astype(F)
        p["PSIl"] = rng.uniform(-4000.0, 4000.0, size=(n, 57)).astype(F)
        p["PHIl"][:, 0] = 0
        p["PSIl"][:, 0] = 0
        p["gamma"] = rng.uniform(0.5, 1.5, size=n).astype(F)
        p["tonePhase"] = rng.integers(0, 1 << 32, size=n, dtype=np.uint64).astype(np.uint32)
        p["swn"] = rng.integers(-(1 << 31), 1 << 31, size=n).astype(np.int32)
        p["localEnergy"] = rng.uniform(20000.0, 150000.0, size=n).astype(F)
        p["previousUw"] = rng.uniform(-20.0, 20.0, size=(n, 256)).astype(F)
        p["noiseSeed"] = rng.integers(0, 53125, size=n).astype(F)
        p["noiseOverlap"] = rng.integers(0, 53125, size=(n, 96)).astype(F)
        out.append(p)
    r = rng_seeded(rng.integers(1, 1 << 31, size=n))
    return out[0], out[1], r


def _voiced(p, s):
    return "".join("v" if v == 1 else ("u" if v == 0 else "x") for v in p["Vl"][s, 1:max(int(p["L"][s]), 0) + 1][:56])


def _line(name, cls, s, cur, prev, note=""):
    return (f"{name}[{s}] class {cls}: L {int(cur['L'][s])} prev.L {int(prev['L'][s])} w0 {float(cur['w0'][s]):.9g} prev.w0 {float(prev['w0'][s]):.9g}"
            + (f" {note}" if note else ""))


def _finish(name, cur, prev, rng, cls, notes=None, extra=None):
    n = cur.shape[0]
    assert n <= MAX_STRUCTS and prev.shape[0] == n and rng.shape[0] == n and len(cls) == n, (name, n)
    cls = np.asarray(cls)
    notes = notes if notes is not None else [""] * n
    text = [_line(name, cls[s], s, cur, prev, notes[s]) for s in range(n)]
    return Lattice(name, cur, prev, rng, cls, text, extra or {})


def _cat(parts):
    """parts: [(cur, prev, rng, cls list, notes list)] -> concatenated"""
    cur = np.concatenate([p[0] for p in parts])
    prev = np.concatenate([p[1] for p in parts])
    rng = np.concatenate([p[2] for p in parts])
    cls = sum([list(p[3]) for p in parts], [])
    notes = sum([list(p[4]) for p in parts], [])
    return cur, prev, rng, cls, notes


# ---- pairs -------------------------------------------------------------------------------------------------------------------------
def _pairs(rng):
    s = np.arange(56 * 56)
    L, pL = s // 56 + 1, s % 56 + 1
    near = (s + s // 56) % 2 == 0
    cur, prev, r = _models(s.size, rng, L, pL, near)
    return _finish("pairs", cur, prev, r, np.where(near, "near", "free"))


# ---- voicing -----------------------------------------------------------------------------------------------------------------------
def _voicing(rng):
    parts = []
    for L in (9, 12, 31, 56):
        for pitch in ("stable", "unstable"):
            sets = []   # (note, cur set, prev set, Vl[0], twos)
            all_l = set(range(1, L + 1))
            for k in range(1, L + 1):
                sets += [(f"cur only {k}", {k}, set()), (f"prev only {k}", set(), {k}), (f"both {k}", {k}, {k}), (f"all but {k}", all_l - {k}, all_l - {k})]
            for note, v in (("1..7", set(range(1, 8))), ("8..L", set(range(8, L + 1))), ("7,8", {7, 8}), ("1", {1}), ("L", {L}),
                            ("1..3 (odd interpolated)", {1, 2, 3}), ("1..4 (even interpolated)", {1, 2, 3, 4}), ("all", all_l), ("none", set())):
                sets.append((note, v, v))
            n = len(sets) + 4
            cur, prev, r = _models(n, rng, L, L, True)
            lo, hi = w0_span()
            if pitch == "stable":
                prev["w0"] = np.clip(cur["w0"] * rng.uniform(0.97, 1.03, size=n), lo, hi).astype(F)
            else:
                prev["w0"] = np.where(cur["w0"] > 0.5 * (lo + hi), cur["w0"] * F(0.6), np.minimum(cur["w0"] * F(1.5), hi)).astype(F)
            notes = []
            for i, (note, cv, pv) in enumerate(sets):
                for p, v in ((cur, cv), (prev, pv)):
                    p["Vl"][i] = 0
                    p["Vl"][i, sorted(v)] = 1
                notes.append(note)
            i = len(sets)
            cur["Vl"][i, 0], cur["Vl"][i + 1, 0] = 0, 1
            notes += ["random, Vl[0] = 0", "random, Vl[0] = 1"]
            for j in (i + 2, i + 3):   # Vl = 2: neither voiced nor counted unvoiced
                for p in (cur, prev):
                    p["Vl"][j, rng.choice(np.arange(1, L + 1), size=3, replace=False)] = 2
                notes.append("random with three Vl = 2")
            parts.append((cur, prev, r, [f"L{L}-{pitch}"] * n, notes))
    cur, prev, r, cls, notes = _cat(parts)
    notes = [f"{t}: cur {_voiced(cur, s)} prev {_voiced(prev, s)}" for s, t in enumerate(notes)]
    return _finish("voicing", cur, prev, r, cls, notes)


def bank_forms(cur, prev):
    """what the voiced bank does with each (cur, prev) pair AS THE ORACLE LEFT THEM (lengths reconciled, smoothing applied): a dict of
    bool / int arrays -- interp (number of harmonics in the interpolated branch), from8 (-1: no windowed harmonic; 1: none below 8;
    0: one below 8), all_voiced (no Vl == 0 in 1..L: the unvoiced FFT has nothing to do), all_unvoiced"""
    slot = np.arange(57)[None, :]
    maxl = np.maximum(cur["L"], prev["L"])[:, None]
    band = (slot >= 1) & (slot <= maxl)
    cv, pv = band & (cur["Vl"] == 1), band & (prev["Vl"] == 1)
    stable = np.abs(cur["w0"] - prev["w0"]) < F(0.1) * cur["w0"]
    interp = (slot < 8) & cv & pv & stable[:, None]
    live = (cv | pv) & ~interp
    in_cur = (slot >= 1) & (slot <= cur["L"][:, None])
    return {"interp": interp.sum(axis=1), "from8": np.where(~live.any(axis=1), -1, (~live[:, 1:8].any(axis=1)).astype(int)),
            "all_voiced": ~((cur["Vl"] == 0) & in_cur).any(axis=1), "all_unvoiced": ~((cur["Vl"] != 0) & in_cur).any(axis=1) & ~pv.any(axis=1),
            "stable": stable}


# ---- pitch -------------------------------------------------------------------------------------------------------------------------
def _stable(cw0, pw0):
    """the reference's float expression (src/core/mbelib.c: fabsf(cw0 - pw0) < 0.1f * cw0), in float32"""
    cw0, pw0 = np.asarray(cw0, dtype=F), np.asarray(pw0, dtype=F)
    return np.abs(cw0 - pw0) < F(0.1) * cw0


def _stability_edge(cw0, below):
    """(inside, outside): the two neighbouring floats pw0 on the low (below) or the high side of cw0 between which the test flips"""
    cw0 = F(cw0)
    p = F(cw0 * F(0.9 if below else 1.1))
    away = (lambda x: _next(x, up=not below))
    toward = (lambda x: _next(x, up=below))
    for _ in range(64):
        if _stable(cw0, p):
            q = away(p)
            if not _stable(cw0, q):
                return F(p), F(q)
            p = q
        else:
            p = toward(p)
    raise AssertionError(f"no stability edge next to {cw0}")


def drift_bound(cur, prev):
    """364 sum_l |d_l| g_l of the windowed-voiced harmonics of both models (the bound the voiced bank decides its drift sums by:
    d_l = w0 l - fl(w0 l), g_l = 2 Ml; 52 samples x 7 = 364 int16 LSB per unit), per struct, in double"""
    slot = np.arange(57)[None, :]
    maxl = np.maximum(cur["L"], prev["L"])[:, None]
    band = (slot >= 1) & (slot <= maxl)
    cv, pv = band & (cur["Vl"] == 1), band & (prev["Vl"] == 1)
    interp = (slot < 8) & cv & pv & _stable(cur["w0"], prev["w0"])[:, None]
    total = np.zeros(cur.shape[0])
    for p, v in ((cur, cv), (prev, pv)):
        w = p["w0"][:, None]
        d = w.astype(np.float64) * slot - (w * slot.astype(F)).astype(np.float64)
        total += (np.abs(d) * 2.0 * np.abs(p["Ml"].astype(np.float64)) * (v & ~interp)).sum(axis=1)
    return 364.0 * total


def _pitch(rng):
    lo, hi = w0_span()
    parts = []
    n = 48
    for below in (True, False):
        for inside in (True, False):
            L = rng.integers(9, 57, size=n)
            cur, prev, r = _models(n, rng, L, L, True)
            cur["w0"] = rng.uniform(lo * 1.15, hi * 0.88, size=n).astype(F)
            for s in range(n):
                a, b = _stability_edge(cur["w0"][s], below)
                prev["w0"][s] = a if inside else b
            assert (_stable(cur["w0"], prev["w0"]) == inside).all()
            for p in (cur, prev):
                p["Vl"][:, 1:8] = 1   # (the interpolated branch is what the test switches)
            parts.append((cur, prev, r, [f"edge-{'low' if below else 'high'}-{'in' if inside else 'out'}"] * n, [""] * n))
    for name, step in (("dw0-zero", 0), ("dw0-ulp-up", 1), ("dw0-ulp-down", -1)):
        L, pL = rng.integers(1, 57, size=n), rng.integers(1, 57, size=n)
        cur, prev, r = _models(n, rng, L, pL, True)
        prev["w0"] = cur["w0"] if step == 0 else _next(cur["w0"], up=step > 0)
        parts.append((cur, prev, r, [name] * n, [""] * n))
    for name, f in (("pi-below", 1.0 - 1e-3), ("pi-above", 1.0 + 1e-3)):
        L = rng.integers(int(math.pi / hi) + 2, 57, size=n)
        cur, prev, r = _models(n, rng, L, L, True)
        cur["w0"] = (math.pi / L * f).astype(F)
        assert ((cur["w0"] > lo) & (cur["w0"] < hi)).all()
        prev["w0"] = np.clip(cur["w0"] * rng.uniform(0.97, 1.03, size=n), lo, hi).astype(F)
        got = cur["w0"].astype(np.float64) * L
        assert ((got < math.pi) if f < 1 else (got > math.pi)).all()
        parts.append((cur, prev, r, [name] * n, [f"w0 L = {g:.6f}" for g in got]))
    for name, target in (("drift-below", 0.0625), ("drift-above", 0.25)):
        # d_l is a rounding error of w0 l, so it grows with w0 l: high fundamentals, long models, most harmonics voiced, and the amplitude
        # on the harmonics whose d_l is large -- the bound is then met at both levels by sums that stay below the amplitude rule's 3000
        L, pL = rng.integers(44, 57, size=n), rng.integers(44, 57, size=n)
        cur, prev, r = _models(n, rng, L, pL, np.arange(n) % 2 == 0)
        cur["w0"] = rng.uniform(0.27, hi, size=n).astype(F)
        prev["w0"] = np.where(np.arange(n) % 2 == 0, np.clip(cur["w0"] * rng.uniform(0.92, 1.08, size=n), 0.25, hi), rng.uniform(0.25, hi, size=n)).astype(F)
        slot = np.arange(57)[None, :]
        for p in (cur, prev):
            p["Vl"][:, 8:] |= (np.arange(8, 57)[None, :] <= p["L"][:, None]) & (rng.random((n, 49)) < 0.8)
            w = p["w0"][:, None]
            d = np.abs(w.astype(np.float64) * slot - (w * slot.astype(F)).astype(np.float64))
            d = np.where((slot >= 8) & (slot <= p["L"][:, None]) & (p["Vl"] == 1), d, 0.0)
            p["Ml"] = np.where((d > 0) & (d >= np.sort(d, axis=1)[:, -12][:, None]), F(3000.0 / (2 * 12)) * rng.uniform(0.5, 1.0, size=(n, 57)).astype(F), F(0.0))
        b = drift_bound(cur, prev)
        assert (b > 0).all()
        for p in (cur, prev):
            p["Ml"] = (p["Ml"] * (target / b)[:, None]).astype(F)
            assert (2.0 * p["Ml"].astype(np.float64).sum(axis=1) < 3000.0).all(), f"pitch {name}: the amplitudes leave the rule ({2.0 * p['Ml'].sum(axis=1).max():.0f})"
        b = drift_bound(cur, prev)
        assert np.allclose(b, target, rtol=1e-4)
        parts.append((cur, prev, r, [name] * n, [f"364 sum |d| g = {x:.5f}" for x in b]))
    return _finish("pitch", *_cat(parts))


# ---- phase -------------------------------------------------------------------------------------------------------------------------
def _near_two_pi(rng, shape, top, step):
    """floats next to multiples of 2 pi below `top`: the float nearest to k 2 pi, moved by `step` float steps"""
    k = np.floor(10.0 ** rng.uniform(0.0, math.log10(top / TWO_PI), size=shape))
    f = (k * TWO_PI).astype(F)
    return _next(f, up=step > 0, steps=abs(step)) if step else f


def _phase(rng):
    n = 48
    parts = []

    def base():
        L, pL = rng.integers(1, 57, size=n), rng.integers(1, 57, size=n)
        return _models(n, rng, L, pL, np.arange(n) % 2 == 0)

    for name, step in (("psi-2pi-below", -1), ("psi-2pi-at", 0), ("psi-2pi-above", 1)):
        cur, prev, r = base()
        prev["PSIl"][:, 1:] = _near_two_pi(rng, (n, 56), 3.9e6, step)
        parts.append((cur, prev, r, [name] * n, [""] * n))
    cur, prev, r = base()
    prev["PSIl"][:, 1:] = 0.0
    parts.append((cur, prev, r, ["psi-zero"] * n, [""] * n))
    cur, prev, r = base()
    prev["PSIl"][:, 1:] = -(10.0 ** rng.uniform(-3.0, 6.5, size=(n, 56))).astype(F)
    prev["PSIl"][:, 1:5] = -_near_two_pi(rng, (n, 4), 3.9e6, 1)
    parts.append((cur, prev, r, ["psi-negative"] * n, [""] * n))
    cur, prev, r = base()
    prev["PSIl"][:, 1:] = (10.0 ** rng.uniform(math.log10(4e6), 9.0, size=(n, 56))).astype(F)
    prev["PSIl"][:, 1] = F(4e6)
    prev["PSIl"][:, 2] = _next(F(4e6), up=False)
    prev["PSIl"][:, 3] = F(1e9)
    parts.append((cur, prev, r, ["psi-huge"] * n, [""] * n))
    cur, prev, r = base()
    for p in (cur, prev):
        p["PHIl"][:, 1:] = np.where(rng.integers(0, 2, size=(n, 56)) == 1, F(4000.0), F(-4000.0))
    parts.append((cur, prev, r, ["phi-edge"] * n, [""] * n))
    cur, prev, r = base()
    for p in (cur, prev):
        sign = np.where(rng.integers(0, 2, size=(n, 56)) == 1, 1.0, -1.0).astype(F)
        p["PHIl"][:, 1:] = sign * _near_two_pi(rng, (n, 56), 4000.0, 1) * np.where(np.arange(56) % 2 == 0, 1, 0).astype(F) \
            + sign * _near_two_pi(rng, (n, 56), 4000.0, -1) * np.where(np.arange(56) % 2 == 1, 1, 0).astype(F)
    parts.append((cur, prev, r, ["phi-2pi"] * n, [""] * n))
    return _finish("phase", *_cat(parts))


# ---- gate --------------------------------------------------------------------------------------------------------------------------
def _gate(rng):
    n = 24
    parts = []

    def base(m=n):
        L, pL = rng.integers(1, 57, size=m), rng.integers(1, 57, size=m)
        return _models(m, rng, L, pL, np.arange(m) % 2 == 0)

    cur, prev, r = base(48)
    notes = []
    for s in range(48):
        bad = (0, 57, -1, 1000)[s % 4]
        where = ("cur", "prev", "both")[(s // 4) % 3]
        if where in ("cur", "both"):
            cur["L"][s] = bad
        if where in ("prev", "both"):
            prev["L"][s] = bad
        notes.append(f"{where} L = {bad}")
    parts.append((cur, prev, r, ["L-invalid"] * 48, notes))
    for rc in (3, 4):
        cur, prev, r = base()
        cur["repeatCount"] = rc
        parts.append((cur, prev, r, [f"repeat-{rc}"] * n, [""] * n))
    for name, thr in (("mute-imbe", MUTE_IMBE), ("mute-ambe", MUTE_AMBE), ("mute-near-ambe", F(MUTE_AMBE + F(2e-6)))):
        for side, up in (("below", False), ("at", None), ("above", True)):
            cur, prev, r = base()
            cur["mutingThreshold"] = thr
            cur["errorRate"] = thr if up is None else _next(thr, up=up)
            cur["errorCountTotal"] = rng.integers(0, 12, size=n)
            parts.append((cur, prev, r, [f"{name}-{side}"] * n, [f"errorRate {float(e):.9g} threshold {float(thr):.9g}" for e in cur["errorRate"]]))
    for name, override in (("seed-negative-override", 1), ("seed-negative-plain", 0)):
        cur, prev, r = base()
        cur["noiseSeed"] = np.where(np.arange(n) % 2 == 0, F(-1.0), F(-0.25))
        r["unvoiced_seed_override"] = override
        parts.append((cur, prev, r, [name] * n, [""] * n))
    cur, prev, r = base()
    cur["noiseSeed"] = np.where(np.arange(n) % 2 == 0, F(100.7), rng.uniform(0.0, 53124.0, size=n).astype(F))
    parts.append((cur, prev, r, ["seed-fraction"] * n, [f"noiseSeed {float(x):.9g}" for x in cur["noiseSeed"]]))
    cur, prev, r = base()
    cur["noiseSeed"] = (10.0 ** rng.uniform(math.log10(53125.0), math.log10(2147483000.0), size=n)).astype(F)
    cur["noiseSeed"][:3] = (F(53125.0), F(2147483520.0), F(16777216.0))
    assert (cur["noiseSeed"] < F(2.0 ** 31)).all()
    parts.append((cur, prev, r, ["seed-large"] * n, [f"noiseSeed {float(x):.9g}" for x in cur["noiseSeed"]]))
    for seeded in (0, 1):   # the comfort noise of a muted frame, from an unseeded and a seeded generator
        cur, prev, r = base()
        cur["repeatCount"] = 4
        r["cn_seeded"] = seeded
        parts.append((cur, prev, r, [f"noise-seeded-{seeded}"] * n, [""] * n))
    return _finish("gate", *_cat(parts))


# ---- energy ------------------------------------------------------------------------------------------------------------------------
def _seq_sum(x):
    """sum of float32 values one after the other, in float32 (the reference's loops)"""
    s = F(0.0)
    for v in np.asarray(x, dtype=F):
        s = F(s + v)
    return s


def reference_vm(cur, prev, s):
    """VM of struct s with the reference's float sequence (src/core/mbe_adaptive.c:164-195), in numpy float32; None where it is FLT_MAX"""
    L = int(cur["L"][s])
    ml = cur["Ml"][s, 1:L + 1]
    rm0 = _seq_sum(ml * ml)
    er, et, e4 = F(cur["errorRate"][s]), int(cur["errorCountTotal"][s]), int(cur["errorCount4"][s])
    pe = F(prev["localEnergy"][s])
    if pe < F(10000.0):
        pe = F(75000.0)
    le = F(F(F(0.95) * pe) + F(F(0.05) * rm0))
    if le < F(10000.0):
        le = F(10000.0)
    if er <= F(0.005) and et <= 4:
        return None
    x8 = np.sqrt(np.sqrt(np.sqrt(le, dtype=F), dtype=F), dtype=F)
    energy = F(F(x8 * x8) * x8)
    if er <= F(0.0125) and e4 == 0:
        return F(F(F(45.255) * energy) / F(math.exp(float(F(F(277.26) * er)))))
    return F(F(1.414) * energy)


VM_STEPS = (0.0, 1e-7, 1e-6, 1e-5, 3e-5, 6e-5, 1e-3)


def _energy(rng):
    parts = []

    def base(m):
        L, pL = rng.integers(2, 57, size=m), rng.integers(1, 57, size=m)
        cur, prev, r = _models(m, rng, L, pL, np.arange(m) % 2 == 0)
        return cur, prev, r

    combos = [(er, up, et, e4) for er in (0.005, 0.0125) for up in (False, True) for et in (4, 5, 6, 7) for e4 in (0, 1)]
    m = 2 * len(combos)
    cur, prev, r = base(m)
    notes = []
    for s in range(m):
        er, up, et, e4 = combos[s % len(combos)]
        cur["errorRate"][s] = F(er) if (s >= len(combos) and not up) else _next(F(er), up=up)
        cur["errorCountTotal"][s], cur["errorCount4"][s] = et, e4
        notes.append(f"errorRate {float(cur['errorRate'][s]):.9g} total {et} c4 {e4}")
    parts.append((cur, prev, r, ["rate-counts"] * m, notes))
    m = 36
    cur, prev, r = base(m)
    le = [_next(F(10000.0), up=False), F(10000.0), _next(F(10000.0)), F(0.0), F(-5.0), F(9000.0)]
    prev["localEnergy"] = np.resize(np.array(le, dtype=F), m)
    cur["errorRate"], cur["errorCountTotal"] = F(0.02), 7
    cur["Ml"] *= F(0.05)   # (quiet: the local energy then sits at its floor on one side)
    parts.append((cur, prev, r, ["prev-energy"] * m, [f"prev.localEnergy {float(x):.9g}" for x in prev["localEnergy"]]))
    m = 40
    cur, prev, r = base(m)
    prev["amplitudeThreshold"] = np.resize(np.array([-5, 0, 1, 20480, 1 << 20], dtype=np.int32), m)
    cur["errorRate"], cur["errorCountTotal"] = F(0.02), np.resize(np.array([7, 19], dtype=np.int32), m)
    parts.append((cur, prev, r, ["prev-threshold"] * m, [f"prev.amplitudeThreshold {int(x)}" for x in prev["amplitudeThreshold"]]))
    for name, et, tm in (("sum-at-positive-threshold", 19, 301), ("sum-at-negative-threshold", 21, -299)):
        m = 48
        cur, prev, r = base(m)
        prev["amplitudeThreshold"] = 1
        cur["errorRate"], cur["errorCountTotal"] = F(0.004), et   # (Tm = 6000 - 300 et + 1)
        notes = []
        for s in range(m):
            L = int(cur["L"][s])
            f = (1.0 - 1e-3, 1.0 + 1e-3, 1.0 - 2e-7, 1.0 + 2e-7)[s % 4]
            cur["Ml"][s] = (cur["Ml"][s] * (abs(tm) * f / float(cur["Ml"][s, 1:L + 1].astype(np.float64).sum()))).astype(F)
            notes.append(f"sum Ml = {abs(tm)} x {f:.7f}, Tm = {tm}")
        parts.append((cur, prev, r, [name] * m, notes))
    for path, er in (("vm-plain", 0.02), ("vm-exp", 0.01)):
        for d in VM_STEPS:
            for sign in ((0,) if d == 0.0 else (-1, 1)):
                m = 8
                cur, prev, r = base(m)
                cur["errorRate"], cur["errorCountTotal"], cur["errorCount4"] = F(er), 5, 0
                cur["Ml"] *= F(0.02)   # (the other amplitudes stay well below VM)
                notes = []
                for s in range(m):
                    L = int(cur["L"][s])
                    k = int(rng.integers(1, L + 1))
                    cur["Vl"][s, k] = 0
                    a = F(100.0)
                    for _ in range(8):
                        cur["Ml"][s, k] = a
                        vm = reference_vm(cur, prev, s)
                        a = F(vm * (1.0 + sign * d))
                        if d > 0 and a == vm:
                            a = _next(vm, up=sign > 0)
                        if a == cur["Ml"][s, k]:
                            break
                    cur["Ml"][s, k] = a
                    notes.append(f"Ml[{k}] = VM x (1 {'+' if sign >= 0 else '-'} {d:g}) = {float(a):.9g}")
                tag = "at" if d == 0.0 else f"{'above' if sign > 0 else 'below'}-{d:g}"
                parts.append((cur, prev, r, [path] * m, [f"{tag}: {t}" for t in notes]))
    return _finish("energy", *_cat(parts))


# ---- weights -----------------------------------------------------------------------------------------------------------------------
SHAPES = ("flat", "single", "decay-0.7", "grow-1.3", "gaps", "all-zero")


def _shape(name, L, rng):
    ml = np.zeros(57, dtype=np.float64)
    l = np.arange(1, L + 1)
    a = 10.0 ** rng.uniform(0.0, 3.0)
    if name == "flat":
        ml[1:L + 1] = a
    elif name == "single":
        ml[int(rng.integers(1, L + 1))] = a
    elif name == "decay-0.7":
        ml[1:L + 1] = a * 0.7 ** (l - 1)
    elif name == "grow-1.3":
        ml[1:L + 1] = a * 1e-3 * 1.3 ** (l - 1)
    elif name == "gaps":
        ml[1:L + 1] = a * rng.random(L) * (l % 2)
    return ml.astype(F)


def _weights(rng):
    lo, hi = w0_span()
    parts = []
    grid = lo + (hi - lo) * (np.arange(24) + 0.37) / 24.0
    s = np.arange(56 * 24)
    L, wi = s // 24 + 1, s % 24
    cur, prev, r = _models(s.size, rng, L, L)
    cur["w0"] = grid[wi].astype(F)
    cls = []
    for k in range(s.size):
        shape = SHAPES[(L[k] + 5 * wi[k]) % len(SHAPES)]
        cur["Ml"][k] = _shape(shape, int(L[k]), rng)
        cls.append(shape)
    parts.append((cur, prev, r, cls, [""] * s.size))
    n = 48
    cur, prev, r = _models(n, rng, rng.integers(2, 57, size=n))
    for k in range(n):
        cur["Ml"][k, int(rng.integers(int(cur["L"][k]) // 8 + 1, int(cur["L"][k]) + 1))] *= F(-1.0)   # (a harmonic the weights apply to)
    parts.append((cur, prev, r, ["negative"] * n, [""] * n))
    for name, draw in (("w0-low", lambda: rng.uniform(0.005, 0.04, size=n)), ("w0-high", lambda: rng.uniform(0.55, 1.0, size=n)),
                       ("w0-zero", lambda: np.zeros(n)), ("w0-ge1", lambda: np.concatenate([[1.0], rng.uniform(1.0, 3.0, size=n - 1)]))):
        cur, prev, r = _models(n, rng, rng.integers(1, 57, size=n))
        cur["w0"] = draw().astype(F)
        parts.append((cur, prev, r, [name] * n, [""] * n))
    return _finish("weights", *_cat(parts))


# ---- tones -------------------------------------------------------------------------------------------------------------------------
TONE_AD = (0, 1, 64, 126, 127)
TONE_SWN = (0, 1, -1, -(1 << 31), 0x7FFFFFFF)


def tone_bits(rng, ids, ad):
    """49 parameter bits that carry tone id ID1 (bits 12..19) and amplitude AD (bits 6..11 and 44), the rest random"""
    n = len(ids)
    bits = rng.integers(0, 2, size=(n, 49), dtype=np.uint8)
    for j in range(8):
        bits[:, 12 + j] = (np.asarray(ids) >> (7 - j)) & 1
    for j in range(6):
        bits[:, 6 + j] = (np.asarray(ad) >> (6 - j)) & 1
    bits[:, 44] = np.asarray(ad) & 1
    return bits


def _tones(rng):
    s = np.arange(256 * len(TONE_AD))
    ids, ad = s // len(TONE_AD), np.array(TONE_AD)[s % len(TONE_AD)]
    cur, prev, r = _models(s.size, rng, 12)
    cur["swn"] = np.array(TONE_SWN, dtype=np.int64)[(s // 7) % len(TONE_SWN)].astype(np.int32)
    third = (s // 3) % 3
    cur["tonePhase"] = np.where(third == 0, 0, np.where(third == 1, 0xFFFFFFFF, cur["tonePhase"])).astype(np.uint32)
    bits = tone_bits(rng, ids, ad)
    dual = (ids >= 128) & (ids <= 163)
    single = (ids >= 5) & (ids <= 122)
    cls = np.where(dual, "dual", np.where(single, "single", "no-tone"))
    notes = [f"id {i} AD {a} swn {int(w)} tonePhase {int(t)}" for i, a, w, t in zip(ids, ad, cur["swn"], cur["tonePhase"])]
    return _finish("tones", cur, prev, r, cls, notes, {"bits": bits, "ids": ids, "ad": ad})


def _tones_dstar(rng):
    ids = np.arange(-5, 301)
    cur, prev, r = _models(ids.size, rng, 12)
    s = np.arange(ids.size)
    cur["swn"] = np.array(TONE_SWN, dtype=np.int64)[s % len(TONE_SWN)].astype(np.int32)
    cls = np.where((ids >= 5) & (ids <= 122), "single", "no-tone")
    return _finish("tones_dstar", cur, prev, r, cls, [f"id {i} swn {int(w)}" for i, w in zip(ids, cur["swn"])], {"ids": ids.astype(np.int32)})


# ---- predict -----------------------------------------------------------------------------------------------------------------------
B0_BITS = {0: (0, 1, 2, 3, 4, 5, 85, 86), 1: (0, 1, 2, 3, 37, 38, 39), 3: (0, 1, 2, 3, 4, 5, 48)}
PREV_L = (9, 30, 56)
MEMORIES = ("patterned", "plus100", "minus100", "zero")


def _predict(codec, rng):
    nb0 = 1 << len(B0_BITS[codec])
    nbits = 88 if codec == 0 else 49
    reps = len(PREV_L) * len(MEMORIES)
    n = nb0 * reps
    s = np.arange(n)
    b0, k = s // reps, s % reps
    pL, mem = np.array(PREV_L)[k % len(PREV_L)], k // len(PREV_L)
    cur, prev, r = _models(n, rng, pL, pL)
    slot = np.arange(57)[None, :]
    pattern = (6.0 + 3.0 * np.sin(0.7 * slot + s[:, None])).astype(F)
    prev["log2Ml"] = np.where((mem == 0)[:, None], pattern, np.where((mem == 1)[:, None], F(100.0), np.where((mem == 2)[:, None], F(-100.0), F(0.0)))).astype(F)
    bits = rng.integers(0, 2, size=(n, nbits), dtype=np.uint8)
    for j, at in enumerate(B0_BITS[codec]):
        bits[:, at] = (b0 >> (len(B0_BITS[codec]) - 1 - j)) & 1
    cls = [f"{MEMORIES[m]}" for m in mem]
    notes = [f"b0 {int(b)} memory {MEMORIES[m]}" for b, m in zip(b0, mem)]
    return _finish(f"predict{codec}", cur, prev, r, cls, notes, {"bits": bits, "b0": b0, "codec": codec})


_BUILDERS = {"pairs": _pairs, "voicing": _voicing, "pitch": _pitch, "phase": _phase, "gate": _gate, "energy": _energy, "weights": _weights,
             "tones": _tones, "tones_dstar": _tones_dstar, "predict0": lambda r: _predict(0, r), "predict1": lambda r: _predict(1, r),
             "predict3": lambda r: _predict(3, r)}
NAMES = tuple(_BUILDERS)


@functools.lru_cache(maxsize=None)
def build(name):
    """the lattice `name`: the same bytes every time (framegen.rng_for, one fixed tag per lattice)"""
    return _BUILDERS[name](framegen.rng_for(0x30DE1000 + TAGS[name]))


def lattice_bytes(name):
    """every input byte of a freshly built lattice (no cache)"""
    lat = _BUILDERS[name](framegen.rng_for(0x30DE1000 + TAGS[name]))
    extra = b"".join(np.ascontiguousarray(v).tobytes() for k, v in sorted(lat.extra.items()) if isinstance(v, np.ndarray))
    return lat.cur.tobytes() + lat.prev.tobytes() + lat.rng.tobytes() + extra + "\n".join(lat.text).encode()


def groups(name):
    """[(class, indices)]: the structs of each class in groups of at most GROUP, the unit the float bounds are applied to"""
    lat = build(name)
    out = []
    for c in sorted(set(lat.cls.tolist())):
        idx = np.flatnonzero(lat.cls == c)
        for a in range(0, idx.size, GROUP):
            out.append((c, idx[a:a + GROUP]))
    return out


def shim_sample(name):
    """a strided sample of SHIM_SAMPLE structs of a lattice"""
    n = build(name).cur.shape[0]
    return np.unique(np.linspace(0, n - 1, SHIM_SAMPLE).astype(np.int64))


# ---- the oracle's answers --------------------------------------------------------------------------------------------------------
def _declare(o):
    h = o.h
    h.mbxo_decode_ambe2400_parms.restype = C.c_int
    h.mbxo_decode_ambe2400_parms.argtypes = [C.c_void_p] * 3
    return h


def _each(arr):
    base, step = arr.ctypes.data, arr.strides[0]
    return [base + i * step for i in range(arr.shape[0])]


@functools.lru_cache(maxsize=None)
def oracle(name, entry):
    """what the oracle makes of lattice `name` through `entry` (a key of ENTRIES): a dict with the structs as it left them and what the
    call returned.  Made once, shared by every test: read it, never write to it."""
    assert name in ENTRIES[entry], (name, entry)
    o = oracle_lib.load()
    h = _declare(o)
    lat = build(name)
    n = lat.cur.shape[0]
    cur, prev, rng = lat.cur.copy(), lat.prev.copy(), lat.rng.copy()
    if entry == "speech":
        pcmf, cur, prev, rng = o.synthesize_speech(cur, prev, rng)
        return {"pcmf": pcmf, "pcm16": o.floattoshort(pcmf), "cur": cur, "prev": prev, "rng": rng}
    if entry == "smoothing":
        for c, p in zip(_each(cur), _each(prev)):
            h.mbxo_adaptive_smoothing(c, p)
        return {"cur": cur, "prev": prev}
    if entry == "enhance":
        rm0 = np.array([h.mbxo_spectral_amp_enhance(c) for c in _each(cur)], dtype=F)
        return {"cur": cur, "rm0": rm0}
    if entry == "noise":   # mbe_synthesizeComfortNoisef on the RNG structs of the lattice alone
        pcmf = np.zeros((n, 160), dtype=F)
        for pp, rp in zip(_each(pcmf), _each(rng)):
            h.mbxo_comfort_noisef(pp, rp)
        return {"pcmf": pcmf, "pcm16": o.floattoshort(pcmf), "rng": rng}
    if entry in ("tone", "tone_dstar"):
        out = {}
        for tones_on in (1, 0):
            o.set_tones(tones_on)
            try:
                c = lat.cur.copy()
                calls = []
                for _ in range(2):   # two calls in a row on the same struct: the second starts from the phases the first left
                    pcm = np.zeros((n, 160), dtype=F)
                    if entry == "tone":
                        bits = np.ascontiguousarray(lat.extra["bits"], dtype=np.int8)
                        for i, (cp, bp, pp) in enumerate(zip(_each(c), _each(bits), _each(pcm))):
                            h.mbxo_tonef(pp, bp, cp)
                    else:
                        for i, (cp, pp) in enumerate(zip(_each(c), _each(pcm))):
                            h.mbxo_tone_dstarf(pp, cp, int(lat.extra["ids"][i]))
                    calls.append((pcm, c.copy()))
                out["on" if tones_on else "off"] = calls
            finally:
                o.set_tones(1)
        return out
    assert entry == "decode_parms"
    codec = lat.extra["codec"]
    bits = np.ascontiguousarray(lat.extra["bits"], dtype=np.int8)
    rc = np.zeros(n, dtype=np.int32)
    for i, (cp, pp, bp) in enumerate(zip(_each(cur), _each(prev), _each(bits))):
        if codec == 0:
            rc[i] = h.mbxo_decode_imbe4400_parms(bp, cp, pp)
        elif codec == 1:
            rc[i] = h.mbxo_decode_ambe2450_parms(bp, cp, pp, 0)
        else:
            rc[i] = h.mbxo_decode_ambe2400_parms(bp, cp, pp)
    return {"cur": cur, "prev": prev, "rc": rc}


def records(name):
    """the parameter records of a lattice that carries bits (tones, predict*): no bit errors"""
    from mbelib_neo_amd import decoder

    lat = build(name)
    return decoder.records_from_bits(lat.extra["bits"], total_errors=np.zeros(lat.cur.shape[0], dtype=np.int32))


def below_clip(pcmf):
    """per struct: the oracle's frame stays below the soft clip"""
    return ~parity.clipped_frames(pcmf)


def untouched(name, entry):
    """bool [n]: structs the entry point must leave byte for byte as they are (an L outside 1..56 on either side)"""
    lat = build(name)
    bad = (lat.cur["L"] < 1) | (lat.cur["L"] > 56)
    if entry in ("speech", "smoothing"):
        bad |= (lat.prev["L"] < 1) | (lat.prev["L"] > 56)
    return bad


def muted(name):
    """bool [n]: structs whose frame is comfort noise in the oracle's reading of the reference (max repeats, or an error rate over a
    threshold that is not AMBE's)"""
    ref = oracle(name, "speech")
    c = ref["cur"]
    rate = np.abs(c["mutingThreshold"] - MUTE_AMBE) > F(1e-6)
    return ~untouched(name, "speech") & ((c["repeatCount"] >= 4) | (rate & (c["errorRate"] > c["mutingThreshold"])))


# ---- composition: from the oracle alone, the lattice holds what it claims ---------------------------------------------------------
def composition(name):
    lat = build(name)
    n = lat.cur.shape[0]
    assert n <= MAX_STRUCTS
    out = {"structs": n, "classes": len(set(lat.cls.tolist()))}
    lo, hi = w0_span()
    if name in SYNTHESIS:
        ref = oracle(name, "speech")
        ok = ~untouched(name, "speech")
        forms = bank_forms(ref["cur"], ref["prev"])
        below = float(np.mean(below_clip(ref["pcmf"])))
        out["below_clip"] = round(below, 4)
        assert np.isfinite(ref["pcmf"]).all(), f"{name}: the oracle's PCM is not finite"
        assert below >= MIN_SHARE_BELOW_CLIP, f"{name}: only {below:.3f} of the structs stay below the soft clip"
        assert ((lat.cur["w0"] >= lo) & (lat.cur["w0"] <= hi) & (lat.prev["w0"] >= lo) & (lat.prev["w0"] <= hi)).all(), f"{name}: a w0 outside the table span"
        out.update(stable=int(forms["stable"][ok].sum()), unstable=int((~forms["stable"][ok]).sum()))
    if name == "pairs":
        seen = np.zeros((57, 57), dtype=bool)
        seen[lat.cur["L"], lat.prev["L"]] = True
        assert seen[1:, 1:].all(), "pairs: an (L, prev.L) is missing"
        assert forms["stable"].any() and (~forms["stable"]).any()
        band = lat.cur["Vl"][:, 1:4]
        assert ((band[:, 0] != band[:, 1]) | (band[:, 1] != band[:, 2])).mean() > 0.5, "pairs: voicing is not per harmonic"
    if name == "voicing":
        st = forms["stable"]
        assert (forms["from8"] == 1).any() and (forms["from8"] == 0).any(), "voicing: one from8 outcome only"
        odd, even = (forms["interp"] % 2 == 1), (forms["interp"] > 0) & (forms["interp"] % 2 == 0)
        assert odd.any() and even.any(), "voicing: one imask parity only"
        assert forms["all_voiced"].any() and forms["all_unvoiced"].any(), "voicing: no all-voiced or no all-unvoiced frame"
        assert (st & (forms["interp"] > 0)).any() and (~st & (forms["interp"] == 0)).any()
        assert (lat.cur["Vl"] == 2).any() and (ref["cur"]["Vl"] == 2).any(), "voicing: no Vl = 2"
        assert set(lat.cur["Vl"][:, 0].tolist()) >= {0, 1}
        out.update(from8=int((forms["from8"] == 1).sum()), interp_odd=int(odd.sum()), interp_even=int(even.sum()),
                   all_voiced=int(forms["all_voiced"].sum()), all_unvoiced=int(forms["all_unvoiced"].sum()))
    if name == "pitch":
        for side in ("low", "high"):
            a, b = lat.cls == f"edge-{side}-in", lat.cls == f"edge-{side}-out"
            assert forms["stable"][a].all() and not forms["stable"][b].any(), f"pitch: the {side} edge is not where the float test flips"
            assert (forms["interp"][a] > 0).all() and (forms["interp"][b] == 0).all()
        z = lat.cls == "dw0-zero"
        assert (lat.cur["w0"][z] == lat.prev["w0"][z]).all() and (lat.cur["w0"][lat.cls == "dw0-ulp-up"] != lat.prev["w0"][lat.cls == "dw0-ulp-up"]).all()
        b = drift_bound(ref["cur"], ref["prev"])
        lo_c, hi_c = lat.cls == "drift-below", lat.cls == "drift-above"
        # (the kernel's own estimate is between 1 and sqrt 2 times this bound: a factor of two on either side of 0.125 decides it)
        assert (b[lo_c] * math.sqrt(2.0) < 0.125).all() and (b[hi_c] > 0.125).all(), "pitch: the drift bound is not on either side of 0.125"
        out.update(drift_below=float(b[lo_c].max()), drift_above=float(b[hi_c].min()))
    if name == "phase":
        psi = lat.prev["PSIl"][:, 1:]
        assert (psi[lat.cls == "psi-huge"] >= F(4e6)).any() and (psi[lat.cls == "psi-negative"] < 0).all() and (psi[lat.cls == "psi-zero"] == 0).all()
        w = ref["prev"]["PSIl"][:, 1:]
        assert ((w >= 0) & (w < F(TWO_PI))).all(), "phase: the oracle leaves a prev.PSIl outside [0, 2 pi)"
        near = lat.cls == "psi-2pi-below"
        assert (w[near] > 6.0).mean() > 0.9 and (w[lat.cls == "psi-2pi-above"] < 0.3).mean() > 0.9, "phase: the values are not on either side of a multiple of 2 pi"
    if name == "gate":
        bad = untouched(name, "speech")
        assert bad.sum() == 48 and not ref["pcmf"][bad].any()
        for x in ("cur", "prev", "rng"):
            assert ref[x][bad].tobytes() == getattr(lat, x)[bad].tobytes(), "gate: the oracle touches a struct behind an invalid L"
        m = muted(name)
        want = {"repeat-3": False, "repeat-4": True, "mute-imbe-below": False, "mute-imbe-at": False, "mute-imbe-above": True, "mute-ambe-below": False,
                "mute-ambe-above": False, "mute-near-ambe-below": False, "mute-near-ambe-above": True, "noise-seeded-0": True, "noise-seeded-1": True}
        for c, v in want.items():
            assert (m[lat.cls == c] == v).all(), f"gate: class {c} is {'not ' if v else ''}muted"
        # a muted frame is the comfort-noise generator's: the model's noise state stays
        assert ref["cur"]["noiseSeed"][m].tobytes() == lat.cur["noiseSeed"][m].tobytes()
        neg = lat.cls == "seed-negative-override"
        assert (ref["cur"]["noiseSeed"][neg] == lat.rng["unvoiced_seed_state"][neg]).all() and (ref["rng"]["unvoiced_seed_override"][neg] == 0).all()
        assert (ref["cur"]["noiseSeed"][lat.cls == "seed-negative-plain"] == 3147.0).all()
        out["muted"] = int(m.sum())
    if name == "energy":
        sm = oracle(name, "smoothing")
        for which, got in (("speech", ref["cur"]), ("smoothing", sm["cur"])):
            forced = ((got["Vl"] == 1) & (lat.cur["Vl"] == 0) & (np.arange(57)[None, :] <= lat.cur["L"][:, None]) & (np.arange(57)[None, :] >= 1)).any(axis=1)
            for path in ("vm-plain", "vm-exp"):
                # (with expf in VM, one step from it is a matter of the last bit of the library's expf: asserted from 1e-6 on)
                for d in (VM_STEPS[1:] if path == "vm-plain" else VM_STEPS[2:]):
                    up = np.array([c == path and f" above-{d:g}:" in t for c, t in zip(lat.cls, lat.text)])
                    dn = np.array([c == path and f" below-{d:g}:" in t for c, t in zip(lat.cls, lat.text)])
                    assert up.sum() == 8 and dn.sum() == 8, (path, d, up.sum(), dn.sum())
                    assert forced[up].all() and not forced[dn].any(), f"energy ({which}): {path} at d = {d:g}: forced {forced[up].sum()} of 8 above, {forced[dn].sum()} of 8 below"
            at = np.array([c in ("vm-plain", "vm-exp") and " at: " in t for c, t in zip(lat.cls, lat.text)])
            assert at.sum() == 16 and not forced[at & (lat.cls == "vm-plain")].any(), f"energy ({which}): an amplitude equal to VM is forced"
            out[f"forced_{which}"] = int(forced.sum())
            thr = set(got["amplitudeThreshold"].tolist())
            assert {301, -299, 20480} <= thr, f"energy ({which}): amplitude thresholds {sorted(thr)[:8]}"
            neg = lat.cls == "sum-at-negative-threshold"
            assert (got["Ml"][neg] <= 0).all() and (got["Ml"][neg] < 0).any(), "energy: no negative scaled amplitudes"
            pos = lat.cls == "sum-at-positive-threshold"
            scaled = (got["Ml"][pos] != lat.cur["Ml"][pos]).any(axis=1)
            assert scaled.any() and (~scaled).any(), "energy: the amplitude sum is on one side of Tm only"
            le = got["localEnergy"][lat.cls == "prev-energy"]
            assert (le == 10000.0).any() and (le > 10000.0).any()
    if name == "weights":
        ref = oracle(name, "enhance")
        inside = np.isin(lat.cls, SHAPES + ("negative",))
        assert ((lat.cur["w0"][inside] >= lo) & (lat.cur["w0"][inside] <= hi)).all()
        seen = np.zeros(57, dtype=int)
        np.add.at(seen, lat.cur["L"][np.isin(lat.cls, SHAPES)], 1)
        assert (seen[1:] == 24).all()
        nan = np.isnan(ref["cur"]["Ml"]).any(axis=1)
        assert nan[lat.cls == "negative"].all(), "weights: a negative amplitude without a NaN"
        assert not nan[np.isin(lat.cls, SHAPES)].any(), "weights: a NaN inside the span"
        z = lat.cls == "all-zero"
        assert ref["cur"]["Ml"][z].tobytes() == lat.cur["Ml"][z].tobytes()
        for lohi in ("w0-low", "w0-high", "w0-ge1"):
            w = lat.cur["w0"][lat.cls == lohi]
            assert ((w < lo) | (w > hi)).all()
        assert (lat.cur["w0"][lat.cls == "w0-ge1"] >= 1).all() and (lat.cur["w0"][lat.cls == "w0-zero"] == 0).all()
        out["nan_structs"] = int(nan.sum())
    if name in ("tones", "tones_dstar"):
        entry = "tone" if name == "tones" else "tone_dstar"
        ref = oracle(name, entry)
        ids = lat.extra["ids"]
        valid = ((ids >= 5) & (ids <= 122)) | ((ids >= 128) & (ids <= 163) & (name == "tones"))
        (p1, c1), (p2, c2) = ref["on"]
        loud = valid if name == "tones_dstar" else valid & (lat.extra["ad"] > 0)
        assert np.isfinite(p1).all() and np.isfinite(p2).all()
        assert (np.abs(p1).max(axis=1) > 0)[loud].all() and not p1[~valid].any(), f"{name}: the tone ids are not where the table says"
        # (a tone of a whole number of cycles per frame -- every eighth single-tone id -- leaves its phase where it was)
        assert (c1["swn"][valid] != lat.cur["swn"][valid]).mean() > 0.8 and (c1["swn"][~valid] == lat.cur["swn"][~valid]).all()
        assert (c2["swn"][valid] != c1["swn"][valid]).mean() > 0.8 and (c2["swn"][~valid] == lat.cur["swn"][~valid]).all()
        if name == "tones":
            dual = lat.cls == "dual"
            assert (c1["tonePhase"][dual] != lat.cur["tonePhase"][dual]).mean() > 0.8 and (c1["tonePhase"][~dual] == lat.cur["tonePhase"][~dual]).all()
            assert set(lat.extra["ad"].tolist()) == set(TONE_AD) and set(ids.tolist()) == set(range(256))
        for pcm, c in ref["off"]:
            assert not pcm.any() and c.tobytes() == lat.cur.tobytes(), f"{name}: tones off, and a struct or a sample changed"
        out.update(valid=int(valid.sum()))
    if name.startswith("predict"):
        ref = oracle(name, "decode_parms")
        codec = lat.extra["codec"]
        rcs = sorted(set(ref["rc"].tolist()))
        assert 0 in rcs and (codec == 3 or len(rcs) > 1), f"{name}: return codes {rcs}"
        voice = ref["rc"] == 0
        assert set(ref["cur"]["L"][voice].tolist()) >= set(range(9, 57))
        out.update(return_codes=rcs, voice=int(voice.sum()))
    return out


# ---- tones through the stream stage -----------------------------------------------------------------------------------------------
# S = 256 streams, stream s = tone id s, T = 4: the tone; the same tone again (the phases carried); a voice frame; the tone with another
# amplitude.  AMBE+2 3600x2450 carries id and amplitude in its tone frame; AMBE 3600x2400 (D-STAR) carries the id alone (its tones are
# rendered at one fixed amplitude), so its fourth frame differs from the first in the bits that are left.
TONE_STREAM_CODECS = (1, 3)
TONE_STREAMS, TONE_STREAM_FRAMES = 256, 4
FLAG_TONE = 0x10
# (form, entry of instance_cases, frames per launch, launches, what the name of the instance that runs must contain)
TONE_STREAM_FORMS = (("one-frame", "batch", 1, 4, "_one"), ("plain", "batch", 2, 2, "stream_kernel"), ("lds", "batch", 4, 1, "_lds"),
                     ("resident", "resident", 4, 1, "_res"))


@functools.lru_cache(maxsize=None)
def tone_stream_frames(codec):
    """uint8 [256, 4, 9]: clean code words"""
    import pitch_lattice

    rng = framegen.rng_for(0x30DE1000 + 32 + codec)
    ids = np.arange(TONE_STREAMS)
    frames, first = [], None
    for t in range(TONE_STREAM_FRAMES):
        if t == 2:
            bits = rng.integers(0, 2, size=(TONE_STREAMS, 49), dtype=np.uint8)
            b0 = rng.integers(0, 120, size=TONE_STREAMS)
            for j, at in enumerate(B0_BITS[codec]):
                bits[:, at] = (b0 >> (6 - j)) & 1
            if codec == 1:
                bits[:, 4] = 0   # (never the tone signature, which needs bits 0..5 set)
        elif codec == 1:
            bits = tone_bits(rng, ids, np.full(TONE_STREAMS, 100 if t < 2 else 37))
            bits[:, 0:6] = 1
            bits[:, 45:49] = 0
        else:
            bits = first.copy() if t == 1 else rng.integers(0, 2, size=(TONE_STREAMS, 49), dtype=np.uint8)
            pitch_lattice._tone_bits_2400(bits, ids)
        if t == 0:
            first = bits
        frames.append(framegen.encode_ambe3600x2450(bits))
    return np.ascontiguousarray(np.stack(frames, axis=1))


def tone_stream_seeds():
    return np.arange(TONE_STREAMS) * 3 + 11   # (the seeds of instance_cases.run_case)


@functools.lru_cache(maxsize=None)
def tone_stream_decode(codec):
    """the oracle's decode of the tone streams from the initial state: Oracle.process_batch's dict (read it, never write to it)"""
    o = oracle_lib.load()
    f = tone_stream_frames(codec)
    S, T = f.shape[:2]
    return o.process_batch(codec, S, T, f.reshape(S * T, -1), o.init_state(S), o.rng_seeded(tone_stream_seeds()))


def tone_stream_composition(codec):
    """From the oracle's flags and PCM: the ids are where the tone tables put them.  AMBE+2 3600x2450 flags every frame with the tone
    signature TONE, whatever its id, and renders ids 5..122 and 128..163; AMBE 3600x2400 renders ids 7..122 WITHOUT the flag (the
    reference's frame policy sets it only for the tone class frames it does not render: every id outside 5..122), so for that codec the
    flag is asserted where the reference sets it."""
    ref = tone_stream_decode(codec)
    S, T = TONE_STREAMS, TONE_STREAM_FRAMES
    flags = (ref["results"]["flags"].reshape(S, T) & FLAG_TONE) != 0
    ids = np.arange(S)
    assert (ref["results"]["total_errors"] == 0).all(), "tone streams: a frame with bit errors"
    assert not flags[:, 2].any(), "tone streams: a voice frame is flagged TONE"
    loud = np.abs(ref["pcmf"]).reshape(S, T, 160).max(axis=2) > 0
    if codec == 1:
        rendered = ((ids >= 5) & (ids <= 122)) | ((ids >= 128) & (ids <= 163))
        assert flags[:, (0, 1, 3)].all(), "AMBE+2: a tone frame is not flagged TONE"
    else:
        rendered = (ids >= 7) & (ids <= 122)
        assert np.array_equal(flags[:, 0], ~((ids >= 5) & (ids <= 122))) and np.array_equal(flags[:, 0], flags[:, 1]) and np.array_equal(flags[:, 0], flags[:, 3]), \
            "AMBE 3600x2400: the tone flag is not where the ids say"
    for t in (0, 1, 3):
        assert loud[rendered, t].all(), f"tone streams: frame {t} of a valid id is silent"
    if codec == 1:   # (AMBE 3600x2400 synthesises its model behind a tone-class frame it does not render)
        assert not loud[~rendered, 0].any(), "AMBE+2: a tone frame of an id that is no tone is not silent"
    st = ref["state"][:, 0]
    assert (st["swn"][rendered] != 0).mean() > 0.8, "tone streams: the tone phase is not carried"
    if codec == 1:
        dual = (ids >= 128) & (ids <= 163)
        assert (st["tonePhase"][dual] != 0).mean() > 0.8 and (st["tonePhase"][~dual] == 0).all(), "AMBE+2: the second phase accumulator is not where the dual tones are"
    return {"streams": S, "rendered": int(rendered.sum()), "flagged": int(flags[:, 0].sum())}


class ToneStreams:
    """what instance_cases.run_case takes in place of the edge mix: the tone streams of a codec"""

    state_block = 64   # (the float state is held to its bound every 64 streams: the dual tones, 36 ids, must not hide among 256)

    def __init__(self, codec):
        self.codec, self.figures = codec, None

    def frames(self, case):
        f = tone_stream_frames(self.codec)
        assert case.codec == self.codec and f.shape[:2] == (case.S, case.T * case.launches), (case, f.shape)
        return f

    def reference(self, case, frames, seeds):
        assert np.array_equal(seeds, tone_stream_seeds())
        return tone_stream_decode(self.codec)

    def assert_classes(self, codec, ref):
        tone_stream_composition(self.codec)

    def naming(self, case):
        import contextlib
        import re

        @contextlib.contextmanager
        def named():
            try:
                yield
            except AssertionError as e:
                msg = re.sub(r"stream (\d+), tick (\d+)\)", lambda m: f"stream {m.group(1)} = tone id {m.group(1)}, frame {m.group(2)})", str(e))
                raise AssertionError(f"tone streams codec {self.codec}: {msg}") from None

        return named()

    def report(self, case, ref, got):
        T = case.T * case.launches
        total, worst, at = parity.pcm_float_stats(ref["pcmf"], got["pcmf"].reshape(-1, 160))
        st, _ = parity.int16_stats(ref["pcmf"], ref["pcm16"], got["pcm16"].reshape(-1, 160), ref["peak"])
        self.figures = {"rel_rms": float(f"{total:.3e}"), "worst_frame": float(f"{worst:.3e}"), "worst_id": (at // T, f"frame {at % T}"),
                        "int16_max": st["int16_max"], "int16_within_1": round(st["int16_within_1"], 6)}
