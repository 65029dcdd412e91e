"""The bit-error history lattices: streams whose frames carry an EXACT, scripted number of bit errors, long enough for the error rate
to move, through the decisions the stream stage takes from that history -- errorRate = 0.95 prev + gain * total against 0.005, 0.0125
and the muting threshold 0.0875 (IMBE), the IMBE repeat rule c0 >= 2 && (float)total >= 10 + 40 errorRate, the adaptive threshold VM
(FLT_MAX | 45.255 E / exp(277.26 er) | 1.414 E, by er, total <= 4 and errorCount4) that forces bands voiced, and the amplitude threshold
Tm = 20480 | 6000 - 300 total + previous Tm that scales the amplitudes.

Exact counts: the decoders count the DATA bits a code word's correction changed, so `flip_data_cells` flips data cells only -- IMBE
7200x4400 the first 12 cells of rows 0..3 (Golay, 0..3 flips) and the first 11 of rows 4..6 (Hamming, 0..1); AMBE wire bits 0..11 and
24..35 (two Golay words); IMBE 7100x4400 the first 7 cells of row 0 (its shortened Golay word), the first 12 of rows 1..3, the first 11
of rows 4 and 5.  errorCount4 is the count of row 4, so a total comes with and without it.  IMBE 7100x4400 has TWO Hamming words, not
three: with c0 <= 1 its totals end at 12, and total 13 needs c0 = 2, which the repeat rule lets through only above er = 0.075 -- its 13
streams hold 12 errors for 40 frames first (no word of its encoder is out of reach; nothing is left clean for that reason).

Voice frames: IMBE pitch_lattice._imbe_bits with the voicing letters u (every voicing bit cleared), r (random), v (set) and a random
valid fundamental per frame; AMBE framegen.ambe_voice_param_bits.  Every stream has a script (`Lattice.text`, `describe`) that the
failure messages print.

Lattices (LATTICES; frames [S, T, bytes]; seeds pitch_lattice.stream_seeds):
  (0, "probe"), T = 56: e_h = 0..13 errors (c0 <= 1) for n frames, ONE probe frame with c0 = 2 | 3 and total 10..15, clean frames
    behind it.  n = 4, 12, 24, 48 and, per e_h and probe total 11, 12, 13, the two n on either side of total = 10 + 40 er.
  (0, "steady"), T = 160: every total 0..13 held with and without the row-4 error in u, r, v (two draws); decay streams (e held 8,
    24, 50, 140 frames, then clean); runs of 1..6 invalid fundamentals behind 50 frames at e = 0, 6, 13; totals 14 and 15 with c0 = 2, 3
    held (a repeat every frame, muted by the count).
  (2, "steady"), T = 160: totals 0..12 held with and without the row-4 error, 13 behind 40 frames of 12, in u, r, v (four draws).
  (1, "steady"), (3, "steady"), T = 64: every (c0, c1) in 0..3 x 0..3 held 4, 16, 40, 64 frames, then clean (four draws of the voice
    bits); a valid tone, a tone signature with an invalid id and (3600x2450) an erasure carrying 1..3 correctable errors, inside a held
    history.

`trajectory` is ONE frame-by-frame oracle decode per lattice (cached): the reference of every test of the lattice (`Workload.
reference`), and per frame and stream, from cur_mp, L, Vl, repeatCount, amplitudeThreshold, errorCountTotal, errorCount4 and the bit
patterns of errorRate, log2Ml and localEnergy -- what `check_checkpoint` holds the card to after every launch --, plus the count of bands 1..L
forced voiced (prev_mp_enhanced.Vl != prev_mp.Vl) and the enhanced amplitudes.  `composition` asserts from the oracle's decode alone
that the lattice holds what the GPU tests rely on.
Test infrastructure: imported without a GPU; nothing in the package uses it."""
import contextlib
import functools
import re
from collections import namedtuple

import numpy as np

from mbelib_neo_amd import framegen
from mbelib_neo_amd.layout import FRAME_BYTES, PARAM_BITS, PARMS_DTYPE, ROW_WIDTHS

import edge_mix
import oracle_lib
import parity
import pitch_lattice
from pitch_lattice import FLAG_MUTE, FLAG_REPEAT, MIN_SHARE_BELOW_CLIP, stream_seeds

LATTICES = [(0, "probe"), (0, "steady"), (2, "steady"), (1, "steady"), (3, "steady")]
FRAMES = {(0, "probe"): 56, (0, "steady"): 160, (2, "steady"): 160, (1, "steady"): 64, (3, "steady"): 64}
GAIN = {0: np.float32(0.000365), 2: np.float32(0.000365), 1: np.float32(0.001064), 3: np.float32(0.001064)}
THRESHOLDS = (np.float32(0.005), np.float32(0.0125), np.float32(0.0875))
PROBE_N = (4, 12, 24, 48)
MAX_FRAME_REPEATS = 4   # include/mbx_types.h
# what a checkpoint compares, all from cur_mp: integers exactly; errorRate bit for bit (a two-operation scalar recurrence: any
# difference is a wrong operation order) and so log2Ml, the prediction memory (IEEE operations in the reference's order: DESIGN.md
# section 4); localEnergy under parity.STATE_REL_RMS per block of 256 streams.  localEnergy is NOT bit for bit on the card: 0.95 pe +
# 0.05 Rm0 has the reference's order and Rm0 is summed in index order, but its terms are the squares of Ml = exp2f(log2Ml) by the
# device's exp2f, which is within an ulp of the C library's, not equal to it (`measure` counts the differences, and log2Ml's)
CHECK_INT = ("L", "Vl", "repeatCount", "amplitudeThreshold", "errorCountTotal", "errorCount4")
CHECK_BITS = ("errorRate", "log2Ml")
CHECK_BOUND = ("localEnergy",)
MEASURED = ("localEnergy", "log2Ml")
BIT_FIELDS = ("errorRate", "localEnergy", "log2Ml")   # kept by the trajectory as bit patterns

# frames, clean (the same frames without the flips) [S, T, bytes]; total, c0, c4 [S, T] as scripted; kind [S, T]: 'v' voice, 'x' an
# invalid fundamental (IMBE), AMBE: the letters of pitch_lattice._ambe_classes; letter [S] the voicing (IMBE); hist [S, 2] = (errors,
# frames) of the held history; probe [S, 3] = (frame, c0, total), -1 without one; text [S] the script in words
Lattice = namedtuple("Lattice", "codec name frames clean total c0 c4 kind letter hist probe text")


# ---- exact error counts -----------------------------------------------------------------------
def data_words(codec):
    """[(wire bit of the first data cell, data cells, most flips the word corrects)] of the protected code words of a frame"""
    off = np.concatenate([[0], np.cumsum(ROW_WIDTHS[codec])])
    if codec == 0:
        return [(int(off[r]), 12, 3) for r in range(4)] + [(int(off[r]), 11, 1) for r in range(4, 7)]
    if codec == 2:
        return [(0, 7, 3)] + [(int(off[r]), 12, 3) for r in range(1, 4)] + [(int(off[r]), 11, 1) for r in range(4, 6)]
    return [(0, 12, 3), (24, 12, 3)]


def flip_data_cells(frames, codec, counts, rng):
    """frames [n, bytes] clean wire frames; counts [n, words] flips per code word (data_words): the frames with that many DATA cells of
    each word flipped, the cells drawn from rng (the same draws whatever the counts)"""
    counts = np.asarray(counts, dtype=np.int64)
    words = data_words(codec)
    assert counts.shape == (frames.shape[0], len(words)), counts.shape
    cells = np.unpackbits(np.ascontiguousarray(frames, dtype=np.uint8), axis=1)
    for w, (at, width, most) in enumerate(words):
        assert (counts[:, w] >= 0).all() and (counts[:, w] <= most).all(), (w, most)
        rank = rng.random((frames.shape[0], width)).argsort(axis=1).argsort(axis=1)
        cells[:, at:at + width] ^= (rank < counts[:, w:w + 1]).astype(np.uint8)
    return np.packbits(cells, axis=1)


# the order in which the errors that are neither c0's nor row 4's fill the other words (one each first, then up to three per Golay word)
_FILL = {0: (1, 2, 3, 5, 6, 1, 2, 3, 1, 2, 3), 2: (1, 2, 3, 5, 1, 2, 3, 1, 2, 3)}


def rest_capacity(codec):
    return len(_FILL[codec])


def spread(codec, total, c0, c4):
    """[n, words] flips per word for frames of (total, c0, c4) errors"""
    total, c0, c4 = (np.asarray(x, dtype=np.int64) for x in (total, c0, c4))
    out = np.zeros((total.size, len(data_words(codec))), dtype=np.int64)
    out[:, 0] = c0
    if codec in (1, 3):
        assert (c4 == 0).all()
        out[:, 1] = total - c0
        return out
    out[:, 4] = c4
    rest = total - c0 - c4
    assert (rest >= 0).all() and (rest <= rest_capacity(codec)).all(), "more errors than the words of a frame correct"
    for k, w in enumerate(_FILL[codec]):
        out[:, w] += rest > k
    return out


def held(codec, e, with4):
    """(total, c0, c4) of a history frame of e errors with c0 <= 1: c0 = 1 only where the other words are full"""
    c4 = 1 if with4 else 0
    assert 0 <= e and (e >= 1 or not with4)
    c0 = 1 if e - c4 > rest_capacity(codec) else 0
    assert e - c4 - c0 <= rest_capacity(codec), (codec, e, with4)
    return e, c0, c4


def er_walk(codec, totals, er=0.0):
    """the error rate behind frames of the given totals from `er`, in float arithmetic as the reference computes it (two roundings)"""
    er = np.float32(er)
    for t in totals:
        er = np.float32(np.float32(0.95) * er) + np.float32(GAIN[codec] * np.float32(t))
    return np.float32(er)


def probe_repeats(e_h, n, total):
    """the reference's repeat rule on a probe frame (c0 >= 2) of `total` errors behind n frames of e_h"""
    er = er_walk(0, [e_h] * n + [total])
    return bool(np.float32(total) >= np.float32(10.0) + np.float32(np.float32(40.0) * er))


def probe_lengths(e_h, total):
    """the history lengths on either side of total = 10 + 40 er, where whole frames reach it inside the lattice"""
    rep = [probe_repeats(e_h, n, total) for n in range(0, 55)]
    for n in range(1, 55):
        if rep[n - 1] and not rep[n]:
            return [n - 1, n]
    return []


class _Script:
    def __init__(self, T):
        self.T, self.rows = T, []

    def add(self, letter, segments, text, hist=(0, 0), probe=(-1, -1, -1)):
        """segments: [(frames, total, c0, c4, kind)], T frames in all"""
        assert sum(s[0] for s in segments) == self.T, (text, segments)
        self.rows.append((letter, [s for s in segments if s[0] > 0], text, hist, probe))

    def arrays(self):
        S, T = len(self.rows), self.T
        total, c0, c4 = (np.zeros((S, T), dtype=np.int64) for _ in range(3))
        kind = np.full((S, T), "v", dtype="U1")
        for s, (_, segments, _, _, _) in enumerate(self.rows):
            at = 0
            for n, t, a, b, k in segments:
                total[s, at:at + n], c0[s, at:at + n], c4[s, at:at + n], kind[s, at:at + n] = t, a, b, k
                at += n
        return (total, c0, c4, kind, np.array([r[0] for r in self.rows]), np.array([r[3] for r in self.rows], dtype=np.int64),
                np.array([r[4] for r in self.rows], dtype=np.int64), [r[2] for r in self.rows])


def _hold(codec, e, with4, n, kind="v"):
    return (n,) + held(codec, e, with4) + (kind,)


def _imbe_script(codec, name):
    T = FRAMES[(codec, name)]
    sc = _Script(T)
    clean = lambda n: (n, 0, 0, 0, "v")   # noqa: E731
    if name == "probe":
        k = 0
        for e_h in range(14):
            probes = [(c0, total) for c0 in (2, 3) for total in range(10, 14 + (c0 == 3) + 1)]
            lengths = {p: list(PROBE_N) for p in probes}
            for total in (11, 12, 13):
                for c0 in (2, 3):
                    lengths[(c0, total)] = sorted(set(lengths[(c0, total)] + probe_lengths(e_h, total)))
            for (c0, total), ns in lengths.items():
                for n in ns:
                    with4 = e_h == 13 or (e_h >= 1 and k % 2 == 1)
                    p4 = 1 if total - c0 > rest_capacity(0) else total % 2
                    sc.add("urv"[k % 3], [_hold(0, e_h, with4, n), (1, total, c0, p4, "v"), clean(T - n - 1)],
                           f"{e_h} errors ({'with' if with4 else 'without'} the row-4 error) for {n} frames, probe (c0 {c0}, total {total}) at frame {n}, then clean",
                           hist=(e_h, n), probe=(n, c0, total))
                    k += 1
        return sc
    draws = 2 if codec == 0 else 4
    most = 13 if codec == 0 else 12
    for draw in range(draws):
        for e in range(most + 1):
            for with4 in (False, True):
                if (e == 0 and with4) or (e - with4 > rest_capacity(codec) + 1):
                    continue
                for letter in "urv":
                    sc.add(letter, [_hold(codec, e, with4, T)], f"{e} errors ({'with' if with4 else 'without'} the row-4 error) held, draw {draw}", hist=(e, T))
        if codec == 2:   # total 13 needs c0 = 2: behind 40 frames of 12 the repeat rule lets it through (10 + 40 er > 13)
            for letter in "urv":
                sc.add(letter, [_hold(2, 12, True, 40), (T - 40, 13, 2, 1, "v")], f"12 errors for 40 frames, then 13 (c0 2) held, draw {draw}", hist=(12, 40))
    if codec == 2:
        return sc
    k = 0
    for letter in "ur":
        for e in range(1, 14):
            for n in (8, 24, 50, 140):
                with4 = e == 13 or k % 2 == 1
                sc.add(letter, [_hold(0, e, with4, n), clean(T - n)], f"{e} errors ({'with' if with4 else 'without'} the row-4 error) for {n} frames, then clean", hist=(e, n))
                k += 1
        for e in (0, 6, 13):
            for run in range(1, 7):
                with4 = e == 13
                sc.add(letter, [_hold(0, e, with4, 50), _hold(0, e, with4, run, "x"), _hold(0, e, with4, 20), clean(T - 70 - run)],
                       f"{e} errors for 50 frames, {run} invalid fundamentals at {e} errors, 20 more frames at {e}, then clean", hist=(e, 50))
    for letter in "urv":
        for c0, total in ((2, 14), (3, 14), (3, 15)):
            sc.add(letter, [(T, total, c0, 1, "v")], f"{total} errors (c0 {c0}) held: a repeat every frame", hist=(total, T))
    return sc


CLASS_ERRORS = ((1, 0), (0, 2), (1, 2))     # (c0, c1) a class frame carries: 1..3 correctable errors
CLASS_HISTORIES = ((0, 0), (1, 1), (0, 3))
CLASS_AT = (20, 44)


def _ambe_script(codec):
    T = FRAMES[(codec, "steady")]
    sc = _Script(T)
    for draw in range(4):
        for c0 in range(4):
            for c1 in range(4):
                for n in (4, 16, 40, 64):
                    sc.add("-", [(n, c0 + c1, c0, 0, "v"), (T - n, 0, 0, 0, "v")], f"(c0 {c0}, c1 {c1}) for {n} frames, then clean, draw {draw}", hist=(c0 + c1, n))
    for cls in ("t", "i", "e") if codec == 1 else ("t", "i"):
        for h0, h1 in CLASS_HISTORIES:
            for k0, k1 in CLASS_ERRORS:
                seg, at = [], 0
                for f in CLASS_AT:
                    seg += [(f - at, h0 + h1, h0, 0, "v"), (1, k0 + k1, k0, 0, cls)]
                    at = f + 1
                seg.append((T - at, h0 + h1, h0, 0, "v"))
                sc.add("-", seg, f"(c0 {h0}, c1 {h1}) held, class '{cls}' frames with (c0 {k0}, c1 {k1}) at frames {CLASS_AT}", hist=(h0 + h1, T))
    return sc


@functools.lru_cache(maxsize=None)
def build(codec, name):
    assert (codec, name) in LATTICES, (codec, name)
    rng = framegen.rng_for(0xE4407000 + 16 * codec + (name == "probe"))
    total, c0, c4, kind, letter, hist, probe, text = (_imbe_script(codec, name) if codec in (0, 2) else _ambe_script(codec)).arrays()
    S, T = total.shape
    n, fb = S * T, FRAME_BYTES[codec]
    flat_kind = kind.reshape(-1)
    if codec in (0, 2):
        b0 = np.where(flat_kind == "x", rng.integers(208, 256, size=n), rng.integers(0, pitch_lattice.IMBE_VALID_B0, size=n)).astype(np.int64)
        which = np.where(flat_kind == "x", "r", np.repeat(letter, T))   # (the ownership table knows the valid fundamentals only)
        bits = np.zeros((n, 88), dtype=np.uint8)
        for c in "urv":
            rows = np.flatnonzero(which == c)
            bits[rows] = pitch_lattice._imbe_bits(c, b0[rows], rng)
        # the gain word b2 from the lower half of its table in three frames of four: random gains, predicted over tens of frames, put 35 % of the frames above the clip
        t = framegen._tables()
        voice = np.flatnonzero(flat_kind == "v")
        bo = t["imbe_bo"][t["imbe_L"][b0[voice]].astype(np.int64) - 9]   # [n, 79, 2]: payload bit i + 6 is bit bo[.., 1] of word bo[.., 0]
        low = (rng.random(voice.size) < 0.75)[:, None]   # (three frames in four: the others keep frames above the clip in the lattice)
        bits[voice, 6:85] &= 1 - ((bo[:, :, 0] == 2) & (bo[:, :, 1] == 5) & low).astype(np.uint8)
        if codec == 0:
            clean = framegen.encode_imbe7200x4400(bits)
        else:
            import imbe7100_frames

            clean = imbe7100_frames.encode_imbe7100x4400(bits, oracle_lib.load())
    else:
        clean = framegen.encode_ambe3600x2450(framegen.ambe_voice_param_bits(n, rng))
        for cls in "tie":
            rows = np.flatnonzero(flat_kind == cls)
            if rows.size == 0:
                continue
            if codec == 1:
                clean[rows] = edge_mix._ambe_class_frames([cls] * rows.size, rng)
            else:
                clean[rows], letters = pitch_lattice._class_frames(3, cls, rows.size, rng)
                kind.reshape(-1)[rows] = letters   # (an id outside 5..122 and 128..163 sets the silence model: 's')
    frames = flip_data_cells(clean, codec, spread(codec, total.reshape(-1), c0.reshape(-1), c4.reshape(-1)), rng)
    return Lattice(codec, name, frames.reshape(S, T, fb), clean.reshape(S, T, fb), total, c0, c4, kind, letter, hist, probe, text)


# ---- the oracle's decode, frame by frame -------------------------------------------------------
def _walk(codec, frames):
    """the oracle's decode of frames [S, T, bytes] one frame per call from the initial state: yields (t, process_batch's dict)"""
    o = oracle_lib.load()
    S, T = frames.shape[:2]
    state, rng = o.init_state(S), o.rng_seeded(stream_seeds(S))
    for t in range(T):
        ref = o.process_batch(codec, S, 1, np.ascontiguousarray(frames[:, t]), state, rng, threads=1)
        state, rng = ref["state"], ref["rng"]
        yield t, ref


def _forced(state, voice):
    """bands 1..L of each stream where prev_mp_enhanced.Vl != prev_mp.Vl (the smoothing forced them voiced); 0 where `voice` is false
    (a tone, an erasure: the two structs are not of this frame)"""
    band = np.arange(57)[None, :]
    live = (band >= 1) & (band <= state[:, 0]["L"][:, None])
    return np.where(voice, ((state[:, 2]["Vl"] != state[:, 1]["Vl"]) & live).sum(axis=1), 0)


@functools.lru_cache(maxsize=None)
def trajectory(codec, name):
    """One frame-by-frame oracle decode of the lattice.  A dict: the keys of Oracle.process_batch laid out as ONE call over [S, T] would
    leave them (records, results, pcm16, pcmf, peak stream-major, state and rng behind the last frame) -- the reference of every test
    of the lattice -- and under "at" per frame [T, S, ...]: the CHECK_INT fields of cur_mp, the bit patterns of errorRate, localEnergy and log2Ml,
    "forced" (bands forced voiced) and "Ml" (the enhanced amplitudes).  Shared: read it, never write to it."""
    lat = build(codec, name)
    S, T = lat.frames.shape[:2]
    per = {k: [] for k in ("records", "results", "pcm16", "pcmf", "peak")}
    at = {k: [] for k in CHECK_INT + BIT_FIELDS + ("forced", "Ml")}
    for t, ref in _walk(codec, lat.frames):
        for k in per:
            per[k].append(ref[k])
        cur = ref["state"][:, 0]
        for k in CHECK_INT:
            at[k].append(cur[k].astype(np.int8 if k == "Vl" else np.int32))
        for k in BIT_FIELDS:
            at[k].append(cur[k].view(np.uint32).copy())
        at["forced"].append(_forced(ref["state"], lat.kind[:, t] == "v"))
        at["Ml"].append(ref["state"][:, 2]["Ml"].copy())
    out = {k: np.ascontiguousarray(np.stack(v, axis=1)).reshape((S * T,) + v[0].shape[1:]) for k, v in per.items()}
    out["state"], out["rng"] = ref["state"], ref["rng"]
    out["at"] = {k: np.stack(v) for k, v in at.items()}
    return out


@functools.lru_cache(maxsize=None)
def clean_amplitudes(codec, name):
    """the enhanced amplitudes [T, S, 57] of the oracle's decode of the same frames without the flips"""
    return np.stack([ref["state"][:, 2]["Ml"].copy() for _, ref in _walk(codec, build(codec, name).clean)])


def one_call(codec, name):
    """the oracle's decode of the whole lattice in one call (what the trajectory, concatenated, must equal byte for byte)"""
    o = oracle_lib.load()
    f = build(codec, name).frames
    S, T = f.shape[:2]
    return o.process_batch(codec, S, T, f.reshape(S * T, -1), o.init_state(S), o.rng_seeded(stream_seeds(S)))


def er_before(codec, name, s, frame):
    """the oracle's errorRate of stream s before `frame` (behind frame - 1; 0 before the first)"""
    if frame <= 0:
        return np.float32(0.0)
    return trajectory(codec, name)["at"]["errorRate"][frame - 1, s:s + 1].view(np.float32)[0]


def describe(codec, name, s, frame=None):
    lat = build(codec, name)
    s = int(s)
    if not 0 <= s < len(lat.text):
        return ""
    out = f" = script [history {int(lat.hist[s, 0])} errors x {int(lat.hist[s, 1])} frames"
    if lat.probe[s, 0] >= 0:
        out += f"; probe (c0 {int(lat.probe[s, 1])}, total {int(lat.probe[s, 2])}) at frame {int(lat.probe[s, 0])}"
    if codec in (0, 2):
        out += f"; voicing {lat.letter[s]}"
    out += f": {lat.text[s]}]"
    if frame is not None and 0 <= int(frame) < lat.total.shape[1]:
        f = int(frame)
        out += (f", frame {f} is '{lat.kind[s, f]}' with total {int(lat.total[s, f])}, c0 {int(lat.c0[s, f])}, row 4 {int(lat.c4[s, f])}, "
                f"er before the frame {float(er_before(codec, name, s, f)):.9g}")
    return out


def _ulps(a, b):
    """distance in units of the last place between float arrays of one sign"""
    return np.abs(np.asarray(a, dtype=np.float32).view(np.int32).astype(np.int64) - np.asarray(b, dtype=np.float32).view(np.int32).astype(np.int64))


def _crossings(er, level):
    """(up, down): per stream, the frames t in 1..T-2 where er[t - 1] <= level < er[t], and where er[t - 1] > level >= er[t]"""
    above = er > level
    up = ~above[:-1] & above[1:]
    down = above[:-1] & ~above[1:]
    up[-1:], down[-1:] = False, False   # (not in the last frame)
    return up, down


@functools.lru_cache(maxsize=None)
def composition(codec, name):
    """From the oracle's decode alone (trajectory): the lattice holds what the GPU tests rely on.  Conditions, not measurements -- the
    inputs are chosen so that the reference meets them.  Returns the figures (the ulp distances are reported, not asserted)."""
    lat, ref = build(codec, name), trajectory(codec, name)
    S, T = lat.total.shape
    what = f"error lattice codec {codec} {name}"
    res = {k: ref["results"][k].reshape(S, T) for k in ref["results"].dtype.names}
    at = ref["at"]
    er = at["errorRate"].view(np.float32).T          # [S, T]
    forced = at["forced"].T

    def first(mask, why):
        bad = np.argwhere(mask)
        if bad.size:
            s, f = (int(x) for x in bad[0])
            raise AssertionError(f"{what}: {why}: {bad.shape[0]} frames, first stream {s}{describe(codec, name, s, f)}; the oracle counts total "
                                 f"{int(res['total_errors'][s, f])}, c0 {int(res['c0_errors'][s, f])}, row 4 {int(res['c4_errors'][s, f])}, flags {int(res['flags'][s, f]):#x}")

    first(res["total_errors"] != lat.total, "total_errors is not as scripted")
    first(res["c0_errors"] != lat.c0, "c0_errors is not as scripted")
    first(res["c4_errors"] != lat.c4, "c4_errors is not as scripted")
    rep = (res["flags"] & FLAG_REPEAT) != 0
    mute = (res["flags"] & FLAG_MUTE) != 0
    below = float(np.mean(ref["peak"] <= parity.CLIP_LEVEL))
    assert below >= MIN_SHARE_BELOW_CLIP, f"{what}: only {below:.3f} of the frames below the soft clip"
    out = {"streams": S, "frames": T, "below_clip": round(below, 4), "repeats": int(rep.sum()), "mutes": int(mute.sum()),
           "frames_with_forced_bands": int((forced > 0).sum())}
    gain = GAIN[codec]
    # the recurrence itself, outside repeats (a repeat takes cur_mp from prev_mp, error rate and all) and re-initialisations
    prev = np.concatenate([np.zeros((S, 1), dtype=np.float32), er[:, :-1]], axis=1)
    want = (np.float32(0.95) * prev).astype(np.float32) + (gain * lat.total.astype(np.float32)).astype(np.float32)
    plain = ~rep & ~mute & (lat.kind == "v")
    plain[:, 1:] &= ~mute[:, :-1] & (lat.kind[:, :-1] == "v")
    first(plain & (want.view(np.uint32) != er.view(np.uint32)), "errorRate is not 0.95 prev + gain * total in float arithmetic")
    out["ulps_to_thresholds"] = {f"{float(level):.4g}": int(_ulps(er[er > 0], level).min()) for level in THRESHOLDS}
    clean_so_far = (np.cumsum(lat.total + (lat.kind != "v"), axis=1) == 0)   # no error and nothing but voice up to and with this frame
    assert clean_so_far[:, -1].any() or name == "probe", f"{what}: no stream without errors"
    assert clean_so_far[:, 24].any(), f"{what}: no stream without errors in its first 25 frames"
    first((forced > 0) & clean_so_far, "a band forced voiced in a stream that had no error yet")

    if codec in (0, 2):
        is_probe = np.zeros((S, T), dtype=bool)
        has = lat.probe[:, 0] >= 0
        is_probe[np.flatnonzero(has), lat.probe[has, 0]] = True
        may = is_probe | (lat.kind == "x") | ((lat.c0 >= 2) & (lat.total >= 14))
        first(rep & ~may, "a frame repeats that is no probe frame, no invalid fundamental and not c0 >= 2 with total >= 14")
        first((lat.kind == "x") & ~rep, "an invalid fundamental is not repeated")
        first((lat.c0 >= 2) & (lat.total >= 14) & ~rep, "a frame of c0 >= 2 and total >= 14 is not repeated")
        # forced voicing: in every u and r stream that holds two errors or more for all its frames
        steady_rows = (lat.hist[:, 1] == T) & (lat.total.min(axis=1) >= 2) & (lat.c0.max(axis=1) <= 1) & np.isin(lat.letter, ("u", "r"))
        if name == "steady":
            assert steady_rows.any()
            none = steady_rows & ~(forced > 0).any(axis=1)
            assert not none.any(), f"{what}: no band forced voiced in stream {int(np.flatnonzero(none)[0])}{describe(codec, name, np.flatnonzero(none)[0])}"
        # (before the stream's first repeat: behind one, the amplitudes are predicted from another frame than in the clean decode)
        scaled = (at["Ml"] != clean_amplitudes(codec, name)).any(axis=2).T & (np.cumsum(rep, axis=1) == 0)
        assert scaled.any(), f"{what}: no frame whose amplitudes the threshold scales"
        out["frames_with_scaled_amplitudes"] = int(scaled.sum())
        out["forced_frames_per_stream"] = (int((forced > 0).sum(axis=1).min()), int((forced > 0).sum(axis=1).max()))
    if (codec, name) == (0, "probe"):
        p = np.flatnonzero(has)
        f, total, outcome = lat.probe[p, 0], lat.probe[p, 2], rep[p, lat.probe[p, 0]]
        assert not outcome[total == 10].any(), f"{what}: a probe frame of total 10 repeats"
        assert outcome[total >= 14].all(), f"{what}: a probe frame of total 14 or 15 does not repeat"
        for k in (11, 12, 13):
            assert outcome[total == k].any() and not outcome[total == k].all(), f"{what}: probe total {k} is seen with one outcome only"
        out["probe_outcomes"] = {int(k): (int((~outcome[total == k]).sum()), int(outcome[total == k].sum())) for k in range(10, 16)}
        # (float)total against 10 + 40 er, er as the probe frame itself computes it
        er_p = (np.float32(0.95) * prev[p, f]).astype(np.float32) + (gain * total.astype(np.float32)).astype(np.float32)
        level = np.float32(10.0) + (np.float32(40.0) * er_p).astype(np.float32)
        assert np.array_equal(outcome, total.astype(np.float32) >= level), f"{what}: a probe frame's outcome is not the repeat rule's"
        out["ulps_total_to_repeat_level"] = int(_ulps(total.astype(np.float32), level).min())
    if (codec, name) == (0, "steady"):
        for level in THRESHOLDS:
            up, down = _crossings(er.T, level)
            assert up.any() and down.any(), f"{what}: {float(level)} is crossed upward {int(up.sum())} and downward {int(down.sum())} times inside a stream"
        twelve = np.flatnonzero((lat.hist[:, 0] == 12) & (lat.hist[:, 1] == T))
        crossed = np.argmax(er[twelve] > THRESHOLDS[2], axis=1)
        assert (er[twelve] > THRESHOLDS[2]).any(axis=1).all() and (crossed > 100).all(), f"{what}: 12 errors a frame cross 0.0875 at frames {crossed}"
        out["twelve_crosses_at"] = int(crossed.min())
        assert (mute & (at["repeatCount"].T == 0)).any(), f"{what}: no frame muted by the error rate alone (repeatCount 0)"
        assert (mute & (at["repeatCount"].T >= MAX_FRAME_REPEATS) & (er <= THRESHOLDS[2])).any(), f"{what}: no frame muted by the repeat count alone"
        tm = at["amplitudeThreshold"].T
        assert (tm > 100000).any(), f"{what}: amplitudeThreshold never grows past 100,000 (largest {int(tm.max())})"
        back = ((tm[:, :-1] > 20480) & (tm[:, 1:] == 20480)).any()
        assert back, f"{what}: amplitudeThreshold never returns to 20480"
        e4 = at["errorCount4"].T != 0
        assert (e4 & (er <= THRESHOLDS[1]) & ~rep).any() and (e4 & (er > THRESHOLDS[1]) & ~rep).any(), f"{what}: errorCount4 != 0 on one side of 0.0125 only"
        out.update(amplitude_threshold_max=int(tm.max()), muted_by_rate_alone=int((mute & (at["repeatCount"].T == 0)).sum()))
    if (codec, name) == (2, "steady"):
        for level in THRESHOLDS:
            up, _ = _crossings(er.T, level)
            assert up.any(), f"{what}: {float(level)} is never crossed upward inside a stream"
        assert (lat.total == 13).any() and mute.any()
    if codec in (1, 3):
        bits = oracle_lib.records_to_bits(ref["records"], PARAM_BITS[codec])
        cls = pitch_lattice._ambe_classes(codec, bits, ref["results"]["flags"]).reshape(S, T)
        first((lat.kind != "v") & (cls != lat.kind), "a class frame is not of the class it was scripted as")
        c1 = lat.total - lat.c0
        rule = ((lat.c0 >= 2) & (lat.total >= 6)) if codec == 1 else (lat.total > 3)
        first((lat.kind == "v") & (rep != rule), "a voice frame's repeat is not the reference's rule on the scripted counts")
        assert (c1 <= 3).all() and rep.any() and mute.any() and (mute[:, :-1]).any(), f"{what}: repeats, mutes, a frame behind a mute"
        for level in THRESHOLDS[:2]:
            up, down = _crossings(er.T, level)
            assert up.any() and down.any(), f"{what}: {float(level)} is crossed upward {int(up.sum())} and downward {int(down.sum())} times inside a stream"
        assert (forced > 0).any(), f"{what}: no band forced voiced"
        tm = at["amplitudeThreshold"].T
        assert (tm > 20480).any() and ((tm[:, :-1] > 20480) & (tm[:, 1:] == 20480)).any(), f"{what}: amplitudeThreshold never grows, or never returns"
        for c in sorted(set(lat.kind.reshape(-1).tolist()) - {"v"}):
            behind = (lat.kind[:, :-1] == c) & (cls[:, 1:] == "v")
            assert behind.any(), f"{what}: no voice frame decoded behind a class '{c}' frame"
            out[f"class_{c}"] = int((lat.kind == c).sum())
        out["amplitude_threshold_max"] = int(tm.max())
    return out


# ---- the per-launch checkpoint ----------------------------------------------------------------
def cur_at(codec, name, frame):
    """cur_mp [S] behind `frame` in the oracle's decode, the checked fields only (the others zero)"""
    at = trajectory(codec, name)["at"]
    cur = np.zeros(at["L"].shape[1], dtype=PARMS_DTYPE)
    for k in CHECK_INT:
        cur[k] = at[k][frame]
    for k in BIT_FIELDS:
        cur[k] = at[k][frame].view(np.float32)
    return cur


def check_checkpoint(codec, name, frame, cur, what="checkpoint"):
    """cur: cur_mp [S] (PARMS_DTYPE) as a launch left it behind `frame`: the decision state is the oracle's -- L, Vl, repeatCount,
    amplitudeThreshold, errorCountTotal, errorCount4 exactly, errorRate and log2Ml bit for bit, localEnergy under parity's bound for
    float state block by block of 256 streams.  The failure names the first stream's script, the frame and the error rate before it."""
    at = trajectory(codec, name)["at"]
    for k in CHECK_BOUND:
        ref, got = at[k][frame].view(np.float32), np.ascontiguousarray(cur[k])
        for a in range(0, ref.size, Workload.state_block):
            r = parity.rel_rms(ref[a:a + Workload.state_block], got[a:a + Workload.state_block])
            if not r <= parity.STATE_REL_RMS:
                s = a + int(np.argmax(np.abs(ref[a:a + Workload.state_block].astype(np.float64) - got[a:a + Workload.state_block])))
                raise AssertionError(f"{what}: behind frame {frame}: {k} of cur_mp: relative RMS {r:.3e} > {parity.STATE_REL_RMS:.1e} over streams {a}.."
                                     f"{min(a + Workload.state_block, ref.size) - 1}, worst stream {s}: ref={float(ref[s]):.9g} got={float(got[s]):.9g}"
                                     f"{describe(codec, name, s, frame)}")
    for k in CHECK_INT + CHECK_BITS:
        ref = at[k][frame]
        got = cur[k].view(np.uint32) if k in CHECK_BITS else cur[k].astype(ref.dtype)
        if np.array_equal(ref, got):
            continue
        bad = ref != got
        rows = np.flatnonzero(bad.reshape(bad.shape[0], -1).any(axis=1))
        s = int(rows[0])
        if k in CHECK_BITS:
            at_s = (s,) + ((int(np.flatnonzero(bad[s])[0]),) if bad.ndim == 2 else ())
            r, g = ref[at_s], got[at_s]
            detail = ((f"band {at_s[1]}: " if bad.ndim == 2 else "") + f"ref={float(r.view(np.float32)):.9g} ({int(r):#010x}) got={float(g.view(np.float32)):.9g} ({int(g):#010x}), "
                      f"{int(r) - int(g):+d} ulp")
        elif k == "Vl":
            band = int(np.flatnonzero(bad[s])[0])
            detail = f"band {band}: ref={int(ref[s, band])} got={int(got[s, band])}"
        else:
            detail = f"ref={int(ref[s])} got={int(got[s])}"
        raise AssertionError(f"{what}: behind frame {frame}: {k} of cur_mp differs in {rows.size} streams, first stream {s}: {detail}{describe(codec, name, s, frame)}")


def measure(codec, name, frame, cur, into):
    """figures, not assertions: how far localEnergy and log2Ml of cur_mp behind `frame` are from the oracle's bit patterns -- into[field]
    = [checkpoints x streams that differ, largest distance in ulps, largest relative difference, the first (stream, frame)]"""
    at = trajectory(codec, name)["at"]
    for k in MEASURED:
        ref, got = at[k][frame], np.ascontiguousarray(cur[k]).view(np.uint32)
        bad = (ref != got).reshape(ref.shape[0], -1).any(axis=1)
        fig = into.setdefault(k, [0, 0, 0.0, None])
        if bad.any():
            rf, gf = ref.view(np.float32).astype(np.float64), got.view(np.float32).astype(np.float64)
            with np.errstate(divide="ignore", invalid="ignore"):
                rel = np.nanmax(np.where(rf != 0, np.abs(rf - gf) / np.abs(rf), 0.0))
            ulp = int(np.abs(ref.astype(np.int64) - got.astype(np.int64)).max())
            fig[:] = [fig[0] + int(bad.sum()), max(fig[1], ulp), max(fig[2], float(f"{rel:.3e}")), fig[3] or (int(np.flatnonzero(bad)[0]), int(frame))]


@contextlib.contextmanager
def named(codec, name, T):
    """an AssertionError of tests/parity.py that names a stream is raised again with the stream's script behind it; a comparison of
    frames (records, results, PCM) also says what the frame carries and the error rate before it (pitch_lattice.named, for scripts)"""
    try:
        yield
    except AssertionError as e:
        msg = str(e)
        final = re.search(r": (rng|state)\b", msg) is not None
        msg = re.sub(r"stream (\d+), tick (\d+)\)", lambda m: m.group(0)[:-1] + describe(codec, name, m.group(1), None if final else m.group(2)) + ")", msg)
        block = re.search(r"streams (\d+)\.\.(\d+); indices within the block", msg)
        first = re.search(r"first at \((?:np\.\w+\()?(\d+)", msg)
        if first:
            s = int(first.group(1)) + (int(block.group(1)) if block else 0)
            msg += f" -- stream {s}{describe(codec, name, s)}"
        elif block:
            msg += f" -- streams {block.group(1)}{describe(codec, name, block.group(1))} to {block.group(2)}{describe(codec, name, block.group(2))}"
        raise AssertionError(f"codec {codec} error lattice {name}, T = {T}: {msg}") from None


class Workload:
    """what instance_cases.run_case takes in place of the edge mix: the lattice (codec, name), its trajectory as the reference, and a
    checkpoint behind every launch"""

    state_block = 256

    def __init__(self, codec, name):
        self.codec, self.name, self.figures, self.checkpoints, self.failed, self.measured = codec, name, None, 0, None, {}

    def frames(self, case):
        f = build(self.codec, self.name).frames
        assert case.codec == self.codec and f.shape[:2] == (case.S, case.T * case.launches), (case, f.shape)
        return f

    def reference(self, case, frames, seeds):
        assert np.array_equal(seeds, stream_seeds(case.S))
        return trajectory(self.codec, self.name)

    def assert_classes(self, codec, ref):
        composition(self.codec, self.name)

    def naming(self, case):
        return named(self.codec, self.name, case.T * case.launches)

    def checkpoint(self, case, launch, state):
        """run_case's hook: state [S, 3] of the case's slots behind launch `launch`.  The FIRST mismatch is kept (self.failed) and the
        launches go on, so that the run's figures are whole when the test raises it"""
        self.checkpoints += 1
        measure(self.codec, self.name, (launch + 1) * case.T - 1, state[:, 0], self.measured)
        if self.failed is None:
            try:
                check_checkpoint(self.codec, self.name, (launch + 1) * case.T - 1, state[:, 0], what=f"{case.id}: launch {launch}")
            except AssertionError as e:
                self.failed = str(e)

    def report(self, case, ref, got):
        """the figures of the run for the record, before anything is asserted (self.figures; the test prints them)"""
        T = case.T * case.launches
        total, worst, at = parity.pcm_float_stats(ref["pcmf"], got["pcmf"].reshape(-1, 160))
        st, _ = parity.int16_stats(ref["pcmf"], ref["pcm16"], got["pcm16"].reshape(-1, 160), ref["peak"])
        d = np.abs(ref["pcm16"].astype(np.int32) - got["pcm16"].reshape(-1, 160).astype(np.int32)).max(axis=1)
        k = int(np.argmax(d - parity.int16_bound(ref["peak"])))   # the frame nearest to (or furthest over) its int16 bound
        lat = build(self.codec, self.name)
        self.figures = {"rel_rms": float(f"{total:.3e}"), "worst_frame": float(f"{worst:.3e}"),
                        "worst_script": (at // T, f"frame {at % T}", lat.text[at // T]),
                        "int16_max_below_clip": st["int16_max_below_clip"], "int16_max_inside_clip": st["int16_max_inside_clip"],
                        "int16_margin": st["int16_margin"], "margin_script": (k // T, f"frame {k % T}", f"{int(d[k])} LSB", lat.text[k // T]),
                        "int16_within_1": round(st["int16_within_1"], 6), "checkpoints": self.checkpoints,
                        "bits_differ [count, ulps, relative, first (stream, frame)]": self.measured}


# ---- the launch forms (tests/test_gpu_error_lattice.py) ----------------------------------------
# (form, entry of instance_cases, frames per launch or None = all of them, the instance that must run by codec; a codec without one: n/a)
FORMS = [
    ("one-batch", "batch", 1, {0: "imbe_one_launch_kernel", 2: "imbe7100_stream_kernel_one_fused", 1: "ambe_one_launch_kernel", 3: "ambe2400_one_launch_kernel"}),
    ("one-resident", "resident", 1, {0: "imbe_one_launch_kernel_res", 2: "imbe7100_stream_kernel_res1_fused", 1: "ambe_one_launch_kernel_res",
                                     3: "ambe2400_one_launch_kernel_res"}),
    ("one-staged", "staged", 1, {0: "imbe_stream_kernel_one", 3: "ambe2400_stream_kernel_one"}),
    ("one-ws", "batch_ws", 1, {0: "imbe_stream_kernel_one_fused", 1: "ambe_stream_kernel_one"}),
    ("two", "batch", 2, {0: "imbe_stream_kernel", 2: "imbe_stream_kernel", 1: "ambe_stream_kernel", 3: "ambe2400_stream_kernel"}),
    ("lds-whole", "batch", None, {0: "imbe_stream_kernel_lds", 1: "ambe_stream_kernel_lds", 3: "ambe2400_stream_kernel_lds"}),
    ("lds-32", "batch", 32, {0: "imbe_stream_kernel_lds"}),
    ("lds-eight", "batch", 8, {0: "imbe_stream_kernel_lds", 1: "ambe_stream_kernel_lds", 3: "ambe2400_stream_kernel_lds"}),
    ("resident-eight", "resident", 8, {0: "imbe_stream_kernel_res", 1: "ambe_stream_kernel_res", 3: "ambe2400_stream_kernel_res"}),
]
# the 160-frame lattices run in these forms only (7100x4400 has no LDS-parked form: the plain looped instance stands in for it)
LONG_FORMS = {0: ("one-batch", "one-resident", "lds-whole", "lds-32", "resident-eight"), 2: ("one-batch", "one-resident", "two")}


def build_size(codec, name):
    """streams of a lattice (the script alone: no frame is generated)"""
    sc = _imbe_script(codec, name) if codec in (0, 2) else _ambe_script(codec)
    return len(sc.rows)


def cases():
    """[(instance_cases.Case, Workload)]: lattice by lattice, so that the tests of one lattice follow each other"""
    import instance_cases

    out = []
    for codec, name in LATTICES:
        S, T = build_size(codec, name), FRAMES[(codec, name)]
        for form, entry, per, names in FORMS:
            if codec not in names or (T == 160 and form not in LONG_FORMS[codec]) or (form == "lds-32" and T != 160):
                continue
            per = T if per is None else per
            assert T % per == 0
            out.append((instance_cases.Case(f"{form}-codec{codec}-{name}", names[codec], codec, S, per, T // per, entry, {}), Workload(codec, name)))
    return out
