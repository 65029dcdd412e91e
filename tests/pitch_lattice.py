"""The pitch-pair lattice: every (previous, current) fundamental through the stream stage, two frames per stream.

The voiced bank of the synthesiser takes one of several forms -- the interpolated branch for harmonics 1..7 when |w0 - w0_prev| <
0.1 w0, the flat form at equal fundamentals, the windowed oscillators with their drift term, max(L, L_prev) with the shorter model
padded, the unvoiced FFT skipped when no band is unvoiced -- and which one is a function of the PAIR (b0_prev, b0_cur) and of the
two voicing patterns.  A lattice is frames[S, 2, bytes] with stream s = p * N + c: frame 0 carries b0 = p, frame 1 carries b0 = c, all
clean code words, every other bit random (generator framegen.rng_for, one fixed tag per codec and pattern).

  IMBE 7200x4400 (codec 0): b0 in bits 0..5, 85, 86; the voicing bits, placed through the imbe_bo ownership table, follow a pattern
    of two letters, one per frame: v every voicing bit set, u every one cleared, r random.  vv, uu, vu, uv: N = 208; rr: N = 256,
    with the invalid fundamentals 208..255 on either side (a repeat, whatever the state).
  IMBE 7100x4400 (codec 2): rr, N = 256, encoded by tests/imbe7100_frames.py.
  AMBE+2 3600x2450 (codec 1), AMBE 3600x2400 (codec 3): N = 128, b0 in bits {0,1,2,3,37,38,39} / {0,1,2,3,4,5,48}, one pattern (rr).
    Behind the N * N streams a class rim: for every voice b0 0..119 one stream with each class frame directly before it and one with
    it directly behind it -- a valid tone, a tone signature with an invalid id, an erasure (codec 1 only: edge_mix._ambe_class_frames),
    b0 = 124 and b0 = 125 (the two silence fundamentals of 3600x2450; plain voice in 3600x2400, whose silence model is set by tone
    frames with an id outside 5..122 and 128..163, so its invalid ids are scripted on both sides of that).  The random voicing indices bring an
    all-voiced and an all-unvoiced frame at every L on either side (`composition` asserts it), so none is scripted.

`quad` repeats the two frames as (p, c, p, c), T = 4, for the looped instances that keep state in LDS or resident: it also brings
c -> p on state the launch made itself.  `composition` asserts from the ORACLE's decode what the GPU tests rely on; `Workload` is
what tests/instance_cases.run_case takes (frames, the oracle decode -- made once per lattice and shared --, the class assertion, and
failure messages that name the pair).
Test infrastructure: imported without a GPU; nothing in the package uses it."""
import contextlib
import functools
import re
from collections import namedtuple

import numpy as np

from mbelib_neo_amd import framegen
from mbelib_neo_amd.layout import FRAME_BYTES, PARAM_BITS

import edge_mix
import oracle_lib
import parity

FLAG_TONE, FLAG_ERASURE, FLAG_REPEAT, FLAG_MUTE = 0x10, 0x20, 0x40, 0x80
PATTERNS = {0: ("vv", "uu", "rr", "vu", "uv"), 1: ("rr",), 2: ("rr",), 3: ("rr",)}
LATTICES = [(codec, pattern) for codec in (0, 2, 1, 3) for pattern in PATTERNS[codec]]
B0_BITS = {0: (0, 1, 2, 3, 4, 5, 85, 86), 2: (0, 1, 2, 3, 4, 5, 85, 86), 1: (0, 1, 2, 3, 37, 38, 39), 3: (0, 1, 2, 3, 4, 5, 48)}
IMBE_VALID_B0 = 208
AMBE_VOICE_B0 = 120
RIM_CLASSES = {1: ("t", "i", "e", "124", "125"), 3: ("t", "i", "124", "125")}
MIN_SHARE_BELOW_CLIP = 0.70
# tone ids of AMBE 3600x2400 that are no tone (5, 6 and the dual tones 128..163 leave the model alone; the others set the silence model)
INVALID_TONE_IDS_2400 = (0, 3, 5, 6, 123, 127, 130, 161, 164, 200, 255)

# frames [S, 2, bytes]; bits [S, 2, 88] (IMBE); b0 [S, 2] as scripted (-1: a tone or erasure frame of the rim); cls [S, 2] (AMBE): the class
# each frame of the rim was scripted as, in the letters of _ambe_classes, '?' in the N x N part (whatever its random bits make it)
Lattice = namedtuple("Lattice", "codec pattern N frames bits b0 cls")


def stream_seeds(S):
    """the RNG seeds of instance_cases.run_case"""
    return np.arange(S) * 3 + 11


def size(codec, pattern):
    if codec in (0, 2):
        return 256 if pattern == "rr" else IMBE_VALID_B0
    return 128


def _set_b0(codec, bits, b0):
    pos = B0_BITS[codec]
    for k, at in enumerate(pos):
        bits[:, at] = (b0 >> (len(pos) - 1 - k)) & 1


def _get_bits(bits, pos):
    v = np.zeros(bits.shape[0], dtype=np.int64)
    for at in pos:
        v = (v << 1) | bits[:, at].astype(np.int64)
    return v


def _imbe_bits(letter, b0, rng):
    bits = rng.integers(0, 2, size=(b0.size, 88), dtype=np.uint8)
    _set_b0(0, bits, b0)
    if letter != "r":
        t = framegen._tables()
        assert (b0 < IMBE_VALID_B0).all(), "the ownership table knows the valid fundamentals only"
        own = (t["imbe_bo"][t["imbe_L"][b0].astype(np.int64) - 9, :, 0] == 1).astype(np.uint8)   # [n, 79]: payload bit i + 6 feeds the voicing word
        bits[:, 6:85] = (bits[:, 6:85] | own) if letter == "v" else (bits[:, 6:85] & (1 - own))
    return bits


def _tone_bits_2400(bits, ids):
    """AMBE 3600x2400 tone-class frames (b0 = 126 | 127) of the given ids: three bits select the id's top three, five carry the rest"""
    select = {0: 1, 1: 2, 2: 3, 3: 4, 4: 0, 5: 7, 6: 6, 7: 5}   # id >> 5 -> the value of bits 6, 7, 8
    bits[:, 0:6] = 1
    for k, tone in enumerate(ids):
        sel = select[int(tone) >> 5]
        bits[k, 6:9] = [(sel >> 2) & 1, (sel >> 1) & 1, sel & 1]
        for at, j in zip((9, 42, 43, 10, 11), range(4, -1, -1)):
            bits[k, at] = (int(tone) >> j) & 1


def _class_frames(codec, cls, n, rng):
    """n clean wire frames of one rim class, and the class the decoder must see in each (the letters of _ambe_classes)"""
    if cls in ("124", "125"):
        bits = rng.integers(0, 2, size=(n, 49), dtype=np.uint8)
        _set_b0(codec, bits, np.full(n, int(cls), dtype=np.int64))
        if codec == 1:
            bits[:, 4] = 0   # (never the tone signature, which needs bits 0..5 set)
        return framegen.encode_ambe3600x2450(bits), np.full(n, "s" if codec == 1 else "v")
    if codec == 1:
        return edge_mix._ambe_class_frames([cls] * n, rng), np.full(n, cls)
    bits = rng.integers(0, 2, size=(n, 49), dtype=np.uint8)
    ids = rng.integers(7, 123, size=n) if cls == "t" else np.resize(np.array(INVALID_TONE_IDS_2400), n)
    _tone_bits_2400(bits, ids)
    leaves_model = ((ids >= 5) & (ids <= 122)) | ((ids >= 128) & (ids <= 163))
    return framegen.encode_ambe3600x2450(bits), np.where(cls == "t", "t", np.where(leaves_model, "i", "s"))


@functools.lru_cache(maxsize=None)
def build(codec, pattern):
    """the lattice of (codec, pattern): a Lattice of frames [S, 2, 18 | 9] uint8"""
    assert pattern in PATTERNS[codec], (codec, pattern)
    N = size(codec, pattern)
    rng = framegen.rng_for(0x917C0000 + 16 * codec + PATTERNS[codec].index(pattern))
    s = np.arange(N * N)
    b0 = np.stack([s // N, s % N], axis=1).astype(np.int64)
    nbits, fb = PARAM_BITS[codec], FRAME_BYTES[codec]
    if codec in (0, 2):
        bits = np.stack([_imbe_bits(pattern[f], b0[:, f], rng) for f in range(2)], axis=1)
        flat = bits.reshape(-1, nbits)
        if codec == 0:
            frames = framegen.encode_imbe7200x4400(flat)
        else:
            import imbe7100_frames

            frames = imbe7100_frames.encode_imbe7100x4400(flat, oracle_lib.load())
        return Lattice(codec, pattern, N, frames.reshape(-1, 2, fb), bits, b0, None)
    bits = rng.integers(0, 2, size=(N * N, 2, nbits), dtype=np.uint8)
    for f in range(2):
        _set_b0(codec, bits[:, f], b0[:, f])
    frames = framegen.encode_ambe3600x2450(bits.reshape(-1, nbits)).reshape(-1, 2, fb)
    # the class rim: (class, voice b0) and (voice b0, class) for every voice b0 and every class
    voice = np.arange(AMBE_VOICE_B0, dtype=np.int64)
    rim_frames, rim_b0, rim_cls = [], [], [np.full((N * N, 2), "?")]
    for cls in RIM_CLASSES[codec]:
        vbits = rng.integers(0, 2, size=(2 * AMBE_VOICE_B0, nbits), dtype=np.uint8)
        _set_b0(codec, vbits, np.concatenate([voice, voice]))
        v = framegen.encode_ambe3600x2450(vbits).reshape(2, AMBE_VOICE_B0, fb)
        k, letters = _class_frames(codec, cls, 2 * AMBE_VOICE_B0, rng)
        k, letters, v_letter = k.reshape(2, AMBE_VOICE_B0, fb), letters.reshape(2, AMBE_VOICE_B0), np.full(AMBE_VOICE_B0, "v")
        marker = np.full(AMBE_VOICE_B0, int(cls) if cls.isdigit() else -1, dtype=np.int64)
        rim_frames += [np.stack([k[0], v[0]], axis=1), np.stack([v[1], k[1]], axis=1)]
        rim_b0 += [np.stack([marker, voice], axis=1), np.stack([voice, marker], axis=1)]
        rim_cls += [np.stack([letters[0], v_letter], axis=1), np.stack([v_letter, letters[1]], axis=1)]
    return Lattice(codec, pattern, N, np.concatenate([frames] + rim_frames), None, np.concatenate([b0] + rim_b0), np.concatenate(rim_cls))


def frames(codec, pattern, variant="pair"):
    """uint8 [S, 2, bytes] ('pair') or the same two frames twice, [S, 4, bytes] ('quad')"""
    f = build(codec, pattern).frames
    assert variant in ("pair", "quad"), variant
    return f if variant == "pair" else np.ascontiguousarray(np.concatenate([f, f], axis=1))


def decode(codec, pattern, variant="pair"):
    """the oracle's decode of a lattice from the initial state, seeds stream_seeds(S): Oracle.process_batch's dict.  Shared by every
    test of the lattice (the last two decodes are kept: a lattice's pair and its quad): read it, never write to it."""
    return _decode(codec, pattern, variant)


@functools.lru_cache(maxsize=2)
def _decode(codec, pattern, variant):
    o = oracle_lib.load()
    f = frames(codec, pattern, variant)
    S, T = f.shape[:2]
    return o.process_batch(codec, S, T, f.reshape(S * T, -1), o.init_state(S), o.rng_seeded(stream_seeds(S)))


@functools.lru_cache(maxsize=None)
def first_state(codec, pattern):
    """the oracle's state [S, 3] behind frame 0 alone (the decode of the pair leaves only what is behind frame 1)"""
    o = oracle_lib.load()
    f = np.ascontiguousarray(build(codec, pattern).frames[:, 0])
    S = f.shape[0]
    return o.process_batch(codec, S, 1, f, o.init_state(S), o.rng_seeded(stream_seeds(S)))["state"]


def _voicing(cur):
    """(all bands 1..L voiced, all unvoiced) per stream of a cur_mp array"""
    band = np.arange(cur["Vl"].shape[1])[None, :]
    live = (band >= 1) & (band <= cur["L"][:, None])
    return ((cur["Vl"] == 1) | ~live).all(axis=1), ((cur["Vl"] == 0) | ~live).all(axis=1)


def _ambe_classes(codec, bits, flags):
    """per frame, from the oracle's corrected parameter bits and result flags: 'v' voice, 'r' repeat, 't' tone with a valid id, 'i' tone
    class with an invalid id, 'e' erasure, 's' a frame that sets the silence model"""
    b0 = _get_bits(bits, B0_BITS[codec])
    out = np.full(b0.shape, "v", dtype="U1")
    if codec == 1:
        tone_id = _get_bits(bits, range(12, 20))
        valid = ((tone_id >= 5) & (tone_id <= 122)) | ((tone_id >= 128) & (tone_id <= 163))
        tone = (flags & FLAG_TONE) != 0
        out[(b0 == 124) | (b0 == 125)] = "s"
        out[(flags & FLAG_ERASURE) != 0] = "e"
        out[tone & valid] = "t"
        out[tone & ~valid] = "i"
    else:
        sel = _get_bits(bits, (6, 7, 8))
        top = np.array([4, 0, 1, 2, 3, 7, 6, 5])[sel]   # bits 7, 6, 5 of the id
        tone_id = (top << 5) | _get_bits(bits, (9, 42, 43, 10, 11))
        tone = (b0 & 0x7E) == 0x7E
        valid = (tone_id >= 7) & (tone_id <= 122)
        leaves_model = ((tone_id >= 5) & (tone_id <= 122)) | ((tone_id >= 128) & (tone_id <= 163))
        out[tone & valid] = "t"
        out[tone & ~valid & leaves_model] = "i"
        out[tone & ~leaves_model] = "s"
        assert np.array_equal(tone & ~((tone_id >= 5) & (tone_id <= 122)), (flags & FLAG_TONE) != 0), "AMBE 3600x2400: the tone flag is not where the ids say"
    out[(flags & FLAG_REPEAT) != 0] = "r"
    return out


def composition(codec, pattern, ref):
    """From the oracle's decode of the pair lattice (decode(codec, pattern)): the lattice holds what the GPU tests rely on.  Conditions,
    not measurements -- the inputs are chosen so that the oracle alone meets them.  Returns the figures."""
    lat = build(codec, pattern)
    S = lat.frames.shape[0]
    assert ref["results"].shape[0] == 2 * S, "composition reads the decode of the pair lattice"
    flags = ref["results"]["flags"].reshape(S, 2)
    errors = ref["results"]["total_errors"].reshape(S, 2)
    bits = oracle_lib.records_to_bits(ref["records"], PARAM_BITS[codec]).reshape(S, 2, -1)
    st = (first_state(codec, pattern)[:, 0], ref["state"][:, 0])   # cur_mp behind frame 0, behind frame 1
    L0, L1 = st[0]["L"].astype(np.int64), st[1]["L"].astype(np.int64)
    what = f"lattice codec {codec} {pattern}"
    assert (errors == 0).all(), f"{what}: a frame with bit errors (every frame is a clean code word)"
    rep = (flags & FLAG_REPEAT) != 0
    below = float(np.mean(ref["peak"] <= parity.CLIP_LEVEL))
    assert below >= MIN_SHARE_BELOW_CLIP, f"{what}: only {below:.3f} of the frames below the soft clip"
    out = {"streams": S, "below_clip": round(below, 4), "repeats": int(rep.sum())}
    scripted = lat.b0[:lat.N * lat.N]
    for f in range(2):
        got = _get_bits(bits[:lat.N * lat.N, f], B0_BITS[codec])
        assert np.array_equal(got, scripted[:, f]), f"{what}: frame {f} does not decode to the b0 it was made of"

    if codec in (0, 2):
        assert np.array_equal(bits, lat.bits.astype(bits.dtype)), f"{what}: a frame does not decode to the bits it was made of"
        assert not (flags & FLAG_MUTE).any(), f"{what}: a muted frame"
        ok = lat.b0 < IMBE_VALID_B0
        both = ok.all(axis=1)
        assert not rep[ok].any(), f"{what}: a frame of a valid fundamental is repeated"
        pairs = np.zeros((57, 57), dtype=bool)
        pairs[L0[both], L1[both]] = True
        assert pairs[9:57, 9:57].all() and pairs.sum() == 48 * 48, f"{what}: (L_prev, L_cur) pairs missing: {np.argwhere(~pairs[9:57, 9:57])[:8] + 9}"
        pw0, cw0 = st[0]["w0"][both], st[1]["w0"][both]
        stable = np.abs(cw0 - pw0) < np.float32(0.1) * cw0   # (float, as the reference's synthesiser decides it)
        assert stable.dtype == bool and pw0.dtype == np.float32
        assert stable.any() and (~stable).any() and (pw0 == cw0).any(), f"{what}: the stability test is met on one side only"
        out.update(L_pairs=int(pairs.sum()), stable=int(stable.sum()), unstable=int((~stable).sum()), equal_w0=int((pw0 == cw0).sum()))
        for f, letter in enumerate(pattern):
            voiced, unvoiced = _voicing(st[f][both])
            assert letter != "v" or voiced.all(), f"{what}: frame {f} has an unvoiced band"
            assert letter != "u" or unvoiced.all(), f"{what}: frame {f} has a voiced band"
        if lat.N > IMBE_VALID_B0:
            assert rep[~ok].all(), f"{what}: a frame of an invalid fundamental is not repeated"
            valid = set(range(IMBE_VALID_B0))
            behind = set(lat.b0[~ok[:, 0] & ok[:, 1] & ~rep[:, 1], 1].tolist())
            before = set(lat.b0[ok[:, 0] & ~ok[:, 1] & ~rep[:, 0], 0].tolist())
            assert behind == valid and before == valid, f"{what}: a valid b0 never meets a repeat"
            out.update(invalid_frames=int((~ok).sum()))
        return out

    cls = _ambe_classes(codec, bits.reshape(2 * S, -1), flags.reshape(-1)).reshape(S, 2)
    rim = lat.cls != "?"
    wrong = np.argwhere(rim & (cls != lat.cls))
    if wrong.size:
        at = tuple(wrong[0])
        raise AssertionError(f"{what}: {wrong.shape[0]} frames of the rim are not of the class they were scripted as, first stream {at[0]} "
                             f"frame {at[1]}: scripted '{lat.cls[at]}', the oracle decodes '{cls[at]}'")
    out["rim_frames"] = int(rim.sum())
    voice = cls == "v"
    decoded = voice[:, 1]
    every_L = set(range(9, 57))
    assert set(L1[decoded].tolist()) >= every_L, f"{what}: an L never current"
    assert set(L0[voice[:, 0] & decoded].tolist()) >= every_L, f"{what}: an L never previous to a decoded frame"
    for f in range(2):
        voiced, unvoiced = _voicing(st[f])
        for name, pick in (("all voiced", voiced), ("all unvoiced", unvoiced)):
            have = set(st[f]["L"][voice[:, f] & pick].tolist())
            assert have >= every_L, f"{what}: frame {f}: no {name} frame at L = {sorted(every_L - have)}"
    for c in "tis" + ("e" if codec == 1 else ""):
        before = int(((cls[:, 0] == c) & voice[:, 1]).sum())
        behind = int((voice[:, 0] & (cls[:, 1] == c)).sum())
        assert before and behind, f"{what}: class '{c}' {before} times directly before a voice frame, {behind} times directly behind one"
        out[f"class_{c}"] = (before, behind)
    return out


# ---- failure messages that name the pair ------------------------------------------------------
@contextlib.contextmanager
def named(codec, pattern, T):
    """an AssertionError of tests/parity.py that names a stream -- "(stream 1234, tick 1)", check_state's "first at (1234, ...)", the
    "streams 1024..1279" of check_state_blocks -- is raised again with the pair behind it: (b0_prev, b0_cur, pattern) and the L of the
    two frames in the oracle's decode; a comparison of frames (records, results, PCM) also says which b0 the frame carries, one of
    what the last frame left (state, RNG) does not: its "tick" is no frame"""
    lat = build(codec, pattern)
    L = (first_state(codec, pattern)[:, 0]["L"], decode(codec, pattern)["state"][:, 0]["L"])

    def pair(s, tick=None):
        s = int(s)
        if not 0 <= s < lat.b0.shape[0]:
            return ""
        at = "" if tick is None else f", frame {int(tick)} carries b0 {int(lat.b0[s, int(tick) % 2])}"
        return f" = pair (b0_prev {int(lat.b0[s, 0])}, b0_cur {int(lat.b0[s, 1])}, {pattern}; L {int(L[0][s])} -> {int(L[1][s])}{at})"

    try:
        yield
    except AssertionError as e:
        msg = str(e)
        final = re.search(r": (rng|state)\b", msg) is not None
        msg = re.sub(r"stream (\d+), tick (\d+)\)", lambda m: m.group(0)[:-1] + pair(m.group(1), None if final else m.group(2)) + ")", msg)
        block = re.search(r"streams (\d+)\.\.(\d+); indices within the block", msg)
        first = re.search(r"first at \((?:np\.\w+\()?(\d+)", msg)   # (numpy 2 prints the index as np.int64(1234))
        if first:
            s = int(first.group(1)) + (int(block.group(1)) if block else 0)
            msg += f" -- stream {s}{pair(s)}"
        elif block:
            msg += f" -- streams {block.group(1)}{pair(block.group(1))} to {block.group(2)}{pair(block.group(2))}"
        raise AssertionError(f"codec {codec} lattice {pattern}, T = {T}: {msg}") from None


class Workload:
    """what instance_cases.run_case takes in place of the edge mix: the lattice of (codec, pattern) as `variant`"""

    def __init__(self, codec, pattern, variant="pair"):
        self.codec, self.pattern, self.variant, self.figures = codec, pattern, variant, None

    # the float state is held to its bound every 256 streams (parity.check_state_blocks): over a whole lattice one pair with a wrong
    # state would be diluted 170 ... 256 times before it met the relative-RMS bound
    state_block = 256

    def frames(self, case):
        f = frames(self.codec, self.pattern, self.variant)
        assert case.codec == self.codec and f.shape[:2] == (case.S, case.T * case.launches), (case, f.shape)
        return f

    def reference(self, case, frames, seeds):
        assert np.array_equal(seeds, stream_seeds(case.S))
        return decode(self.codec, self.pattern, self.variant)

    def assert_classes(self, codec, ref):
        pair = decode(self.codec, self.pattern)
        if self.variant == "quad":   # the same two frames first: what the pair's decode holds, the quad's holds
            S = pair["state"].shape[0]
            assert ref["records"].reshape(S, 4)[:, :2].tobytes() == pair["records"].reshape(S, 2).tobytes()
        composition(self.codec, self.pattern, pair)

    def naming(self, case):
        return named(self.codec, self.pattern, case.T * case.launches)

    def report(self, case, ref, got):
        """the figures of the run for the record, before anything is asserted: relative RMS, the worst frame and its pair, the int16
        maxima below and inside the clip, the smallest margin to the bound (self.figures; the test prints them)"""
        lat = build(self.codec, self.pattern)
        T = case.T * case.launches
        total, worst, at = parity.pcm_float_stats(ref["pcmf"], got["pcmf"].reshape(-1, 160))
        st, _ = parity.int16_stats(ref["pcmf"], ref["pcm16"], got["pcm16"].reshape(-1, 160), ref["peak"])
        s, tick = at // T, at % T
        d = np.abs(ref["pcm16"].astype(np.int32) - got["pcm16"].reshape(-1, 160).astype(np.int32)).max(axis=1)
        k = int(np.argmax(d - parity.int16_bound(ref["peak"])))   # the frame nearest to (or furthest over) its int16 bound
        self.figures = {"rel_rms": float(f"{total:.3e}"), "worst_frame": float(f"{worst:.3e}"),
                        "worst_pair": (int(lat.b0[s, 0]), int(lat.b0[s, 1]), self.pattern, f"frame {tick}"),
                        "int16_max_below_clip": st["int16_max_below_clip"], "int16_max_inside_clip": st["int16_max_inside_clip"],
                        "int16_margin": st["int16_margin"], "margin_pair": (int(lat.b0[k // T, 0]), int(lat.b0[k // T, 1]), f"frame {k % T}", f"{int(d[k])} LSB"),
                        "int16_within_1": round(st["int16_within_1"], 6)}


# ---- the launch forms the lattices run through (tests/test_gpu_pitch_lattice.py) ---------------
# (form, entry of instance_cases, frames per launch, launches, variant, the instance that must run by codec; a codec without one: n/a)
FORMS = [
    ("one-batch", "batch", 1, 2, "pair", {0: "imbe_one_launch_kernel", 2: "imbe7100_stream_kernel_one_fused", 1: "ambe_one_launch_kernel",
                                          3: "ambe2400_one_launch_kernel"}),
    ("one-resident", "resident", 1, 2, "pair", {0: "imbe_one_launch_kernel_res", 2: "imbe7100_stream_kernel_res1_fused",
                                                1: "ambe_one_launch_kernel_res", 3: "ambe2400_one_launch_kernel_res"}),
    ("one-staged", "staged", 1, 2, "pair", {0: "imbe_stream_kernel_one", 3: "ambe2400_stream_kernel_one"}),
    ("one-ws", "batch_ws", 1, 2, "pair", {0: "imbe_stream_kernel_one_fused", 1: "ambe_stream_kernel_one"}),
    ("two", "batch", 2, 1, "pair", {0: "imbe_stream_kernel", 2: "imbe_stream_kernel", 1: "ambe_stream_kernel", 3: "ambe2400_stream_kernel"}),
    ("quad-lds", "batch", 4, 1, "quad", {0: "imbe_stream_kernel_lds", 1: "ambe_stream_kernel_lds", 3: "ambe2400_stream_kernel_lds"}),
    ("quad-resident", "resident", 4, 1, "quad", {0: "imbe_stream_kernel_res", 1: "ambe_stream_kernel_res", 3: "ambe2400_stream_kernel_res"}),
]
QUAD_PATTERNS = {0: ("rr", "vu"), 1: ("rr",), 3: ("rr",)}
# the one-frame resident launch of AMBE 3600x2400 goes through an index into a larger pool, as its instance case does
INDEXED = {("one-resident", 3)}


def cases():
    """[(instance_cases.Case, Workload)]: lattice by lattice, so that the tests of one lattice follow each other and share its decode"""
    import instance_cases

    out = []
    for codec, pattern in LATTICES:
        S = build_size(codec, pattern)
        for form, entry, T, launches, variant, names in FORMS:
            if codec not in names or (variant == "quad" and pattern not in QUAD_PATTERNS[codec]):
                continue
            if (form, codec) in INDEXED:
                entry += "_indexed"
            case = instance_cases.Case(f"{form}-codec{codec}-{pattern}", names[codec], codec, S, T, launches, entry, {})
            out.append((case, Workload(codec, pattern, variant)))
    return out


def build_size(codec, pattern):
    """streams of a lattice, without building it"""
    N = size(codec, pattern)
    return N * N + (2 * AMBE_VOICE_B0 * len(RIM_CLASSES[codec]) if codec in RIM_CLASSES else 0)
