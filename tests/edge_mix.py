"""The workload of the kernel-instance tests (tests/instance_cases.py): per codec, S streams x T frames in which every third
stream is random channel bits (every error bucket, repeats, mutes, headroom resets, invalid fundamentals), every third clean or
lightly flipped voice, and the rest scripted: for the AMBE codecs tone frames (valid and invalid ids) and erasures between voice
frames, for every codec runs of uncorrectable frames long enough to pass the max-repeat re-initialisation (and, IMBE, muting),
all-zero and all-one frames.  `assert_classes` then reads from the ORACLE's decode what of this the mix really held: repeats, clean
and heavily damaged frames, frames above the soft clip, a run of repeats up to the mute AND through the re-initialisation behind it
with frames decoded after it, tone and erasure frames for the AMBE codecs.  Two things it cannot or does not assert: tone frames
with an invalid id are scripted but carry the same result flags as valid ones; and IMBE 7100x4400, for which framegen has no
encoder, gets neither clean frames nor a guaranteed run (its runs are random bits), so for that codec only repeats, damage and the
clip are asserted -- its two kernel instances share the stream body of the 7200x4400 ones, which run on the full mix.
Test infrastructure: imported without a GPU; nothing in the package uses it."""
import numpy as np

from mbelib_neo_amd import framegen
from mbelib_neo_amd.layout import FRAME_BYTES

import parity

FLAG_TONE, FLAG_ERASURE, FLAG_REPEAT, FLAG_MUTE = 0x10, 0x20, 0x40, 0x80


def _voice(codec, n, rng):
    """clean voice frames of a codec (IMBE 7100x4400 has no encoder in framegen: frames with few set bits stand in for it)"""
    if codec == 0:
        return framegen.imbe_clean_voiced_frames(n, rng)
    if codec == 2:
        return framegen.random_frames(2, n, rng) & framegen.random_frames(2, n, rng) & framegen.random_frames(2, n, rng)
    return framegen.encode_ambe3600x2450(framegen.ambe_voice_param_bits(n, rng))


def _ambe_class_frames(classes, rng):
    """clean AMBE wire frames: 'v' voice, 't' valid tone id, 'i' tone signature with an invalid id, 'e' erasure (b0 = 120..123)"""
    bits = framegen.ambe_voice_param_bits(len(classes), rng)
    for k, c in enumerate(classes):
        if c in "ti":
            bits[k, 0:6] = 1
            bits[k, 45:49] = 0
            tone_id = int(rng.integers(7, 123)) if c == "t" else int(rng.choice([0, 3, 124, 127, 200, 255]))
            bits[k, 12:20] = [(tone_id >> (7 - j)) & 1 for j in range(8)]
        elif c == "e":
            bits[k, 0:4] = 1
            bits[k, 4] = 0
            bits[k, 37] = 0
    return framegen.encode_ambe3600x2450(bits)


def _uncorrectable(codec, n, rng):
    """frames the decoders answer with a REPEAT, whatever came before: IMBE 7200x4400 clean code words of an invalid fundamental
    (b0 = 208..255); AMBE voice with three flipped DATA cells in each Golay word (c0 = 3, total = 6: the error counts are differences in
    the data bits; wire bits 0..11 and 24..35); IMBE 7100x4400 (no encoder here) random bits, which repeat often but not always"""
    if codec == 2:
        return framegen.random_frames(2, n, rng)
    if codec == 0:
        bits = framegen.imbe_voiced_param_bits(n, rng)
        b0 = rng.integers(208, 256, size=n)
        for k in range(6):
            bits[:, k] = (b0 >> (7 - k)) & 1
        bits[:, 85] = (b0 >> 1) & 1
        bits[:, 86] = b0 & 1
        return framegen.encode_imbe7200x4400(bits)
    cells = np.unpackbits(_voice(codec, n, rng), axis=1)
    for i in range(n):
        cells[i, rng.choice(12, 3, replace=False)] ^= 1
        cells[i, 24 + rng.choice(12, 3, replace=False)] ^= 1
    return np.packbits(cells, axis=1)


def frames(codec, S, T, tag):
    """uint8 [S, T, 18|9]; stream s follows script s % 3 (0 random bits, 1 voice, 2 scripted: sub-script (s // 3) % 4)"""
    rng = framegen.rng_for(0xED6E0000 + 16 * int(tag) + codec)
    fb = FRAME_BYTES[codec]
    out = framegen.random_frames(codec, S * T, rng).reshape(S, T, fb)
    voice = np.arange(S) % 3 == 1
    n = int(voice.sum())
    v = _voice(codec, n * T, rng).reshape(n, T, fb)
    v[::2] = framegen.flip_bits(v[::2].reshape(-1, fb), codec, 0.005, rng).reshape(-1, T, fb)   # every other one lightly flipped
    out[voice] = v
    for s in range(2, S, 3):
        sub = (s // 3) % 4
        if sub == 0:       # voice, then a run of uncorrectable frames to the end of the stream (max-repeat, muting), voice again at the last
            k0 = int(rng.integers(0, 2))
            out[s] = _uncorrectable(codec, T, rng)
            out[s, :k0] = _voice(codec, k0, rng)
            if T > 6:
                out[s, -1:] = _voice(codec, 1, rng)
        elif sub == 1:     # all-zero and all-one frames between voice
            out[s] = _voice(codec, T, rng)
            out[s, 0::3] = 0
            out[s, 1::3] = 0xFF
        elif codec in (1, 3):   # AMBE: tones, invalid tones and erasures between voice, a tone as the very first frame
            first = "t" if sub == 2 else "e"
            out[s] = _ambe_class_frames([first] + list(rng.choice(list("vtie"), size=T - 1)), rng)
        else:              # IMBE: voice with one heavily damaged frame in the middle
            out[s] = _voice(codec, T, rng)
            out[s, T // 2] = framegen.flip_bits(out[s, T // 2:T // 2 + 1], codec, 0.2, rng)
    return out


def assert_classes(codec, ref):
    """from the oracle's decode of the mix (Oracle.process_batch): every class the instance tests rely on is in it"""
    flags = ref["results"]["flags"]
    assert (flags & FLAG_REPEAT).any(), "edge mix: no repeated frame"
    errors = ref["results"]["total_errors"]
    assert (errors == 0).any() or codec == 2, "edge mix: no clean frame"   # (IMBE 7100x4400: no encoder in framegen, no clean frames)
    assert (errors >= 6).any(), "edge mix: no heavily damaged frame"
    assert (ref["peak"] > parity.CLIP_LEVEL).any(), "edge mix: no frame above the soft clip"
    assert (ref["state"]["repeatCount"] == 0).any() and (ref["state"]["repeatCount"] > 0).any(), "edge mix: repeat counters"
    # (IMBE 7100x4400 has no encoder in framegen: its runs are random bits, which repeat often, but four in a row are not certain in six frames)
    assert (flags & FLAG_MUTE).any() or codec == 2, "edge mix: no muted frame (a run of repeats past the maximum)"
    S = ref["state"].shape[0]
    by_stream = flags.reshape(S, -1)
    T = by_stream.shape[1]
    if codec == 0 and T >= 6:     # IMBE: the fifth repeat in a row goes through the headroom reset, and a frame is decoded on what it left
        rep = (by_stream & FLAG_REPEAT) != 0
        run5 = np.zeros(S, dtype=bool)
        for t in range(T - 5):
            run5 |= rep[:, t:t + 5].all(axis=1)
        assert run5.any(), "edge mix: no run of five repeats followed by a frame (max-repeat re-initialisation)"
    if codec in (1, 3) and T >= 6:   # AMBE: the muted frame IS the re-initialisation; a frame must follow it in its stream
        assert ((by_stream[:, :-1] & FLAG_MUTE) != 0).any(), "edge mix: no frame decoded after a max-repeat re-initialisation"
    if codec in (1, 3):
        assert (flags & FLAG_TONE).any(), "edge mix: no tone frame"
        assert (flags & FLAG_ERASURE).any() or codec == 3, "edge mix: no erasure frame"   # (AMBE 3600x2400 has no erasure class)
