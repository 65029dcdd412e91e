"""Workloads and runners of tests/test_gpu_silent_stores.py: the one-frame stream instances skip the stores of an all-zero
previousUw over zeros (store_parms, mbx_stream.hip), and that must never change a byte of the state.

Frames: 'V' clean all-voiced (framegen), 'U' clean code words of random parameter bits with a valid fundamental (unvoiced bands),
'X' clean code words of an invalid fundamental (b0 = 208..255: a REPEAT whatever came before, no bit errors), 'D' an all-voiced
frame with the most errors the codes still correct (three data cells in every Golay word, one in every Hamming word: 15 of IMBE
7200x4400, 14 of 7100x4400: a REPEAT with errors), 'E' the same with ONE error in C0 (13 / 12: decoded, c0 < 2 never repeats).
A run of four X reaches the mute through the repeat counter.  A mute directly behind a decoded frame can only come from the error
rate, and only on a frame that is not repeated (a repeat takes prev_mp's error rate): an E on an error rate planted just below
the muting threshold (PLANTED_ERROR_RATE in the INITIAL state, the same for every launch form compared) crosses it.  IMBE 7100x4400 has no encoder in framegen: `encode_imbe7100x4400`
(tests/imbe7100_frames.py) is the inverse of the oracle's front end, checked against it frame by frame here (`check_encoder`).
Test infrastructure: imported without a GPU; nothing in the package uses it."""
import numpy as np

from mbelib_neo_amd import framegen
from mbelib_neo_amd.layout import FRAME_BYTES, PARMS_DTYPE, ROW_WIDTHS, init_state

from imbe7100_frames import encode_imbe7100x4400

FLAG_REPEAT, FLAG_MUTE = 0x40, 0x80
S = 67          # nine chunks of eight streams, the last one short
TICKS = 6
UW_BYTE = PARMS_DTYPE.fields["previousUw"][1]
# errorRate' = 0.95 errorRate + 0.000365 total, muted above 0.0875.  The clean first frame must stay at or below the threshold and
# the E behind it (total 13 / 12: + 0.004745 / 0.00438) must cross it: 7200x4400 0.0919 -> 0.087305 -> 0.087685; 7100x4400 has
# 5e-6 of room, 0.0921037 -> 0.0874985 -> 0.0875036 (float arithmetic, the same on the oracle and the device; `classes` asserts it)
PLANTED_ERROR_RATE = {0: 0.0919, 2: 0.0921037}
CLASSES = "VURM"
# per stream (s % len): the frame kinds of its six ticks and whether its initial error rate is planted
SCRIPTS = (("VEEXVU", True), ("UEVDUV", True), ("VVUUXX", False), ("XXXXXV", False), ("VEUXUV", True), ("UXVXXX", False),
           ("VEXVDX", True), ("UUXVVU", False), ("XUDDXV", True), ("XXXXVU", False))


# ---- frames -----------------------------------------------------------------------------------
def _set_b0(bits, b0):
    for k in range(6):
        bits[:, k] = (b0 >> (7 - k)) & 1
    bits[:, 85] = (b0 >> 1) & 1
    bits[:, 86] = b0 & 1


def param_bits(kind, n, rng):
    """[n, 88] parameter bits in the 7200x4400 order for frames of one kind (D, E: as V, the damage is done on the wire)"""
    bits = framegen.imbe_voiced_param_bits(n, rng)
    if kind == "U":
        b0 = rng.integers(0, 208, size=n, dtype=np.int64)
        bits = rng.integers(0, 2, size=(n, 88), dtype=np.uint8)
        _set_b0(bits, b0)
    elif kind == "X":
        _set_b0(bits, rng.integers(208, 256, size=n, dtype=np.int64))
    return bits


def _damage(codec, frames, rng, c0=3):
    """`c0` flipped data cells in C0, three in every other Golay word, one in every Hamming word (all corrected)"""
    cells = np.unpackbits(frames, axis=1)
    widths = ROW_WIDTHS[codec]
    # row -> its leading cells that are DATA bits (the error counts are differences in the data bits: flips of parity cells count nothing)
    golay = {0: {0: 12, 1: 12, 2: 12, 3: 12}, 2: {0: 7, 1: 12, 2: 12, 3: 12}}[codec]
    hamming = {0: (4, 5, 6), 2: (4, 5)}[codec]
    for i in range(cells.shape[0]):
        at = 0
        for r, w in enumerate(widths):
            if r in golay:
                cells[i, at + rng.choice(golay[r], 3 if r else c0, replace=False)] ^= 1
            elif r in hamming:
                cells[i, at + int(rng.integers(0, 11))] ^= 1
            at += w
    return np.packbits(cells, axis=1)


def frames_of(codec, kinds, rng, oracle):
    """one wire frame per letter of `kinds`"""
    fb = FRAME_BYTES[codec]
    out = np.zeros((len(kinds), fb), dtype=np.uint8)
    for kind in set(kinds):
        pick = np.array([i for i, c in enumerate(kinds) if c == kind])
        bits = param_bits(kind, len(pick), rng)
        fr = framegen.encode_imbe7200x4400(bits) if codec == 0 else encode_imbe7100x4400(bits, oracle)
        out[pick] = _damage(codec, fr, rng, 3 if kind == "D" else 1) if kind in "DE" else fr
    return out


def check_encoder(codec, oracle):
    """clean frames decode to the bits they were made of, without an error; damaged ones too, with 15 / 14 (D) and 13 / 12 (E)"""
    import oracle_lib

    rng = framegen.rng_for(0x51E70000 + codec)
    for kind, total in (("V", 0), ("U", 0), ("X", 0), ("D", 15 if codec == 0 else 14), ("E", 13 if codec == 0 else 12)):
        bits = param_bits(kind, 48, rng)
        fr = framegen.encode_imbe7200x4400(bits) if codec == 0 else encode_imbe7100x4400(bits, oracle)
        if kind in "DE":
            fr = _damage(codec, fr, rng, 3 if kind == "D" else 1)
        rec = oracle.fec_batch(codec, fr)
        assert np.array_equal(oracle_lib.records_to_bits(rec, 88), bits), (codec, kind)
        assert (oracle_lib.records_to_results(rec)["total_errors"] == total).all(), (codec, kind)


def scripted(codec, oracle, scripts=SCRIPTS, tag=0):
    """(frames uint8 [S, ticks, 18], initial state [S, 3], seeds): stream s follows scripts[s % len(scripts)]"""
    rng = framegen.rng_for(0x51E71000 + 16 * tag + codec)
    ticks = len(scripts[0][0])
    frames = np.zeros((S, ticks, FRAME_BYTES[codec]), dtype=np.uint8)
    state = init_state(S)
    for s in range(S):
        kinds, planted = scripts[s % len(scripts)]
        frames[s] = frames_of(codec, kinds, rng, oracle)
        if planted:
            state[s]["errorRate"] = PLANTED_ERROR_RATE[codec]
    return frames, state, np.arange(S) * 7 + 31 + codec


def classes(codec, oracle, frames, state, seeds):
    """[S, ticks] of 'V', 'U', 'R', 'M' from the ORACLE's decode: mute and repeat from the result flags of the tick, all-voiced or
    not from the voicing decisions cur_mp holds after it (bands 1..L)"""
    n, ticks = frames.shape[:2]
    rng = oracle.rng_seeded(seeds)
    out = np.empty((n, ticks), dtype="U1")
    for k in range(1, ticks + 1):
        ref = oracle.process_batch(codec, n, k, frames[:, :k].reshape(n * k, -1), state, rng)
        flags = ref["results"]["flags"].reshape(n, k)[:, k - 1]
        cur = ref["state"][:, 0]
        band = np.arange(cur["Vl"].shape[1])[None, :]
        live = (band >= 1) & (band <= cur["L"][:, None])
        voiced = ((cur["Vl"] == 1) | ~live).all(axis=1)
        out[:, k - 1] = np.where(flags & FLAG_MUTE, "M", np.where(flags & FLAG_REPEAT, "R", np.where(voiced, "V", "U")))
    return out


def pairs_seen(cls):
    return {a + b for row in cls for a, b in zip(row[:-1], row[1:])}


# ---- GPU runners ------------------------------------------------------------------------------
def _decoder(codec, state, seeds, resident=False):
    from mbelib_neo_amd import decoder

    dec = decoder.BatchDecoder(codec, state.shape[0], seeds=seeds, resident=resident)
    dec.set_state(state)
    return dec


def _snapshot(dec):
    """state [S, 3] and rng bytes as the ABI holds them; a resident decoder is materialised on a COPY, so its elision stays on"""
    import torch

    from mbelib_neo_amd import decoder

    if dec.resident is None:
        st = dec.state_numpy()
    else:
        tmp = decoder.BatchDecoder(dec.codec, dec.streams, resident=True)
        tmp.state.copy_(dec.state)
        tmp.resident.copy_(dec.resident)
        st = tmp.state_numpy()
    torch.cuda.synchronize()
    return st.copy(), dec.rng_numpy().copy()


def _outputs(out, n, k):
    from mbelib_neo_amd import decoder

    return (decoder.results_numpy(out["results"]).reshape(n, k), out["pcm16"].cpu().numpy().reshape(n, k, 160),
            out["pcmf"].cpu().numpy().reshape(n, k, 160))


def run_history(codec, frames, state, seeds, resident=False):
    """Tick by tick through T = 1 launches; after tick k everything must be byte-identical to ONE launch of T = k from the same
    initial state (a multi-frame instance, which stores every struct whole).  The library alternates the walking order of
    successive launches, and the reference launches sit between the one-frame ones, so all six of those walk one way; a second
    pass, one launch later, walks the other way."""
    from mbelib_neo_amd import _native

    n, ticks = frames.shape[:2]
    L = _native.lib()
    previous = L.mbx_set_stream_order(1)
    try:
        for direction in range(2):
            dec = _decoder(codec, state, seeds, resident)
            for k in range(1, ticks + 1):
                res1, pcm1, pcmf1 = _outputs(dec.decode(frames[:, k - 1], 1, want_float=True), n, 1)
                got_state, got_rng = _snapshot(dec)
                ref = _decoder(codec, state, seeds)
                resk, pcmk, pcmfk = _outputs(ref.decode(frames[:, :k].reshape(n * k, -1), k, want_float=True), n, k)
                ref_state, ref_rng = _snapshot(ref)
                what = f"codec {codec} resident {resident} pass {direction} tick {k}"
                for name in PARMS_DTYPE.names:
                    for slot in range(3):
                        a, b = got_state[:, slot][name], ref_state[:, slot][name]
                        same = (a.view(np.uint32) == b.view(np.uint32)).reshape(n, -1).all(axis=1)
                        assert same.all(), f"{what}: state slot {slot} field {name} differs in streams {np.flatnonzero(~same)[:8]}"
                assert got_state.tobytes() == ref_state.tobytes(), f"{what}: state bytes"
                assert got_rng.tobytes() == ref_rng.tobytes(), f"{what}: rng"
                assert res1[:, 0].tobytes() == np.ascontiguousarray(resk[:, k - 1]).tobytes(), f"{what}: results"
                assert pcm1[:, 0].tobytes() == np.ascontiguousarray(pcmk[:, k - 1]).tobytes(), f"{what}: int16 PCM"
                assert pcmf1[:, 0].tobytes() == np.ascontiguousarray(pcmfk[:, k - 1]).tobytes(), f"{what}: float PCM"
            _decoder(codec, state, seeds).decode(frames[:, 0], 1)   # one launch more: the next pass starts in the other direction
    finally:
        L.mbx_set_stream_order(previous)


def staged_step(dec, frames):
    """one T = 1 step as three calls: mbx_fec_*, mbx_expand_records, mbx_stream_expanded (the staged one-frame stream instance)"""
    import torch

    from mbelib_neo_amd import _native

    L = _native.lib()
    n = dec.streams
    d_frames = dec.to_device(frames)
    out = dec.make_outputs(1, want_float=True)
    strm = torch.cuda.current_stream().cuda_stream
    fec = {0: L.mbx_fec_imbe7200x4400, 2: L.mbx_fec_imbe7100x4400}[dec.codec]
    _native.check(fec(d_frames.data_ptr(), n, out["records"].data_ptr(), strm), "mbx_fec")
    _native.check(L.mbx_expand_records(0, out["records"].data_ptr(), n, strm), "mbx_expand_records")
    _native.check(L.mbx_stream_expanded(0, n, 1, out["records"].data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(),
                                        out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(), strm),
                  "mbx_stream_expanded")
    return out


# ---- planted previousUw -----------------------------------------------------------------------
NAN_BITS, NEG_ZERO_BITS = 0x7FC00001, 0x80000000


def planted_patterns():
    """name -> (cur_mp.previousUw, prev_mp_enhanced.previousUw) as uint32 [256] (None: left as initialised, all zero)"""
    ramp = (np.arange(256, dtype=np.float32) * 0.25 + 0.5).view(np.uint32)
    zero = np.zeros(256, dtype=np.uint32)

    def one(i, bits):
        v = zero.copy()
        v[i] = bits
        return v

    upper, lower = zero.copy(), zero.copy()
    upper[128:] = ramp[128:]
    lower[:128] = ramp[:128]
    return {
        "i cur zero, enhanced upper half set": (zero, upper),
        "ii cur set, enhanced upper half zero": (ramp, lower),
        "iii -0.0f in lane 17 of uw[1]": (one(64 + 17, NEG_ZERO_BITS), None),
        "iv a NaN in one dword": (one(150, NAN_BITS), None),
        "v previousUw[0] set": (one(0, ramp[3]), None),
        "vi previousUw[255] set": (one(255, ramp[3]), None),
        "vii cur zero, enhanced lower half set": (zero, lower),
    }


PLANTED_STREAMS = (3, 8, 15, 24, 41, 58, 66)   # one stream per pattern: first and last of a chunk, the short last chunk


def plant(dec, patterns):
    """write the patterns into the decoder's device state (dec.state, bytes), one stream each"""
    import torch

    words = dec.state.view(torch.int32).reshape(dec.streams, 3, PARMS_DTYPE.itemsize // 4)
    lo = UW_BYTE // 4
    for s, (cur, enh) in zip(PLANTED_STREAMS, patterns.values()):
        words[s, 0, lo:lo + 256] = torch.from_numpy(cur.view(np.int32)).to(words.device)
        if enh is not None:
            words[s, 2, lo:lo + 256] = torch.from_numpy(enh.view(np.int32)).to(words.device)
