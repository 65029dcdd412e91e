"""Workloads and runners of tests/test_gpu_lean_state_io.py: the IMBE one-frame stream instances request of prev_mp only what the decode
reads (a repeat takes Ml from the struct it reloads, with the decode's padding), carry log2Ml across the synthesiser in LDS and leave
an unchanged rng record unstored (kLean*, mbx_stream.hip).  None of that may change a byte.

Frame kinds: those of tests/silent_store_cases.py ('V' all-voiced, 'U' unvoiced bands at a random fundamental, 'X' an invalid
fundamental: a repeat WITHOUT a decode, 'D' a corrected frame with the most errors the codes allow: a repeat BEHIND a good decode, 'E'
decoded with errors) and four with a set fundamental: 'S' / 'G' clean frames of b0 = 20 / 190 (a short and a long harmonic count),
's' / 'g' the same damaged like 'D'.  "Sg" is then a repeat with prev_L < cur_L (the decode padded harmonics prev_L + 1 .. cur_L of the
prediction memory before the policy copied it), "Gs" one with prev_L > cur_L (only harmonic 0 is padded), "SX" / "GX" repeats the
padding never reached.
Test infrastructure: imported without a GPU; nothing in the package uses it.  `python tests/lean_state_cases.py <form>` runs one
scripted history in a fresh process, for the forms that need a launch switch in the environment (FORMS)."""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import silent_store_cases as ssc  # noqa: E402
from mbelib_neo_amd import framegen  # noqa: E402
from mbelib_neo_amd.layout import FRAME_BYTES, PARMS_DTYPE, RESULT_DTYPE, RNG_DTYPE, init_state, rng_default, rng_seeded  # noqa: E402

FLAG_REPEAT, FLAG_MUTE = ssc.FLAG_REPEAT, ssc.FLAG_MUTE
TICKS = 8
B0_SHORT, B0_LONG = 20, 190
MAX_REPEATS = 4   # MBE_MAX_FRAME_REPEATS

# A launch form of the T = 1 step: the kernel a launch must report, the codec, the streams (67: nine chunks of eight, the last one
# short; 320: the smallest count above the 256-frame limit below which a step is staged, in chunks of eight), resident state or the
# ABI triplets, and the launch switches the process needs.  The fused instances are selected only above that limit: they run at 320.
Form = namedtuple("Form", "kernel codec n resident env")
FORMS = {
    "one": Form("imbe_stream_kernel_one", 0, 67, False, {}),
    "res1": Form("imbe_stream_kernel_res1", 0, 67, True, {}),
    "one_7100": Form("imbe_stream_kernel_one", 2, 67, False, {}),
    "one_launch": Form("imbe_one_launch_kernel", 0, 320, False, {}),
    "one_launch_res": Form("imbe_one_launch_kernel_res", 0, 320, True, {}),
    "fused_7100": Form("imbe7100_stream_kernel_one_fused", 2, 320, False, {}),
    "fused_7100_res": Form("imbe7100_stream_kernel_res1_fused", 2, 320, True, {}),
    "fused": Form("imbe_stream_kernel_one_fused", 0, 320, False, {"MBX_FUSE_ONE": "1"}),
    "fused_res": Form("imbe_stream_kernel_res1_fused", 0, 320, True, {"MBX_FUSE_ONE": "1"}),
}

# per stream (s % len): the frame kinds of its eight ticks, whether its initial error rate is planted just below the muting threshold
# (silent_store_cases.PLANTED_ERROR_RATE) and whether a cold-start seed is pending in its rng record
SCRIPTS = (
    ("SgVGsVUV", False, True),    # repeats behind a good decode, prev_L < cur_L and prev_L > cur_L
    ("GsSgXVUV", False, False),
    ("XXXXXXVU", False, True),    # five repeats in a row and one more: mute, headroom reset; the cold start comes late
    ("VXXXXXXV", False, False),
    ("VUVUVVUV", False, True),    # unvoiced bands between all-voiced frames
    ("VEEXVUVU", True, False),    # a mute from the error rate
    ("SXGXSgGs", False, True),    # repeats without a decode behind both harmonic counts
    ("UUXVVUDU", False, False),
    ("XUDDXVUV", True, True),
    ("GVUVSUVg", False, False),
)


# ---- frames -----------------------------------------------------------------------------------
def frames_of(codec, kinds, rng, oracle):
    """one wire frame per letter of `kinds`"""
    from imbe7100_frames import encode_imbe7100x4400

    out = np.zeros((len(kinds), FRAME_BYTES[codec]), dtype=np.uint8)
    for kind in set(kinds):
        pick = np.array([i for i, c in enumerate(kinds) if c == kind])
        if kind in "SGsg":
            bits = framegen.imbe_voiced_param_bits(len(pick), rng)
            ssc._set_b0(bits, B0_SHORT if kind in "Ss" else B0_LONG)
            fr = framegen.encode_imbe7200x4400(bits) if codec == 0 else encode_imbe7100x4400(bits, oracle)
            out[pick] = ssc._damage(codec, fr, rng, 3) if kind in "sg" else fr
        else:
            out[pick] = ssc.frames_of(codec, "".join(kind for _ in pick), rng, oracle)
    return out


def scripted(codec, n, oracle, scripts=SCRIPTS, tag=0):
    """(frames uint8 [n, ticks, 18], initial state [n, 3], initial rng records [n]): stream s follows scripts[s % len(scripts)]"""
    rng = framegen.rng_for(0x1EA70000 + 4096 * tag + 16 * n + codec)
    ticks = len(scripts[0][0])
    frames = np.zeros((n, ticks, FRAME_BYTES[codec]), dtype=np.uint8)
    state = init_state(n)
    records = rng_default(n)
    seeded = rng_seeded(np.arange(n) * 7 + 31 + codec)
    for s in range(n):
        kinds, planted, pending = scripts[s % len(scripts)]
        frames[s] = frames_of(codec, kinds, rng, oracle)
        if planted:
            state[s]["errorRate"] = ssc.PLANTED_ERROR_RATE[codec]
        if pending:
            records[s] = seeded[s]
    return frames, state, records


def trace(codec, oracle, frames, state, records):
    """the ORACLE's decode tick by tick: dict of [n, ticks] arrays -- flags, total errors, c0 errors, cur_mp.L / repeatCount behind the
    tick, prev_mp.L in front of it, the class of silent_store_cases.classes, whether the rng record changed, and the records [n, ticks]"""
    n, ticks = frames.shape[:2]
    out = {k: np.zeros((n, ticks), dtype=np.int64) for k in ("flags", "total", "c0", "L", "repeats", "prev_L", "rng_changed")}
    out["cls"] = np.empty((n, ticks), dtype="U1")
    out["rng"] = np.zeros((n, ticks), dtype=RNG_DTYPE)
    out["cold"] = np.zeros((n, ticks), dtype=bool)      # cur_mp.noiseSeed < 0 in front of the tick
    out["pending"] = np.zeros((n, ticks), dtype=bool)   # a cold-start seed waits in the record in front of the tick
    st, rg = state, records
    for k in range(ticks):
        ref = oracle.process_batch(codec, n, 1, frames[:, k], st, rg)
        flags = ref["results"]["flags"]
        cur = ref["state"][:, 0]
        band = np.arange(cur["Vl"].shape[1])[None, :]
        live = (band >= 1) & (band <= cur["L"][:, None])
        voiced = ((cur["Vl"] == 1) | ~live).all(axis=1)
        out["cls"][:, k] = np.where(flags & FLAG_MUTE, "M", np.where(flags & FLAG_REPEAT, "R", np.where(voiced, "V", "U")))
        out["flags"][:, k] = flags
        out["total"][:, k] = ref["results"]["total_errors"]
        out["c0"][:, k] = ref["results"]["c0_errors"]
        out["L"][:, k] = cur["L"]
        out["repeats"][:, k] = cur["repeatCount"]
        out["prev_L"][:, k] = np.asarray(st)[:, 1]["L"]
        out["cold"][:, k] = np.asarray(st)[:, 0]["noiseSeed"] < 0
        out["pending"][:, k] = np.asarray(rg)["unvoiced_seed_override"] != 0
        out["rng_changed"][:, k] = [a.tobytes() != b.tobytes() for a, b in zip(np.asarray(rg), ref["rng"])]
        out["rng"][:, k] = ref["rng"]
        st, rg = ref["state"], ref["rng"]
    return out


def kinds_of(n, scripts=SCRIPTS):
    return np.array([list(scripts[s % len(scripts)][0]) for s in range(n)])


def assert_cases(codec, n, tr, scripts=SCRIPTS):
    """every case the histories are written for occurs, by the oracle's own flags and state"""
    kinds = kinds_of(n, scripts)
    rep = (tr["flags"] & FLAG_REPEAT) != 0
    mute = (tr["flags"] & FLAG_MUTE) != 0
    most = 15 if codec == 0 else 14
    L_short, L_long = set(tr["L"][(kinds == "S") & ~rep]), set(tr["L"][(kinds == "G") & ~rep])
    assert len(L_short) == 1 and len(L_long) == 1 and min(L_short) + 8 < min(L_long), (L_short, L_long)
    L_short, L_long = min(L_short), min(L_long)
    decoded_repeat = rep & (tr["total"] == most) & (tr["c0"] >= 2)      # a good decode, repeated for its error counts
    up = decoded_repeat[:, 1:] & (kinds[:, 1:] == "g") & (tr["prev_L"][:, 1:] == L_short)
    down = decoded_repeat[:, 1:] & (kinds[:, 1:] == "s") & (tr["prev_L"][:, 1:] == L_long)
    assert up.any(axis=0).sum() >= 2 and down.any(axis=0).sum() >= 2, "no repeat behind a decode with prev_L < cur_L / prev_L > cur_L"
    undecoded = rep & (kinds == "X") & (tr["total"] == 0)
    assert (undecoded & (tr["prev_L"] == L_short)).any() and (undecoded & (tr["prev_L"] == L_long)).any(), "no repeat from an invalid b0"
    run5 = np.zeros(n, dtype=bool)
    for k in range(tr["flags"].shape[1] - 4):
        run5 |= rep[:, k:k + 5].all(axis=1)
    assert run5.any(), "no five repeats in a row"
    assert (rep & mute & (tr["repeats"] >= MAX_REPEATS)).any(), "no mute from the repeat counter"
    assert (rep[:, 1:] & (tr["repeats"][:, 1:] == 0) & (tr["repeats"][:, :-1] >= MAX_REPEATS)).any(), "no headroom reset"
    assert (mute & ~rep).any(), "no mute from the error rate"
    cls = tr["cls"]
    vuv = (cls[:, :-2] == "V") & (cls[:, 1:-1] == "U") & (cls[:, 2:] == "V")
    assert len(set(tr["L"][:, 1:-1][vuv])) >= 3, "unvoiced bands between all-voiced frames at fewer than three harmonic counts"
    # rng: a cold start with and without a pending seed, a pending seed that waits for a late cold start, comfort noise, and frames
    # behind each of them that leave the record as it is
    pending_before = tr["pending"]
    pending_after = tr["rng"]["unvoiced_seed_override"] != 0
    changed = tr["rng_changed"] != 0
    assert (changed & pending_before & ~pending_after & tr["cold"]).any(), "no pending seed taken by a cold start"
    assert (tr["cold"][:, 1:] & changed[:, 1:]).any(), "no pending seed that waited for a late cold start"
    assert (~changed & tr["cold"] & ~mute & ~pending_before).any(), "no cold start without a pending seed"
    assert (changed & mute).any(), "no comfort-noise frame"
    assert (~changed[:, 1:] & mute[:, :-1] & ~mute[:, 1:]).any(), "no unchanged record behind a muted frame"
    assert (~changed).mean() > 0.5, "the record should be left alone by most frames"


# ---- GPU runners ------------------------------------------------------------------------------
def _decoder(form, state, records):
    from mbelib_neo_amd import decoder

    dec = decoder.BatchDecoder(form.codec, state.shape[0], resident=form.resident)
    dec.set_state(state, records)
    return dec


def _ran(form, L, what):
    import torch

    name = L.mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream)
    assert name is not None and name.decode() == form.kernel, f"{what}: ran {name!r}, the case is for {form.kernel}"


def same_bytes(what, got, ref, pick=None):
    """state [n, 3] against state [n, 3], field by field as bits; names the field and the streams"""
    n = got.shape[0]
    pick = np.arange(n) if pick is None else pick
    for name in PARMS_DTYPE.names:
        for slot in range(3):
            a, b = got[pick, slot][name], ref[pick, slot][name]
            same = (np.ascontiguousarray(a).view(np.uint32) == np.ascontiguousarray(b).view(np.uint32)).reshape(len(pick), -1).all(axis=1)
            assert same.all(), f"{what}: state slot {slot} field {name} differs in streams {pick[np.flatnonzero(~same)][:8]}"
    assert np.ascontiguousarray(got[pick]).tobytes() == np.ascontiguousarray(ref[pick]).tobytes(), f"{what}: state bytes"


def run_history(form, frames, state, records, oracle, passes=2):
    """Tick by tick through T = 1 launches of the form; behind tick k state, rng records, results and PCM are byte-identical to ONE
    launch of T = k from the same initial state on the ABI triplets (a multi-frame instance: whole views, every store made, log2Ml
    read back from the slot or kept in registers), in both walking orders (cf. silent_store_cases.run_history).  The last pass is then
    held to the oracle: results and rng records exact, PCM and state under tests/parity.py."""
    import parity
    from mbelib_neo_amd import _native

    for k, v in form.env.items():
        assert os.environ.get(k) == v, f"{form.kernel}: needs {k}={v} in the environment of a fresh process"
    n, ticks = frames.shape[:2]
    plain = form._replace(resident=False)
    L = _native.lib()
    previous = L.mbx_set_stream_order(1)
    try:
        for direction in range(passes):
            dec = _decoder(form, state, records)
            got = {"results": [], "pcm16": [], "pcmf": []}
            for k in range(1, ticks + 1):
                what = f"{form.kernel} codec {form.codec} pass {direction} tick {k}"
                res1, pcm1, pcmf1 = ssc._outputs(dec.decode(frames[:, k - 1], 1, want_float=True), n, 1)
                _ran(form, L, what)
                got_state, got_rng = ssc._snapshot(dec)
                ref = _decoder(plain, state, records)
                resk, pcmk, pcmfk = ssc._outputs(ref.decode(frames[:, :k].reshape(n * k, -1), k, want_float=True), n, k)
                ref_state, ref_rng = ssc._snapshot(ref)
                same_bytes(what, got_state, ref_state)
                assert got_rng.tobytes() == ref_rng.tobytes(), f"{what}: rng records of streams {np.flatnonzero(got_rng != ref_rng)[:8]}"
                assert res1[:, 0].tobytes() == np.ascontiguousarray(resk[:, k - 1]).tobytes(), f"{what}: results"
                assert pcm1[:, 0].tobytes() == np.ascontiguousarray(pcmk[:, k - 1]).tobytes(), f"{what}: int16 PCM"
                assert pcmf1[:, 0].tobytes() == np.ascontiguousarray(pcmfk[:, k - 1]).tobytes(), f"{what}: float PCM"
                got["results"].append(res1)
                got["pcm16"].append(pcm1)
                got["pcmf"].append(pcmf1)
            _decoder(plain, state, records).decode(frames[:, 0], 1)   # one launch more: the next pass starts in the other direction
    finally:
        L.mbx_set_stream_order(previous)
    ref = oracle.process_batch(form.codec, n, ticks, frames.reshape(n * ticks, -1), state, records)
    what = f"{form.kernel} codec {form.codec} against the oracle"
    with parity.located(ticks):
        parity.check_results(ref["results"], np.concatenate(got["results"], axis=1).reshape(-1).view(RESULT_DTYPE), what + ": results")
        parity.check_pcm(ref["pcmf"], np.concatenate(got["pcmf"], axis=1).reshape(-1, 160), ref["pcm16"],
                         np.concatenate(got["pcm16"], axis=1).reshape(-1, 160), what=what + ": pcm", peak=ref["peak"])
    parity.check_state(ref["state"], got_state, what=what + ": state (rows are streams)")
    parity.check_exact(ref["rng"], got_rng, what + ": rng")


# ---- planted prev_mp: sentinels a repeat must carry into cur_mp ---------------------------------
NAN_BITS, NEG_ZERO_BITS = ssc.NAN_BITS, ssc.NEG_ZERO_BITS
PLANT_SCRIPTS = (("SX", False, True), ("Sg", False, True), ("GX", False, True), ("Gs", False, True), ("SS", False, True))


def pad(v, prev_L, cur_L):
    """the decode's padding of one prediction-memory array [57]: harmonics prev_L + 1 .. cur_L take harmonic prev_L's value, 0 takes 1's"""
    out = v.copy()
    out[prev_L + 1:cur_L + 1] = v[prev_L]
    out[0] = out[1]
    return out


def planted_prev(codec, n, oracle):
    """(frames [n, 2, 18], state [n, 3] behind the FIRST frame with prev_mp.Ml / prev_mp.noiseSeed replaced by sentinels, records, and the
    sentinels): a distinct value per stream and harmonic, a -0.0f in harmonic 7 of every stream, a NaN in harmonic 23 of every fourth"""
    frames, state, records = scripted(codec, n, oracle, scripts=PLANT_SCRIPTS, tag=1)
    ref = oracle.process_batch(codec, n, 1, frames[:, 0], state, records)
    state, records = ref["state"].copy(), ref["rng"].copy()
    ml = (1.0 + np.arange(57, dtype=np.float32)[None, :] / 64.0 + np.arange(n, dtype=np.float32)[:, None] / 1024.0).astype(np.float32)
    bits = ml.view(np.uint32).copy()
    bits[:, 7] = NEG_ZERO_BITS
    bits[1::4, 23] = NAN_BITS
    seeds = (1000.0 + 3.0 * np.arange(n)).astype(np.float32)   # integer-valued and below 53,125, as every seed the generator leaves
    state[:, 1]["Ml"] = bits.view(np.float32)
    state[:, 1]["noiseSeed"] = seeds
    return frames, state, records, bits, seeds


def run_planted_prev(form, oracle):
    """one T = 1 launch of the form over planted prev_mp structs.  The snapshot the frame leaves in prev_mp is the struct a repeat
    copied: Ml as planted -- with the decode's padding where the decode ran, untouched where it did not, every bit of the -0.0f and
    the NaN included --, the planted noiseSeed, repeatCount one up; a decoded frame replaces them.  The streams without a NaN are
    byte-identical to one T = 2 launch of the same two frames (a multi-frame instance) behind one more all-voiced tick."""
    from mbelib_neo_amd import _native

    frames, state, records, bits, seeds = planted_prev(form.codec, form.n, oracle)
    n = form.n
    first, kinds = kinds_of(n, PLANT_SCRIPTS).T
    tr = trace(form.codec, oracle, frames[:, 1:], state, records)
    rep = (tr["flags"][:, 0] & FLAG_REPEAT) != 0
    assert (rep == (kinds != "S")).all() and (tr["repeats"][:, 0] == rep).all(), "the scripts' repeats"
    prev_L = state[:, 1]["L"]
    L_of = {k: int(prev_L[first == k][0]) for k in "SG"}   # the harmonic counts of the two set fundamentals, from the oracle's decode
    assert L_of["S"] + 8 < L_of["G"] and all((prev_L[first == k] == L_of[k]).all() for k in "SG"), L_of
    dec = _decoder(form, state, records)
    dec.decode(frames[:, 1], 1, want_float=True)
    _ran(form, _native.lib(), "planted prev_mp")
    got, _ = ssc._snapshot(dec)
    snap_ml = got[:, 1]["Ml"].view(np.uint32)
    for s in np.flatnonzero(rep):
        want = bits[s] if kinds[s] == "X" else pad(bits[s], int(prev_L[s]), L_of[kinds[s].upper()])
        assert np.array_equal(snap_ml[s], want), f"stream {s} ({kinds[s]} behind L = {prev_L[s]}): prev_mp.Ml {snap_ml[s]} is not the planted {want}"
        assert got[s, 1]["noiseSeed"] == seeds[s] and got[s, 1]["repeatCount"] == 1, f"stream {s}: noiseSeed / repeatCount of the copied struct"
    assert np.array_equal(got[~rep][:, 1]["noiseSeed"], state[~rep][:, 0]["noiseSeed"]), "a decoded frame snapshots cur_mp's noiseSeed, not prev_mp's"
    assert (state[~rep][:, 0]["noiseSeed"] != seeds[~rep]).all()
    # ... and the whole state against a multi-frame instance, one all-voiced tick later (the NaN streams left out: which of two
    # NaN operands an addition returns is the instruction order's business, not the state's)
    clean = np.flatnonzero(~(bits == NAN_BITS).any(axis=1))
    third = frames_of(form.codec, "V" * n, framegen.rng_for(0x1EA7F000 + form.codec), oracle)
    dec.decode(third, 1, want_float=True)
    got2, got_rng = ssc._snapshot(dec)
    ref = _decoder(form._replace(resident=False), state, records)
    ref.decode(np.concatenate([frames[:, 1:2], third[:, None]], axis=1).reshape(2 * n, -1), 2, want_float=True)
    ref2, ref_rng = ssc._snapshot(ref)
    same_bytes(f"{form.kernel}: planted prev_mp, two ticks", got2, ref2, clean)
    assert got_rng.tobytes() == ref_rng.tobytes(), "rng records"


# ---- planted rng records ------------------------------------------------------------------------
RESERVED = 0xDEADBEEF
# name -> (cold state?, muted by a planted error rate?, the record's cn_seeded, unvoiced_seed_override, the fields a frame changes)
RNG_CASES = {
    "warm, nothing pending": (False, False, 1, 0, ()),
    "cold start, seed pending": (True, False, 1, 1, ("unvoiced_seed_override",)),
    "cold start, nothing pending": (True, False, 1, 0, ()),
    "warm, seed pending (waits)": (False, False, 1, 1, ()),
    "comfort noise, generator seeded": (False, True, 1, 0, ("cn_seed48",)),
    "comfort noise, generator unseeded": (False, True, 0, 0, ("cn_seed48", "cn_seeded")),
}


def planted_rng(codec, n, oracle):
    """(frames [n, 18] all-voiced, state [n, 3], records [n]): stream s is RNG_CASES[s % 6]; every record carries a value of its own in
    every field, the reserved word included"""
    gen = framegen.rng_for(0x1EA7A000 + codec)
    warm_frames = frames_of(codec, "V" * n, gen, oracle)
    frames = frames_of(codec, "V" * n, gen, oracle)
    cold = init_state(n)
    warm = oracle.process_batch(codec, n, 1, warm_frames, cold, rng_default(n))["state"]
    state = cold.copy()
    records = np.zeros(n, dtype=RNG_DTYPE)
    for s in range(n):
        is_cold, muted, seeded, pending, _ = list(RNG_CASES.values())[s % len(RNG_CASES)]
        state[s] = cold[s] if is_cold else warm[s]
        if muted:
            state[s]["errorRate"] = 0.2   # 0.95 x 0.2 is far above the muting threshold
        records[s] = (0x123456789ABC + 0x10001 * s, seeded, 777 + s, pending, RESERVED)
    return frames, state, records


def run_planted_rng(form, oracle):
    """one T = 1 launch over planted rng records: the record behind the frame is the oracle's in every field the ABI defines, the
    reserved word is as planted, and -- on the oracle's word -- exactly the fields of RNG_CASES changed"""
    import parity
    from mbelib_neo_amd import _native

    n = form.n
    frames, state, records = planted_rng(form.codec, n, oracle)
    ref = oracle.process_batch(form.codec, n, 1, frames, state, records)
    fields = ("cn_seed48", "cn_seeded", "unvoiced_seed_state", "unvoiced_seed_override")
    for s in range(n):
        name, (_, muted, _, _, changes) = list(RNG_CASES.items())[s % len(RNG_CASES)]
        assert bool(ref["results"]["flags"][s] & FLAG_MUTE) == muted, (s, name)
        assert tuple(f for f in fields if ref["rng"][s][f] != records[s][f]) == changes, (s, name, records[s], ref["rng"][s])
    dec = _decoder(form, state, records)
    out = dec.decode(frames, 1, want_float=True)
    _ran(form, _native.lib(), "planted rng records")
    got_state, got_rng = ssc._snapshot(dec)
    for f in fields:
        bad = np.flatnonzero(got_rng[f] != ref["rng"][f])
        assert bad.size == 0, f"{form.kernel}: rng field {f} of streams {bad[:8]}: {got_rng[f][bad[:4]]} for the oracle's {ref['rng'][f][bad[:4]]}"
    assert (got_rng["reserved"] == RESERVED).all(), "the reserved word of a record was written"
    res1, pcm1, pcmf1 = ssc._outputs(out, n, 1)
    parity.check_results(ref["results"], res1.reshape(-1), f"{form.kernel}: results")
    parity.check_pcm(ref["pcmf"], pcmf1.reshape(-1, 160), ref["pcm16"], pcm1.reshape(-1, 160), what=f"{form.kernel}: pcm", peak=ref["peak"])
    parity.check_state(ref["state"], got_state, what=f"{form.kernel}: state")


# ---- a form in a fresh process (launch switches are read once per process) ------------------------
def run_form(name, oracle):
    form = FORMS[name]
    frames, state, records = scripted(form.codec, form.n, oracle)
    assert_cases(form.codec, form.n, trace(form.codec, oracle, frames, state, records))
    run_history(form, frames, state, records, oracle)
    run_planted_prev(form, oracle)
    run_planted_rng(form, oracle)


def main():
    import oracle_lib
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    try:
        run_form(sys.argv[1], oracle_lib.load())
    except AssertionError as e:
        print(f"MISMATCH {sys.argv[1]}: {e}")
        return 1
    print(f"ok {sys.argv[1]}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
