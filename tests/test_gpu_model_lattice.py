"""GPU suite (-m gpu): the model lattices (tests/model_lattice.py: caller-made models, free of the codec tables) through the
single-stage entry points -- mbx_synthesize_speech, mbx_spectral_amp_enhance, mbx_adaptive_smoothing, mbx_comfort_noise,
mbx_synthesize_tone, mbx_decode_parms, one launch per (entry point, lattice) on device buffers through the C ABI -- and, a strided sample, through their
mbe_* twins of the per-frame library; and the tone streams (every tone id of both AMBE codecs) through the stream-stage launch forms.

The checker is the ORACLE (oracle/mbx_oracle.c), no fixture.  Integers and decisions are exact: Vl, L, K, thresholds, counters, tone
phases, the noise state, the whole RNG struct, return codes, prev.PSIl after the synthesis (the wrap is exact), muted frames (an
integer generator), and every byte behind an invalid L.  Floats are held to the unchanged bounds of tests/parity.py, PER GROUP of at
most 256 structs of one class, never over a whole lattice: one wrong struct must not be diluted, and a quiet class must not hide
behind a loud one.  Every class lies inside the domain include/mbx.h states for its entry point -- the fundamentals outside
the codec tables' span that the `weights` lattice carries included: they meet the same bounds.  The figures of every group go out on one
LATTICE line per test, before anything is asserted."""
import os
import time

import numpy as np
import pytest

import model_lattice
import parity
from mbelib_neo_amd.layout import EXACT_FLOAT_FIELDS, FLOAT_FIELDS, INT_FIELDS, PARMS_DTYPE, RNG_DTYPE, rng_seeded

pytestmark = pytest.mark.gpu
CASES = [(entry, name) for entry, names in model_lattice.ENTRIES.items() for name in names]


@pytest.fixture(scope="module")
def device():
    import mbelib_neo_amd as m

    m.lib()   # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)


def _up(arr):
    import torch

    return torch.from_numpy(np.ascontiguousarray(arr).reshape(-1).view(np.uint8).copy()).cuda()


def _down(t, dtype):
    return t.cpu().numpy().view(dtype)


def _run(entry, name):
    """one launch of `entry` on lattice `name` (the tone entries: two, the second on the structs the first left); what it returned"""
    import torch

    from mbelib_neo_amd import _native

    L = _native.lib()
    lat = model_lattice.build(name)
    n = lat.cur.shape[0]
    strm = torch.cuda.current_stream().cuda_stream
    cur, prev, rng = _up(lat.cur), _up(lat.prev), _up(lat.rng)
    pcmf = torch.full((n, 160), 7.0, dtype=torch.float32, device="cuda")
    pcm16 = torch.full((n, 160), 7, dtype=torch.int16, device="cuda")
    out = {}
    if entry == "speech":
        _native.check(L.mbx_synthesize_speech(n, cur.data_ptr(), prev.data_ptr(), rng.data_ptr(), pcmf.data_ptr(), pcm16.data_ptr(), strm), entry)
    elif entry == "smoothing":
        _native.check(L.mbx_adaptive_smoothing(n, cur.data_ptr(), prev.data_ptr(), strm), entry)
    elif entry == "enhance":
        _native.check(L.mbx_spectral_amp_enhance(n, cur.data_ptr(), strm), entry)
    elif entry == "noise":
        _native.check(L.mbx_comfort_noise(n, rng.data_ptr(), pcmf.data_ptr(), pcm16.data_ptr(), strm), entry)
    elif entry in ("tone", "tone_dstar"):
        rec = _up(model_lattice.records(name)) if entry == "tone" else None
        ids = _up(lat.extra["ids"].astype(np.int32)) if entry == "tone_dstar" else None
        calls = []
        for _ in range(2):
            pcmf.fill_(7.0)
            _native.check(L.mbx_synthesize_tone(n, rec.data_ptr() if rec is not None else None, ids.data_ptr() if ids is not None else None,
                                                cur.data_ptr(), pcmf.data_ptr(), pcm16.data_ptr(), strm), entry)
            torch.cuda.synchronize()
            calls.append((pcmf.cpu().numpy(), pcm16.cpu().numpy(), _down(cur, PARMS_DTYPE)))
        return {"calls": calls}
    else:
        assert entry == "decode_parms"
        rec = _up(model_lattice.records(name))
        rc = torch.full((n,), -99, dtype=torch.int32, device="cuda")
        _native.check(L.mbx_decode_parms(lat.extra["codec"], rec.data_ptr(), n, cur.data_ptr(), prev.data_ptr(), rc.data_ptr(), strm), entry)
        out["rc"] = rc.cpu().numpy()
    torch.cuda.synchronize()
    out.update(cur=_down(cur, PARMS_DTYPE), prev=_down(prev, PARMS_DTYPE), rng=_down(rng, RNG_DTYPE), pcmf=pcmf.cpu().numpy(), pcm16=pcm16.cpu().numpy())
    return out


def _first(lat, idx, bad):
    s = int(idx[np.flatnonzero(bad)[0]])
    return f"{int(bad.sum())} structs, first: {lat.text[s]}"


def _exact_fields(lat, idx, ref, got, what, fields=INT_FIELDS + EXACT_FLOAT_FIELDS):
    """integers, decisions and the integer-valued noise state of a group, bit for bit; the failure prints the struct's line"""
    for f in fields:
        a, b = ref[f][idx], got[f][idx]
        a, b = (a.view(np.uint32), b.view(np.uint32)) if a.dtype == np.float32 else (a, b)
        bad = (a != b).reshape(len(idx), -1).any(axis=1)
        assert not bad.any(), f"{what}: {f} differs in {_first(lat, idx, bad)}"


def _state(lat, cls, idx, ref, got, what, figures):
    """a group of structs against the oracle's: exact fields, then parity.check_state (the float fields' relative RMS over this group)"""
    _exact_fields(lat, idx, ref, got, what)
    for f in FLOAT_FIELDS:
        bad = (np.isnan(ref[f][idx]) != np.isnan(got[f][idx])).reshape(len(idx), -1).any(axis=1)
        assert not bad.any(), f"{what}: the NaN pattern of {f} differs in {_first(lat, idx, bad)}"
    measured = {f: parity.rel_rms(ref[f][idx], got[f][idx]) for f in FLOAT_FIELDS}
    worst = max(measured, key=measured.get)
    figures[what.split(" class ")[-1]] = (worst, float(f"{measured[worst]:.2e}"))
    try:
        parity.check_state(ref[idx], got[idx], what=what)
    except AssertionError as e:
        f = str(e).split("float field ")[-1].split(" ")[0]
        per = np.array([parity.rel_rms(ref[f][s:s + 1], got[f][s:s + 1]) for s in idx]) if f in FLOAT_FIELDS else np.zeros(len(idx))
        raise AssertionError(f"{e}; worst struct: {lat.text[int(idx[per.argmax()])]} ({per.max():.3e})") from None


def _synthesis(name, ref, got, figures):
    lat = model_lattice.build(name)
    n = lat.cur.shape[0]
    everything = np.arange(n)
    keep = model_lattice.untouched(name, "speech")
    muted = model_lattice.muted(name)
    figures["localEnergy_not_identical"] = int((ref["cur"]["localEnergy"].view(np.uint32) != got["cur"]["localEnergy"].view(np.uint32)).sum())
    # gated: silence, and every byte of cur, prev and rng as it was
    if keep.any():
        idx = np.flatnonzero(keep)
        for x, was in (("cur", lat.cur), ("prev", lat.prev), ("rng", lat.rng)):
            bad = np.array([got[x][s].tobytes() != was[s].tobytes() for s in idx])
            assert not bad.any(), f"{name}: {x} changed behind an invalid L in {_first(lat, idx, bad)}"
        assert not got["pcmf"][keep].any() and not got["pcm16"][keep].any(), f"{name}: no silence behind an invalid L"
    # the RNG struct, whole
    bad = np.array([ref["rng"][s].tobytes() != got["rng"][s].tobytes() for s in everything])
    assert not bad.any(), f"{name}: the RNG struct differs in {_first(lat, everything, bad)}"
    # muted frames: the comfort-noise generator is integer arithmetic
    if muted.any():
        idx = np.flatnonzero(muted)
        bad = (ref["pcmf"][idx].view(np.uint32) != got["pcmf"][idx].view(np.uint32)).any(axis=1) | (ref["pcm16"][idx] != got["pcm16"][idx]).any(axis=1)
        assert not bad.any(), f"{name}: a muted frame is not the oracle's bit for bit in {_first(lat, idx, bad)}"
    # prev.PSIl: the wrap into [0, 2 pi) is exact
    synth = ~keep & ~muted
    idx = np.flatnonzero(synth)
    bad = (ref["prev"]["PSIl"][idx].view(np.uint32) != got["prev"]["PSIl"][idx].view(np.uint32)).any(axis=1)
    figures["prev_PSIl_not_identical"] = int(bad.sum())
    assert not bad.any(), f"{name}: prev.PSIl is not the reference's bit for bit in {_first(lat, idx, bad)}"
    ref16 = ref["pcm16"]
    failures = []
    for g, (cls, idx) in enumerate(model_lattice.groups(name)):
        what = f"{name} class {cls} group {g}"
        total, worst, at = parity.pcm_float_stats(ref["pcmf"][idx], got["pcmf"][idx])
        st, _ = parity.int16_stats(ref["pcmf"][idx], ref16[idx], got["pcm16"][idx])
        figures[f"{cls}/{g}"] = (len(idx), float(f"{total:.2e}"), float(f"{worst:.2e}"), st["int16_max"], round(st["int16_within_1"], 5))
        try:
            _state(lat, cls, idx, ref["cur"], got["cur"], what + ": cur", figures)
            _state(lat, cls, idx, ref["prev"], got["prev"], what + ": prev", figures)
            try:
                parity.check_pcm(ref["pcmf"][idx], got["pcmf"][idx], ref16[idx], got["pcm16"][idx], what=what + ": pcm")
            except AssertionError as e:
                raise AssertionError(f"{e}; worst frame: {lat.text[int(idx[at])]}") from None
        except AssertionError as e:
            failures.append(str(e))
    return failures


def _stage(entry, name, ref, got, figures):
    """mbx_adaptive_smoothing / mbx_spectral_amp_enhance: cur against the oracle's per group; prev (smoothing) and everything behind an
    invalid L untouched"""
    lat = model_lattice.build(name)
    keep = model_lattice.untouched(name, entry)
    if keep.any():
        idx = np.flatnonzero(keep)
        bad = np.array([got["cur"][s].tobytes() != lat.cur[s].tobytes() for s in idx])
        assert not bad.any(), f"{name}: cur changed behind an invalid L in {_first(lat, idx, bad)}"
    assert got["prev"].tobytes() == lat.prev.tobytes(), f"{name} through {entry}: prev changed"
    assert got["rng"].tobytes() == lat.rng.tobytes()
    figures["localEnergy_not_identical"] = int((ref["cur"]["localEnergy"].view(np.uint32) != got["cur"]["localEnergy"].view(np.uint32)).sum())
    failures = []
    for g, (cls, idx) in enumerate(model_lattice.groups(name)):
        try:
            _state(lat, cls, idx, ref["cur"], got["cur"], f"{name} class {cls} group {g}: cur", figures)
        except AssertionError as e:
            failures.append(str(e))
    return failures


def _tones(entry, name, ref, figures):
    from mbelib_neo_amd import _native

    lat = model_lattice.build(name)
    o = model_lattice.oracle_lib.load()
    failures = []
    got = _run(entry, name)["calls"]
    for k, ((rp, rc), (gp, g16, gc)) in enumerate(zip(ref["on"], got)):
        for f in INT_FIELDS + EXACT_FLOAT_FIELDS:
            bad = (rc[f] != gc[f]).reshape(len(rc), -1).any(axis=1)
            assert not bad.any(), f"{name} call {k}: {f} differs in {_first(lat, np.arange(len(rc)), bad)}"
        r16 = o.floattoshort(rp)
        for g, (cls, idx) in enumerate(model_lattice.groups(name)):
            what = f"{name} call {k} class {cls} group {g}"
            total, worst, at = parity.pcm_float_stats(rp[idx], gp[idx])
            st, _ = parity.int16_stats(rp[idx], r16[idx], g16[idx])
            figures[f"{k}/{cls}/{g}"] = (len(idx), float(f"{total:.2e}"), float(f"{worst:.2e}"), st["int16_max"])
            try:
                if cls == "no-tone":
                    assert not gp[idx].any() and not g16[idx].any(), f"{what}: an id that is no tone is not silent"
                    assert gc[idx].tobytes() == lat.cur[idx].tobytes(), f"{what}: the struct of an id that is no tone changed"
                else:
                    parity.check_pcm(rp[idx], gp[idx], r16[idx], g16[idx], what=what)
                    parity.check_state(rc[idx], gc[idx], what=what)
            except AssertionError as e:
                failures.append(f"{e}; worst frame: {lat.text[int(idx[at])]}")
    L = _native.lib()
    assert L.mbx_set_tone_synthesis(0) == 1
    try:
        for k, (gp, g16, gc) in enumerate(_run(entry, name)["calls"]):
            assert not gp.any() and not g16.any(), f"{name}: tones off, call {k} is not silence"
            assert gc.tobytes() == lat.cur.tobytes(), f"{name}: tones off, call {k} changed a struct"
    finally:
        assert L.mbx_set_tone_synthesis(1) == 0
    return failures


def _predict(name, ref, got, figures):
    lat = model_lattice.build(name)
    n = lat.cur.shape[0]
    idx = np.arange(n)
    bad = ref["rc"] != got["rc"]
    assert not bad.any(), f"{name}: return code differs in {_first(lat, idx, bad)}: ref {ref['rc'][bad][:4]} got {got['rc'][bad][:4]}"
    assert got["rng"].tobytes() == lat.rng.tobytes()
    for x in ("cur", "prev"):
        _exact_fields(lat, idx, ref[x], got[x], f"{name}: {x}", fields=INT_FIELDS + EXACT_FLOAT_FIELDS + ("w0", "log2Ml"))
    failures = []
    for g, (cls, gi) in enumerate(model_lattice.groups(name)):
        for x in ("cur", "prev"):
            try:
                _state(lat, cls, gi, ref[x], got[x], f"{name} class {cls} group {g}: {x}", figures)
            except AssertionError as e:
                failures.append(str(e))
    return failures


@pytest.mark.parametrize("entry,name", CASES, ids=[f"{e}-{n}" for e, n in CASES])
def test_lattice_through_the_entry_point_against_the_oracle(device, entry, name):
    ref = model_lattice.oracle(name, entry)   # (made, or found, before the clock starts: CPU work)
    model_lattice.composition(name)
    t0 = time.perf_counter()
    figures, failures = {}, ["did not finish"]
    try:
        if entry in ("tone", "tone_dstar"):
            failures = _tones(entry, name, ref, figures)
        else:
            got = _run(entry, name)
            if entry == "speech":
                failures = _synthesis(name, ref, got, figures)
            elif entry == "noise":   # an integer generator: every sample and the RNG struct bit for bit, cn_seeded 0 and 1
                lat = model_lattice.build(name)
                assert set(lat.rng["cn_seeded"].tolist()) == {0, 1}
                bad = (ref["pcmf"].view(np.uint32) != got["pcmf"].view(np.uint32)).any(axis=1) | (ref["pcm16"] != got["pcm16"]).any(axis=1) | \
                    np.array([ref["rng"][s].tobytes() != got["rng"][s].tobytes() for s in range(len(lat.text))])
                assert not bad.any(), f"{name}: comfort noise differs in {_first(lat, np.arange(len(lat.text)), bad)}"
                assert got["cur"].tobytes() == lat.cur.tobytes() and got["prev"].tobytes() == lat.prev.tobytes()
                failures = []
            elif entry == "decode_parms":
                failures = _predict(name, ref, got, figures)
            else:
                failures = _stage(entry, name, ref, got, figures)
    finally:   # (the figures are taken before the comparisons assert: a failing run prints them too)
        print("LATTICE", entry, name, f"{time.perf_counter() - t0:.2f} s", figures)
    assert not failures, f"{len(failures)} group(s) outside the bounds:\n" + "\n".join(failures)


# ---- the shim: the per-frame twins return the bytes of the batched call ------------------------------------------------------------
@pytest.mark.parametrize("name", model_lattice.SYNTHESIS)
def test_shim_twins_return_the_bytes_of_the_batched_call(device, name):
    import shim_lib
    from shim_lib import p

    mbe = shim_lib.load()
    lat = model_lattice.build(name)
    n = lat.cur.shape[0]
    # the per-frame library keeps its RNG per thread, set from a seed: the structs whose RNG struct is what a seed makes
    seeds = (lat.rng["cn_seed48"] ^ np.uint64(0x5DEECE66D)).astype(np.int64)
    plain = np.array([lat.rng[s].tobytes() == rng_seeded([seeds[s]])[0].tobytes() for s in range(n)])
    pick = np.flatnonzero(plain)[np.unique(np.linspace(0, plain.sum() - 1, model_lattice.SHIM_SAMPLE).astype(np.int64))]
    assert len(pick) >= model_lattice.SHIM_SAMPLE - 1
    batched = {e: _run(e, name) for e in ("speech", "smoothing", "enhance")}
    for s in pick:
        cur, prev, out = lat.cur[s:s + 1].copy(), lat.prev[s:s + 1].copy(), np.full(160, 7.0, dtype=np.float32)
        mbe.mbe_setThreadRngSeed(int(seeds[s]))
        mbe.mbe_synthesizeSpeechf(p(out), p(cur), p(prev))
        b = batched["speech"]
        assert out.tobytes() == b["pcmf"][s].tobytes() and cur.tobytes() == b["cur"][s:s + 1].tobytes() and prev.tobytes() == b["prev"][s:s + 1].tobytes(), \
            f"mbe_synthesizeSpeechf: not the bytes of mbx_synthesize_speech for {lat.text[s]}"
        cur, prev = lat.cur[s:s + 1].copy(), lat.prev[s:s + 1].copy()
        mbe.mbe_applyAdaptiveSmoothing(p(cur), p(prev))
        b = batched["smoothing"]
        assert cur.tobytes() == b["cur"][s:s + 1].tobytes() and prev.tobytes() == lat.prev[s:s + 1].tobytes(), \
            f"mbe_applyAdaptiveSmoothing: not the bytes of mbx_adaptive_smoothing for {lat.text[s]}"
        cur = lat.cur[s:s + 1].copy()
        mbe.mbe_spectralAmpEnhance(p(cur))
        assert cur.tobytes() == batched["enhance"]["cur"][s:s + 1].tobytes(), f"mbe_spectralAmpEnhance: not the bytes of mbx_spectral_amp_enhance for {lat.text[s]}"


# ---- tones through the stream stage ------------------------------------------------------------------------------------------------
TONE_CASES = [(codec, form) for codec in model_lattice.TONE_STREAM_CODECS for form in model_lattice.TONE_STREAM_FORMS]


@pytest.mark.parametrize("codec,form", TONE_CASES, ids=[f"codec{c}-{f[0]}" for c, f in TONE_CASES])
def test_tone_streams_through_the_stream_stage(device, codec, form):
    import instance_cases
    from mbelib_neo_amd import _native

    keep = ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")
    if any(k.startswith("MBX_") and k not in keep for k in os.environ):
        pytest.skip("the suite runs under MBX_* switches: the tone streams are for the launcher's own choice of instance")
    label, entry, T, launches, fragment = form
    S = model_lattice.TONE_STREAMS
    name = _native.lib().mbx_batch_kernel_name(codec, S, T, 1 if entry == "resident" else 0).decode()
    assert fragment in name and ("_one" in name) == (T == 1) and ("_lds" in name) == (label == "lds"), f"{label}: the launcher takes {name}"
    case = instance_cases.Case(f"tones-codec{codec}-{label}", name, codec, S, T, launches, entry, {})
    workload = model_lattice.ToneStreams(codec)
    model_lattice.tone_stream_decode(codec)
    t0 = time.perf_counter()
    try:
        instance_cases.run_case(case, workload=workload)
    finally:
        print("LATTICE tone-streams", case.id, name, f"{time.perf_counter() - t0:.2f} s", workload.figures)
