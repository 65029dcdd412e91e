"""CPU suite: pins the ORACLE (oracle/mbx_oracle.c) to the reference.

Two kinds of evidence:
  * the golden values the reference's own tests hold -- FNV-1a hashes of tests/test_golden_pcm.c:78-84,
    the Golay/Hamming known answers of tests/test_ecc.c, the scalar known answers of
    tests/test_params.c, the edge values of tests/test_floattoshort_parity.c;
  * fixtures written by oracle/tools/gen_fixtures.c linked against the real reference
    (IEEE scalar build, oracle/Makefile) -- tests/golden/*.bin.
"""
import os

import numpy as np
import pytest

import golden_io
import oracle_lib
import parity
from mbelib_neo_amd.layout import PARMS_DTYPE, RESULT_DTYPE

REF_F32_HASH_SCALAR = 0x59741032  # reference tests/test_golden_pcm.c:78
REF_S16_HASH = 0x4EDB8636  # reference tests/test_golden_pcm.c:84


def test_golden_synth_hashes(oracle):
    g = golden_io.golden_synth()
    assert int(g["hash_f32"]) == REF_F32_HASH_SCALAR and int(g["hash_s16"]) == REF_S16_HASH  # fixture == reference test
    rng = oracle.rng_seeded([0xC0FFEE])
    pcmf, cur, prev, _ = oracle.synthesize_speech(g["cur_in"].reshape(1), g["prev_in"].reshape(1), rng)
    s16 = oracle.floattoshort(pcmf)
    # int16 hash is reproduced exactly; the float hash depends on PFFFT's rounding, so floats are
    # compared numerically (the oracle's FFT is double precision)
    assert oracle.fnv(s16) == REF_S16_HASH
    m = parity.check_pcm(g["pcmf"], pcmf, g["pcm16"], s16, rel=1e-6, worst=1e-5)
    assert m["int16_exact"] == 1.0
    parity.check_state(g["cur_out"].reshape(1), cur, rel=1e-6)
    parity.check_state(g["prev_out"].reshape(1), prev, rel=1e-6)
    # with the reference's own float transform restated (FFTPACK's real radix-4 passes, what PFFFT's scalar build runs) the
    # oracle IS the reference: the float hash of the reference's golden test, and every float of PCM and state bit for bit
    oracle.set_fft_float(1)
    try:
        pcmf2, cur2, prev2, _ = oracle.synthesize_speech(g["cur_in"].reshape(1), g["prev_in"].reshape(1), oracle.rng_seeded([0xC0FFEE]))
    finally:
        oracle.set_fft_float(0)
    assert oracle.fnv(pcmf2.astype(np.float32)) == REF_F32_HASH_SCALAR
    assert pcmf2.tobytes() == np.asarray(g["pcmf"], dtype=np.float32).tobytes()
    assert cur2.tobytes() == g["cur_out"].reshape(1).tobytes() and prev2.tobytes() == g["prev_out"].reshape(1).tobytes()


def test_ecc_known_answers(oracle):
    golay, ham = golden_io.ecc_kat()
    for r in golay:
        out, errs = oracle.golay(int(r["inp"]))
        assert (out, errs) == (int(r["out"]), int(r["errs"]))
    # reference tests/test_ecc.c:356-375: data 0xA55 with bit 5 flipped decodes back to 0xA55
    last = golay[-1]
    assert (int(last["out"]) >> 11) == 0xA55 and int(last["errs"]) == 1
    for r in ham[::7]:  # every 7th of the exhaustive 32768 (the HIP test runs all of them)
        out, errs = oracle.hamming(int(r["inp"]))
        assert (out, errs) == (int(r["out"]), int(r["errs"]))


@pytest.mark.parametrize("codec", [0, 1])
def test_fec_fixtures(oracle, codec):
    fx = golden_io.fec(codec)
    rcs, packed = oracle.pack(codec, fx["cells"])
    assert all(rc == 0 for rc in rcs)
    rec = oracle.fec_batch(codec, packed)
    nbits = 88 if codec == 0 else 49
    assert np.array_equal(oracle_lib.records_to_bits(rec, nbits), fx["bits"])
    res = oracle_lib.records_to_results(rec)
    parity.check_results(fx["result"], res)
    assert np.array_equal(res["total_errors"], fx["ret"])


@pytest.mark.parametrize("codec", [0, 1])
def test_invalid_bits_rejected(oracle, codec):
    # reference tests/test_input_validation.c:72-122: any cell outside {0,1} -> -2, NULL -> -1
    ncell = 184 if codec == 0 else 96
    cells = np.zeros((1, ncell), dtype=np.int8)
    cells[0, ncell - 1] = 2  # even an unused cell is validated
    rcs, _ = oracle.pack(codec, cells)
    assert rcs == [-2]
    fn = oracle.h.mbxo_pack_imbe_frame if codec == 0 else oracle.h.mbxo_pack_ambe_frame
    assert fn(None, None) == -1


@pytest.mark.parametrize("codec", [0, 1])
def test_stream_fixtures(oracle, codec):
    S, T, fx = golden_io.stream(codec)
    frames = fx["frames"]
    _, packed = oracle.pack(codec, frames["cells"].reshape(S * T, -1))
    out = oracle.process_batch(codec, S, T, packed, oracle.init_state(S), oracle.rng_seeded([1234 + s for s in range(S)]))
    nbits = 88 if codec == 0 else 49
    assert np.array_equal(oracle_lib.records_to_bits(out["records"], nbits), frames["bits"].reshape(S * T, nbits))
    parity.check_results(frames["result"].reshape(-1), out["results"])
    assert np.array_equal(out["results"]["total_errors"], frames["ret"].reshape(-1))
    m = parity.check_pcm(frames["pcmf"], out["pcmf"], frames["pcm16"], out["pcm16"], rel=1e-6, worst=1e-5)
    assert m["int16_max"] <= 1
    parity.check_state(fx["final"], out["state"], rel=1e-6)
    flags = frames["result"]["flags"].reshape(-1)
    if codec == 0:
        assert (flags & 0x40).any() and (flags & 0x80).any()  # repeat and mute are covered
    else:
        assert (flags & 0x20).any() and (flags & 0x10).any() and (flags & 0x40).any()  # erasure, tone, repeat
    # ... and with the reference's float transform restated (oracle.set_fft_float) NOTHING differs: every float of the PCM and of
    # the final state of all 64 golden streams is the real reference's, bit for bit (fixtures written by oracle/_ref)
    oracle.set_fft_float(1)
    try:
        exact = oracle.process_batch(codec, S, T, packed, oracle.init_state(S), oracle.rng_seeded([1234 + s for s in range(S)]))
    finally:
        oracle.set_fft_float(0)
    assert np.asarray(exact["pcmf"], dtype=np.float32).tobytes() == np.ascontiguousarray(frames["pcmf"], dtype=np.float32).tobytes()
    assert np.array_equal(np.asarray(exact["pcm16"]).reshape(-1), np.asarray(frames["pcm16"]).reshape(-1))
    assert np.asarray(exact["state"]).tobytes() == np.ascontiguousarray(fx["final"]).tobytes()


def test_synth_sequences(oracle):
    # the reference's bench recipes as multi-frame known answers (bench/bench_synth.c:40-67,
    # bench/bench_unvoiced.c:33-52,87)
    frames, fx = golden_io.synth_seq()
    for recipe in range(2):
        cur = np.zeros(1, dtype=PARMS_DTYPE)
        st = oracle.init_state(1)
        cur[0] = st[0, 0]
        l = np.arange(57)
        if recipe == 0:
            rng = oracle.rng_seeded([0x123456])
            cur["w0"] = np.float32(0.09378)
            cur["L"] = 40
            for k in range(1, 41):
                cur["Vl"][0, k] = int((k % 3) != 0)
                cur["Ml"][0, k] = np.float32(0.05) + np.float32(0.002) * np.float32(k)
                cur["log2Ml"][0, k] = 0.0
                cur["PHIl"][0, k] = np.float32(k) * np.float32(0.1)
                cur["PSIl"][0, k] = np.float32(k) * np.float32(0.05)
        else:
            rng = oracle.rng_seeded([0xBEEF])
            cur["w0"] = np.float32(0.11)
            cur["L"] = 36
            for k in range(1, 37):
                cur["Vl"][0, k] = 0
                cur["Ml"][0, k] = np.float32(0.03) + np.float32(0.002) * np.float32(k & 7)
                cur["PHIl"][0, k] = 0.0
                cur["PSIl"][0, k] = 0.0
        prev = cur.copy()
        got = []
        for i in range(frames):
            if recipe == 0:
                cur["w0"] = np.float32(0.09) if (i & 1) else np.float32(0.11)
                for k in range(1, 41):
                    cur["Vl"][0, k] = 1 if ((i + k) % 5) else 0
                    cur["Ml"][0, k] = np.float32(0.04) + np.float32(0.003) * np.float32((i + k) % 7)
            else:
                cur["w0"] = np.float32(0.10) if (i & 1) else np.float32(0.12)
            pcmf, cur, prev, rng = oracle.synthesize_speech(cur, prev, rng)
            prev = cur.copy()
            got.append(pcmf[0])
        parity.check_pcm(fx[recipe]["pcmf"], np.array(got), rel=1e-6, worst=1e-5, what=f"recipe{recipe}")
        parity.check_state(fx[recipe]["cur"].reshape(1), cur, rel=1e-6)


def test_floattoshort_exact(oracle):
    fx = golden_io.f2s()  # inputs of reference tests/test_floattoshort_parity.c:36-68
    for case in fx:
        assert np.array_equal(oracle.floattoshort(case["inp"])[0], case["out"])
    # the reference test's own scalar model: NaN -> 0, +-Inf -> +-31128, clip at 31128.65
    edge = np.zeros(160, dtype=np.float32)
    edge[:3] = [np.nan, np.inf, -np.inf]
    assert list(oracle.floattoshort(edge)[0][:3]) == [0, 31128, -31128]


def test_parameter_known_answers(oracle):
    t_imbe, t_ambe, full_imbe, full_ambe = golden_io.params_kat()
    h = oracle.h
    for b0 in range(256):
        d = np.zeros(88, dtype=np.int8)
        for i in range(8):
            d[i if i < 6 else (85 if i == 6 else 86)] = (b0 >> (7 - i)) & 1
        st = oracle.init_state(1)
        rc = h.mbxo_decode_imbe4400_parms(d.ctypes.data, st[0, 0:1].ctypes.data, st[0, 1:2].ctypes.data)
        r = t_imbe[b0]
        assert rc == r["rc"]
        if rc == 0:
            assert st[0, 0]["w0"] == r["w0"] and st[0, 0]["L"] == r["L"] and st[0, 0]["K"] == r["K"]
    # reference tests/test_params.c:227-253 spot values
    import math
    for b0 in (0, 100, 206):
        w0 = np.float32((4.0 * math.pi) / (b0 + 39.5))
        L = int(0.9254 * int((math.pi / float(w0)) + 0.25))
        assert abs(float(t_imbe[b0]["w0"]) - float(w0)) <= 1e-6 and t_imbe[b0]["L"] == L
        assert t_imbe[b0]["K"] == ((L + 2) // 3 if L < 37 else 12)
    for b0 in range(128):
        d = np.zeros(49, dtype=np.int8)
        for k, i in enumerate((0, 1, 2, 3, 37, 38, 39)):
            d[i] = (b0 >> (6 - k)) & 1
        st = oracle.init_state(1)
        rc = h.mbxo_decode_ambe2450_parms(d.ctypes.data, st[0, 0:1].ctypes.data, st[0, 1:2].ctypes.data, -1)
        r = t_ambe[b0]
        assert rc == r["rc"], b0
        if rc == 0:
            assert st[0, 0]["w0"] == r["w0"] and st[0, 0]["L"] == r["L"]
    # reference tests/test_params.c:303-341: AMBE b0 0 -> L 9, 119 -> L 56, silence 124/125 -> L 15/14
    assert t_ambe[0]["L"] == 9 and t_ambe[119]["L"] == 56 and t_ambe[124]["L"] == 15 and t_ambe[125]["L"] == 14
    for codec, fx in ((0, full_imbe), (1, full_ambe)):
        for r in fx:
            st = oracle.init_state(1)
            l = np.arange(57)
            st[0, 1]["log2Ml"] = (np.float32(0.25) * ((l * 7) % 11).astype(np.float32) - np.float32(1.0)).astype(np.float32)
            st[0, 1]["Ml"] = np.exp2(st[0, 1]["log2Ml"].astype(np.float32)).astype(np.float32)
            st[0, 1]["L"] = r["prev_L"]
            st[0, 1]["gamma"] = 1.5
            bits = np.ascontiguousarray(r["bits"])
            if codec == 0:
                rc = h.mbxo_decode_imbe4400_parms(bits.ctypes.data, st[0, 0:1].ctypes.data, st[0, 1:2].ctypes.data)
            else:
                rc = h.mbxo_decode_ambe2450_parms(bits.ctypes.data, st[0, 0:1].ctypes.data, st[0, 1:2].ctypes.data, -1)
            assert rc == r["rc"]
            if rc == 0:
                parity.check_state(r["cur"].reshape(1), st[0, 0:1], rel=2e-7)


def test_misc_known_answers(oracle):
    fx = golden_io.misc_kat()
    h = oracle.h
    # reference tests/test_params.c:573-594: Tm is not clamped, -2999 scales Ml negative
    assert int(fx["tm"]) == -2999
    st = oracle.init_state(1)
    cur, prev = st[0, 0:1], st[0, 1:2]
    cur["L"] = 4
    cur["Ml"][0, 1:5] = 10.0
    cur["Vl"][0, 1:5] = 0
    cur["errorRate"] = 0.5
    cur["errorCountTotal"] = 30
    cur["errorCount4"] = 2
    prev["amplitudeThreshold"] = 1
    h.mbxo_adaptive_smoothing(cur.ctypes.data, prev.ctypes.data)
    assert int(cur["amplitudeThreshold"][0]) == -2999 and cur["Ml"][0, 1] == fx["ml1"] and cur["Ml"][0, 1] < 0
    assert cur["localEnergy"][0] == fx["local_energy"]
    # reference tests/test_params.c:596-618: seeded comfort noise; cold-start seed = 0x1234 % 53125
    rng = oracle.rng_seeded([0x12345678])
    noise = np.zeros(160, dtype=np.float32)
    h.mbxo_comfort_noisef(noise.ctypes.data, rng.ctypes.data)
    assert np.array_equal(noise, fx["comfort"])
    assert float(fx["cold_seed"]) == float(0x1234 % 53125)
    # reference tests/test_params.c:717-740: repeat headroom reset -> default model, L = 39
    st = oracle.init_state(1)
    st[0, 1]["repeatCount"] = 4
    st[0, 0] = st[0, 1]
    res = np.zeros(1, dtype=RESULT_DTYPE)
    res["total_errors"] = 6
    out = np.zeros(160, dtype=np.float32)
    d = np.zeros(88, dtype=np.int8)
    rng = oracle.rng_seeded([77])
    rc = h.mbxo_process_imbe4400_dataf(out.ctypes.data, res.ctypes.data, d.ctypes.data, st[0, 0:1].ctypes.data,
                                       st[0, 1:2].ctypes.data, st[0, 2:3].ctypes.data, rng.ctypes.data)
    assert rc == int(fx["hr_rc"]) and int(st[0, 0]["L"]) == 39 and int(st[0, 0]["repeatCount"]) == 0
    parity.check_results(fx["hr_result"].reshape(1), res)
    parity.check_state(fx["hr_cur"].reshape(1), st[0, 0:1], rel=1e-6)
    parity.check_pcm(fx["hr_pcm"], out, rel=1e-6, worst=1e-5)


# ---- soft-decision front end against the real reference's outputs -------
def test_soft_golay_hamming_match_reference(oracle):
    kat = golden_io.soft_kat()
    for row in kat["golay"]:
        out, ret = oracle.golay_soft(row["soft"])
        assert ret == row["ret"] and np.array_equal(out, row["out"])
    for row in kat["hamming"]:
        out, ret = oracle.hamming_soft(row["soft"])
        assert ret == row["ret"] and np.array_equal(out, row["out"])


@pytest.mark.parametrize("codec", [0, 1])
def test_soft_frames_match_reference(oracle, codec):
    kat = golden_io.soft_kat()["imbe" if codec == 0 else "ambe"]
    for row in kat:
        bits, ret, res = oracle.decode_soft_frame(codec, row["soft"])
        assert ret == row["ret"]
        assert np.array_equal(bits, row["bits"])
        for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
            assert res[name] == row["result"][name], name
    # the batch driver used by the GPU tests agrees with the per-frame entry
    rec = oracle.fec_soft_batch(codec, kat["soft"])
    nbits = 88 if codec == 0 else 49
    assert np.array_equal(oracle_lib.records_to_bits(rec, nbits), kat["bits"])


def test_soft_bits_from_llr(oracle):
    kat = golden_io.soft_kat()["llr"]
    assert np.array_equal(oracle.soft_from_llr(kat["llr"]), kat["soft"])


# ---- IMBE 7100x4400 front end against the real reference's outputs -------
def test_imbe7100_hamming_and_convert_match_reference(oracle):
    kat = golden_io.imbe7100_kat()
    for row in kat["hamming"][::7]:
        out, errs = oracle.hamming7100(row["inp"])
        assert out == row["out"] and errs == row["errs"]
    for row in kat["convert"]:
        assert np.array_equal(oracle.convert7100(row["inp"]), row["out"])


def test_imbe7100_frames_match_reference(oracle):
    kat = golden_io.imbe7100_kat()
    for row in kat["fec"]:
        bits, ret, res = oracle.decode_imbe7100_frame(row["cells"])
        assert ret == row["ret"]
        assert np.array_equal(bits, row["bits"])
        for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
            assert res[name] == row["result"][name], name
    rcs, packed = oracle.pack(2, kat["fec"]["cells"])
    assert all(rc == 0 for rc in rcs)
    rec = oracle.fec_batch(2, packed)
    assert np.array_equal(oracle_lib.records_to_bits(rec, 88), kat["fec"]["bits"])


def test_imbe7100_stream_matches_reference(oracle):
    st = golden_io.imbe7100_kat()["stream"]
    S, T = st.shape[0], st["frames"].shape[1]
    cells = st["frames"]["cells"].reshape(S * T, 168)
    rcs, packed = oracle.pack(2, cells)
    assert all(rc == 0 for rc in rcs)
    out = oracle.process_batch(2, S, T, packed, oracle.init_state(S), oracle.rng_seeded([1234 + s for s in range(S)]))
    ref = st["frames"].reshape(-1)
    parity.check_results(ref["result"], out["results"])
    parity.check_pcm(ref["pcmf"], out["pcmf"], rel=2e-6, worst=2e-5)
    parity.check_state(st["final"], out["state"][:, 0])


def test_imbe7100_soft_matches_reference(oracle):
    kat = golden_io.imbe7100_kat()
    for row in kat["hamming_soft"]:
        out, ret = oracle.hamming_soft(row["soft"], variant7100=True)
        assert ret == row["ret"] and np.array_equal(out, row["out"])
    for row in kat["fec_soft"]:
        bits, ret, res = oracle.decode_soft_frame(2, row["soft"])
        assert ret == row["ret"]
        assert np.array_equal(bits, row["bits"])
        for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
            assert res[name] == row["result"][name], name
    rec = oracle.fec_soft_batch(2, kat["fec_soft"]["soft"])
    assert np.array_equal(oracle_lib.records_to_bits(rec, 88), kat["fec_soft"]["bits"])


# ---- AMBE 3600x2400 / D-STAR against the real reference's outputs ----------
def test_ambe2400_frame_streams_match_reference(oracle):
    framed, _ = golden_io.ambe2400_kat()
    S, T = framed.shape[0], framed["frames"].shape[1]
    rcs, packed = oracle.pack(3, framed["frames"]["cells"].reshape(S * T, 96))
    assert all(rc == 0 for rc in rcs)
    out = oracle.process_batch(3, S, T, packed, oracle.init_state(S), oracle.rng_seeded([1234 + s for s in range(S)]))
    ref = framed["frames"].reshape(-1)
    assert np.array_equal(oracle_lib.records_to_bits(out["records"], 49), ref["bits"])
    parity.check_results(ref["result"], out["results"])
    parity.check_pcm(ref["pcmf"], out["pcmf"], rel=2e-6, worst=2e-5)
    parity.check_state(framed["final"], out["state"])


def test_ambe2400_scripted_data_streams_match_reference(oracle):
    """voice, valid D-STAR tones, silence / invalid tone classes and error-count driven repeats"""
    _, data = golden_io.ambe2400_kat()
    seen = set()
    for s, stream in enumerate(data):
        state = oracle.init_state(1)[0]
        rng = oracle.rng_seeded([5000 + s])
        pcm = np.zeros((len(stream["frames"]), 160), dtype=np.float32)
        for t, fr in enumerate(stream["frames"]):
            pcm[t], ret, res = oracle.process_ambe2400_data(fr["bits"], fr["total_in"], state, rng)
            assert ret == fr["ret"]
            for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
                assert res[name] == fr["result"][name], (s, t, name)
            seen.add(int(res["flags"]))
        parity.check_pcm(stream["frames"]["pcmf"], pcm, rel=2e-6, worst=2e-5)
        parity.check_state(stream["final"].reshape(1, 3), state.reshape(1, 3))
    assert any(f & 0x10 for f in seen) and any(f & 0x40 for f in seen)   # tone class and repeats both occurred


def test_tone_frames_match_reference(oracle):
    """mbe_synthesizeTonef / mbe_synthesizeTonefdstar with their phase continuity across frames"""
    ambe, dstar = golden_io.tone_kat()
    cur = oracle.init_state(1)[0, 0:1].copy()
    for row in ambe:
        pcm = np.zeros(160, dtype=np.float32)
        bits = np.ascontiguousarray(row["bits"])
        oracle.h.mbxo_tonef(pcm.ctypes.data, bits.ctypes.data, cur.ctypes.data)
        assert np.array_equal(pcm, row["pcmf"])
        assert int(cur["swn"][0]) == row["swn"] and int(cur["tonePhase"][0]) == row["tonePhase"]
    cur = oracle.init_state(1)[0, 0:1].copy()
    for row in dstar:
        pcm = np.zeros(160, dtype=np.float32)
        oracle.h.mbxo_tone_dstarf(pcm.ctypes.data, cur.ctypes.data, int(row["id"]))
        assert np.array_equal(pcm, row["pcmf"])
        assert int(cur["swn"][0]) == row["swn"] and int(cur["tonePhase"][0]) == row["tonePhase"]


def test_notones_option_matches_the_reference_built_with_it(oracle):
    """The reference's NOTONES build option (-DDISABLE_AMBE_TONES, ref CMakeLists.txt:330-337): tone frames are silence and the tone
    phases stay (ref src/core/mbelib.c:747-751, 815-819).  tests/golden/notones_kat.bin was written by the reference built that way
    (oracle/Makefile `notones`); the restatement with set_tones(0) must reproduce it: the tone entry points, and scripted data-level
    streams of both AMBE codecs (voice, verified / unverified / invalid tones, error-count driven repeats) with results, PCM and
    final state.  And the ordinary fixture (tone_kat.bin) must NOT be silent, or the option would prove nothing."""
    ambe, dstar, plus2, dst = golden_io.notones_kat()
    loud, _ = golden_io.tone_kat()
    assert np.any(loud["pcmf"] != 0.0) and not np.any(ambe["pcmf"] != 0.0) and not np.any(dstar["pcmf"] != 0.0)
    oracle.set_tones(0)
    try:
        cur = oracle.init_state(1)[0, 0:1].copy()
        for row in ambe:
            pcm = np.ones(160, dtype=np.float32)
            bits = np.ascontiguousarray(row["bits"])
            oracle.h.mbxo_tonef(pcm.ctypes.data, bits.ctypes.data, cur.ctypes.data)
            assert not pcm.any() and int(cur["swn"][0]) == row["swn"] and int(cur["tonePhase"][0]) == row["tonePhase"]
        for row in dstar:
            pcm = np.ones(160, dtype=np.float32)
            oracle.h.mbxo_tone_dstarf(pcm.ctypes.data, cur.ctypes.data, int(row["id"]))
            assert not pcm.any() and int(cur["swn"][0]) == row["swn"] and int(cur["tonePhase"][0]) == row["tonePhase"]
        for data, seed0, is_plus2 in ((plus2, 7000, True), (dst, 8000, False)):
            tones = 0
            for s, stream in enumerate(data):
                state = oracle.init_state(1)[0]
                rng = oracle.rng_seeded([seed0 + s])
                pcm = np.zeros((len(stream["frames"]), 160), dtype=np.float32)
                for t, fr in enumerate(stream["frames"]):
                    pcm[t], ret, res = oracle.process_ambe2400_data(fr["bits"], fr["total_in"], state, rng, plus2=is_plus2)
                    assert ret == fr["ret"]
                    for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
                        assert res[name] == fr["result"][name], (is_plus2, s, t, name)
                    tones += bool(res["flags"] & 0x10)
                parity.check_pcm(stream["frames"]["pcmf"], pcm, rel=2e-6, worst=2e-5)
                parity.check_state(stream["final"].reshape(1, 3), state.reshape(1, 3))
            assert tones >= 40
    finally:
        oracle.set_tones(1)


def test_tail_cases_fixture_is_pinned_and_shows_the_references_own_spread(oracle, golden_dir):
    """tests/golden/tail_cases.npz (oracle/tools/gen_tail_fixture.py): the frames with the largest HIP-vs-oracle int16
    differences found in 94 M samples.  Here, without a GPU: the oracle reproduces the REFERENCE's IEEE build on them
    (within the 1 LSB its double-precision FFT allows), every one of them is a clipped frame, and the reference's own build
    for an FMA target differs from its IEEE build by MORE than the HIP path differed from the oracle -- the evidence behind
    the 6-LSB bound of parity.py for clipped frames."""
    import parity

    fx = np.load(os.path.join(golden_dir, "tail_cases.npz"))
    n = int(fx["n"])
    assert n >= 8
    worst_hip = 0
    for k in range(n):
        codec, t, seed, diff = (int(x) for x in fx[f"c{k}_meta"])
        frames = fx[f"c{k}_frames"]
        out = oracle.process_batch(codec, 1, t + 1, frames.reshape(t + 1, -1), oracle.init_state(1), oracle.rng_seeded([seed]))
        o16 = np.asarray(out["pcm16"]).reshape(t + 1, 160)[t].astype(np.int32)
        assert np.array_equal(o16, fx[f"c{k}_oracle"].astype(np.int32))
        ieee, fma, hip = (fx[f"c{k}_{name}"].astype(np.int32) for name in ("ref_ieee", "ref_fma", "hip"))
        assert np.abs(o16 - ieee).max() <= 1
        assert parity.clipped_frames(np.asarray(out["pcmf"]).reshape(t + 1, 160)[t])[0]
        d_hip, d_ref = int(np.abs(hip - o16).max()), int(np.abs(fma - ieee).max())
        assert d_hip == diff and d_hip <= parity.INT16_MAX_LSB_CLIPPED
        assert d_ref >= d_hip, (k, d_ref, d_hip)
        worst_hip = max(worst_hip, d_hip)
    assert worst_hip >= 3   # the fixture really holds the tail
    for codec in range(4):   # the histograms the cases were drawn from: >= 31 M samples per codec, nothing beyond 4 LSB
        h = fx[f"hist{codec}"]
        assert h.sum() >= 30_000_000 and h[5:].sum() == 0 and h[:2].sum() / h.sum() >= 0.99999


def _same_bytes(a, b, what):
    for k in a:
        assert a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes(), (what, k)


@pytest.mark.parametrize("fft_float", [0, 1])
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_threaded_batch_gives_the_bytes_of_the_single_thread(oracle, codec, fft_float):
    """Oracle.process_batch splits a batch into contiguous ranges of streams on a thread pool (the GPU suite compares every
    stream of its full-shape launches with it).  1,000 random-bit streams x 6 frames -- every error bucket, repeats, mutes,
    tone and erasure frames -- decoded on one thread and on seven (ranges of 142 and 143 streams): every returned array,
    the pre-clip peaks included, is the same bytes, for every codec and both FFT forms."""
    from mbelib_neo_amd import framegen

    S, T = 1000, 6
    frames = framegen.random_frames(codec, S * T, framegen.rng_for(900 + codec))
    state, rng = oracle.init_state(S), oracle.rng_seeded(np.arange(S) * 7 + 1)
    oracle.set_fft_float(fft_float)
    try:
        one = oracle.process_batch(codec, S, T, frames, state, rng, threads=1)
        seven = oracle.process_batch(codec, S, T, frames, state, rng, threads=7)
    finally:
        oracle.set_fft_float(0)
    assert one["peak"].max() > 0 and len(np.unique(one["results"]["flags"])) > 1   # the workload is not a trivial one
    _same_bytes(one, seven, (codec, fft_float, "threads=7"))


def test_default_stays_on_one_thread_for_the_batches_the_benchmark_times(oracle, monkeypatch):
    """bench.py's cpu_baseline leg times Oracle.process_batch without a `threads` argument and reports it as one core: 4,096 x 1
    (512 x 1 soft), 256 x 16 ... 64 x 128 = at most 8,192 frames.  For those the default is ONE thread, whatever the host has --
    in the function that decides and in the calls that are made; the full-shape comparisons (>= 262,144 frames) get the pool."""
    import concurrent.futures

    from mbelib_neo_amd import framegen

    monkeypatch.setattr(os, "sched_getaffinity", lambda pid: set(range(64)))
    shapes = [(4096 if T == 1 else max(64, 4096 // T), T) for T in (1, 2, 4, 16, 40, 128)] + [(512, 1)]
    for S, T in shapes:
        assert oracle_lib.default_threads(S * T) == 1, (S, T)
    assert oracle_lib.default_threads(65536 * 4) == oracle_lib.MAX_THREADS and oracle_lib.default_threads(8192 * 128) == oracle_lib.MAX_THREADS

    def no_pool(*a, **k):
        raise AssertionError("a thread pool for a batch the benchmark times as one core")

    monkeypatch.setattr(oracle_lib, "ThreadPoolExecutor", no_pool)
    assert concurrent.futures.ThreadPoolExecutor is not no_pool
    for codec, S, T in ((0, 4096, 1), (0, 256, 16), (1, 64, 128)):
        frames = framegen.random_frames(codec, S * T, framegen.rng_for(960 + T))
        oracle.process_batch(codec, S, T, frames, oracle.init_state(S), oracle.rng_seeded(np.arange(S) + 1234))


def test_default_thread_count_of_a_large_batch_gives_the_bytes_of_the_single_thread(oracle):
    from mbelib_neo_amd import framegen

    S, T = 2000, 10   # above SMALL_BATCH_FRAMES: the default is the pool
    assert oracle_lib.default_threads(S * T) == min(len(os.sched_getaffinity(0)), oracle_lib.MAX_THREADS)
    frames = framegen.random_frames(1, S * T, framegen.rng_for(970))
    state, rng = oracle.init_state(S), oracle.rng_seeded(np.arange(S) + 3)
    _same_bytes(oracle.process_batch(1, S, T, frames, state, rng, threads=1), oracle.process_batch(1, S, T, frames, state, rng), "threads=None")


def test_threaded_soft_batch_gives_the_bytes_of_the_single_thread(oracle):
    from mbelib_neo_amd import framegen

    S, T = 1000, 6
    soft = framegen.soft_frames(0, S * T, framegen.rng_for(950))
    state, rng = oracle.init_state(S), oracle.rng_seeded(np.arange(S) + 77)
    one = oracle.process_batch(0, S, T, soft, state, rng, soft=True, threads=1)
    seven = oracle.process_batch(0, S, T, soft, state, rng, soft=True, threads=7)
    assert one["peak"].max() > 0
    _same_bytes(one, seven, "soft")


def test_state_and_rng_builders_equal_one_call_per_stream(oracle):
    """init_state / rng_default repeat one call's result; every stream's entry is what its own call writes"""
    import ctypes as C

    st = oracle.init_state(5)
    own = np.zeros((1, 3), dtype=PARMS_DTYPE)
    oracle.h.mbxo_init_parms(own[0, 0:1].ctypes.data, own[0, 1:2].ctypes.data, own[0, 2:3].ctypes.data)
    assert st.shape == (5, 3) and all(st[i].tobytes() == own[0].tobytes() for i in range(5))
    r = oracle.rng_seeded([0, 1, 0xFFFFFFFF])
    for i, seed in enumerate([0, 1, 0xFFFFFFFF]):
        one = oracle.rng_default(1)
        oracle.h.mbxo_rng_seed(one.ctypes.data, C.c_uint32(seed))
        assert r[i].tobytes() == one[0].tobytes()
