"""GPU suite (-m gpu): the HIP path, called through the C-ABI launcher, against the CPU oracle
on the same seeded inputs and against the golden fixtures produced by the real reference.
Nothing here reads /root/reference."""
import os

import numpy as np
import pytest

import golden_io
import oracle_lib
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()  # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _host_batch(m, codec, S, T, frames, state, rng):
    from mbelib_neo_amd import decoder

    return decoder.process_batch_host(codec, S, T, frames, state, rng)


# ---- FEC stage: bit-exact ------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1])
def test_fec_random_frames_bit_exact(mbx, oracle, codec):
    from mbelib_neo_amd import decoder, framegen

    n = 65536
    frames = framegen.random_frames(codec, n, framegen.rng_for(100 + codec))
    # a share of frames with few channel errors so every error-count bucket is exercised
    frames[::3] &= framegen.random_frames(codec, (n + 2) // 3, framegen.rng_for(200 + codec)) & framegen.random_frames(
        codec, (n + 2) // 3, framegen.rng_for(300 + codec)
    )
    dec = decoder.BatchDecoder(codec, 1)
    got = decoder.records_numpy(dec.fec(frames))
    ref = oracle.fec_batch(codec, frames)
    assert np.array_equal(got["w"], ref["w"])


@pytest.mark.parametrize("codec", [0, 1])
def test_fec_golden_fixtures(mbx, oracle, codec):
    from mbelib_neo_amd import decoder

    fx = golden_io.fec(codec)
    _, packed = oracle.pack(codec, fx["cells"])
    dec = decoder.BatchDecoder(codec, 1)
    rec = decoder.records_numpy(dec.fec(packed))
    nbits = 88 if codec == 0 else 49
    assert np.array_equal(oracle_lib.records_to_bits(rec, nbits), fx["bits"])
    parity.check_results(fx["result"], oracle_lib.records_to_results(rec))


def _ecc_words(kind, words):
    import torch

    from mbelib_neo_amd import _native

    d_in = torch.from_numpy(np.ascontiguousarray(words, dtype=np.uint32).view(np.int32)).cuda()
    d_out = torch.empty_like(d_in)
    d_err = torch.empty_like(d_in)
    rc = _native.lib().mbx_ecc_words(kind, d_in.data_ptr(), d_in.numel(), d_out.data_ptr(), d_err.data_ptr(),
                                     torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "mbx_ecc_words")
    return d_out.cpu().numpy().view(np.uint32), d_err.cpu().numpy()


def test_ecc_exhaustive_hamming_and_golay_syndromes(mbx, oracle):
    """Every known answer of the reference's exhaustive ECC fixture through the HIP code-word kernel: Golay(23,12) --
    4 data words x all 2,048 parity patterns (every syndrome) + 4,096 random words + the 0xA55 / bit-5 case of
    tests/test_ecc.c:356-375; Hamming(15,11) -- all 32,768 words (tests/test_ecc.c:163-259).  Bit-exact, including
    the returned error counts.  Then the same decoders inside the frame kernel on noisy encoded frames vs the oracle."""
    from mbelib_neo_amd import decoder, framegen

    golay, ham = golden_io.ecc_kat()
    assert len(golay) >= 4 * 2048 + 4096 and len(ham) == 32768
    out, errs = _ecc_words(0, golay["inp"])
    assert np.array_equal(out, golay["out"]) and np.array_equal(errs, golay["errs"])
    assert (int(out[-1]) >> 11) == 0xA55 and int(errs[-1]) == 1
    out, errs = _ecc_words(1, ham["inp"])
    assert np.array_equal(out, ham["out"]) and np.array_equal(errs, ham["errs"])
    kat7100 = golden_io.imbe7100_kat()["hamming"]   # the 7100x4400 bit mapping of the same code (src/ecc/ecc.c:422-464)
    out, errs = _ecc_words(2, kat7100["inp"])
    assert np.array_equal(out, kat7100["out"]) and np.array_equal(errs, kat7100["errs"])

    n = 32768
    rng = framegen.rng_for(7)
    param = rng.integers(0, 2, size=(n, 88), dtype=np.uint8)
    frames = framegen.encode_imbe7200x4400(param)
    frames ^= framegen.random_frames(0, n, rng) & framegen.random_frames(0, n, rng) & framegen.random_frames(0, n, rng)
    dec = decoder.BatchDecoder(0, 1)
    got = decoder.records_numpy(dec.fec(frames))
    ref = oracle.fec_batch(0, frames)
    assert np.array_equal(got["w"], ref["w"])


# ---- float -> int16: exact -------------------------------------------------------------------
def test_floattoshort_exact(mbx, oracle):
    from mbelib_neo_amd import decoder, framegen

    fx = golden_io.f2s()
    got = decoder.floattoshort(fx["inp"])
    assert np.array_equal(got, fx["out"])
    rng = framegen.rng_for(9)
    x = (rng.standard_normal((4096, 160)) * 3000.0).astype(np.float32)
    x[::17, 5] = np.nan
    x[::19, 6] = np.inf
    x[::23, 7] = -np.inf
    assert np.array_equal(decoder.floattoshort(x), oracle.floattoshort(x))


# ---- the per-batch tally of results, formed on the device ---------------------------------------
def test_result_histogram_counts_what_the_host_would(mbx, oracle):
    """mbx_result_histogram (include/mbx.h; ref include/mbelib-neo/mbelib.h:154-166 -- the flags and error counts a host tallies per
    frame): the device's counters over (a) synthetic results with every flag combination and (b) the results of a real mixed AMBE
    batch equal a numpy tally of the same structs; launches accumulate; sizes that are no multiple of anything."""
    import torch
    from mbelib_neo_amd import decoder, framegen

    def tally(r):
        f = r["flags"].astype(np.int64)
        t = {"frames": len(r), "c0_errors": int(r["c0_errors"].sum()), "protected_errors": int(r["protected_errors"].sum()),
             "c4_errors": int(r["c4_errors"].sum()), "total_errors": int(r["total_errors"].sum()),
             "frames_with_errors": int((r["total_errors"] > 0).sum())}
        for b, name in enumerate(("soft_input", "c0_valid", "c4_valid", "flag3", "tone", "erasure", "repeat", "mute")):
            t[name] = int(((f >> b) & 1).sum())
        return t

    rng = framegen.rng_for(77)
    for n in (1, 255, 1024, 65536 + 3, 1 << 20):
        r = np.zeros(n, dtype=decoder.RESULT_DTYPE)
        r["flags"] = rng.integers(0, 256, size=n)
        r["c0_errors"] = rng.integers(0, 4, size=n)
        r["protected_errors"] = rng.integers(0, 12, size=n)
        r["c4_errors"] = rng.integers(0, 2, size=n)
        r["total_errors"] = np.where(rng.random(n) < 0.3, 0, r["c0_errors"] + r["protected_errors"])
        d = torch.from_numpy(r.view(np.uint8).copy()).cuda()
        assert decoder.result_histogram(d) == tally(r), n
    # a real batch: AMBE+2 frames of random bits (voice, erasures, tones, repeats)
    S, T = 512, 6
    frames = framegen.random_frames(1, S * T, rng)
    ref = oracle.process_batch(1, S, T, frames, oracle.init_state(S), oracle.rng_seeded(list(range(S))))
    dec = decoder.BatchDecoder(1, S, seeds=list(range(S)))
    out = dec.decode(frames, T)
    torch.cuda.synchronize()
    got = decoder.result_histogram(out["results"])
    assert got == tally(np.asarray(ref["results"]))
    assert got["frames"] == S * T and got["repeat"] + got["erasure"] + got["tone"] > 0
    # two launches into one tally
    L = mbx.lib()
    hist = torch.zeros(len(decoder.RESULT_HIST_FIELDS), dtype=torch.int64, device="cuda")
    for _ in range(2):
        assert L.mbx_result_histogram(out["results"].data_ptr(), S * T, hist.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
    assert hist.cpu().tolist() == [2 * got[k] for k in decoder.RESULT_HIST_FIELDS]
    assert L.mbx_result_histogram(None, 1, hist.data_ptr(), None) == -1 and L.mbx_result_histogram(out["results"].data_ptr(), 0, hist.data_ptr(), None) == 0


# ---- synthesis: golden hash scenario ----------------------------------------------------------
def test_golden_synth_scenario(mbx, oracle):
    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import rng_seeded

    g = golden_io.golden_synth()
    pcmf, cur, prev, _, pcm16 = decoder.synthesize_speech(
        g["cur_in"].reshape(1), g["prev_in"].reshape(1), rng_seeded([0xC0FFEE]), want_pcm16=True
    )
    m = parity.check_pcm(g["pcmf"], pcmf, g["pcm16"], pcm16)
    print("golden synth:", m)
    parity.check_state(g["cur_out"].reshape(1), cur)
    parity.check_state(g["prev_out"].reshape(1), prev)


def test_synth_sequences_match_reference(mbx, oracle):
    """The reference's bench recipes as 24-frame known answers (bench/bench_synth.c:40-67: L = 40, w0 alternating
    0.09 / 0.11, Vl and Ml patterns; bench/bench_unvoiced.c:33-52,87: L = 36 all unvoiced), produced by the real
    reference (tests/golden/synth_seq.bin), through the HIP mbe_synthesizeSpeechf frame by frame."""
    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import PARMS_DTYPE, rng_seeded

    frames, fx = golden_io.synth_seq()
    for recipe in range(2):
        cur = np.zeros(1, dtype=PARMS_DTYPE)
        cur[0] = oracle.init_state(1)[0, 0]
        if recipe == 0:
            rng = rng_seeded([0x123456])
            cur["w0"] = np.float32(0.09378)
            cur["L"] = 40
            for k in range(1, 41):
                cur["Vl"][0, k] = int((k % 3) != 0)
                cur["Ml"][0, k] = np.float32(0.05) + np.float32(0.002) * np.float32(k)
                cur["log2Ml"][0, k] = 0.0
                cur["PHIl"][0, k] = np.float32(k) * np.float32(0.1)
                cur["PSIl"][0, k] = np.float32(k) * np.float32(0.05)
        else:
            rng = rng_seeded([0xBEEF])
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
            pcmf, cur, prev, rng, _ = decoder.synthesize_speech(cur, prev, rng)
            prev = cur.copy()
            got.append(pcmf[0])
        m = parity.check_pcm(fx[recipe]["pcmf"], np.array(got), what=f"recipe{recipe}")
        print("synth_seq recipe", recipe, m)
        parity.check_state(fx[recipe]["cur"].reshape(1), cur)


def test_synth_int16_of_non_finite_samples(mbx, oracle):
    """The stream / synthesis kernels convert to int16 with the reference's rules (NaN -> 0, clamp at +-31128)
    without testing for NaN / Inf explicitly: amplitudes that make the float PCM non-finite or huge must still give
    the int16 the reference's mbe_floattoshort gives for the same float samples."""
    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import rng_seeded

    g = golden_io.golden_synth()
    cur = np.repeat(g["cur_in"].reshape(1), 3)
    prev = np.repeat(g["prev_in"].reshape(1), 3)
    cur["Ml"][0, 3] = np.nan        # NaN amplitude: every sample of the frame becomes NaN
    cur["Ml"][1, 2] = 3.0e38        # overflows to +-Inf in the sum
    cur["Ml"][2, 2] = 1.0e6         # finite, far beyond the clip level
    pcmf, _, _, _, pcm16 = decoder.synthesize_speech(cur, prev, rng_seeded([1, 2, 3]), want_pcm16=True)
    assert np.array_equal(pcm16, oracle.floattoshort(pcmf)), "int16 differs from mbe_floattoshort of the same floats"
    assert not np.isfinite(pcmf[0]).any() and (pcm16[0] == 0).all()
    assert np.abs(pcm16[1:]).max() <= 31128


# ---- full path vs the reference's golden streams ------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1])
def test_stream_golden_fixtures(mbx, oracle, codec):
    from mbelib_neo_amd.layout import init_state, rng_seeded

    S, T, fx = golden_io.stream(codec)
    frames = fx["frames"]
    _, packed = oracle.pack(codec, frames["cells"].reshape(S * T, -1))
    out = _host_batch(mbx, codec, S, T, packed, init_state(S), rng_seeded([1234 + s for s in range(S)]))
    nbits = 88 if codec == 0 else 49
    assert np.array_equal(oracle_lib.records_to_bits(out["records"], nbits), frames["bits"].reshape(S * T, nbits))
    parity.check_results(frames["result"].reshape(-1), out["results"])
    m = parity.check_pcm(frames["pcmf"], out["pcmf"], frames["pcm16"], out["pcm16"])
    print(f"codec {codec} golden streams:", m)
    parity.check_state(fx["final"], out["state"])


# ---- full path vs the oracle on seeded random streams --------------------------------------------
@pytest.mark.parametrize("codec,S,T", [(0, 512, 16), (1, 512, 16), (0, 2048, 2), (1, 1024, 6)])
def test_random_streams_vs_oracle(mbx, oracle, codec, S, T):
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    frames = framegen.random_frames(codec, S * T, framegen.rng_for(1000 + 10 * codec + T))
    seeds = [1234 + s for s in range(S)]
    ref = oracle.process_batch(codec, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    got = _host_batch(mbx, codec, S, T, frames, init_state(S), rng_seeded(seeds))
    assert np.array_equal(got["records"]["w"], ref["records"]["w"])
    parity.check_results(ref["results"], got["results"])
    m = parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
    print(f"codec {codec} S={S} T={T}:", m)
    parity.check_state(ref["state"], got["state"])
    assert np.array_equal(ref["rng"], got["rng"])
    # the same against the oracle in its "reference, bit for bit" form (set_fft_float: FFTPACK's float transform as the reference's
    # PFFFT runs it; tests/test_oracle_golden.py pins that form on the reference's float hash and on every golden stream)
    oracle.set_fft_float(1)
    try:
        ref_f = oracle.process_batch(codec, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    finally:
        oracle.set_fft_float(0)
    parity.check_results(ref_f["results"], got["results"])
    parity.check_pcm(ref_f["pcmf"], got["pcmf"], ref_f["pcm16"], got["pcm16"])
    parity.check_state(ref_f["state"], got["state"])


def test_clean_voiced_imbe_vs_oracle(mbx, oracle):
    """BASELINE config 2 at a size the oracle finishes in seconds: clean all-voiced IMBE frames,
    one warm-up frame then the measured frame."""
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    S = 2048
    rng = framegen.rng_for(2)
    f0 = framegen.imbe_clean_voiced_frames(S, rng)
    f1 = framegen.imbe_clean_voiced_frames(S, rng)
    frames = np.stack([f0, f1], axis=1).reshape(S * 2, 18)
    seeds = [1234 + s for s in range(S)]
    ref = oracle.process_batch(0, S, 2, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    got = _host_batch(mbx, 0, S, 2, frames, init_state(S), rng_seeded(seeds))
    assert int(ref["results"]["total_errors"].max()) == 0  # the encoder produces clean code words
    parity.check_results(ref["results"], got["results"])
    m = parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
    print("clean voiced:", m)
    parity.check_state(ref["state"], got["state"])


def test_ambe_noisy_voice_vs_oracle(mbx, oracle):
    """BASELINE config 3 shape: clean AMBE+2 voice frames with 1 % bit flips."""
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    S, T = 1024, 4
    frames = framegen.ambe_noisy_voice_frames(S * T, framegen.rng_for(3))
    seeds = [1234 + s for s in range(S)]
    ref = oracle.process_batch(1, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    got = _host_batch(mbx, 1, S, T, frames, init_state(S), rng_seeded(seeds))
    parity.check_results(ref["results"], got["results"])
    m = parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
    print("ambe noisy voice:", m)
    parity.check_state(ref["state"], got["state"])


# ---- size-independent properties at BASELINE's full batch size ------------------------------------
def test_full_size_properties(mbx, oracle):
    """65,536 streams (config 2 size): (1) splitting T = 4 into 2 + 2 launches gives bit-identical
    PCM and state (the state round-trips through HBM losslessly); (2) a re-run is bit-identical
    (determinism); (3) a strided sample of streams matches the oracle."""
    import torch
    from mbelib_neo_amd import decoder, framegen

    S, T = 65536, 4
    frames = framegen.random_frames(0, S * T, framegen.rng_for(4)).reshape(S, T, 18)
    seeds = np.arange(S) + 1234

    pick = np.arange(0, S, 257)
    d_pick = torch.from_numpy(pick).cuda()

    def run(splits):
        dec = decoder.BatchDecoder(0, S, seeds=seeds)
        pcs, pfs = [], []
        t0 = 0
        for t in splits:
            out = dec.decode(np.ascontiguousarray(frames[:, t0 : t0 + t]).reshape(-1, 18), t, want_float=True)
            pcs.append(out["pcm16"].reshape(S, t, 160))
            pfs.append(out["pcmf"].reshape(S, t, 160)[d_pick])   # float PCM of the sampled streams only (host memory)
            t0 += t
        torch.cuda.synchronize()
        return torch.cat(pcs, dim=1).cpu().numpy(), torch.cat(pfs, dim=1).cpu().numpy(), dec.state_numpy(), dec.rng_numpy()

    a_pcm, a_f, a_state, a_rng = run([4])
    b_pcm, b_f, b_state, b_rng = run([2, 2])
    c_pcm, c_f, c_state, _ = run([4])
    assert np.array_equal(a_pcm, c_pcm) and a_f.tobytes() == c_f.tobytes() and a_state.tobytes() == c_state.tobytes()
    assert np.array_equal(a_pcm, b_pcm) and a_f.tobytes() == b_f.tobytes()
    assert a_state.tobytes() == b_state.tobytes() and a_rng.tobytes() == b_rng.tobytes()
    ref = oracle.process_batch(0, len(pick), T, frames[pick].reshape(-1, 18), oracle.init_state(len(pick)),
                               oracle.rng_seeded(seeds[pick]))
    parity.check_pcm(ref["pcmf"], a_f.reshape(-1, 160), ref["pcm16"], a_pcm[pick].reshape(-1, 160))
    parity.check_state(ref["state"], a_state[pick])


def test_ambe_long_streams_config5_shape(mbx, oracle):
    """BASELINE configs[4], one GPU's shard: 8,192 AMBE+2 streams x T = 128 random-bit frames in ONE launch (the
    capped-occupancy kernel instance; 128 frames of phase wrap, IIR memories, LCG hand-overs, erasures, tones, repeats
    and max-repeat re-initialisations per stream), int16 output; ALL 8,192 streams against the oracle over all 128 frames
    (1,048,576 frames: the tail group and the tail slice of the sliced launch are under it, not only under the HIP-against-HIP
    legs), then determinism (a second run is bit-identical) and the T = 64 + 64 split."""
    import torch
    from mbelib_neo_amd import decoder, framegen

    S, T = 8192, 128
    frames = framegen.random_frames(1, S * T, framegen.rng_for(55)).reshape(S, T, 9)
    seeds = np.arange(S) + 1234
    pick = np.arange(S)
    assert len(pick) == S
    d_pick = torch.from_numpy(pick).cuda()

    def run(splits):
        dec = decoder.BatchDecoder(1, S, seeds=seeds)
        pcs, pfs, res, recs = [], [], [], []
        t0 = 0
        for t in splits:
            out = dec.decode(np.ascontiguousarray(frames[:, t0 : t0 + t]).reshape(-1, 9), t, want_float=True)
            recs.append(out["records"].reshape(S, t, 4))
            pcs.append(out["pcm16"].reshape(S, t, 160)[d_pick])
            pfs.append(out["pcmf"].reshape(S, t, 160)[d_pick])
            res.append(out["results"].reshape(S, t, 5)[d_pick])
            digest = out["pcm16"].to(torch.int64).sum().item()   # every sample of every stream
            t0 += t
            del out
        torch.cuda.synchronize()
        return (torch.cat(pcs, dim=1).cpu().numpy(), torch.cat(pfs, dim=1).cpu().numpy(), torch.cat(res, dim=1).cpu().numpy(),
                dec.state_numpy(), dec.rng_numpy(), digest, torch.cat(recs, dim=1).cpu().numpy())

    a = run([128])
    ran = mbx.lib().mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream)
    ref = oracle.process_batch(1, len(pick), T, frames[pick].reshape(-1, 9), oracle.init_state(len(pick)), oracle.rng_seeded(seeds[pick]))
    from mbelib_neo_amd.layout import RESULT_DTYPE

    with parity.located(T, pick):
        parity.check_results(ref["results"], np.ascontiguousarray(a[2]).view(RESULT_DTYPE).reshape(-1))
    m = parity.check_pcm_located(ref["pcmf"], a[1].reshape(-1, 160), ref["pcm16"], a[0].reshape(-1, 160), T, pick)
    print("AMBE+2 8192 x 128:", m)
    parity.check_state(ref["state"], a[3][pick])
    _every_stream_extras(ref, a, T)
    flags = ref["results"]["flags"]
    assert (flags & 0x20).any() and (flags & 0x40).any() and (flags & 0x10).any()   # erasures, repeats, tones are in the sample
    del ref
    b = run([128])
    assert a[5] == b[5] and a[3].tobytes() == b[3].tobytes() and a[0].tobytes() == b[0].tobytes()
    del b
    c = run([64, 64])
    assert a[3].tobytes() == c[3].tobytes() and a[4].tobytes() == c[4].tobytes()
    assert a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()
    del c
    # 8,192 streams do not fill the device's wave slots evenly, so this shape is a SLICED launch (two groups of streams x slices of 16
    # frames on two internal HIP streams, include/mbx.h): the comparisons above -- oracle, determinism, 64 + 64 -- are of that form; a
    # launch of eight frames per stream is never sliced, so sixteen of them are the unsliced reference, bit for bit
    L = mbx.lib()
    Tc = L.mbx_launch_slices(1, S, T)
    print("slice length for 8,192 x 128:", Tc)
    if os.environ.get("MBX_SLICE") != "0" and not os.environ.get("MBX_NO_LDS_RESIDENT"):   # (tools/test_env_matrix.sh runs the suite under those switches too)
        assert Tc == 16 and L.mbx_launch_slices(1, S, 8) == 0 and L.mbx_launch_slices(0, 65536, 16) == 0
        assert L.mbx_batch_kernel_name(1, S, T, 0) == b"ambe_stream_kernel_lds_slice"
        assert ran == b"ambe_stream_kernel_lds_slice"   # ... and it is what the launch of 128 frames recorded
    d = run([8] * 16)
    if not os.environ.get("MBX_NO_LDS_RESIDENT") and not os.environ.get("MBX_LDS_MIN_FRAMES"):
        assert L.mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream) == b"ambe_stream_kernel_lds"
    assert a[3].tobytes() == d[3].tobytes() and a[4].tobytes() == d[4].tobytes()
    assert a[0].tobytes() == d[0].tobytes() and a[1].tobytes() == d[1].tobytes()


def _full_shape_run(codec, S, splits, frames, seeds, d_pick, resident=False):
    """decode S streams in launches of `splits` frames each; returns (pcm16, pcmf, results) of the picked streams, the final
    state / rng, and a digest over every int16 sample of every stream"""
    import torch
    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import FRAME_BYTES

    fb = FRAME_BYTES[codec]
    dec = decoder.BatchDecoder(codec, S, seeds=seeds, resident=resident)
    pcs, pfs, res, recs, digest = [], [], [], [], 0
    t0 = 0
    for t in splits:
        out = dec.decode(np.ascontiguousarray(frames[:, t0:t0 + t]).reshape(-1, fb), t, want_float=True)
        recs.append(out["records"].reshape(S, t, 4))
        pcs.append(out["pcm16"].reshape(S, t, 160)[d_pick])
        pfs.append(out["pcmf"].reshape(S, t, 160)[d_pick])
        res.append(out["results"].reshape(S, t, 5)[d_pick])
        digest += out["pcm16"].to(torch.int64).sum().item() * (t0 + 1)
        t0 += t
        del out
    torch.cuda.synchronize()
    return (torch.cat(pcs, dim=1).cpu().numpy(), torch.cat(pfs, dim=1).cpu().numpy(), torch.cat(res, dim=1).cpu().numpy(),
            dec.state_numpy(), dec.rng_numpy(), digest, torch.cat(recs, dim=1).cpu().numpy())


def _every_stream_extras(ref, a, T):
    """what a full-shape test can hold to the oracle once EVERY stream is on both sides (a = a _full_shape_run tuple, all streams in
    order): the records and the RNG state byte for byte, and the state block by block of 256 streams -- the bound the sampled
    comparison of about 260 streams used to apply, now to each 256 on their own (parity.check_state_blocks)"""
    from mbelib_neo_amd.layout import RECORD_DTYPE

    parity.check_exact(ref["records"], np.ascontiguousarray(a[6]).view(RECORD_DTYPE).reshape(-1), "records", T)
    parity.check_exact(ref["rng"], a[4], "rng state")
    parity.check_state_blocks(ref["state"], a[3])


def test_ambe_fec_config3_full_shape(mbx, oracle):
    """BASELINE configs[2] at its full shape through the kernel bench.py times for it: 65,536 AMBE+2 streams x T = 1 per launch
    (mbx_process_batch takes ONE launch for it, `ambe_one_launch_kernel`: front blocks and stream blocks in one grid; the resident
    form `ambe_one_launch_kernel_res`), clean voice frames with 1 % bit flips, four ticks in a row so that the state is warm and
    both walking directions run.  HIP vs ORACLE (the CPU restatement, double-precision FFT) on ALL 65,536 streams -- the lead
    chunks of the grid and its last stream blocks included --: results exact, PCM / state in tolerance; then determinism (a second
    run is bit-identical in every int16 sample, state and RNG) and the resident form (bit-identical again)."""
    import torch
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import RESULT_DTYPE

    S, T = 65536, 4
    frames = framegen.ambe_noisy_voice_frames(S * T, framegen.rng_for(203), ber=0.01).reshape(S, T, 9)
    seeds = np.arange(S) + 4321
    pick = np.arange(S)
    assert len(pick) == S
    d_pick = torch.from_numpy(pick).cuda()
    L, strm = mbx.lib(), torch.cuda.current_stream().cuda_stream
    a = _full_shape_run(1, S, [1, 1, 1, 1], frames, seeds, d_pick)
    assert L.mbx_stream_kernel_name(1, 1) == b"ambe_stream_kernel_one"   # (what the staged calls take for this shape)
    assert L.mbx_last_kernel_name(strm) == b"ambe_one_launch_kernel" or os.environ.get("MBX_FUSE_ONE") in ("0", "1")   # what ran
    ref = oracle.process_batch(1, len(pick), T, frames[pick].reshape(-1, 9), oracle.init_state(len(pick)), oracle.rng_seeded(seeds[pick]))
    with parity.located(T, pick):
        parity.check_results(ref["results"], np.ascontiguousarray(a[2]).view(RESULT_DTYPE).reshape(-1))
    m = parity.check_pcm_located(ref["pcmf"], a[1].reshape(-1, 160), ref["pcm16"], a[0].reshape(-1, 160), T, pick)
    print("AMBE+2 65,536 x 1 x 4 ticks:", m)
    parity.check_state(ref["state"], a[3][pick])
    _every_stream_extras(ref, a, T)
    del ref
    b = _full_shape_run(1, S, [1, 1, 1, 1], frames, seeds, d_pick)
    assert a[5] == b[5] and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes() and a[0].tobytes() == b[0].tobytes()
    del b
    c = _full_shape_run(1, S, [1, 1, 1, 1], frames, seeds, d_pick, resident=True)
    assert L.mbx_last_kernel_name(strm) == b"ambe_one_launch_kernel_res" or os.environ.get("MBX_FUSE_ONE") in ("0", "1")
    assert a[5] == c[5] and a[3].tobytes() == c[3].tobytes() and a[1].tobytes() == c[1].tobytes()


def _full_shape_run_staged(codec, S, ticks, frames, seeds, d_pick):
    """the same ticks through the staged calls (mbx_fec_* + mbx_process_records: FEC, expansion and stream launches)"""
    import torch
    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import FRAME_BYTES

    fb = FRAME_BYTES[codec]
    dec = decoder.BatchDecoder(codec, S, seeds=seeds)
    pcs, pfs, res, recs, digest = [], [], [], [], 0
    for t in range(ticks):
        out = dec.decode(np.ascontiguousarray(frames[:, t:t + 1]).reshape(-1, fb), 1, want_float=True, staged=True)
        pcs.append(out["pcm16"].reshape(S, 1, 160)[d_pick])
        pfs.append(out["pcmf"].reshape(S, 1, 160)[d_pick])
        res.append(out["results"].reshape(S, 1, 5)[d_pick])
        recs.append(out["records"].to(torch.int64).sum().item())
        digest += out["pcm16"].to(torch.int64).sum().item() * (t + 1)
        del out
    torch.cuda.synchronize()
    return (torch.cat(pcs, dim=1).cpu().numpy(), torch.cat(pfs, dim=1).cpu().numpy(), torch.cat(res, dim=1).cpu().numpy(),
            dec.state_numpy(), dec.rng_numpy(), digest, recs)


def test_imbe_voiced_config2_full_shape(mbx, oracle):
    """BASELINE configs[1] -- the HEADLINE -- at its full shape through the kernels bench.py times for it: 65,536 IMBE streams
    x T = 1 per launch, clean all-voiced frames, one warm-up tick then four measured ticks (every tick a launch of its own, as a
    decoder that is called every 20 ms issues them).  mbx_process_batch takes ONE launch for this shape
    (`imbe_one_launch_kernel`: front blocks -- FEC + expansion of eight frames per wave -- and stream blocks in one grid); the staged
    calls take `imbe_stream_kernel_one` behind the FEC and expansion launches -- both instances are run here, each under the name
    the launcher recorded for it, and must agree bit for bit.
    HIP vs ORACLE on ALL 65,536 streams in BOTH transform forms (double-precision FFT; the reference's float PFFFT
    restated): results exact, PCM / state in tolerance; then determinism (a second run is bit-identical in
    every int16 sample, state and RNG) and the resident form (`imbe_one_launch_kernel_res`, bit-identical again).
    ref src/core/mbelib.c:1020-1040 (the voiced bank this workload isolates), tests/test_golden_pcm.c:67-211."""
    import torch
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import RESULT_DTYPE

    S, T = 65536, 5
    rng = framegen.rng_for(0xC2)
    frames = np.stack([framegen.imbe_clean_voiced_frames(S, rng) for _ in range(T)], axis=1)   # [S, T, 18]
    seeds = np.arange(S) + 1234
    pick = np.arange(S)
    assert len(pick) == S
    d_pick = torch.from_numpy(pick).cuda()
    L, strm = mbx.lib(), torch.cuda.current_stream().cuda_stream
    assert L.mbx_stream_kernel_name(0, 1) == b"imbe_stream_kernel_one"
    one_launch = L.mbx_batch_kernel_name(0, S, 1, 0) in (b"imbe_one_launch_kernel", b"imbe_stream_kernel_one_fused")
    assert one_launch or os.environ.get("MBX_FUSE_ONE") == "0"
    a = _full_shape_run(0, S, [1] * T, frames, seeds, d_pick)                 # mbx_process_batch: the one launch
    assert L.mbx_last_kernel_name(strm) == L.mbx_batch_kernel_name(0, S, 1, 0)   # the prediction for this call is what ran ...
    assert L.mbx_last_kernel_name(strm) == b"imbe_one_launch_kernel" or os.environ.get("MBX_FUSE_ONE") in ("0", "1")   # ... by name
    st = _full_shape_run_staged(0, S, T, frames, seeds, d_pick)               # imbe_stream_kernel_one behind FEC + expansion
    assert L.mbx_last_kernel_name(strm) == b"imbe_stream_kernel_one"
    assert a[3].tobytes() == st[3].tobytes() and a[4].tobytes() == st[4].tobytes()
    assert a[0].tobytes() == st[0].tobytes() and a[1].tobytes() == st[1].tobytes() and a[2].tobytes() == st[2].tobytes() and a[5] == st[5]
    del st
    sel = frames[pick].reshape(-1, 18)
    ref = oracle.process_batch(0, len(pick), T, sel, oracle.init_state(len(pick)), oracle.rng_seeded(seeds[pick]))
    assert int(ref["results"]["total_errors"].max()) == 0 and not (ref["results"]["flags"] & 0xC0).any()   # clean: no repeat, no mute
    with parity.located(T, pick):
        parity.check_results(ref["results"], np.ascontiguousarray(a[2]).view(RESULT_DTYPE).reshape(-1))
    m = parity.check_pcm_located(ref["pcmf"], a[1].reshape(-1, 160), ref["pcm16"], a[0].reshape(-1, 160), T, pick)
    print("IMBE voiced 65,536 x 1 x 5 ticks (double FFT):", m)
    parity.check_state(ref["state"], a[3][pick])
    _every_stream_extras(ref, a, T)
    del ref
    oracle.set_fft_float(1)
    try:
        ref_f = oracle.process_batch(0, len(pick), T, sel, oracle.init_state(len(pick)), oracle.rng_seeded(seeds[pick]))
    finally:
        oracle.set_fft_float(0)
    with parity.located(T, pick):
        parity.check_results(ref_f["results"], np.ascontiguousarray(a[2]).view(RESULT_DTYPE).reshape(-1))
    m = parity.check_pcm_located(ref_f["pcmf"], a[1].reshape(-1, 160), ref_f["pcm16"], a[0].reshape(-1, 160), T, pick)
    print("IMBE voiced 65,536 x 1 x 5 ticks (float FFT):", m)
    parity.check_state(ref_f["state"], a[3][pick])
    _every_stream_extras(ref_f, a, T)
    del ref_f
    b = _full_shape_run(0, S, [1] * T, frames, seeds, d_pick)
    assert a[5] == b[5] and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes() and a[0].tobytes() == b[0].tobytes()
    del b
    c = _full_shape_run(0, S, [1] * T, frames, seeds, d_pick, resident=True)
    assert L.mbx_last_kernel_name(strm) == b"imbe_one_launch_kernel_res" or os.environ.get("MBX_FUSE_ONE") in ("0", "1")
    assert a[5] == c[5] and a[3].tobytes() == c[3].tobytes() and a[1].tobytes() == c[1].tobytes()


@pytest.mark.parametrize("codec", [0, 1, 3])
def test_one_launch_fall_back_path_gives_the_same_bytes(mbx, oracle, codec):
    """A stream block of the one-launch kernels that does not see its front block's flag in time decodes its own frame (IMBE: FEC by
    lanes + expansion in its own wave; AMBE: scalar-unit FEC + expansion by its first eight lanes).  No ordinary launch has ever taken
    that path (mbx_front_fallbacks = 0 everywhere), so it is FORCED -- by a hook the product library does not have: a child process
    (tests/front_skip_case.py) loads libmbx_hip_testing.so, the -DMBX_TESTING build of the same sources, makes every fourth front block
    do nothing, and holds records, results, PCM, state and RNG of four ticks to the bytes of its undisturbed launches, the fall-back
    counter to exactly the streams of the skipped chunks, and what the forced fall-back launches wrote to the ORACLE on every stream
    (a fault both paths share cannot hide behind their agreement).  Here: the product library on the same input gives those same
    bytes, and does not export the hook."""
    import json
    import subprocess
    import sys

    import front_skip_case

    L = mbx.lib()
    assert not hasattr(L, "mbx_testing_set_front_skip") and not hasattr(L, "mbx_debug_set_front_skip")
    if b"one_launch" not in L.mbx_batch_kernel_name(codec, 4096, 1, 0):
        pytest.skip("the one-launch form is switched off (MBX_FUSE_ONE)")
    here = os.path.dirname(os.path.abspath(__file__))
    testing = os.path.join(os.path.dirname(here), "mbelib-neo_amd", "libmbx_hip_testing.so")
    assert os.path.exists(testing), "build it: make -C mbelib-neo_amd/csrc testing (part of __graft_entry__.build())"
    r = subprocess.run([sys.executable, os.path.join(here, "front_skip_case.py"), str(codec)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, MBX_HIP_LIBRARY=testing))
    assert r.returncode == 0, r.stdout[-1500:] + r.stderr[-3000:]
    child = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert child["fallbacks_counted"] > 0
    for resident in (False, True):
        assert front_skip_case.run(codec, resident) == child["resident" if resident else "abi"], resident


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_fused_one_frame_launch_equals_the_staged_launches(mbx, oracle, codec):
    """T = 1 and S > 256, all four codecs: mbx_process_batch (ONE launch: `imbe_one_launch_kernel` / `ambe_one_launch_kernel` /
    `ambe2400_one_launch_kernel` -- front blocks and stream blocks in one grid -- or, IMBE 7100x4400, the front end in the stream's
    own wave) against mbx_fec_* + mbx_process_records (FEC launch, expansion launch, `*_stream_kernel_one`) on RANDOM-BIT frames --
    every error-count bucket, repeats, mutes, headroom resets, invalid fundamentals -- eight ticks of 8,192 + 3 streams (an odd
    batch: frames alternate between the two alignments the scalar fetch handles, and the last one ends the buffer): records,
    results, int16 / float PCM, state and RNG byte for byte; likewise through an index (mbx_process_batch_indexed) and with a
    frame buffer that is only 2-byte aligned (the launcher then takes the staged launches)."""
    import torch
    from mbelib_neo_amd import _native, decoder, framegen

    from mbelib_neo_amd.layout import FRAME_BYTES

    fb = FRAME_BYTES[codec]
    S, T = 8192 + 3, 8
    frames = framegen.random_frames(codec, S * T, framegen.rng_for(0xF0 + codec)).reshape(S, T, fb)
    frames[::5] &= framegen.random_frames(codec, ((S + 4) // 5) * T, framegen.rng_for(0xF8 + codec)).reshape(-1, T, fb)   # some with few errors
    seeds = np.arange(S) + 77
    L = mbx.lib()
    assert L.mbx_batch_kernel_name(codec, S, 1, 0) in (b"imbe_one_launch_kernel", b"imbe_stream_kernel_one_fused", b"imbe7100_stream_kernel_one_fused",
                                                       b"ambe_one_launch_kernel", b"ambe2400_one_launch_kernel") \
        or os.environ.get("MBX_FUSE_ONE") in ("0", "1")

    def run(staged):
        dec = decoder.BatchDecoder(codec, S, seeds=seeds)
        outs = []
        for t in range(T):
            o = dec.decode(np.ascontiguousarray(frames[:, t]), 1, want_float=True, staged=staged)
            outs.append({k: v.cpu().numpy().copy() for k, v in o.items()})
        return outs, dec.state_numpy(), dec.rng_numpy()

    fallbacks_before = max(L.mbx_front_fallbacks(torch.cuda.current_stream().cuda_stream), 0)   # (the counter lives as long as the stream's workspace)
    fo, fs, fr = run(False)
    so, ss, sr = run(True)
    for t in range(T):
        for k in ("records", "results", "pcm16", "pcmf"):
            assert fo[t][k].tobytes() == so[t][k].tobytes(), (t, k)
    assert fs.tobytes() == ss.tobytes() and fr.tobytes() == sr.tobytes()
    flags = decoder.results_numpy(torch.from_numpy(np.concatenate([o["results"] for o in fo])))["flags"]
    assert (flags & 0x40).any() and ((flags & 0x80).any() or codec in (1, 3))   # repeats (and, IMBE, mutes) were in it

    # the caller-workspace entry point takes the in-wave form of the one-launch step (FEC by lanes + expansion in the stream's own
    # wave -- also what a stream block of imbe_one_launch_kernel falls back to): same bytes again
    ws_bytes = int(L.mbx_workspace_bytes(S))
    ws = torch.empty(ws_bytes, dtype=torch.uint8, device="cuda")
    dec = decoder.BatchDecoder(codec, S, seeds=seeds)
    strm = torch.cuda.current_stream().cuda_stream
    for t in range(2):
        out = dec.make_outputs(1, want_float=True)
        d_fr = dec.to_device(np.ascontiguousarray(frames[:, t]))
        _native.check(L.mbx_process_batch_ws(codec, S, 1, d_fr.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(),
                                             out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(), ws.data_ptr(), ws_bytes,
                                             strm), "mbx_process_batch_ws")
        torch.cuda.synchronize()
        for k in ("records", "results", "pcm16", "pcmf"):
            assert out[k].cpu().numpy().tobytes() == fo[t][k].tobytes(), (t, k)
    fallbacks = L.mbx_front_fallbacks(strm)
    print("front-block fall-backs of this test's launches:", fallbacks - fallbacks_before if fallbacks >= 0 else fallbacks)
    assert fallbacks <= 0 or fallbacks - fallbacks_before < S // 50   # (a stream block that does not find its row in time expands its own frame: rare, never wrong)

    # a 2-byte aligned frame buffer: same results (the staged launches serve it)
    dec = decoder.BatchDecoder(codec, S, seeds=seeds)
    buf = torch.zeros(S * fb + 2, dtype=torch.uint8, device="cuda")
    out = dec.make_outputs(1, want_float=True)
    strm = torch.cuda.current_stream().cuda_stream
    buf[2:].copy_(torch.from_numpy(np.ascontiguousarray(frames[:, 0]).reshape(-1)))
    _native.check(L.mbx_process_batch(codec, S, 1, buf.data_ptr() + 2, dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(),
                                      out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(), strm), "mbx_process_batch")
    torch.cuda.synchronize()
    for k in ("records", "results", "pcm16", "pcmf"):
        assert out[k].cpu().numpy().tobytes() == fo[0][k].tobytes(), k

    # through an index: the streams of a larger pool that have a frame this tick
    pool = 2 * S
    dec = decoder.BatchDecoder(codec, pool, seeds=np.repeat(seeds, 2))
    idx = torch.arange(1, pool, 2, dtype=torch.int32, device="cuda")
    d_frames = dec.to_device(np.ascontiguousarray(frames[:, 0]))
    _native.check(L.mbx_process_batch_indexed(codec, S, 1, idx.data_ptr(), d_frames.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(),
                                              out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(),
                                              out["records"].data_ptr(), strm), "mbx_process_batch_indexed")
    torch.cuda.synchronize()
    for k in ("records", "results", "pcm16", "pcmf"):
        assert out[k].cpu().numpy().tobytes() == fo[0][k].tobytes(), k
    st = dec.state_numpy()
    ref0 = decoder.BatchDecoder(codec, S, seeds=seeds)
    ref0.decode(np.ascontiguousarray(frames[:, 0]), 1, staged=True)
    assert st[1::2].tobytes() == ref0.state_numpy().tobytes()


def test_imbe_mixed_config4_full_shape(mbx, oracle):
    """BASELINE configs[3] at the shape bench.py runs it: 65,536 IMBE streams x T = 16 random-bit frames (mixed voiced /
    unvoiced, repeats, mutes) in ONE launch of `imbe_stream_kernel_lds` (the recorded name).  HIP vs ORACLE on ALL 65,536 streams
    over all 16 frames (1,048,576 frames); then determinism and the 8 + 8 split (state through HBM in between)."""
    import torch
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import RESULT_DTYPE

    S, T = 65536, 16
    frames = framegen.random_frames(0, S * T, framegen.rng_for(204)).reshape(S, T, 18)
    seeds = np.arange(S) + 99
    pick = np.arange(S)
    assert len(pick) == S
    d_pick = torch.from_numpy(pick).cuda()
    a = _full_shape_run(0, S, [16], frames, seeds, d_pick)
    switched = any(os.environ.get(k) for k in ("MBX_NO_LDS_RESIDENT", "MBX_LDS_MIN_FRAMES", "MBX_SLICE"))   # (tools/test_env_matrix.sh)
    assert mbx.lib().mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream) == b"imbe_stream_kernel_lds" or switched
    ref = oracle.process_batch(0, len(pick), T, frames[pick].reshape(-1, 18), oracle.init_state(len(pick)), oracle.rng_seeded(seeds[pick]))
    with parity.located(T, pick):
        parity.check_results(ref["results"], np.ascontiguousarray(a[2]).view(RESULT_DTYPE).reshape(-1))
    m = parity.check_pcm_located(ref["pcmf"], a[1].reshape(-1, 160), ref["pcm16"], a[0].reshape(-1, 160), T, pick)
    print("IMBE 65,536 x 16:", m)
    parity.check_state(ref["state"], a[3][pick])
    _every_stream_extras(ref, a, T)
    flags = ref["results"]["flags"]
    assert (flags & 0x40).any() and (flags & 0x80).any()   # repeats and mutes are in the sample
    del ref
    b = _full_shape_run(0, S, [16], frames, seeds, d_pick)
    assert a[5] == b[5] and a[3].tobytes() == b[3].tobytes() and a[4].tobytes() == b[4].tobytes() and a[0].tobytes() == b[0].tobytes()
    del b
    c = _full_shape_run(0, S, [8, 8], frames, seeds, d_pick)
    assert a[3].tobytes() == c[3].tobytes() and a[4].tobytes() == c[4].tobytes() and a[0].tobytes() == c[0].tobytes() and a[1].tobytes() == c[1].tobytes()


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_lds_resident_and_hbm_slot_kernel_instances_are_identical(mbx, oracle, codec):
    """Launches with T >= 4 frames per stream take the stream-kernel instance that keeps prev_mp / prev_mp_enhanced in LDS
    for the whole launch; shorter ones park them in their HBM slots (mbx_api.hip launch_stream, mbx_stream.hip
    ParkedState), and launches of ONE frame per stream have instances of their own without a frame loop (`*_stream_kernel_one`:
    every request of the frame before the first wait, gathered header loads / stores).  Same arithmetic, different homes and
    orders of memory operations: 4,096 streams x 12 frames as one launch (LDS), as 3 x 4 (LDS, state through HBM between
    launches), as 4 x 3 (HBM slots, looped) and as 12 x 1 (the one-frame instances) must be bit-identical in PCM and state, and
    a strided sample must match the oracle."""
    import torch
    from mbelib_neo_amd import decoder, framegen
    from mbelib_neo_amd.layout import FRAME_BYTES

    S, T = 4096, 12
    fb = FRAME_BYTES[codec]
    frames = framegen.random_frames(codec, S * T, framegen.rng_for(41 + codec)).reshape(S, T, fb)
    seeds = np.arange(S) + 77

    def run(split):
        dec = decoder.BatchDecoder(codec, S, seeds=seeds)
        p16, pf = [], []
        for t0 in range(0, T, split):
            out = dec.decode(np.ascontiguousarray(frames[:, t0:t0 + split]).reshape(-1, fb), split, want_float=True)
            p16.append(out["pcm16"].reshape(S, split, 160))
            pf.append(out["pcmf"].reshape(S, split, 160))
        torch.cuda.synchronize()
        return torch.cat(p16, dim=1).cpu().numpy(), torch.cat(pf, dim=1).cpu().numpy(), dec.state_numpy(), dec.rng_numpy()

    a = run(12)
    for split in (4, 3, 1):
        b = run(split)
        assert np.array_equal(a[0], b[0]) and a[1].tobytes() == b[1].tobytes(), f"PCM differs between T=12 and T={split} launches"
        assert a[2].tobytes() == b[2].tobytes() and a[3].tobytes() == b[3].tobytes()
    pick = np.arange(0, S, 61)
    ref = oracle.process_batch(codec, len(pick), T, frames[pick].reshape(-1, fb), oracle.init_state(len(pick)), oracle.rng_seeded(seeds[pick]))
    parity.check_pcm(ref["pcmf"], a[1][pick].reshape(-1, 160), ref["pcm16"], a[0][pick].reshape(-1, 160))
    parity.check_state(ref["state"], a[2][pick])


@pytest.mark.parametrize("codec", [0, 1])
def test_both_stream_orders_small_batches(mbx, oracle, codec):
    """Successive launches walk the streams in opposite directions (launch_stream, mbx_api.hip).  Odd and tiny
    stream counts, two launches in a row on fresh state each: both directions must give the oracle's result."""
    from mbelib_neo_amd import decoder, framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    for S in (1, 3, 65):
        T = 3
        frames = framegen.random_frames(codec, S * T, framegen.rng_for(500 + S + codec))
        seeds = [9 + 5 * s for s in range(S)]
        ref = oracle.process_batch(codec, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
        for _ in range(2):   # one launch in each direction
            got = decoder.process_batch_host(codec, S, T, frames, init_state(S), rng_seeded(seeds))
            assert np.array_equal(got["records"]["w"], ref["records"]["w"])
            parity.check_results(ref["results"], got["results"])
            parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
            parity.check_state(ref["state"], got["state"])


def test_edge_cases(mbx, oracle):
    from mbelib_neo_amd import _native, decoder
    from mbelib_neo_amd.layout import init_state, rng_default

    # empty batch is a no-op
    out = decoder.process_batch_host(0, 0, 4, np.zeros((0, 18), np.uint8), init_state(0), rng_default(0))
    assert out["pcm16"].shape == (0, 160)
    # all-zero and all-one frames
    for fill in (0, 255):
        fr = np.full((4, 18), fill, dtype=np.uint8)
        ref = oracle.process_batch(0, 2, 2, fr, oracle.init_state(2), oracle.rng_default(2))
        got = decoder.process_batch_host(0, 2, 2, fr, init_state(2), rng_default(2))
        parity.check_results(ref["results"], got["results"])
        parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
        parity.check_state(ref["state"], got["state"])
    # invalid bits never reach the device: packer returns -2 and writes nothing
    cells = np.zeros(184, dtype=np.int8)
    cells[3] = 7
    packed = np.full(18, 0xAA, dtype=np.uint8)
    assert _native.lib().mbx_pack_imbe7200x4400(cells.ctypes.data, 1, packed.ctypes.data) == -2
    assert (packed == 0xAA).all()


# ---- soft-decision front end: bit-exact against the reference's own outputs ----
def test_soft_ecc_words_match_reference_fixture(mbx):
    from mbelib_neo_amd import decoder

    kat = golden_io.soft_kat()
    for kind, name, width in ((0, "golay", 23), (1, "hamming", 15)):
        rows = kat[name]
        words, errs = decoder.ecc_soft_words_host(kind, rows["soft"])
        expect = (rows["out"].astype(np.uint32) << np.arange(width, dtype=np.uint32)).sum(axis=1).astype(np.uint32)
        assert np.array_equal(words, expect), name
        assert np.array_equal(errs, rows["ret"]), name


@pytest.mark.parametrize("codec", [0, 1])
def test_soft_frames_match_reference_fixture_and_oracle(mbx, oracle, codec):
    from mbelib_neo_amd import decoder, framegen

    kat = golden_io.soft_kat()["imbe" if codec == 0 else "ambe"]
    nbits = 88 if codec == 0 else 49
    rec = decoder.fec_soft_host(codec, kat["soft"])
    assert np.array_equal(oracle_lib.records_to_bits(rec, nbits), kat["bits"])
    res = oracle_lib.records_to_results(rec)
    for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
        assert np.array_equal(res[name], kat["result"][name]), name
    # a larger seeded batch against the oracle: noisy code words with confidence tied to the noise
    rng = framegen.rng_for(4100 + codec)
    n = 4096
    soft = framegen.soft_frames(codec, n, rng)
    got = decoder.fec_soft_host(codec, soft)
    ref = oracle.fec_soft_batch(codec, soft)
    assert np.array_equal(got["w"], ref["w"])


def test_soft_process_matches_reference_stream(mbx, oracle):
    """mbe_processImbe7200x4400SoftFramef over 12 frames of one stream (fixture from the real reference)."""
    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import init_state, rng_seeded

    kat = golden_io.soft_kat()["process"]
    T = len(kat)
    out = decoder.process_batch_soft_host(0, 1, T, kat["soft"], init_state(1), rng_seeded([4242]))
    res = out["results"]
    for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
        assert np.array_equal(res[name], kat["result"][name]), name
    parity.check_pcm(kat["pcmf"], out["pcmf"])


@pytest.mark.parametrize("codec,S,T", [(0, 192, 4), (1, 256, 4)])
def test_soft_pipeline_vs_oracle(mbx, oracle, codec, S, T):
    """soft FEC + the whole stream stage against the oracle on seeded soft frames"""
    from mbelib_neo_amd import decoder, framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    soft = framegen.soft_frames(codec, S * T, framegen.rng_for(4200 + codec))
    seeds = [1234 + s for s in range(S)]
    ref = oracle.process_batch(codec, S, T, soft, oracle.init_state(S), oracle.rng_seeded(seeds), soft=True)
    got = decoder.process_batch_soft_host(codec, S, T, soft, init_state(S), rng_seeded(seeds))
    assert np.array_equal(got["records"]["w"], ref["records"]["w"])
    parity.check_results(ref["results"], got["results"])
    assert np.all((got["results"]["flags"] & 1) == 1)   # MBE_PROCESS_FLAG_SOFT_INPUT survives the stream stage
    parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
    parity.check_state(ref["state"], got["state"])


@pytest.mark.parametrize("codec", [0, 1])
def test_soft_fec_pruned_search_bit_exact_on_coded_and_degenerate_frames(mbx, oracle, codec):
    """The soft-decision search skips whole rounds of candidates that cannot hold the minimum (mbx_fec.hip, "exact
    pruning").  Bit-exact against the oracle's exhaustive search on the inputs where the bound is tightest and ties are
    most frequent: encoded frames through noise at three noise levels, all-equal reliabilities (every cost ties),
    all-zero reliabilities, and saturated ones."""
    from mbelib_neo_amd import decoder, framegen

    n = 3000
    batches = [framegen.soft_frames_coded(codec, n, framegen.rng_for(8100 + codec + 10 * k), snr_like=snr)
               for k, snr in enumerate((0.8, 2.0, 4.0))]
    rnd = framegen.soft_frames(codec, n, framegen.rng_for(8200 + codec))
    for value in (0, 1, 7, 255):
        f = rnd.copy()
        f[..., 1] = value
        batches.append(f)
    two = rnd.copy()
    two[..., 1] = (two[..., 1] & 1) * 200   # two confidence levels only
    batches.append(two)
    for soft in batches:
        got = decoder.fec_soft_host(codec, soft)
        ref = oracle.fec_soft_batch(codec, soft)
        assert np.array_equal(got["w"], ref["w"])


# ---- IMBE 7100x4400 front end ---------------------------------------------
def test_imbe7100_fec_bit_exact(mbx, oracle):
    from mbelib_neo_amd import decoder, framegen

    kat = golden_io.imbe7100_kat()["fec"]
    rcs, packed = oracle.pack(2, kat["cells"])
    assert all(rc == 0 for rc in rcs)
    dec = decoder.BatchDecoder(2, 1)
    got = decoder.records_numpy(dec.fec(packed))
    assert np.array_equal(oracle_lib.records_to_bits(got, 88), kat["bits"])            # the reference's own outputs
    res = oracle_lib.records_to_results(got)
    for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
        assert np.array_equal(res[name], kat["result"][name]), name
    n = 65536
    frames = framegen.random_frames(2, n, framegen.rng_for(7100))
    frames[::3] &= framegen.random_frames(2, (n + 2) // 3, framegen.rng_for(7101)) & framegen.random_frames(2, (n + 2) // 3, framegen.rng_for(7102))
    assert np.array_equal(decoder.records_numpy(dec.fec(frames))["w"], oracle.fec_batch(2, frames)["w"])


def test_imbe7100_stream_matches_reference_and_oracle(mbx, oracle):
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    st = golden_io.imbe7100_kat()["stream"]
    S, T = st.shape[0], st["frames"].shape[1]
    rcs, packed = oracle.pack(2, st["frames"]["cells"].reshape(S * T, 168))
    out = _host_batch(mbx, 2, S, T, packed, init_state(S), rng_seeded([1234 + s for s in range(S)]))
    ref = st["frames"].reshape(-1)
    parity.check_results(ref["result"], out["results"])
    parity.check_pcm(ref["pcmf"], out["pcmf"])
    parity.check_state(st["final"], out["state"][:, 0])
    # a larger seeded batch against the oracle
    S, T = 512, 6
    frames = framegen.random_frames(2, S * T, framegen.rng_for(7110))
    seeds = [1234 + s for s in range(S)]
    ref = oracle.process_batch(2, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    got = _host_batch(mbx, 2, S, T, frames, init_state(S), rng_seeded(seeds))
    assert np.array_equal(got["records"]["w"], ref["records"]["w"])
    parity.check_results(ref["results"], got["results"])
    parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
    parity.check_state(ref["state"], got["state"])


def test_imbe7100_soft_matches_reference_and_oracle(mbx, oracle):
    from mbelib_neo_amd import decoder, framegen

    kat = golden_io.imbe7100_kat()
    words, errs = decoder.ecc_soft_words_host(2, kat["hamming_soft"]["soft"])
    expect = (kat["hamming_soft"]["out"].astype(np.uint32) << np.arange(15, dtype=np.uint32)).sum(axis=1).astype(np.uint32)
    assert np.array_equal(words, expect) and np.array_equal(errs, kat["hamming_soft"]["ret"])
    rec = decoder.fec_soft_host(2, kat["fec_soft"]["soft"])
    assert np.array_equal(oracle_lib.records_to_bits(rec, 88), kat["fec_soft"]["bits"])
    res = oracle_lib.records_to_results(rec)
    for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
        assert np.array_equal(res[name], kat["fec_soft"]["result"][name]), name
    soft = framegen.soft_frames(2, 2048, framegen.rng_for(7120))
    assert np.array_equal(decoder.fec_soft_host(2, soft)["w"], oracle.fec_soft_batch(2, soft)["w"])


# ---- AMBE 3600x2400 / D-STAR -----------------------------------------------
def test_ambe2400_frame_streams_match_reference_and_oracle(mbx, oracle):
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    framed, _ = golden_io.ambe2400_kat()
    S, T = framed.shape[0], framed["frames"].shape[1]
    rcs, packed = oracle.pack(3, framed["frames"]["cells"].reshape(S * T, 96))
    out = _host_batch(mbx, 3, S, T, packed, init_state(S), rng_seeded([1234 + s for s in range(S)]))
    ref = framed["frames"].reshape(-1)
    assert np.array_equal(oracle_lib.records_to_bits(out["records"], 49), ref["bits"])
    parity.check_results(ref["result"], out["results"])
    parity.check_pcm(ref["pcmf"], out["pcmf"])
    parity.check_state(framed["final"], out["state"])
    # larger seeded batches against the oracle: random bits, and mostly clean channels
    for S, T, clean in ((512, 8, False), (256, 16, True)):
        rng = framegen.rng_for(2400 + T)
        frames = framegen.random_frames(3, S * T, rng)
        if clean:
            frames &= framegen.random_frames(3, S * T, rng) & framegen.random_frames(3, S * T, rng) & framegen.random_frames(3, S * T, rng)
        seeds = [1234 + s for s in range(S)]
        ref = oracle.process_batch(3, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
        got = _host_batch(mbx, 3, S, T, frames, init_state(S), rng_seeded(seeds))
        assert np.array_equal(got["records"]["w"], ref["records"]["w"])
        parity.check_results(ref["results"], got["results"])
        parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
        parity.check_state(ref["state"], got["state"])
        assert np.array_equal(ref["rng"], got["rng"])


def test_ambe2400_scripted_data_streams_match_reference(mbx):
    """mbe_processAmbe2400Dataf through mbx_process_records: voice, valid D-STAR tones, silence / invalid tone
    classes, repeats driven by the error count (fixture from the real reference)"""
    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import init_state, rng_seeded

    _, data = golden_io.ambe2400_kat()
    S, T = data.shape[0], data["frames"].shape[1]
    fr = data["frames"].reshape(-1)
    rec = decoder.records_from_bits(fr["bits"], total_errors=fr["total_in"])
    out = decoder.process_records_host(3, S, T, rec, init_state(S), rng_seeded([5000 + s for s in range(S)]))
    parity.check_results(fr["result"], out["results"])
    parity.check_pcm(fr["pcmf"], out["pcmf"])
    parity.check_state(data["final"], out["state"])
    flags = fr["result"]["flags"]
    assert np.any(flags & 0x10) and np.any(flags & 0x40)


def test_notones_switch_matches_the_reference_built_with_notones(mbx):
    """mbx_set_tone_synthesis(0) = the reference's NOTONES build option at run time (ref CMakeLists.txt:330-337, src/core/mbelib.c:747-751,
    815-819).  Against tests/golden/notones_kat.bin, written by the reference built with -DDISABLE_AMBE_TONES: the tone kernel
    (mbx_synthesize_tone: silence, phases untouched) and scripted data-level streams of both AMBE codecs through mbx_process_records
    -- results, PCM and final state -- and after mbx_set_tone_synthesis(1) the ordinary fixture again.  Checker: reference-made fixtures."""
    import torch

    from mbelib_neo_amd import _native, decoder
    from mbelib_neo_amd.layout import PARMS_DTYPE, init_state, rng_seeded

    L = mbx.lib()
    ambe, dstar, plus2, dst = golden_io.notones_kat()
    strm = torch.cuda.current_stream().cuda_stream

    def tone_rows(rows, by_id):
        """each row of a tone fixture on its own copy of the default state (the phases are checked against the row before it)"""
        n = len(rows)
        cur = torch.from_numpy(np.ascontiguousarray(init_state(n)[:, 0]).view(np.uint8).reshape(-1)).cuda()
        pcm = torch.full((n, 160), 7.0, dtype=torch.float32, device="cuda")
        if by_id:
            ids = torch.from_numpy(np.ascontiguousarray(rows["id"], dtype=np.int32)).cuda()
            rc = L.mbx_synthesize_tone(n, None, ids.data_ptr(), cur.data_ptr(), pcm.data_ptr(), None, strm)
        else:
            rec = decoder.records_from_bits(rows["bits"], total_errors=np.zeros(n, dtype=np.int32))
            d_rec = torch.from_numpy(np.ascontiguousarray(rec).view(np.uint8).reshape(-1)).cuda()
            rc = L.mbx_synthesize_tone(n, d_rec.data_ptr(), None, cur.data_ptr(), pcm.data_ptr(), None, strm)
        _native.check(rc, "mbx_synthesize_tone")
        return pcm.cpu().numpy(), cur.cpu().numpy().view(PARMS_DTYPE)

    assert L.mbx_set_tone_synthesis(0) == 1
    try:
        default = init_state(1)[0, 0]
        for rows, by_id in ((ambe, False), (dstar, True)):
            pcm, cur = tone_rows(rows, by_id)
            assert not pcm.any() and np.all(cur["swn"] == default["swn"]) and np.all(cur["tonePhase"] == default["tonePhase"])
        for data, codec, seed0 in ((plus2, 1, 7000), (dst, 3, 8000)):
            S, T = data.shape[0], data["frames"].shape[1]
            fr = data["frames"].reshape(-1)
            rec = decoder.records_from_bits(fr["bits"], total_errors=fr["total_in"])
            out = decoder.process_records_host(codec, S, T, rec, init_state(S), rng_seeded([seed0 + s for s in range(S)]))
            parity.check_results(fr["result"], out["results"])
            parity.check_pcm(fr["pcmf"], out["pcmf"])
            parity.check_state(data["final"], out["state"])
            assert np.count_nonzero(fr["result"]["flags"] & 0x10) >= 40
    finally:
        assert L.mbx_set_tone_synthesis(1) == 0
    loud, _ = golden_io.tone_kat()
    pcm, _ = tone_rows(loud[:1], False)   # (tones are back: the fixture's first row starts from the default state, like this call)
    assert np.max(np.abs(pcm - loud["pcmf"][:1])) <= 2e-3 and pcm.any()


def test_batch_api_concurrent_threads_and_streams(mbx, oracle):
    """The batch launcher from 4 host threads, each on its own HIP stream with its own decoder (AMBE+2 and IMBE at
    T = 1 both go through the per-stream expand workspace): every thread gets what it gets alone."""
    import threading

    import torch

    from mbelib_neo_amd import decoder, framegen

    S, T, rounds = 256, 1, 6
    jobs = []
    for k in range(4):
        codec = k % 2
        frames = [framegen.random_frames(codec, S * T, framegen.rng_for(900 + 10 * k + r)) for r in range(rounds)]
        jobs.append((codec, frames, np.arange(S) + 77 * k))

    def run(job, stream):
        codec, frames, seeds = job
        with torch.cuda.stream(stream):
            dec = decoder.BatchDecoder(codec, S, seeds=seeds)
            outs = []
            for fr in frames:
                o = dec.decode(fr, T, want_float=True)
                outs.append((o["pcmf"], o["pcm16"], o["results"]))
            stream.synchronize()
            return [tuple(t.cpu().numpy().tobytes() for t in o) for o in outs], dec.state_numpy().tobytes()

    alone = [run(job, torch.cuda.Stream()) for job in jobs]
    for attempt in range(3):
        got, errors = [None] * 4, []

        def work(k):
            try:
                got[k] = run(jobs[k], torch.cuda.Stream())
            except Exception as e:   # noqa: BLE001
                errors.append(e)

        threads = [threading.Thread(target=work, args=(k,)) for k in range(4)]
        for th in threads:
            th.start()
        for th in threads:
            th.join()
        assert not errors, errors
        for k in range(4):
            assert got[k] == alone[k], f"thread {k}: results differ from the run on its own"
    # and the run on its own is the oracle's
    codec, frames, seeds = jobs[1]
    st, rg = oracle.init_state(S), oracle.rng_seeded(seeds)
    for r, fr in enumerate(frames):
        ref = oracle.process_batch(codec, S, T, fr, st, rg)
        st, rg = ref["state"], ref["rng"]
        assert np.frombuffer(alone[1][0][r][2], dtype=np.int32).reshape(-1, 5)[:, 4].tolist() == ref["results"]["flags"].tolist()


def test_explicit_workspace_and_expand_token(mbx, oracle):
    """mbx_process_batch_ws with a caller-owned workspace == mbx_process_batch; mbx_stream_expanded refuses a workspace
    that the last mbx_expand_records() on the stream did not fill for this batch."""
    import torch

    from mbelib_neo_amd import _native, decoder, framegen

    L = _native.lib()
    S, T = 128, 2
    for codec in (0, 1):
        frames = framegen.random_frames(codec, S * T, framegen.rng_for(31 + codec))
        seeds = np.arange(S) + 5
        a = decoder.BatchDecoder(codec, S, seeds=seeds)
        ref = a.decode(frames, T, want_float=True)
        b = decoder.BatchDecoder(codec, S, seeds=seeds)
        out = b.make_outputs(T, want_float=True)
        ws = torch.empty(L.mbx_workspace_bytes(S * T), dtype=torch.uint8, device="cuda")
        d_frames = b.to_device(frames)
        strm = torch.cuda.current_stream().cuda_stream
        rc = L.mbx_process_batch_ws(codec, S, T, d_frames.data_ptr(), b.state.data_ptr(), b.rng.data_ptr(), out["pcm16"].data_ptr(),
                                    out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(), ws.data_ptr(),
                                    ws.numel(), strm)
        assert rc == 0
        torch.cuda.synchronize()
        assert torch.equal(ref["pcmf"], out["pcmf"]) and torch.equal(ref["pcm16"], out["pcm16"])
        assert a.state_numpy().tobytes() == b.state_numpy().tobytes()
        if codec == 1:   # too small a workspace is refused, nothing launched
            assert L.mbx_process_batch_ws(codec, S, T, d_frames.data_ptr(), b.state.data_ptr(), b.rng.data_ptr(), None, None, None,
                                          out["records"].data_ptr(), ws.data_ptr(), 256, strm) == -1
        # expand token
        rec = out["records"]
        assert L.mbx_expand_records(codec, rec.data_ptr(), S * T, strm) == 0
        other = torch.empty_like(rec)
        assert L.mbx_stream_expanded(codec, S, T, other.data_ptr(), b.state.data_ptr(), b.rng.data_ptr(), None, None, None, strm) == -1
        assert L.mbx_stream_expanded(codec, S // 2, T, rec.data_ptr(), b.state.data_ptr(), b.rng.data_ptr(), None, None, None, strm) == -1
        assert L.mbx_stream_expanded(codec, S, T, rec.data_ptr(), b.state.data_ptr(), b.rng.data_ptr(), out["pcm16"].data_ptr(), None,
                                     None, strm) == 0
        torch.cuda.synchronize()


# ---- sessions: device-resident state, host frames in / host PCM out (include/mbx.h "sessions") -------------------
def _session(L, codec, S, max_frames, outputs):
    import ctypes as C

    h = C.c_void_p()
    from mbelib_neo_amd import _native

    _native.check(L.mbx_session_create(C.byref(h), codec, S, max_frames, outputs), "mbx_session_create")
    return h


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_session_matches_batch_decoder_and_oracle(mbx, oracle, codec):
    """A session fed from pageable host memory over several pipelined submits (T = 1, 1, 3, 1, 2) gives bit for bit what
    the device-pointer batch API gives for the same frames, its state comes back identical, and the whole run is the
    oracle's within the PCM tolerance."""
    import ctypes as C

    from mbelib_neo_amd import _native, decoder, framegen
    from mbelib_neo_amd.layout import FRAME_BYTES, PARMS_DTYPE, RESULT_DTYPE, RNG_DTYPE

    L = _native.lib()
    S, Ts = 300, (1, 1, 3, 1, 2)
    fb = FRAME_BYTES[codec]
    seeds = (np.arange(S) + 4321).astype(np.uint32)
    h = _session(L, codec, S, S * max(Ts), 1 | 2 | 4)
    _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
    dec = decoder.BatchDecoder(codec, S, seeds=seeds)
    rng = framegen.rng_for(70 + codec)
    keep, outs = [], []
    st, rg = oracle.init_state(S), oracle.rng_seeded(seeds)
    refs = []
    for T in Ts:
        frames = framegen.random_frames(codec, S * T, rng)
        o16 = np.zeros((S * T, 160), dtype=np.int16)
        of = np.zeros((S * T, 160), dtype=np.float32)
        ores = np.zeros(S * T, dtype=RESULT_DTYPE)
        keep.append(frames)   # pageable input is staged before submit returns, but keep it anyway
        _native.check(L.mbx_session_submit(h, T, frames.ctypes.data, o16.ctypes.data, of.ctypes.data, ores.ctypes.data), "submit")
        outs.append((o16, of, ores))
        ref = oracle.process_batch(codec, S, T, frames, st, rg)
        st, rg = ref["state"], ref["rng"]
        refs.append(ref)
    _native.check(L.mbx_session_wait(h), "wait")
    for T, frames, (o16, of, ores), ref in zip(Ts, keep, outs, refs):
        got = dec.decode(frames, T, want_float=True)
        assert np.array_equal(got["pcm16"].cpu().numpy(), o16) and got["pcmf"].cpu().numpy().tobytes() == of.tobytes()
        assert decoder.results_numpy(got["results"]).tobytes() == ores.tobytes()
        parity.check_results(ref["results"], ores)
        parity.check_pcm(ref["pcmf"], of, ref["pcm16"], o16)
    state = np.zeros((S, 3), dtype=PARMS_DTYPE)
    srng = np.zeros(S, dtype=RNG_DTYPE)
    _native.check(L.mbx_session_get_state(h, 0, S, state.ctypes.data, srng.ctypes.data), "get_state")
    assert state.tobytes() == dec.state_numpy().tobytes() and srng.tobytes() == dec.rng_numpy().tobytes()
    parity.check_state(st, state)
    assert L.mbx_session_submit(h, max(Ts) + 1, keep[0].ctypes.data, None, None, None) == -1   # more frames than the session was sized for
    assert L.mbx_session_destroy(h) == 0


def test_session_indexed_subset_pinned_buffers(mbx, oracle):
    """Each tick only some of the session's streams have a frame (mbx_session_submit_indexed); buffers from mbx_host_alloc
    are used in place.  Every stream's PCM sequence equals the one it produces when decoded alone."""
    import ctypes as C

    from mbelib_neo_amd import _native, framegen
    from mbelib_neo_amd.layout import RECORD_DTYPE

    L = _native.lib()
    S, ticks = 96, 10
    codec = 1
    seeds = (np.arange(S) + 99).astype(np.uint32)
    h = _session(L, codec, S, S, 1)
    _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
    gen = np.random.default_rng(5)
    frames_of = {s: [] for s in range(S)}
    pcm_of = {s: [] for s in range(S)}
    pin_in = L.mbx_host_alloc(S * 9)
    pin_out = [L.mbx_host_alloc(S * 320) for _ in range(ticks)]
    assert pin_in and all(pin_out)
    views = []
    subsets = []
    for k in range(ticks):
        active = np.sort(gen.choice(S, size=int(gen.integers(1, S + 1)), replace=False)).astype(np.int32)
        fr = framegen.random_frames(codec, len(active), framegen.rng_for(1000 + k))
        _native.check(L.mbx_session_wait(h), "wait")   # the one pinned input buffer is reused every tick
        C.memmove(pin_in, fr.ctypes.data, fr.size)
        rec = np.zeros(len(active), dtype=RECORD_DTYPE)
        _native.check(L.mbx_session_submit_indexed(h, len(active), 1, active.ctypes.data, pin_in, pin_out[k], None, None,
                                                   rec.ctypes.data), "submit_indexed")
        subsets.append((active, fr, rec))
    _native.check(L.mbx_session_wait(h), "wait")
    for k, (active, fr, rec) in enumerate(subsets):
        out = np.ctypeslib.as_array(C.cast(pin_out[k], C.POINTER(C.c_int16)), shape=(S, 160))[: len(active)].copy()
        assert np.array_equal(rec["w"], oracle.fec_batch(codec, fr)["w"])   # the records come back too
        for i, s in enumerate(active):
            frames_of[int(s)].append(fr.reshape(-1, 9)[i])
            pcm_of[int(s)].append(out[i])
    bad = np.array([0, S], dtype=np.int32)
    assert L.mbx_session_submit_indexed(h, 2, 1, bad.ctypes.data, pin_in, None, None, None, None) == -1
    for s in (0, 17, 95):
        if not frames_of[s]:
            continue
        T = len(frames_of[s])
        ref = oracle.process_batch(codec, 1, T, np.array(frames_of[s]).reshape(-1), oracle.init_state(1), oracle.rng_seeded([int(seeds[s])]))
        d = np.abs(ref["pcm16"].astype(np.int32) - np.array(pcm_of[s]).astype(np.int32))
        assert d.max() <= 3 and np.mean(d <= 1) >= 0.999
    L.mbx_host_free(pin_in)
    for q in pin_out:
        L.mbx_host_free(q)
    assert L.mbx_session_destroy(h) == 0


def test_near_threshold_smoothing_decisions_are_the_references(mbx, oracle):
    """tests/golden/threshold_cases.npz: streams (found by tools/find_flips.py over the seeded soak of tools/soak.py) in
    which an enhanced amplitude lands within a few ulp of the adaptive-smoothing threshold VM
    (src/core/mbe_adaptive.c:217-233), so that wave-parallel sums used to put a band on the other side of `Ml > VM`
    than the reference's sequential ones.  Such frames are replayed with the reference's own operation order
    (mbx_stream.hip, enhance_exact): the voicing decisions (integer state) must be the oracle's in every frame, as one
    launch over the whole stream and frame by frame."""
    import os

    import torch

    from mbelib_neo_amd import decoder
    from mbelib_neo_amd.layout import FRAME_BYTES

    z = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "threshold_cases.npz"))
    for codec, seed, frames in zip(z["codec"], z["seed"], z["frames"]):
        codec, seed = int(codec), int(seed)
        T = frames.shape[0]
        fb = FRAME_BYTES[codec]
        flat = np.ascontiguousarray(frames).reshape(-1)[: T * fb].reshape(T, fb)
        st, rg = oracle.init_state(1), oracle.rng_seeded([seed])
        refs = []
        for t in range(T):   # frame by frame: the state after every frame is compared, not just the last
            r = oracle.process_batch(codec, 1, 1, flat[t], st, rg)
            st, rg = r["state"], r["rng"]
            refs.append(r)
        for split in (T, 1):
            dec = decoder.BatchDecoder(codec, 1, seeds=[seed])
            k = 0
            for t0 in range(0, T, split):
                out = dec.decode(np.ascontiguousarray(flat[t0:t0 + split]).reshape(-1), split, want_float=True)
                torch.cuda.synchronize()
                k = t0 + split - 1
                got = dec.state_numpy()
                assert np.array_equal(refs[k]["state"]["Vl"], got["Vl"]), f"codec {codec} seed {seed}: voicing differs after frame {k}"
                parity.check_state(refs[k]["state"], got)
                pf = out["pcmf"].cpu().numpy().reshape(split, 160)
                want = np.concatenate([refs[t]["pcmf"].reshape(1, 160) for t in range(t0, t0 + split)])
                parity.check_pcm(want, pf, what=f"codec {codec} seed {seed} frames {t0}..{k}")


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_device_cell_packing_matches_host_packer(mbx, oracle, codec):
    """mbx_pack_cells (cell arrays -> wire frames on the device, whole-array validation) against the host packer, on a
    ragged count (not a multiple of the 32 frames a workgroup takes), with invalid cells -- also in unused positions --
    flagged per frame."""
    import torch

    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import FRAME_BYTES, FRAME_CELLS

    L = _native.lib()
    rows, cols = FRAME_CELLS[codec]
    ncell, n = rows * cols, 1000 + codec
    rng = np.random.default_rng(17 + codec)
    cells = rng.integers(0, 2, size=(n, ncell), dtype=np.int8)
    host_pack = {0: L.mbx_pack_imbe7200x4400, 1: L.mbx_pack_ambe3600x2450, 2: L.mbx_pack_imbe7100x4400, 3: L.mbx_pack_ambe3600x2450}[codec]
    want = np.zeros((n, FRAME_BYTES[codec]), dtype=np.uint8)
    assert host_pack(cells.ctypes.data, n, want.ctypes.data) == 0
    bad_frames = [0, 31, 32, 500, n - 1]
    dirty = cells.copy()
    for k, f in enumerate(bad_frames):
        dirty[f, (ncell - 1) if k % 2 else 3] = (2, -1, 77, 3, -128)[k]
    d_cells = torch.from_numpy(dirty).cuda()
    d_packed = torch.zeros((n, FRAME_BYTES[codec]), dtype=torch.uint8, device="cuda")
    d_status = torch.full((n,), 5, dtype=torch.int32, device="cuda")
    _native.check(L.mbx_pack_cells(codec, d_cells.data_ptr(), n, d_packed.data_ptr(), d_status.data_ptr(),
                                   torch.cuda.current_stream().cuda_stream), "mbx_pack_cells")
    status = d_status.cpu().numpy()
    got = d_packed.cpu().numpy()
    expect = np.zeros(n, dtype=np.int32)
    expect[bad_frames] = -2
    assert np.array_equal(status, expect)
    ok = status == 0
    assert np.array_equal(got[ok], want[ok])


def test_bench_rccl_code_path_runs_with_one_rank():
    """bench.py under torch.distributed.run with one rank and --force-dist: the process group is initialised on RCCL, the
    table blob goes through a device-tensor broadcast, timings through all_reduce, checksums through all_gather -- the
    code path of --gpus N, on the one GPU this box has.  (The N-rank launch itself is covered on CPU:
    tests/test_host_logic.py::test_bench_self_launch_starts_ranks_and_relays_rank0 and the gloo broadcast test.)"""
    import json
    import os
    import subprocess
    import sys

    import socket

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY=os.environ.get("HSA_ENABLE_IPC_MODE_LEGACY", "0"))
    with socket.socket() as sock:   # a free port for the rendezvous
        sock.bind(("127.0.0.1", 0))
        port = sock.getsockname()[1]
    r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "1", "--master-addr", "127.0.0.1",
                        "--master-port", str(port), os.path.join(root, "bench.py"), "--gpus", "1", "--force-dist", "--steps", "3", "--warmup", "1",
                        "--streams", "4096", "--no-cpu-baseline", "--no-extras"], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 1 and line["value"] > 0 and "process group initialised" in line["config"]["parallelism"]


def test_bench_default_line_keeps_its_contract(tmp_path):
    """`python bench.py` (the driver's call, shortened by --min-time-ms): ONE JSON line with the contract's keys -- the metric string
    with both halves, whole-job value, roofline {bound, achieved, peak, unit, frac, traffic}, cpu_baseline {value, unit, cores, kind,
    sample} and the parity object (no bound violated).  --steps IS the number of timed steps, and --dump-outputs leaves the last
    timed step's outputs as float arrays of at most 64 MB."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--steps", "5", "--warmup", "2", "--min-time-ms", "20",
                        "--dump-outputs", str(tmp_path / "dump")], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.strip()]
    assert len(lines) == 1 and lines[0].startswith("{"), lines[:3]
    assert len(lines[0]) <= 4096, len(lines[0])   # the driver keeps the tail of stdout: a 20 KB line was not parsed (round 5)
    assert r.stderr.strip() == "" or "amdgpu.ids" in r.stderr or len(r.stderr) < 2000, r.stderr[-500:]
    d = json.loads(lines[0])
    detail = json.load(open(os.path.join(root, d["detail"])))   # everything else: the sidecar next to bench.py
    assert detail["value"] == pytest.approx(d["value"], rel=1e-5) and "cpu_baselines" in detail and "host_path" in detail
    assert set(d["other_configs"]) == set(detail["other_configs"]) and all(
        set(v) == {"value", "ms_per_step", "kernel", "kernel_ms", "frac"} for v in d["other_configs"].values())
    assert "frames/sec" in d["metric"] and "PCM RMS error vs reference" in d["metric"]
    assert d["unit"] and d["n_gpus"] == 1 and d["steps"] == 5 and d["warmup"] == 2 and d["higher_is_better"] is True and d["scaling"] == "weak"
    assert d["steps_effective"] == 5 and detail["roofline"]["kernel_ms_stats"]["launches"] == 5
    assert d["value"] > 1e7 and abs(d["ms_per_step"] * 1e-3 * d["value"] / d["config"]["frames_per_step"] - 1.0) < 0.02
    assert "vs_baseline" in d and d["dtype"] and "synthetic" in d["data"] and "workload" in d["config"] and "model" not in d["config"]
    rf = d["roofline"]
    assert rf["bound"] in ("hbm", "mfma") and rf["unit"] in ("GB/s", "TFLOP/s") and rf["peak"] > 0 and "traffic" in rf
    assert abs(rf["frac"] - rf["achieved"] / rf["peak"]) < 1e-9 and 0.2 < rf["frac"] < 1.0 and rf["kernel"] == "imbe_one_launch_kernel"
    cb = d["cpu_baseline"]
    assert cb["value"] > 0 and cb["unit"] and cb["cores"] >= 1 and cb["kind"] in ("reference", "port") and cb["sample"]
    par = d["parity"]
    assert "FAILED" not in par and par["rel_rms"] <= 1e-4 and par["results_exact"] and par["state_in_tolerance"] and par["streams_checked"] >= 256
    for oc in detail["other_configs"].values():   # the other configs' own parity legs, if they ran one, hold the same bounds
        assert "FAILED" not in (oc.get("parity") or {})
    dump = {f[:-4]: np.load(tmp_path / "dump" / f) for f in os.listdir(tmp_path / "dump")}
    assert set(dump) == {"pcm16", "results", "records", "state", "rng"} and sum(a.nbytes for a in dump.values()) <= 64e6
    assert all(a.dtype in (np.float32, np.float64) for a in dump.values())
    assert dump["pcm16"].shape == (65536, 160) and dump["results"].shape == (65536, 5) and dump["records"].shape == (65536, 4)
    assert dump["state"].shape == (512, 3, 651) and dump["rng"].shape == (512, 5)
    assert np.abs(dump["pcm16"]).max() > 1000 and (dump["pcm16"] == np.round(dump["pcm16"])).all()   # voiced speech, int16 values


def test_bench_dumped_outputs_repeat_from_run_to_run(tmp_path):
    """bench.py --dump-outputs with the same arguments twice: the same arrays, value for value -- frames, seeds and the number of
    launches in front of the last timed step depend on the arguments only.  One T = 1 shape dumped whole and one whose frames and
    streams are sampled."""
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ)
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    for workload, frames in (("imbe_voiced", 65536), ("ambe_stream", 65536)):
        for run in ("a", "b"):
            r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--workload", workload, "--steps", "3", "--warmup", "1",
                                "--no-cpu-baseline", "--no-extras", "--dump-outputs", str(tmp_path / workload / run)],
                               capture_output=True, text=True, timeout=900, env=env)
            assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        names = sorted(os.listdir(tmp_path / workload / "a"))
        assert names == sorted(os.listdir(tmp_path / workload / "b")) == ["pcm16.npy", "records.npy", "results.npy", "rng.npy", "state.npy"]
        for f in names:
            a, b = np.load(tmp_path / workload / "a" / f), np.load(tmp_path / workload / "b" / f)
            assert a.dtype == b.dtype and a.shape == b.shape and np.array_equal(a, b, equal_nan=True), (workload, f)
        assert np.load(tmp_path / workload / "a" / "pcm16.npy").shape == (frames, 160)


def test_bench_two_ranks_self_launched_on_one_card():
    """`python bench.py --gpus 2` from a plain shell: bench.py starts the two ranks itself (no launcher), they shard the
    streams, run, meet at the barriers and rank 0 prints the line.  This box has one GPU, so both ranks use device 0
    (MBX_BENCH_SHARE_GPU=1) and the collectives go over gloo -- RCCL refuses two ranks on one device; its code path is
    covered with one rank in test_bench_rccl_code_path_runs_with_one_rank."""
    import json
    import os
    import subprocess
    import sys

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    env = dict(os.environ, MBX_BENCH_SHARE_GPU="1")
    for k in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT"):
        env.pop(k, None)
    r = subprocess.run([sys.executable, os.path.join(root, "bench.py"), "--gpus", "2", "--dist-backend", "gloo", "--steps", "3", "--warmup", "1",
                        "--streams", "8192", "--no-cpu-baseline", "--no-extras"], capture_output=True, text=True, timeout=900, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    line = json.loads([x for x in r.stdout.splitlines() if x.startswith("{")][-1])
    assert line["n_gpus"] == 2 and line["config"]["frames_per_step"] == 2 * 8192 and line["value"] > 0


def test_launchers_are_graph_capturable(mbx, oracle):
    """include/mbx.h: the launchers never synchronise and never allocate once the stream's expand workspace has been sized,
    so a tick can be captured into a HIP graph and replayed.  One AMBE+2 tick (FEC + expand + stream kernel, i.e. the path
    that uses the workspace) is captured on a side stream after mbx_reserve_stream(); three replays equal three eager
    ticks on a second decoder.  Without the reservation the capture is refused instead of synchronising mid-capture."""
    import torch

    from mbelib_neo_amd import _native, decoder, framegen

    L = _native.lib()
    codec, S = 1, 2048
    frames = framegen.random_frames(codec, S, framegen.rng_for(77))
    seeds = np.arange(S) + 9
    eager = decoder.BatchDecoder(codec, S, seeds=seeds)
    want = []
    for _ in range(3):
        o = eager.decode(frames, 1, want_float=True)
        want.append((o["pcm16"].clone(), o["pcmf"].clone()))
    torch.cuda.synchronize()

    dec = decoder.BatchDecoder(codec, S, seeds=seeds)
    d_frames = dec.to_device(frames)
    out = dec.make_outputs(1, want_float=True)
    side = torch.cuda.Stream()
    args = (codec, S, 1, d_frames.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(),
            out["results"].data_ptr(), out["records"].data_ptr())
    g = torch.cuda.CUDAGraph()
    refused = torch.cuda.CUDAGraph()
    with torch.cuda.graph(refused, stream=side):   # nothing reserved for this stream yet: growth during capture is refused
        rc = L.mbx_process_batch(*args, side.cuda_stream)
    assert rc == -1 and b"capture" in L.mbx_last_error()
    _native.check(L.mbx_reserve_stream(side.cuda_stream, S), "mbx_reserve_stream")
    with torch.cuda.graph(g, stream=side):
        rc = L.mbx_process_batch(*args, side.cuda_stream)
    assert rc == 0
    for k in range(3):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["pcm16"], want[k][0]) and torch.equal(out["pcmf"], want[k][1]), f"replay {k}"
    assert dec.state_numpy().tobytes() == eager.state_numpy().tobytes()


# ---- the int16 tail ------------------------------------------------------------------------------
def test_tail_cases_through_hip(mbx, oracle, golden_dir):
    """The frames of tests/golden/tail_cases.npz (largest HIP-vs-oracle int16 differences in 94 M samples, all in clipped
    frames) decoded again by the HIP path: within the stated bound of the oracle, and no further from it than when found."""
    from mbelib_neo_amd.layout import init_state, rng_seeded

    fx = np.load(os.path.join(golden_dir, "tail_cases.npz"))
    for k in range(int(fx["n"])):
        codec, t, seed, diff = (int(x) for x in fx[f"c{k}_meta"])
        frames = fx[f"c{k}_frames"].reshape(t + 1, -1)
        got = _host_batch(mbx, codec, 1, t + 1, frames, init_state(1), rng_seeded([seed]))
        g16 = np.asarray(got["pcm16"]).reshape(t + 1, 160)[t].astype(np.int32)
        d = int(np.abs(g16 - fx[f"c{k}_oracle"].astype(np.int32)).max())
        peak = oracle.process_batch(codec, 1, t + 1, frames, oracle.init_state(1), oracle.rng_seeded([seed]))["peak"][t]
        assert d <= parity.INT16_MAX_LSB_CLIPPED and d <= int(parity.int16_bound(peak)), (k, d, float(peak))
        assert d <= max(diff, 3), (k, d, diff)
        assert d <= int(np.abs(fx[f"c{k}_ref_fma"].astype(np.int32) - fx[f"c{k}_ref_ieee"].astype(np.int32)).max())


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_int16_tail_over_ten_million_samples(mbx, oracle, codec):
    """65,536 random-bit frames (4,096 streams x 16) = 10.5 M samples per codec against the oracle: the whole distribution
    of the int16 difference, not only its bulk -- >= 99.99 % within 1 LSB, at most 3 LSB below the clip, at most 6 inside
    clipped frames, and nothing beyond 2 LSB outside clipped frames in practice."""
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    S, T = 4096, 16
    frames = framegen.random_frames(codec, S * T, framegen.rng_for(5150 + codec))
    seeds = [99 + 7 * s for s in range(S)]
    ref = oracle.process_batch(codec, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    got = _host_batch(mbx, codec, S, T, frames, init_state(S), rng_seeded(seeds))
    parity.check_results(ref["results"], got["results"])
    m = parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
    d = np.abs(np.asarray(ref["pcm16"], dtype=np.int32).reshape(-1) - np.asarray(got["pcm16"], dtype=np.int32).reshape(-1))
    assert d.size >= 10_000_000
    assert float(np.mean(d <= 1)) >= 0.9999
    print(f"codec {codec} tail:", m, np.bincount(np.minimum(d, 7), minlength=8).tolist())


@pytest.mark.parametrize("name", ["ambe_fec", "ambe_fec_resident", "imbe_voiced"])
def test_replayed_frame_workloads_hold_the_int16_bound(mbx, oracle, name):
    """bench.py's T = 1 workloads repeat ONE frame per stream, launch after launch, for thousands of launches; the AMBE+2 ones drive
    their prediction far beyond the output range (pre-clip peaks of several 1e5) and showed up to 8 LSB against the oracle in frames
    at the clip, depending on which launch the timed region ended on (profiles/r05/parity_by_replay_length.log).  Here the same
    workloads (bench.make_frames, the bench's kernel instances: 4,096 streams, one launch per tick) run for 2,300 launches and a
    strided sample of 64 streams is compared with the oracle at eight launches along the way -- the ones that log names and the
    last -- under THE bound of tests/parity.py: per frame int16_bound(pre-clip peak), float criteria, results exact.  Checker: oracle."""
    import sys

    import torch

    sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    import bench
    from mbelib_neo_amd import _native, decoder
    from mbelib_neo_amd.layout import FRAME_BYTES, RESULT_DTYPE

    codec, _, T, _ = bench.WORKLOADS[name]
    S, n_launch, resident = 4096, 2300, name.endswith("_resident")
    marks = [353, 382, 954, 1055, 2000, 2249, 2299, 2300]
    frames = bench.make_frames(name, codec, S, T, rank=0)
    seeds = np.arange(S) + 1234
    dec = decoder.BatchDecoder(codec, S, seeds=seeds, resident=resident)
    kernel = _native.lib().mbx_batch_kernel_name(codec, S, T, 1 if resident else 0).decode()
    assert "one_launch" in kernel or os.environ.get("MBX_FUSE_ONE") in ("0", "1"), kernel   # (tools/test_env_matrix.sh: the other T = 1 forms)
    d_frames = dec.to_device(frames)
    out = dec.make_outputs(T, want_pcm16=True, want_float=True, want_results=True)
    pick = np.arange(S // 128, S, S // 64)[:64]
    d_pick = torch.from_numpy(pick).cuda()
    seen = {}
    for k in range(1, n_launch + 1):
        dec.decode(d_frames, T, out=out)
        if k in marks:
            seen[k] = tuple(out[x].reshape(S, -1)[d_pick].cpu().numpy() for x in ("pcm16", "pcmf", "results"))
    state = dec.state_numpy()[pick]
    fb = FRAME_BYTES[codec]
    hist = np.ascontiguousarray(np.tile(np.asarray(frames).reshape(S, T, fb)[pick], (1, n_launch, 1))).reshape(-1, fb)
    ref = oracle.process_batch(codec, len(pick), n_launch, hist, oracle.init_state(len(pick)), oracle.rng_seeded(seeds[pick]))
    r16, rf = ref["pcm16"].reshape(len(pick), n_launch, 160), ref["pcmf"].reshape(len(pick), n_launch, 160)
    rres, peak = ref["results"].reshape(len(pick), n_launch), ref["peak"].reshape(len(pick), n_launch)
    worst = {}
    for k in marks:
        g16, gf, gres = seen[k]
        parity.check_results(rres[:, k - 1], np.ascontiguousarray(gres).view(RESULT_DTYPE).reshape(-1), what=f"{name} launch {k}")
        m = parity.check_pcm(rf[:, k - 1], gf, r16[:, k - 1], g16, peak=peak[:, k - 1], what=f"{name} launch {k}")
        worst[k] = (m["int16_max"], m["int16_margin"], float(peak[:, k - 1].max()))
    parity.check_state(ref["state"], state)
    print(name, "launch: (int16 max, margin to the bound, largest pre-clip peak)", worst)


# ---- AMBE+2 frame classes inside LDS-resident launches ---------------------------------------------------------------
def _ambe_class_frames(classes, rng):
    """clean AMBE+2 wire frames of the given classes: 'v' voice, 't' valid tone, 'i' tone frame with an invalid id,
    'e' erasure (ref src/ambe/ambe3600x2450.c:176-240 classification)"""
    from mbelib_neo_amd import framegen

    n = len(classes)
    bits = framegen.ambe_voice_param_bits(n, rng)
    for k, c in enumerate(classes):
        if c in "ti":
            bits[k, 0:6] = 1                       # u0 >> 6 == 63: the tone signature ...
            bits[k, 45:49] = 0                     # ... with u3 & 0xf == 0
            tone_id = int(rng.integers(7, 123)) if c == "t" else int(rng.choice([0, 3, 124, 127, 200, 255]))
            for j in range(8):
                bits[k, 12 + j] = (tone_id >> (7 - j)) & 1
        elif c == "e":
            bits[k, 0:4] = 1                       # b0 = 120..123
            bits[k, 4] = 0                         # (not the tone signature)
            bits[k, 37] = 0
    return framegen.encode_ambe3600x2450(bits)


def test_ambe_tone_and_erasure_classes_in_lds_resident_launches(mbx, oracle):
    """prev_mp_enhanced has no LDS home in the LDS-resident AMBE instances: it travels in registers and is written to HBM
    only around tone-class frames (mbx_stream.hip, `synced`).  Scripted class sequences -- a tone as the very first frame
    of a stream, invalid tones (which replay prev_mp_enhanced whole) before and after voice, runs of invalid tones,
    erasures in between -- as ONE launch of T = 12 (LDS-resident) against the oracle and against twelve T = 1 launches
    (HBM-slot instance): integer state and results exact, PCM in tolerance, both instances bit-identical."""
    from mbelib_neo_amd import framegen
    from mbelib_neo_amd.layout import init_state, rng_seeded

    rng = framegen.rng_for(4711)
    scripts = ["tvvivvtvvevv", "ivvvvvvvvvvv", "vvviiivvtvie", "evtvivvvviiv", "vvvvvvvvvvvi", "tttvvviveevi", "viviviviviei", "vvetvivtveiv"]
    S, T = 256, 12
    rows = []
    for s_ in range(S):
        sc = scripts[s_ % len(scripts)] if s_ < 64 else "".join(rng.choice(list("vvvvvtie"), size=T))
        rows.append(_ambe_class_frames(sc, rng))
    frames = np.stack(rows).reshape(S * T, 9)
    seeds = [4000 + s_ for s_ in range(S)]
    ref = oracle.process_batch(1, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    flags = np.asarray(ref["results"]["flags"])
    assert (flags & 0x10).any() and (flags & 0x20).any()   # tone and erasure frames are really there
    got = _host_batch(mbx, 1, S, T, frames, init_state(S), rng_seeded(seeds))
    parity.check_results(ref["results"], got["results"])
    parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"])
    parity.check_state(ref["state"], got["state"])
    assert np.array_equal(ref["rng"], got["rng"])
    # the same streams tick by tick (T = 1: the HBM-slot instance)
    state, rg = init_state(S), rng_seeded(seeds)
    pcm = np.zeros((S, T, 160), dtype=np.int16)
    fr = frames.reshape(S, T, 9)
    for t in range(T):
        out = _host_batch(mbx, 1, S, 1, np.ascontiguousarray(fr[:, t]), state, rg)
        state, rg = out["state"], out["rng"]
        pcm[:, t] = np.asarray(out["pcm16"]).reshape(S, 160)
    assert np.array_equal(pcm.reshape(-1, 160), np.asarray(got["pcm16"]).reshape(-1, 160))
    assert np.array_equal(np.asarray(state).view(np.uint8), np.asarray(got["state"]).view(np.uint8))


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_resident_state_is_bit_identical_to_the_abi_triplets(mbx, oracle, codec):
    """Resident launches (mbx_process_batch_resident: prev_mp_enhanced elided while it equals cur_mp, prev_mp fetched lazily;
    what sessions and the queue mode's device pool use) against the drop-in launcher on the same frames: launches of
    T = 1, 1, 2, 4, 1, 3, 16, 1 frames per stream in a row -- random channel bits (repeats, mutes, headroom resets; AMBE: erasures
    and tone classes by chance) and, for AMBE+2, scripted tone / invalid-tone / erasure sequences.  PCM and results must be
    bit-identical launch by launch, and the materialised triplets bit-identical to the ones mbx_process_batch leaves -- after
    every launch, i.e. from every mix of elided / whole structs.  ref include/mbelib-neo/mbelib.h:88-139 (the three structs)."""
    import torch
    from mbelib_neo_amd import decoder, framegen
    from mbelib_neo_amd.layout import FRAME_BYTES

    S = 768
    fb = FRAME_BYTES[codec]
    plan = [1, 1, 2, 4, 1, 3, 16, 1]
    total = sum(plan)
    rng = framegen.rng_for(900 + codec)
    frames = framegen.random_frames(codec, S * total, rng).reshape(S, total, fb)
    if codec == 1:   # scripted classes on the first 256 streams: every tone / erasure transition around launch boundaries
        for s_ in range(256):
            frames[s_] = _ambe_class_frames("".join(rng.choice(list("vvvtie"), size=total)), rng)
    seeds = np.arange(S) + 31
    a = decoder.BatchDecoder(codec, S, seeds=seeds)
    b = decoder.BatchDecoder(codec, S, seeds=seeds, resident=True)
    t0 = 0
    for k, T in enumerate(plan):
        chunk = np.ascontiguousarray(frames[:, t0:t0 + T]).reshape(-1, fb)
        oa = a.decode(chunk, T, want_float=True)
        ob = b.decode(chunk, T, want_float=True)
        torch.cuda.synchronize()
        assert torch.equal(oa["pcm16"], ob["pcm16"]), f"launch {k} (T={T}): int16 PCM differs"
        assert oa["pcmf"].cpu().numpy().tobytes() == ob["pcmf"].cpu().numpy().tobytes(), f"launch {k} (T={T}): float PCM differs"
        assert torch.equal(oa["results"], ob["results"]), f"launch {k} (T={T}): results differ"
        if k % 2 == 1 or k == len(plan) - 1:   # materialise only now and then: the elided form must survive several launches
            elided = int((b.resident != 0).sum().item())
            sa, sb = a.state_numpy(), b.state_numpy()
            assert int((b.resident != 0).sum().item()) == 0
            assert sa.tobytes() == sb.tobytes(), f"after launch {k}: state triplets differ ({elided} streams were elided)"
            assert a.rng_numpy().tobytes() == b.rng_numpy().tobytes()
        t0 += T
    assert elided > S // 2, "the resident form was hardly exercised"


# ---- multi-GPU readiness -----------------------------------------------------------------------------
def test_c_abi_rccl_table_broadcast_every_visible_device(mbx):
    """The C library's own collective (mbx_comm_* / mbx_init_broadcast / mbx_comm_agree: ncclBroadcast of the table blob + min/max
    all-reduce of the per-rank checksums) with ONE RANK PER VISIBLE DEVICE, one host thread each, in this process: rank 0 passes
    the blob, every other rank an empty buffer that must come back filled with it; every rank ends initialised with the same
    checksum.  Then the failure paths, which must RETURN on every rank instead of hanging: a rank that passes a different value to
    mbx_comm_agree (needs >= 2 devices), and a root whose blob is corrupt (mbx_init refuses it on every rank: the ranks still meet
    in the agreement).  On a one-GPU box this is the one-rank case; on the first multi-GPU box it runs the non-root and mismatch
    branches without anyone editing it.  RCCL is bound at run time; libmbx_hip.so must not carry a link-time dependency on it."""
    import ctypes as C
    import subprocess
    import threading

    import torch
    from mbelib_neo_amd import _native
    MBX_EBADTABLE = -102   # include/mbx.h

    L = _native.lib()
    needed = subprocess.run(["objdump", "-p", _native.library_path()], capture_output=True, text=True).stdout
    assert "librccl" not in needed
    blob = bytes(mbx.load_tables_blob())
    N = torch.cuda.device_count()
    ident = C.create_string_buffer(128)
    _native.check(L.mbx_comm_unique_id(ident), "mbx_comm_unique_id")
    out = [dict() for _ in range(N)]

    def rank_main(r):
        o = out[r]
        try:
            comm = C.c_void_p()
            o["init"] = L.mbx_comm_init(C.byref(comm), N, ident, r, r)
            if o["init"] < 0:
                return
            buf = C.create_string_buffer(blob if r == 0 else bytes(len(blob)), len(blob))
            minmax = (C.c_uint32 * 2)()
            o["bcast"] = L.mbx_init_broadcast(comm, 0, r, buf, len(blob), minmax, None)
            o["blob_ok"] = buf.raw == blob
            o["minmax"] = (minmax[0], minmax[1])
            o["checksum"] = L.mbx_table_checksum()   # (of the calling thread's current device: set by mbx_init_broadcast)
            o["agree_same"] = L.mbx_comm_agree(comm, 7, minmax, None)
            o["agree_diff"] = L.mbx_comm_agree(comm, 7 if r + 1 < N or N == 1 else 8, minmax, None)
            o["agree_diff_minmax"] = (minmax[0], minmax[1])
            bad = bytearray(blob if r == 0 else bytes(len(blob)))
            if r == 0:
                bad[len(bad) // 2] ^= 0x40   # the root's copy is corrupt: what arrives fails mbx_init's checksum test on every rank
            buf2 = C.create_string_buffer(bytes(bad), len(bad))
            o["bcast_bad"] = L.mbx_init_broadcast(comm, 0, r, buf2, len(blob), minmax, None)
            o["bad_args"] = (L.mbx_init_broadcast(comm, N, r, buf, len(blob), minmax, None),       # root outside the communicator
                             L.mbx_init_broadcast(comm, 0, r, buf, len(blob) - 4, minmax, None))   # not a table blob
            o["destroy"] = L.mbx_comm_destroy(comm)
        except Exception as e:   # noqa: BLE001
            o["exception"] = repr(e)

    threads = [threading.Thread(target=rank_main, args=(r,)) for r in range(N)]
    for t in threads:
        t.start()
    for t in threads:
        t.join(timeout=240)
    assert not any(t.is_alive() for t in threads), f"a rank is stuck in a collective: {out}"
    sums = {o.get("checksum") for o in out}
    for r, o in enumerate(out):
        assert "exception" not in o, (r, o)
        assert o["init"] == 0 and o["bcast"] == 0 and o["blob_ok"], (r, o)
        assert o["minmax"][0] == o["minmax"][1] == o["checksum"] != 0, (r, o)
        assert o["agree_same"] == 0, (r, o)
        if N > 1:
            assert o["agree_diff"] == MBX_EBADTABLE and o["agree_diff_minmax"] == (7, 8), (r, o)   # on EVERY rank
        else:
            assert o["agree_diff"] == 0
        assert o["bcast_bad"] < 0, (r, o)                                   # every rank returns, none hangs
        assert o["bad_args"][0] < 0 and o["bad_args"][1] < 0 and o["destroy"] == 0, (r, o)
    assert len(sums) == 1
    torch.cuda.set_device(0)   # (mbx_init refuses a corrupt blob before it touches the device's context: the good tables are still there)
    assert L.mbx_table_checksum() == out[0]["checksum"]


def test_collective_control_flow_with_thread_ranks(mbx, tmp_path):
    """mbx_init_broadcast / mbx_comm_agree with N = 2, 4 and 8 RANKS on the one GPU of a test box: the ranks are host threads of a
    child process and RCCL is tests/fake_rccl.c (bound through MBX_RCCL_LIBRARY), whose collectives are rendezvous of those threads
    around plain device copies -- real RCCL refuses two ranks on one device, so before this test the non-root, mismatch and
    failed-rank branches of csrc/mbx_collective.hip had never run.  Checked: (a) every non-root rank receives the blob (root 0 and
    root N - 1) and all end with one checksum; (b) a different value on one rank makes mbx_comm_agree return MBX_EBADTABLE with
    (min, max) = (7, 8) on EVERY rank; (c) one rank's copy of the blob arrives corrupted -> that rank's mbx_init refuses it and every
    rank returns MBX_EBADTABLE; (d) one rank's ncclBroadcast fails -> it reports its own error, the others MBX_EBADTABLE, nobody
    hangs.  NOT a scaling measurement: no multi-GPU box has been available.
    ref include/mbelib-neo/mbelib.h:28-30 (threading contract: per-thread state, re-entrant per stream)."""
    import json
    import subprocess
    import sys

    MBX_EBADTABLE, MBX_ENODEVICE = -102, -100   # include/mbx.h
    here = os.path.dirname(os.path.abspath(__file__))
    fake = str(tmp_path / "libfake_rccl.so")
    subprocess.check_call(["gcc", "-shared", "-fPIC", "-O1", "-D__HIP_PLATFORM_AMD__", "-I/opt/rocm/include", os.path.join(here, "fake_rccl.c"),
                           "-L/opt/rocm/lib", "-lamdhip64", "-lpthread", "-Wl,-rpath,/opt/rocm/lib", "-o", fake])

    def run(n, root, **inject):
        env = dict(os.environ, MBX_RCCL_LIBRARY=fake)
        env.update({k: str(v) for k, v in inject.items()})
        p = subprocess.run([sys.executable, os.path.join(here, "rccl_thread_ranks.py"), str(n), str(root)], env=env, capture_output=True,
                           text=True, timeout=300)
        assert p.returncode == 0, (p.returncode, p.stdout[-600:], p.stderr[-600:])
        d = json.loads(p.stdout.strip().splitlines()[-1])
        assert not any(d["stuck"]), d
        for r, o in enumerate(d["ranks"]):
            assert "exception" not in o and o["init"] == 0 and o["destroy"] == 0, (r, o)
        return d

    for n in (2, 4, 8):
        for root in (0, n - 1):
            d = run(n, root)
            for r, o in enumerate(d["ranks"]):
                assert o["bcast"] == 0 and o["blob_ok"], f"n={n} root={root} rank={r}: {json.dumps(o)}"
                assert o["minmax"][0] == o["minmax"][1] == d["checksum"] != 0, (n, root, r, o)
                assert o["agree_same"] == 0, (n, root, r, o)
                assert o["agree_diff"] == MBX_EBADTABLE and tuple(o["agree_diff_minmax"]) == (7, 8), (n, root, r, o)
        d = run(n, 0, FAKE_RCCL_CORRUPT_RANK=1)
        for r, o in enumerate(d["ranks"]):
            assert o["bcast"] == MBX_EBADTABLE, (n, r, o)                    # on EVERY rank: the corrupted one by mbx_init, the others by the agreement
            assert o["blob_ok"] == (r != 1), (n, r, o)
            assert o["agree_same"] == 0, (n, r, o)                           # the communicator is still usable afterwards
        d = run(n, 0, FAKE_RCCL_FAIL_BCAST_RANK=n - 1)
        for r, o in enumerate(d["ranks"]):
            assert o["bcast"] == (MBX_ENODEVICE if r == n - 1 else MBX_EBADTABLE), (n, r, o)
            assert o["agree_same"] == 0, (n, r, o)


def test_every_visible_device_decodes(mbx, oracle):
    """One context per device: every device torch can see (one on the test box, eight on a node) is initialised and decodes
    a small batch against the oracle -- device index > 0 is exercised the moment a box has it."""
    import torch

    from mbelib_neo_amd import decoder, framegen

    S, T = 64, 4
    frames = framegen.random_frames(0, S * T, framegen.rng_for(8080))
    seeds = np.arange(S) + 5
    ref = oracle.process_batch(0, S, T, frames, oracle.init_state(S), oracle.rng_seeded(seeds))
    for dev in range(torch.cuda.device_count()):
        dec = decoder.BatchDecoder(0, S, device=dev, seeds=seeds)
        out = dec.decode(frames, T, want_float=True)
        torch.cuda.synchronize(dev)
        parity.check_results(ref["results"], decoder.results_numpy(out["results"]))
        parity.check_pcm(ref["pcmf"], out["pcmf"].cpu().numpy(), ref["pcm16"], out["pcm16"].cpu().numpy())
        parity.check_state(ref["state"], dec.state_numpy())
    torch.cuda.set_device(0)


def test_ambe_rows_from_a_workspace_equal_in_kernel_expansion(mbx, oracle):
    """T >= 4 AMBE launches expand the records inside the stream kernel (eight frames of a stream at a time); the same
    kernel still accepts FrameParams rows made by mbx_expand_records (mbx_stream_expanded).  Both ways, both AMBE codecs:
    identical PCM, results and state."""
    import torch

    from mbelib_neo_amd import _native, decoder, framegen

    L = _native.lib()
    S, T = 256, 11   # T not a multiple of eight: the last group of rows is partial
    for codec in (1, 3):
        frames = framegen.random_frames(codec, S * T, framegen.rng_for(6060 + codec))
        outs = []
        for split in (False, True):
            dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) + 9)
            d_frames = dec.to_device(frames)
            out = dec.make_outputs(T, want_pcm16=True, want_float=True, want_results=True)
            stream = torch.cuda.current_stream().cuda_stream
            _native.check(L.mbx_fec_ambe3600x2450(d_frames.data_ptr(), S * T, out["records"].data_ptr(), stream), "fec")
            if split:
                assert L.mbx_uses_expand_launch(codec, S, T) == 0
                _native.check(L.mbx_expand_records(codec, out["records"].data_ptr(), S * T, stream), "expand")
                run = L.mbx_stream_expanded
            else:
                run = L.mbx_process_records
            _native.check(run(codec, S, T, out["records"].data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(),
                              out["pcmf"].data_ptr(), out["results"].data_ptr(), stream), "stream")
            torch.cuda.synchronize()
            outs.append((out["pcmf"].cpu().numpy().tobytes(), out["pcm16"].cpu().numpy().tobytes(), out["results"].cpu().numpy().tobytes(),
                         dec.state.cpu().numpy().tobytes()))
        assert outs[0] == outs[1], f"codec {codec}"


def test_single_frame_kernel_equals_batch_launch(mbx, oracle):
    """mbx_process_frame (one launch of one wavefront: FEC by lane 0 + the LDS-resident stream body + completion word) against
    mbx_process_batch with S = T = 1 on the same frames and state, all four codecs, twenty frames of one stream each: PCM,
    result, record and the three structs bit for bit; the completion word carries the token."""
    import torch

    from mbelib_neo_amd import _native, framegen
    from mbelib_neo_amd.layout import FRAME_BYTES, init_state, rng_seeded

    L = _native.lib()
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream().cuda_stream
    for codec in (0, 1, 2, 3):
        T = 20
        frames = framegen.random_frames(codec, T, framegen.rng_for(7000 + codec))
        if codec in (1, 3):
            frames[::2] = framegen.encode_ambe3600x2450(framegen.ambe_voice_param_bits(T // 2, framegen.rng_for(7100 + codec)))
        d_frames = torch.from_numpy(np.ascontiguousarray(frames).reshape(-1)).to(dev)
        fb = FRAME_BYTES[codec]

        def fresh():
            st = torch.from_numpy(init_state(1).view(np.uint8).reshape(-1).copy()).to(dev)
            rg = torch.from_numpy(rng_seeded([4321]).view(np.uint8).reshape(-1).copy()).to(dev)
            return st, rg

        outs = []
        for single in (True, False):
            st, rg = fresh()
            pcm16 = torch.zeros((T, 160), dtype=torch.int16, device=dev)
            pcmf = torch.zeros((T, 160), dtype=torch.float32, device=dev)
            res = torch.zeros((T, 5), dtype=torch.int32, device=dev)
            rec = torch.zeros((T, 4), dtype=torch.int32, device=dev)
            done = torch.zeros(1, dtype=torch.int32, device=dev)
            for t in range(T):
                fptr = d_frames.data_ptr() + t * fb
                if single:
                    _native.check(L.mbx_process_frame(codec, fptr, st.data_ptr(), rg.data_ptr(), pcm16[t].data_ptr(), pcmf[t].data_ptr(),
                                                      res[t].data_ptr(), rec[t].data_ptr(), done.data_ptr(), 1000 + t, stream), "mbx_process_frame")
                else:
                    _native.check(L.mbx_process_batch(codec, 1, 1, fptr, st.data_ptr(), rg.data_ptr(), pcm16[t].data_ptr(), pcmf[t].data_ptr(),
                                                      res[t].data_ptr(), rec[t].data_ptr(), stream), "mbx_process_batch")
            torch.cuda.synchronize()
            if single:
                assert int(done.item()) == 1000 + T - 1
            outs.append(tuple(x.cpu().numpy().tobytes() for x in (pcm16, pcmf, res, rec, st, rg)))
        for a, b, name in zip(outs[0], outs[1], ("pcm16", "pcmf", "results", "records", "state", "rng")):
            assert a == b, f"codec {codec}: {name}"
