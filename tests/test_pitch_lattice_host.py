"""Host test (no GPU): the pitch-pair lattices of tests/pitch_lattice.py hold, in the ORACLE's decode, what the GPU tests of
tests/test_gpu_pitch_lattice.py rely on -- every (L_prev, L_cur) pair, both sides of the stability test, the voicing patterns, the
repeats of the invalid fundamentals, every AMBE frame class before and behind a voice frame, at least 70 % of the frames below the
soft clip -- and the IMBE 7100x4400 encoder is the inverse of the oracle's front end.  The oracle's decodes are cached in
pitch_lattice (per codec, pattern and variant)."""
import numpy as np
import pytest

import instance_cases
import pitch_lattice
import silent_store_cases


@pytest.mark.parametrize("codec,pattern", pitch_lattice.LATTICES)
def test_the_lattice_holds_what_the_gpu_tests_rely_on(codec, pattern):
    lat = pitch_lattice.build(codec, pattern)
    N, S = lat.N, lat.frames.shape[0]
    assert S == pitch_lattice.build_size(codec, pattern) and S <= 65536
    s = np.arange(N * N)
    assert np.array_equal(lat.b0[:N * N, 0], s // N) and np.array_equal(lat.b0[:N * N, 1], s % N)
    figures = pitch_lattice.composition(codec, pattern, pitch_lattice.decode(codec, pattern))
    print(codec, pattern, figures)
    if codec in (0, 2):   # the same fundamentals, so the same pairs on either side of the stability test, whatever the pattern
        assert figures["equal_w0"] == pitch_lattice.IMBE_VALID_B0 and figures["L_pairs"] == 48 * 48


def test_two_generations_of_a_lattice_are_the_same_bytes():
    first = pitch_lattice.build(3, "rr").frames.copy()
    pitch_lattice.build.cache_clear()
    assert pitch_lattice.build(3, "rr").frames.tobytes() == first.tobytes()


@pytest.mark.parametrize("codec", [0, 2])
def test_imbe_encoders_are_the_inverse_of_the_oracles_front_end(oracle, codec):
    silent_store_cases.check_encoder(codec, oracle)


def test_imbe7100_lattice_decodes_frame_by_frame_to_the_bits_it_was_made_of(oracle):
    """131,072 frames of the 7100x4400 lattice through the oracle's front end alone: no error, the parameter bits in 7200x4400 order"""
    import oracle_lib

    lat = pitch_lattice.build(2, "rr")
    rec = oracle.fec_batch(2, lat.frames.reshape(-1, 18))
    assert np.array_equal(oracle_lib.records_to_bits(rec, 88), lat.bits.reshape(-1, 88).astype(np.int8))
    assert not oracle_lib.records_to_results(rec)["total_errors"].any()


@pytest.mark.parametrize("codec,pattern", [(c, p) for c in sorted(pitch_lattice.QUAD_PATTERNS) for p in pitch_lattice.QUAD_PATTERNS[c]])
def test_the_quads_first_two_frames_decode_to_the_bytes_of_the_pair(codec, pattern):
    pair, quad = pitch_lattice.decode(codec, pattern), pitch_lattice.decode(codec, pattern, "quad")
    S = pair["state"].shape[0]
    f = pitch_lattice.frames(codec, pattern, "quad")
    assert f.shape[:2] == (S, 4) and np.array_equal(f[:, :2], pitch_lattice.frames(codec, pattern)) and np.array_equal(f[:, 2:], f[:, :2])
    for name in ("records", "results", "pcm16", "pcmf", "peak"):
        a, b = pair[name].reshape(S, 2, -1), quad[name].reshape(S, 4, -1)[:, :2]
        assert a.tobytes() == np.ascontiguousarray(b).tobytes(), name
    # ... and the third frame is p again on state the first two made: it is not a replay of the first
    assert pair["pcmf"].reshape(S, 2, 160)[:, 0].tobytes() != np.ascontiguousarray(quad["pcmf"].reshape(S, 4, 160)[:, 2]).tobytes()


def test_every_form_names_an_instance_the_instance_cases_know_and_the_table_is_whole():
    """the form table against the issue's: seven forms, 22 cells that are not n/a, every name one tests/instance_cases.py runs for
    that codec.  (That the launch plan picks each name at the lattice's S is tests/test_launch_plan_host.py's, on the CPU, and
    run_case's on the card.)"""
    cases = pitch_lattice.cases()
    assert len({c.id for c, _ in cases}) == len(cases)
    known = {(c.codec, c.name) for c in instance_cases.CASES}
    entries = {c.entry for c in instance_cases.CASES}
    for case, work in cases:
        assert (case.codec, case.name) in known, case
        assert case.entry in entries and not case.env and case.S * case.T <= 4 * 65536 and case.T * case.launches in (2, 4), case
        assert (work.variant == "quad") == (case.T == 4)
        assert case.S == pitch_lattice.build_size(case.codec, work.pattern)
    assert len({(c.codec, c.name, c.T) for c, _ in cases}) == sum(len(names) for *_, names in pitch_lattice.FORMS) == 22
    per_codec = {codec: sum(c.codec == codec for c, _ in cases) for codec in (0, 1, 2, 3)}
    # codec 0: five patterns on four one-frame forms and T = 2, two on the two quad forms; the others one lattice on their forms
    assert per_codec == {0: 5 * 5 + 2 * 2, 2: 3, 1: 6, 3: 6}


def _doctored(codec, pattern, variant):
    """the oracle's decode as `got` in the shapes run_case compares, for a test to damage"""
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

    ref = pitch_lattice.decode(codec, pattern, variant)
    got = {k: ref[k].copy() for k in ("records", "results", "pcm16", "pcmf", "state", "rng")}
    assert got["records"].dtype == RECORD_DTYPE and got["results"].dtype == RESULT_DTYPE
    return ref, got


def test_a_failure_of_each_comparison_names_the_pair():
    """a real mismatch through each comparison of run_case -- parity.check_exact (records, RNG), check_results, check_pcm inside
    parity.located, check_state and check_state_blocks -- under pitch_lattice.named: the message carries (b0_prev, b0_cur, pattern)
    and the two L; a frame comparison also says which b0 the frame carries, a comparison of what the last frame left does not"""
    import parity

    codec, pattern, T, N = 3, "rr", 2, 128
    s = 2 * N + 1                      # pair (2, 1)
    pair = "(b0_prev 2, b0_cur 1, rr; L "

    def message(check):
        with pytest.raises(AssertionError) as e:
            with pitch_lattice.named(codec, pattern, T):
                check()
        return str(e.value)

    ref, got = _doctored(codec, pattern, "pair")
    got["records"]["w"][s * T + 1, 0] ^= 1
    m = message(lambda: parity.check_exact(ref["records"], got["records"], "x: records", T))
    assert pair in m and "frame 1 carries b0 1" in m, m

    got["results"]["flags"][s * T] ^= 0x40
    def results():
        with parity.located(T):
            parity.check_results(ref["results"], got["results"], "x: results")
    m = message(results)
    assert pair in m and "frame 0 carries b0 2" in m, m

    got["pcm16"][s * T + 1, 7] += 9
    def pcm():
        with parity.located(T):
            parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"], what="x: pcm", peak=ref["peak"])
    m = message(pcm)
    assert pair in m and "frame 1 carries b0 1" in m, m

    got["state"]["L"][s, 0] += 1
    for check in (lambda: parity.check_state(ref["state"], got["state"], what="x: state (rows are streams)"),
                  lambda: parity.check_state_blocks(ref["state"], got["state"], block=256, what="x: state (rows are streams)")):
        m = message(check)
        assert pair in m and f"stream {s} " in m and "carries b0" not in m, m
    got["state"]["L"][s, 0] -= 1
    got["state"]["PSIl"][s] += np.float32(0.005) * np.abs(ref["state"]["PSIl"][s])   # a float field, 0.5 % off in one stream: the failure names the block's pairs
    m = message(lambda: parity.check_state_blocks(ref["state"], got["state"], block=256, what="x: state (rows are streams)"))
    assert "streams 256 = pair (b0_prev 2, b0_cur 0, rr; L " in m and "to 511 = pair (b0_prev 3, b0_cur 127, rr; L " in m, m
    # ... and over all streams at once the same damage is diluted below the bound: why the lattices compare block by block
    parity.check_state(ref["state"], got["state"], what="x: state")

    got["rng"]["unvoiced_seed_state"][s] ^= 1
    m = message(lambda: parity.check_exact(ref["rng"], got["rng"], "x: rng"))
    assert pair in m and "carries b0" not in m, m


def test_a_rim_frame_of_the_wrong_class_is_found():
    """composition holds every rim frame to the class it was scripted as: a rim whose generator made another class does not pass on
    the chance frames of that class in the N x N part"""
    lat = pitch_lattice.build(1, "rr")
    row = 128 * 128 + 5                # (valid tone, voice b0 5)
    assert lat.cls[row, 0] == "t" and lat.cls[row, 1] == "v"
    lat.cls[row, 0] = "e"
    try:
        with pytest.raises(AssertionError, match="not of the class they were scripted as"):
            pitch_lattice.composition(1, "rr", pitch_lattice.decode(1, "rr"))
    finally:
        lat.cls[row, 0] = "t"
