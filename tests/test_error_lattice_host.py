"""Host test (no GPU): the bit-error history lattices of tests/error_lattice.py hold, in the ORACLE's decode, what the GPU tests of
tests/test_gpu_error_lattice.py rely on -- every frame's error counts as scripted, repeats only where the scripts put them and the
probe totals 11, 12, 13 with both outcomes, every threshold of the error rate crossed in both directions inside a stream, bands forced
voiced and amplitudes scaled under errors and never without, at least 70 % of the frames below the soft clip --; the frame-by-frame
decode is the one-call decode byte for byte; the forms name instances the instance cases know; and a mismatch in each compared thing
raises with the stream's script in the message.  The oracle's decodes are cached in error_lattice (one trajectory per lattice)."""
import numpy as np
import pytest

import error_lattice
import instance_cases
import parity
from pitch_lattice import FLAG_REPEAT


@pytest.mark.parametrize("codec,name", error_lattice.LATTICES)
def test_the_lattice_holds_what_the_gpu_tests_rely_on(codec, name):
    lat = error_lattice.build(codec, name)
    S, T = lat.frames.shape[:2]
    assert S == error_lattice.build_size(codec, name) and T == error_lattice.FRAMES[(codec, name)] and S * T < 200_000
    assert 256 < S < 5120, "above the small-batch limit, below the wave slots of a whole device: the one-launch kernels, and no form is sliced"
    figures = error_lattice.composition(codec, name)
    print(codec, name, figures)
    if (codec, name) == (0, "probe"):
        assert S >= 616
        assert {tuple(p) for p in lat.probe[:, 1:].tolist()} == {(c0, t) for c0 in (2, 3) for t in range(10, 15 + (c0 == 3))}
        assert set(lat.hist[:, 0].tolist()) == set(range(14)) and set(error_lattice.PROBE_N) <= set(lat.hist[:, 1].tolist())


def test_flipped_data_cells_are_the_error_counts_of_the_front_end(oracle):
    """flip_data_cells against the oracle's FEC alone, every codec: the counts asked for, and the parameter bits of the clean frames"""
    import oracle_lib

    for codec, name in error_lattice.LATTICES:
        lat = error_lattice.build(codec, name)
        rec = oracle.fec_batch(codec, lat.frames.reshape(-1, lat.frames.shape[2]))
        res = oracle_lib.records_to_results(rec)
        for field, want in (("total_errors", lat.total), ("c0_errors", lat.c0), ("c4_errors", lat.c4)):
            assert np.array_equal(res[field], want.reshape(-1)), (codec, name, field)
        clean = oracle.fec_batch(codec, lat.clean.reshape(-1, lat.frames.shape[2]))
        assert not oracle_lib.records_to_results(clean)["total_errors"].any()
        assert np.array_equal(rec["w"][:, :3], clean["w"][:, :3]), (codec, name, "corrected bits")


def test_two_generations_of_a_lattice_are_the_same_bytes():
    first = error_lattice.build(3, "steady").frames.copy()
    error_lattice.build.cache_clear()
    assert error_lattice.build(3, "steady").frames.tobytes() == first.tobytes()


@pytest.mark.parametrize("codec,name", error_lattice.LATTICES)
def test_the_trajectory_is_the_one_call_decode_byte_for_byte(codec, name):
    traj, whole = error_lattice.trajectory(codec, name), error_lattice.one_call(codec, name)
    for key in ("records", "results", "pcm16", "pcmf", "peak", "state", "rng"):
        assert traj[key].dtype == whole[key].dtype and traj[key].shape == whole[key].shape, key
        assert traj[key].tobytes() == whole[key].tobytes(), key
    last = error_lattice.cur_at(codec, name, error_lattice.FRAMES[(codec, name)] - 1)
    for key in error_lattice.CHECK_INT + error_lattice.BIT_FIELDS:
        assert last[key].tobytes() == np.ascontiguousarray(whole["state"][:, 0][key]).tobytes(), key


def test_every_form_names_an_instance_the_instance_cases_know():
    """(that the launch plan picks each name at the lattice's S and the form's T, through mbx_batch_kernel_name's plan as well, is
    tests/test_launch_plan_host.py's, on the CPU, and run_case's on the card)"""
    cases = error_lattice.cases()
    assert len({c.id for c, _ in cases}) == len(cases)
    known = {(c.codec, c.name) for c in instance_cases.CASES}
    entries = {c.entry for c in instance_cases.CASES}
    for case, work in cases:
        assert (case.codec, case.name) in known, case
        assert case.entry in entries and not case.env, case
        assert case.S == error_lattice.build_size(case.codec, work.name) and case.T * case.launches == error_lattice.FRAMES[(case.codec, work.name)]
    shapes = lambda codec, name: sorted((c.T, c.launches) for c, w in cases if (c.codec, w.name) == (codec, name))   # noqa: E731
    assert shapes(0, "probe") == [(1, 56)] * 4 + [(2, 28), (8, 7), (8, 7), (56, 1)]
    assert shapes(0, "steady") == [(1, 160), (1, 160), (8, 20), (32, 5), (160, 1)]
    assert shapes(2, "steady") == [(1, 160), (1, 160), (2, 80)]
    assert shapes(1, "steady") == shapes(3, "steady") == [(1, 64)] * 3 + [(2, 32), (8, 8), (8, 8), (64, 1)]
    # 21 instances: every row of the table but the sliced ones and the one-frame resident instances that only a switch or a small batch selects
    names = {c.name for c, _ in cases}
    rest = {c.name for c in instance_cases.CASES} - names
    assert len(names) == 21 and all("slice" in n or "res1" in n for n in rest), rest


def _message(check):
    with pytest.raises(AssertionError) as e:
        check()
    return str(e.value)


def test_a_failure_of_each_comparison_names_the_script():
    """the oracle's decode as `got` with ONE field altered -- a probe frame's REPEAT flag, an errorRate and a log2Ml by one ulp at a checkpoint, an
    amplitudeThreshold, a band of Vl, a localEnergy by one per cent: each raises, and the message names the stream's script (history count and length, the probe's
    (c0, total)), the frame and the error rate before it"""
    codec, name = 0, "probe"
    lat, ref = error_lattice.build(codec, name), error_lattice.trajectory(codec, name)
    S, T = lat.total.shape
    s = int(np.flatnonzero((lat.hist[:, 0] == 7) & (lat.hist[:, 1] == 24) & (lat.probe[:, 1] == 2) & (lat.probe[:, 2] == 12))[0])
    f = 24
    script = "history 7 errors x 24 frames; probe (c0 2, total 12) at frame 24"
    er = f"er before the frame {float(error_lattice.er_before(codec, name, s, f)):.9g}"
    assert float(error_lattice.er_before(codec, name, s, f)) > 0.03

    got = ref["results"].copy()
    got["flags"][s * T + f] ^= FLAG_REPEAT

    def results():
        with error_lattice.named(codec, name, T):
            with parity.located(T):
                parity.check_results(ref["results"], got, "x: results")
    m = _message(results)
    assert f"stream {s}, tick {f} = script [{script}" in m and f"frame {f} is 'v' with total 12, c0 2" in m and er in m, m

    def altered(field, change):
        cur = error_lattice.cur_at(codec, name, f)
        error_lattice.check_checkpoint(codec, name, f, cur)   # (unaltered: passes)
        change(cur[field])
        return _message(lambda: error_lattice.check_checkpoint(codec, name, f, cur, what="x: launch 3"))

    def one_ulp(a):
        a.view(np.uint32)[s] += 1
    m = altered("errorRate", one_ulp)
    assert f"behind frame {f}: errorRate of cur_mp differs in 1 streams, first stream {s}:" in m and "-1 ulp" in m and script in m and er in m, m

    def threshold(a):
        a[s] += 300
    m = altered("amplitudeThreshold", threshold)
    assert "amplitudeThreshold of cur_mp differs" in m and f"first stream {s}:" in m and script in m and er in m, m

    def band(a):
        a[s, 3] ^= 1
    m = altered("Vl", band)
    assert f"Vl of cur_mp differs in 1 streams, first stream {s}: band 3:" in m and script in m and f"frame {f} is" in m and er in m, m

    # ... and the workload's checkpoint keeps the first mismatch of a run, with the launch it was behind
    work = error_lattice.Workload(codec, name)
    case = [c for c, _ in error_lattice.cases() if c.id == "lds-eight-codec0-probe"][0]
    for launch in range(case.launches):
        state = np.zeros((S, 3), dtype=error_lattice.PARMS_DTYPE)
        state[:, 0] = error_lattice.cur_at(codec, name, (launch + 1) * case.T - 1)
        if launch >= 1:
            state[:, 0]["localEnergy"].view(np.uint32)[s] ^= 1     # an ulp of localEnergy is counted, not refused ...
        if launch >= 2:
            state[:, 0]["errorCount4"][s] ^= 1
        work.checkpoint(case, launch, state)
    assert work.checkpoints == 7 and "launch 2: behind frame 23: errorCount4 of cur_mp differs in 1 streams" in work.failed and script in work.failed
    assert work.measured["localEnergy"][:2] == [6, 1] and work.measured["localEnergy"][3] == (s, 15) and work.measured["log2Ml"][0] == 0

    def memory(a):
        a.view(np.uint32)[s, 9] -= 1
    m = altered("log2Ml", memory)
    assert f"log2Ml of cur_mp differs in 1 streams, first stream {s}: band 9:" in m and "+1 ulp" in m and script in m and er in m, m

    def energy(a):   # ... and one per cent of it in one stream is over the bound of its block of 256
        a[s] *= np.float32(1.01)
    m = altered("localEnergy", energy)
    assert "localEnergy of cur_mp: relative RMS" in m and f"worst stream {s}:" in m and script in m and er in m, m
