"""GPU suite (-m gpu): the IMBE one-frame stream instances fetch of prev_mp only what the decode reads, keep log2Ml in LDS across the
synthesiser and leave an unchanged rng record unstored (kLean*, mbx_stream.hip).  None of it may change a byte: every tick of a scripted
history is compared as bytes with one launch of T = k through a multi-frame instance, planted prev_mp structs and rng records are
held to their planted bits, and results, PCM and state are under the oracle (tests/parity.py).  Workloads, the cases the oracle must
show and the runners: tests/lean_state_cases.py.  Nothing here knows which library it runs on: it holds for any build."""
import os
import subprocess
import sys

import pytest

import lean_state_cases as cases

pytestmark = pytest.mark.gpu

IN_PROCESS = [name for name, form in cases.FORMS.items() if not form.env]
SWITCHED = [name for name, form in cases.FORMS.items() if form.env]


@pytest.fixture(scope="module")
def device():
    import mbelib_neo_amd as m

    m.lib()   # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)


_scripted = {}


def scripted(codec, n, oracle):
    """the scripted history of a codec and a stream count, made once and held to its cases (on the CPU, before anything runs on the GPU)"""
    if (codec, n) not in _scripted:
        cases.ssc.check_encoder(codec, oracle)
        frames, state, records = cases.scripted(codec, n, oracle)
        cases.assert_cases(codec, n, cases.trace(codec, oracle, frames, state, records))
        _scripted[codec, n] = (frames, state, records)
    return _scripted[codec, n]


@pytest.mark.parametrize("name", IN_PROCESS)
def test_scripted_history_tick_by_tick_equals_one_long_launch(device, oracle, name):
    """eight T = 1 launches of each form -- repeats behind a decode with prev_L < cur_L and prev_L > cur_L, repeats from an invalid b0,
    five repeats in a row, unvoiced bands between all-voiced frames at several harmonic counts, cold starts with and without a pending
    seed, comfort noise and the frames behind it: behind every tick state, rng records, results and PCM are byte-identical to one
    launch of T = k, in both walking orders, and the whole history is under the oracle."""
    form = cases.FORMS[name]
    assert not any(k.startswith("MBX_FUSE_ONE") or k == "MBX_NO_RES1" for k in os.environ), "the forms are the default launch plan's"
    frames, state, records = scripted(form.codec, form.n, oracle)
    cases.run_history(form, frames, state, records, oracle)


@pytest.mark.parametrize("name", IN_PROCESS)
def test_a_repeat_carries_planted_prev_mp_into_cur_mp(device, oracle, name):
    """prev_mp.Ml (a value per stream and harmonic, a -0.0f, a NaN) and prev_mp.noiseSeed planted in front of a repeat: the struct the
    repeat copied holds them bit for bit, with the decode's padding exactly where the decode ran."""
    cases.run_planted_prev(cases.FORMS[name], oracle)


@pytest.mark.parametrize("name", IN_PROCESS)
def test_planted_rng_records_change_in_the_oracles_fields_only(device, oracle, name):
    """rng records that a frame leaves as they are, changes in one field (a pending seed taken, comfort noise) or in two: the oracle's
    record in every field, the reserved word untouched."""
    cases.run_planted_rng(cases.FORMS[name], oracle)


@pytest.mark.parametrize("name", SWITCHED)
def test_forms_behind_a_launch_switch(name):
    """the in-wave front end for 7200x4400 frames is chosen by MBX_FUSE_ONE=1, which the library reads once per process: the same three
    checks in a fresh child"""
    form = cases.FORMS[name]
    env = {k: v for k, v in os.environ.items() if not k.startswith("MBX_") or k.startswith(("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY"))}
    env.update(form.env)
    out = subprocess.run([sys.executable, os.path.abspath(cases.__file__), name], env=env, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0 and f"ok {name}" in out.stdout, out.stdout[-2000:] + out.stderr[-2000:]
