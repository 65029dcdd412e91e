"""GPU suite (-m gpu): the bit-error history lattices (tests/error_lattice.py: exact, scripted error counts per frame, 56 to 160 frames
per stream) through the stream-stage launch forms -- one frame per launch (batch, resident, staged, caller workspace), two frames per
launch through the plain looped instances, the whole history in ONE launch of the LDS-parked instances, and eight (or 32) frames per
launch through the LDS-parked and the resident looped instances.  Every run is tests/instance_cases.run_case with the lattice as its
workload: the same buffers, entries, name and prediction assertions and the same comparisons against the oracle under the bounds of
tests/parity.py -- and behind EVERY launch the decision state of cur_mp against the oracle's frame-by-frame decode: L, Vl,
repeatCount, amplitudeThreshold, errorCountTotal, errorCount4 exactly, errorRate and log2Ml bit for bit, localEnergy under the bound for float
state (error_lattice.check_checkpoint; how many of its bit patterns differ, and by how much, is in the line each test prints).  In this process, under no switch; when the suite itself runs under MBX_* switches the lattices are
skipped, as the pitch-pair lattices are."""
import os
import time

import pytest

import error_lattice
import instance_cases

pytestmark = pytest.mark.gpu
CASES = error_lattice.cases()


@pytest.fixture(scope="module")
def device():
    import mbelib_neo_amd as m

    m.lib()   # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)


@pytest.mark.parametrize("case,workload", CASES, ids=[c.id for c, _ in CASES])
def test_error_lattice_through_the_named_instance_against_the_oracle(device, case, workload):
    keep = ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")
    if any(k.startswith("MBX_") and k not in keep for k in os.environ):
        pytest.skip("the suite runs under MBX_* switches: the lattices are for the launcher's own choice of instance")
    error_lattice.composition(workload.codec, workload.name)   # (the oracle's work, made or found before the clock starts: CPU)
    t0 = time.perf_counter()
    workload.figures, workload.checkpoints, workload.failed, workload.measured, later = None, 0, None, {}, None
    try:
        instance_cases.run_case(case, workload=workload)
    except AssertionError as e:
        later = e
    # (the figures are taken before the comparisons assert: a failing run prints them too)
    print("LATTICE", case.id, case.name, f"{case.T} x {case.launches}", f"{time.perf_counter() - t0:.2f} s",
          f"checkpoints {workload.checkpoints}/{case.launches}, first mismatch: {workload.failed}", workload.figures)
    if workload.failed is not None:   # the first launch boundary at which the decision state is not the oracle's comes first
        raise AssertionError(workload.failed + (f" -- and behind the last launch: {later}" if later else ""))
    if later is not None:
        raise later
    assert workload.checkpoints == case.launches
