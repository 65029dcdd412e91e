"""GPU suite (-m gpu): the pitch-pair lattices (tests/pitch_lattice.py: every (previous, current) fundamental, two frames per stream,
per voicing pattern; AMBE with its class rim) through the one-frame stream instances -- two launches of one frame --, the plain
looped instances -- one launch of two frames -- and, as (p, c, p, c), the LDS-parked and resident looped instances.  Every run is
tests/instance_cases.run_case with the lattice as its workload: the same buffers, entries, name and prediction assertions and the
same comparisons against the oracle, under the bounds of tests/parity.py.  In this process, under no switch; when the suite itself
runs under MBX_* switches the lattices are skipped (tests/test_gpu_instances.py then runs its cases in children of their own)."""
import os
import time

import pytest

import instance_cases
import pitch_lattice

pytestmark = pytest.mark.gpu
CASES = pitch_lattice.cases()


@pytest.fixture(scope="module")
def device():
    import mbelib_neo_amd as m

    m.lib()   # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)


@pytest.mark.parametrize("case,workload", CASES, ids=[c.id for c, _ in CASES])
def test_lattice_through_the_named_instance_against_the_oracle(device, case, workload):
    keep = ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")
    if any(k.startswith("MBX_") and k not in keep for k in os.environ):
        pytest.skip("the suite runs under MBX_* switches: the lattices are for the launcher's own choice of instance")
    pitch_lattice.decode(workload.codec, workload.pattern, workload.variant)   # (made, or found, before the clock starts: CPU work)
    t0 = time.perf_counter()
    workload.figures = None
    try:
        instance_cases.run_case(case, workload=workload)
    finally:   # (the figures are taken before the comparisons assert: a failing run prints them too)
        print("LATTICE", case.id, case.name, f"{time.perf_counter() - t0:.2f} s", workload.figures)
