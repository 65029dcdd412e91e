"""GPU suite (-m gpu): every row of kInstances (mbelib-neo_amd/csrc/mbx_api.hip) by the name the launcher recorded for the launch,
against the oracle on every stream -- the cases, their shapes and the comparison are tests/instance_cases.py.  Cases without
environment switches run in this process when its own environment is free of MBX_* switches; a case with switches, and every case
when this process runs under switches of its own (tools/test_env_matrix.sh), runs in a fresh child process with exactly the case's
switches (the library reads them once), one at a time, under a time limit sized to the case."""
import os
import subprocess
import sys

import pytest

import instance_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def device():
    import mbelib_neo_amd as m

    m.lib()   # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)


@pytest.mark.parametrize("case_id", [c.id for c in instance_cases.CASES])
def test_instance_by_recorded_name_against_the_oracle(device, case_id):
    case = instance_cases.BY_ID[case_id]
    keep = ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")
    if not case.env and not any(k.startswith("MBX_") and k not in keep for k in os.environ):
        print(case_id, instance_cases.run_case(case))
        return
    env = {k: v for k, v in os.environ.items() if not k.startswith("MBX_") or k in keep}
    env.update(case.env)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "instance_cases.py"), case_id], capture_output=True, text=True,
                           timeout=instance_cases.child_timeout(case), env=env)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"{case_id}: the child process did not finish in {e.timeout} s -- nothing more is started on the card", returncode=3)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"{case_id}: the child process ended with status {r.returncode} (a signal, an abort or a fault) -- nothing more is "
                    f"started on the card\n{tail}", returncode=3)
    assert r.returncode == 0, f"{case_id}: exit status {r.returncode}\n{tail}"
    print(r.stdout.strip().splitlines()[-1])
