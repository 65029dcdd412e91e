"""Host test (no GPU): what a batch step launches (mbelib-neo_amd/csrc/mbx_launch_plan.h, plan_step) through the stand-alone program
tests/launch_plan_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program is an executable of its own;
nothing is loaded into this process."""
import os
import re
import shutil
import subprocess

import pytest

import instance_cases

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
SWITCHES = ("MBX_LDS_MIN_FRAMES", "MBX_NO_RES1", "MBX_NO_LDS_RESIDENT", "MBX_SLICE", "MBX_SLICE_GROUPS", "MBX_SLICE_OWN", "MBX_RAGGED_ORDER",
            "MBX_FUSE_ONE", "MBX_FRONT_LEAD")
# the entries whose call is what mbx_batch_kernel_name predicts: mbx_process_batch / _indexed / _resident on the slot's own workspace
PREDICTED_ENTRIES = ("batch", "batch_indexed", "resident", "resident_indexed")


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/launch_plan_check.cpp")
    exe = str(tmp_path_factory.mktemp("launch_plan") / "launch_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "launch_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def clean_env(extra=None):
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(extra or {})
    return env


def test_the_plan_gives_the_parents_decisions_and_holds_its_properties_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.strip().endswith("launch_plan_check: ok"), run.stdout
    m = re.search(r"(\d+) decisions, hash (0x[0-9a-f]{16}), (\d+) parser cases", run.stdout)
    assert m and int(m.group(1)) == 12_870_144 and m.group(2) == "0x8785e233af7ae182" and int(m.group(3)) == 47, run.stdout


def test_the_plan_names_every_instance_case_and_the_prediction_agrees(check_exe):
    """every case of tests/instance_cases.py, and every form of the pitch-pair and the bit-error history lattices (tests/pitch_lattice.py, tests/error_lattice.py), planned for a whole MI355X (1,024 SIMDs) under the case's switches: the plan's index,
    through the order of the kInstances rows, is the case's instance -- and for the entries the prediction is made for, the plan behind
    mbx_batch_kernel_name names the same one (what tests/instance_cases.py then asserts on the card after every launch)"""
    api = open(os.path.join(ROOT, "mbelib-neo_amd", "csrc", "mbx_api.hip")).read()
    table = api[api.index("kInstances[] = {"):]
    names = re.findall(r'\{"(\w+)",\s*mbx::\w+\}', table[:table.index("};")])
    assert len(names) == 28
    import pitch_lattice

    import error_lattice

    lattices = [case for case, _ in pitch_lattice.cases() + error_lattice.cases()]   # (the same entries at 17,344 ... 65,536 streams, and at 274 ... 690)
    for c in instance_cases.CASES + lattices:
        run = subprocess.run([check_exe, "case", str(c.codec), str(c.S), str(c.T), c.entry], capture_output=True, text=True, timeout=60, env=clean_env(c.env))
        assert run.returncode == 0, (c.id, (run.stdout + run.stderr)[-4000:])
        real, predicted = (names[int(x)] for x in run.stdout.split())
        assert real == c.name, f"{c.id}: the plan of the call names {real}"
        if c.entry in PREDICTED_ENTRIES:
            assert predicted == c.name, f"{c.id}: the prediction's plan names {predicted}"
