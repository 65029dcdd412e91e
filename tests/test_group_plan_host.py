"""Host test (no GPU): where the burst groups of one call sit in the gather's grid, in the rows of the mixed step and in the
workspace (mbelib-neo_amd/csrc/mbx_group_plan.h), through the stand-alone program tests/group_plan_check.cpp, built with
AddressSanitizer and UndefinedBehaviorSanitizer.  The program is an executable of its own; nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_group_plan_holds_its_properties_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/group_plan_check.cpp")
    exe = str(tmp_path / "group_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program, as tests/test_flush_plan_host.py links them)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "group_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    lines = run.stdout.strip().splitlines()
    # every assignment of 600 per group to three groups is stood for by one of the distinct inputs cubed (the program checks the sum)
    distinct = int(lines[0].split()[1])
    assert lines[0].endswith("distinct inputs of 600 assignments per group") and 100 < distinct <= 600, run.stdout
    assert lines[-1].endswith("cases ok") and int(lines[-1].split()[1]) == distinct ** 3 + 2 * (8 * 5 + 2) + 1 + 12 + 1, run.stdout
