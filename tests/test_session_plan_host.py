"""Host test (no GPU): the integer decisions of a session (mbelib-neo_amd/csrc/mbx_session_plan.h) -- the output table, the refusals of
a submit and their order, the stream-index walks, the byte layout of a group submit -- through the stand-alone program
tests/session_plan_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program is an executable of its own;
nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# outputs: 64 flag sets + 8 * 8 * 3 sizes; frames submits: 7,680 shapes x 64 flag sets x 8 requests; bursts submits; group submits;
# texts; the index walks; layouts: (1 + 96 + 96^2 + 96^3 + 30 * 96) hard and soft
CASES = 256 + 3_932_160 + 61_440 + 24_576 + 16 + 50_630 + 2 * 896_929


def test_the_session_plan_holds_the_formulas_it_replaced_and_its_properties_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/session_plan_check.cpp")
    exe = str(tmp_path / "session_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: with the shared runtime, ASan's link-order check stops the program at once
                            # in a process environment that preloads any other library)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "session_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.strip().endswith("cases ok") and int(run.stdout.split()[1]) == CASES, run.stdout
