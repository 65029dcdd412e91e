"""Host test (no GPU): the layout arithmetic of a queue-mode flush (mbelib-neo_amd/csrc/mbe_flush_plan.h) through the stand-alone
program tests/flush_plan_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program is an executable of its
own; nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_the_flush_plan_holds_its_properties_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/flush_plan_check.cpp")
    exe = str(tmp_path / "flush_plan_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: with the shared runtime, ASan's link-order check stops the program at once
                            # in a process environment that preloads any other library)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "flush_plan_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.strip().endswith("cases ok") and int(run.stdout.split()[1]) == 2 * 32 ** 3 + 2 * 6 + 2, run.stdout
