"""Host test (no GPU) of keystream input: the row -> words conversion the kernels and the host function share
(mbelib-neo_amd/csrc/mbx_keystream_words.h) and the planner's rule for a keyed step (mbx_launch_plan.h), through the stand-alone
program tests/keystream_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as
tests/test_launch_plan_host.py builds its program.  The program is an executable of its own; nothing is loaded into this process."""
import os
import re
import shutil
import subprocess

import pytest

from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/keystream_check.cpp")
    exe = str(tmp_path_factory.mktemp("keystream") / "keystream_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "keystream_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_words_are_the_bit_loop_and_a_keyed_plan_is_the_unfused_plan_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    assert run.stdout.strip().splitlines()[-1].startswith("keystream_check: ok"), run.stdout
    m = re.search(r"ok \((\d+) rows, (\d+) plans\)", run.stdout)
    # 2 x (1 + 96 + 1 + 20,000) rows; 3 values of MBX_FUSE_ONE x 4 codecs x 5 S x 4 T x 2 kinds x 64 flag sets
    assert m and int(m.group(1)) == 2 * 20098 and int(m.group(2)) == 3 * 4 * 5 * 4 * 2 * 64, run.stdout
    assert int(re.search(r"(\d+) of them one-launch forms when unkeyed", run.stdout).group(1)) > 0
