"""Host tests (no GPU) of the per-frame library's device list, MBX_DEVICES: the parser and the placement arithmetic
(mbelib-neo_amd/csrc/mbe_device_list.h) through the stand-alone program tests/device_list_check.cpp, built with AddressSanitizer and
UndefinedBehaviorSanitizer -- the program is an executable of its own; nothing is loaded into this process --, and the five mbq_*
reporting functions: exported by the built library, declared in include/mbe_neo_shards.h, absent from include/mbe_neo_amd.h."""
import os
import re
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
MBQ = {"mbq_shard_count", "mbq_shard_device", "mbq_thread_home", "mbq_channel_shard", "mbq_shard_census"}


def test_the_device_list_holds_its_rules_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/device_list_check.cpp")
    exe = str(tmp_path / "device_list_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program, as tests/test_flush_plan_host.py has them)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "device_list_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    # 15 accepted texts, 25 refused ones, the NULL-why case, and one case per (n, home) with n = 1..32
    assert run.stdout.strip().endswith("cases ok") and int(run.stdout.split()[1]) == 15 + 25 + 1 + 32 * 33 // 2, run.stdout


def test_the_shard_functions_are_exported_and_declared_in_a_header_of_their_own():
    import shim_lib

    out = subprocess.check_output(["nm", "-D", "--defined-only", shim_lib.PATH]).decode()
    assert set(re.findall(r" T (mbq_\w+)$", out, re.M)) == MBQ
    with open(os.path.join(ROOT, "include", "mbe_neo_shards.h")) as f:
        shards = f.read()
    assert set(re.findall(r"\b(mbq_[a-z_]+)\s*\(", shards)) == MBQ
    assert not re.search(r"#\s*include", shards), "the header stands alone: plain C types, no other header"
    with open(shim_lib.HEADER) as f:
        assert "mbq_" not in f.read(), "include/mbe_neo_amd.h is the reference's interface and keeps to mbe_*"
