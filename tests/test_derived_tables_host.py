"""Host test (no GPU): what mbx_init() does before a device is involved -- the blob checks and the derived tables of
mbelib-neo_amd/csrc/mbx_derive.h -- and the per-frame cell arithmetic of mbelib-neo_amd/csrc/mbx_cells.h, through the stand-alone
program tests/derived_tables_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer.  The program is an executable of
its own; nothing is loaded into this process."""
import os
import shutil
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

# what the loops of derived_tables_check.cpp imply, section by section
CELLS = 184 + 96 + 168 + 96                                      # the four codecs' frame arrays
CASES = (1 + 2 + 1 + 1 + 3 + 2                                   # blob: accepted; size -4 / +4; magic; checksum; window 55 / 105 / 264; imbe_bo 58 / 12
         + 1                                                     # the Hamming-basis refusal
         + 48 * 161 + 161                                        # lcg: x0 x k; lcg_pack
         + 4096 * 114 + 4096 + 1 + 116 + 64                      # pr: seed x step; unused bits per seed; the padding row; pr_mul / pr_add; pr_lane
         + 4096 + 12 + 2 * 11                                    # golay_half_syn; golay_rot; the two Hamming bases
         + 48 + 11 + 208 + 64                                    # imbe: ownership per L; imbe_len_rows per length; imbe_b0; imbe_L_lanes
         + 57 * 57 + 2 * 57 + 192 + 160                          # l_ratio; imbe_rho_over_l, ambe_pred_over_l; nfrac; wola_inv
         + 63 + 128                                              # log2_int; ambep_f0
         + 2                                                     # padding zero; pinned hash
         + 4 * (4096 + 2) + CELLS                                # pack_rows: random, all-zero, all-one, single-cell arrays
         + 3 * CELLS + 5 + 3 * (1 + 7 + 15 + 23 + 49) + 1)       # validate_bits: 2 / 0x80 / 0xFF at every cell; short counts; NULL


def test_blob_checks_derived_tables_and_cell_arithmetic_hold_under_asan_and_ubsan(tmp_path):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/derived_tables_check.cpp")
    rocm = os.environ.get("ROCM_PATH") or "/opt/rocm"
    exe = str(tmp_path / "derived_tables_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-ffp-contract=off", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program, as for tests/flush_plan_check.cpp)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            # (hip_vector_types.h, for the uint2 members of DerivedTables: types only, no HIP runtime is linked)
                            "-D__HIP_PLATFORM_AMD__", "-I" + os.path.join(rocm, "include"),
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "derived_tables_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    run = subprocess.run([exe, os.path.join(ROOT, "mbelib-neo_amd", "data", "mbx_tables.bin")], capture_output=True, text=True, timeout=300)
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last.endswith("cases ok") and int(last.split()[1]) == CASES, run.stdout
