"""CPU suite for the soft-decision batch paths: what the libraries export and declare, and where the soft front kernels and the
search they share with the FEC-only kernels live.  The GPU half is tests/test_gpu_soft_paths.py."""
import ctypes as C
import os
import re
import subprocess

import pytest

import shim_lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mbelib-neo_amd", "csrc")
NEW_MBX = ("mbx_process_batch_soft_resident", "mbx_process_batch_soft_ws", "mbx_session_submit_soft", "mbx_session_submit_soft_indexed")
QUEUE_CALLS = {"mbe_batchBegin", "mbe_flush", "mbe_batchPending", "mbe_batchRelease", "mbe_batchEnd"}


def _read(*parts):
    return open(os.path.join(*parts)).read()


def test_soft_launchers_are_exported_bound_and_cite_the_reference():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    header = _read(ROOT, "include", "mbx.h")
    exported = subprocess.run(["nm", "-D", "--defined-only", m.library_path()], capture_output=True, text=True).stdout
    for name in NEW_MBX:
        assert re.search(rf"\b{name}\s*\(", header), f"{name} is not declared in include/mbx.h"
        assert name in _native.EXPORTED_SYMBOLS
        assert re.search(rf" T {name}$", exported, re.M), f"libmbx_hip.so does not export {name}"
        # the comment block that ends right above the declaration names its reference lines
        comment = header[:header.index(f"int {name}(")]
        comment = comment[comment.rindex("/*"):]
        assert "ref:" in comment, f"{name}: no ref: citation above its declaration"
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in NEW_MBX:
        assert hasattr(handle, name)


def test_queue_mode_gains_a_flag_not_an_export():
    header = _read(ROOT, "include", "mbe_neo_amd.h")
    flag = re.search(r"#define\s+MBE_BATCH_QUEUE_SOFT\s+(\w+)", header)
    assert flag, "MBE_BATCH_QUEUE_SOFT is not defined in include/mbe_neo_amd.h"
    value = int(flag.group(1), 0)
    assert value not in (0, 1) and value & 1 == 0, "the flag must not collide with the two state modes"
    out = subprocess.check_output(["nm", "-D", "--defined-only", shim_lib.PATH]).decode()
    exported = set(re.findall(r" T (mbe_\w+)$", out, re.M))
    assert exported == set(shim_lib.declared_symbols())
    assert len(exported) == 92
    assert {n for n in exported if "batch" in n.lower() or n == "mbe_flush"} == QUEUE_CALLS


def test_every_soft_front_kernel_is_declared_once_and_defined_once():
    header = _read(CSRC, "mbx_kernels.h")
    sources = {f: _read(CSRC, f) for f in sorted(os.listdir(CSRC)) if f.endswith(".hip")}
    declared = re.findall(r"__global__\s+void\s+(soft_front_\w+)\s*\(", header)
    assert declared and len(declared) == len(set(declared)), declared
    defined = [k for text in sources.values() for k in re.findall(r"^(soft_front_\w+)\(", text, re.M)]
    assert sorted(defined) == sorted(declared), (defined, declared)
    api = sources["mbx_api.hip"]
    for k in declared:   # launched, and from one place
        assert api.count(f"mbx::{k},") == 1, k
    # the search has one home: the header next to mbx_fec_frame.h, included by both users, defined in neither
    shared = _read(CSRC, "mbx_fec_soft.h")
    for name in ("load_soft_cells", "soft_block", "golay_soft_wave", "hamming_soft_wave"):
        assert re.search(rf"__device__[^\n;]*\b{name}\(", shared), name
        for f in ("mbx_fec.hip", "mbx_soft_front.hip"):
            assert '#include "mbx_fec_soft.h"' in sources[f]
            assert not re.search(rf"__device__[^\n;]*\b{name}\(", sources[f]), f"{name} defined again in {f}"
    assert "struct SoftScratch {" in shared and not any("struct SoftScratch {" in t for t in sources.values())
