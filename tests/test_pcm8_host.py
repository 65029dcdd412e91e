"""CPU suite for companded PCM out (include/mbx_pcm8.h): the arithmetic of mbelib-neo_amd/csrc/mbx_compand.h through the stand-alone
program tests/compand_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as
tests/test_keystream_plan_host.py builds its program (an executable of its own; nothing is loaded into this process); the numpy
definition (mbelib_neo_amd.pcm8) over all 65,536 int16 values against the pinned hashes, the known answers and, where it imports,
audioop; mbx_pcm_compand_host held to numpy; the refusals of mbx_pcm_compand before a device is asked for; the header held to the
library's exports and to the ctypes table of its own (_native.PCM8_SYMBOLS).  No GPU compute here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mbelib_neo_amd import pcm8
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_pcm8.h")
INVALID = -1
FUNCTIONS = ["mbx_pcm_compand_host", "mbx_pcm_compand", "mbx_session_next_pcm8"]
ULAW_HASH, ALAW_HASH = 0xF2471A71, 0x826FE2C5
KNOWN = [(-32768, 0x00, 0x2A), (-1000, 0x4E, 0x7A), (-1, 0x7E, 0x55), (0, 0xFF, 0xD5), (3, 0xFF, 0xD5), (4, 0xFE, 0xD5), (1000, 0xCE, 0xFA),
         (32767, 0x80, 0xAA)]
ALL = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)   # every int16 value, x = -32768 .. 32767 in that order


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/compand_check.cpp")
    exe = str(tmp_path_factory.mktemp("compand") / "compand_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "compand_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_leading_one_arithmetic_is_the_segment_search_and_holds_its_pins_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    assert last == "compand_check: ok (131072 samples, hashes 0xF2471A71 0x826FE2C5)", run.stdout


def test_the_numpy_definition_holds_the_pins_the_known_answers_and_audioop():
    u, a = pcm8.ulaw(ALL), pcm8.alaw(ALL)
    assert u.dtype == np.uint8 and a.dtype == np.uint8 and u.shape == a.shape == (65536,)
    assert pcm8.fnv1a32(u) == ULAW_HASH and pcm8.fnv1a32(a) == ALAW_HASH
    for x, mu, al in KNOWN:
        assert (int(u[x + 32768]), int(a[x + 32768])) == (mu, al), x
    assert len(np.unique(u)) == 255 and 0x7F not in u and len(np.unique(a)) == 256
    assert pcm8.ulaw(ALL.reshape(256, 256)).shape == (256, 256)   # any shape
    assert pcm8.compand(ALL, pcm8.LAW_ULAW).tobytes() == u.tobytes() and pcm8.compand(ALL, pcm8.LAW_ALAW).tobytes() == a.tobytes()
    with pytest.raises(ValueError):
        pcm8.compand(ALL, 2)
    with pytest.raises(TypeError):
        pcm8.ulaw(ALL.astype(np.int32))
    # the expansion tables: every code comes back but mu-law 0x7F (it expands to 0, and 0 is 0xFF); decode(encode(x)) never falls
    codes = np.arange(256)
    assert pcm8.ULAW_EXPAND.dtype == np.int16 and pcm8.ALAW_EXPAND.dtype == np.int16
    back = pcm8.ulaw(pcm8.ULAW_EXPAND)
    assert (back != codes).nonzero()[0].tolist() == [0x7F] and pcm8.ULAW_EXPAND[0x7F] == 0 and back[0x7F] == 0xFF
    assert (pcm8.alaw(pcm8.ALAW_EXPAND) == codes).all()
    assert (np.diff(pcm8.ULAW_EXPAND[u].astype(np.int32)) >= 0).all() and (np.diff(pcm8.ALAW_EXPAND[a].astype(np.int32)) >= 0).all()
    try:
        import audioop
    except ImportError:   # (removed from CPython 3.13: only this comparison is left out)
        return
    assert audioop.lin2ulaw(ALL.tobytes(), 2) == u.tobytes() and audioop.lin2alaw(ALL.tobytes(), 2) == a.tobytes()
    every = bytes(range(256))
    assert audioop.ulaw2lin(every, 2) == pcm8.ULAW_EXPAND.tobytes() and audioop.alaw2lin(every, 2) == pcm8.ALAW_EXPAND.tobytes()


def _declared():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mbx_\w+)\s*\(([^;{]*?)\)\s*;", text)}


def _lib():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    if not os.path.exists(m.library_path()):
        pytest.fail(f"{m.library_path()} is missing: build it first")
    try:
        C.CDLL(m.library_path())
    except OSError as e:   # the one thing a host may lack: a loadable HIP runtime
        pytest.skip(f"HIP runtime not loadable here: {e}")
    return _native.lib()   # a library that lost a symbol fails here, it does not skip


def test_every_function_of_the_pcm8_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert sorted(declared) == sorted(FUNCTIONS)
    assert tuple(declared) == _native.PCM8_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS):
        assert not set(_native.PCM8_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    for name, value in (("MBX_LAW_ULAW", pcm8.LAW_ULAW), ("MBX_LAW_ALAW", pcm8.LAW_ALAW), ("MBX_SESSION_PCM8", pcm8.SESSION_PCM8)):
        assert int(re.search(rf"#define {name}\s+(\d+)u?\b", text).group(1)) == value, name
    # the alignment row of the new kind is stated, in a table in the style of the one in mbx.h
    assert "Alignment, in the style of the table in mbx.h" in text and re.search(r"^ \*   pcm8\s+1\b", text, flags=re.M)
    # include/mbx.h does not know the new calls or the new bit: a header of its own
    mbx_h = open(os.path.join(ROOT, "include", "mbx.h")).read()
    assert not any(f in mbx_h for f in FUNCTIONS) and "MBX_SESSION_PCM8" not in mbx_h and "mbx_pcm" not in mbx_h
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name


def test_the_host_function_is_the_numpy_definition_over_every_value():
    L = _lib()
    for law, want in ((pcm8.LAW_ULAW, pcm8.ulaw(ALL)), (pcm8.LAW_ALAW, pcm8.alaw(ALL))):
        got = np.full(65536 + 2, 0xA5, dtype=np.uint8)
        assert L.mbx_pcm_compand_host(law, ALL.ctypes.data, 65536, got[1:].ctypes.data) == 0
        assert got[1:-1].tobytes() == want.tobytes() and got[0] == 0xA5 and got[-1] == 0xA5, law
        assert L.mbx_pcm_compand_host(law, ALL.ctypes.data, 0, got.ctypes.data) == 0 and got[0] == 0xA5
    out = np.zeros(4, dtype=np.uint8)
    for args in ((0, None, 4, out.ctypes.data), (0, ALL.ctypes.data, 4, None), (2, ALL.ctypes.data, 4, out.ctypes.data), (-1, ALL.ctypes.data, 4, out.ctypes.data)):
        assert L.mbx_pcm_compand_host(*args) == INVALID and b"mbx_pcm_compand_host" in L.mbx_last_error(), args
    assert not out.any()


def test_the_launcher_refuses_its_arguments_before_it_asks_for_a_device():
    """in the manner of test_the_launcher_refuses_pointers_below_their_alignment_before_it_asks_for_a_device
    (tests/test_memory_contract_host.py): never dereferenced, every call below is refused first, on a host with no GPU as well"""
    L = _lib()

    def refused(*args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert L.mbx_pcm_compand(*args) == INVALID, args
        text = L.mbx_last_error()
        assert b"mbx_pcm_compand" in text and b"mbx_pcm_compand_host" not in text, text
        return text

    refused(0, None, 4, 0x2000, None)
    refused(1, 0x1000, 4, None, None)
    assert b"law" in refused(2, 0x1000, 4, 0x2000, None)
    refused(-1, 0x1000, 4, 0x2000, None)
    for law in (0, 1):
        text = refused(law, 0x1001, 4, 0x2000, None)   # an odd d_pcm16
        assert b"alignment" in text and b"mbx_pcm8.h" in text, text
        assert L.mbx_pcm_compand(law, 0x1001, 0, 0x2000, None) == INVALID   # ... whatever the count
    # d_pcm8 may sit anywhere, and an even d_pcm16 is enough: nothing to refuse, and no frames launch nothing, device or none
    for out in (0x2000, 0x2001, 0x2003, 0x2007):
        assert L.mbx_pcm_compand(0, 0x1002, 0, out, None) == 0
    # the session call refuses a missing session by name
    assert L.mbx_session_next_pcm8(None, 0, 0x2000) == INVALID and b"mbx_session_next_pcm8" in L.mbx_last_error()
