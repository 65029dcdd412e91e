"""CPU suite for mix-down out (include/mbx_mixdown.h): the arithmetic of mbelib-neo_amd/csrc/mbx_mixdown.h, the host-only plan of
mbx_mixdown_plan.h and the long kernel form's partition through the stand-alone program tests/mixdown_check.cpp, built with
AddressSanitizer and UndefinedBehaviorSanitizer exactly as tests/test_pcm8_host.py builds its program (an executable of its own;
nothing is loaded into this process); the numpy definition (mbelib_neo_amd.mixdown.mix) on known answers; mbx_mixdown_host held to
numpy in all three forms; the refusals of the plan calls, of mbx_mixdown and of mbx_session_next_mixdown before a device is asked for;
the header held to the library's exports and to the ctypes table of its own (_native.MIXDOWN_SYMBOLS).  No GPU compute here.

A host without a device can make no plan, so what mbx_mixdown refuses of a plan it HAS (nrows below the rows needed, arrays that
overlap) is held here through the function the launcher calls for it (mixdown_launch_refused, in mixdown_check.cpp) and through
mbx_mixdown_host, and through the library itself in tests/test_gpu_mixdown.py."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mbelib_neo_amd import mixdown, pcm8
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_mixdown.h")
INVALID = -1
FUNCTIONS = ["mbx_mixdown_plan_create", "mbx_mixdown_plan_create_split", "mbx_mixdown_plan_destroy", "mbx_mixdown_plan_buses",
             "mbx_mixdown_plan_rows", "mbx_mixdown_plan_long_buses", "mbx_mixdown_host", "mbx_mixdown", "mbx_session_next_mixdown"]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/mixdown_check.cpp")
    exe = str(tmp_path_factory.mktemp("mixdown") / "mixdown_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "mixdown_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_arithmetic_the_plan_and_the_long_forms_partition_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"mixdown_check: ok \(default split (\d+), 12 slices of 20 pieces\)", last)
    assert found, run.stdout
    assert int(found.group(1)) == mixdown.LONG_ABOVE, "mixdown.LONG_ABOVE is the library's default split"


def _rows(rng, rows):
    x = rng.integers(-32768, 32768, size=(rows, 160), dtype=np.int64).astype(np.int16)
    x[rng.integers(0, rows, 12), rng.integers(0, 160, 12)] = np.tile(np.array([-32768, 32767, 0, -1], dtype=np.int16), 3)
    return x


def test_the_numpy_definition_on_known_answers():
    rng = np.random.default_rng(3)
    x = _rows(rng, 5)
    # a unity single input is the row itself, and as bytes its companded row; no inputs are silence
    off, row = np.array([0, 1, 1, 2]), np.array([3, 3])
    for gain in (None, np.array([4096, 4096], dtype=np.int16)):
        y = mixdown.mix(x, off, row, gain, mixdown.PCM16)
        assert y.dtype == np.int16 and y.shape == (3, 160)
        assert y[0].tobytes() == x[3].tobytes() and not y[1].any() and y[2].tobytes() == x[3].tobytes()
        u, a = mixdown.mix(x, off, row, gain, mixdown.ULAW), mixdown.mix(x, off, row, gain, mixdown.ALAW)
        assert u.dtype == np.uint8 and u[0].tobytes() == pcm8.ulaw(x[3]).tobytes() and a[2].tobytes() == pcm8.alaw(x[3]).tobytes()
        assert (u[1] == 0xFF).all() and (a[1] == 0xD5).all()
    # term by term: x * g with the rounding at half an LSB, a floor for negative products
    one = np.zeros((1, 160), dtype=np.int16)
    one[0, :8] = [1, -1, 1, -1, 3, -3, 1, -1]
    gains = {2048: [1, 0, 1, 0, 2, -1, 1, 0], 2047: [0, 0, 0, 0, 1, -1, 0, 0], 6144: [2, -1, 2, -1, 5, -4, 2, -1], -2048: [0, 1, 0, 1, -1, 2, 0, 1]}
    for g, want in gains.items():
        y = mixdown.mix(one, [0, 1], [0], np.array([g], dtype=np.int16))
        assert y[0, :8].tolist() == want, g
    # a row twice is twice the row; both saturations; polarity
    big = np.full((2, 160), 30000, dtype=np.int16)
    big[1] = -30000
    y = mixdown.mix(big, [0, 2, 4, 6, 7], [0, 0, 1, 1, 0, 1, 0], np.array([4096, 4096, 4096, 4096, 4096, 4096, -4096], dtype=np.int16))
    assert (y[0] == 32767).all() and (y[1] == -32768).all() and not y[2].any() and (y[3] == -30000).all()
    # 4,096 inputs of (-32768, -32768): 2^30 in the sum, no wrap
    low = np.full((1, 160), -32768, dtype=np.int16)
    y = mixdown.mix(low, [0, 4096, 8192], np.zeros(8192, dtype=np.int32), np.repeat(np.array([-32768, 32767], dtype=np.int16), 4096))
    assert (y[0] == 32767).all() and (y[1] == -32768).all()
    for bad in (lambda: mixdown.mix(x, [0, 1], [5]), lambda: mixdown.mix(x, [0, 1], [-1]), lambda: mixdown.mix(x, [1, 1], [0]),
                lambda: mixdown.mix(x, [0, 2, 1], [0, 0]), lambda: mixdown.mix(x, [0, 1], [0], None, 3),
                lambda: mixdown.mix(x, [0, 4097], np.zeros(4097, dtype=np.int32))):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        mixdown.mix(x.astype(np.int32), [0, 1], [0])


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


def test_every_function_of_the_mixdown_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.MIXDOWN_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS):
        assert not set(_native.MIXDOWN_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    for name, value in (("MBX_MIXDOWN_PCM16", mixdown.PCM16), ("MBX_MIXDOWN_ULAW", mixdown.ULAW), ("MBX_MIXDOWN_ALAW", mixdown.ALAW),
                        ("MBX_MIXDOWN_UNITY", mixdown.UNITY), ("MBX_MIXDOWN_MAX_INPUTS", mixdown.MAX_INPUTS), ("MBX_SESSION_MIXDOWN", mixdown.SESSION_MIXDOWN)):
        assert int(re.search(rf"#define {name}\s+(\d+)u?\b", text).group(1)) == value, name
    assert (mixdown.PCM16, mixdown.ULAW, mixdown.ALAW, mixdown.UNITY, mixdown.MAX_INPUTS, mixdown.SESSION_MIXDOWN) == (0, 1, 2, 4096, 4096, 16)
    assert mixdown.SESSION_MIXDOWN & (1 | 2 | 4 | pcm8.SESSION_PCM8) == 0, "an outputs bit of its own"
    # the alignment rows of the new kinds are stated, in a table in the style of the one in mbx.h
    assert "Alignment, in the style of the table in mbx.h" in text
    for kind, align in (("mix rows", 16), ("bus pcm16", 16), ("bus bytes", 8)):
        assert re.search(rf"^ \*   {kind}\s+{align}\b", text, flags=re.M), kind
    # include/mbx.h and include/mbx_pcm8.h do not know the new calls or the new bit: a header of its own
    for other in ("mbx.h", "mbx_pcm8.h"):
        theirs = open(os.path.join(ROOT, "include", other)).read()
        assert not any(f in theirs for f in FUNCTIONS) and "MBX_SESSION_MIXDOWN" not in theirs and "mbx_mixdown_plan" not in theirs, other
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name


def _case(rng, rows, sizes):
    """buses of the given sizes over `rows` rows: gains of both signs with the extremes among them, a row twice in the first bus that
    has two inputs"""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    row = rng.integers(0, rows, size=n, dtype=np.int64).astype(np.int32)
    gain = rng.integers(-9000, 9001, size=n, dtype=np.int64).astype(np.int16)
    gain[rng.integers(0, n, size=max(1, n // 8))] = rng.choice(np.array([-32768, 32767, 4096, -4096, 0, 1, -1], dtype=np.int16), size=max(1, n // 8))
    for b, size in enumerate(sizes):
        if size >= 2:
            row[off[b] + 1] = row[off[b]]
            break
    return off, row, gain


def test_the_host_function_is_the_numpy_definition_in_all_three_forms():
    L = _lib()
    rng = np.random.default_rng(7)
    x = _rows(rng, 9)
    for sizes in ([1], [0], [2, 0, 1, 5, 13, 0], [48, 49, 4096, 3]):
        off, row, gain = _case(rng, 9, sizes) if sum(sizes) else (np.zeros(len(sizes) + 1, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int16))
        for g in (gain, None):
            for form in mixdown.FORMS:
                want = mixdown.mix(x, off, row, g, form)
                got = np.full(len(sizes) * 160 + 2, 0x5A, dtype=mixdown.out_dtype(form))
                rc = L.mbx_mixdown_host(form, len(sizes), off.ctypes.data, row.ctypes.data if row.size else None, None if g is None else g.ctypes.data,
                                        x.ctypes.data, 9, got[1:].ctypes.data)
                assert rc == 0, L.mbx_last_error()
                assert got[1:-1].tobytes() == want.tobytes() and got[0] == 0x5A and got[-1] == 0x5A, (sizes, form)
    # a unity single-input bus returns the row itself; as bytes, pcm8.compand of the row
    off, row = np.array([0, 1], dtype=np.int32), np.array([4], dtype=np.int32)
    for form, want in ((mixdown.PCM16, x[4]), (mixdown.ULAW, pcm8.compand(x[4], pcm8.LAW_ULAW)), (mixdown.ALAW, pcm8.compand(x[4], pcm8.LAW_ALAW))):
        got = np.zeros(160, dtype=mixdown.out_dtype(form))
        assert L.mbx_mixdown_host(form, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, got.ctypes.data) == 0
        assert got.tobytes() == want.tobytes(), form
    # its refusals, by name: the form, the plan's own, the pointers, rows short of the plan
    out = np.zeros(160, dtype=np.int16)
    bad = [(3, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"form"),
           (0, 0, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"n_buses"),
           (0, 1, None, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"bus_offset and src_row"),
           (0, 1, off.ctypes.data, None, None, x.ctypes.data, 5, out.ctypes.data, b"bus_offset and src_row"),
           (0, 1, off.ctypes.data, row.ctypes.data, None, None, 5, out.ctypes.data, b"pcm16 and out"),
           (0, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, None, b"pcm16 and out"),
           (0, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 4, out.ctypes.data, b"nrows")]
    for *args, part in bad:
        assert L.mbx_mixdown_host(*args) == INVALID, args
        assert b"mbx_mixdown_host" in L.mbx_last_error() and part in L.mbx_last_error(), L.mbx_last_error()
    assert not out.any()
    # their order: everything wrong at once, then one thing fewer each time -- the form, the plan's own, the pointers, the rows
    both = [(3, 0, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"form"),
            (0, 0, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"n_buses"),
            (0, 1, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"pcm16 and out"),
            (0, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 4, None, b"pcm16 and out"),
            (0, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 4, out.ctypes.data, b"nrows")]
    for *args, part in both:
        assert L.mbx_mixdown_host(*args) == INVALID, args
        assert L.mbx_last_error().startswith(b"mbx_mixdown_host: ") and part in L.mbx_last_error(), L.mbx_last_error()
    assert not out.any()


def test_a_plan_is_checked_on_the_host_before_a_device_is_asked_for():
    """every refusal with its text, on a host with no GPU as well; the handle comes back NULL"""
    L = _lib()
    ok_off, ok_row = np.array([0, 2, 3], dtype=np.int32), np.array([4, 4, 0], dtype=np.int32)
    many = np.zeros(4097, dtype=np.int32)

    def refused(part, n, off, row, gain=None, split=None, out=True):
        L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
        h = C.c_void_p(0x1234)
        args = (C.byref(h) if out else None, n, None if off is None else off.ctypes.data, None if row is None else row.ctypes.data, gain)
        rc = L.mbx_mixdown_plan_create(*args) if split is None else L.mbx_mixdown_plan_create_split(*args, split)
        assert rc == INVALID, (part, rc)
        assert b"mbx_mixdown_plan_create" in L.mbx_last_error() and part in L.mbx_last_error(), L.mbx_last_error()
        assert not out or h.value is None

    refused(b"handle", 2, ok_off, ok_row, out=False)
    refused(b"n_buses", 0, ok_off, ok_row)
    refused(b"n_buses", -3, ok_off, ok_row, split=4)
    refused(b"bus_offset and src_row", 2, None, ok_row)
    refused(b"bus_offset and src_row", 2, ok_off, None)
    refused(b"bus_offset[0]", 2, np.array([1, 2, 3], dtype=np.int32), ok_row)
    refused(b"must not decrease", 2, np.array([0, 2, 1], dtype=np.int32), ok_row)
    refused(b"MBX_MIXDOWN_MAX_INPUTS", 1, np.array([0, 4097], dtype=np.int32), many)
    refused(b"negative src_row", 2, ok_off, np.array([4, -1, 0], dtype=np.int32))
    refused(b"2^31-1", 2, ok_off, np.array([4, 2**31 - 1, 0], dtype=np.int32))
    refused(b"long_above", 2, ok_off, ok_row, split=-1)
    # NULL handles read as refusals, destroy takes NULL
    assert L.mbx_mixdown_plan_buses(None) == INVALID and L.mbx_mixdown_plan_rows(None) == INVALID and L.mbx_mixdown_plan_long_buses(None) == INVALID
    assert L.mbx_mixdown_plan_destroy(None) == 0


def test_the_launcher_and_the_session_call_refuse_their_arguments_before_they_ask_for_a_device():
    """in the manner of test_the_launcher_refuses_its_arguments_before_it_asks_for_a_device (tests/test_pcm8_host.py): never
    dereferenced, every call below is refused first, on a host with no GPU as well"""
    L = _lib()

    def refused(*args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert L.mbx_mixdown(*args) == INVALID, args
        text = L.mbx_last_error()
        assert b"mbx_mixdown:" in text, text
        return text

    assert b"form" in refused(None, 3, 0x1000, 4, 0x2000, None)
    assert b"form" in refused(None, -1, 0x1000, 4, 0x2000, None)
    for form in mixdown.FORMS:
        assert b"needed" in refused(None, form, None, 4, 0x2000, None)
        assert b"needed" in refused(None, form, 0x1000, 4, None, None)
        assert b"needed" in refused(None, form, 0x1000, 4, 0x2000, None)   # no plan
        for off in (2, 4, 8):   # d_pcm16 below 16
            text = refused(None, form, 0x1000 + off, 4, 0x2000, None)
            assert b"alignment" in text and b"mbx_mixdown.h" in text, text
        for off in (1, 2, 4, 8):   # d_out below 16 as int16, below 8 as bytes
            if form == mixdown.PCM16 or off < 8:
                text = refused(None, form, 0x1000, 4, 0x2000 + off, None)
                assert b"alignment" in text and b"mbx_mixdown.h" in text, (form, off, text)
            else:
                assert b"needed" in refused(None, form, 0x1000, 4, 0x2000 + off, None)   # aligned: the missing plan is what is left
    # the session call refuses a missing session by name, whatever else it is given
    for args in ((None, None, 0, 0x2000), (None, 0x3000, 1, 0x2000), (None, 0x3000, 0, None)):
        assert L.mbx_session_next_mixdown(*args) == INVALID and b"mbx_session_next_mixdown" in L.mbx_last_error()
