"""CPU suite for levels out and the gated mix-down (include/mbx_levels.h): the arithmetic of mbelib-neo_amd/csrc/mbx_levels.h and the
host-only checks of mbx_levels_plan.h through the stand-alone program tests/levels_check.cpp, built with AddressSanitizer and
UndefinedBehaviorSanitizer exactly as tests/test_mixdown_host.py builds its program (an executable of its own; nothing is loaded into
this process); the numpy definition (mbelib_neo_amd.levels) on known answers; mbx_pcm_levels_host and mbx_mixdown_gated_host held to
numpy in all three forms; a gate {0, 0} held to mbx_mixdown_host; the refusals of the launchers and of the session calls before a
device is asked for; the header held to the library's exports and to the ctypes table of its own (_native.LEVELS_SYMBOLS).  No GPU
compute here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

from mbelib_neo_amd import levels, mixdown, pcm8
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_levels.h")
INVALID = -1
FUNCTIONS = ["mbx_pcm_levels", "mbx_pcm_levels_host", "mbx_mixdown_gated", "mbx_mixdown_gated_host", "mbx_session_next_levels",
             "mbx_session_next_mixdown_gated"]
GATES = [(0, 0), (900, 0), (0, 1), (0, 3), (0, 8), (900, 1), (900, 3), (900, 8), (32768, 0), (32768, 2)]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/levels_check.cpp")
    exe = str(tmp_path_factory.mktemp("levels") / "levels_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "levels_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_levels_the_keys_the_thresholds_and_the_refusals_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"levels_check: ok \(16 lanes per row, loudest_n up to (\d+)\)", last)
    assert found, run.stdout
    assert int(found.group(1)) == levels.GATE_MAX_LOUDEST


def _rows(rng, rows):
    """rows of very different loudness (so that a peak gate and a ranking both have something to decide), full-range ones among them,
    with planted extremes at the first and the last position and behind the first: all -32768, all 0, a single 32767, +-1"""
    scale = rng.choice(np.array([3, 40, 700, 5000, 32768]), size=rows)
    x = (rng.integers(-32768, 32768, size=(rows, 160), dtype=np.int64) * scale[:, None] // 32768).astype(np.int16)
    planted = [np.full(160, -32768), np.zeros(160), np.eye(1, 160, 77)[0] * 32767, np.where(np.arange(160) & 1, -1, 1)]
    for r, p in zip((0, rows - 1, 1, 2)[:min(rows, 4)], planted):
        x[r] = p.astype(np.int16)
    return x


def test_the_numpy_definition_on_known_answers():
    x = np.zeros((6, 160), dtype=np.int16)
    x[0] = -32768
    x[2, 77] = 32767
    x[3] = np.where(np.arange(160) & 1, -1, 1)
    x[4, [0, 159]] = [-32768, 32767]
    x[5, 3] = -32767
    lv = levels.measure(x)
    assert lv.dtype == levels.LEVEL_DTYPE and lv.dtype.itemsize == 16 and lv.shape == (6,)
    assert [lv.dtype.fields[f][1] for f in ("energy", "peak", "clipped", "zero")] == [0, 8, 10, 12]
    assert lv["energy"].tolist() == [160 << 30, 0, 32767 ** 2, 160, (1 << 30) + 32767 ** 2, 32767 ** 2]
    assert lv["peak"].tolist() == [32768, 0, 32767, 1, 32768, 32767]
    assert lv["clipped"].tolist() == [160, 0, 1, 0, 2, 0] and not lv["zero"].any()
    assert levels.measure(np.zeros((0, 160), np.int16)).shape == (0,)
    # the gate: open at exactly the peak, closed one above; rows 2 and 5 tie in energy, the earlier position wins
    off, row = [0, 6, 6, 8], [5, 1, 2, 3, 0, 4, 2, 2]
    assert levels.chosen(lv, off, row).all()
    assert levels.chosen(lv, off, row, open_peak=32767).tolist() == [True, False, True, False, True, True, True, True]
    assert levels.chosen(lv, off, row, open_peak=32768).tolist() == [False, False, False, False, True, True, False, False]
    assert levels.chosen(lv, off, row, loudest_n=1).tolist() == [False, False, False, False, True, False, True, False]
    assert levels.chosen(lv, off, row, loudest_n=3).tolist() == [True, False, False, False, True, True, True, True]
    assert levels.chosen(lv, off, row, loudest_n=4).tolist() == [True, False, True, False, True, True, True, True]
    assert levels.chosen(lv, off, row, open_peak=2, loudest_n=8).tolist() == [True, False, True, False, True, True, True, True]
    assert levels.chosen(lv, off, row, open_peak=1, loudest_n=8).tolist() == [True, False, True, True, True, True, True, True]
    # the gated bus: the unchosen left out, silence by form where none is open, {0, 0} is mix itself
    gain = np.array([4096, 4096, -4096, 4096, 0, 2048, 4096, 4096], dtype=np.int16)
    for form in mixdown.FORMS:
        assert levels.mix_gated(x, off, row, gain, form).tobytes() == mixdown.mix(x, off, row, gain, form).tobytes()
    y = levels.mix_gated(x, off, row, gain, mixdown.PCM16, loudest_n=1)
    assert not y[0].any(), "row 0 is the loudest of bus 0 and has the gain 0: it still competes"
    assert not y[1].any() and y[2].tobytes() == x[2].tobytes()
    y = levels.mix_gated(x, [0, 2], [3, 1], None, mixdown.PCM16, open_peak=2)
    assert not y.any()
    assert (levels.mix_gated(x, [0, 2], [3, 1], None, mixdown.ULAW, open_peak=2) == 0xFF).all()
    assert (levels.mix_gated(x, [0, 2], [3, 1], None, mixdown.ALAW, open_peak=2) == 0xD5).all()
    for bad in (lambda: levels.chosen(lv, off, row, open_peak=32769), lambda: levels.chosen(lv, off, row, loudest_n=9),
                lambda: levels.chosen(lv, off, row, loudest_n=-1), lambda: levels.mix_gated(x, [0, 1], [6])):
        with pytest.raises(ValueError):
            bad()
    with pytest.raises(TypeError):
        levels.measure(x.astype(np.int32))


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


def test_every_function_of_the_levels_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.LEVELS_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS):
        assert not set(_native.LEVELS_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    for name, value in (("MBX_GATE_MAX_LOUDEST", levels.GATE_MAX_LOUDEST), ("MBX_SESSION_LEVELS", levels.SESSION_LEVELS)):
        assert int(re.search(rf"#define {name}\s+(\d+)u?\b", text).group(1)) == value, name
    assert (levels.GATE_MAX_LOUDEST, levels.SESSION_LEVELS) == (8, 32)
    # the outputs bit is disjoint from the other five: PCM16, PCMF, RESULTS (include/mbx.h), PCM8, MIXDOWN
    others = [1, 2, 4, pcm8.SESSION_PCM8, mixdown.SESSION_MIXDOWN]
    assert len(set(others)) == 5 and all(levels.SESSION_LEVELS & bit == 0 for bit in others)
    mbx_h = open(os.path.join(ROOT, "include", "mbx.h")).read()
    for name, bit in (("MBX_SESSION_PCM16", 1), ("MBX_SESSION_PCMF", 2), ("MBX_SESSION_RESULTS", 4)):
        assert int(re.search(rf"#define {name}\s+(\d+)u?\b", mbx_h).group(1)) == bit, name
    assert C.sizeof(levels.Gate) == 4 and levels.Gate.open_peak.offset == 0 and levels.Gate.loudest_n.offset == 2
    # the alignment rows of the new kinds are stated, in a table in the style of the one in mbx_mixdown.h
    assert "Alignment, in the style of the table in mbx_mixdown.h" in text
    for kind, align in (("level rows", 16), ("levels", 16), ("bus pcm16", 16), ("bus bytes", 8)):
        assert re.search(rf"^ \*   {kind}\s+{align}\b", text, flags=re.M), kind
    # the other headers do not know the new calls or the new bit: a header of its own
    for other in ("mbx.h", "mbx_pcm8.h", "mbx_mixdown.h"):
        theirs = open(os.path.join(ROOT, "include", other)).read()
        assert not any(f in theirs for f in FUNCTIONS) and "MBX_SESSION_LEVELS" not in theirs and "mbx_row_level" not in theirs, other
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
    """buses of the given sizes over `rows` rows: gains of both signs with 0 and the extremes among them, a row twice in the first
    bus that has two inputs, a row beside its negation's twin in the next"""
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    n = int(off[-1])
    row = rng.integers(0, rows, size=n, dtype=np.int64).astype(np.int32)
    gain = rng.integers(-9000, 9001, size=n, dtype=np.int64).astype(np.int16)
    if n:
        gain[rng.integers(0, n, size=max(1, n // 8))] = rng.choice(np.array([-32768, 32767, 4096, -4096, 0, 1, -1], dtype=np.int16), size=max(1, n // 8))
    for b, size in enumerate(sizes):
        if size >= 2:
            row[off[b] + 1] = row[off[b]]
            break
    return off, row, gain


def test_the_host_functions_are_the_numpy_definition_in_all_three_forms():
    L = _lib()
    rng = np.random.default_rng(11)
    x = _rows(rng, 40)
    x[6] = np.clip(x[6], -32767, 32767)
    x[7] = -x[6]   # a row beside its negation: equal energies
    want = levels.measure(x)
    got = np.full(42, 0x5A, dtype=np.uint8).repeat(16).view(levels.LEVEL_DTYPE)
    assert L.mbx_pcm_levels_host(x.ctypes.data, 40, got[1:].ctypes.data) == 0, L.mbx_last_error()
    assert got[1:-1].tobytes() == want.tobytes() and got[:1].tobytes() == b"\x5a" * 16 and got[-1:].tobytes() == b"\x5a" * 16
    assert (want["peak"] == 32768).any() and (want["clipped"] == 160).any() and (want["energy"] == 0).any()
    assert L.mbx_pcm_levels_host(x.ctypes.data, 0, got.ctypes.data) == 0
    for args in ((None, 4, got.ctypes.data), (x.ctypes.data, 4, None)):
        assert L.mbx_pcm_levels_host(*args) == INVALID and b"mbx_pcm_levels_host" in L.mbx_last_error()

    for sizes in ([1], [0], [2, 0, 1, 5, 13, 0, 9], [23, 257, 4096, 3]):
        off, row, gain = _case(rng, 40, sizes)
        if sum(sizes) >= 9:
            row[off[-2]:off[-2] + 2] = [6, 7]   # the row and its negation side by side in the last bus
        for g in (gain, None):
            for form in mixdown.FORMS:
                for peak, n in GATES:
                    gate = levels.Gate(peak, n)
                    expect = levels.mix_gated(x, off, row, g, form, peak, n)
                    out = np.full(len(sizes) * 160 + 2, 0x5A, dtype=mixdown.out_dtype(form))
                    rc = L.mbx_mixdown_gated_host(form, C.addressof(gate), len(sizes), off.ctypes.data, row.ctypes.data if row.size else None,
                                                  None if g is None else g.ctypes.data, x.ctypes.data, 40, out[1:].ctypes.data)
                    assert rc == 0, L.mbx_last_error()
                    assert out[1:-1].tobytes() == expect.tobytes() and out[0] == 0x5A and out[-1] == 0x5A, (sizes, form, peak, n)
                # a gate {0, 0} gives the bytes of mbx_mixdown_host
                plain = np.zeros(len(sizes) * 160, dtype=mixdown.out_dtype(form))
                assert L.mbx_mixdown_host(form, len(sizes), off.ctypes.data, row.ctypes.data if row.size else None, None if g is None else g.ctypes.data,
                                          x.ctypes.data, 40, plain.ctypes.data) == 0
                assert plain.tobytes() == levels.mix_gated(x, off, row, g, form, 0, 0).tobytes(), (sizes, form)
    # the gates decided something: with {900, 3} some bus lost inputs to the peak and some to the ranking
    lv = levels.measure(x)
    assert 0 < levels.chosen(lv, off, row, 900, 3).sum() < levels.chosen(lv, off, row, 900, 0).sum() < off[-1]
    # its refusals, by name: the gate's, the form, the plan's own, the pointers, rows short of the plan
    off, row = np.array([0, 1], dtype=np.int32), np.array([4], dtype=np.int32)
    out = np.zeros(160, dtype=np.int16)
    ok, nine, loud = levels.Gate(0, 0), levels.Gate(0, 9), levels.Gate(32769, 0)
    bad = [(0, None, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"gate is needed"),
           (0, C.addressof(nine), 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"MBX_GATE_MAX_LOUDEST"),
           (0, C.addressof(loud), 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"32768"),
           (3, C.addressof(ok), 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"form"),
           (0, C.addressof(ok), 0, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"n_buses"),
           (0, C.addressof(ok), 1, None, row.ctypes.data, None, x.ctypes.data, 5, out.ctypes.data, b"bus_offset and src_row"),
           (0, C.addressof(ok), 1, off.ctypes.data, row.ctypes.data, None, None, 5, out.ctypes.data, b"pcm16 and out"),
           (0, C.addressof(ok), 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, None, b"pcm16 and out"),
           (0, C.addressof(ok), 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 4, out.ctypes.data, b"nrows")]
    for *args, part in bad:
        assert L.mbx_mixdown_gated_host(*args) == INVALID, args
        assert b"mbx_mixdown_gated_host" in L.mbx_last_error() and part in L.mbx_last_error(), L.mbx_last_error()
    assert not out.any()
    # their order: everything wrong at once, then one thing fewer each time -- the gate, the form, the plan's own, the pointers, the rows
    both = [(3, None, 0, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"gate is needed"),
            (3, C.addressof(nine), 0, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"MBX_GATE_MAX_LOUDEST"),
            (3, C.addressof(ok), 0, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"form"),
            (0, C.addressof(ok), 0, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"n_buses"),
            (0, C.addressof(ok), 1, off.ctypes.data, row.ctypes.data, None, None, 4, None, b"pcm16 and out"),
            (0, C.addressof(ok), 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 4, None, b"pcm16 and out"),
            (0, C.addressof(ok), 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 4, out.ctypes.data, b"nrows")]
    for *args, part in both:
        assert L.mbx_mixdown_gated_host(*args) == INVALID, args
        assert L.mbx_last_error().startswith(b"mbx_mixdown_gated_host: ") and part in L.mbx_last_error(), L.mbx_last_error()
    assert not out.any()


def test_the_launchers_and_the_session_calls_refuse_their_arguments_before_they_ask_for_a_device():
    """never dereferenced: every call below is refused first, on a host with no GPU as well.  What needs a plan (rows short of it, the
    overlaps of the gated launch) is held through gated_launch_refused in levels_check.cpp and through the library in
    tests/test_gpu_levels.py."""
    L = _lib()

    def refused(fn, name, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = L.mbx_last_error()
        assert name + b":" in text, text
        return text

    lv = lambda *a: refused(L.mbx_pcm_levels, b"mbx_pcm_levels", *a)
    assert b"needed" in lv(None, 4, 0x2000, None) and b"needed" in lv(0x1000, 4, None, None)
    for off in (2, 4, 8):
        for args in ((0x1000 + off, 4, 0x2000, None), (0x1000, 4, 0x2000 + off, None)):
            text = lv(*args)
            assert b"alignment" in text and b"mbx_levels.h" in text, text
    assert b"overlap" in lv(0x1000, 4, 0x1000 + 4 * 320 - 16, None) and b"overlap" in lv(0x1040, 4, 0x1010, None)
    assert b"rows" in lv(0x1000, 2**31, 0x10, None)
    assert L.mbx_pcm_levels(0x1000, 0, 0x2000, None) == 0, "no rows: nothing is launched, no device is asked for"

    ok, nine, loud = levels.Gate(0, 0), levels.Gate(0, 9), levels.Gate(32769, 0)
    gd = lambda *a: refused(L.mbx_mixdown_gated, b"mbx_mixdown_gated", *a)
    assert b"gate is needed" in gd(None, None, 0, 0x1000, 4, 0x2000, 0x3000, None)
    assert b"MBX_GATE_MAX_LOUDEST" in gd(None, C.addressof(nine), 0, 0x1000, 4, 0x2000, 0x3000, None)
    assert b"32768" in gd(None, C.addressof(loud), 0, 0x1000, 4, 0x2000, 0x3000, None)
    g = C.addressof(ok)
    assert b"d_levels" in gd(None, g, 0, 0x1000, 4, None, 0x3000, None)
    assert b"form" in gd(None, g, 3, 0x1000, 4, 0x2000, 0x3000, None) and b"form" in gd(None, g, -1, 0x1000, 4, 0x2000, 0x3000, None)
    for form in mixdown.FORMS:
        assert b"needed" in gd(None, g, form, None, 4, 0x2000, 0x3000, None)
        assert b"needed" in gd(None, g, form, 0x1000, 4, 0x2000, None, None)
        assert b"needed" in gd(None, g, form, 0x1000, 4, 0x2000, 0x3000, None)   # no plan
        for off in (2, 4, 8):
            for args in ((0x1000 + off, 4, 0x2000, 0x3000), (0x1000, 4, 0x2000 + off, 0x3000)):   # d_pcm16, d_levels below 16
                text = gd(None, g, form, *args, None)
                assert b"alignment" in text and b"mbx_levels.h" in text, text
        for off in (1, 2, 4, 8):   # d_out below 16 as int16, below 8 as bytes
            if form == mixdown.PCM16 or off < 8:
                text = gd(None, g, form, 0x1000, 4, 0x2000, 0x3000 + off, None)
                assert b"alignment" in text and b"mbx_levels.h" in text, (form, off, text)
            else:
                assert b"needed" in gd(None, g, form, 0x1000, 4, 0x2000, 0x3000 + off, None)   # aligned: the missing plan is what is left
    # the session calls refuse a missing session by name, whatever else they are given
    for args in ((None, None), (None, 0x2000)):
        assert L.mbx_session_next_levels(*args) == INVALID and b"mbx_session_next_levels" in L.mbx_last_error()
    for args in ((None, None, 0, None, 0x2000), (None, 0x3000, 1, g, 0x2000), (None, 0x3000, 0, g, None)):
        assert L.mbx_session_next_mixdown_gated(*args) == INVALID and b"mbx_session_next_mixdown_gated" in L.mbx_last_error()
    # ... and no existing call learned the new bit by accident: a session cannot be made here, but the mask is in the source
    src = open(os.path.join(ROOT, "mbelib-neo_amd", "csrc", "mbx_session.hip")).read()
    assert "MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS)) != 0u" in src
