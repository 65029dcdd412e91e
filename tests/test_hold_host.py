"""CPU suite for the held gate (include/mbx_hold.h): the checks and the arithmetic of mbelib-neo_amd/csrc/mbx_hold_plan.h through the
stand-alone program tests/hold_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as tests/test_levels_host.py
builds its program (an executable of its own; nothing is loaded into this process); the numpy definition (mbelib_neo_amd.hold) on
hand-written known answers; mbx_mixdown_held_host held to numpy byte for byte, outputs and state after every frame, over the frame
script of tests/hold_cases.py in all three forms; the two identities of the header against levels.mix_gated and mixdown.mix; a hold
that changes mid-script; the condition the script must meet (every kind of event in every bus of 22 inputs or more and in the planted
buses); the refusals of the host call and of the launchers before a device is asked for; the header held to the library's exports and
to the ctypes table of its own (_native.HOLD_SYMBOLS).  No GPU compute here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import hold_cases as H
from mbelib_neo_amd import hold, levels, mixdown
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_hold.h")
INVALID = -1
FUNCTIONS = ["mbx_gate_state_create", "mbx_gate_state_destroy", "mbx_gate_state_inputs", "mbx_gate_state_reset", "mbx_gate_state_get",
             "mbx_gate_state_set", "mbx_mixdown_held", "mbx_mixdown_held_host", "mbx_session_next_mixdown_held"]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/hold_check.cpp")
    exe = str(tmp_path_factory.mktemp("hold") / "hold_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "hold_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_refusals_the_decision_the_weights_and_the_accumulator_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"hold_check: ok \(ramp_log2 up to (\d+), loudest_n up to (\d+)\)", last)
    assert found, run.stdout
    assert (int(found.group(1)), int(found.group(2))) == (hold.MAX_RAMP_LOG2, levels.GATE_MAX_LOUDEST)


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


def test_every_function_of_the_hold_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.HOLD_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS, _native.LEVELS_SYMBOLS):
        assert not set(_native.HOLD_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    assert int(re.search(r"#define MBX_HOLD_MAX_RAMP_LOG2\s+(\d+)\b", text).group(1)) == hold.MAX_RAMP_LOG2 == 7
    assert C.sizeof(hold.Hold) == 8
    assert [getattr(hold.Hold, f).offset for f in ("open_peak", "close_peak", "hang_frames", "loudest_n", "ramp_log2")] == [0, 2, 4, 6, 7]
    assert hold.STATE_DTYPE.itemsize == 4 and [hold.STATE_DTYPE.fields[f][1] for f in ("hang_left", "open", "on")] == [0, 2, 3]
    # the header states the accumulator bound, the two identities and whose duty one state per stream is
    for part in ("4,096 * (2^18 + 2) < 2^31", "Two identities follow", "ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME", "latches", "two states"):
        assert part in text, part
    # the older headers point here and know none of the new calls
    for other in ("mbx.h", "mbx_pcm8.h", "mbx_mixdown.h", "mbx_levels.h"):
        theirs = open(os.path.join(ROOT, "include", other)).read()
        assert not any(f in theirs for f in FUNCTIONS) and "mbx_gate_input_state" not in theirs, other
    for other in ("mbx_mixdown.h", "mbx_levels.h"):
        assert "mbx_hold.h" in open(os.path.join(ROOT, "include", other)).read(), other
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name


def test_the_numpy_definition_on_known_answers():
    """a bus of two inputs at unity under {900, 500, 2, 0, 3}: input 0 opens, stays, is held by the hysteresis, by the hang for two
    frames, expires and opens again; input 1 never reaches open_peak.  R = 8."""
    off, row = [0, 2], [0, 1]
    h = (900, 500, 2, 0, 3)
    value = [1000, 1000, 600, -100, -100, -100, -100, 1000]       # every sample of row 0, frame by frame
    states = [(2, 1, 1), (2, 1, 1), (2, 1, 1), (1, 1, 1), (0, 1, 1), (0, 0, 0), (0, 0, 0), (2, 1, 1)]
    rising = [125, 250, 375, 500, 625, 750, 875] + [1000] * 153   # (1000 q + 4) >> 3, q = 1 .. 8
    falling = [-87, -75, -62, -50, -37, -25, -12] + [0] * 153     # (-100 q + 4) >> 3, q = 7 .. 0: floors, half an LSB rounds up
    want = [rising, [1000] * 160, [600] * 160, [-100] * 160, [-100] * 160, falling, [0] * 160, rising]
    st = hold.zero_state(2)
    for f, v in enumerate(value):
        x = np.zeros((2, 160), dtype=np.int16)
        x[0] = v
        x[1] = 899 if f % 2 else -899   # one below open_peak: closed throughout
        out, st = hold.step(x, off, row, None, mixdown.PCM16, h, st)
        assert out.dtype == np.int16 and out.shape == (1, 160) and out[0].tolist() == want[f], f
        assert st.dtype == hold.STATE_DTYPE and st[0].tolist() == states[f] and st[1].tolist() == (0, 0, 0), f
    # the same rising frame as bytes; a step (ramp_log2 = 0) is the whole row at once; silence by form
    x = np.zeros((2, 160), dtype=np.int16)
    x[0] = 1000
    for form in (mixdown.ULAW, mixdown.ALAW):
        out, _ = hold.step(x, off, row, None, form, h, hold.zero_state(2))
        assert out.dtype == np.uint8 and out.tobytes() == mixdown.mix(np.array([rising], dtype=np.int16), [0, 1], [0], None, form).tobytes()
    out, _ = hold.step(x, off, row, None, mixdown.PCM16, (900, 500, 2, 0, 0), hold.zero_state(2))
    assert out[0].tolist() == [1000] * 160
    x[0] = 899
    assert (hold.step(x, off, row, None, mixdown.ULAW, h, hold.zero_state(2))[0] == 0xFF).all()
    assert (hold.step(x, off, row, None, mixdown.ALAW, h, hold.zero_state(2))[0] == 0xD5).all()
    # "the loudest 1": a held input competes with the energy it has now, and loses the bus to a louder one while it is still open
    one = (900, 500, 2, 1, 3)
    x[0], x[1] = 1000, 0
    _, st = hold.step(x, off, row, None, mixdown.PCM16, one, hold.zero_state(2))
    x[0], x[1] = 100, 950
    out, st = hold.step(x, off, row, None, mixdown.PCM16, one, st)
    assert st.tolist() == [(1, 1, 0), (2, 1, 1)]
    assert out[0, :8].tolist() == [(100 * (7 - n) + 4 >> 3) + (950 * (n + 1) + 4 >> 3) for n in range(8)] and (out[0, 8:] == 950).all()
    # equal energies: the earlier position wins; a row twice in a bus has two states
    x[0], x[1] = 1000, -1000
    _, st = hold.step(x, off, row, None, mixdown.PCM16, one, hold.zero_state(2))
    assert st.tolist() == [(2, 1, 1), (2, 1, 0)]
    _, st = hold.step(x, [0, 2], [1, 1], None, mixdown.PCM16, one, hold.zero_state(2))
    assert st.tolist() == [(2, 1, 1), (2, 1, 0)]
    # close_peak = 0 latches
    latch = (900, 0, 0, 0, 0)
    _, st = hold.step(x, off, row, None, mixdown.PCM16, latch, hold.zero_state(2))
    x[:] = 0
    _, st = hold.step(x, off, row, None, mixdown.PCM16, latch, st)
    assert st.tolist() == [(0, 1, 1), (0, 1, 1)]
    for bad in ((901, 902, 0, 0, 0), (32769, 0, 0, 0, 0), (900, 500, 0, 9, 0), (900, 500, 0, 0, 8), (900, 500, 65536, 0, 0)):
        with pytest.raises(ValueError):
            hold.step(x, off, row, None, mixdown.PCM16, bad, hold.zero_state(2))
    for bad_state in ([(0, 2, 0), (0, 0, 0)], [(0, 0, 1), (0, 0, 0)], [(0, 1, 2), (0, 0, 0)]):
        with pytest.raises(ValueError):
            hold.step(x, off, row, None, mixdown.PCM16, h, np.array(bad_state, dtype=hold.STATE_DTYPE))
    with pytest.raises(ValueError):
        hold.step(x, off, row, None, mixdown.PCM16, h, hold.zero_state(3))
    with pytest.raises(ValueError):
        hold.step(x, off, row, None, 3, h, hold.zero_state(2))


def test_the_script_shows_every_bus_of_22_inputs_or_more_and_the_planted_buses_every_kind_of_event():
    """from numpy alone, under every hold of the suites: rising, falling, steady, hysteresis hold, hang hold, expiry"""
    sizes = H.script()[4]
    must = [b for b, n in enumerate(sizes) if n >= 22] + list(H.planted_buses())
    assert [sizes[b] for b in must] == [22, 23, 24, 255, 256, 257, 4096, 2, 9]
    for h in H.HOLDS:
        got = H.seen(h)
        missing = [(kind, sizes[b]) for kind in H.KINDS for b in must if not got[kind][b]]
        assert not missing, (h, missing)


def _host(L, form, h, off, row, gain, x, state, n_buses):
    """mbx_mixdown_held_host between guard elements: (out, state after); `state` is not changed"""
    hd = H.hold_of(h)
    out = np.full(n_buses * 160 + 2, 0x5A, dtype=mixdown.out_dtype(form))
    st = np.full(state.size + 2, 0x5A, dtype=np.uint8).repeat(4).view(hold.STATE_DTYPE)
    st[1:-1] = state
    rc = L.mbx_mixdown_held_host(form, C.addressof(hd), n_buses, off.ctypes.data, row.ctypes.data, None if gain is None else gain.ctypes.data,
                                 x.ctypes.data, x.shape[0], st[1:].ctypes.data, out[1:].ctypes.data)
    assert rc == 0, L.mbx_last_error()
    assert out[0] == 0x5A and out[-1] == 0x5A and st[:1].tobytes() == b"\x5a" * 4 and st[-1:].tobytes() == b"\x5a" * 4
    return out[1:-1].reshape(n_buses, 160), st[1:-1].copy()


@pytest.mark.parametrize("form", mixdown.FORMS)
def test_the_host_function_is_the_numpy_definition_frame_by_frame_outputs_and_state(form):
    L = _lib()
    x, off, row, gain, sizes = H.script()
    for h in H.HOLDS:
        st = hold.zero_state(off[-1])
        for f, (want_out, want_state) in enumerate(H.expected(h, form)):
            out, st = _host(L, form, h, off, row, gain, x[f], st, len(sizes))
            bad = np.flatnonzero((out != want_out).any(axis=1))
            assert out.tobytes() == want_out.tobytes(), (h, form, f, "buses", bad[:8], "of sizes", [sizes[b] for b in bad[:8]])
            assert st.tobytes() == want_state.tobytes(), (h, form, f, np.flatnonzero(st != want_state)[:8])


def test_the_two_identities_against_the_gated_and_the_plain_mix_down():
    L = _lib()
    x, off, row, gain, sizes = H.script()
    # {t, t, 0, n, 0} on zeroed state: in every frame the bytes of the gated mix-down under {t, n}
    for t, n in ((H.OPEN, 0), (H.OPEN, 3), (0, 1), (32768, 8)):
        for form in mixdown.FORMS:
            st_np = st_c = hold.zero_state(off[-1])
            for f in range(H.FRAMES):
                want = levels.mix_gated(x[f], off, row, gain, form, t, n)
                out_np, st_np = hold.step(x[f], off, row, gain, form, (t, t, 0, n, 0), st_np)
                out_c, st_c = _host(L, form, (t, t, 0, n, 0), off, row, gain, x[f], st_c, len(sizes))
                assert out_np.tobytes() == want.tobytes() and out_c.tobytes() == want.tobytes(), (t, n, form, f)
                assert st_np["on"].tobytes() == levels.chosen(levels.measure(x[f]), off, row, t, n).astype(np.uint8).tobytes()
    # open_peak = 0, loudest_n = 0: from the second frame on the bytes of the plain mix-down; from the first if ramp_log2 = 0
    for h in ((0, 0, 0, 0, 0), (0, 0, 5, 0, 3), (0, 0, 0, 0, 7)):
        for form in mixdown.FORMS:
            st_np = st_c = hold.zero_state(off[-1])
            differs = False
            for f in range(4):
                want = mixdown.mix(x[f], off, row, gain, form)
                out_np, st_np = hold.step(x[f], off, row, gain, form, h, st_np)
                out_c, st_c = _host(L, form, h, off, row, gain, x[f], st_c, len(sizes))
                assert out_np.tobytes() == out_c.tobytes()
                if f or h[4] == 0:
                    assert out_np.tobytes() == want.tobytes(), (h, form, f)
                else:
                    differs = out_np.tobytes() != want.tobytes()
                assert st_np["on"].all() and st_np["open"].all()
            assert differs == (h[4] != 0), "the first frame fades every input in"


def test_a_hold_that_changes_mid_script_loudest_0_then_3_then_0():
    """after four frames of "every open input" the 4,096 bus has hundreds of inputs on; "the 3 loudest" makes all but 3 fall at once"""
    L = _lib()
    x, off, row, gain, sizes = H.script()
    holds = [(H.OPEN, H.CLOSE, H.HANG, n, 3) for n in (0, 0, 0, 0, 3, 3, 3, 3, 0, 0, 0, 0)]
    big = sizes.index(4096)
    for form in (mixdown.PCM16, mixdown.ALAW):
        steps = H.run(holds, form)
        st = hold.zero_state(off[-1])
        for f, (want_out, want_state) in enumerate(steps):
            out, st = _host(L, form, holds[f], off, row, gain, x[f], st, len(sizes))
            assert out.tobytes() == want_out.tobytes() and st.tobytes() == want_state.tobytes(), (form, f)
    on = [int(s["on"][off[big]:off[big + 1]].sum()) for _, s in steps]
    assert on[3] > 300 and on[4] == 3 and on[8] > 300, on
    fell = hold.codes(steps[3][1], steps[4][1])[off[big]:off[big + 1]]
    assert (fell == hold.FALLING).sum() > 300 and (hold.codes(steps[7][1], steps[8][1])[off[big]:off[big + 1]] == hold.RISING).sum() > 300


def test_the_host_call_and_the_launchers_refuse_their_arguments_before_they_ask_for_a_device():
    """never dereferenced: every call below is refused first, on a host with no GPU as well.  What needs a plan (a state of another
    plan, a bad record given to mbx_gate_state_set) is held through hold_check.cpp and through the library in tests/test_gpu_hold.py."""
    L = _lib()

    def refused(fn, name, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = L.mbx_last_error()
        assert name + b":" in text, text
        return text

    x = np.zeros((5, 160), dtype=np.int16)
    off, row = np.array([0, 1], dtype=np.int32), np.array([4], dtype=np.int32)
    out, st = np.zeros(160, dtype=np.int16), hold.zero_state(1)
    ok = hold.Hold(900, 500, 2, 3, 3)
    g = C.addressof(ok)
    bad_holds = [(hold.Hold(500, 501, 0, 0, 0), b"close_peak is above open_peak"), (hold.Hold(32769, 0, 0, 0, 0), b"32768"),
                 (hold.Hold(900, 500, 0, 9, 0), b"MBX_GATE_MAX_LOUDEST"), (hold.Hold(900, 500, 0, 0, 8), b"MBX_HOLD_MAX_RAMP_LOG2")]
    hh = lambda *a: refused(L.mbx_mixdown_held_host, b"mbx_mixdown_held_host", *a)
    good = [0, g, 1, off.ctypes.data, row.ctypes.data, None, x.ctypes.data, 5, st.ctypes.data, out.ctypes.data]

    def but(at, value):
        args = list(good)
        args[at] = value
        return args

    assert b"hold is needed" in hh(*but(1, None))
    for bad, part in bad_holds:
        assert part in hh(*but(1, C.addressof(bad)))
    assert b"form" in hh(*but(0, 3)) and b"n_buses" in hh(*but(2, 0)) and b"bus_offset and src_row" in hh(*but(3, None))
    assert b"pcm16 and out" in hh(*but(6, None)) and b"pcm16 and out" in hh(*but(9, None)) and b"nrows" in hh(*but(7, 4))
    assert b"state is needed" in hh(*but(8, None))
    for record in ((0, 2, 0), (0, 1, 2), (0, 0, 1)):
        wrong = np.array([record], dtype=hold.STATE_DTYPE)
        assert b"state record" in hh(*but(8, wrong.ctypes.data))
        assert wrong[0].tolist() == record
    # their order: everything wrong at once, then one thing fewer each time -- the hold, the form, the plan's own, the pointers, the
    # rows, the missing state, the bad record
    wrong = np.array([(0, 0, 1)], dtype=hold.STATE_DTYPE)
    worst = [3, C.addressof(bad_holds[0][0]), 0, off.ctypes.data, row.ctypes.data, None, None, 4, None, None]
    for at, value, part in ((None, None, bad_holds[0][1]), (1, g, b"form"), (0, 0, b"n_buses"), (2, 1, b"pcm16 and out"),
                            (6, x.ctypes.data, b"pcm16 and out"), (9, out.ctypes.data, b"nrows"), (7, 5, b"state is needed"),
                            (8, wrong.ctypes.data, b"state record")):
        if at is not None:
            worst[at] = value
        text = hh(*worst)
        assert text.startswith(b"mbx_mixdown_held_host: ") and part in text, text
    worst[1] = None   # no hold at all, in front of a bad record and of everything else
    worst[0], worst[2], worst[6], worst[7] = 3, 0, None, 4
    assert b"hold is needed" in hh(*worst)
    assert not out.any() and not st.view(np.uint32).any() and wrong[0].tolist() == (0, 0, 1)
    assert L.mbx_mixdown_held_host(*good) == 0, L.mbx_last_error()

    # the launcher: a zeroed stand-in for a state (never reached: no plan can be made without a device, and "no plan" is refused first)
    fake = (C.c_uint64 * 8)()
    s = C.addressof(fake)
    hd = lambda *a: refused(L.mbx_mixdown_held, b"mbx_mixdown_held", *a)
    assert b"hold is needed" in hd(None, None, s, 0, 0x1000, 4, 0x2000, 0x3000, None)
    for bad, part in bad_holds:
        assert part in hd(None, C.addressof(bad), s, 0, 0x1000, 4, 0x2000, 0x3000, None)
    assert b"state is needed" in hd(None, g, None, 0, 0x1000, 4, 0x2000, 0x3000, None)
    assert b"d_levels" in hd(None, g, s, 0, 0x1000, 4, None, 0x3000, None)
    assert b"form" in hd(None, g, s, 3, 0x1000, 4, 0x2000, 0x3000, None) and b"form" in hd(None, g, s, -1, 0x1000, 4, 0x2000, 0x3000, None)
    for form in mixdown.FORMS:
        assert b"needed" in hd(None, g, s, form, None, 4, 0x2000, 0x3000, None)
        assert b"needed" in hd(None, g, s, form, 0x1000, 4, 0x2000, None, None)
        assert b"needed" in hd(None, g, s, form, 0x1000, 4, 0x2000, 0x3000, None)   # no plan
        for o in (2, 4, 8):
            for args in ((0x1000 + o, 4, 0x2000, 0x3000), (0x1000, 4, 0x2000 + o, 0x3000)):   # d_pcm16, d_levels below 16
                text = hd(None, g, s, form, *args, None)
                assert b"alignment" in text and b"mbx_levels.h" in text, text
        for o in (1, 2, 4, 8):   # d_out below 16 as int16, below 8 as bytes
            if form == mixdown.PCM16 or o < 8:
                assert b"alignment" in hd(None, g, s, form, 0x1000, 4, 0x2000, 0x3000 + o, None), (form, o)
            else:
                assert b"needed" in hd(None, g, s, form, 0x1000, 4, 0x2000, 0x3000 + o, None)   # aligned: the missing plan is what is left
    # the state calls and the session call, by name
    handle = C.c_void_p(0x5A5A)
    assert b"plan is needed" in refused(L.mbx_gate_state_create, b"mbx_gate_state_create", C.byref(handle), None) and handle.value is None
    refused(L.mbx_gate_state_create, b"mbx_gate_state_create", None, None)
    assert L.mbx_gate_state_destroy(None) == 0 and L.mbx_gate_state_inputs(None) == INVALID
    refused(L.mbx_gate_state_reset, b"mbx_gate_state_reset", None, None)
    refused(L.mbx_gate_state_get, b"mbx_gate_state_get", None, st.ctypes.data, None)
    refused(L.mbx_gate_state_set, b"mbx_gate_state_set", None, st.ctypes.data, None)
    for args in ((None, None, 0, None, None, 0x2000), (None, 0x3000, 1, g, s, 0x2000), (None, 0x3000, 0, g, s, None)):
        assert L.mbx_session_next_mixdown_held(*args) == INVALID and b"mbx_session_next_mixdown_held" in L.mbx_last_error()
