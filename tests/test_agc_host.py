"""CPU suite for levelled rows (include/mbx_agc.h): the checks and the arithmetic of mbelib-neo_amd/csrc/mbx_agc_plan.h through the
stand-alone program tests/agc_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as tests/test_hold_host.py
builds its program (an executable of its own; nothing is loaded into this process); the numpy definition (mbelib_neo_amd.agc) on
hand-written known answers; the condition the script of tests/agc_cases.py must meet, asserted from agc.step; mbx_pcm_agc_host held to
numpy bit for bit, rows and state, frame by frame and with T = 3 in one call, over that script under both parameter sets and every
ramp_log2; the three identities of the header and "one call of T = 3 is three calls of T = 1"; the refusals of the host call and of
the launcher before a device is asked for; the header held to the library's exports and to the ctypes table of its own
(_native.AGC_SYMBOLS).  No GPU compute here.

"An envelope decaying to below floor_peak" is read as: in a row that is not frozen the decayed envelope env0 - ((env0 * release +
255) >> 8) lies below floor_peak while env0 did not, so that the peak takes over -- the new envelope itself is never below
floor_peak, being at least the peak of a row that was not frozen."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import agc_cases as A
from mbelib_neo_amd import agc
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_agc.h")
INVALID = -1
FUNCTIONS = ["mbx_agc_state_create", "mbx_agc_state_destroy", "mbx_agc_state_streams", "mbx_agc_state_reset", "mbx_agc_state_get", "mbx_agc_state_set",
             "mbx_pcm_agc", "mbx_pcm_agc_host", "mbx_session_next_agc"]
N, F = A.STREAMS, A.FRAMES


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/agc_check.cpp")
    exe = str(tmp_path_factory.mktemp("agc") / "agc_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "agc_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_refusals_the_bounds_and_the_arithmetic_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"agc_check: ok \(ramp_log2 up to (\d+), gains up to (\d+)\)", last)
    assert found, run.stdout
    assert (int(found.group(1)), int(found.group(2))) == (agc.MAX_RAMP_LOG2, agc.MAX_GAIN)


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


def test_every_function_of_the_agc_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.AGC_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS, _native.LEVELS_SYMBOLS, _native.HOLD_SYMBOLS):
        assert not set(_native.AGC_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    assert int(re.search(r"#define MBX_AGC_UNITY_Q10\s+(\d+)\b", text).group(1)) == agc.UNITY == 1024
    assert int(re.search(r"#define MBX_AGC_MAX_GAIN_Q10\s+(\d+)\b", text).group(1)) == agc.MAX_GAIN == 32768
    assert re.search(r"#define MBX_AGC_MAX_RAMP_LOG2\s+MBX_HOLD_MAX_RAMP_LOG2\b", text) and agc.MAX_RAMP_LOG2 == 7
    assert C.sizeof(agc.Agc) == 12
    assert [getattr(agc.Agc, f).offset for f, _ in agc.Agc._fields_] == [0, 2, 4, 6, 8, 9, 10, 11]
    assert agc.RECORD_DTYPE.itemsize == 4 and [agc.RECORD_DTYPE.fields[f][1] for f in ("gain_q10", "env")] == [0, 2]
    assert agc.fresh_state(3).view(np.uint32).tolist() == [1024] * 3
    # the header states the bounds, the identities, the pass-through, whose duty a doubled entry is and what a session leaves alone
    for part in ("2^15 * 2^15 = 2^30", "2^22", "< 2^24", "< 2^25", "Three identities follow", "NO LOOK-AHEAD", "PASSED THROUGH", "listed TWICE",
                 "ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME", "pcmf, results and records are untouched"):
        assert part in text, part
    for other in ("mbx.h", "mbx_pcm8.h", "mbx_mixdown.h", "mbx_levels.h", "mbx_hold.h"):
        theirs = open(os.path.join(ROOT, "include", other)).read()
        assert not any(f in theirs for f in FUNCTIONS) and "mbx_agc_record" not in theirs, other
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
    """one stream under {target 8000, floor 200, gains 512 .. 4096, release 128, rise 64, ramp_log2 2}: R = 4"""
    a = (8000, 200, 512, 4096, 128, 64, 2)
    x = np.zeros((1, 160), dtype=np.int16)
    st = agc.fresh_state(1)

    def run(value):
        nonlocal st
        x[0] = value
        out, st, ev = agc.step(x, 1, a, st)
        return out[0].tolist(), st[0].tolist(), int(ev[0])

    # silence: frozen on the fresh state, bit for bit
    assert run(100) == ([100] * 160, (1024, 0), agc.FREEZE)
    # 1000: env 1000, want 8192 -> 4096; the gain may rise by (1024 * 64 + 255) >> 8 = 256 to 1280, over 4 samples: 1088, 1152, 1216, 1280
    out, rec, ev = run(1000)
    assert (rec, ev) == ((1280, 1000), agc.RISE_SLEWED)
    assert out[:5] == [(1000 * g + 512) >> 10 for g in (1088, 1152, 1216, 1280, 1280)] == [1063, 1125, 1188, 1250, 1250] and out[4:] == [1250] * 156
    # -1000: the same envelope; 1280 + 320 = 1600
    out, rec, ev = run(-1000)
    assert (rec, ev) == ((1600, 1000), agc.RISE_SLEWED) and out[3:] == [(-1000 * 1600 + 512) >> 10] * 157 == [-1562] * 157
    # 300: the envelope decays by half (1000 - 500) and stays above the peak: want 16384 -> 4096, 1600 + 400
    assert run(300)[1:] == ((2000, 500), agc.RISE_SLEWED)
    # 50: frozen on a raised gain: the static gain 2000
    assert run(50) == ([(50 * 2000 + 512) >> 10] * 160, (2000, 500), agc.FREEZE)
    # 20000: the envelope jumps, want 409 -> 512: the gain falls at once over 4 samples, 2000 -> 1628, 1256, 884, 512 (no look-ahead:
    # the first samples are louder than the rest)
    out, rec, ev = run(20000)
    assert (rec, ev) == ((512, 20000), agc.FALL)
    assert out[:5] == [(20000 * g + 512) >> 10 for g in (1628, 1256, 884, 512, 512)] == [31797, 24531, 17266, 10000, 10000]
    out, rec, ev = run(-20000)
    assert (rec, ev) == ((512, 20000), agc.HOLD) and out == [-10000] * 160
    # 4000: env 10000 > peak, want 819; 512 + 128 = 640, then 800, then the rise reaches 819 and holds there as the envelope settles
    assert run(4000)[1:] == ((640, 10000), agc.RISE_SLEWED)
    assert run(4000)[1:] == ((800, 5000), agc.RISE_SLEWED)        # want 1638
    assert run(4000)[1:] == ((1000, 4000), agc.RISE_SLEWED)       # want 2048, 800 + 200
    assert run(8000)[1:] == ((1024, 8000), agc.RISE_REACHED)      # want 1024 <= 1250
    assert run(8000)[1:] == ((1024, 8000), agc.HOLD)
    # -32768 at a static x 32 and x 1/1024
    x[0] = -32768
    top = agc.fresh_state(1)
    top["gain_q10"] = 32768
    out, after, _ = agc.step(x, 1, (32767, 1, 32768, 32768, 255, 255, 7), top)
    assert (out == -32768).all() and after[0].tolist() == (32768, 32768)
    out, after, _ = agc.step(x, 1, (1, 1, 1, 1, 0, 0, 0), top)
    assert (out == -32).all() and after[0].tolist() == (1, 32768)
    # an entry outside the state is passed through; T = 0 and no rows
    out, after, ev = agc.step(x, 1, a, top, stream_index=[5])
    assert out.tobytes() == x.tobytes() and after.tobytes() == top.tobytes() and ev.tolist() == [agc.PASSED]
    out, after, ev = agc.step(np.zeros((0, 160), np.int16), 0, a, top)
    assert out.shape == (0, 160) and after.tobytes() == top.tobytes() and ev.size == 0
    for bad in ((0, 200, 512, 4096, 0, 0, 0), (32768, 200, 512, 4096, 0, 0, 0), (8000, 0, 512, 4096, 0, 0, 0), (8000, 32769, 512, 4096, 0, 0, 0),
                (8000, 200, 0, 4096, 0, 0, 0), (8000, 200, 512, 32769, 0, 0, 0), (8000, 200, 4097, 4096, 0, 0, 0), (8000, 200, 512, 4096, 256, 0, 0),
                (8000, 200, 512, 4096, 0, 256, 0), (8000, 200, 512, 4096, 0, 0, 8), (8000, 200, 512, 4096, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            agc.step(x, 1, bad, top)
    for record in ((0, 0), (32769, 0), (1024, 32769)):
        with pytest.raises(ValueError):
            agc.step(x, 1, a, np.array([record], dtype=agc.RECORD_DTYPE))
    with pytest.raises(ValueError):
        agc.step(x, 1, a, top, stream_index=[0, 0])
    with pytest.raises(ValueError):
        agc.step(np.zeros((3, 160), np.int16), 2, a, top)


@pytest.mark.parametrize("ramp", A.RAMPS)
def test_the_script_shows_every_kind_of_event_at_every_ramp(ramp):
    """from numpy alone: each kind at least once under one of the two parameter sets, and what each set is there for under that set"""
    got = {name: A.coverage(name, ramp) for name in A.SETS}
    missing = set(A.KINDS) - got["voice"] - got["extreme"]
    assert not missing, (ramp, sorted(missing))
    assert {"freeze-fresh", "freeze-raised", "hold", "fall", "rise-slewed", "rise-reached", "want-at-min", "want-at-max", "decay-wins",
            "decay-below-floor"} <= got["voice"], (ramp, sorted(got["voice"]))
    assert {"freeze-fresh", "freeze-raised", "hold", "rise-slewed", "rise-reached", "saturated-high", "saturated-low",
            "full-scale-at-top-gain"} <= got["extreme"], (ramp, sorted(got["extreme"]))
    if ramp >= 2:   # a gain that falls over four samples or more clips in them
        assert {"saturated-high", "saturated-low"} <= got["voice"], (ramp, sorted(got["voice"]))
    amp = np.abs(A.script().astype(np.int64)).max(axis=2).T
    assert amp.tolist() == A.amplitudes().tolist() and (A.script() == -32768).any() and (A.script() == 32767).any()


def _host(L, a, state, T, x, index=None, in_place=False, streams=None):
    """mbx_pcm_agc_host between guard elements: (out, state after); `state` and `x` are not changed"""
    streams = state.size if streams is None else streams
    rows = x.shape[0]
    st = np.full(state.size + 2, 0x5A, dtype=np.uint8).repeat(4).view(agc.RECORD_DTYPE)
    st[1:-1] = state
    out = np.full((rows + 2) * 160, 0x5A5A, dtype=np.int16)
    src = np.ascontiguousarray(x)
    if in_place:
        out[160:-160] = src.reshape(-1)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    rc = L.mbx_pcm_agc_host(C.addressof(a), st[1:].ctypes.data, streams, None if idx is None else idx.ctypes.data, rows // T if T else 0, T,
                            out[160:].ctypes.data if in_place else src.ctypes.data, out[160:].ctypes.data)
    assert rc == 0, L.mbx_last_error()
    assert (out[:160] == 0x5A5A).all() and (out[-160:] == 0x5A5A).all() and st[:1].tobytes() == b"\x5a" * 4 and st[-1:].tobytes() == b"\x5a" * 4
    return out[160:-160].reshape(rows, 160).copy(), st[1:-1].copy()


@pytest.mark.parametrize("name,ramp", A.CASES)
def test_the_host_function_is_the_numpy_definition_frame_by_frame_and_three_frames_a_call(name, ramp):
    L = _lib()
    a = A.params(name, ramp)
    st = agc.fresh_state(N)
    for f, (want_out, want_state, _, before) in enumerate(A.expected(name, ramp)):
        out, st = _host(L, a, st, 1, A.script()[f], in_place=bool(f & 1))
        assert out.tobytes() == want_out.tobytes(), (name, ramp, f, "streams", np.flatnonzero((out != want_out).any(axis=1)))
        assert st.tobytes() == want_state.tobytes(), (name, ramp, f, st, want_state)
    # T = 3 in one call: the rows regathered stream-major; numpy's own T = 3 is its frame-by-frame run, and so is the library's
    st = st_np = agc.fresh_state(N)
    for k in range(F // 3):
        x3 = A.rows(3 * k, 3)
        out, st = _host(L, a, st, 3, x3, in_place=bool(k & 1))
        out_np, st_np, _ = agc.step(x3, 3, a, st_np)
        steps = A.expected(name, ramp)[3 * k:3 * k + 3]
        frame_by_frame = np.stack([s[0] for s in steps]).transpose(1, 0, 2).reshape(N * 3, 160)
        assert out.tobytes() == out_np.tobytes() == frame_by_frame.tobytes(), (name, ramp, k)
        assert st.tobytes() == st_np.tobytes() == steps[-1][1].tobytes(), (name, ramp, k)


def test_the_three_identities_and_one_call_of_three_frames_is_three_calls_of_one():
    L = _lib()
    x = A.script()
    for ramp in (0, 3, 7):
        # min = max = 1024 on a fresh state: the input bit for bit, whatever else the parameters say
        unity = agc.Agc(8000, 200, 1024, 1024, 64, 32, ramp, 0)
        st = agc.fresh_state(N)
        for f in range(6):
            out, st = _host(L, unity, st, 1, x[f])
            assert out.tobytes() == x[f].tobytes() and agc.step(x[f], 1, unity, agc.fresh_state(N))[0].tobytes() == x[f].tobytes(), (ramp, f)
            assert (st["gain_q10"] == 1024).all()
        # min = max = G on a state at G: the static gain
        for G in (1, 300, 5000, 32768):
            static = agc.Agc(8000, 200, G, G, 64, 32, ramp, 0)
            st = agc.fresh_state(N)
            st["gain_q10"] = G
            for f in (0, 12, 13):
                want = np.clip((x[f].astype(np.int64) * G + 512) >> 10, -32768, 32767).astype(np.int16)
                out, after = _host(L, static, st, 1, x[f])
                assert out.tobytes() == want.tobytes() and agc.step(x[f], 1, static, st)[0].tobytes() == want.tobytes(), (ramp, G, f)
                assert (after["gain_q10"] == G).all()
        # rise_q8 = 0 never raises a gain
        never = agc.Agc(8000, 200, 512, 8192, 64, 0, ramp, 0)
        st = agc.fresh_state(N)
        for f in range(F):
            _, after = _host(L, never, st, 1, x[f])
            assert (after["gain_q10"] <= st["gain_q10"]).all() and after.tobytes() == agc.step(x[f], 1, never, st)[1].tobytes(), (ramp, f)
            st = after
        assert (st["gain_q10"] < 1024).any()
    # T = 3 in one call against three calls of T = 1 on the regathered rows, through the library alone, with an index onto a larger state
    a = A.params("voice", 5)
    index = np.array([9, 2, 11, 0, 5, 7, 1, 4], dtype=np.int32)
    one = three = agc.fresh_state(12)
    for k in range(4):
        x3 = A.rows(3 * k, 3)
        out3, three = _host(L, a, three, 3, x3, index)
        singles = []
        for t in range(3):
            o, one = _host(L, a, one, 1, x[3 * k + t], index)
            singles.append(o)
        assert out3.tobytes() == np.stack(singles).transpose(1, 0, 2).tobytes() and three.tobytes() == one.tobytes(), k
    untouched = np.setdiff1d(np.arange(12), index)
    assert three[untouched].tobytes() == agc.fresh_state(4).tobytes() and not (three[index] == agc.fresh_state(8)).all()
    # two entries outside the state: their rows come back bit for bit, no record moves
    index[[1, 6]] = (-1, 12)
    out, after = _host(L, a, three, 1, x[20], index)
    want, want_state, ev = agc.step(x[20], 1, a, three, index)
    assert out.tobytes() == want.tobytes() and after.tobytes() == want_state.tobytes() and ev[[1, 6]].tolist() == [agc.PASSED] * 2
    assert out[[1, 6]].tobytes() == x[20][[1, 6]].tobytes() and after[[2, 1]].tobytes() == three[[2, 1]].tobytes()


def test_the_host_call_and_the_launcher_refuse_their_arguments_before_they_ask_for_a_device():
    """never dereferenced: every call below is refused first, on a host with no GPU as well"""
    L = _lib()

    def refused(fn, name, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = L.mbx_last_error()
        assert name + b":" in text, text
        return text

    ok = agc.Agc(8000, 200, 512, 8192, 64, 32, 3, 0)
    g = C.addressof(ok)
    bad_params = [(agc.Agc(0, 200, 512, 8192, 64, 32, 3, 0), b"target_peak"), (agc.Agc(32768, 200, 512, 8192, 64, 32, 3, 0), b"target_peak"),
                  (agc.Agc(8000, 0, 512, 8192, 64, 32, 3, 0), b"floor_peak"), (agc.Agc(8000, 32769, 512, 8192, 64, 32, 3, 0), b"floor_peak"),
                  (agc.Agc(8000, 200, 0, 8192, 64, 32, 3, 0), b"1 .. 32768"), (agc.Agc(8000, 200, 512, 32769, 64, 32, 3, 0), b"1 .. 32768"),
                  (agc.Agc(8000, 200, 8193, 8192, 64, 32, 3, 0), b"min_gain_q10 is above max_gain_q10"),
                  (agc.Agc(8000, 200, 512, 8192, 64, 32, 8, 0), b"MBX_AGC_MAX_RAMP_LOG2"), (agc.Agc(8000, 200, 512, 8192, 64, 32, 3, 1), b"zero")]
    x = np.zeros((4, 160), dtype=np.int16)
    out = np.full((4, 160), 0x5A5A, dtype=np.int16)
    st = agc.fresh_state(2)
    hh = lambda *a: refused(L.mbx_pcm_agc_host, b"mbx_pcm_agc_host", *a)
    good = [g, st.ctypes.data, 2, None, 2, 2, x.ctypes.data, out.ctypes.data]

    def but(at, value):
        args = list(good)
        args[at] = value
        return args

    assert b"agc is needed" in hh(*but(0, None))
    for bad, part in bad_params:
        assert part in hh(*but(0, C.addressof(bad)))
    assert b"state is needed" in hh(*but(1, None)) and b"negative" in hh(*but(2, -1)) and b"negative" in hh(*but(4, -1)) and b"negative" in hh(*but(5, -1))
    assert b"2^31-1" in hh(*(but(4, 65536)[:5] + [32768] + good[6:]))
    assert b"rows in and out" in hh(*but(6, None)) and b"rows in and out" in hh(*but(7, None))
    assert b"overlap" in hh(*but(7, x.ctypes.data + 320)) and b"overlap" in hh(*but(7, x.ctypes.data + 2))
    for record in ((0, 0), (32769, 0), (1024, 32769)):
        wrong = np.array([(1024, 0), record], dtype=agc.RECORD_DTYPE)
        assert b"state record" in hh(*but(1, wrong.ctypes.data))
        assert wrong[1].tolist() == record
    assert (out == 0x5A5A).all() and st.tobytes() == agc.fresh_state(2).tobytes()
    assert L.mbx_pcm_agc_host(*good) == 0 and L.mbx_pcm_agc_host(*but(7, x.ctypes.data)) == 0, L.mbx_last_error()
    assert L.mbx_pcm_agc_host(*but(4, 0)) == 0 and L.mbx_pcm_agc_host(*but(5, 0)) == 0

    # the launcher: a zeroed stand-in for a state (never reached: every call below is refused before the state is looked at, and a
    # call that passes every check asks for a device first)
    fake = (C.c_uint64 * 8)()
    s = C.addressof(fake)
    hd = lambda *a: refused(L.mbx_pcm_agc, b"mbx_pcm_agc", *a)
    assert b"agc is needed" in hd(None, s, None, 4, 1, 0x1000, 0x2000, None)
    for bad, part in bad_params:
        assert part in hd(C.addressof(bad), s, None, 4, 1, 0x1000, 0x2000, None)
    assert b"state is needed" in hd(g, None, None, 4, 1, 0x1000, 0x2000, None)
    assert b"negative" in hd(g, s, None, -1, 1, 0x1000, 0x2000, None) and b"negative" in hd(g, s, None, 4, -1, 0x1000, 0x2000, None)
    assert b"2^31-1" in hd(g, s, None, 65536, 32768, 0x1000, 0x1000, None) and b"2^31-1" in hd(g, s, None, 2 ** 31 - 1, 2, 0x1000, 0x1000, None)
    assert b"rows in and out" in hd(g, s, None, 4, 1, None, 0x2000, None) and b"rows in and out" in hd(g, s, None, 4, 1, 0x1000, None, None)
    for o in (2, 4, 8):
        for args in ((0x1000 + o, 0x2000), (0x1000, 0x2000 + o), (0x1000 + o, 0x1000 + o)):
            text = hd(g, s, None, 4, 1, *args, None)
            assert b"alignment" in text and b"mbx_agc.h" in text, text
    for args in ((0x1000, 0x1010), (0x1000, 0x1000 + 1280 - 16), (0x1140, 0x1000)):
        assert b"overlap" in hd(g, s, None, 4, 1, *args, None)
    # their order: the agc, its fields, the state, the counts, the rows, the pointers, the alignment, the overlap
    worst = [None, None, None, -1, -1, None, None, None]
    for at, value, part in ((None, None, b"agc is needed"), (0, C.addressof(bad_params[7][0]), b"MBX_AGC_MAX_RAMP_LOG2"), (0, g, b"state is needed"),
                            (1, s, b"negative"), (3, 65536, b"negative"), (4, 32768, b"2^31-1"), (4, 1, b"rows in and out"), (5, 0x1008, b"rows in and out"),
                            (6, 0x1010, b"alignment"), (5, 0x1000, b"overlap")):
        if at is not None:
            worst[at] = value
        text = hd(*worst)
        assert text.startswith(b"mbx_pcm_agc: ") and part in text, text
    # nothing to do is not an error, and is decided before a device is asked for
    assert L.mbx_pcm_agc(g, s, None, 0, 1, 0x1000, 0x2000, None) == 0 and L.mbx_pcm_agc(g, s, None, 4, 0, 0x1000, 0x2000, None) == 0
    # the state calls and the session call, by name
    handle = C.c_void_p(0x5A5A)
    refused(L.mbx_agc_state_create, b"mbx_agc_state_create", None, 4)
    assert b"negative" in refused(L.mbx_agc_state_create, b"mbx_agc_state_create", C.byref(handle), -1) and handle.value is None
    assert L.mbx_agc_state_destroy(None) == 0 and L.mbx_agc_state_streams(None) == INVALID
    assert b"state is needed" in refused(L.mbx_agc_state_reset, b"mbx_agc_state_reset", None, 0, 1, None)
    assert b"state is needed" in refused(L.mbx_agc_state_get, b"mbx_agc_state_get", None, 0, 1, st.ctypes.data, None)
    assert b"state is needed" in refused(L.mbx_agc_state_set, b"mbx_agc_state_set", None, 0, 1, st.ctypes.data, None)
    for args in ((None, None, None), (None, g, s), (None, None, s)):
        assert L.mbx_session_next_agc(*args) == INVALID and b"mbx_session_next_agc" in L.mbx_last_error()
