"""CPU suite for wide rows (include/mbx_resample.h): the checks and the arithmetic of mbelib-neo_amd/csrc/mbx_resample_plan.h through the
stand-alone program tests/resample_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as
tests/test_agc_host.py builds its program (an executable of its own; nothing is loaded into this process); the numpy definition
(mbelib_neo_amd.resample) on hand-written known answers and on the four identities of the header; mbx_pcm_resample_host held to numpy
bit for bit, rows and records, over L in 2, 3, 4, 6 x K in 2, 16, 32 x T in 1, 3, three calls in a row, on the script of
tests/resample_cases.py; an index that is a permutation with one entry outside the records; the filter changed between two calls on
one state; the refusals of the host call and of the launcher before a device is asked for; the designer's figures; the header held to
the library's exports and to the ctypes table of its own (_native.RESAMPLE_SYMBOLS).  No GPU compute here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import resample_cases as A
from mbelib_neo_amd import resample
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_resample.h")
INVALID = -1
FUNCTIONS = ["mbx_resample_state_create", "mbx_resample_state_destroy", "mbx_resample_state_streams", "mbx_resample_state_reset", "mbx_resample_state_get",
             "mbx_resample_state_set", "mbx_pcm_resample", "mbx_pcm_resample_host", "mbx_session_next_resample"]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/resample_check.cpp")
    exe = str(tmp_path_factory.mktemp("resample") / "resample_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "resample_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_refusals_the_bound_the_packing_and_the_identities_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"resample_check: ok \(taps up to (\d+), phase sums up to (\d+)\)", last)
    assert found, run.stdout
    assert (int(found.group(1)), int(found.group(2))) == (resample.MAX_TAPS, resample.PHASE_BOUND)


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


def test_every_function_of_the_resample_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.RESAMPLE_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS, _native.LEVELS_SYMBOLS, _native.HOLD_SYMBOLS, _native.AGC_SYMBOLS, _native.LIMIT_SYMBOLS):
        assert not set(_native.RESAMPLE_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    assert int(re.search(r"#define MBX_RESAMPLE_MAX_TAPS\s+(\d+)\b", text).group(1)) == resample.MAX_TAPS == 192
    assert int(re.search(r"#define MBX_RESAMPLE_UNITY_Q14\s+(\d+)\b", text).group(1)) == resample.UNITY == 16384
    assert int(re.search(r"#define MBX_RESAMPLE_HISTORY\s+(\d+)\b", text).group(1)) == resample.HISTORY == 32
    assert C.sizeof(resample.Resample) == 388
    assert [getattr(resample.Resample, f).offset for f, _ in resample.Resample._fields_] == [0, 1, 2, 4]
    assert resample.RECORD_DTYPE.itemsize == 64 and not resample.fresh_state(3).view(np.uint8).any()
    # the header states the bound, that the clamp is needed, the identities, the zero history and whose duty a doubled entry is
    for part in ("65535 * 32768 =", "2,147,450,880", "A FINAL CLAMP IS NEEDED", "Four identities follow", "HOLD.", "DELAY.", "BATCHING.", "DC.", "ZERO HISTORY",
                 "listed\n * TWICE", "ANY overlap", "NO FRAME OF LATENCY", "ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME", "NO filter designer"):
        assert part in text, part
    for other in ("mbx.h", "mbx_pcm8.h", "mbx_mixdown.h", "mbx_levels.h", "mbx_hold.h", "mbx_agc.h", "mbx_limit.h"):
        theirs = open(os.path.join(ROOT, "include", other)).read()
        assert not any(f in theirs for f in FUNCTIONS) and "mbx_resample_record" not in theirs, other
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name


def test_the_numpy_definition_on_known_answers_and_the_four_identities():
    # L = 2, K = 2, h = [16384, 8192, 0, 8192]: phase 0 is x[n], phase 1 is (x[n] + x[n-1]) / 2 rounded half up (a floor of +0.5)
    h = [16384, 8192, 0, 8192]
    x = np.zeros((1, 160), np.int16)
    x[0, :6] = [100, 201, -300, -301, 32767, -32768]
    st = resample.fresh_state(1)
    st["hist"][0, -1] = 51
    out, after = resample.step((2, 2, h), st, 1, x)
    assert out.shape == (1, 320) and out[0, :12].tolist() == [100, 76, 201, 151, -300, -49, -301, -300, 32767, 16233, -32768, 0]
    assert after["hist"][0].tolist() == [0] * 32 and st["hist"][0, -1] == 51, "the record is the last 32 samples; the caller's array is not changed"
    # overshoot: a phase of gain 2 clips at both rails
    out, _ = resample.step((2, 2, [32767, 16384, 0, 16384]), resample.fresh_state(1), 1, x)
    assert out[0, 8:12].tolist() == [32767, 32466, -32768, -1] and out[0, :2].tolist() == [200, 100]
    rng = np.random.default_rng(7)
    rows = rng.integers(-32768, 32768, size=(6, 160)).astype(np.int16)
    start = resample.fresh_state(2)
    start["hist"] = rng.integers(-32768, 32768, size=(2, 32))
    start["hist"][0, ::2], start["hist"][0, 1::2] = -32768, 32767
    for L in A.FACTORS:
        for K in A.KS:
            # HOLD
            out, after = resample.step((L, K, resample.hold_taps(L, K)), start, 3, rows)
            assert out.tobytes() == np.repeat(rows, L, axis=1).tobytes(), (L, K)
            assert after["hist"].tobytes() == rows[[2, 5], 128:].tobytes()
            # DELAY: x_ext[n - (K-1)], across frames and out of the record
            out3, after3 = resample.step((L, K, resample.delay_taps(L, K)), start, 3, rows)
            ext = np.concatenate([start["hist"], rows.reshape(2, 480)], axis=1)
            assert out3.tobytes() == np.repeat(ext[:, 32 - (K - 1):32 - (K - 1) + 480].reshape(6, 160), L, axis=1).tobytes(), (L, K)
            # BATCHING: three calls of T = 1 on the regathered rows
            st, singles = start, []
            for t in range(3):
                o, st = resample.step((L, K, resample.delay_taps(L, K)), st, 1, rows[t::3])
                singles.append(o)
            assert np.stack(singles, axis=1).reshape(6, 160 * L).tobytes() == out3.tobytes() and st.tobytes() == after3.tobytes(), (L, K)
            # DC
            for c in (-32768, -1, 0, 1, 12345, 32767):
                const = resample.fresh_state(1)
                const["hist"] = c
                out, _ = resample.step((L, K, resample.design(L, K)), const, 1, np.full((1, 160), c, np.int16))
                assert (out == c).all(), (L, K, c)
    # an entry outside the records: a zero history, no record touched; T = 0 and no rows
    d = (2, 4, resample.delay_taps(2, 4))
    out, after = resample.step(d, start, 1, rows[:2], stream_index=[2, 0])
    zero, _ = resample.step(d, resample.fresh_state(1), 1, rows[:1])
    own, own_after = resample.step(d, start[:1], 1, rows[1:2])
    assert out[0].tobytes() == zero.tobytes() and out[1].tobytes() == own.tobytes()
    assert after[1].tobytes() == start[1].tobytes() and after[0].tobytes() == own_after[0].tobytes()
    out, after = resample.step(d, start, 0, np.zeros((0, 160), np.int16))
    assert out.shape == (0, 320) and after.tobytes() == start.tobytes()
    for bad in ((5, 2, [0] * 10), (2, 3, [0] * 6), (2, 34, [0] * 68), (2, 0, []), (2, 2, [1, 0, 0, 0, 1]), (2, 4, [32767, 0, 32767, 0, 1, 0, 1, 0])):
        with pytest.raises(ValueError):
            resample.step(bad, start, 1, rows[:2])
    assert resample.step((2, 4, [32767, 0, 32767, 0, 1, 0, 0, 0]), start, 1, rows[:2])[0].shape == (2, 320), "a phase of 65535 is accepted"
    rs = resample.Resample.of(2, 2, [1, 2, 3, 4])
    rs.zero[1] = 1
    with pytest.raises(ValueError):
        resample.step(rs, start, 1, rows[:2])
    with pytest.raises(ValueError):
        resample.step(d, start, 1, rows[:2], stream_index=[0])
    with pytest.raises(ValueError):
        resample.step(d, start, 4, rows)


# ---- the designer ------------------------------------------------------------------------------------------------------------------------
def _response_db(h, L, freqs_hz):
    """|H| of the prototype at the output rate 8000 L, relative to the interpolator's unity (a DC gain of L), in dB"""
    w = 2 * np.pi * np.asarray(freqs_hz, dtype=np.float64) / (8000.0 * L)
    H = np.exp(-1j * np.outer(w, np.arange(h.size))) @ (h.astype(np.float64) / resample.UNITY)
    return 20 * np.log10(np.maximum(np.abs(H) / L, 1e-12))


@pytest.mark.parametrize("L", A.FACTORS)
def test_the_designer_has_exact_dc_unity_stays_inside_the_bound_and_meets_its_figures(L):
    worst = 0
    for K in range(2, 34, 2):
        h = resample.design(L, K).astype(np.int64)
        assert h.reshape(K, L).sum(axis=0).tolist() == [resample.UNITY] * L, (L, K)
        worst = max(worst, int(np.abs(h).reshape(K, L).sum(axis=0).max()))
        resample._fields((L, K, h))
    assert worst < resample.PHASE_BOUND, worst
    print(f"L {L}: largest phase sum of magnitudes {worst}")
    band = np.arange(0, 3001, 25)
    stop = np.arange(5000, 4000 * L + 1, 25)
    for K, ripple, floor in ((16, 0.6, -65.0), (32, 0.05, -70.0)):
        h = resample.design(L, K)
        pb, sb = _response_db(h, L, band), _response_db(h, L, stop)
        print(f"L {L} K {K}: 0-3 kHz {pb.min():+.3f} .. {pb.max():+.3f} dB, from 5 kHz up at most {sb.max():.1f} dB")
        assert np.abs(pb).max() <= ripple, (L, K, pb.min(), pb.max())
        assert sb.max() < floor, (L, K, sb.max())


def test_a_sine_through_the_designed_filter_is_the_delayed_sine_within_five_lsb():
    """1 kHz at amplitude 20,000 through design(6, 16) over four frames of T = 1; behind the first K * L outputs the wide rows are the ideal
    sine at 48 kHz delayed by (K * L - 1) / 2 outputs"""
    L, K = 6, 16
    h = resample.design(L, K)
    n = np.arange(4 * 160)
    x = np.rint(20000 * np.sin(2 * np.pi * 1000 * n / 8000.0)).astype(np.int16).reshape(4, 160)
    st, got = resample.fresh_state(1), []
    for f in range(4):
        out, st = resample.step((L, K, h), st, 1, x[f:f + 1])
        got.append(out[0])
    y = np.concatenate(got).astype(np.float64)
    m = np.arange(y.size)
    ideal = 20000 * np.sin(2 * np.pi * 1000 * (m - (K * L - 1) / 2.0) / 48000.0)
    err = (y - ideal)[K * L:]
    print(f"max {np.abs(err).max():.2f} LSB, rms {np.sqrt((err ** 2).mean()):.2f} LSB")
    assert np.abs(err).max() <= 5.0, np.abs(err).max()


# ---- the host function ---------------------------------------------------------------------------------------------------------------------
def _host(L, rs, records, T, x, index=None, streams=None):
    """mbx_pcm_resample_host between guard elements: (out, records after); `records` and `x` are not changed"""
    streams = records.size if streams is None else streams
    rows, wide = x.shape[0], 160 * int(rs.L)
    st = np.full((records.size + 2) * 64, 0x5A, dtype=np.uint8).view(resample.RECORD_DTYPE)
    st[1:-1] = records
    out = np.full((rows + 2) * wide, 0x5A5A, dtype=np.int16)
    src = np.ascontiguousarray(x)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    rc = L.mbx_pcm_resample_host(C.addressof(rs), st[1:].ctypes.data, streams, None if idx is None else idx.ctypes.data, rows // T if T else 0, T, src.ctypes.data,
                                 out[wide:].ctypes.data)
    assert rc == 0, L.mbx_last_error()
    assert (out[:wide] == 0x5A5A).all() and (out[-wide:] == 0x5A5A).all() and st[:1].tobytes() == b"\x5a" * 64 and st[-1:].tobytes() == b"\x5a" * 64
    return out[wide:-wide].reshape(rows, wide).copy(), st[1:-1].copy()


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("K", A.KS)
@pytest.mark.parametrize("L", A.FACTORS)
def test_the_host_function_is_the_numpy_definition_rows_and_records_call_after_call(L, K, T):
    lib = _lib()
    for kind in ("design", "rail"):
        rs = A.filt(kind, L, K)
        st = resample.fresh_state(A.NMAX)
        for c, (want, want_state) in enumerate(A.expected(kind, L, K, T)):
            out, st = _host(lib, rs, st, T, A.call_rows(A.NMAX, T, c))
            assert out.tobytes() == want.tobytes(), (kind, L, K, T, c, "rows", np.flatnonzero((out != want).any(axis=1))[:8])
            assert st.tobytes() == want_state.tobytes(), (kind, L, K, T, c)
    want = A.expected("rail", L, K, T)
    assert (want[0][0][T:2 * T] == -32768).all() and (want[1][0][T:2 * T, 2 * L:] == 32767).all(), "the clamp fired at both rails"


def test_an_index_that_is_a_permutation_with_one_entry_outside_the_records():
    lib = _lib()
    rs = A.filt("design", 3, 16)
    index = np.array([6, 2, 9, 0, 11, 5, 12, 1, 4], dtype=np.int32)   # 12 is outside a state of 12 records
    st = st_np = resample.fresh_state(12)
    for c in range(A.CALLS):
        x = A.call_rows(9, 3, c)
        out, st = _host(lib, rs, st, 3, x, index)
        want, st_np = resample.step(rs, st_np, 3, x, index)
        assert out.tobytes() == want.tobytes() and st.tobytes() == st_np.tobytes(), c
        # the entry outside ran over a zero history, whatever the calls before it left
        zero, _ = resample.step(rs, resample.fresh_state(1), 3, x[18:21])
        assert out[18:21].tobytes() == zero.tobytes(), c
    untouched = np.setdiff1d(np.arange(12), index)
    assert not st[untouched].view(np.uint8).any() and st[index[index < 12]].view(np.uint8).reshape(8, 64).any(axis=1).all()
    assert st["hist"][6].tobytes() == x[2, 128:].tobytes() and st["hist"][4].tobytes() == x[26, 128:].tobytes()
    # a negative entry as well, and a state the call is told is shorter than its array
    index[0] = -1
    out, after = _host(lib, rs, st, 3, x, index, streams=11)
    want, want_state = resample.step(rs, st[:11], 3, x, index)
    assert out.tobytes() == want.tobytes() and after[:11].tobytes() == want_state.tobytes() and after[11].tobytes() == st[11].tobytes()


def test_the_filter_may_change_between_two_calls_on_one_state():
    """the record is input samples and does not depend on K: a call at (6, 32) behind one at (2, 2) reads 31 samples of history"""
    lib = _lib()
    st = st_np = resample.fresh_state(5)
    for c, (kind, L, K) in enumerate((("design", 2, 2), ("design", 6, 32), ("delay", 4, 16))):
        rs = A.filt(kind, L, K)
        x = A.call_rows(5, 1, c)
        out, st = _host(lib, rs, st, 1, x)
        want, st_np = resample.step(rs, st_np, 1, x)
        assert out.tobytes() == want.tobytes() and st.tobytes() == st_np.tobytes(), (kind, L, K)
        if c:
            fresh, _ = resample.step(rs, resample.fresh_state(5), 1, x)
            assert (out != fresh).any(axis=1).all(), "every row read its history"
    assert st["hist"].tobytes() == x[:, 128:].tobytes()


def test_the_host_call_and_the_launcher_refuse_their_arguments_before_they_ask_for_a_device():
    """never dereferenced: every call below is refused first, on a host with no GPU as well"""
    lib = _lib()

    def refused(fn, name, *args):
        assert lib.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in lib.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = lib.mbx_last_error()
        assert name + b":" in text, text
        return text

    ok = A.filt("design", 2, 4)
    g = C.addressof(ok)

    def made(L, K, taps, zero=(0, 0)):
        rs = resample.Resample()
        rs.L, rs.K, rs.zero[0], rs.zero[1] = L, K, zero[0], zero[1]
        for i, v in enumerate(taps):
            rs.taps[i] = v
        return rs

    edge = made(2, 4, [32767, 0, -32767, 0, 1, 0, 0, 0])
    bad_filters = [(made(5, 4, [1]), b"L is 2, 3, 4 or 6"), (made(0, 4, [1]), b"L is 2, 3, 4 or 6"), (made(2, 3, [1]), b"K is even, 2 .. 32"),
                   (made(2, 34, [1]), b"K is even, 2 .. 32"), (made(2, 0, [1]), b"K is even, 2 .. 32"), (made(2, 4, [1], (1, 0)), b"zero bytes"),
                   (made(2, 4, [1], (0, 1)), b"zero bytes"), (made(2, 4, [0] * 8 + [1]), b"beyond K * L"), (made(2, 4, [0] * 191 + [-1]), b"beyond K * L"),
                   (made(2, 4, [32767, 0, -32767, 0, 1, 0, -1, 0]), b"more than 65535"), (made(6, 32, [0] * 5 + [-32768] * 1 + [0] * 5 + [-32768]), b"more than 65535")]
    x = np.zeros((4, 160), dtype=np.int16)
    out = np.full((4, 320), 0x5A5A, dtype=np.int16)
    st = resample.fresh_state(2)
    hh = lambda *a: refused(lib.mbx_pcm_resample_host, b"mbx_pcm_resample_host", *a)
    good = [g, st.ctypes.data, 2, None, 2, 2, x.ctypes.data, out.ctypes.data]

    def but(at, value):
        args = list(good)
        args[at] = value
        return args

    assert b"resampler is needed" in hh(*but(0, None))
    for bad, part in bad_filters:
        assert part in hh(*but(0, C.addressof(bad))), part
    assert b"state is needed" in hh(*but(1, None)) and b"negative" in hh(*but(2, -1)) and b"negative" in hh(*but(4, -1)) and b"negative" in hh(*but(5, -1))
    assert b"2^31-1" in hh(*(but(4, 65536)[:5] + [32768] + good[6:])) and b"2^31-1" in hh(*but(4, 6710887)[:5] + [1] + good[6:])
    assert b"rows in and out" in hh(*but(6, None)) and b"rows in and out" in hh(*but(7, None))
    assert b"overlap" in hh(*but(7, x.ctypes.data)) and b"overlap" in hh(*but(7, x.ctypes.data + 1278)) and b"overlap" in hh(*but(6, out.ctypes.data + 2558))
    assert (out == 0x5A5A).all() and not st.view(np.uint8).any()
    assert lib.mbx_pcm_resample_host(*good) == 0 and lib.mbx_pcm_resample_host(*but(0, C.addressof(edge))) == 0, lib.mbx_last_error()
    assert lib.mbx_pcm_resample_host(*but(4, 0)) == 0 and lib.mbx_pcm_resample_host(*but(5, 0)) == 0
    assert lib.mbx_pcm_resample_host(g, None, 0, None, 2, 2, x.ctypes.data, out.ctypes.data) == 0, "no records at all: every entry runs over zeros"

    # the launcher: a zeroed stand-in for a state (never reached: every call below is refused before the state is looked at, and a
    # call that passes every check asks for a device first)
    fake = (C.c_uint64 * 8)()
    s = C.addressof(fake)
    hd = lambda *a: refused(lib.mbx_pcm_resample, b"mbx_pcm_resample", *a)
    assert b"resampler is needed" in hd(None, s, None, 4, 1, 0x1000, 0x2000, None)
    for bad, part in bad_filters:
        assert part in hd(C.addressof(bad), s, None, 4, 1, 0x1000, 0x2000, None)
    assert b"state is needed" in hd(g, None, None, 4, 1, 0x1000, 0x2000, None)
    assert b"negative" in hd(g, s, None, -1, 1, 0x1000, 0x2000, None) and b"negative" in hd(g, s, None, 4, -1, 0x1000, 0x2000, None)
    assert b"2^31-1" in hd(g, s, None, 65536, 32768, 0x1000, 0x1000, None) and b"2^31-1" in hd(g, s, None, 6710887, 1, 0x1000, 0x1000, None)
    assert b"rows in and out" in hd(g, s, None, 4, 1, None, 0x2000, None) and b"rows in and out" in hd(g, s, None, 4, 1, 0x1000, None, None)
    for o in (2, 4, 8):
        for args in ((0x1000 + o, 0x2000), (0x1000, 0x2000 + o), (0x1000 + o, 0x1000 + o)):
            text = hd(g, s, None, 4, 1, *args, None)
            assert b"alignment" in text and b"mbx_resample.h" in text, text
    for args in ((0x1000, 0x1000), (0x1000, 0x1010), (0x1000, 0x1000 + 1280 - 16), (0x1000 + 2560 - 16, 0x1000)):
        assert b"overlap" in hd(g, s, None, 4, 1, *args, None)
    # their order: the filter, its fields, the state, the counts, the size, the pointers, the alignment, the overlap
    worst = [None, None, None, -1, -1, None, None, None]
    for at, value, part in ((None, None, b"resampler is needed"), (0, C.addressof(bad_filters[9][0]), b"more than 65535"), (0, g, b"state is needed"),
                            (1, s, b"negative"), (3, 65536, b"negative"), (4, 32768, b"2^31-1"), (4, 1, b"rows in and out"), (5, 0x1008, b"rows in and out"),
                            (6, 0x1010, b"alignment"), (5, 0x1000, b"overlap")):
        if at is not None:
            worst[at] = value
        text = hd(*worst)
        assert text.startswith(b"mbx_pcm_resample: ") and part in text, text
    # nothing to do is not an error, and is decided before a device is asked for
    assert lib.mbx_pcm_resample(g, s, None, 0, 1, 0x1000, 0x2000, None) == 0 and lib.mbx_pcm_resample(g, s, None, 4, 0, 0x1000, 0x2000, None) == 0
    # the state calls and the session call, by name
    handle = C.c_void_p(0x5A5A)
    refused(lib.mbx_resample_state_create, b"mbx_resample_state_create", None, 4)
    assert b"negative" in refused(lib.mbx_resample_state_create, b"mbx_resample_state_create", C.byref(handle), -1) and handle.value is None
    assert lib.mbx_resample_state_destroy(None) == 0 and lib.mbx_resample_state_streams(None) == INVALID
    assert b"state is needed" in refused(lib.mbx_resample_state_reset, b"mbx_resample_state_reset", None, 0, 1, None)
    assert b"state is needed" in refused(lib.mbx_resample_state_get, b"mbx_resample_state_get", None, 0, 1, st.ctypes.data, None)
    assert b"state is needed" in refused(lib.mbx_resample_state_set, b"mbx_resample_state_set", None, 0, 1, st.ctypes.data, None)
    for args in ((None, None, None, None), (None, g, s, out.ctypes.data), (None, None, s, None)):
        assert lib.mbx_session_next_resample(*args) == INVALID and b"mbx_session_next_resample" in lib.mbx_last_error()
