"""CPU suite for limited buses (include/mbx_limit.h): the checks and the arithmetic of mbelib-neo_amd/csrc/mbx_limit_plan.h through the
stand-alone program tests/limit_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as tests/test_agc_host.py
builds its program (an executable of its own; nothing is loaded into this process); the numpy definition (mbelib_neo_amd.limit) on
hand-written known answers; the events the script of tests/limit_cases.py must show, asserted from limit.step alone; mbx_bus_limit_host
held to numpy bit for bit, rows and records, frame by frame and with T = 3 in one call, over that script under both parameter sets and
every ramp_log2; the three identities of the header and |y| <= ceiling on every sample; the three _sums_host calls equal to the int64
numpy sums, and clamp(sums) equal to the PCM16 rows of their parents bit for bit; the refusals of the host call and of the launchers
before a device is asked for; the header held to the library's exports and to the ctypes table of its own (_native.LIMIT_SYMBOLS).
No GPU compute here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import limit_cases as A
from mbelib_neo_amd import hold, levels, limit, mixdown, pcm8
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_limit.h")
INVALID = -1
FUNCTIONS = ["mbx_limit_state_create", "mbx_limit_state_destroy", "mbx_limit_state_buses", "mbx_limit_state_reset", "mbx_limit_state_get", "mbx_limit_state_set",
             "mbx_limit_state_sums", "mbx_bus_limit", "mbx_bus_limit_host", "mbx_mixdown_sums", "mbx_mixdown_sums_host", "mbx_mixdown_gated_sums",
             "mbx_mixdown_gated_sums_host", "mbx_mixdown_held_sums", "mbx_mixdown_held_sums_host", "mbx_session_next_limit"]
N, F = A.BUSES, A.FRAMES


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/limit_check.cpp")
    exe = str(tmp_path_factory.mktemp("limit") / "limit_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "limit_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_refusals_the_bounds_and_the_arithmetic_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"limit_check: ok \(ramp_log2 up to (\d+), range 2\^(\d+), ceilings (\d+) \.\. (\d+)\)", last)
    assert found, run.stdout
    assert tuple(int(v) for v in found.groups()) == (limit.MAX_RAMP_LOG2, limit.RANGE_LOG2, limit.MIN_CEILING, limit.MAX_CEILING)


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


def test_every_function_of_the_limit_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.LIMIT_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS, _native.LEVELS_SYMBOLS, _native.HOLD_SYMBOLS, _native.AGC_SYMBOLS):
        assert not set(_native.LIMIT_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    assert int(re.search(r"#define MBX_LIMIT_UNITY_Q15\s+(\d+)\b", text).group(1)) == limit.UNITY == 32768
    assert int(re.search(r"#define MBX_LIMIT_MIN_CEILING\s+(\d+)\b", text).group(1)) == limit.MIN_CEILING == 1024
    assert int(re.search(r"#define MBX_LIMIT_MAX_CEILING\s+(\d+)\b", text).group(1)) == limit.MAX_CEILING == 32767
    assert int(re.search(r"#define MBX_LIMIT_RANGE_LOG2\s+(\d+)\b", text).group(1)) == limit.RANGE_LOG2 == 22 and limit.RANGE == 1 << 22
    assert re.search(r"#define MBX_LIMIT_MAX_RAMP_LOG2\s+MBX_HOLD_MAX_RAMP_LOG2\b", text) and limit.MAX_RAMP_LOG2 == 7
    assert C.sizeof(limit.Limit) == 8
    assert [getattr(limit.Limit, f).offset for f, _ in limit.Limit._fields_] == [0, 2, 3, 4, 5]
    assert limit.RECORD_DTYPE.itemsize == 4 and [limit.RECORD_DTYPE.fields[f][1] for f in ("gain_q15", "hold_left")] == [0, 2]
    assert limit.fresh_state(3).view(np.uint32).tolist() == [32768] * 3
    # the header states the bounds, the identities, the look-ahead and whose duty the ordering of a state is
    for part in ("|s'[n] * g(n)| <= ceiling << 15 < 2^30", "|y[n]| <= ceiling ALWAYS", "NO FINAL CLAMP", "2^22", "< 2^24", "Three identities follow",
                 "LOOK-AHEAD INSIDE THE FRAME", "which is exactly need < g0", "ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME", "3 is refused"):
        assert part in text, part
    for other in ("mbx.h", "mbx_pcm8.h", "mbx_mixdown.h", "mbx_levels.h", "mbx_hold.h", "mbx_agc.h"):
        theirs = open(os.path.join(ROOT, "include", other)).read()
        assert not any(f in theirs for f in FUNCTIONS) and "mbx_limit_record" not in theirs, other
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
    """one bus under {ceiling 16000, release 128, hold 1, ramp_log2 2}: R = 4, ceiling << 15 = 524,288,000"""
    p = (16000, 128, 1, 2)
    x = np.zeros((1, 160), dtype=np.int32)
    st = limit.fresh_state(1)

    def run(row):
        nonlocal st
        x[0] = row
        out, st, ev = limit.step(x, 1, p, st)
        return out[0].tolist(), st[0].tolist(), int(ev[0])

    # at the ceiling and below: untouched, bit for bit
    assert run(16000) == ([16000] * 160, (32768, 0), limit.IDLE)
    assert run(-16000) == ([-16000] * 160, (32768, 0), limit.IDLE)
    # 32000 in sample 10 over 1000: need = 524288000 // 32000 = 16384; the gain comes down over the four samples in front of it --
    # 32768 - 16384 = 16384, a quarter of it per sample: g(6) = 32768, g(7) = 28672, g(8) = 24576, g(9) = 20480, g(10 ..) = 16384
    row = np.full(160, 1000)
    row[10] = 32000
    out, rec, ev = run(row)
    assert (rec, ev) == ((16384, 1), limit.ATTACK)
    assert out[:7] == [1000] * 7 and out[7:11] == [(1000 * g + 16384) >> 15 for g in (28672, 24576, 20480)] + [16000] == [875, 750, 625, 16000]
    assert out[11:] == [500] * 149
    # quiet: the hold counts 1 -> 0 with the gain held
    assert run(1000) == ([500] * 160, (16384, 0), limit.HELD)
    # then half the distance to unity per frame, over four samples: 16384 -> 24576; g = 18432, 20480, 22528, 24576
    out, rec, ev = run(1000)
    assert (rec, ev) == ((24576, 0), limit.RELEASE_SLEWED) and out[:5] == [(1000 * g + 16384) >> 15 for g in (18432, 20480, 22528, 24576, 24576)] == [563, 625, 688, 750, 750]
    # 20000 everywhere: need = 26214 < 24576 + 4096: the release stops there; 20000 * 26214 = 524,280,000 is just below ceiling << 15
    # and rounds to the ceiling itself
    out, rec, ev = run(20000)
    assert (rec, ev) == ((26214, 0), limit.RELEASE_STOPPED) and out[3:] == [(20000 * 26214 + 16384) >> 15] * 157 == [16000] * 157
    # a spike in sample 0 on a reduced gain: no room for a ramp, the gain steps down in front of the first sample
    row = np.full(160, 1000)
    row[0] = -64000
    out, rec, ev = run(row)
    assert (rec, ev) == ((8192, 1), limit.ATTACK) and out == [-16000] + [250] * 159
    # a spike in sample 2: the ramp the frame start cuts short begins with a step -- g(0) = 8192 + ((24576 - 8192) * 2 >> 2)
    st = np.array([(24576, 0)], dtype=limit.RECORD_DTYPE)
    row[0], row[2] = 1000, 64000
    out, rec, ev = run(row)
    assert (rec, ev) == ((8192, 1), limit.ATTACK) and out[:3] == [(1000 * 16384 + 16384) >> 15, (1000 * 12288 + 16384) >> 15, 16000] == [500, 375, 16000]
    # release up to unity: 32000 -> 32384 -> 32576 -> ... -> 32767 -> 32768 (the term is a ceiling, so the last LSB is reached)
    st = np.array([(32000, 0)], dtype=limit.RECORD_DTYPE)
    gains = []
    for _ in range(12):
        gains.append(run(0)[1][0])
    assert gains[:3] == [32384, 32576, 32672] and gains[-1] == 32768 and 32767 in gains
    assert run(0) == ([0] * 160, (32768, 0), limit.IDLE)
    # beyond the range: clamped to 2^22 first; need = 524288000 // 4194304 = 125
    row = np.zeros(160, dtype=np.int64)
    row[159] = 2 ** 31 - 1
    out, rec, ev = run(row)
    assert (rec, ev) == ((125, 1), limit.ATTACK) and out[159] == (4194304 * 125 + 16384) >> 15 == 16000
    # the byte forms are the G.711 bytes of y
    x[0] = np.arange(-80, 80) * 400
    for form, law in ((mixdown.ULAW, pcm8.LAW_ULAW), (mixdown.ALAW, pcm8.LAW_ALAW)):
        y, after, _ = limit.step(x, 1, p, limit.fresh_state(1))
        b, after_b, _ = limit.step(x, 1, p, limit.fresh_state(1), form=form)
        assert b.dtype == np.uint8 and b.tobytes() == pcm8.compand(y, law).tobytes() and after.tobytes() == after_b.tobytes()
    # what is refused
    for bad in ((1023, 0, 0, 0), (32768, 0, 0, 0), (16000, 256, 0, 0), (16000, 0, 256, 0), (16000, 0, 0, 8), (16000, 0, 0, 0, 1)):
        with pytest.raises(ValueError):
            limit.step(x, 1, bad, limit.fresh_state(1))
    for record in ((0, 0), (32769, 0), (32768, 256)):
        with pytest.raises(ValueError):
            limit.step(x, 1, p, np.array([record], dtype=limit.RECORD_DTYPE))
    with pytest.raises(ValueError):
        limit.step(np.zeros((3, 160), np.int32), 2, p, limit.fresh_state(3))
    with pytest.raises(ValueError):
        limit.step(np.zeros((2, 160), np.int32), 1, p, limit.fresh_state(1))
    with pytest.raises(ValueError):
        limit.step(x, 1, p, limit.fresh_state(1), form=3)
    out, after, ev = limit.step(np.zeros((0, 160), np.int32), 0, p, limit.fresh_state(2))
    assert out.shape == (0, 160) and after.tobytes() == limit.fresh_state(2).tobytes() and ev.size == 0


@pytest.mark.parametrize("ramp", A.RAMPS)
def test_the_script_shows_every_kind_of_event_at_every_ramp(ramp):
    """from numpy alone: each kind at least once under one of the two parameter sets, and what each set is there for under that set.
    (limit.step itself asserts "n* < 160 exactly when need < g0" and |y| <= ceiling on every row it is given.)"""
    got = {name: A.coverage(name, ramp) for name in A.SETS}
    possible = set(A.KINDS) - ({"attack-inside-ramp"} if ramp == 0 else set())   # (R = 1 has no sample with 0 < n* < R)
    missing = possible - got["bridge"] - got["rails"]
    assert not missing, (ramp, sorted(missing))
    assert {"attack-at-0", "attack-beyond-ramp", "attack-at-159", "attack-on-reduced-gain", "hold-to-zero", "release-slewed", "release-stopped", "beyond-range",
            "all-zero-row"} <= got["bridge"], (ramp, sorted(got["bridge"]))
    assert {"attack-at-0", "attack-at-159", "release-reaches-unity", "minus-32768-under-32767", "beyond-range", "all-zero-row"} <= got["rails"], (ramp, sorted(got["rails"]))
    x = A.script()
    assert (x == -32768).any() and (x > limit.RANGE).any() and (x < -limit.RANGE).any() and (x == limit.RANGE).any() and not x[0, 0].any()


def _host(L, p, records, T, x, form=mixdown.PCM16, n=None):
    """mbx_bus_limit_host between guard elements: (out, records after); `records` and `x` are not changed"""
    rows = x.shape[0]
    n = (rows // T if T else 0) if n is None else n
    st = np.full(records.size + 2, 0x5A, dtype=np.uint8).repeat(4).view(limit.RECORD_DTYPE)
    st[1:-1] = records
    dtype = mixdown.out_dtype(form)
    guard = np.array(0x5A5A).astype(dtype)
    out = np.full((rows + 2) * 160, guard, dtype=dtype)
    src = np.ascontiguousarray(x, dtype=np.int32)
    rc = L.mbx_bus_limit_host(C.addressof(p), st[1:].ctypes.data, n, T, src.ctypes.data, form, out[160:].ctypes.data)
    assert rc == 0, L.mbx_last_error()
    assert (out[:160] == guard).all() and (out[-160:] == guard).all() and st[:1].tobytes() == b"\x5a" * 4 and st[-1:].tobytes() == b"\x5a" * 4
    return out[160:-160].reshape(rows, 160).copy(), st[1:-1].copy()


@pytest.mark.parametrize("name,ramp", A.CASES)
def test_the_host_function_is_the_numpy_definition_frame_by_frame_and_three_frames_a_call(name, ramp):
    L = _lib()
    p = A.params(name, ramp)
    ceiling = A.SETS[name]["ceiling"]
    st = limit.fresh_state(N)
    for f, (want_out, want_state, _, before, _) in enumerate(A.expected(name, ramp)):
        out, st = _host(L, p, st, 1, A.script()[f])
        assert out.tobytes() == want_out.tobytes(), (name, ramp, f, "buses", np.flatnonzero((out != want_out).any(axis=1)))
        assert st.tobytes() == want_state.tobytes(), (name, ramp, f, st, want_state)
        assert int(np.abs(out.astype(np.int64)).max()) <= ceiling, (name, ramp, f)
    # T = 3 in one call: the rows regathered bus-major; numpy's own T = 3 is its frame-by-frame run, and so is the library's
    st = st_np = limit.fresh_state(N)
    for k in range(F // 3):
        x3 = A.rows(3 * k, 3)
        form = mixdown.FORMS[k % 3]
        out, st = _host(L, p, st, 3, x3, form)
        out_np, st_np, _ = limit.step(x3, 3, p, st_np, form)
        steps = A.expected(name, ramp)[3 * k:3 * k + 3]
        frame_by_frame = np.stack([s[0] for s in steps]).transpose(1, 0, 2).reshape(N * 3, 160)
        if form != mixdown.PCM16:
            frame_by_frame = pcm8.compand(frame_by_frame, pcm8.LAW_ULAW if form == mixdown.ULAW else pcm8.LAW_ALAW)
        assert out.tobytes() == out_np.tobytes() == frame_by_frame.tobytes(), (name, ramp, k)
        assert st.tobytes() == st_np.tobytes() == steps[-1][1].tobytes(), (name, ramp, k)


def test_the_three_identities_and_the_ceiling_on_every_sample():
    L = _lib()
    x = A.script()
    rng = np.random.default_rng(5)
    inside = rng.integers(-32767, 32768, size=(6, N, 160)).astype(np.int32)
    inside[0, 0, :2], inside[5, N - 1, -2:] = (32767, -32767), (-32767, 32767)
    for ramp in (0, 3, 7):
        # ceiling = 32767 on a fresh state over sums inside -32767 .. 32767: bit for bit, whatever else the parameters say -- and that is
        # the PCM16 row mbx_mixdown writes for those sums
        rails = limit.Limit(32767, 64, 2, ramp)
        st = limit.fresh_state(N)
        for f in range(6):
            out, st = _host(L, rails, st, 1, inside[f])
            assert out.tobytes() == inside[f].astype(np.int16).tobytes() == np.clip(inside[f], -32768, 32767).astype(np.int16).tobytes(), (ramp, f)
            assert limit.step(inside[f], 1, rails, limit.fresh_state(N))[0].tobytes() == out.tobytes()
            assert st.tobytes() == limit.fresh_state(N).tobytes()
        # release_q8 = 0 never raises a gain
        never = limit.Limit(24000, 0, 1, ramp)
        st = limit.fresh_state(N)
        for f in range(F):
            out, after = _host(L, never, st, 1, x[f])
            assert (after["gain_q15"] <= st["gain_q15"]).all() and after.tobytes() == limit.step(x[f], 1, never, st)[1].tobytes(), (ramp, f)
            assert int(np.abs(out.astype(np.int64)).max()) <= 24000
            st = after
        assert (st["gain_q15"] < limit.UNITY).any()
        # |y| <= ceiling at the smallest ceiling, where every speech row attacks
        tight = limit.Limit(1024, 200, 0, ramp)
        st = limit.fresh_state(N)
        for f in range(F):
            out, st = _host(L, tight, st, 1, x[f])
            assert int(np.abs(out.astype(np.int64)).max()) <= 1024, (ramp, f)
    # T = 3 in one call against three calls of T = 1 on the regathered rows, through the library alone, on the first 5 records of a larger state
    p = A.params("bridge", 5)
    one = three = limit.fresh_state(12)
    for k in range(4):
        x3 = A.rows(3 * k, 3)[:15]
        out3, three = _host(L, p, three, 3, x3, n=5)
        singles = []
        for t in range(3):
            o, one = _host(L, p, one, 1, x[3 * k + t][:5], n=5)
            singles.append(o)
        assert out3.tobytes() == np.stack(singles).transpose(1, 0, 2).tobytes() and three.tobytes() == one.tobytes(), k
    assert three[5:].tobytes() == limit.fresh_state(7).tobytes() and not (three[:5] == limit.fresh_state(5)).all()


# ---- the sums ---------------------------------------------------------------------------------------------------------------------------
COUNTS = (0, 1, 2, 5, 0, 30, 3)   # inputs per bus


@pytest.fixture(scope="module")
def buses():
    rng = np.random.default_rng(11)
    rows = 24
    pcm = rng.integers(-32768, 32768, size=(3, rows, 160)).astype(np.int16)
    pcm[:, ::3] //= 40                      # quiet rows, for the gates to close
    pcm[0, 5], pcm[1, 5], pcm[2, 7] = 32767, -32768, 32767
    off = np.concatenate([[0], np.cumsum(COUNTS)]).astype(np.int32)
    row = rng.integers(0, rows, size=int(off[-1])).astype(np.int32)
    row[off[5]:off[5] + 12] = 5             # a bus that is far beyond the rails
    gain = rng.integers(-8192, 8193, size=int(off[-1])).astype(np.int16)
    gain[off[5]:off[5] + 12] = 4096
    return pcm, off, row, gain


def _sums_host(L, fn, pcm, off, row, gain, front=(), behind=()):
    out = np.full((off.size + 1) * 160, 0x5A5A5A5A, dtype=np.int32)
    rc = fn(*front, off.size - 1, off.ctypes.data, row.ctypes.data, None if gain is None else gain.ctypes.data, pcm.ctypes.data, pcm.shape[0], *behind, out[160:].ctypes.data)
    assert rc == 0, L.mbx_last_error()
    assert (out[:160] == 0x5A5A5A5A).all() and (out[-160:] == 0x5A5A5A5A).all()
    return out[160:-160].reshape(off.size - 1, 160).copy()


def _parent_host(L, fn, pcm, off, row, gain, front=(), behind=()):
    out = np.zeros((off.size - 1, 160), dtype=np.int16)
    rc = fn(mixdown.PCM16, *front, off.size - 1, off.ctypes.data, row.ctypes.data, None if gain is None else gain.ctypes.data, pcm.ctypes.data, pcm.shape[0], *behind,
            out.ctypes.data)
    assert rc == 0, L.mbx_last_error()
    return out


def test_the_sums_host_calls_are_the_int64_sums_and_their_clamp_is_the_parents_pcm16(buses):
    L = _lib()
    pcm, off, row, gain = buses
    for f in range(3):
        for g in (gain, None):
            got = _sums_host(L, L.mbx_mixdown_sums_host, pcm[f], off, row, g)
            assert got.tobytes() == limit.sums(pcm[f], off, row, g).tobytes(), f
            assert np.clip(got, -32768, 32767).astype(np.int16).tobytes() == _parent_host(L, L.mbx_mixdown_host, pcm[f], off, row, g).tobytes()
            assert np.clip(got, -32768, 32767).astype(np.int16).tobytes() == mixdown.mix(pcm[f], off, row, g).tobytes()
        assert np.abs(got.astype(np.int64)).max() > 100000, "a bus far beyond the rails"
        for open_peak, loudest_n in ((2000, 2), (0, 0), (2000, 0), (1, 8)):
            gate = levels.Gate(open_peak, loudest_n)
            got = _sums_host(L, L.mbx_mixdown_gated_sums_host, pcm[f], off, row, gain, front=(C.addressof(gate),))
            assert got.tobytes() == limit.sums_gated(pcm[f], off, row, gain, open_peak, loudest_n).tobytes(), (f, open_peak, loudest_n)
            parent = _parent_host(L, L.mbx_mixdown_gated_host, pcm[f], off, row, gain, front=(C.addressof(gate),))
            assert np.clip(got, -32768, 32767).astype(np.int16).tobytes() == parent.tobytes()
    # held, three calls with the state carried: the twin and the parent walk the same states
    for h in (hold.Hold(2000, 1000, 1, 2, 3), hold.Hold(500, 500, 0, 0, 0), hold.Hold(3000, 100, 2, 8, 7)):
        st_np = hold.zero_state(int(off[-1]))
        st_sums, st_parent = st_np.copy(), st_np.copy()
        for f in range(3):
            numpy_parent = hold.step(pcm[f], off, row, gain, mixdown.PCM16, h, st_np)[0]
            want, st_np = limit.sums_held(pcm[f], off, row, gain, h, st_np)
            got = _sums_host(L, L.mbx_mixdown_held_sums_host, pcm[f], off, row, gain, front=(C.addressof(h),), behind=(st_sums.ctypes.data,))
            parent = _parent_host(L, L.mbx_mixdown_held_host, pcm[f], off, row, gain, front=(C.addressof(h),), behind=(st_parent.ctypes.data,))
            assert got.tobytes() == want.tobytes(), f
            assert np.clip(got, -32768, 32767).astype(np.int16).tobytes() == parent.tobytes() == numpy_parent.tobytes(), f
            assert st_sums.tobytes() == st_parent.tobytes() == st_np.tobytes(), f


def test_the_host_calls_and_the_launchers_refuse_their_arguments_before_they_ask_for_a_device(buses):
    """never dereferenced: every call below is refused first, on a host with no GPU as well"""
    L = _lib()

    def refused(fn, name, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = L.mbx_last_error()
        assert name + b":" in text, text
        return text

    ok = limit.Limit(24000, 64, 2, 3)
    g = C.addressof(ok)
    zeroed = limit.Limit(24000, 64, 2, 3)
    zeroed.zero[2] = 1
    bad_params = [(limit.Limit(1023, 64, 2, 3), b"ceiling"), (limit.Limit(32768, 64, 2, 3), b"ceiling"), (limit.Limit(24000, 64, 2, 8), b"MBX_LIMIT_MAX_RAMP_LOG2"),
                  (zeroed, b"zero")]
    x = np.zeros((4, 160), dtype=np.int32)
    out = np.full((4, 160), 0x5A5A, dtype=np.int16)
    st = limit.fresh_state(2)
    hh = lambda *a: refused(L.mbx_bus_limit_host, b"mbx_bus_limit_host", *a)
    good = [g, st.ctypes.data, 2, 2, x.ctypes.data, 0, out.ctypes.data]

    def but(at, value):
        args = list(good)
        args[at] = value
        return args

    assert b"limit is needed" in hh(*but(0, None))
    for bad, part in bad_params:
        assert part in hh(*but(0, C.addressof(bad)))
    assert b"state is needed" in hh(*but(1, None)) and b"negative" in hh(*but(2, -1)) and b"negative" in hh(*but(3, -1))
    assert b"2^31-1" in hh(g, st.ctypes.data, 65536, 32768, x.ctypes.data, 0, out.ctypes.data)
    assert b"form is" in hh(*but(5, 3)) and b"form is" in hh(*but(5, -1))
    assert b"sums in and the rows out" in hh(*but(4, None)) and b"sums in and the rows out" in hh(*but(6, None))
    assert b"overlap" in hh(*but(6, x.ctypes.data)) and b"overlap" in hh(*but(6, x.ctypes.data + 2558))
    for record in ((0, 0), (32769, 0), (32768, 256)):
        wrong = np.array([(32768, 0), record], dtype=limit.RECORD_DTYPE)
        assert b"state record" in hh(*but(1, wrong.ctypes.data))
        assert wrong[1].tolist() == record
    assert (out == 0x5A5A).all() and st.tobytes() == limit.fresh_state(2).tobytes()
    assert L.mbx_bus_limit_host(*good) == 0, L.mbx_last_error()
    assert L.mbx_bus_limit_host(*but(2, 0)) == 0 and L.mbx_bus_limit_host(*but(3, 0)) == 0 and L.mbx_bus_limit_host(g, None, 0, 1, x.ctypes.data, 0, out.ctypes.data) == 0

    # the launcher.  No state can be made without a device, and n is held against the state's size, so every refusal below comes in
    # front of that look, against a stand-in that is never reached
    fake = (C.c_uint64 * 8)()
    s = C.addressof(fake)
    hd = lambda *a: refused(L.mbx_bus_limit, b"mbx_bus_limit", *a)
    assert b"limit is needed" in hd(None, s, 0, 1, 0x1000, 0, 0x8000, None)
    for bad, part in bad_params:
        assert part in hd(C.addressof(bad), s, 0, 1, 0x1000, 0, 0x8000, None)
    assert b"state is needed" in hd(g, None, 0, 1, 0x1000, 0, 0x8000, None)
    assert b"negative" in hd(g, s, -1, 1, 0x1000, 0, 0x8000, None) and b"negative" in hd(g, s, 0, -1, 0x1000, 0, 0x8000, None)
    assert b"2^31-1" in hd(g, s, 65536, 32768, 0x1000, 0, 0x8000, None)
    assert b"form is" in hd(g, s, 0, 1, 0x1000, 3, 0x8000, None)
    assert b"sums in and the rows out" in hd(g, s, 0, 1, None, 0, 0x8000, None) and b"sums in and the rows out" in hd(g, s, 0, 1, 0x1000, 0, None, None)
    for o in (2, 4, 8):
        for form, args in ((0, (0x1000 + o, 0x8000)), (0, (0x1000, 0x8000 + o)), (1, (0x1000 + o, 0x8000)), (2, (0x1000, 0x8000 + (o & 7)))):
            if form == 2 and o == 8:
                continue
            text = hd(g, s, 0, 1, args[0], form, args[1], None)
            assert b"alignment" in text and b"mbx_limit.h" in text, text
    # (the stand-in reads as a state of no buses: n = 4 is above it -- behind the overlap, which needs no state)
    for form, args in ((0, (0x1000, 0x1000)), (0, (0x1000, 0x1000 + 2560 - 16)), (1, (0x1000, 0x1000 - 640 + 8)), (2, (0x1000, 0x1000 + 2552))):
        assert b"overlap" in hd(g, s, 4, 1, args[0], form, args[1], None)
    assert b"above the buses of the state" in hd(g, s, 4, 1, 0x1000, 0, 0x8000, None)
    # nothing to do is not an error, and is decided before a device is asked for
    assert L.mbx_bus_limit(g, s, 0, 1, 0x1000, 0, 0x8000, None) == 0 and L.mbx_bus_limit(g, s, 0, 0, 0x1000, 1, 0x8008, None) == 0
    # the state calls and the session call, by name
    handle = C.c_void_p(0x5A5A)
    refused(L.mbx_limit_state_create, b"mbx_limit_state_create", None, 4)
    assert b"negative" in refused(L.mbx_limit_state_create, b"mbx_limit_state_create", C.byref(handle), -1) and handle.value is None
    assert L.mbx_limit_state_destroy(None) == 0 and L.mbx_limit_state_buses(None) == INVALID and L.mbx_limit_state_sums(None) is None
    assert b"state is needed" in refused(L.mbx_limit_state_reset, b"mbx_limit_state_reset", None, 0, 1, None)
    assert b"state is needed" in refused(L.mbx_limit_state_get, b"mbx_limit_state_get", None, 0, 1, st.ctypes.data, None)
    assert b"state is needed" in refused(L.mbx_limit_state_set, b"mbx_limit_state_set", None, 0, 1, st.ctypes.data, None)
    for args in ((None, None, None), (None, g, s), (None, None, s)):
        assert L.mbx_session_next_limit(*args) == INVALID and b"mbx_session_next_limit" in L.mbx_last_error()

    # the sums launchers refuse what their parents refuse, under their own names; the parents still refuse the form 3
    pcm, off, row, gain = buses
    gate, h = levels.Gate(100, 2), hold.Hold(2000, 1000, 1, 2, 3)
    assert b"d_pcm16 and d_out" in refused(L.mbx_mixdown_sums, b"mbx_mixdown_sums", None, 0x1000, 8, 0x8000, None)
    assert b"d_pcm16 and d_out" in refused(L.mbx_mixdown_sums, b"mbx_mixdown_sums", s, None, 8, 0x8000, None)
    for o in (4, 8):
        assert b"alignment" in refused(L.mbx_mixdown_sums, b"mbx_mixdown_sums", s, 0x1000, 8, 0x8000 + o, None)
    assert b"gate" in refused(L.mbx_mixdown_gated_sums, b"mbx_mixdown_gated_sums", s, None, 0x1000, 8, 0x4000, 0x8000, None)
    assert b"alignment" in refused(L.mbx_mixdown_gated_sums, b"mbx_mixdown_gated_sums", s, C.addressof(gate), 0x1000, 8, 0x4000, 0x8008, None)
    assert refused(L.mbx_mixdown_held_sums, b"mbx_mixdown_held_sums", s, None, s, 0x1000, 8, 0x4000, 0x8000, None)
    assert b"alignment" in refused(L.mbx_mixdown_held_sums, b"mbx_mixdown_held_sums", None, C.addressof(h), s, 0x1000, 8, 0x4000, 0x8008, None)
    assert b"form is" in refused(L.mbx_mixdown, b"mbx_mixdown", s, 3, 0x1000, 8, 0x8000, None)
    assert b"form is" in refused(L.mbx_mixdown_gated, b"mbx_mixdown_gated", s, C.addressof(gate), 3, 0x1000, 8, 0x4000, 0x8000, None)
    assert b"form is" in refused(L.mbx_mixdown_held, b"mbx_mixdown_held", s, C.addressof(h), s, 3, 0x1000, 8, 0x4000, 0x8000, None)
    out16 = np.zeros((off.size - 1, 160), dtype=np.int32)
    args = (off.size - 1, off.ctypes.data, row.ctypes.data, gain.ctypes.data, pcm[0].ctypes.data, pcm.shape[1])
    assert b"form is" in refused(L.mbx_mixdown_host, b"mbx_mixdown_host", 3, *args, out16.ctypes.data)
    assert b"form is" in refused(L.mbx_mixdown_gated_host, b"mbx_mixdown_gated_host", 3, C.addressof(gate), *args, out16.ctypes.data)
    st_h = hold.zero_state(int(off[-1]))
    assert b"form is" in refused(L.mbx_mixdown_held_host, b"mbx_mixdown_held_host", 3, C.addressof(h), *args, st_h.ctypes.data, out16.ctypes.data)
    assert not out16.any() and st_h.tobytes() == hold.zero_state(int(off[-1])).tobytes()
    assert b"pcm16 and out" in refused(L.mbx_mixdown_sums_host, b"mbx_mixdown_sums_host", *args, None)
    assert b"nrows" in refused(L.mbx_mixdown_sums_host, b"mbx_mixdown_sums_host", *args[:5], 1, out16.ctypes.data)
    assert b"gate" in refused(L.mbx_mixdown_gated_sums_host, b"mbx_mixdown_gated_sums_host", None, *args, out16.ctypes.data)
    assert refused(L.mbx_mixdown_held_sums_host, b"mbx_mixdown_held_sums_host", None, *args, st_h.ctypes.data, out16.ctypes.data)
