"""CPU suite for filtered rows (include/mbx_filter.h): the checks and the arithmetic of mbelib-neo_amd/csrc/mbx_filter_plan.h through
the stand-alone program tests/filter_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as
tests/test_agc_host.py builds its program (an executable of its own; nothing is loaded into this process); the numpy definition
(mbelib_neo_amd.filters) on hand-written known answers for the four identities of the header; mbx_pcm_filter_host held to numpy bit for
bit, rows and records after every call, over the script of tests/filter_cases.py -- the designed high-pass, the integrators that reach
both rails, the delays and the sections at the corner of the bound, S in 1, 2, 4 and T in 1, 3, three calls --, under an index that is a
permutation with one entry outside the state and one negative, and three calls of T = 1 against one of T = 3; the designers; the
definition against a float64 recursion; the refusals of the host call and of the launcher before a device is asked for; the header held
to the library's exports and to the ctypes table of its own (_native.FILTER_SYMBOLS).  No GPU compute here.

THE DESIGNER'S BOUND.  The float64 response of the quantised cascade highpass(fc, 2) against the unquantised design at 25, 50, 100, 200,
300, 500, 1000 and 3000 Hz, for fc in 60, 100, 150, 200, 250, 300 Hz, is within 0.070 dB on the CPU (the worst is fc = 60 Hz at 25 Hz,
0.0699 dB); the test holds it to 0.070 + 0.05 dB for the platform's libm.

THE DEFINITION'S DISTANCE from a float64 recursion with the same quantised coefficients, on 440 Hz + 50 Hz + an offset + noise through
highpass(200, 2): 0.864 LSB rms and 3.02 LSB at most on the CPU; the test holds it to twice that, 1.73 rms and 6.04 at most."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import filter_cases as A
from mbelib_neo_amd import filters
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_filter.h")
INVALID = -1
FUNCTIONS = ["mbx_filter_state_create", "mbx_filter_state_destroy", "mbx_filter_state_streams", "mbx_filter_state_reset", "mbx_filter_state_get",
             "mbx_filter_state_set", "mbx_pcm_filter", "mbx_pcm_filter_host", "mbx_session_next_filter"]
N = 9
DESIGN_DB = 0.070 + 0.05     # what the comparison gives on the CPU for the designs below, plus 0.05 dB for the platform's libm
SANITY_RMS, SANITY_MAX = 2 * 0.864, 2 * 3.02   # twice what this file's own script measures on the CPU


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/filter_check.cpp")
    exe = str(tmp_path_factory.mktemp("filter") / "filter_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "filter_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_section_the_refusals_and_the_records_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"filter_check: ok \(sections up to (\d+), sums of magnitudes up to (\d+)\)", last)
    assert found, run.stdout
    assert (int(found.group(1)), int(found.group(2))) == (filters.MAX_SECTIONS, filters.COEFF_BOUND)


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


def test_every_function_of_the_filter_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.FILTER_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS, _native.LEVELS_SYMBOLS, _native.HOLD_SYMBOLS, _native.AGC_SYMBOLS, _native.LIMIT_SYMBOLS, _native.RESAMPLE_SYMBOLS):
        assert not set(_native.FILTER_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    assert int(re.search(r"#define MBX_FILTER_MAX_SECTIONS\s+(\d+)\b", text).group(1)) == filters.MAX_SECTIONS == 4
    assert int(re.search(r"#define MBX_FILTER_UNITY_Q14\s+(\d+)\b", text).group(1)) == filters.UNITY == 16384
    assert int(re.search(r"#define MBX_FILTER_COEFF_BOUND\s+(\d+)\b", text).group(1)) == filters.COEFF_BOUND == 65535
    assert C.sizeof(filters.Filter) == 44 and C.sizeof(filters.Section) == 10
    assert [getattr(filters.Filter, f).offset for f, _ in filters.Filter._fields_] == [0, 1, 4]
    R = filters.RECORD_DTYPE
    assert R.itemsize == 32 and [R.fields[f][1] for f in ("x1", "x2", "sec", "zero")] == [0, 2, 4, 28] and R.fields["sec"][0].base.itemsize == 6
    assert not filters.fresh_state(3).view(np.uint8).any()
    # the header states the bounds, the identities, the zero record, whose duty a doubled entry is and what a session leaves alone
    for part in ("32768 * 65535 < 2^31", "34 bits", "|q| < 2^19", "Four identities follow", "STABILITY IS THE CALLER'S", "LIMIT CYCLES", "RUNS OVER A ZERO RECORD",
                 "listed TWICE", "ONE STATE MAY BE IN FLIGHT ON ONE STREAM AT A TIME", "BY VALUE", "IN FRONT OF an AGC", "pcmf, results and records are untouched"):
        assert part in text, part
    for other in ("mbx.h", "mbx_pcm8.h", "mbx_mixdown.h", "mbx_levels.h", "mbx_hold.h", "mbx_agc.h", "mbx_limit.h", "mbx_resample.h"):
        theirs = open(os.path.join(ROOT, "include", other)).read()
        assert not any(f in theirs for f in FUNCTIONS) and "mbx_filter_record" not in theirs, other
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name


# ---- the numpy definition ------------------------------------------------------------------------------------------------------------------
def _run(coeffs, samples, state=None, T=1):
    """one entry: the samples (a multiple of 160) through filters.step -> (a list of outputs, the state after)"""
    x = np.asarray(samples, dtype=np.int16).reshape(-1, 160)
    st = filters.fresh_state(1) if state is None else state
    outs = []
    for k in range(0, x.shape[0], T):
        out, st = filters.step(coeffs, st, T, x[k:k + T])
        outs.append(out.reshape(-1))
    return np.concatenate(outs).tolist(), st


def test_the_numpy_definition_on_the_four_identities_by_hand():
    rng = np.random.default_rng(7)
    x = rng.integers(-32768, 32768, size=480).astype(np.int16)
    x[:4] = (100, -32768, 32767, 7)
    # {16384, 0, 0 | 0, 0}: the input bit for bit, through one and through four sections
    for S in (1, 4):
        out, st = _run([(16384, 0, 0, 0, 0)] * S, x)
        assert out == x.tolist() and st["x1"][0] == x[-1] and st["x2"][0] == x[-2] and not st["sec"]["e"].any()
        assert st["sec"]["y1"][0, :S].tolist() == [x[-1]] * S and not st["sec"]["y1"][0, S:].any()
    # {0, 16384, 0}: one sample; {0, 0, 16384}: two, 2 S through S sections -- across frames (T = 3) and across calls (T = 1)
    for T in (1, 3):
        out, _ = _run([(0, 16384, 0, 0, 0)], x, T=T)
        assert out == [0] + x[:-1].tolist(), T
        for S in (1, 2, 4):
            out, st = _run([(0, 0, 16384, 0, 0)] * S, x, T=T)
            assert out == [0] * (2 * S) + x[:-2 * S].tolist(), (T, S)
            assert (st["sec"]["y1"][0, S - 1], st["sec"]["y2"][0, S - 1]) == (x[-2 * S - 1], x[-2 * S - 2])
    # {8192, 0, 0} on a constant 1: 0, 1, 0, 1 ... (the fraction is saved); on -1: -1, 0, -1, 0 (the shift floors)
    out, st = _run([(8192, 0, 0, 0, 0)], [1] * 160)
    assert out == [0, 1] * 80 and st["sec"]["e"][0, 0] == 0
    out, st = _run([(8192, 0, 0, 0, 0)], [1] * 159 + [0])
    assert out[:159] == ([0, 1] * 80)[:159] and out[159] == 0 and st["sec"]["e"][0, 0] == 8192
    assert _run([(8192, 0, 0, 0, 0)], [-1] * 160)[0] == [-1, 0] * 80
    # {16384, 0, 0 | -16384, 0}: an integrator that runs into the rail and stays there, then into the other
    out, st = _run([(16384, 0, 0, -16384, 0)], [10000] * 5 + [0, 0, 1] + [0] * 152)
    assert out == [10000, 20000, 30000] + [32767] * 157
    out, st = _run([(16384, 0, 0, -16384, 0)], [-32768, -32768, -1] + [0] * 157, st)
    assert out == [-1] + [-32768] * 159 and st["sec"]["y1"][0, 0] == -32768
    # a launch under S sections leaves the records of sections >= S as they were; an entry outside the state runs over a zero record
    planted = filters.fresh_state(2)
    planted["sec"]["y1"][:], planted["sec"]["y2"][:], planted["sec"]["e"][:] = 77, -78, 16383
    out, after = filters.step([(0, 16384, 0, 0, 0)], planted, 1, np.full((2, 160), 5, np.int16), index=[1, 7])
    assert after[0].tobytes() == planted[0].tobytes() and after["sec"][1, 1:].tobytes() == planted["sec"][1, 1:].tobytes()
    assert (after["x1"][1], after["x2"][1], after["sec"]["y1"][1, 0], after["sec"]["y2"][1, 0], after["sec"]["e"][1, 0]) == (5, 5, 5, 5, 16383)
    assert out[0].tolist() == [0] + [5] * 159 and out[1].tolist() == [0, 5] + [5] * 158   # (e = 16383 in front: 16383 >> 14 = 0, and it stays)
    out, after = filters.step([(16384, 0, 0, 0, 0)], planted, 0, np.zeros((0, 160), np.int16))
    assert out.shape == (0, 160) and after.tobytes() == planted.tobytes()
    # what the library refuses
    x1 = np.zeros((1, 160), np.int16)
    for bad in ([], [(16384, 0, 0, 0, 0)] * 5, [(32767, 32767, 2, 0, 0)], [(0, 0, 0, -32768, 32767 + 1)], [(16384, 0, 0, -32768, -32768)], [(40000, 0, 0, 0, 0)]):
        with pytest.raises(ValueError):
            filters.step(bad, filters.fresh_state(1), 1, x1)
    f = filters.Filter.of([(16384, 0, 0, 0, 0)])
    f.sec[2].a2 = 1
    with pytest.raises(ValueError):
        filters.step(f, filters.fresh_state(1), 1, x1)
    f.sec[2].a2, f.zero[1] = 0, 1
    with pytest.raises(ValueError):
        filters.step(f, filters.fresh_state(1), 1, x1)
    for field, value in (("e", 16384), ("zero", 1)):
        wrong = filters.fresh_state(1)
        (wrong["sec"]["e"] if field == "e" else wrong["zero"])[0, 1] = value
        with pytest.raises(ValueError):
            filters.step([(16384, 0, 0, 0, 0)], wrong, 1, x1)
    with pytest.raises(ValueError):
        filters.step([(16384, 0, 0, 0, 0)], filters.fresh_state(1), 1, x1, index=[0, 0])
    with pytest.raises(ValueError):
        filters.step([(16384, 0, 0, 0, 0)], filters.fresh_state(1), 2, np.zeros((3, 160), np.int16))


def test_the_script_reaches_both_rails_and_the_corner_of_the_bound():
    """from numpy alone: what each kind is there for"""
    for S in A.SECTIONS:
        for T in A.FRAMES:
            rail = A.expected("rail", S, T)
            assert (rail[0][0][(T - 1)::T, -1] == 32767).all() and (rail[1][0][(T - 1)::T, -1] == -32768).all() and (rail[2][0][(T - 1)::T, -1] == 32767).all(), (S, T)
            assert (rail[1][1]["sec"]["y1"][:, :S] == -32768).all()
            corner = A.expected("corner", S, T)
            assert all((c[0] == -32768).any() and (c[0] == 32767).any() for c in corner), (S, T)
    c = A.coeffs("corner", 1)[0]
    assert int(np.abs(c[:3]).sum()) == int(np.abs(c[3:]).sum()) == filters.COEFF_BOUND
    x = A.rows("corner", 1, 0)[1].astype(np.int64)
    assert x[0] == -32768 and x[1] == 32767 and c[0] * x[0] + c[1] * x[1] == -2 * 32767 * 32768   # ff at sample 0 of the call behind it
    assert A.rows("design", 3, 2)[3 * 3:3 * 4].tolist() == [[0] * 160] * 3 and (A.rows("design", 3, 0)[9:12] == 12345).all()


# ---- the host function -----------------------------------------------------------------------------------------------------------------------
def _host(L, f, state, T, x, index=None, in_place=False, streams=None):
    """mbx_pcm_filter_host between guard elements: (out, state after); `state` and `x` are not changed"""
    streams = state.size if streams is None else streams
    rows = x.shape[0]
    st = np.full((state.size + 2) * 32, 0x5A, dtype=np.uint8).view(filters.RECORD_DTYPE)
    st[1:-1] = state
    out = np.full((rows + 2) * 160, 0x5A5A, dtype=np.int16)
    src = np.ascontiguousarray(x)
    if in_place:
        out[160:-160] = src.reshape(-1)
    idx = None if index is None else np.ascontiguousarray(index, dtype=np.int32)
    rc = L.mbx_pcm_filter_host(C.addressof(f), st[1:].ctypes.data, streams, None if idx is None else idx.ctypes.data, rows // T if T else 0, T,
                               out[160:].ctypes.data if in_place else src.ctypes.data, out[160:].ctypes.data)
    assert rc == 0, L.mbx_last_error()
    assert (out[:160] == 0x5A5A).all() and (out[-160:] == 0x5A5A).all() and st[:1].tobytes() == b"\x5a" * 32 and st[-1:].tobytes() == b"\x5a" * 32
    return out[160:-160].reshape(rows, 160).copy(), st[1:-1].copy()


@pytest.mark.parametrize("S", A.SECTIONS)
@pytest.mark.parametrize("kind", A.KINDS)
def test_the_host_function_is_the_numpy_definition_rows_and_records_after_every_call(kind, S):
    L = _lib()
    f = A.filt(kind, S)
    for T in A.FRAMES:
        st = filters.fresh_state(N)
        for c, (want, want_state) in enumerate(A.expected(kind, S, T)):
            out, st = _host(L, f, st, T, A.call_rows(kind, N, T, c), in_place=bool(c & 1))
            assert out.tobytes() == want[:N * T].tobytes(), (kind, S, T, c, "entries", np.flatnonzero((out != want[:N * T]).any(axis=1)) // T)
            assert st.tobytes() == want_state[:N].tobytes(), (kind, S, T, c)
    # an index that is a permutation onto a larger state, one entry outside it, one negative; the state read back after every call
    index = np.array([9, 2, 11, 12, 5, 7, -1, 4, 0], dtype=np.int32)   # 12 is outside a state of 12 records
    planted = filters.fresh_state(12)
    planted["sec"]["y1"][:], planted["sec"]["e"][:] = 321, 9999
    st = st_np = planted
    for c in range(A.CALLS):
        x = A.call_rows(kind, N, 3, c)
        out, st = _host(L, f, st, 3, x, index)
        want, st_np = filters.step(f, st_np, 3, x, index)
        assert out.tobytes() == want.tobytes() and st.tobytes() == st_np.tobytes(), (kind, S, c)
        zero, _ = filters.step(f, filters.fresh_state(1), 3, x[9:12])
        assert out[9:12].tobytes() == zero.tobytes() and out[18:21].tobytes() == filters.step(f, filters.fresh_state(1), 3, x[18:21])[0].tobytes()
    untouched = np.setdiff1d(np.arange(12), index)
    assert st[untouched].tobytes() == planted[untouched].tobytes() and st["sec"][:, S:].tobytes() == planted["sec"][:, S:].tobytes()
    # three calls of T = 1 against one of T = 3, through the library alone
    one = three = filters.fresh_state(N)
    for c in range(2):
        x3 = A.call_rows(kind, N, 3, c)
        out3, three = _host(L, f, three, 3, x3)
        singles = []
        for t in range(3):
            o, one = _host(L, f, one, 1, x3[t::3], in_place=bool(t & 1))
            singles.append(o)
        assert out3.tobytes() == np.stack(singles, axis=1).reshape(N * 3, 160).tobytes() and three.tobytes() == one.tobytes(), (kind, S, c)


# ---- the designers ---------------------------------------------------------------------------------------------------------------------------
HP_CUTS = (60, 100, 150, 200, 250, 300, 400)


@pytest.mark.parametrize("S", [1, 2])
def test_every_highpass_sums_to_zero_and_settles_at_exactly_zero(S):
    """a constant 12345, then -32768, then 0, ten frames each: the output ends at exactly 0 each time"""
    for fc in HP_CUTS:
        f = filters.highpass(fc, S)
        c = f.coeffs()
        assert (c[:S, :3].sum(axis=1) == 0).all() and not c[S:].any() and f.sections == S, fc
        st = filters.fresh_state(1)
        for value in (12345, -32768, 0):
            out, st = filters.step(f, st, 10, np.full((10, 160), value, np.int16))
            assert not out[-1].any(), (fc, S, value, out[-1, -4:])
    # without the zero-sum fix a 200 Hz section idles away from zero
    plain = filters.quantise(filters.highpass_prototype(200, 1))
    assert plain.coeffs()[0, :3].sum() != 0
    out, _ = filters.step(plain, filters.fresh_state(1), 10, np.full((10, 160), -32768, np.int16))
    assert abs(int(out[-1, -1])) > 30


def test_the_quantised_designs_keep_their_response_and_the_plain_designers_their_bounds():
    freqs = np.array([25, 50, 100, 200, 300, 500, 1000, 3000], dtype=np.float64)
    worst = 0.0
    for fc in (60, 100, 150, 200, 250, 300):
        dev = np.abs(filters.response_db(filters.highpass(fc, 2), freqs) - filters.response_db(filters.highpass_prototype(fc, 2), freqs))
        print(f"highpass({fc}, 2): {dev.max():.4f} dB at {freqs[int(dev.argmax())]:.0f} Hz")
        worst = max(worst, float(dev.max()))
    assert worst <= DESIGN_DB, worst
    # a 4th-order Butterworth: -3.01 dB at the corner, 24 dB an octave below it
    hp = filters.highpass(200, 2)
    at = filters.response_db(hp, [200.0, 100.0, 2000.0])
    assert abs(at[0] + 3.01) < 0.1 and -25.5 < at[1] < -23.0 and abs(at[2]) < 0.05
    lp = filters.lowpass(3400, 2)
    at = filters.response_db(lp, [3400.0, 300.0])
    assert abs(at[0] + 3.01) < 0.1 and abs(at[1]) < 0.05 and lp.sections == 2
    nt = filters.notch(1000, 8)
    assert filters.response_db(nt, [1000.0])[0] < -40 and abs(filters.response_db(nt, [300.0])[0]) < 0.2 and nt.sections == 1
    pk = filters.peaking(1000, 2, 6)
    at = filters.response_db(pk, [1000.0, 60.0, 3900.0])
    assert abs(at[0] - 6.0) < 0.05 and abs(at[1]) < 0.1 and abs(at[2]) < 0.1
    # refused where a coefficient leaves int16 or a section leaves the bound
    for make in (lambda: filters.highpass(0.01, 1), lambda: filters.peaking(1000, 0.3, 18), lambda: filters.highpass(200, 5), lambda: filters.lowpass(4000, 1),
                 lambda: filters.notch(1000, 0)):
        with pytest.raises(ValueError):
            make()


def test_the_definition_stays_within_a_few_lsb_of_a_float_recursion():
    """sanity of the definition, not the parity criterion: 440 Hz + 50 Hz + an offset + noise through highpass(200, 2), against a
    float64 recursion with the same quantised coefficients"""
    rng = np.random.default_rng(5)
    n = np.arange(1600)
    x = (6000 * np.sin(2 * np.pi * 440 * n / 8000) + 8000 * np.sin(2 * np.pi * 50 * n / 8000) + 3000 + rng.normal(0, 300, n.size)).round().astype(np.int16)
    f = filters.highpass(200, 2)
    out, _ = filters.step(f, filters.fresh_state(1), 10, x.reshape(10, 160))
    y = x.astype(np.float64)
    for b0, b1, b2, a1, a2 in (f.coeffs()[:2] / 16384.0).tolist():
        z, x1, x2, y1, y2 = np.zeros_like(y), 0.0, 0.0, 0.0, 0.0
        for k in range(y.size):
            v = b0 * y[k] + b1 * x1 + b2 * x2 - a1 * y1 - a2 * y2
            x2, x1, y2, y1, z[k] = x1, y[k], y1, v, v
        y = z
    d = out.reshape(-1) - y
    rms, top = float(np.sqrt((d * d).mean())), float(np.abs(d).max())
    print(f"rms {rms:.3f} LSB, max {top:.2f} LSB")
    assert rms <= SANITY_RMS and top <= SANITY_MAX, (rms, top)
    assert float(np.abs(out.reshape(-1)[800:]).max()) > 5000 and abs(float(out.reshape(-1)[800:].mean())) < 40, "the tone passed, the offset did not"


# ---- refusals that need no device ------------------------------------------------------------------------------------------------------------
def test_the_host_call_and_the_launcher_refuse_their_arguments_before_they_ask_for_a_device():
    """never dereferenced: every call below is refused first, on a host with no GPU as well"""
    L = _lib()

    def refused(fn, name, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = L.mbx_last_error()
        assert name + b":" in text, text
        return text

    ok = filters.highpass(200, 2)
    g = C.addressof(ok)

    def broken(change):
        f = filters.highpass(200, 2)
        change(f)
        return f

    def set_sections(v):
        return lambda f: setattr(f, "sections", v)

    def over_b(f):
        f.sec[1].b0, f.sec[1].b1, f.sec[1].b2 = 32767, -32768, 1

    def over_a(f):
        f.sec[0].a1, f.sec[0].a2 = -32768, -32768

    def beyond(f):
        f.sec[3].b1 = -1

    def zero(f):
        f.zero[2] = 1

    bad_filters = [(broken(set_sections(0)), b"sections is 1 .. MBX_FILTER_MAX_SECTIONS"), (broken(set_sections(5)), b"sections is 1 .. MBX_FILTER_MAX_SECTIONS"),
                   (broken(zero), b"zero bytes"), (broken(over_b), b"above 65535"), (broken(over_a), b"above 65535"), (broken(beyond), b"beyond sections")]
    x = np.zeros((4, 160), dtype=np.int16)
    out = np.full((4, 160), 0x5A5A, dtype=np.int16)
    st = filters.fresh_state(2)
    hh = lambda *a: refused(L.mbx_pcm_filter_host, b"mbx_pcm_filter_host", *a)
    good = [g, st.ctypes.data, 2, None, 2, 2, x.ctypes.data, out.ctypes.data]

    def but(at, value):
        args = list(good)
        args[at] = value
        return args

    assert b"filter is needed" in hh(*but(0, None))
    for bad, part in bad_filters:
        assert part in hh(*but(0, C.addressof(bad)))
    assert b"state is needed" in hh(*but(1, None)) and b"negative" in hh(*but(2, -1)) and b"negative" in hh(*but(4, -1)) and b"negative" in hh(*but(5, -1))
    assert b"2^31-1" in hh(*(but(4, 65536)[:5] + [32768] + good[6:]))
    assert b"rows in and out" in hh(*but(6, None)) and b"rows in and out" in hh(*but(7, None))
    assert b"overlap" in hh(*but(7, x.ctypes.data + 320)) and b"overlap" in hh(*but(7, x.ctypes.data + 2))
    for field, value in (("e", 16384), ("e", 65535), ("zero", 1)):
        wrong = filters.fresh_state(2)
        (wrong["sec"]["e"] if field == "e" else wrong["zero"])[1, 1] = value
        before = wrong.tobytes()
        assert b"state record" in hh(*but(1, wrong.ctypes.data)) and wrong.tobytes() == before
    assert (out == 0x5A5A).all() and not st.view(np.uint8).any()
    assert L.mbx_pcm_filter_host(*good) == 0 and L.mbx_pcm_filter_host(*but(7, x.ctypes.data)) == 0, L.mbx_last_error()
    assert L.mbx_pcm_filter_host(*but(4, 0)) == 0 and L.mbx_pcm_filter_host(*but(5, 0)) == 0

    # the launcher: a zeroed stand-in for a state (never reached: every call below is refused before the state is looked at, and a
    # call that passes every check asks for a device first)
    fake = (C.c_uint64 * 8)()
    s = C.addressof(fake)
    hd = lambda *a: refused(L.mbx_pcm_filter, b"mbx_pcm_filter", *a)
    assert b"filter is needed" in hd(None, s, None, 4, 1, 0x1000, 0x2000, None)
    for bad, part in bad_filters:
        assert part in hd(C.addressof(bad), s, None, 4, 1, 0x1000, 0x2000, None)
    assert b"state is needed" in hd(g, None, None, 4, 1, 0x1000, 0x2000, None)
    assert b"negative" in hd(g, s, None, -1, 1, 0x1000, 0x2000, None) and b"negative" in hd(g, s, None, 4, -1, 0x1000, 0x2000, None)
    assert b"2^31-1" in hd(g, s, None, 65536, 32768, 0x1000, 0x1000, None) and b"2^31-1" in hd(g, s, None, 2 ** 31 - 1, 2, 0x1000, 0x1000, None)
    assert b"rows in and out" in hd(g, s, None, 4, 1, None, 0x2000, None) and b"rows in and out" in hd(g, s, None, 4, 1, 0x1000, None, None)
    for o in (2, 4, 8):
        for args in ((0x1000 + o, 0x2000), (0x1000, 0x2000 + o), (0x1000 + o, 0x1000 + o)):
            text = hd(g, s, None, 4, 1, *args, None)
            assert b"alignment" in text and b"mbx_filter.h" in text, text
    for args in ((0x1000, 0x1010), (0x1000, 0x1000 + 1280 - 16), (0x1140, 0x1000)):
        assert b"overlap" in hd(g, s, None, 4, 1, *args, None)
    # their order: the filter, its fields, the state, the counts, the rows, the pointers, the alignment, the overlap
    worst = [None, None, None, -1, -1, None, None, None]
    for at, value, part in ((None, None, b"filter is needed"), (0, C.addressof(bad_filters[3][0]), b"above 65535"), (0, g, b"state is needed"),
                            (1, s, b"negative"), (3, 65536, b"negative"), (4, 32768, b"2^31-1"), (4, 1, b"rows in and out"), (5, 0x1008, b"rows in and out"),
                            (6, 0x1010, b"alignment"), (5, 0x1000, b"overlap")):
        if at is not None:
            worst[at] = value
        text = hd(*worst)
        assert text.startswith(b"mbx_pcm_filter: ") and part in text, text
    # nothing to do is not an error, and is decided before a device is asked for
    assert L.mbx_pcm_filter(g, s, None, 0, 1, 0x1000, 0x2000, None) == 0 and L.mbx_pcm_filter(g, s, None, 4, 0, 0x1000, 0x2000, None) == 0
    # the state calls and the session call, by name
    handle = C.c_void_p(0x5A5A)
    refused(L.mbx_filter_state_create, b"mbx_filter_state_create", None, 4)
    assert b"negative" in refused(L.mbx_filter_state_create, b"mbx_filter_state_create", C.byref(handle), -1) and handle.value is None
    assert L.mbx_filter_state_destroy(None) == 0 and L.mbx_filter_state_streams(None) == INVALID
    assert b"state is needed" in refused(L.mbx_filter_state_reset, b"mbx_filter_state_reset", None, 0, 1, None)
    assert b"state is needed" in refused(L.mbx_filter_state_get, b"mbx_filter_state_get", None, 0, 1, st.ctypes.data, None)
    assert b"state is needed" in refused(L.mbx_filter_state_set, b"mbx_filter_state_set", None, 0, 1, st.ctypes.data, None)
    for args in ((None, None, None), (None, g, s), (None, None, s)):
        assert L.mbx_session_next_filter(*args) == INVALID and b"mbx_session_next_filter" in L.mbx_last_error()
