"""CPU suite for band records (include/mbx_bands.h): the arithmetic, the bound and the refusals of mbelib-neo_amd/csrc/mbx_bands_plan.h
through the stand-alone program tests/bands_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as
tests/test_levels_host.py builds its program (an executable of its own; nothing is loaded into this process); the numpy definition
(mbelib_neo_amd.bands) on known answers and the identities of the header; the designers held to the bound; the synthetic DTMF rows
decided by the power records of bands.dtmf(); mbx_pcm_bands_host held to numpy byte for byte in both forms; the refusals of the
launcher, of the bank and of the session call before a device is asked for; the header held to the library's exports and to the ctypes
table of its own (_native.BANDS_SYMBOLS).  No GPU compute here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import bands_cases
from mbelib_neo_amd import bands
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_bands.h")
INVALID = -1
FUNCTIONS = ["mbx_band_bank_create", "mbx_band_bank_destroy", "mbx_band_bank_probes", "mbx_pcm_bands", "mbx_pcm_bands_host", "mbx_session_next_bands"]
AT_BOUND = 32768 * 65535   # 2,147,450,880


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/bands_check.cpp")
    exe = str(tmp_path_factory.mktemp("bands") / "bands_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "bands_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_arithmetic_the_bound_and_the_refusals_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"bands_check: ok \(16 lanes per row, up to (\d+) probes, bound (\d+)\)", last)
    assert found, run.stdout
    assert (int(found.group(1)), int(found.group(2))) == (bands.MAX_PROBES, bands.VECTOR_BOUND)


def test_the_numpy_definition_on_known_answers_and_the_identities_of_the_header():
    rng = np.random.default_rng(3)
    x = bands_cases.rows(rng, 12)
    # the bound reached: a vector of 32767 + 32767 + 1 against the row of -32768, either sign, and both at once in the power form
    p = np.zeros((2, 2, 160), dtype=np.int16)
    p[0, 0, [0, 77, 159]] = [32767, 32767, 1]
    p[0, 1, [3, 4, 158]] = [-32767, -32767, -1]
    p[1, 0, [9, 10, 11]] = [32767, -32767, 1]
    got = bands.measure(x, p, bands.COMPLEX)
    assert got.dtype == bands.RECORD_DTYPE and got.dtype.itemsize == 8 and got.shape == (12, 2)
    assert [got.dtype.fields[f][1] for f in ("re", "im")] == [0, 4]
    assert (got["re"][1, 0], got["im"][1, 0]) == (-AT_BOUND, AT_BOUND), "the row of -32768"
    assert (got["re"][0, 0], got["im"][0, 0]) == (32767 * 65535, -32767 * 65535), "the row of 32767"
    power = bands.measure(x, p, bands.POWER)
    assert power.dtype == np.dtype("<u4") and power.shape == (12, 2)
    assert power[1, 0] == 4294836225 == (2 * AT_BOUND ** 2) >> 31
    assert power[1, 1] == ((-32768) ** 2) >> 31 == 0 and got["re"][1, 1] == -32768
    assert (power == ((got["re"].astype(object) ** 2 + got["im"].astype(object) ** 2) >> 31)).all()
    assert bands.measure(np.zeros((0, 160), np.int16), p, bands.POWER).shape == (0, 2)
    # IMPULSE: c = 16384 delta[n - m], s = 0 gives re = 16384 x[m], im = 0
    for m in (0, 1, 77, 159):
        imp = np.zeros((1, 2, 160), dtype=np.int16)
        imp[0, 0, m] = 16384
        r = bands.measure(x, imp)
        assert (r["re"][:, 0] == 16384 * x[:, m].astype(np.int64)).all() and not r["im"].any(), m
    # ZERO: a probe of zeros gives zeros in both forms
    zero = np.zeros((3, 2, 160), dtype=np.int16)
    zero[1] = bands.tone(1000)
    for form in bands.FORMS:
        r = bands.measure(x, zero, form)
        raw = [np.ascontiguousarray(r[:, k]).view(np.uint8) for k in range(3)]
        assert not raw[0].any() and not raw[2].any() and raw[1].any(), form
    # LINEAR: the COMPLEX records are additive over two rows whose sum does not clip
    a = rng.integers(-16000, 16001, size=(9, 160)).astype(np.int16)
    b = rng.integers(-16000, 16001, size=(9, 160)).astype(np.int16)
    bank = bands_cases.bank(rng, 6)
    ra, rb, rs = (bands.measure(v, bank) for v in (a, b, (a + b).astype(np.int16)))
    assert (rs["re"] == ra["re"] + rb["re"]).all() and (rs["im"] == ra["im"] + rb["im"]).all() and ra["re"].any()
    # LEVELS: a probe pair cannot give the energy -- two rows of equal energy and different records
    e1, e2 = np.zeros((1, 160), np.int16), np.zeros((1, 160), np.int16)
    e1[0, 3], e2[0, 4] = 1000, 1000
    one = bands.tone(1000)[None]
    assert (e1.astype(np.int64) ** 2).sum() == (e2.astype(np.int64) ** 2).sum() and bands.measure(e1, one).tobytes() != bands.measure(e2, one).tobytes()
    # what check() refuses, in the library's words
    over = p.copy()
    over[1, 1, [5, 6, 7]] = [32767, 32767, 2]
    with pytest.raises(ValueError, match=re.escape("probe 1: the |s[n]| sum to 65536, above MBX_BANDS_VECTOR_BOUND (65535)")):
        bands.check(over)
    over[0, 0, 1] = 1
    with pytest.raises(ValueError, match=re.escape("probe 0: the |c[n]| sum to 65536")):
        bands.measure(x, over)
    for K in (0, 33):
        with pytest.raises(ValueError, match="K is 1 .. MBX_BANDS_MAX_PROBES"):
            bands.check(np.zeros((K, 2, 160), np.int16))
    with pytest.raises(ValueError, match="form"):
        bands.measure(x, p, 2)
    with pytest.raises(TypeError):
        bands.measure(x.astype(np.int32), p)
    with pytest.raises(TypeError):
        bands.check(p.astype(np.int32))
    with pytest.raises(ValueError):
        bands.check(np.zeros((2, 160), np.int16)[:, :159])


@pytest.mark.parametrize("window", ["rect", "hann"])
def test_the_designers_meet_the_bound_by_construction(window):
    worst = 0
    for f in list(bands.DTMF_HZ) + [0, 1, 50, 60, 440, 1000, 1004, 2000, 2175, 3999, 4000, 1234.5]:
        probe = bands.tone(f, window)
        assert probe.dtype == np.int16 and probe.shape == (2, 160)
        sums = np.abs(probe.astype(np.int64)).sum(axis=1)
        assert sums.max() <= bands.VECTOR_BOUND, (f, sums)
        assert sums.max() >= bands.VECTOR_BOUND - 160, "truncation loses less than one unit per tap"
        worst = max(worst, int(sums.max()))
        bands.check(probe)
        # one factor for both vectors: c^2 + s^2 follows the window, so with a rectangular one it is flat to the truncation
        if window == "rect" and f not in (0, 4000):
            mag = np.hypot(probe[0].astype(float), probe[1].astype(float))
            assert mag.max() - mag.min() < 1.5, f
    assert worst <= bands.VECTOR_BOUND
    d = bands.dtmf(window)
    assert d.shape == (8, 2, 160) and d.tobytes() == np.stack([bands.tone(f, window) for f in (697, 770, 852, 941, 1209, 1336, 1477, 1633)]).tobytes()
    assert bands.check(d) is not None
    assert bands.tone(0, window)[1].any() == False and bands.tone(0, window)[0].min() >= 0   # noqa: E712
    with pytest.raises(ValueError):
        bands.tone(1000, "hamming")


@pytest.mark.parametrize("window", ["rect", "hann"])
def test_the_power_records_of_dtmf_decide_every_one_of_2400_synthetic_rows(window):
    """16 digits, two tones at -10, -20 and -30 dBFS each with random phases, white noise at -50 dBFS rms, default_rng(7), 50 rows per
    case: the largest row probe and the largest column probe name the digit.  All 2,400 right, none left out."""
    x, keys = bands_cases.dtmf_rows()
    assert x.shape == (2400, 160) and len(keys) == 2400 and sorted(set(keys)) == sorted(bands.DTMF_KEYS)
    power = bands.measure(x, bands.dtmf(window), bands.POWER)
    got = bands.dtmf_key(power)
    assert len(got) == 2400
    wrong = [i for i in range(2400) if got[i] != keys[i]]
    assert not wrong, (len(wrong), wrong[:10])


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


def test_every_function_of_the_bands_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.BANDS_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS, _native.LEVELS_SYMBOLS, _native.HOLD_SYMBOLS, _native.AGC_SYMBOLS, _native.LIMIT_SYMBOLS, _native.RESAMPLE_SYMBOLS,
                  _native.FILTER_SYMBOLS):
        assert not set(_native.BANDS_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    for name, value in (("MBX_BANDS_MAX_PROBES", bands.MAX_PROBES), ("MBX_BANDS_VECTOR_BOUND", bands.VECTOR_BOUND), ("MBX_BANDS_COMPLEX", bands.COMPLEX),
                        ("MBX_BANDS_POWER", bands.POWER)):
        assert int(re.search(rf"#define {name}\s+(\d+)u?\b", text).group(1)) == value, name
    assert (bands.MAX_PROBES, bands.VECTOR_BOUND, bands.COMPLEX, bands.POWER) == (32, 65535, 0, 1)
    # no new outputs bit: the header defines no MBX_SESSION_* flag
    assert not re.search(r"#define\s+MBX_SESSION_", text)
    # the alignment rows of the new kinds, the identities and the statelessness are stated
    assert "Alignment, in the style of the table in mbx_mixdown.h" in text
    for kind, align in (("band rows", 16), ("band records", 16)):
        assert re.search(rf"^ \*   {kind}\s+{align}\b", text, flags=re.M), kind
    for word in ("IMPULSE", "LEVELS", "ZERO", "LINEAR", "stateless", "40 ms"):
        assert word in text, word
    # the other headers do not know the new calls: a header of its own
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "mbx_bands.h":
            theirs = open(os.path.join(ROOT, "include", other)).read()
            assert not any(f in theirs for f in FUNCTIONS) and "mbx_band_bank" not in theirs, other
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name


@pytest.mark.parametrize("K", [1, 2, 8, 17, 32])
def test_the_host_function_is_the_numpy_definition_byte_for_byte_in_both_forms(K):
    L = _lib()
    nrows = 37
    x, p, want = bands_cases.case(nrows, K)
    for form in bands.FORMS:
        per = K * bands.record_bytes(form)
        got = np.full((nrows + 2) * per, 0x5A, dtype=np.uint8)
        assert L.mbx_pcm_bands_host(p.ctypes.data, K, form, x.ctypes.data, nrows, got[per:].ctypes.data) == 0, L.mbx_last_error()
        assert got[per:-per].tobytes() == want[form].tobytes(), (K, form)
        assert (got[:per] == 0x5A).all() and (got[-per:] == 0x5A).all(), "nothing in front of the records or behind them"
        assert L.mbx_pcm_bands_host(p.ctypes.data, K, form, x.ctypes.data, 0, got.ctypes.data) == 0 and (got[:per] == 0x5A).all()
    assert abs(int(want[bands.COMPLEX]["re"][1, 0])) == AT_BOUND, "the sign-aligned probe reaches the bound on the row of -32768"


def test_the_host_function_refuses_by_name_and_in_order():
    L = _lib()
    x, p, _ = bands_cases.case(37, 2)
    out = np.zeros(37 * 2 * 8, dtype=np.uint8)
    over = np.array(p)
    over[1, 1] = 0
    over[1, 1, [5, 6, 7]] = [32767, 32767, 2]

    def refused(part, *args):
        L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
        assert L.mbx_pcm_bands_host(*args) == INVALID, args
        text = L.mbx_last_error()
        assert text.startswith(b"mbx_pcm_bands_host: ") and part in text, text

    # everything wrong at once, then one thing fewer each time: the pointers, K, the bound, the form, the size
    refused(b"needed", None, 0, 7, None, 2**40, None)
    refused(b"needed", over.ctypes.data, 0, 7, x.ctypes.data, 2**40, None)
    refused(b"needed", None, 0, 7, x.ctypes.data, 2**40, out.ctypes.data)
    refused(b"K is 1 .. MBX_BANDS_MAX_PROBES", over.ctypes.data, 0, 7, x.ctypes.data, 2**40, out.ctypes.data)
    refused(b"K is 1 .. MBX_BANDS_MAX_PROBES", over.ctypes.data, 33, 7, x.ctypes.data, 2**40, out.ctypes.data)
    refused(b"probe 1: the |s[n]| sum to 65536, above MBX_BANDS_VECTOR_BOUND (65535)", over.ctypes.data, 2, 7, x.ctypes.data, 2**40, out.ctypes.data)
    refused(b"form is MBX_BANDS_COMPLEX or MBX_BANDS_POWER", p.ctypes.data, 2, 7, x.ctypes.data, 2**40, out.ctypes.data)
    refused(b"form is", p.ctypes.data, 2, -1, x.ctypes.data, 4, out.ctypes.data)
    refused(b"2^31-1", p.ctypes.data, 2, 0, x.ctypes.data, 2**40, out.ctypes.data)
    refused(b"2^31-1", p.ctypes.data, 2, 0, x.ctypes.data, (2**31 - 1) // 16 + 1, out.ctypes.data)
    assert L.mbx_pcm_bands_host(over.ctypes.data, 1, 0, x.ctypes.data, 37, out.ctypes.data) == 0, "K = 1 does not look at probe 1"
    assert not out[37 * 8:].any()


def test_the_launcher_the_bank_and_the_session_call_refuse_their_arguments_before_they_ask_for_a_device():
    """never dereferenced: every call below is refused first, on a host with no GPU as well.  What needs a bank (the form, the size, the
    alignment and the overlap of a launch; the session's own refusals) is held through bands_launch_refused in bands_check.cpp and through
    the library in tests/test_gpu_bands.py."""
    L = _lib()

    def refused(fn, name, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = L.mbx_last_error()
        assert name + b":" in text, text
        return text

    # the launcher without a bank: the pointers come first, whatever else is wrong
    for args in ((None, 0, 0x1000, 4, 0x9000, None), (None, 7, 0x1008, 2**40, 0x1008, None), (None, 0, None, 4, None, None)):
        assert b"needed" in refused(L.mbx_pcm_bands, b"mbx_pcm_bands", *args)
    # the bank: the pointers, K, the bound with its probe and vector by name -- and the handle's place is cleared
    _, p, _ = bands_cases.case(37, 2)
    over = np.array(p)
    over[0, 0] = 0
    over[0, 0, [5, 6, 7]] = [-32768, -32767, 1]
    h = C.c_void_p(0x1234)
    create = lambda *a: refused(L.mbx_band_bank_create, b"mbx_band_bank_create", *a)
    assert b"needed" in create(None, p.ctypes.data, 2) and b"needed" in create(C.byref(h), None, 2) and h.value is None
    for K in (0, -1, 33, 2**20):
        h = C.c_void_p(0x1234)
        assert b"K is 1 .. MBX_BANDS_MAX_PROBES" in create(C.byref(h), p.ctypes.data, K) and h.value is None
    h = C.c_void_p(0x1234)
    assert b"probe 0: the |c[n]| sum to 65536, above MBX_BANDS_VECTOR_BOUND (65535)" in create(C.byref(h), over.ctypes.data, 2) and h.value is None
    over[0, 0, 7] = 0
    over[1, 1] = 0
    over[1, 1, [0, 80, 159]] = [32767, -32767, -2]
    assert b"probe 1: the |s[n]| sum to 65536" in create(C.byref(h), over.ctypes.data, 2)
    assert L.mbx_band_bank_destroy(None) == 0 and L.mbx_band_bank_probes(None) == INVALID
    # the session call refuses a missing session by name, whatever else it is given
    for args in ((None, None, 0, None), (None, 0x3000, 0, 0x2000), (None, None, 7, 0x2000)):
        assert L.mbx_session_next_bands(*args) == INVALID and b"mbx_session_next_bands: no session" in L.mbx_last_error()
    # ... and no outputs bit was added: the mask of a session's outputs in the source is the parent's
    src = open(os.path.join(ROOT, "mbelib-neo_amd", "csrc", "mbx_session.hip")).read()
    assert "MBX_SESSION_MIXDOWN | MBX_SESSION_LEVELS)) != 0u" in src and "MBX_SESSION_BANDS" not in src
