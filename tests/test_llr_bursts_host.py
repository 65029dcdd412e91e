"""CPU suite for soft bursts as LLRs (include/mbx_burst.h: mbx_burst_schedule_create_llr, mbx_burst_schedule_soft_bytes;
include/mbx_llr.h: mbx_soft_from_llr): the conversion over every int16 and int8 value against the reference-made fixture, the
oracle and the bytes mbx_soft_bits_from_llr gave before, every refusal of the LLR creator before a device is asked for, the
accessors, and the numpy definition of an LLR gather held to the per-bit one.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import golden_io
import llr_burst_cases as cases
from mbelib_neo_amd import bursts as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def _lib():
    from mbelib_neo_amd import _native

    try:
        return _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))


def _device_ready(L):
    import torch

    if not torch.cuda.is_available():
        return False
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return bool(L.mbx_device_ready(torch.cuda.current_device()))


# ---- the conversion ---------------------------------------------------------------------------------------------------------------
def test_the_conversion_over_every_int16_and_int8_value(oracle):
    L = _lib()
    every16 = np.arange(-32768, 32768, dtype=np.int32).astype(np.int16)
    got = cases.host_cells(L, every16)
    assert np.array_equal(got, cases.old_conversion(every16)), "mbx_soft_bits_from_llr gives other bytes than it gave"
    assert np.array_equal(got, oracle.soft_from_llr(every16))
    assert np.array_equal(got, B.cells_from_llr(every16))
    kat = golden_io.soft_kat()["llr"]
    assert len(kat) and np.array_equal(cases.host_cells(L, kat["llr"]), kat["soft"]) and np.array_equal(B.cells_from_llr(kat["llr"]), kat["soft"])
    at = lambda v: tuple(got[v + 32768])   # noqa: E731
    assert (at(0), at(1), at(-1), at(255), at(256), at(-256), at(32767), at(-32768)) == \
        ((0, 0), (1, 1), (0, 1), (1, 255), (1, 255), (0, 255), (1, 255), (0, 255))
    # an int8 LLR is the int16 LLR of the same value
    every8 = np.arange(-128, 128, dtype=np.int32).astype(np.int8)
    assert np.array_equal(B.cells_from_llr(every8), got[32768 - 128:32768 + 128])
    assert np.array_equal(cases.host_cells(L, every8), B.cells_from_llr(every8))
    assert tuple(B.cells_from_llr(every8)[0]) == (0, 128) and tuple(B.cells_from_llr(every8)[-1]) == (1, 127)
    # ... and back: the LLRs that llr_from_cells makes convert to the cells they were made from
    for form, dtype in B.LLR_DTYPE.items():
        top = np.iinfo(dtype).max
        cells = np.array([(b, r) for b in (0, 1) for r in range(0, min(top, 255) + 1) if (b, r) != (1, 0)], dtype=np.uint8)
        llr = B.llr_from_cells(cells, form)
        assert llr.dtype == dtype and np.array_equal(B.cells_from_llr(llr), cells)
        with pytest.raises(ValueError):
            B.llr_from_cells(np.array([(1, 0)], dtype=np.uint8), form)
    with pytest.raises(ValueError):
        B.llr_from_cells(np.array([(1, 128)], dtype=np.uint8), B.FORM_LLR8)
    assert L.mbx_soft_bits_from_llr(None, got.ctypes.data, 1) == INVALID and L.mbx_soft_bits_from_llr(every16.ctypes.data, None, 1) == INVALID


def test_the_conversion_is_written_once():
    """the host loop, the gather and the flat kernel call the one function of csrc/mbx_llr_cell.h"""
    csrc = os.path.join(ROOT, "mbelib-neo_amd", "csrc")
    read = lambda name: re.sub(r"//.*", "", open(os.path.join(csrc, name)).read())   # noqa: E731  (the code, without its comments)
    assert re.search(r"__host__ __device__", read("mbx_llr_cell.h")) and "soft_cell_from_llr(int v)" in read("mbx_llr_cell.h")
    api = read("mbx_api.hip")
    body = api[api.index("int mbx_soft_bits_from_llr("):]
    assert "soft_cell_from_llr(" in body[:body.index("\n}\n")]
    assert read("mbx_burst.hip").count("soft_cell_from_llr(") == 2 and read("mbx_fec.hip").count("soft_cell_from_llr(") == 2
    for name in ("mbx_soft_front.hip", "mbx_stream.hip"):
        assert "llr" not in read(name).lower(), "the soft fronts take cells: no LLR flag in their kernels"


# ---- the header and the binding -----------------------------------------------------------------------------------------------------
def test_the_llr_entry_points_are_declared_exported_and_bound():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "mbx_llr.h")).read(), flags=re.S)
    declared = re.findall(r"\b(mbx_\w+)\s*\(", text)
    assert declared == ["mbx_soft_from_llr"] == list(_native.LLR_SYMBOLS)
    burst = open(os.path.join(ROOT, "include", "mbx_burst.h")).read()
    macro = lambda n: int(re.search(rf"#define {n}\s+(\d+)", burst).group(1))   # noqa: E731
    assert (macro("MBX_BURST_FORM_LLR16"), macro("MBX_BURST_FORM_LLR8")) == (B.FORM_LLR16, B.FORM_LLR8) == (16, 8)
    assert re.search(r"int mbx_burst_schedule_create_llr\(mbx_burst_schedule\*\* out, int codec, int frames_per_burst, int burst_bits,", burst)
    for name in ("mbx_burst_schedule_create_llr", "mbx_burst_schedule_soft_bytes"):
        assert name in _native.BURST_SYMBOLS
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in ("mbx_soft_from_llr", "mbx_burst_schedule_create_llr", "mbx_burst_schedule_soft_bytes"):
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
        assert getattr(_lib(), name).argtypes is not None


# ---- refusals, before a device is asked for -------------------------------------------------------------------------------------------
def test_every_refusal_of_schedule_create_llr_comes_before_a_device_is_asked_for():
    L = _lib()
    rng = np.random.default_rng(14)
    for codec in (0, 1, 2, 3):
        s = B.random_schedule(codec, 3, 601, rng)
        ok = (s.src_bit, s.cell_row, s.cell_col)

        def refused(why, *args):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            rc, h, text = cases.create_llr(L, *args)
            assert rc == INVALID and not h.value and "mbx_burst_schedule_create" in text and why in text, (why, rc, text)
            return text

        for llr_bytes in (0, -1, 3, 4, 8, 16):
            refused("llr_bytes", codec, 3, 601, *ok, llr_bytes, None)
        for llr_bytes in cases.WIDTHS:
            # the checks mbx_burst_schedule_create_form makes, with its texts
            twice, off_wire, src_twice, outside = (s.cell_row.copy(), s.cell_col.copy()), s.cell_col.copy(), s.src_bit.copy(), s.src_bit.copy()
            twice[0][1, 5], twice[1][1, 5] = twice[0][1, 6], twice[1][1, 6]
            off_wire[2, 0] = 24
            src_twice[2, 7] = src_twice[0, 1]
            outside[0, 0] = 601
            mask = np.zeros(601, dtype=np.uint8)
            mask[600] = 2
            inherited = [
                ("no such codec", (4, 3, 601, *ok, llr_bytes, None)),
                ("frames_per_burst", (codec, 0, 601, *ok, llr_bytes, None)),
                ("frames_per_burst", (codec, B.MAX_FRAMES + 1, 601, *ok, llr_bytes, None)),
                ("burst_bits must be", (codec, 3, 0, *ok, llr_bytes, None)),
                ("burst_bits must be", (codec, 3, B.MAX_BITS + 1, *ok, llr_bytes, None)),
                ("invert", (codec, 3, 601, *ok, llr_bytes, mask)),
                ("fewer bits", (codec, 3, 3 * B.channel_bits(codec) - 1, *ok, llr_bytes, None)),
                ("named twice", (codec, 3, 601, s.src_bit, *twice, llr_bytes, None)),
                ("not on the codec's wire", (codec, 3, 601, s.src_bit, s.cell_row, off_wire, llr_bytes, None)),
                ("burst bit is named twice", (codec, 3, 601, src_twice, s.cell_row, s.cell_col, llr_bytes, None)),
                ("outside [0, burst_bits)", (codec, 3, 601, outside, s.cell_row, s.cell_col, llr_bytes, None)),
            ]
            for why, args in inherited:
                text = refused(why, *args)
                # the same refusal, word for word, as the creator of the three other forms gives (its form check passes: PACKED)
                h = C.c_void_p()
                a = [np.ascontiguousarray(x, dtype=np.int32) for x in args[3:6]]
                inv = None if args[7] is None else np.ascontiguousarray(args[7], dtype=np.uint8)
                rc = L.mbx_burst_schedule_create_form(C.byref(h), *args[:3], *(x.ctypes.data for x in a), B.FORM_PACKED, None if inv is None else inv.ctypes.data)
                assert rc == INVALID and (L.mbx_last_error() or b"").decode() == text
            # the order of the checks: what create_form finds in front of its form check is found in front of llr_bytes too, the rest behind
            assert "frames_per_burst" in refused("frames_per_burst", codec, 0, 601, *ok, 3, None)
            assert "llr_bytes" in refused("llr_bytes", codec, 3, 601, *ok, 3, mask)
            h = C.c_void_p(1)
            assert L.mbx_burst_schedule_create_llr(C.byref(h), codec, 3, 601, None, None, None, llr_bytes, None) == INVALID and not h.value
            assert L.mbx_burst_schedule_create_llr(None, codec, 3, 601, *(x.ctypes.data for x in ok), llr_bytes, None) == INVALID
            # a valid one: now, and only now, a device is asked for
            mask = rng.integers(0, 2, size=601, dtype=np.uint8)
            ready = _device_ready(L)   # (initialises the device where there is one)
            rc, h, text = cases.create_llr(L, codec, 3, 601, *ok, llr_bytes, mask)
            if ready:
                assert rc == 0 and h.value, text
                assert (L.mbx_burst_schedule_form(h), L.mbx_burst_schedule_bits(h)) == (cases.WIDTHS[llr_bytes], 601)
                assert L.mbx_burst_schedule_bytes(h) == 0 and L.mbx_burst_schedule_soft_bytes(h) == 601 * llr_bytes
                assert L.mbx_burst_schedule_soft_cells(h) == (601 if llr_bytes == 2 else 0)
                L.mbx_burst_schedule_destroy(h)
            else:
                assert rc in (-100, -101) and not h.value and text, (rc, text)   # MBX_ENODEVICE / MBX_ENOTINIT


def test_create_form_still_refuses_the_llr_form_values():
    L = _lib()
    rng = np.random.default_rng(15)
    s = B.random_schedule(1, 3, 602, rng)
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (s.src_bit, s.cell_row, s.cell_col)]
    for form in (3, B.FORM_LLR8, B.FORM_LLR16):
        h = C.c_void_p(1)
        assert L.mbx_burst_schedule_create_form(C.byref(h), 1, 3, 602, *(x.ctypes.data for x in a), form, None) == INVALID and not h.value
        assert b"form must be one of MBX_BURST_FORM_*" in L.mbx_last_error()


def test_accessors_of_every_form_and_of_null():
    L = _lib()
    for f in (L.mbx_burst_schedule_soft_bytes, L.mbx_burst_schedule_soft_cells, L.mbx_burst_schedule_bytes):
        assert f(None) == 0
    assert L.mbx_burst_schedule_form(None) == INVALID
    assert L.mbx_burst_validate(None, b"\0" * 8, 0, 1, 1) == INVALID
    assert L.mbx_soft_from_llr(None, 2, 4, None, None) == INVALID and b"mbx_soft_from_llr" in L.mbx_last_error()
    # the Python model of every form
    rng = np.random.default_rng(16)
    for form, want in ((B.FORM_PACKED, (76, 602, 1204)), (B.FORM_BITS, (602, 602, 1204)), (B.FORM_DIBITS, (301, 301, 602)), (B.FORM_LLR16, (0, 602, 1204)),
                       (B.FORM_LLR8, (0, 0, 602))):
        s = B.random_schedule(1, 3, 602, rng, form=form)
        assert (s.burst_bytes, s.soft_cells, s.soft_bytes) == want
    if not _device_ready(L):
        pytest.skip("the accessors of a schedule need a schedule, a schedule needs a device (tests/test_gpu_llr_bursts.py runs the same check)")
    for form in (B.FORM_PACKED, B.FORM_BITS, B.FORM_DIBITS, B.FORM_LLR16, B.FORM_LLR8):
        s = B.random_schedule(1, 3, 602, rng, device=True, form=form)
        cases.check_accessors(L, s)
        s.close()


# ---- the numpy definition --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("llr_bytes", [2, 1], ids=["int16", "int8"])
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_apply_schedule_of_llr_bursts_is_the_per_bit_model_on_host_converted_cells(codec, llr_bytes, masked):
    L = _lib()
    rng = np.random.default_rng(500 + 100 * codec + 10 * llr_bytes + masked)
    n = 23
    for F, nbits in cases.gather_shapes(codec):
        mask = rng.integers(0, 2, size=nbits, dtype=np.uint8) if masked else None
        s = B.random_schedule(codec, F, nbits, rng, form=cases.WIDTHS[llr_bytes], invert=mask)
        per_bit = s.in_form(B.FORM_PACKED, mask)
        llr = cases.random_llrs(rng, n, s, llr_bytes)
        assert llr.dtype == cases.DTYPE[llr_bytes] and llr.shape == (n, nbits)
        for v in cases.PLANTED[llr_bytes]:
            assert (llr[:, np.unique(s.src_bit)] == v).any(), v
        cells = cases.host_cells(L, llr)
        want = B.apply_schedule(per_bit, cells, soft=True)
        assert want.any() and np.array_equal(B.apply_schedule(s, llr, soft=True), want)
        assert np.array_equal(B.apply_schedule(s, llr.view(np.uint8), soft=True), want), "the bytes of the LLRs are taken as they are"
        if masked:
            assert not np.array_equal(want, B.apply_schedule(s.in_form(B.FORM_PACKED), cells, soft=True)), "the sequence changes the hard decisions"
        # to_form: the LLRs that say what the cells say convert back to them
        again = B.to_form(s, B.cells_from_llr(cases.llrs_carrying(cells, llr_bytes)), soft=True)
        assert again.dtype == cases.DTYPE[llr_bytes] and np.array_equal(again, cases.llrs_carrying(cells, llr_bytes))
        with pytest.raises(ValueError):
            B.apply_schedule(s, np.zeros((n, 8), dtype=np.uint8))   # no hard bursts
        with pytest.raises(ValueError):
            B.to_form(s, np.zeros((n, s.packed_bytes), dtype=np.uint8))


def test_bursts_per_workgroup_of_the_shapes_the_gpu_suite_runs():
    """the counts of tests/test_gpu_llr_bursts.py end inside, at and behind the first workgroup for every shape and width"""
    assert [cases.bursts_per_workgroup(w, b) for w, b in ((2, 601), (1, 601), (2, 2159), (1, 2159), (2, 72), (1, 72), (1, 4096), (2, 4096))] == \
        [16, 32, 7, 15, 16, 32, 8, 4]
    assert cases.counts(1, 2159) == [1, 15, 16, 97]
    src = open(os.path.join(ROOT, "mbelib-neo_amd", "csrc", "mbx_burst.hip")).read()
    assert re.search(r"kSoftStageBytes = (\d+)", src).group(1) == str(cases.STAGE_BYTES)
    assert re.search(r"kSoftLlr8Bursts = (\d+)", src).group(1) == str(cases.MOST_BURSTS[1])
