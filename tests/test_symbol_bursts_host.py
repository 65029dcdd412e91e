"""CPU suite for burst input in the receiver's forms (include/mbx_burst.h: mbx_burst_schedule_create_form, mbx_burst_validate):
every new refusal of schedule creation before a device is asked for, mbx_burst_schedule_create held to create_form(PACKED, NULL),
the host check, and the numpy definition of every form and inversion sequence (bursts.apply_schedule of bursts.to_form) held to
the packed form with the sequence XORed on by the host.  No GPU compute here."""
import ctypes as C

import numpy as np
import pytest

import symbol_burst_cases as cases
from mbelib_neo_amd import bursts as B
from mbelib_neo_amd.layout import FRAME_BYTES

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


def _create_form(L, codec, F, nbits, src, row, col, form, invert):
    h = C.c_void_p()
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (src, row, col)]
    inv = None if invert is None else np.ascontiguousarray(invert, dtype=np.uint8)
    rc = L.mbx_burst_schedule_create_form(C.byref(h), codec, F, nbits, *(x.ctypes.data for x in a), form, None if inv is None else inv.ctypes.data)
    return rc, h, (L.mbx_last_error() or b"").decode()


def _create(L, codec, F, nbits, src, row, col):
    h = C.c_void_p()
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (src, row, col)]
    rc = L.mbx_burst_schedule_create(C.byref(h), codec, F, nbits, *(x.ctypes.data for x in a))
    return rc, h, (L.mbx_last_error() or b"").decode()


def test_every_new_refusal_of_schedule_create_form_comes_before_a_device_is_asked_for():
    L = _lib()
    rng = np.random.default_rng(4)
    for codec in (0, 1, 2, 3):
        s = B.random_schedule(codec, 3, 700, rng)
        ok = (s.src_bit, s.cell_row, s.cell_col)

        def refused(why, *args):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            rc, h, text = _create_form(L, *args)
            assert rc == INVALID and not h.value and "mbx_burst_schedule_create" in text and why in text, (why, rc, text)

        for form in (-1, 3, 7):
            refused("form", codec, 3, 700, *ok, form, None)
        odd = B.random_schedule(codec, 3, 701, rng)
        refused("even burst_bits", codec, 3, 701, odd.src_bit, odd.cell_row, odd.cell_col, B.FORM_DIBITS, None)
        for form in cases.FORMS.values():
            for at in (0, 350, 699):
                mask = cases.random_mask(rng, 700)
                mask[at] = 2
                refused("invert", codec, 3, 700, *ok, form, mask)
            # the checks mbx_burst_schedule_create makes are made for every form
            src = s.src_bit.copy()
            src[0, 0] = 700
            refused("outside [0, burst_bits)", codec, 3, 700, src, s.cell_row, s.cell_col, form, None)
            refused("fewer bits", codec, 3, 3 * B.channel_bits(codec) - 2, *ok, form, None)
        # valid ones: now, and only now, a device is asked for
        for form, nbits, arrays in ((B.FORM_BITS, 701, odd), (B.FORM_DIBITS, 700, s), (B.FORM_PACKED, 700, s)):
            mask = cases.random_mask(rng, nbits)
            rc, h, text = _create_form(L, codec, 3, nbits, arrays.src_bit, arrays.cell_row, arrays.cell_col, form, mask)
            if _device_ready(L):
                assert rc == 0 and h.value, text
                assert (L.mbx_burst_schedule_form(h), L.mbx_burst_schedule_bits(h)) == (form, nbits)
                assert L.mbx_burst_schedule_bytes(h) == {B.FORM_BITS: 701, B.FORM_DIBITS: 350, B.FORM_PACKED: 88}[form]
                assert L.mbx_burst_schedule_soft_cells(h) == (350 if form == B.FORM_DIBITS else nbits)
                L.mbx_burst_schedule_destroy(h)
            else:
                assert rc in (-100, -101) and not h.value and text, (rc, text)   # MBX_ENODEVICE / MBX_ENOTINIT
    assert L.mbx_burst_schedule_form(None) == INVALID and L.mbx_burst_schedule_soft_cells(None) == 0
    assert L.mbx_burst_validate(None, None, 0, 0, 0) == INVALID


def test_schedule_create_is_create_form_packed_without_a_sequence():
    """the same arguments are accepted or refused alike, with the same code and the same reason"""
    L = _lib()
    rng = np.random.default_rng(5)
    for codec in (0, 1, 2, 3):
        s = B.random_schedule(codec, 3, 700, rng)
        twice, off_wire, src_twice, outside = (s.cell_row.copy(), s.cell_col.copy()), s.cell_col.copy(), s.src_bit.copy(), s.src_bit.copy()
        twice[0][1, 5], twice[1][1, 5] = twice[0][1, 6], twice[1][1, 6]
        off_wire[2, 0] = 24
        src_twice[2, 7] = src_twice[0, 1]
        outside[0, 0] = -1
        argsets = [
            (codec, 3, 700, s.src_bit, s.cell_row, s.cell_col),
            (codec, 3, 700, s.src_bit, *twice),
            (codec, 3, 700, s.src_bit, s.cell_row, off_wire),
            (codec, 3, 700, src_twice, s.cell_row, s.cell_col),
            (codec, 3, 700, outside, s.cell_row, s.cell_col),
            (4, 3, 700, s.src_bit, s.cell_row, s.cell_col),
            (codec, 0, 700, s.src_bit, s.cell_row, s.cell_col),
            (codec, B.MAX_FRAMES + 1, 700, s.src_bit, s.cell_row, s.cell_col),
            (codec, 3, B.MAX_BITS + 1, s.src_bit, s.cell_row, s.cell_col),
            (codec, 3, 3 * B.channel_bits(codec) - 1, s.src_bit, s.cell_row, s.cell_col),
        ]
        for i, args in enumerate(argsets):
            rc_a, h_a, text_a = _create(L, *args)
            rc_b, h_b, text_b = _create_form(L, *args, B.FORM_PACKED, None)
            assert rc_a == rc_b and bool(h_a.value) == bool(h_b.value), (i, rc_a, rc_b)
            if rc_a < 0:
                assert text_a == text_b and text_a, (i, text_a, text_b)
                assert (rc_a == INVALID) == (i > 0), "only the first set is a valid schedule"
            else:
                for f in (L.mbx_burst_schedule_form, L.mbx_burst_schedule_bytes, L.mbx_burst_schedule_soft_cells, L.mbx_burst_schedule_bits):
                    assert f(h_a) == f(h_b)
                assert (L.mbx_burst_schedule_form(h_a), L.mbx_burst_schedule_bytes(h_a), L.mbx_burst_schedule_soft_cells(h_a)) == (B.FORM_PACKED, 88, 700)
            L.mbx_burst_schedule_destroy(h_a)
            L.mbx_burst_schedule_destroy(h_b)
    h = C.c_void_p()
    assert L.mbx_burst_schedule_create_form(C.byref(h), 0, 1, 144, None, None, None, B.FORM_PACKED, None) == INVALID and not h.value


def test_burst_validate_looks_at_the_bytes_a_gather_reads_and_at_no_others():
    """(a schedule lives on a device: without one only the NULL refusals can be seen here, and tests/test_gpu_symbol_bursts.py runs
    the same matrix)"""
    L = _lib()
    assert L.mbx_burst_validate(None, b"\0" * 8, 8, 1, 0) == INVALID and L.mbx_burst_validate(None, b"\0" * 8, 8, 1, 1) == INVALID
    if not _device_ready(L):
        pytest.skip("mbx_burst_validate needs a schedule, a schedule needs a device")
    rng = np.random.default_rng(6)
    cases.validate_matrix(L, lambda form: B.random_schedule(1, 3, 602, rng, device=True, form=form))


@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("form", list(cases.FORMS.values()), ids=list(cases.FORMS))
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_apply_schedule_of_to_form_is_apply_schedule_of_the_packed_bursts(codec, form, masked):
    rng = np.random.default_rng(100 * codec + 10 * form + masked)
    n = 23
    for F, nbits in ((3, 3 * B.channel_bits(codec) + 170), (1, B.channel_bits(codec)), (9, 9 * B.channel_bits(codec) + 431 + (form == B.FORM_DIBITS))):
        mask = cases.random_mask(rng, nbits) if masked else None
        s = B.random_schedule(codec, F, nbits, rng, form=form, invert=mask)
        assert s.burst_bytes == {B.FORM_PACKED: (nbits + 7) // 8, B.FORM_BITS: nbits, B.FORM_DIBITS: nbits // 2}[form]
        assert s.soft_cells == (nbits // 2 if form == B.FORM_DIBITS else nbits)
        plain = s.in_form(B.FORM_PACKED)
        # hard
        packed = cases.packed_input(s, n, rng, False)
        want = B.apply_schedule(plain, cases.scrambled(packed, mask, False))
        assert want.shape == (n * F, FRAME_BYTES[codec]) and want.any()
        if mask is not None:
            assert not np.array_equal(want, B.apply_schedule(plain, packed)), "the sequence changes the frames"
        clean, junky = B.to_form(s, packed), B.to_form(s, packed, junk=rng)
        assert clean.shape == junky.shape == (n, s.burst_bytes)
        if form != B.FORM_PACKED:
            assert clean.max() <= (1 if form == B.FORM_BITS else 3) and junky.max() > 3
        assert np.array_equal(B.apply_schedule(s, clean), want) and np.array_equal(B.apply_schedule(s, junky), want)
        stride = s.burst_bytes + 3
        assert np.array_equal(B.apply_schedule(s, cases.strided(junky, stride, rng), burst_stride=stride), want)
        if codec == 2:   # the two bits that pad the last byte are zero whatever the sequence says
            assert not (want[:, -1] & 3).any()
        # soft
        soft = cases.packed_input(s, n, rng, True)
        want = B.apply_schedule(plain, cases.scrambled(soft, mask, True), soft=True)
        clean, junky = B.to_form(s, soft, soft=True), B.to_form(s, soft, soft=True, junk=rng)
        assert clean.shape == junky.shape == (n, s.soft_cells, 2)
        assert np.array_equal(B.apply_schedule(s, clean, soft=True), want) and np.array_equal(B.apply_schedule(s, junky, soft=True), want)
        on_wire = np.zeros((F, want.shape[1]), dtype=bool)
        from mbelib_neo_amd.layout import FRAME_CELLS

        for k in range(F):
            on_wire[k, s.cell_row[k] * FRAME_CELLS[codec][1] + s.cell_col[k]] = True
        assert not want.reshape(n, F, -1, 2)[:, ~on_wire].any(), "cells that are not on the wire stay {0, 0}"
        if form == B.FORM_DIBITS and nbits > 1:
            uneven = soft.copy()
            uneven[3, 1, 1] ^= 0x10
            with pytest.raises(ValueError):
                B.to_form(s, uneven, soft=True)
