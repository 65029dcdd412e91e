"""CPU suite for burst input (include/mbx_burst.h): the header held to the library's exports and to the ctypes table, the numpy
definition (bursts.apply_schedule) held to the host route of INTEGRATION.md and to the packers, every refusal of
mbx_burst_schedule_create without a device, the alignment refusals before a device is asked for, and a guarded memory-contract
case (tests/burst_cases.py) demanded for every entry point of the header that takes a device pointer.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import burst_cases
from mbelib_neo_amd import bursts as B
from mbelib_neo_amd.layout import FRAME_BYTES, FRAME_CELLS

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def _declared():
    text = open(os.path.join(ROOT, "include", "mbx_burst.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mbx_\w+)\s*\(([^;{]*?)\)\s*;", text)}


def _lib():
    from mbelib_neo_amd import _native

    try:
        return _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))


def test_every_function_of_the_burst_header_is_exported_and_bound():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert len(declared) >= 13
    assert set(declared) == set(_native.BURST_SYMBOLS)
    assert not set(declared) & set(_native.EXPORTED_SYMBOLS), "EXPORTED_SYMBOLS stays what include/mbx.h declares"
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None, name
    # the limits and the mixed rows are the ones Python uses
    text = open(os.path.join(ROOT, "include", "mbx_burst.h")).read()
    macro = lambda n: int(re.search(rf"#define {n}\s+(\d+)", text).group(1))   # noqa: E731
    assert (macro("MBX_BURST_MAX_FRAMES"), macro("MBX_BURST_MAX_BITS")) == (B.MAX_FRAMES, B.MAX_BITS)
    assert (macro("MBX_MIXED_ROW_BYTES"), macro("MBX_MIXED_ROW_CELLS")) == (B.MIXED_ROW_BYTES, B.MIXED_ROW_CELLS)
    assert B.MAX_FRAMES >= 2 * 9 and B.MAX_BITS >= 2 * 1728, "room above a P25 LDU"


def test_every_burst_entry_point_with_a_device_pointer_has_a_guarded_case():
    declared = _declared()
    with_device_pointer = sorted(f for f, params in declared.items() if re.search(r"\*\s*d_\w+", params))
    assert with_device_pointer == ["mbx_deinterleave", "mbx_deinterleave_soft", "mbx_process_bursts", "mbx_process_bursts_soft"]
    covered = set()
    for c in burst_cases.CASES:
        covered.update(c.covers)
    assert covered == set(with_device_pointer)
    ids = [c.id for c in burst_cases.CASES]
    assert len(ids) == len(set(ids))
    for skip in ("pcm16", "pcmf", "results"):
        assert f"optional-hard-{skip}" in ids and f"optional-soft-{skip}" in ids


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
@pytest.mark.parametrize("F", [1, 3, 9])
def test_apply_schedule_is_the_host_scatter_and_the_packers(codec, F):
    L = _lib()
    rng = np.random.default_rng(100 * codec + F)
    n = B.channel_bits(codec)
    s = B.random_schedule(codec, F, F * n + 131, rng)   # 131 burst bits that no entry names, scattered between the others
    bursts = rng.integers(0, 256, size=(23, s.burst_bytes), dtype=np.uint8)
    got = B.apply_schedule(s, bursts)
    assert got.shape == (23 * F, FRAME_BYTES[codec])
    # (a) the host loop of INTEGRATION.md over mbx_wire_permutation
    assert np.array_equal(got, burst_cases.scatter_like_the_integration_guide(L, s, bursts))
    # (b) the cell arrays the same schedule fills, through the packers
    rows, stride = FRAME_CELLS[codec]
    bits = np.unpackbits(bursts, axis=1)
    cells = np.zeros((23, F, rows * stride), dtype=np.int8)
    for k in range(F):
        cells[:, k, s.cell_row[k] * stride + s.cell_col[k]] = bits[:, s.src_bit[k]]
    packed = np.zeros_like(got)
    pack = {0: L.mbx_pack_imbe7200x4400, 1: L.mbx_pack_ambe3600x2450, 2: L.mbx_pack_imbe7100x4400, 3: L.mbx_pack_ambe3600x2450}[codec]
    assert pack(cells.ctypes.data, 23 * F, packed.ctypes.data) == 0
    assert np.array_equal(got, packed)
    # (c) soft: the cell arrays, off-wire cells zero; its hard decisions are (b)'s cells
    soft = np.stack([bits[:, :s.burst_bits], rng.integers(0, 256, size=(23, s.burst_bits), dtype=np.uint8)], axis=-1)
    got_soft = B.apply_schedule(s, soft, soft=True)
    assert got_soft.shape == (23 * F, rows * stride, 2)
    assert np.array_equal(got_soft[:, :, 0], cells.reshape(23 * F, -1).astype(np.uint8))
    on_wire = np.zeros((F, rows * stride), dtype=bool)
    for k in range(F):
        on_wire[k, s.cell_row[k] * stride + s.cell_col[k]] = True
    assert not got_soft.reshape(23, F, -1, 2)[:, ~on_wire].any()
    # and the inverse the GPU tests build their bursts with
    back = burst_cases.make_bursts(s, got, rng)
    assert np.array_equal(B.apply_schedule(s, back), got)


def test_the_gap_schedule_reads_as_written():
    """48 bits that are not voice, then the frames back to back in row-major cell order: frame k's cell [0][0] is burst bit 48 + 144 k"""
    s = B.gap_schedule(0, 2, gap=48)
    assert s.burst_bits == 48 + 2 * 144 and s.src_bit[1, 0] == 48 + 144 and (s.cell_row[1, 0], s.cell_col[1, 0]) == (0, 0)
    burst = np.zeros((1, s.burst_bytes), dtype=np.uint8)
    burst[0, (48 + 144) >> 3] = 0x80 >> ((48 + 144) & 7)
    frames = B.apply_schedule(s, burst)
    assert not frames[0].any() and frames[1, 2] == 0x02 and not np.delete(frames[1], 2).any()   # cell [0][0] is wire bit 22


def _create(L, codec, F, nbits, src, row, col):
    h = C.c_void_p()
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (src, row, col)]
    rc = L.mbx_burst_schedule_create(C.byref(h), codec, F, nbits, *(x.ctypes.data for x in a))
    return rc, h, (L.mbx_last_error() or b"").decode()


def test_every_refusal_of_schedule_create_comes_before_a_device_is_asked_for():
    import torch

    L = _lib()
    rng = np.random.default_rng(3)
    for codec in (0, 1, 2, 3):
        s = B.random_schedule(codec, 3, 700, rng)
        ok = (s.src_bit, s.cell_row, s.cell_col)

        def refused(why, *args):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            rc, h, text = _create(L, *args)
            assert rc == INVALID and not h.value and "mbx_burst_schedule_create" in text and why in text, (why, rc, text)

        row, col = s.cell_row.copy(), s.cell_col.copy()
        row[1, 5], col[1, 5] = row[1, 6], col[1, 6]
        refused("named twice", codec, 3, 700, s.src_bit, row, col)
        col = s.cell_col.copy()
        col[2, 0] = 24
        refused("not on the codec's wire", codec, 3, 700, s.src_bit, s.cell_row, col)
        src = s.src_bit.copy()
        src[2, 7] = src[0, 1]
        refused("burst bit is named twice", codec, 3, 700, src, s.cell_row, s.cell_col)
        src = s.src_bit.copy()
        src[0, 0] = 700
        refused("outside [0, burst_bits)", codec, 3, 700, src, s.cell_row, s.cell_col)
        src[0, 0] = -1
        refused("outside [0, burst_bits)", codec, 3, 700, src, s.cell_row, s.cell_col)
        refused("no such codec", 4, 3, 700, *ok)
        refused("no such codec", -1, 3, 700, *ok)
        refused("frames_per_burst", codec, 0, 700, *ok)
        refused("frames_per_burst", codec, B.MAX_FRAMES + 1, 700, *ok)
        refused("burst_bits", codec, 3, B.MAX_BITS + 1, *ok)
        refused("fewer bits", codec, 3, 3 * B.channel_bits(codec) - 1, *ok)
        # a valid schedule: now, and only now, a device is asked for -- and fails the way the launchers do
        rc, h, text = _create(L, codec, 3, 700, *ok)
        if torch.cuda.is_available() and L.mbx_device_ready(torch.cuda.current_device()):
            assert rc == 0 and h.value
            assert (L.mbx_burst_schedule_codec(h), L.mbx_burst_schedule_frames(h), L.mbx_burst_schedule_bits(h), L.mbx_burst_schedule_bytes(h)) == (codec, 3, 700, 88)
            L.mbx_burst_schedule_destroy(h)
        else:
            assert rc == (-101 if torch.cuda.is_available() else -100) and not h.value and text, (rc, text)   # MBX_ENOTINIT / MBX_ENODEVICE
    h = C.c_void_p()
    assert L.mbx_burst_schedule_create(C.byref(h), 0, 1, 144, None, None, None) == INVALID
    assert L.mbx_burst_schedule_destroy(None) == 0 and L.mbx_burst_schedule_codec(None) == INVALID and L.mbx_burst_schedule_bytes(None) == 0
    assert L.mbx_burst_workspace_frames(None, 4, 0) == 0


def test_burst_launchers_refuse_pointers_below_their_alignment_before_they_ask_for_a_device():
    L = _lib()

    def refused(who, fn, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()
        assert fn(*args) == INVALID, who
        text = L.mbx_last_error()
        assert b"alignment" in text and who.encode() in text, (who, text)

    # (never dereferenced, no schedule needed: the alignment is looked at first)
    ok = dict(index=0x1000, bursts=0x1000, state=0x1000, resident=0x1000, rng=0x1000, pcm16=0x1000, pcmf=0x1000, results=0x1000, records=0x1000)
    below = dict(index=2, state=2, resident=2, rng=4, pcm16=1, pcmf=2, results=2, records=8)
    for name, by in below.items():
        a = dict(ok)
        a[name] += by
        refused("mbx_process_bursts", L.mbx_process_bursts, None, 4, a["index"], a["bursts"], 64, *list(a.values())[2:], None)
        refused("mbx_process_bursts_soft", L.mbx_process_bursts_soft, None, 4, a["index"], a["bursts"], *list(a.values())[2:], None)
    a = dict(ok, bursts=0x1001)   # soft bursts are 16-bit pairs; hard bursts may sit anywhere
    refused("mbx_process_bursts_soft", L.mbx_process_bursts_soft, None, 4, a["index"], a["bursts"], *list(a.values())[2:], None)
    assert L.mbx_process_bursts(None, 4, a["index"], a["bursts"], 64, *list(a.values())[2:], None) == INVALID
    assert b"alignment" not in L.mbx_last_error() and b"mbx_process_bursts" in L.mbx_last_error()
    refused("mbx_deinterleave_soft", L.mbx_deinterleave_soft, None, 0x1001, 4, 0x1000, 184, None)
    refused("mbx_deinterleave_soft", L.mbx_deinterleave_soft, None, 0x1000, 4, 0x1001, 184, None)
    assert L.mbx_deinterleave(None, 0x1001, 64, 4, 0x1003, 18, None) == INVALID and b"alignment" not in L.mbx_last_error()
