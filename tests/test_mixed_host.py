"""CPU suite for mixed-codec ragged batches: the two entry points are declared, exported and bound; the mixed kernels are declared
once, written out and named once in a table of their own; the Python face checks codecs, lengths and row counts on the host before
the library is touched, and its row packer puts every frame at the front of a row of one size."""
import ctypes as C
import os
import re
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mbelib-neo_amd", "csrc")
ENTRY_POINTS = ("mbx_process_batch_mixed", "mbx_process_batch_soft_mixed")
MBE_STATUS_INVALID_ARGUMENT = -1


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_mixed_entry_points_are_declared_exported_and_bound():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    header = open(os.path.join(ROOT, "include", "mbx.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(int S, const uint8_t\* d_stream_codec, const int32_t\* d_frame_offset, size_t total_frames" % name, header), name
        assert name in _native.EXPORTED_SYMBOLS, name
    assert "MBX_IMBE_FRAME_BYTES (18)" in header and "MBX_IMBE_SOFT_BITS (184)" in header, "the one row size of a mixed batch is stated"
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in ENTRY_POINTS:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"


def test_the_mixed_kernels_are_written_out_share_one_lds_block_and_have_a_table_of_their_own():
    header, stream, api = _read("mbx_kernels.h"), _read("mbx_stream.hip"), _read("mbx_api.hip")
    assert header.count("#define MBX_MIXED_PARAMS") == 1
    for name in ("mixed_stream_kernel_ragged", "mixed_stream_kernel_ragged_res"):
        assert len(re.findall(r"__global__\s+void\s+%s\s*\(MBX_MIXED_PARAMS\);" % name, header)) == 1, name
        assert len(re.findall(r"^__global__\s+void\s+__launch_bounds__\([^)]*\)\s*%s\s*\(MBX_MIXED_PARAMS\)" % name, stream, re.M)) == 1, name
        assert api.count(f'"{name}"') == 1 and len(re.findall(r"mbx::%s\b" % name, api)) == 1, name
    body = stream[stream.index("void mixed_stream_body("):]
    body = body[:body.index("\n}\n")]
    assert body.count("__shared__") == 1 and "__shared__ ParkedLds lds;" in body, "the three bodies share ONE block of LDS"
    assert body.count("imbe_stream_body<") == 1 and body.count("ambe_stream_body<") == 2 and "default:" in body
    inst = api[api.index("kInstances[] = {"):]
    inst = inst[:inst.index("};")]
    names = re.findall(r'\{"(\w+)",\s*mbx::\w+\}', inst)
    assert len(names) == 28 and not any("mixed" in n for n in names)
    ragged = api[api.index("kRagged[2][3] = {"):]
    assert "mixed" not in ragged[:ragged.index("};")]
    # the fronts and the expansion call the per-frame functions of the single-codec kernels: no second copy of any of them
    for src, fns in (("mbx_fec.hip", ("fec_imbe7200x4400_frame(", "fec_imbe7100x4400_frame(", "fec_ambe3600x2450_frame(")),
                     ("mbx_soft_front.hip", ("soft_record_imbe7200x4400(", "soft_record_imbe7100x4400(", "soft_record_ambe3600(")),
                     ("mbx_expand.hip", ("expand_imbe_frame_rec(", "expand_ambe_frame<false>(", "expand_ambe_frame<true>("))):
        text = _read(src)
        kernel = text[text.index("_mixed_kernel("):]
        for fn in fns:
            assert fn in kernel, (src, fn)


def test_the_launcher_refuses_bad_arguments_before_it_asks_for_a_device():
    from mbelib_neo_amd import _native

    try:
        L = _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))
    ok = dict(S=4, codec=0x1000, off=0x1000, total=8, index=None, frames=0x1000, state=0x1000, resident=None, rng=0x1000, pcm16=None, pcmf=None,
              results=None, records=0x1000, stream=None)   # (never dereferenced: every call below is refused first)
    for fn in (L.mbx_process_batch_mixed, L.mbx_process_batch_soft_mixed):
        for bad in (dict(codec=None), dict(off=None), dict(frames=None), dict(records=None), dict(state=None), dict(rng=None), dict(S=-1)):
            a = dict(ok, **bad)
            assert fn(*a.values()) == MBE_STATUS_INVALID_ARGUMENT, (fn.__name__, bad)


def _untouchable(monkeypatch):
    from mbelib_neo_amd import _native, decoder

    def boom(*a, **k):
        raise AssertionError("the library (or torch) was touched before the host checks")

    monkeypatch.setattr(_native, "lib", boom)
    monkeypatch.setattr(decoder, "_torch", boom)
    return decoder


def test_the_python_face_rejects_bad_mixed_batches_on_the_host(monkeypatch):
    decoder = _untouchable(monkeypatch)
    me = types.SimpleNamespace(streams=4, codec=0)
    counts = [1, 0, 2, 3]
    rows = np.zeros((6, 18), np.uint8)
    call = decoder.BatchDecoder.decode_ragged
    with pytest.raises(ValueError, match="codec"):
        call(me, rows, counts, codec=[0, 1, 4, 3])
    with pytest.raises(ValueError, match="codec"):
        call(me, rows, counts, codec=[0, 1, -1, 3])
    with pytest.raises(ValueError, match="codec"):
        call(me, rows, counts, codec=[0, 1, 2])
    with pytest.raises(ValueError, match="codec"):
        call(me, rows, counts, codec=[0.5, 1, 2, 3])
    with pytest.raises(ValueError, match="rows"):
        call(me, np.zeros((5, 18), np.uint8), counts, codec=[0, 1, 2, 3])
    with pytest.raises(ValueError, match="rows"):
        call(me, np.zeros((6, 96, 2), np.uint8), counts, codec=[0, 1, 2, 3], soft=True)
    with pytest.raises(ValueError, match=r"frames\[2\]"):
        call(me, [np.zeros(18, np.uint8), np.zeros(0, np.uint8), np.zeros(18, np.uint8), np.zeros(27, np.uint8)], counts, codec=[0, 1, 2, 3])
    with pytest.raises(AssertionError, match="touched"):   # a well-formed batch gets as far as the device
        call(me, rows, counts, codec=[0, 1, 2, 3])


def test_the_row_packer_puts_every_frame_at_the_front_of_a_row_of_one_size():
    from mbelib_neo_amd import _native, decoder
    from mbelib_neo_amd.layout import FRAME_BYTES

    try:
        L = _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))
    assert (decoder.MIXED_ROW_BYTES, decoder.MIXED_ROW_CELLS) == (18, 184)
    codec, counts = np.array([1, 0, 3, 2, 1]), np.array([2, 1, 0, 3, 1])
    rng = np.random.default_rng(5)
    frames = [rng.integers(0, 256, size=(k, FRAME_BYTES[int(c)]), dtype=np.uint8) for c, k in zip(codec, counts)]
    # the AMBE frames: what mbx_pack_ambe3600x2450 makes of cells (the library's own packer, host code)
    cells = rng.integers(0, 2, size=(2, 4, 24), dtype=np.uint8).astype(np.int8)
    packed = np.zeros((2, 9), np.uint8)
    assert L.mbx_pack_ambe3600x2450(cells.ctypes.data, 2, packed.ctypes.data) == 0
    frames[0] = packed
    rows = decoder.pack_mixed_rows(codec, counts, frames)
    assert rows.shape == (7, 18) and rows.dtype == np.uint8
    assert rows[0:2, :9].tobytes() == packed.tobytes() and not rows[0:2, 9:].any(), "a 9-byte frame sits at the front of its 18-byte row"
    assert rows[2].tobytes() == frames[1].tobytes() and rows[3:6].tobytes() == frames[3].tobytes()
    assert rows[6, :9].tobytes() == frames[4].tobytes() and not rows[6, 9:].any()
    soft = [rng.integers(0, 2, size=(k, decoder.SOFT_CELLS[int(c)], 2), dtype=np.uint8) for c, k in zip(codec, counts)]
    srows = decoder.pack_mixed_rows(codec, counts, soft, soft=True)
    assert srows.shape == (7, 184, 2)
    assert srows[0:2, :96].tobytes() == soft[0].tobytes() and not srows[0:2, 96:].any()
    assert srows[3:6, :168].tobytes() == soft[3].tobytes() and not srows[3:6, 168:].any()
    with pytest.raises(ValueError):
        decoder.pack_mixed_rows(codec, counts, frames[:4])
