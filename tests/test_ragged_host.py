"""CPU suite for ragged batches (a frame count per stream): the two entry points are declared, exported and bound; the six ragged
stream kernels and the order kernel are declared once, written out (no instance macro) and named once each in the launcher's ragged
table, outside kInstances; what the launcher can refuse without a device it refuses as an argument error."""
import ctypes as C
import os
import re

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "mbelib-neo_amd", "csrc")
ENTRY_POINTS = ("mbx_process_batch_ragged", "mbx_process_batch_soft_ragged")
KERNELS = [f"{c}_stream_kernel_ragged{r}" for r in ("", "_res") for c in ("imbe", "ambe", "ambe2400")]
MBE_STATUS_INVALID_ARGUMENT = -1


def _read(name):
    return open(os.path.join(CSRC, name)).read()


def test_the_ragged_entry_points_are_declared_exported_and_bound():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    header = open(os.path.join(ROOT, "include", "mbx.h")).read()
    for name in ENTRY_POINTS:
        assert re.search(r"\bint\s+%s\s*\(int codec, int S, const int32_t\* d_frame_offset, size_t total_frames" % name, header), name
        assert name in _native.EXPORTED_SYMBOLS, name
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in ENTRY_POINTS:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"


def test_the_ragged_kernels_are_declared_once_written_out_and_named_once_in_their_own_table():
    header, stream, api = _read("mbx_kernels.h"), _read("mbx_stream.hip"), _read("mbx_api.hip")
    assert header.count("#define MBX_RAGGED_PARAMS") == 1
    for name in KERNELS:
        assert len(re.findall(r"__global__\s+void\s+%s\s*\(MBX_RAGGED_PARAMS\);" % name, header)) == 1, name
        assert len(re.findall(r"^__global__\s+void\s+__launch_bounds__\([^)]*\)\s*%s\s*\(MBX_RAGGED_PARAMS\)" % name, stream, re.M)) == 1, name
        assert not re.search(r"^MBX_\w+_KERNEL\(%s," % name, stream, re.M), f"{name} is an instance-table macro definition"
        assert api.count(f'"{name}"') == 1 and len(re.findall(r"mbx::%s\b" % name, api)) == 1, name
    assert len(re.findall(r"__global__\s+void\s+ragged_order_kernel\s*\(", header)) == 1
    assert len(re.findall(r"^__global__\s+void\s+__launch_bounds__\([^)]*\)\s*ragged_order_kernel\s*\(", stream, re.M)) == 1
    # the ragged table: all six, each under its own name, ABI row then resident row, columns as in kInstances
    table = api[api.index("kRagged[2][3] = {"):]
    table = table[:table.index("};")]
    rows = re.findall(r'\{"(\w+)",\s*mbx::(\w+)\}', table)
    assert [n for n, _ in rows] == KERNELS and all(n == fn for n, fn in rows)
    # ... and kInstances is what it was
    inst = api[api.index("kInstances[] = {"):]
    inst = inst[:inst.index("};")]
    names = re.findall(r'\{"(\w+)",\s*mbx::\w+\}', inst)
    assert len(names) == 28 and not any("ragged" in n for n in names)
    # the ragged path reads one switch, its own (the launcher's switches are read in mbx_launch_plan.h)
    assert re.findall(r'getenv\("(MBX_RAGGED\w*)"\)', api + _read("mbx_launch_plan.h")) == ["MBX_RAGGED_ORDER"]


def test_the_body_clamps_device_offsets_and_returns_before_the_state_for_a_stream_without_frames():
    """what keeps a bad offset array from faulting a shared card is in the source, not in a test that provokes it"""
    stream = _read("mbx_stream.hip")
    helper = stream[stream.index("StreamRows stream_rows("):]
    helper = helper[:helper.index("\n}\n")]
    assert "slice.total" in helper and re.search(r"lo = lo < 0 \? 0 : \(lo > slice\.total \? slice\.total : lo\)", helper)
    assert re.search(r"hi = hi < lo \? lo : \(hi > slice\.total \? slice\.total : hi\)", helper)
    assert len(re.findall(r"if \(slice\.frame_offset && Tn == 0\) \{[^\n]*\n\s*return;", stream)) == 2   # both bodies, ...
    for body in ("imbe_stream_body(", "ambe_stream_body("):   # ... in front of the first state request
        text = stream[stream.index("\n" + body):]
        assert text.index("Tn == 0") < text.index("stream_map[s]") < text.index("load_"), body


def test_the_launcher_refuses_bad_arguments_before_it_asks_for_a_device():
    from mbelib_neo_amd import _native

    try:
        L = _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))
    ok = dict(codec=0, S=4, off=0x1000, total=8, index=None, frames=0x1000, state=0x1000, resident=None, rng=0x1000, pcm16=None, pcmf=None,
              results=None, records=0x1000, stream=None)   # (never dereferenced: every call below is refused first)
    for fn in (L.mbx_process_batch_ragged, L.mbx_process_batch_soft_ragged):
        for bad in (dict(off=None), dict(frames=None), dict(records=None), dict(state=None), dict(rng=None), dict(S=-1), dict(codec=4),
                    dict(codec=-1)):
            a = dict(ok, **bad)
            assert fn(*a.values()) == MBE_STATUS_INVALID_ARGUMENT, (fn.__name__, bad)
