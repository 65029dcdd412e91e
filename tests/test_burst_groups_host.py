"""CPU suite for burst groups (include/mbx_burst_groups.h): the header held to the library's exports and to the ctypes table of its
own (_native.GROUP_SYMBOLS), every refusal that needs no schedule returned without a device (the ones that need one: the GPU suite),
the numpy definition (bursts.apply_groups) held to per-group apply_schedule with hand-made offsets, and a guarded memory-contract
case demanded for the entry point that takes device pointers.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import burst_group_cases as G
from mbelib_neo_amd import bursts as B

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INVALID = -1


def _declared():
    text = open(os.path.join(ROOT, "include", "mbx_burst_groups.h")).read()
    text = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    return {m.group(1): m.group(2) for m in re.finditer(r"\b(mbx_\w+)\s*\(([^;{]*?)\)\s*;", text)}


def _lib():
    from mbelib_neo_amd import _native

    try:
        return _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))


def test_every_function_of_the_groups_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert sorted(declared) == sorted(["mbx_process_burst_groups", "mbx_burst_groups_workspace_frames", "mbx_burst_groups_rows",
                                       "mbx_session_create_mixed", "mbx_session_submit_burst_groups"])
    assert set(declared) == set(_native.GROUP_SYMBOLS)
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS):
        assert not set(_native.GROUP_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name
    text = open(os.path.join(ROOT, "include", "mbx_burst_groups.h")).read()
    assert int(re.search(r"#define MBX_BURST_MAX_GROUPS\s+(\d+)", text).group(1)) == B.MAX_GROUPS == 8
    # the struct Python fills is the header's, field for field
    body = re.search(r"typedef struct mbx_burst_group \{(.*?)\} mbx_burst_group;", re.sub(r"/\*.*?\*/", "", text, flags=re.S), flags=re.S).group(1)
    fields = [re.search(r"(\w+)\s*$", f).group(1) for f in body.split(";") if f.strip()]
    assert fields == [f[0] for f in _native.BurstGroupStruct._fields_]
    assert C.sizeof(_native.BurstGroupStruct) == 48
    # the alignment rows of the new pointers are stated
    for kind in ("bursts", "softbursts", "index"):
        assert re.search(rf"^ \*   {kind}\s+\d", text, flags=re.M), kind


def test_the_entry_point_with_device_pointers_has_its_guarded_cases_in_a_list_of_its_own():
    import burst_cases

    ids = [c.id for c in G.GROUP_CASES]
    assert len(ids) == len(set(ids)) and not set(ids) & {c.id for c in burst_cases.CASES}
    covered = set()
    for c in G.GROUP_CASES:
        covered.update(c.covers)
    assert covered == {"mbx_process_burst_groups"}
    for skip in ("pcm16", "pcmf", "results"):
        assert f"groups-optional-hard-{skip}" in ids and f"groups-optional-soft-{skip}" in ids
    for form in ("hard-resident", "hard-abi", "soft-resident", "soft-abi"):
        assert f"groups-{form}" in ids


def _group(**over):
    g = dict(sched=None, bursts=0x1000, burst_stride=64, n_streams=4, bursts_per_stream=1, stream_index=0x1000, first_slot=0)
    g.update(over)
    return g


def _array(*groups):
    from mbelib_neo_amd import _native

    arr = (_native.BurstGroupStruct * max(len(groups), 1))()
    for a, g in zip(arr, groups):
        for k, v in g.items():
            setattr(a, k, v)
    return arr


def test_every_refusal_that_needs_no_schedule_comes_before_a_device_is_asked_for():
    L = _lib()
    pool = dict(state=0x1000, resident=0x1000, rng=0x1000, pcm16=0x1000, pcmf=0x1000, results=0x1000, records=0x1000)

    def refused(why, arr, n, soft=0, who="mbx_process_burst_groups", **over):
        a = dict(pool, **over)
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        if who == "mbx_process_burst_groups":
            rc = L.mbx_process_burst_groups(arr, n, soft, *a.values(), None)
        else:
            rc = L.mbx_session_submit_burst_groups(0x1000 if over.get("session", True) else None, arr, n, soft, None, None, None)
        text = (L.mbx_last_error() or b"").decode()
        assert rc == INVALID and who in text and why in text, (why, rc, text)

    ok = _array(_group())
    # (a session is looked at only after the groups: 0x1000 is never dereferenced)
    for who in ("mbx_process_burst_groups", "mbx_session_submit_burst_groups"):
        refused("n_groups", ok, -1, who=who)
        refused("n_groups", ok, B.MAX_GROUPS + 1, who=who)
        refused("groups is NULL", None, 1, who=who)
        refused("without a schedule", ok, 1, who=who)
        refused("negative", _array(_group(n_streams=-1)), 1, who=who)
        refused("bursts_per_stream", _array(_group(bursts_per_stream=0)), 1, who=who)
        refused("bursts_per_stream", _array(_group(bursts_per_stream=-2), _group()), 2, who=who)
        refused("alignment", _array(_group(stream_index=0x1002)), 1, who=who)
        refused("alignment", _array(_group(bursts=0x1001)), 1, soft=1, who=who)   # soft bursts are 16-bit pieces ...
        refused("without a schedule", _array(_group(bursts=0x1001)), 1, soft=0, who=who)   # ... hard bursts may sit anywhere
        # of a group without streams neither pointer is looked at, not even its alignment
        refused("without a schedule", _array(_group(n_streams=0, bursts=0x1001, stream_index=0x1002)), 1, soft=1, who=who)
    refused("no session", ok, 1, who="mbx_session_submit_burst_groups", session=False)
    # the pools and outputs of the device call, below their alignment
    for name, by in dict(state=2, resident=2, rng=4, pcm16=1, pcmf=2, results=2, records=8).items():
        refused("alignment", ok, 1, **{name: pool[name] + by})
    # the two host-only calls
    rows = np.zeros(B.MAX_GROUPS + 1, dtype=np.int32)
    assert L.mbx_burst_groups_rows(ok, 1, rows.ctypes.data) == INVALID and b"mbx_burst_groups_rows" in L.mbx_last_error()
    assert L.mbx_burst_groups_rows(ok, 9, rows.ctypes.data) == INVALID and L.mbx_burst_groups_rows(None, 0, None) == INVALID
    assert L.mbx_burst_groups_rows(None, 0, rows.ctypes.data) == 0 and rows[0] == 0
    assert L.mbx_burst_groups_workspace_frames(ok, 1, 0) == 0 and L.mbx_burst_groups_workspace_frames(None, 0, 0) == 0
    # no groups: nothing to do, and no device is asked for
    assert L.mbx_session_create_mixed(None, 4, None, 16, 1) == INVALID
    h = C.c_void_p()
    bad = np.array([0, 1, 4, 3], dtype=np.uint8)
    assert L.mbx_session_create_mixed(C.byref(h), 4, None, 16, 1) == INVALID and b"mbx_session_create_mixed" in L.mbx_last_error()
    assert L.mbx_session_create_mixed(C.byref(h), 4, bad.ctypes.data, 16, 1) == INVALID and b"stream_codec" in L.mbx_last_error() and not h.value
    assert L.mbx_session_create_mixed(C.byref(h), 0, bad.ctypes.data, 16, 1) == INVALID


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_apply_groups_is_apply_schedule_per_group_with_hand_made_offsets(soft):
    shapes = G.SOFT if soft else G.HARD
    scheds = G.schedules(shapes, 7, device=False)
    groups = G.make_groups(shapes, scheds, soft, 11, tag=1)
    empty = B.BurstGroup(scheds[1], np.zeros(0, dtype=np.uint8), 0, 3)
    slots = G.slots_of_groups(shapes)
    free = int(np.setdiff1d(np.arange(G.POOL), np.concatenate(slots))[-1])   # a slot no group names
    by_slot = B.BurstGroup(scheds[2], groups[2].bursts, 1, 1, stream_index=None, first_slot=free, burst_stride=groups[2].burst_stride)
    order = [groups[0], empty, groups[1], by_slot, groups[3]]
    lay = B.apply_groups(order, soft)
    assert lay["row_of_group"].tolist() == [0, 130, 130, 340, 341, G.FRAMES] and np.array_equal(lay["row_of_group"], B.group_rows(order))
    # by hand: 65 streams of 2 frames, 35 of 2 x 3, one of 1, 64 of 1
    offsets = np.concatenate([np.arange(65) * 2, 130 + np.arange(35) * 6, [340], 341 + np.arange(64), [G.FRAMES]])
    assert np.array_equal(lay["frame_offset"], offsets) and lay["frame_offset"].dtype == np.int32
    assert np.array_equal(lay["stream_codec"], np.repeat([0, 1, 3, 2], [65, 35, 1, 64])) and lay["stream_codec"].dtype == np.uint8
    assert np.array_equal(lay["stream_index"], np.concatenate([slots[0], slots[1], [free], slots[3]])) and lay["stream_index"].dtype == np.int32
    assert np.unique(lay["stream_index"]).size == G.STREAMS
    width = {0: 18, 1: 9, 2: 18, 3: 9} if not soft else {0: 184, 1: 96, 2: 168, 3: 96}
    for g, first in zip(order, lay["row_of_group"][:-1]):
        if not g.n_streams:
            continue
        s = g.schedule
        own = B.apply_schedule(s, g.bursts, soft=True) if soft else B.apply_schedule(s, g.bursts, burst_stride=g.burst_stride)
        rows = lay["rows"][first:first + g.frames]
        assert own.shape[:2] == (g.frames, width[s.codec])
        assert np.array_equal(rows[:, :width[s.codec]], own) and not rows[:, width[s.codec]:].any()
    assert lay["rows"].shape == ((G.FRAMES, 184, 2) if soft else (G.FRAMES, 18))
    # what the host can refuse
    with pytest.raises(ValueError):
        B.apply_groups([groups[0]] * 9, soft)
    with pytest.raises(ValueError):
        B.apply_groups([B.BurstGroup(scheds[0], groups[0].bursts, 65, 0, stream_index=slots[0])], soft)
    with pytest.raises(ValueError):
        B.apply_groups([B.BurstGroup(scheds[0], groups[0].bursts, 65, 1, stream_index=slots[0][:-1])], soft)
