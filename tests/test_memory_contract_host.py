"""CPU suite: the guard-band helper of the memory-contract tests (tests/guarded.py) held to planted bytes in a numpy arena; its
alignment table held to the table in include/mbx.h; every exported function that takes a device pointer, and every *_host call, named
by a guarded case (tests/instance_cases.py, tests/memory_cases.py) or by the exemption table below; the launchers' refusal of pointers
below their alignment, before they ask for a device.  Outside this file's reach: the sessions' host buffers and the mbe_* shim (another
header), and the library's own allocations."""
import os
import re

import numpy as np
import pytest

import guarded
import instance_cases
import memory_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MBE_STATUS_INVALID_ARGUMENT = -1


def _header():
    with open(os.path.join(ROOT, "include", "mbx.h")) as f:
        return f.read()


SPECS = [guarded.buf("frames", 18 * 257, "frames", True), guarded.buf("records", 16 * 257, "records"), guarded.buf("pcm16", 320 * 257, "pcm16"),
         guarded.buf("rng", 24 * 257, "rng"), guarded.buf("state", 7812 * 3, "state"), guarded.buf("soft", 368, "soft", True)]


def test_layout_gives_exactly_the_alignment_asked_for_and_guards_of_their_own():
    for base in (0x7F0000000000, 0x7F0000000010, 0x1008, 0x1001, 0x100F):
        slots, total = guarded.plan(SPECS, base)
        assert total <= guarded.plan_bytes(SPECS)
        at = 0
        for s, spec in zip(slots, SPECS):
            a = guarded.ALIGN[spec.kind]
            assert (base + s.start) % a == 0 and (base + s.start) % (2 * a) == a, (hex(base), s)   # this alignment and NO better
            assert s.end - s.start == spec.nbytes                                                   # exact size, no rounding
            assert s.front == at and s.start - s.front >= guarded.GUARD and s.back - s.end == guarded.GUARD   # never shared
            at = s.back
        assert at == total
    assert guarded.GUARD >= 16384 and guarded.GUARD > 7812 and guarded.GUARD > 64 * 16


def test_the_pattern_depends_on_position_and_seed():
    p1, p2 = guarded.pattern_numpy(0, 1 << 16, 1), guarded.pattern_numpy(0, 1 << 16, 2)
    assert p1.dtype == np.uint8 and len(np.unique(p1)) == 256
    assert (p1 != p2).mean() > 0.98
    for shift in (1, 2, 4, 16, 64, 256, 4096):   # no copy of neighbouring guard reproduces it
        assert (p1[shift:] != p1[:-shift]).mean() > 0.98
    assert guarded.pattern_numpy(1000, 2000, 1).tobytes() == p1[1000:2000].tobytes()   # a function of the absolute offset
    assert np.bincount(p1, minlength=256).max() < 2 * (1 << 16) / 256                    # ... that no memset reproduces


def test_a_planted_byte_is_found_and_named():
    a = guarded.Arena(SPECS, where="numpy", seed=1)
    a.load("frames", np.arange(18 * 257, dtype=np.uint8))
    a.load("soft", np.ones(368, dtype=np.uint8))
    a.check()
    s = a.by_name["pcm16"]
    for at, text in ((s.start - 1, r"pcm16: 1 guard byte\(s\) changed IN FRONT OF the payload, 1 \.\. 1 bytes before its first byte"),
                     (s.end, r"pcm16: 1 guard byte\(s\) changed BEHIND the payload of 82240 bytes, 0 \.\. 0 bytes past its end"),
                     (s.end + guarded.GUARD // 2, r"pcm16: 1 guard byte\(s\) changed BEHIND the payload of 82240 bytes, 8192 \.\. 8192 bytes past its end"),
                     (s.end + guarded.GUARD, r"rng: 1 guard byte\(s\) changed IN FRONT OF the payload, \d+ \.\. \d+ bytes before its first byte"),
                     (0, r"frames: 1 guard byte"), (a.used - 1, r"soft: 1 guard byte\(s\) changed BEHIND the payload of 368 bytes, 16383 \.\. 16383")):
        a.mem[at] ^= 0x01
        with pytest.raises(guarded.GuardError, match=text):
            a.check("case x")
        a.mem[at] ^= 0x01
        a.check()
    # a whole row behind the end, and a zeroing memset: counted and located
    a.mem[s.end:s.end + 320] = 0
    with pytest.raises(AssertionError, match=r"case x: pcm16: 3\d\d guard byte\(s\) changed BEHIND the payload of 82240 bytes, [0-2] \.\. 31[7-9] bytes past its end"):
        a.check("case x")
    a.fill(s.end, s.back)
    a.check()
    # writes INSIDE payloads are nobody's business here ...
    a.view("pcm16")[:] = 7
    a.view("records")[-1] = 9
    a.check()
    # ... unless the buffer is a read-only input
    a.view("frames")[4000] ^= 0x10
    a.view("frames")[4100] ^= 0x10
    with pytest.raises(guarded.GuardError, match=r"frames: read-only input changed: 2 byte\(s\), first at offset 4000, last at offset 4100 of 4626"):
        a.check()


def test_outputs_are_prefilled_with_the_pattern_of_their_own_offsets():
    a, b = guarded.Arena(SPECS, seed=1), guarded.Arena(SPECS, seed=2)
    assert a.read("pcm16").tobytes() == a.prefill_bytes("pcm16").tobytes()
    assert a.prefill_bytes("pcm16", 320, 640).tobytes() == a.read("pcm16")[320:640].tobytes()
    assert (a.read("pcm16") != b.read("pcm16")).mean() > 0.98
    a.view("pcm16")[:] = 0
    a.prefill("pcm16")
    assert a.read("pcm16").tobytes() == a.prefill_bytes("pcm16").tobytes()
    assert a.array("records", np.uint32, 257, 4).shape == (257, 4) and a.ptr("records") % 32 == 16


def test_the_alignment_table_is_the_one_in_the_header():
    text = _header()
    table = text[text.index("/* Alignment."):]
    table = table[:table.index("*/")]
    rows = dict((m.group(1), int(m.group(2))) for m in re.finditer(r"^ \*   (\w+) +(\d+) +\S", table, re.M) if m.group(1) != "kind")
    assert rows == guarded.ALIGN
    assert list(rows) == list(guarded.ALIGN), "same order, line for line"


# exported functions with a device pointer that need no guarded case, each with the reason
EXEMPT = {
    "mbx_frame_server_start": "launches a persistent wave that lives until its idle time runs out and writes the buffers of mbx_process_frame through the "
                              "same frame body: there is no one launch to put between two checks, and a second run cannot start from the first one's state",
}
ENTRY_FUNCTIONS = {"batch": ["mbx_process_batch"], "batch_ws": ["mbx_process_batch_ws"], "batch_indexed": ["mbx_process_batch_indexed"],
                   "resident": ["mbx_process_batch_resident", "mbx_resident_materialize"], "resident_indexed": ["mbx_process_batch_resident"],
                   "staged": ["mbx_process_records"]}


def test_every_entry_point_with_a_device_pointer_has_a_guarded_case_or_a_stated_exemption():
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    declared = {m.group(1): m.group(2) for m in re.finditer(r"\b(mbx_\w+)\s*\(([^;{]*?)\)\s*;", text)}
    with_device_pointer = sorted(f for f, params in declared.items()   # ... or the host arrays of the *_host calls
                                 if re.search(r"\*\s*d_\w+", params) or f.endswith("_host"))
    assert len(with_device_pointer) > 35, with_device_pointer
    covered = set()
    for c in instance_cases.CASES:
        covered.update(ENTRY_FUNCTIONS[c.entry])
    for c in memory_cases.CASES:
        covered.update(c.covers)
    assert covered <= set(declared), covered - set(declared)
    assert not covered & set(EXEMPT), covered & set(EXEMPT)
    assert set(EXEMPT) <= set(with_device_pointer), set(EXEMPT) - set(with_device_pointer)
    missing = [f for f in with_device_pointer if f not in covered and f not in EXEMPT]
    assert not missing, f"no memory-contract case (tests/memory_cases.py) and no exemption for: {missing}"


def test_every_instance_case_and_every_form_is_a_guarded_test_id():
    ids = [c.id for c in memory_cases.CASES]
    for soft in ("hard", "soft"):
        for form in ("plain", "resident", "indexed", "resident_indexed"):
            assert f"ragged-{soft}-{form}" in ids and f"mixed-{soft}-{form}" in ids
    for fam in ("stream", "one-launch", "fused", "resident", "indexed", "ragged", "mixed", "soft", "records"):
        assert f"optional-{fam}" in ids
    for needed in ("soft-plain", "soft-ws", "soft-resident-indexed", "records-ws", "expanded-ws", "stage-in", "floattoshort", "materialize", "process-frame",
                   "single-stages", "host-calls"):
        assert needed in ids
    assert {c.entry for c in instance_cases.CASES} <= set(ENTRY_FUNCTIONS)


def test_the_launcher_refuses_pointers_below_their_alignment_before_it_asks_for_a_device():
    from mbelib_neo_amd import _native

    try:
        L = _native.lib()
    except _native.NativeLibraryError as e:
        pytest.skip(str(e))

    def refused(who, fn, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == MBE_STATUS_INVALID_ARGUMENT and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == MBE_STATUS_INVALID_ARGUMENT, who
        text = L.mbx_last_error()
        assert b"alignment" in text and who.encode() in text, (who, text)

    # (never dereferenced: every call below is refused first)
    ok = dict(off=0x1000, total=8, index=0x1000, frames=0x1000, state=0x1000, resident=0x1000, rng=0x1000, pcm16=0x1000, pcmf=0x1000,
              results=0x1000, records=0x1000, stream=None)
    below = dict(off=2, index=2, state=2, resident=2, rng=4, pcm16=1, pcmf=2, results=2, records=8, frames=1)
    for name, by in below.items():
        a = dict(ok)
        a[name] += by
        for codec in (0, 2) if name == "frames" else (0, 1, 2, 3):   # IMBE frames are read in 16-bit pieces, soft cells as 16-bit words
            refused("mbx_process_batch_ragged", L.mbx_process_batch_ragged, codec, 4, *a.values())
            refused("mbx_process_batch_soft_ragged", L.mbx_process_batch_soft_ragged, codec, 4, *a.values())
        refused("mbx_process_batch_mixed", L.mbx_process_batch_mixed, 4, 0x1000, *a.values())   # (rows of 18 bytes: as IMBE frames)
        refused("mbx_process_batch_soft_mixed", L.mbx_process_batch_soft_mixed, 4, 0x1000, *a.values())
        if name in ("state", "rng", "pcm16", "pcmf", "results", "records", "frames"):
            refused("mbx_process_batch", L.mbx_process_batch, 0, 4, 1, a["frames"], a["state"], a["rng"], a["pcm16"], a["pcmf"], a["results"], a["records"], None)
    a = dict(ok, frames=0x1001)   # the 9-byte AMBE frames are read byte by byte and may sit anywhere: a different refusal (no device, or not initialised)
    for codec in (1, 3):
        assert L.mbx_process_batch_ragged(codec, 4, *a.values()) != MBE_STATUS_INVALID_ARGUMENT
        assert L.mbx_process_batch(codec, 4, 1, 0x1001, 0x1000, 0x1000, None, None, None, 0x1000, None) != MBE_STATUS_INVALID_ARGUMENT
