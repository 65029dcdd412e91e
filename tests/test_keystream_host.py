"""CPU suite for keystream input (include/mbx_keystream.h): the header held to the library's exports and to the ctypes table of its
own (_native.KEYSTREAM_SYMBOLS), the row size and the alignment row stated, mbx_keystream_apply_host held to the numpy definition
(mbelib_neo_amd.keystream) and, bit by bit, to mbx_unpack_records, and the guarded memory-contract cases demanded by id for every
entry point that takes device pointers.  No GPU compute here."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import keystream_cases as KC
from mbelib_neo_amd import keystream as K
from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "mbx_keystream.h")
INVALID = -1
FUNCTIONS = ["mbx_keystream_apply_host", "mbx_apply_keystream", "mbx_process_batch_keyed", "mbx_process_batch_ragged_keyed", "mbx_session_submit_keyed"]


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


def test_every_function_of_the_keystream_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert sorted(declared) == sorted(FUNCTIONS)
    assert set(declared) == set(_native.KEYSTREAM_SYMBOLS)
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS):
        assert not set(_native.KEYSTREAM_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name
    text = open(HEADER).read()
    assert int(re.search(r"#define MBX_KEYSTREAM_ROW_BYTES\s+(\d+)", text).group(1)) == K.ROW_BYTES == 12
    # the alignment row of the new kind is stated: keystream 4
    assert re.search(r"^ \*   keystream\s+4\b", text, flags=re.M)
    # include/mbx.h does not know the new calls: a header of its own
    assert not any(f in open(os.path.join(ROOT, "include", "mbx.h")).read() for f in FUNCTIONS)
    # every entry point names the reference lines it stands in for
    for name in FUNCTIONS:
        comment = text[:text.index("int " + name + "(")].rsplit("/*", 1)[1]
        assert "ref " in comment or "reference" in comment, name


def test_every_entry_point_with_device_pointers_has_its_guarded_cases_in_a_list_of_its_own():
    import burst_group_cases
    import memory_cases

    ids = [c.id for c in KC.KEYSTREAM_CASES]
    assert len(ids) == len(set(ids))
    assert not set(ids) & ({c.id for c in memory_cases.CASES} | {c.id for c in burst_group_cases.GROUP_CASES})
    covered = set()
    for c in KC.KEYSTREAM_CASES:
        covered.update(c.covers)
    assert covered == {"mbx_apply_keystream", "mbx_process_batch_keyed", "mbx_process_batch_ragged_keyed"}
    for cid in ("keystream-apply-0", "keystream-apply-1", "keystream-batch-hard", "keystream-batch-soft", "keystream-batch-indexed-resident",
                "keystream-ragged-mixed-hard-abi", "keystream-ragged-mixed-hard-resident", "keystream-ragged-mixed-soft-abi",
                "keystream-ragged-mixed-soft-resident", "keystream-misaligned"):
        assert cid in ids, cid
    for skip in ("pcm16", "pcmf", "results"):
        assert f"keystream-optional-batch-{skip}" in ids and f"keystream-optional-ragged-{skip}" in ids
    # the keystream is registered with the kind whose alignment is its own, 4 bytes; the table of kinds is not extended
    import guarded

    assert guarded.ALIGN["index"] == 4 and "keystream" not in guarded.ALIGN


def _records(n, rng):
    rec = np.zeros(n, dtype=RECORD_DTYPE)
    rec["w"] = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    return rec


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_the_host_function_is_the_numpy_definition_and_the_bit_order_of_unpack_records(codec):
    L = _lib()
    rng = np.random.default_rng(100 + codec)
    n, nbits = 301, K.NBITS[codec]
    assert nbits == (88 if codec in (0, 2) else 49)
    rec0 = _records(n, rng)
    rows = KC.random_rows(n, rng)
    rec = rec0.copy()
    assert L.mbx_keystream_apply_host(codec, rec.ctypes.data, n, rows.ctypes.data) == 0
    assert rec.tobytes() == K.apply(rec0, rows, codec).tobytes()
    assert np.array_equal(rec["w"][:, 3], rec0["w"][:, 3]), "w[3] carries the error context: never touched"
    # record bits beyond nbits are unchanged
    keep = np.array([~np.uint32(m) & np.uint32(0xFFFFFFFF) for m in K.words(np.full((1, 12), 0xFF, dtype=np.uint8), codec)[0]], dtype=np.uint32)
    assert np.array_equal(rec["w"][:, :3] & keep, rec0["w"][:, :3] & keep)
    assert sum(bin(int(~k & 0xFFFFFFFF)).count("1") for k in keep) == nbits
    # the bit order, through the library's own unpacking: imbe_d ^ bits with bits[i] = (row[i >> 3] >> (7 - (i & 7))) & 1
    def unpack(r):
        bits = np.zeros((n, nbits), dtype=np.int8)
        res = np.zeros(n, dtype=RESULT_DTYPE)
        L.mbx_unpack_records(r.ctypes.data, n, nbits, bits.ctypes.data, res.ctypes.data)
        return bits, res

    before, res0 = unpack(rec0)
    after, res1 = unpack(rec)
    key = np.array([[(int(rows[f, i >> 3]) >> (7 - (i & 7))) & 1 for i in range(nbits)] for f in range(n)], dtype=np.int8)
    assert np.array_equal(after, before ^ key) and res0.tobytes() == res1.tobytes()
    assert np.array_equal(key, K.bits_from_rows(rows, codec)) and np.array_equal(K.bits_from_rows(K.rows_from_bits(key), codec), key)
    # bits of the row beyond nbits set to junk change nothing
    junk = rows.copy()
    tail = np.unpackbits(junk, axis=1)
    tail[:, nbits:] ^= rng.integers(0, 2, size=(n, 96 - nbits), dtype=np.uint8)
    junk = np.packbits(tail, axis=1)
    assert not np.array_equal(junk, rows)
    rec2 = rec0.copy()
    assert L.mbx_keystream_apply_host(codec, rec2.ctypes.data, n, junk.ctypes.data) == 0 and rec2.tobytes() == rec.tobytes()
    # applied twice is the identity; an all-zero row leaves its record alone; a row anywhere in memory (no alignment on the host)
    assert L.mbx_keystream_apply_host(codec, rec2.ctypes.data, n, rows.ctypes.data) == 0 and rec2.tobytes() == rec0.tobytes()
    assert L.mbx_keystream_apply_host(codec, rec2.ctypes.data, n, np.zeros((n, 12), dtype=np.uint8).ctypes.data) == 0 and rec2.tobytes() == rec0.tobytes()
    odd = np.zeros(12 * n + 1, dtype=np.uint8)
    odd[1:] = rows.reshape(-1)
    assert L.mbx_keystream_apply_host(codec, rec2.ctypes.data, n, odd.ctypes.data + 1) == 0 and rec2.tobytes() == rec.tobytes()
    assert L.mbx_keystream_apply_host(codec, rec2.ctypes.data, 0, rows.ctypes.data) == 0 and rec2.tobytes() == rec.tobytes()


def test_what_needs_no_device_is_refused_without_one():
    L = _lib()
    rec = _records(4, np.random.default_rng(1))
    rows = np.zeros((4, 12), dtype=np.uint8)
    before = rec.tobytes()
    for codec in (-1, 4, 9):
        assert L.mbx_keystream_apply_host(codec, rec.ctypes.data, 4, rows.ctypes.data) == INVALID and b"mbx_keystream_apply_host" in L.mbx_last_error()
    assert L.mbx_keystream_apply_host(0, None, 4, rows.ctypes.data) == INVALID and L.mbx_keystream_apply_host(0, rec.ctypes.data, 4, None) == INVALID
    assert rec.tobytes() == before
    # the device calls: NULL and bad codec, a pointer below its alignment, both or neither of frames / soft -- before a device is asked for
    assert L.mbx_apply_keystream(0, None, 4, 0x1000, None) == INVALID and L.mbx_apply_keystream(0, 0x1000, 4, None, None) == INVALID
    assert L.mbx_apply_keystream(7, 0x1000, 4, 0x1000, None) == INVALID and b"mbx_apply_keystream" in L.mbx_last_error()
    assert L.mbx_apply_keystream(0, 0x1000, 4, 0x1002, None) == INVALID and b"mbx_keystream.h" in L.mbx_last_error()
    assert L.mbx_apply_keystream(0, 0x1008, 4, 0x1000, None) == INVALID and b"alignment" in L.mbx_last_error()
    pool = (0x1000,) * 8   # state, resident, rng, pcm16, pcmf, results, records, and the stream argument (never reached)
    for frames, soft in ((None, None), (0x1000, 0x1000)):
        assert L.mbx_process_batch_keyed(0, 4, 1, None, frames, soft, 0x1000, *pool[:7], None) == INVALID
        assert b"mbx_process_batch_keyed" in L.mbx_last_error() and b"exactly one" in L.mbx_last_error()
        assert L.mbx_process_batch_ragged_keyed(0, None, 4, 0x1000, 4, None, frames, soft, 0x1000, *pool[:7], None) == INVALID
        assert b"mbx_process_batch_ragged_keyed" in L.mbx_last_error()
        assert L.mbx_session_submit_keyed(None, 4, 1, None, frames, soft, 0x1000, None, None, None, None) == INVALID
    assert L.mbx_process_batch_ragged_keyed(0, None, 4, 0x1000, 4, None, 0x1000, None, 0x1002, *pool[:7], None) == INVALID
    assert b"mbx_keystream.h" in L.mbx_last_error()
    assert L.mbx_session_submit_keyed(None, 4, 1, None, 0x1000, None, 0x1000, None, None, None, None) == INVALID


def test_rows_from_bits_and_apply_refuse_what_they_cannot_take():
    with pytest.raises(ValueError):
        K.rows_from_bits(np.full((2, 88), 2))
    with pytest.raises(ValueError):
        K.rows_from_bits(np.zeros((2, 97), dtype=np.uint8))
    with pytest.raises(ValueError):
        K.apply(np.zeros(2, dtype=RECORD_DTYPE), np.zeros((3, 12), dtype=np.uint8), 0)
    with pytest.raises(ValueError):
        K.words(np.zeros((2, 11), dtype=np.uint8), 0)
    rows = K.rows_from_bits(np.eye(88, dtype=np.uint8))
    assert rows.shape == (88, 12) and rows.dtype == np.uint8 and rows[0, 0] == 0x80 and rows[9, 1] == 0x40 and rows[87, 10] == 0x01
    w = K.words(rows, 0)
    assert w[0, 0] == 0x80000000 and w[31, 0] == 1 and w[32, 1] == 0x80000000 and w[87, 2] == 0x100
    assert not K.words(rows[49:], 1).any() and K.words(rows[48:49], 1)[0, 1] == 0x8000
