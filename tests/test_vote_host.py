"""CPU suite for voted streams (include/mbx_vote.h): the arithmetic and the refusals of mbelib-neo_amd/csrc/mbx_vote_plan.h through the
stand-alone program tests/vote_check.cpp, built with AddressSanitizer and UndefinedBehaviorSanitizer exactly as tests/test_bands_host.py
builds its program (an executable of its own; nothing is loaded into this process); the numpy definition (mbelib_neo_amd.vote) on
answers written out by hand for every clause of the two rules; mbx_vote_select_host and mbx_vote_combine_host held to numpy byte for
byte; the refusals of the plan, the launchers and the whole steps before a device is asked for; the header held to the library's exports
and to the ctypes table of its own (_native.VOTE_SYMBOLS); the launch plan's entry for the voted forms; and the decoding experiment:
four noisy sites of 200 clean frames through the CPU oracle's FEC.  No GPU compute here."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import vote_cases
from mbelib_neo_amd import vote
from test_launch_plan_host import clean_env

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HEADER = os.path.join(ROOT, "include", "mbx_vote.h")
INVALID = -1
FUNCTIONS = ["mbx_vote_plan_create", "mbx_vote_plan_destroy", "mbx_vote_plan_streams", "mbx_vote_plan_candidates", "mbx_vote_select", "mbx_vote_combine",
             "mbx_vote_select_host", "mbx_vote_combine_host", "mbx_vote_workspace_frames", "mbx_process_batch_voted", "mbx_process_batch_soft_voted"]


@pytest.fixture(scope="module")
def check_exe(tmp_path_factory):
    cxx = shutil.which("g++")
    if cxx is None:
        pytest.fail("g++ is needed to build tests/vote_check.cpp")
    exe = str(tmp_path_factory.mktemp("vote") / "vote_check")
    build = subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                            # (the sanitizer runtimes linked into the program: see tests/test_flush_plan_host.py)
                            "-static-libasan", "-static-libubsan",
                            "-Wall", "-Wextra", "-Werror",
                            "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "mbelib-neo_amd", "csrc"),
                            os.path.join(HERE, "vote_check.cpp"), "-o", exe], capture_output=True, text=True, timeout=300)
    assert build.returncode == 0, build.stderr[-4000:]
    return exe


def test_the_arithmetic_and_the_refusals_hold_under_asan_and_ubsan(check_exe):
    run = subprocess.run([check_exe], capture_output=True, text=True, timeout=300, env=clean_env())
    assert run.returncode == 0, (run.stdout + run.stderr)[-4000:]
    last = run.stdout.strip().splitlines()[-1]
    found = re.fullmatch(r"vote_check: ok \(16 lanes per frame, up to (\d+) candidates, pieces of 8 cells\)", last)
    assert found, run.stdout
    assert int(found.group(1)) == vote.MAX_CANDIDATES


# ---- the numpy definition on answers written out by hand ------------------------------------------------------------------------------
def test_select_on_known_answers():
    """a tie on the total broken by c0; a tie on both broken by the lower index; a winner that is the last of 32; absent candidates
    skipped; all absent: candidate 0's record and MBX_VOTE_NONE; agree and second by hand; best saturating at 255"""
    rec, present, off, rows = vote_cases.crafted_select()
    assert off[-1] == 48 and len(rows) == 7 and max(np.diff(off)) == 32
    voted, votes = vote.select(rec, present, off, 1)
    assert voted.shape == (7, 1, 4) and votes.shape == (7, 1) and votes.dtype == vote.VOTE_DTYPE
    assert [votes.dtype.fields[f][1] for f in ("winner", "present", "best", "second", "agree")] == [0, 1, 2, 3, 4]
    for s, (row, winner, there, best, second, agree) in enumerate(rows):
        assert voted[s, 0].tobytes() == rec[row, 0].tobytes(), f"group {s}: the winner's 16 bytes, unchanged"
        assert tuple(int(x) for x in votes[s, 0]) == (winner, there, best, second, agree), (s, votes[s, 0])
    # without the present bytes everybody is there: group 3 is won by its candidate 0 (no errors), group 4 by its candidate 1
    voted, votes = vote.select(rec, None, off, 1)
    assert (int(votes["winner"][3, 0]), int(votes["present"][3, 0]), int(votes["second"][3, 0])) == (0, 3, 2)
    assert (int(votes["winner"][4, 0]), int(votes["best"][4, 0]), int(votes["second"][4, 0]), int(votes["agree"][4, 0])) == (1, 0, 0, 0b10)
    # the layout: frame t of candidate row c at c * T + t, the voted arrays S rows of T
    rng = np.random.default_rng(5)
    r3 = vote_cases.random_records(rng, vote_cases.C, 3)
    p3 = vote_cases.present_of("random", rng, 3)
    v3, k3 = vote.select(r3, p3, vote_cases.OFFSETS, 3)
    for t in range(3):
        v1, k1 = vote.select(np.ascontiguousarray(r3[:, t:t + 1]), np.ascontiguousarray(p3[:, t:t + 1]), vote_cases.OFFSETS, 1)
        assert v1[:, 0].tobytes() == np.ascontiguousarray(v3[:, t]).tobytes() and k1[:, 0].tobytes() == np.ascontiguousarray(k3[:, t]).tobytes(), t
    with pytest.raises(ValueError, match=re.escape("stream 1: 33 candidates (offsets 1 .. 34), a group has 1 .. MBX_VOTE_MAX_CANDIDATES (32)")):
        vote.check_offsets([0, 1, 34])
    with pytest.raises(ValueError, match="stream 2: 0 candidates"):
        vote.check_offsets([0, 1, 2, 2])
    with pytest.raises(ValueError, match=r"cand_offset\[0\] is 0"):
        vote.check_offsets([1, 2])
    with pytest.raises(TypeError):
        vote.select(rec.astype(np.int64), None, off, 1)


def test_combine_on_known_answers():
    """V = 0 with disagreeing bits; 32 x {1, 255} saturating at 255; {1, 0} alone staying {1, 0}; identity ONE over random cells; a group
    with one present candidate equalling that candidate; nobody present: candidate 0's cells"""
    cells = 96
    off = np.array([0, 2, 34, 35, 36, 40, 43], dtype=np.int32)
    c = np.zeros((43, 1, cells, 2), dtype=np.uint8)
    present = np.ones((43, 1), dtype=np.uint8)
    c[0, 0, :, :] = (1, 77)      # group 0: {1, 77} against {0, 77}: V = 0, the bit of the lowest-index present candidate
    c[1, 0, :, :] = (0, 77)
    c[0, 0, 5] = (0, 10)         # ... cell 5 the other way round; cell 6: 10 against 77
    c[1, 0, 5] = (1, 10)
    c[0, 0, 6] = (1, 10)
    c[2:34, 0, :, :] = (1, 255)  # group 1: 32 x {1, 255}
    c[2:34, 0, 7] = (0, 255)
    c[34, 0, :, :] = (1, 0)      # group 2: {1, 0} alone
    rng = np.random.default_rng(9)
    c[35] = vote_cases.random_cells(rng, 1, 1, cells)[0]   # group 3: identity ONE
    c[36:40] = vote_cases.random_cells(rng, 4, 1, cells)   # group 4: only candidate 2 is there
    present[36:40, 0] = (0, 0, 9, 0)
    c[40:43] = vote_cases.random_cells(rng, 3, 1, cells)   # group 5: nobody
    present[40:43] = 0
    out, votes = vote.combine(c, present, off, 1)
    assert out.shape == (6, 1, cells, 2) and votes.shape == (6, 1)
    g0 = out[0, 0]
    assert (g0[np.r_[0:5, 7:cells]] == (1, 0)).all() and tuple(g0[5]) == (0, 0) and tuple(g0[6]) == (0, 67)
    assert (np.delete(out[1, 0], 7, axis=0) == (1, 255)).all() and tuple(out[1, 0, 7]) == (0, 255), "|V| = 8160 saturates at 255"
    assert (out[2, 0] == (1, 0)).all(), "{1, 0} alone stays {1, 0}"
    assert out[3, 0].tobytes() == c[35, 0].tobytes(), "ONE"
    assert out[4, 0].tobytes() == c[38, 0].tobytes(), "SOLE"
    assert out[5, 0].tobytes() == c[40, 0].tobytes(), "nobody present: candidate 0's cells"
    want = [(vote.COMBINED, 2, 255, 255, 0b11), (vote.COMBINED, 32, 255, 255, 2**32 - 1), (vote.COMBINED, 1, 255, 255, 1), (vote.COMBINED, 1, 255, 255, 1),
            (vote.COMBINED, 1, 255, 255, 0b100), (vote.NONE, 0, 255, 255, 0)]
    assert [tuple(int(x) for x in v) for v in votes[:, 0]] == want
    # the second candidate of group 0 alone (the first absent): its cells, whatever the absent one holds
    present[0] = 0
    out2, _ = vote.combine(c, present, off, 1)
    assert out2[0, 0].tobytes() == c[1, 0].tobytes()
    # SAME: n equal cells {b, r} give {b, min(255, n r)}
    same = np.zeros((3, 1, 184, 2), dtype=np.uint8)
    same[:, 0, :, 0] = np.arange(184) & 1
    same[:, 0, :, 1] = np.arange(184)
    out3, _ = vote.combine(same, None, [0, 3], 1)
    assert (out3[0, 0, :, 0] == (np.arange(184) & 1)).all() and (out3[0, 0, :, 1] == np.minimum(255, 3 * np.arange(184))).all()
    # identity ONE over every row length
    for n in vote.ROW_CELLS:
        one = vote_cases.random_cells(rng, 1, 3, n)
        assert vote.combine(one, None, [0, 1], 3)[0].tobytes() == one.tobytes(), n
    with pytest.raises(ValueError, match="row_cells is 184, 168 or 96"):
        vote.combine(np.zeros((1, 1, 72, 2), np.uint8), None, [0, 1], 1)


# ---- the library ------------------------------------------------------------------------------------------------------------------------------
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


def test_every_function_of_the_vote_header_is_exported_and_bound_in_a_table_of_its_own():
    import mbelib_neo_amd as m
    from mbelib_neo_amd import _native

    declared = _declared()
    assert list(declared) == FUNCTIONS
    assert tuple(declared) == _native.VOTE_SYMBOLS, "name for name, in the header's order"
    for other in (_native.EXPORTED_SYMBOLS, _native.BURST_SYMBOLS, _native.LLR_SYMBOLS, _native.GROUP_SYMBOLS, _native.KEYSTREAM_SYMBOLS, _native.PCM8_SYMBOLS,
                  _native.MIXDOWN_SYMBOLS, _native.LEVELS_SYMBOLS, _native.HOLD_SYMBOLS, _native.AGC_SYMBOLS, _native.LIMIT_SYMBOLS, _native.RESAMPLE_SYMBOLS,
                  _native.FILTER_SYMBOLS, _native.BANDS_SYMBOLS):
        assert not set(_native.VOTE_SYMBOLS) & set(other), "the headers keep their own symbol lists"
    text = open(HEADER).read()
    for name, value in (("MBX_VOTE_MAX_CANDIDATES", vote.MAX_CANDIDATES), ("MBX_VOTE_NONE", vote.NONE), ("MBX_VOTE_COMBINED", vote.COMBINED),
                        ("MBX_VOTE_SELECT", vote.SELECT), ("MBX_VOTE_COMBINE", vote.COMBINE)):
        assert int(re.search(rf"#define {name}\s+(0x[0-9A-Fa-f]+|\d+)\b", text).group(1), 0) == value, name
    assert (vote.MAX_CANDIDATES, vote.NONE, vote.COMBINED, vote.SELECT, vote.COMBINE) == (32, 0xFF, 0xFE, 0, 1)
    # the order of the header: conventions, the definition in integers, identities, the alignment table, then the calls
    places = [text.index(w) for w in ("Conventions are those of mbx.h", "Select: fewest errors", "Combine: soft input only", "Identities:", "Alignment, in the style of the table in mbx.h",
                                       "Workspace.", "#define MBX_VOTE_MAX_CANDIDATES", "int mbx_vote_plan_create")]
    assert places == sorted(places)
    for kind, align in (("cand records", 16), ("cand cells", 16), ("present", 1), ("vote records", 8)):
        assert re.search(rf"^ \*   {kind}\s+{align}\b", text, flags=re.M), kind
    for word in ("ONE", "SOLE", "SAME", "ORDER", "candidate 0's as it stands", "what a host with nothing better would feed the reference", "mbx_reserve_stream",
                 "before a device is asked for"):
        assert word in text, word
    # the other headers do not know the new calls: a header of its own
    for other in sorted(os.listdir(os.path.join(ROOT, "include"))):
        if other != "mbx_vote.h":
            theirs = open(os.path.join(ROOT, "include", other)).read()
            assert not any(f in theirs for f in FUNCTIONS) and "mbx_vote" not in theirs, other
    try:
        handle = C.CDLL(m.library_path())
    except OSError as e:
        pytest.skip(f"HIP runtime not loadable here: {e}")
    for name in declared:
        assert hasattr(handle, name), f"libmbx_hip.so does not export {name}"
    L = _lib()
    for name in declared:
        assert getattr(L, name).argtypes is not None and len(getattr(L, name).argtypes) == declared[name].count(",") + 1, name


@pytest.mark.parametrize("T", vote_cases.FRAMES)
@pytest.mark.parametrize("form", vote_cases.PRESENT_FORMS)
def test_the_host_functions_are_the_numpy_definition_byte_for_byte(T, form):
    """S = 5 groups of 1, 2, 3, 16 and 32 candidates, random records with ties and repeated words, and random cells of all three row
    lengths (the four codecs' shapes); the arrays between bytes that must stay"""
    L = _lib()
    rng = np.random.default_rng(100 * T + len(form))
    off, S, n_cand = vote_cases.OFFSETS, vote_cases.S, vote_cases.C
    present = vote_cases.present_of(form, rng, T)
    pp = present.ctypes.data if present is not None else None
    rec = vote_cases.random_records(rng, n_cand, T)
    want, want_votes = vote.select(rec, present, off, T)
    got = np.full((S * T + 2) * 16, 0x5A, dtype=np.uint8)
    got_votes = np.full((S * T + 2) * 8, 0x5A, dtype=np.uint8)
    assert L.mbx_vote_select_host(off.ctypes.data, S, T, rec.ctypes.data, pp, got[16:].ctypes.data, got_votes[8:].ctypes.data) == 0, L.mbx_last_error()
    assert got[16:-16].tobytes() == want.tobytes() and got_votes[8:-8].tobytes() == want_votes.tobytes()
    assert (got[:16] == 0x5A).all() and (got[-16:] == 0x5A).all() and (got_votes[:8] == 0x5A).all() and (got_votes[-8:] == 0x5A).all()
    again = np.zeros_like(want)
    assert L.mbx_vote_select_host(off.ctypes.data, S, T, rec.ctypes.data, pp, again.ctypes.data, None) == 0 and again.tobytes() == want.tobytes(), "votes are optional"
    if form == "stream-gone":
        assert (want_votes["winner"][3] == vote.NONE).all() and want[3].tobytes() == np.ascontiguousarray(rec[off[3]]).tobytes()
    for codec, cells in vote_cases.CELLS.items():
        c = vote_cases.random_cells(rng, n_cand, T, cells)
        want, want_votes = vote.combine(c, present, off, T)
        row = cells * 2
        got = np.full((S * T + 2) * row, 0x5A, dtype=np.uint8)
        got_votes = np.full((S * T + 2) * 8, 0x5A, dtype=np.uint8)
        assert L.mbx_vote_combine_host(off.ctypes.data, S, cells, T, c.ctypes.data, pp, got[row:].ctypes.data, got_votes[8:].ctypes.data) == 0, L.mbx_last_error()
        assert got[row:-row].tobytes() == want.tobytes() and got_votes[8:-8].tobytes() == want_votes.tobytes(), (codec, cells)
        assert (got[:row] == 0x5A).all() and (got[-row:] == 0x5A).all() and (got_votes[:8] == 0x5A).all() and (got_votes[-8:] == 0x5A).all()
        assert want[0].tobytes() == np.ascontiguousarray(c[0]).tobytes() or form == "random", "identity ONE: group 0 has one candidate"


def test_the_host_functions_on_the_crafted_records():
    L = _lib()
    rec, present, off, rows = vote_cases.crafted_select()
    want, want_votes = vote.select(rec, present, off, 1)
    got, got_votes = np.zeros_like(want), np.zeros_like(want_votes)
    assert L.mbx_vote_select_host(off.ctypes.data, 7, 1, rec.ctypes.data, present.ctypes.data, got.ctypes.data, got_votes.ctypes.data) == 0
    assert got.tobytes() == want.tobytes() and got_votes.tobytes() == want_votes.tobytes()


def test_every_refusal_comes_before_a_device_is_asked_for():
    """never dereferenced: every call below is refused first, on a host with no GPU as well.  What needs a plan (T, the size, the
    alignment and the overlap of a launch) is held through vote_select_refused / vote_combine_refused in vote_check.cpp and through the
    library in tests/test_gpu_vote.py."""
    L = _lib()

    def refused(fn, name, *args):
        assert L.mbx_stage_in(0x1008, 0x1000, 16, None) == INVALID and b"mbx_stage_in" in L.mbx_last_error()   # another call's text first
        assert fn(*args) == INVALID, args
        text = L.mbx_last_error()
        assert name + b":" in text, text
        return text

    good = vote_cases.OFFSETS
    create = lambda *a: refused(L.mbx_vote_plan_create, b"mbx_vote_plan_create", *a)   # noqa: E731
    h = C.c_void_p(0x1234)
    assert b"needed" in create(None, good.ctypes.data, 5) and b"needed" in create(C.byref(h), None, 5) and h.value is None
    for S in (0, -1):
        h = C.c_void_p(0x1234)
        assert b"S is at least 1" in create(C.byref(h), good.ctypes.data, S) and h.value is None
    bad = np.array([1, 2, 3], dtype=np.int32)
    assert b"cand_offset[0] is 0" in create(C.byref(h), bad.ctypes.data, 2)
    for offsets, text in (([0, 2, 2, 3], b"stream 1: 0 candidates (offsets 2 .. 2)"), ([0, 1, 34], b"stream 1: 33 candidates (offsets 1 .. 34)"),
                          ([0, 4, 3, 5], b"stream 1: -1 candidates (offsets 4 .. 3)"), ([0, 32, 64, 97], b"stream 2: 33 candidates")):
        a = np.array(offsets, dtype=np.int32)
        h = C.c_void_p(0x1234)
        assert text in create(C.byref(h), a.ctypes.data, len(offsets) - 1) and h.value is None, offsets
    assert L.mbx_vote_plan_destroy(None) == 0 and L.mbx_vote_plan_streams(None) == INVALID and L.mbx_vote_plan_candidates(None) == INVALID
    assert L.mbx_vote_workspace_frames(None, 0, 0, 1) == 0
    # the launchers and the whole steps without a plan: the pointers come first, whatever else is wrong
    for args in ((None, 1, 0x1000, None, 0x9000, None, None), (None, -1, 0x1008, 0x3, 0x1008, 0x4, None), (None, 0, None, None, None, None, None)):
        assert b"needed" in refused(L.mbx_vote_select, b"mbx_vote_select", *args)
    for args in ((None, 184, 1, 0x1000, None, 0x9000, None, None), (None, 7, -1, 0x1002, None, 0x1002, 0x4, None)):
        assert b"needed" in refused(L.mbx_vote_combine, b"mbx_vote_combine", *args)
    assert b"needed" in refused(L.mbx_process_batch_voted, b"mbx_process_batch_voted", None, 9, -1, None, 0x1001, None, 0x1000, None, 0x1000, None, None, None, 0x1008, 0x4, None)
    assert b"needed" in refused(L.mbx_process_batch_soft_voted, b"mbx_process_batch_soft_voted", None, 9, 7, -1, None, 0x1001, None, 0x1000, None, 0x1000, None, None, None,
                                0x1008, 0x4, None)
    # the host definitions: NULLs, S, the offsets, (row_cells,) T, the size -- one thing fewer wrong each time
    rec = np.zeros((54, 1, 4), dtype=np.uint32)
    out = np.zeros((5, 1, 4), dtype=np.uint32)
    sel = lambda *a: refused(L.mbx_vote_select_host, b"mbx_vote_select_host", *a)   # noqa: E731
    assert b"needed" in sel(None, 0, -1, None, None, None, None) and b"needed" in sel(good.ctypes.data, 0, -1, rec.ctypes.data, None, None, None)
    assert b"needed" in sel(None, 0, -1, rec.ctypes.data, None, out.ctypes.data, None)
    assert b"S is at least 1" in sel(bad.ctypes.data, 0, -1, rec.ctypes.data, None, out.ctypes.data, None)
    assert b"cand_offset[0] is 0" in sel(bad.ctypes.data, 2, -1, rec.ctypes.data, None, out.ctypes.data, None)
    big = np.array([0, 1, 34], dtype=np.int32)
    assert b"stream 1: 33 candidates" in sel(big.ctypes.data, 2, -1, rec.ctypes.data, None, out.ctypes.data, None)
    assert b"T is not negative" in sel(good.ctypes.data, 5, -1, rec.ctypes.data, None, out.ctypes.data, None)
    assert b"C * T is above 2^31-1" in sel(good.ctypes.data, 5, (2**31 - 1) // 54 + 1, rec.ctypes.data, None, out.ctypes.data, None)
    cells = np.zeros((54, 1, 96, 2), dtype=np.uint8)
    cout = np.zeros((5, 1, 96, 2), dtype=np.uint8)
    com = lambda *a: refused(L.mbx_vote_combine_host, b"mbx_vote_combine_host", *a)   # noqa: E731
    assert b"needed" in com(None, 0, 7, -1, None, None, None, None)
    assert b"S is at least 1" in com(good.ctypes.data, 0, 7, -1, cells.ctypes.data, None, cout.ctypes.data, None)
    assert b"stream 1: 33 candidates" in com(big.ctypes.data, 2, 7, -1, cells.ctypes.data, None, cout.ctypes.data, None)
    assert b"row_cells is 184, 168 or 96" in com(good.ctypes.data, 5, 7, -1, cells.ctypes.data, None, cout.ctypes.data, None)
    assert b"T is not negative" in com(good.ctypes.data, 5, 96, -1, cells.ctypes.data, None, cout.ctypes.data, None)
    assert b"C * T is above 2^31-1" in com(good.ctypes.data, 5, 96, 2**30, cells.ctypes.data, None, cout.ctypes.data, None)
    assert L.mbx_vote_combine_host(good.ctypes.data, 5, 96, 0, cells.ctypes.data, None, cout.ctypes.data, None) == 0, "T = 0: nothing to do"


def test_the_voted_forms_have_their_entry_in_the_launch_plan():
    """the voted steps are planned by plan_step (csrc/mbx_launch_plan.h), not by a code path of their own: the launcher asks it, and the
    unit that launches holds no decision of its own about expansion, instance or workspace"""
    plan = open(os.path.join(ROOT, "mbelib-neo_amd", "csrc", "mbx_launch_plan.h")).read()
    api = open(os.path.join(ROOT, "mbelib-neo_amd", "csrc", "mbx_api.hip")).read()
    for word in ("enum VoteKind { kNoVote, kSelectVote, kCombineVote }", "q.vote != kNoVote", "vote_offset", "front_frames"):
        assert word in plan, word
    body = api[api.index("static int process_batch_voted("):api.index("size_t mbx_vote_workspace_frames(")]
    assert "plan_of(c, q)" in body and "vp.workspace_frames" in body and "vp.vote_offset" in body and "vp.front_frames" in body
    for word in ("getenv", "kSmallBatchFrames", "lds_min_frames", "hipStreamCreate", "hipEventRecord", "hipStreamSynchronize", "hipDeviceSynchronize"):
        assert word not in body, word


# ---- the decoding experiment ----------------------------------------------------------------------------------------------------------------
def test_vote_and_combine_against_the_oracle():
    """Do the two rules help decoding?  200 clean voiced IMBE 7200x4400 frames (framegen, rng_for(2001)) heard by four sites of equal
    quality, every channel bit flipped with probability 0.02 per site (rng_for(2002)): the best single site's records differ from the
    clean ones in 39 of 200 frames, 19.5 %, inside the 10 - 50 % the experiment asks for (asserted below).  n(x) = frames whose parameter
    bits equal the clean ones, through the CPU oracle's FEC (the device's mbx_fec_host / mbx_fec_soft_host need a GPU: tests/test_gpu_vote.py
    repeats the chain through them).  Measured: hard sites 157, 150, 161, 158; select over their records 170; combine over the soft
    sites 200 of 200.  The chain asserted is n(combine) >= n(select) >= n(best single site), select and the single sites on hard
    records.
    A finding about the select rule, printed and not asserted: over the SOFT sites' records (167, 172, 169, 160 alone) select gives 166,
    below the best site.  The rule sees only the errors the FEC counts; the seven unprotected bits of a frame are wrong in 13 % of a
    site's frames at this rate, select cannot tell, and the soft FEC leaves few protected errors for it to avoid.  With sites of unequal
    quality (0.02 .. 0.05) select over hard records fell below the best site as well (146 against 161 at one draw)."""
    import oracle_lib

    o = oracle_lib.load()
    clean, hard, soft = vote_cases.sites()
    assert clean.shape == (200, 18) and hard.shape == (4, 200, 18) and soft.shape == (4, 200, 184, 2)
    clean_rec = o.fec_batch(0, clean)["w"]
    assert not (clean_rec[:, 3] & 0xFFFF).any(), "the clean frames decode without an error"
    off = np.array([0, 4], dtype=np.int32)
    hard_rec = np.stack([o.fec_batch(0, h)["w"] for h in hard]).astype(np.uint32)
    soft_rec = np.stack([o.fec_soft_batch(0, s)["w"] for s in soft]).astype(np.uint32)
    n_site = [vote_cases.same_parameters(r, clean_rec) for r in hard_rec]
    n_soft_site = [vote_cases.same_parameters(r, clean_rec) for r in soft_rec]
    voted, votes = vote.select(hard_rec, None, off, 200)
    n_select = vote_cases.same_parameters(voted, clean_rec)
    n_soft_select = vote_cases.same_parameters(vote.select(soft_rec, None, off, 200)[0], clean_rec)
    combined, _ = vote.combine(soft, None, off, 200)
    n_combine = vote_cases.same_parameters(o.fec_soft_batch(0, combined[0])["w"], clean_rec)
    print(f"hard sites {n_site} select {n_select} | soft sites {n_soft_site} select {n_soft_select} | combine {n_combine}")
    differ = 200 - max(n_site)
    assert 20 <= differ <= 100, f"the best single site differs in {differ} of 200 frames: 10 - 50 % is what the experiment asks for"
    assert (votes["present"] == 4).all() and (votes["winner"] < 4).all()
    assert n_combine >= n_select >= max(n_site), (n_combine, n_select, n_site)
