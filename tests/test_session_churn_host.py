"""Host test (no GPU): the scripts of tests/session_churn.py hold, in the ORACLE's decode, what tests/test_gpu_session_churn.py relies
on -- every submit form, every operation with both, one and none of its pointers, count = 0, the refusals, every listed range, an
operation of each kind directly behind a submit without a wait and one behind three submits in a row; around the operations the
frame classes that make a stale or wrongly cleared resident word audible (read from the oracle's result flags and parameter bits, not
from the script's intent); for the AMBE codecs migrated triplets with prev_mp_enhanced != cur_mp in front of a repeat or an invalid
tone; and, operation kind by operation kind, that the oracle's PCM of the affected streams leaves the PCM tolerance when that kind of
operation is skipped: a session that skipped it could not pass the GPU test.  The refusals' argument tuples are only listed here; they
run on the card."""
import numpy as np
import pytest

import parity
import session_churn as SC

CASES = [(codec, S) for codec in (0, 1, 2, 3) for S in SC.SIZES]


def _row(t, s):
    return int(s) if t.index is None else int(np.flatnonzero(t.index == s)[0])


def _around(sc, cls, mark):
    """(class of the last frame before the operation, class of the first one after it) of a mark's stream, in the oracle's decode"""
    _, _, s, ib, ia, _, _ = mark
    tb, ta = sc.ticks[ib], sc.ticks[ia]
    return str(cls[ib][_row(tb, s) * tb.T + tb.T - 1]), str(cls[ia][_row(ta, s) * ta.T])


@pytest.mark.parametrize("codec,S", CASES)
def test_the_script_holds_every_form_operation_range_and_timing(codec, S):
    sc = SC.script(codec, S)
    main = [t for t in sc.ticks if t.session == 0]
    assert 12 <= len(main) <= 16 and {t.form for t in main} == set(SC.FORMS) and sum(t.form == "keyed" for t in main) == 1
    assert {t.T for t in main} == {1, 3, 5}
    frames = sum(t.frames.shape[0] * t.T for t in sc.ticks)
    assert 2000 <= frames <= 12000, frames
    for t in main:
        n = t.frames.shape[0]
        if t.form == "indexed":
            assert n < S and (np.diff(t.index) > 0).all()
        if t.form == "indexed_perm":
            assert n < S and not (np.diff(t.index) > 0).all() and np.unique(t.index).size == n
        if t.form == "keyed":
            zero = ~t.rows.reshape(n, -1).any(axis=1)
            assert n == S and 0.4 <= zero.mean() <= 0.7 and t.rows[~np.repeat(zero, t.T)].any()
        if t.form == "soft_indexed":
            assert t.soft.shape[0] == n * t.T and set(np.unique(t.soft[:, :, 1]).tolist()) <= {0, 255} and t.soft[:, :, 0].max() <= 1
    # T = 1, 3 (below the LDS threshold of 4 frames) and 5 (above) as plain hard submits; S = 96 within the small-batch limit of 256, S = 320 above
    assert {(t.form, t.T) for t in main} >= {("submit", 1), ("submit", 3), ("submit", 5)}
    ops = [op for t in sc.ticks for op in t.ops] + list(sc.pre)
    have = {(op.kind, bool(op.state), bool(op.rng)) for op in ops if op.count > 0 and op.kind in ("get", "set")}
    assert have == {(k, a, b) for k in ("get", "set") for a, b in ((True, True), (True, False), (False, True))}, have
    assert {op.kind for op in ops if op.count > 0} >= {"reset", "seed", "streams"}
    assert {op.kind for op in ops if op.count == 0} == set(SC.KINDS)
    assert all(op.kind != "streams" or op.count == sc.sizes[op.session] for op in ops)
    # the refusals: first < 0, first + count > S, both pointers NULL, NULL seeds
    refused = [op for op in ops if op.kind == "refuse"]
    for fn in SC.KINDS:
        mine = [op for op in refused if op.buf == fn]
        assert any(op.first < 0 for op in mine) and any(op.first >= 0 and op.first + op.count > S for op in mine), fn
        if fn in ("get", "set"):
            assert any(0 <= op.first and op.first + op.count <= S and not op.state and not op.rng for op in mine), fn
        if fn == "seed":
            assert any(0 <= op.first and op.first + op.count <= S and not op.rng for op in mine)
    # every listed range is the range of an operation
    used = {(op.first, op.count) for op in ops if op.session == 0 and op.kind in SC.KINDS}
    assert used >= set(SC.ranges(S)), set(SC.ranges(S)) - used
    assert (61, 6) in used and (S <= 258 or (253, 6) in used)
    # an operation of each kind as the FIRST thing behind a submit, no wait; and one behind three submits in a row
    direct = {t.ops[0].kind for t in main if t.wait is False and t.ops and t.ops[0].count > 0}
    assert direct >= set(SC.KINDS), direct
    in_flight, busy = 0, False
    for t in main:
        in_flight += 1
        if t.wait is False and t.ops and t.ops[0].count > 0 and in_flight >= 3:
            busy = True
        if t.wait is not None:   # a wait, or an operation, which waits itself
            in_flight = 0
    assert busy, "no operation behind three submits in a row"
    # the guard of the byte checks: the whole-session get_state on both sides of the count = 0 calls and the refusals
    bracket = [t for t in main if any(op.buf == "whole0" for op in t.ops)][0]
    names = [op.buf for op in bracket.ops]
    inside = bracket.ops[names.index("whole0") + 1:names.index("whole1")]
    assert {op.kind for op in inside if op.count == 0} == set(SC.KINDS) and len([op for op in inside if op.kind == "refuse"]) == len(refused)


@pytest.mark.parametrize("codec,S", CASES)
def test_the_classes_around_the_operations_in_the_oracles_decode(codec, S):
    sc, ref = SC.script(codec, S), SC.reference(codec, S)
    cls = SC.classes(sc, ref)
    table = {}
    for mark in sc.marks:
        before, after = _around(sc, cls, mark)
        key = (mark[0], before, after)
        table[key] = table.get(key, 0) + 1
    print("COMPOSITION", f"codec {codec} S {S}:", {f"{k[0]} {k[1]}->{k[2]}": v for k, v in sorted(table.items())})
    for kind in SC.KINDS:
        after = {k[2] for k in table if k[0] == kind}
        assert "r" in after and "v" in after, f"{kind}: first frames after it are {after}"
    # seed: a stream whose next frame is random bits (unvoiced bands): the new noise generator shows -- asserted on the PCM below
    assert any(m[0] == "seed" and m[6] == "u" for m in sc.marks)
    # the destination of every set_state of a triplet decoded plain voice last: its word is set when the triplet arrives
    for mark in sc.marks:
        if mark[0] == "set" and mark[5] == "v":
            assert _around(sc, cls, mark)[0] == "v", mark
    gets = {op.buf: ref["gets"][(k, j)] for k, t in enumerate(sc.ticks) for j, op in enumerate(t.ops) if op.kind == "get" and op.count and (k, j) in ref["gets"]}
    moved = {"a": (gets["a"][0], SC.MIG_A, 0), "b": (gets["b"][0], SC.MIG_B, 0), "c": (sc.given["c"][0], SC.MIG_C_TO, 0)}
    if not SC.ambe(codec):
        # IMBE: no decoder-made state has prev_mp_enhanced != cur_mp (the module's docstring): what moves is elidable
        for name, (state, _, _) in moved.items():
            assert state[:, 2].tobytes() == state[:, 0].tobytes(), f"migration ({name}): an IMBE triplet with prev_mp_enhanced != cur_mp"
        return
    for name, (state, (first, count), session) in moved.items():
        differs = np.array([state[j, 2].tobytes() != state[j, 0].tobytes() for j in range(count)])
        if name == "c":
            tone_before = sc.given["c_classes"][:, -1] == "t"
            marks = [m for m in sc.marks if m[0] == "set" and m[1] == 0 and first <= m[2] < first + count]
        else:
            marks = [m for m in sc.marks if m[0] == "get" and m[1] == session and first <= m[2] < first + count]
            tone_before = np.array([_around(sc, cls, m)[0] == "t" for m in marks])
        assert len(marks) == count
        after = np.array([_around(sc, cls, m)[1] for m in marks])
        hit = differs & tone_before & np.isin(after, ("r", "i"))
        assert hit.any(), f"migration ({name}): no stream with a valid tone before, prev_mp_enhanced != cur_mp in the moved bytes, and a repeat or invalid tone next"
        # (only behind a valid tone, and not behind every one: what differs is the tone's running phase, which may be where the model's is)
        assert not (differs & ~tone_before).any(), f"migration ({name}): prev_mp_enhanced != cur_mp behind something else than a valid tone"
        flags = np.array([ref["ticks"][m[4]]["results"]["flags"][_row(sc.ticks[m[4]], m[2]) * sc.ticks[m[4]].T] for m in marks])
        assert ((flags[hit] & (0x40 | 0x10)) != 0).all(), f"migration ({name}): the frame after carries neither the repeat nor the tone flag"
        print("COMPOSITION", f"codec {codec} S {S} migration ({name}):", {"enh != cur": int(differs.sum()), "then r|i": int(hit.sum()), "of": count})


def _affected(sc, kind):
    """[(session, stream, first tick whose decode the operations of `kind` change)]"""
    out = []
    filled = {op.buf for t in sc.ticks for op in t.ops if op.kind == "get" and op.count}
    for k, t in enumerate(sc.ticks):
        for op in t.ops:
            if op.count <= 0 or op.buf in ("whole0", "whole1"):
                continue
            if op.kind == kind and kind != "get" or (kind == "get" and op.kind == "set" and op.buf in filled):
                out += [(op.session, op.first + j, k + 1) for j in range(op.count)]
    return out


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
@pytest.mark.parametrize("kind", SC.KINDS)
def test_the_oracle_with_one_kind_of_operation_left_out_leaves_the_pcm_tolerance(codec, kind):
    """S = 96.  get_state left out means that the caller's buffer keeps what it held (here: the defaults), so what is skipped shows in the
    streams a later set_state writes those bytes to"""
    S = SC.SIZES[0]
    sc, ref, without = SC.script(codec, S), SC.reference(codec, S), SC.reference(codec, S, leave_out=kind)
    streams = _affected(sc, kind)
    assert streams
    beyond, worst = 0, 0.0
    for session, s, first in streams:
        a = SC.stream_output(sc, ref["ticks"], "pcmf", session, s, first)
        b = SC.stream_output(sc, without["ticks"], "pcmf", session, s, first)
        total = parity.pcm_float_stats(a, b)[0]
        worst = max(worst, total)
        beyond += total > parity.PCM_REL_RMS
    print("COMPOSITION", f"codec {codec} without {kind}:", {"streams": len(streams), "beyond the PCM tolerance": int(beyond), "largest relative RMS": float(f"{worst:.3e}")})
    assert beyond >= 1
    if kind == "seed":   # ... and in particular on a stream whose next frames are random bits: within three frames (the noise buffer's delay)
        noisy = [(m[1], m[2], m[4]) for m in sc.marks if m[0] == "seed" and m[6] == "u"]
        assert any(parity.pcm_float_stats(SC.stream_output(sc, ref["ticks"], "pcmf", i, s, k)[:3], SC.stream_output(sc, without["ticks"], "pcmf", i, s, k)[:3])[0]
                   > parity.PCM_REL_RMS for i, s, k in noisy)
    # the streams no operation of the kind names are the same bytes: the reference applies an operation to its range alone
    named = {(i, s) for i, s, _ in streams} | {(op.session, op.first + j) for t in sc.ticks for op in t.ops
                                                  if op.kind in SC.KINDS and op.count < sc.sizes[op.session] for j in range(op.count)}
    for i, n in enumerate(sc.sizes):
        for s in range(n):
            if (i, s) not in named:
                assert SC.stream_output(sc, ref["ticks"], "pcm16", i, s).tobytes() == SC.stream_output(sc, without["ticks"], "pcm16", i, s).tobytes(), (i, s)


def test_two_generations_of_a_script_are_the_same_bytes():
    first = SC.script(3, 96)
    keep = [(t.frames.tobytes(), None if t.index is None else t.index.tobytes(), None if t.rows is None else t.rows.tobytes()) for t in first.ticks]
    SC.script.cache_clear()
    again = SC.script(3, 96)
    assert keep == [(t.frames.tobytes(), None if t.index is None else t.index.tobytes(), None if t.rows is None else t.rows.tobytes()) for t in again.ticks]
    assert first.given["c"][0].tobytes() == again.given["c"][0].tobytes() and first.marks == again.marks
    SC.reference.cache_clear()


def test_sources_and_destinations_of_the_migrations_are_fed_the_same_frames():
    for codec, S in CASES:
        sc = SC.script(codec, S)
        main = [k for k, t in enumerate(sc.ticks) if t.session == 0]
        set_a = [k for k in main if any(op.kind == "set" and op.buf == "a" and op.count for op in sc.ticks[k].ops)][0]
        set_b = [k for k in main if any(op.kind == "set" and op.buf == "b" for op in sc.ticks[k].ops)][0]
        for k in main:
            t = sc.ticks[k]
            if k > set_a:
                for j in range(SC.MIG_A[1]):
                    assert np.array_equal(t.frames[_row(t, SC.MIG_A[0] + j)], t.frames[_row(t, SC.MIG_A_TO[0] + j)])
            if k > set_b:
                side = sc.ticks[k + 1]
                assert side.session == 1 and side.T == t.T and (side.form == "soft_indexed") == (t.form == "soft_indexed")
                for j in range(SC.MIG_B[1]):
                    assert np.array_equal(t.frames[_row(t, SC.MIG_B[0] + j)], side.frames[SC.MIG_B_TO[0] + j])
                    if t.form == "keyed":
                        assert not t.rows[(SC.MIG_B[0] + j) * t.T:(SC.MIG_B[0] + j + 1) * t.T].any()
        # no later operation names a source or a destination alone (the whole-session reads aside)
        later = [op for k in main if k > set_b for op in sc.ticks[k].ops if op.kind in SC.KINDS and op.count and op.count < S]
        moved = set(range(5, 12)) | set(range(20, 27)) | set(range(61, 67))
        assert all(not (set(range(op.first, op.first + op.count)) & moved) for op in later)
