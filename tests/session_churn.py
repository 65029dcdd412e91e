"""Channel churn in sessions (include/mbx.h "sessions"): a scripted run of submits with the four state functions between them --
mbx_session_reset, mbx_session_seed, mbx_session_get_state, mbx_session_set_state -- and its two references.

`script(codec, S)` is a list of TICKS over two sessions of one codec (session 0: S streams; session 1: SIDE streams, the far end of a
migration).  A tick is a submit form (mbx_session_submit, _submit_indexed with a sorted or a permuted subset, _submit_soft_indexed with
cells made from the hard frames at full reliability, _submit_keyed once: an all-zero keystream on half the rows -- the streams with a
scripted frame there and the migrated ones among them --, a random one on the rest), its batch (streams, T in {1, 3, 5}, frames), and
the state operations between that submit and the next -- issued with or without an mbx_session_wait first, and once behind three
submits in a row, which is every pipeline slot busy.  A seed is audible only behind a reset (the unvoiced noise takes a new seed up
when the stream's noise state is next initialised, as in the reference), so the seeds that must show follow a reset of their range.
The operations cover every function with both, one and none of its two pointers, count = 0, the refusals, and the ranges (0, 1),
(S - 1, 1), (5, 7), (61, 6) across slot 64, (253, 6) across the small-batch limit when S allows, and the whole session.

Three MIGRATIONS make the bookkeeping of the resident words observable: (a) get_state of streams 5..11, set_state of those bytes into
20..26 of the same session; (b) get_state of 61..66, set_state into 3..8 of session 1; (c) triplets and noise generators the ORACLE
left after three frames, set into 30..37.  From then on source and destination are fed the same frames, so their PCM, results and
final state must be the same bytes.

What stands around an operation is scripted, because a stale or wrongly cleared word only shows in a frame that reads
prev_mp_enhanced, and only when that struct differs from cur_mp: per affected stream j of a range, the last frame before the
operation and the first one after it follow BEFORE[j % 4] and AFTER[j % 4] -- a valid tone before (the one decoder-made state with
prev_mp_enhanced != cur_mp: mbx_stream.hip, keeps_enh) and a repeat or an invalid tone after (which replay prev_mp_enhanced whole),
voice before and after, and random bits after (unvoiced bands: a new noise generator shows).  The destination of a migration has
plain voice as its own last frame, so its word is set when set_state arrives.  For the IMBE codecs no decoder-made state has
prev_mp_enhanced != cur_mp: there the tone and invalid-tone places hold voice and repeats, the clear of the words is not observable
through decoder-made states, and what these scripts hold the IMBE sessions to is the ranges, the waits and the noise generators.
States no decoder can produce are tests/model_lattice.py's.

`reference(codec, S)` is the ORACLE's decode of the script, tick by tick on host arrays, every operation plain numpy on them (reset =
Oracle.init_state and rng_default rows, seed = rng_seeded rows, get / set = row copies, indexed ticks gather and scatter);
`reference(codec, S, leave_out=kind)` is the same with every operation of one kind skipped (tests/test_session_churn_host.py: a session
that skipped it could not pass).  `run_twin` is the HIP twin without sessions: BatchDecoders on ABI triplets, the operations as
state_numpy(), a numpy edit, set_state().  `run_session` drives real sessions; `python tests/session_churn.py <codec> <S> <out.npz>`
does that in a process of its own (for MBX_SESSION_ABI_STATE, which the library reads when a session is created) and keeps every array.
Test infrastructure: the script and the oracle's decode need no GPU; nothing in the package uses this module."""
import ctypes as C
import functools
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from mbelib_neo_amd import framegen  # noqa: E402
from mbelib_neo_amd.layout import FRAME_BYTES, PARAM_BITS, PARMS_DTYPE, RECORD_DTYPE, RESULT_DTYPE, RNG_DTYPE  # noqa: E402

SIZES = (96, 320)
SIDE = 24                      # streams of session 1
INVALID = -1                   # MBE_STATUS_INVALID_ARGUMENT
FORMS = ("submit", "indexed", "indexed_perm", "soft_indexed", "keyed")
KINDS = ("reset", "seed", "get", "set")
BEFORE = {True: "tvtv", False: "vvvv"}     # by j % 4 of a range: AMBE, IMBE
AFTER = {True: "rviu", False: "rvru"}
MIG_A, MIG_A_TO = (5, 7), (20, 7)
MIG_B, MIG_B_TO = (61, 6), (3, 6)
MIG_C_TO, MIG_C_FRAMES = (30, 8), 3
GUARD = 0xA5                   # what get_state buffers and outputs hold before a call

# session: 0 | 1.  form: one of FORMS.  index: int32 [n] or None (every stream).  frames: uint8 [n, T, bytes].  soft: uint8 [n * T, cells, 2]
# or None.  rows: keystream rows uint8 [n * T, 12] or None.  wait: True = mbx_session_wait before the operations, False = none (the
# first operation must complete the submit), None = no operations: the next submit follows at once.  ops: [Op].
Tick = namedtuple("Tick", "session form T index frames soft rows wait ops")
# kind: reset | seed | get | set | streams | refuse.  buf: get: the name the bytes are kept under; set: the name they are taken from;
# refuse: the function refused.  state / rng: whether that pointer is passed (seed, and refuse of seed: rng = the seeds pointer).
# seeds: uint32 [count] of a seed.
Op = namedtuple("Op", "kind session first count buf state rng seeds")
Op.__new__.__defaults__ = (None, True, True, None)
# marks: (kind, session, stream, tick before or None, tick after or None, scripted class before, scripted class after)
Script = namedtuple("Script", "codec S sizes seeds pre ticks given marks special")


def ambe(codec):
    return codec in (1, 3)


def ranges(S):
    """the ranges the issue of this lattice lists; every one is the range of some operation (test_session_churn_host)"""
    return [(0, 1), (S - 1, 1), (5, 7), (61, 6)] + ([(253, 6)] if S > 258 else []) + [(0, S)]


# ---- frames of a class ------------------------------------------------------------------------------------------------------------------
def class_frames(codec, letters, rng):
    """clean wire frames [n, bytes]: 'v' voice, 'r' a frame the decoder answers with a repeat, 't' a valid tone, 'i' a tone signature with
    an id that leaves the model alone, 'u' random bits.  (edge_mix's builders; the 2400 tone bits of pitch_lattice; IMBE 7100x4400
    through tests/imbe7100_frames.py, so that its voice is voice and its repeats are certain: an invalid fundamental.)"""
    import edge_mix
    import pitch_lattice

    letters = np.array(list(letters))
    out = np.zeros((len(letters), FRAME_BYTES[codec]), dtype=np.uint8)
    for c in sorted(set(letters.tolist())):
        at = np.flatnonzero(letters == c)
        n = at.size
        if c == "u":
            out[at] = framegen.random_frames(codec, n, rng)
        elif codec == 2:
            import imbe7100_frames
            import oracle_lib

            bits = framegen.imbe_voiced_param_bits(n, rng)
            if c == "r":
                pitch_lattice._set_b0(2, bits, rng.integers(208, 256, size=n))
            out[at] = imbe7100_frames.encode_imbe7100x4400(bits, oracle_lib.load())
        elif c == "v":
            out[at] = edge_mix._voice(codec, n, rng)
        elif c == "r":
            out[at] = edge_mix._uncorrectable(codec, n, rng)
        elif codec == 1:
            out[at] = edge_mix._ambe_class_frames([c] * n, rng)
        else:
            assert codec == 3 and c in "ti", (codec, c)
            bits = rng.integers(0, 2, size=(n, 49), dtype=np.uint8)
            pitch_lattice._tone_bits_2400(bits, rng.integers(7, 123, size=n) if c == "t" else rng.choice([128, 130, 161, 163], size=n))
            out[at] = framegen.encode_ambe3600x2450(bits)
    return out


def soft_cells(codec, packed):
    """mbe_soft_bit cells [n, cells, 2] of hard frames at full reliability (tests/soft_mix.py: cells_from_packed, script 2)"""
    import soft_mix

    hard, used = soft_mix.cells_from_packed(codec, packed)
    rel = np.where(used[None, :], 255, 0).astype(np.uint8) * np.ones_like(hard)
    return np.ascontiguousarray(np.stack([hard * used[None, :], rel], axis=-1).astype(np.uint8))


# ---- the plan: forms, T, waits and operations ------------------------------------------------------------------------------------------
def _plan(S):
    o = Op
    across = [(253, 6)] if S > 258 else []
    seeds = lambda first, count, tag: (np.arange(count) * 7 + 1000 * tag + first + 1).astype(np.uint32)   # noqa: E731
    count0 = [o("reset", 0, 7, 0), o("seed", 0, 7, 0, seeds=seeds(7, 1, 9)), o("get", 0, 7, 0, "zero"), o("set", 0, 7, 0, "a"),
              o("reset", 0, S, 0), o("get", 0, S, 0, "zero", True, False), o("set", 0, S, 0, "a", False, True)]
    refusals = [o("refuse", 0, -1, 1, "reset"), o("refuse", 0, S - 1, 2, "reset"), o("refuse", 0, S, 1, "reset"),
                o("refuse", 0, -1, 1, "seed"), o("refuse", 0, S - 3, 4, "seed"), o("refuse", 0, 0, 1, "seed", rng=False),
                o("refuse", 0, -1, 1, "get"), o("refuse", 0, 0, S + 1, "get"), o("refuse", 0, 0, 1, "get", False, False),
                o("refuse", 0, -2, 2, "set"), o("refuse", 0, S - 5, 6, "set"), o("refuse", 0, 0, 1, "set", False, False)]
    return [
        ("submit", 1, False, [o("reset", 0, 0, 1), o("reset", 0, *MIG_B)] + [o("reset", 0, *r) for r in across]),
        # (a new seed of the unvoiced noise is taken up when the stream's noise state is next initialised: the seeds behind a reset are the audible ones)
        ("indexed", 3, False, [o("seed", 0, S - 1, 1, seeds=seeds(S - 1, 1, 1)), o("reset", 0, *MIG_A), o("seed", 0, *MIG_A, seeds=seeds(5, 7, 2))]),
        ("soft_indexed", 3, False, [o("get", 0, *MIG_A, "a"), o("set", 0, *MIG_A_TO, "a")]),                     # migration (a)
        ("indexed_perm", 5, None, []),
        ("submit", 1, None, []),
        ("submit", 3, False, [o("get", 0, *MIG_B, "b"), o("set", 1, *MIG_B_TO, "b")]),                           # (b), every slot busy
        ("soft_indexed", 1, True, [o("set", 0, *MIG_C_TO, "c")]),                                                # (c)
        ("keyed", 3, True, [o("get", 0, 12, 4, "rewind"), o("get", 0, 0, 1, "model", True, False), o("get", 0, S - 1, 1, "noise", False, True)]),
        ("indexed", 3, False, [o("set", 0, 12, 4, "rewind", True, False), o("set", 0, 16, 4, "rewind", False, True)]),
        ("soft_indexed", 1, True,[o("get", 0, 0, S, "whole0")] + count0 + refusals + [o("streams", 0, 0, S), o("get", 0, 0, S, "whole1")]),
        ("indexed_perm", 5, False, [o("reset", 0, S - 1, 1), o("seed", 0, S - 1, 1, seeds=seeds(S - 1, 1, 5)), o("seed", 0, 0, 1, seeds=seeds(0, 1, 3))] + [o("get", 0, *r, "across") for r in across]),
        ("submit", 1, False, [o("seed", 0, 40, 6, seeds=seeds(40, 6, 4)), o("reset", 0, 46, 4), o("seed", 0, 46, 4, seeds=seeds(46, 4, 6))]),
        ("indexed", 3, True, [o("get", 0, 50, 4, "late"), o("set", 0, 54, 4, "late")]),
        ("submit", 5, None, []),
    ]


def _marked(op):
    """operations whose neighbouring frames are scripted: every one on a part of a session"""
    return op.kind in KINDS and op.count > 0 and not op.buf in ("whole0", "whole1")


@functools.lru_cache(maxsize=None)
def script(codec, S):
    """the script of (codec, S): a Script.  Deterministic; cached -- read it, never write to it."""
    import oracle_lib

    assert S in SIZES and codec in (0, 1, 2, 3)
    rng = framegen.rng_for(0x5E550000 + 16 * S + codec)
    fb = FRAME_BYTES[codec]
    plan = _plan(S)
    sizes = (S, SIDE)
    special = sorted({s for _, _, _, ops in plan for op in ops if _marked(op) and op.session == 0 for s in range(op.first, op.first + op.count)})
    special = np.array(special, dtype=np.int32)
    rest = np.setdiff1d(np.arange(S, dtype=np.int32), special)
    # ---- the ticks of both sessions, frames still plain: the streams an operation names carry voice, of the others every third random bits
    ticks, mirror = [], {}
    first_b = [k for k, (_, _, _, ops) in enumerate(plan) if any(op.buf == "b" and op.kind == "set" for op in ops)][0]

    def plain(streams, T, named):
        letters = ["v" if (s in named or s % 3) else "u" for s in streams for _ in range(T)]
        return class_frames(codec, letters, rng).reshape(len(streams), T, fb)

    named0, named1 = set(special.tolist()), set(range(SIDE))
    for k, (form, T, wait, ops) in enumerate(plan):
        index = None
        if form in ("indexed", "indexed_perm", "soft_indexed"):
            some = rng.permutation(rest)[: len(rest) // 2]
            index = np.concatenate([special, some]).astype(np.int32)
            index = rng.permutation(index).astype(np.int32) if form == "indexed_perm" else np.sort(index)
        streams = np.arange(S) if index is None else index
        ticks.append(dict(session=0, form=form, T=T, index=index, frames=plain(streams, T, named0), wait=wait, ops=list(ops), k=k))
        if k == 0 or k > first_b:   # session 1: one tick of voice before migration (b), then a twin of every tick of session 0
            side = "soft_indexed" if form == "soft_indexed" else "submit"
            ticks.append(dict(session=1, form=side, T=T, index=np.arange(SIDE, dtype=np.int32) if side == "soft_indexed" else None,
                              frames=plain(np.arange(SIDE), T, named1), wait=True if k == 0 else None, ops=[], k=k))
            mirror[k] = len(ticks) - 1
    of_plan = {t["k"]: i for i, t in enumerate(ticks) if t["session"] == 0}

    def row(t, s):
        return int(s) if t["index"] is None else int(np.flatnonzero(t["index"] == s)[0])

    # ---- the classes around the operations
    marks = []
    tone = ambe(codec)
    for k, (_, _, _, ops) in enumerate(plan):
        for op in ops:
            if not _marked(op):
                continue
            dest = op.kind == "set" and op.state   # its own last frame is voice: the word of the slot is set when the triplet arrives
            for j in range(op.count):
                s = op.first + j
                if op.session == 1:
                    before, after = ticks[mirror[0]], ticks[mirror[k + 1]]
                    ib, ia = mirror[0], mirror[k + 1]
                else:
                    ib, ia = of_plan[k], of_plan[k + 1]
                    before, after = ticks[ib], ticks[ia]
                cb = "v" if dest or op.kind in ("reset", "seed") else BEFORE[tone][j % 4]
                ca = AFTER[tone][j % 4]
                before["frames"][row(before, s), -1] = class_frames(codec, cb, rng)[0]
                after["frames"][row(after, s), 0] = class_frames(codec, ca, rng)[0]
                if ca == "u" and op.kind == "seed":   # (the noise of a newly seeded generator reaches the PCM a frame or two later: random bits throughout)
                    after["frames"][row(after, s)] = class_frames(codec, "u" * after["T"], rng)
                marks.append((op.kind, op.session, s, ib, ia, cb, ca))
    # ---- what the oracle alone decoded, for migration (c): three frames, the last one by BEFORE
    o = oracle_lib.load()
    n_c = MIG_C_TO[1]
    letters = [("vv" + BEFORE[tone][j % 4])[f] for j in range(n_c) for f in range(MIG_C_FRAMES)]
    cpu_frames = class_frames(codec, letters, rng)
    cpu = o.process_batch(codec, n_c, MIG_C_FRAMES, cpu_frames, o.init_state(n_c), o.rng_seeded(np.arange(n_c) + 900))
    given = {"c": (cpu["state"], cpu["rng"]), "c_frames": cpu_frames.reshape(n_c, MIG_C_FRAMES, fb),
             "c_classes": _classes_of(codec, cpu).reshape(n_c, MIG_C_FRAMES)}
    # ---- source and destination of (a) and (b) are fed the same frames from the migration on
    first_a = [k for k, (_, _, _, ops) in enumerate(plan) if any(op.buf == "a" and op.kind == "set" and op.count for op in ops)][0]
    for k in range(len(plan)):
        t = ticks[of_plan[k]]
        if k > first_a:
            for j in range(MIG_A[1]):
                t["frames"][row(t, MIG_A_TO[0] + j)] = t["frames"][row(t, MIG_A[0] + j)]
        if k > first_b:
            for j in range(MIG_B[1]):
                ticks[mirror[k]]["frames"][MIG_B_TO[0] + j] = t["frames"][row(t, MIG_B[0] + j)]
    # ---- soft cells and the keystream
    out = []
    for t in ticks:
        n, T = t["frames"].shape[:2]
        soft = soft_cells(codec, t["frames"].reshape(n * T, fb)) if t["form"] == "soft_indexed" else None
        rows = None
        if t["form"] == "keyed":
            import keystream_cases

            rows = keystream_cases.random_rows(n * T, rng).reshape(n, T, -1)
            at = len(out)   # no keystream on half the rows: the streams with a scripted frame here, the migrated ones, then the lowest others
            clear = {m[2] for m in marks if m[1] == 0 and at in (m[3], m[4])}
            for first, count in (MIG_A, MIG_A_TO, MIG_B):
                clear |= set(range(first, first + count))
            assert len(clear) <= n // 2
            clear |= set([s for s in range(n) if s not in clear][: n // 2 - len(clear)])
            rows[sorted(clear)] = 0
            rows = np.ascontiguousarray(rows.reshape(n * T, -1))
        frames = np.ascontiguousarray(t["frames"])
        frames.setflags(write=False)
        out.append(Tick(t["session"], t["form"], T, t["index"], frames, soft, rows, t["wait"], tuple(t["ops"])))
    seeds = tuple((np.arange(n) * 5 + 4321 + 77 * i).astype(np.uint32) for i, n in enumerate(sizes))
    pre = tuple(x for i, n in enumerate(sizes) for x in (Op("streams", i, 0, n), Op("seed", i, 0, n, seeds=seeds[i])))
    return Script(codec, S, sizes, seeds, pre, tuple(out), given, tuple(marks), special)


def instance_names(L, sc):
    """mbx_batch_kernel_name(codec, n, T, resident) of every hard, unkeyed tick of session 0: {(form, n, T): name}"""
    out = {}
    for t in sc.ticks:
        if t.session == 0 and t.form in ("submit", "indexed", "indexed_perm"):
            n = t.frames.shape[0]
            out[(t.form, n, t.T)] = (L.mbx_batch_kernel_name(sc.codec, n, t.T, 1) or b"").decode()
    return out


# ---- reference 1: the oracle -------------------------------------------------------------------------------------------------------------
def _rows_of(op):
    return slice(op.first, op.first + op.count)


def _apply_numpy(op, st, rg, bufs, init_state, rng_default, rng_seeded, skip=None):
    """one operation on host arrays st [n, 3], rg [n] of its session; get keeps (state rows or None, rng rows or None) in bufs"""
    if op.kind == skip or op.kind in ("streams", "refuse") or op.count == 0:
        return
    r = _rows_of(op)
    if op.kind == "reset":
        st[r], rg[r] = init_state(op.count), rng_default(op.count)
    elif op.kind == "seed":
        rg[r] = rng_seeded(op.seeds)
    elif op.kind == "get":
        bufs[op.buf] = (st[r].copy() if op.state else None, rg[r].copy() if op.rng else None)
    else:
        have = bufs.get(op.buf)
        state, rng = have if have is not None else (None, None)
        if op.state:
            st[r] = state[: op.count] if state is not None else init_state(op.count)   # (a get_state that was skipped left the caller's buffer as it was)
        if op.rng:
            rg[r] = rng[: op.count] if rng is not None else rng_default(op.count)


@functools.lru_cache(maxsize=6)
def reference(codec, S, leave_out=None):
    """the oracle's decode of script(codec, S): {"ticks": [Oracle.process_batch's dict per tick, rows in the tick's order], "gets": {(tick,
    op number): (state rows, rng rows)}, "state": [per session], "rng": [per session]}.  leave_out: a kind of KINDS that is skipped."""
    import keyed_reference
    import oracle_lib

    o = oracle_lib.load()
    sc = script(codec, S)
    st = [o.init_state(n) for n in sc.sizes]
    rg = [o.rng_default(n) for n in sc.sizes]
    bufs = {"c": sc.given["c"]}
    gets, ticks = {}, []
    for op in sc.pre:
        _apply_numpy(op, st[op.session], rg[op.session], bufs, o.init_state, o.rng_default, o.rng_seeded)
    for k, t in enumerate(sc.ticks):
        i = t.session
        idx = np.arange(sc.sizes[i]) if t.index is None else t.index
        n = len(idx)
        if t.form == "keyed":
            ref = keyed_reference.process_batch_keyed(o, codec, n, t.T, t.frames.reshape(n * t.T, -1), t.rows, st[i][idx], rg[i][idx])
            # (the per-frame reference calls report no pre-clip peak: the largest reference sample stands in, never a wider bound than the
            # true peak's -- tests/test_gpu_keystream.py)
            ref["peak"] = np.abs(ref["pcmf"]).max(axis=1)
        else:
            ref = o.process_batch(codec, n, t.T, t.soft if t.soft is not None else t.frames.reshape(n * t.T, -1), st[i][idx], rg[i][idx], soft=t.soft is not None)
        st[i][idx], rg[i][idx] = ref["state"], ref["rng"]
        ticks.append(ref)
        for j, op in enumerate(t.ops):
            _apply_numpy(op, st[op.session], rg[op.session], bufs, o.init_state, o.rng_default, o.rng_seeded, skip=leave_out)
            if op.kind == "get" and op.count and op.kind != leave_out:
                gets[(k, j)] = bufs[op.buf]
    return {"ticks": ticks, "gets": gets, "state": st, "rng": rg}


def stream_rows(sc, session, stream, first_tick=0):
    """[(tick, first row of the stream's frames in the tick's outputs, T)] of one stream, from tick `first_tick` on"""
    out = []
    for k, t in enumerate(sc.ticks):
        if k < first_tick or t.session != session:
            continue
        at = np.flatnonzero(t.index == stream) if t.index is not None else np.array([stream])
        if at.size:
            out.append((k, int(at[0]) * t.T, t.T))
    return out


def stream_output(sc, outs, key, session, stream, first_tick=0):
    """the rows of one stream in outs[tick][key], in time order, from tick `first_tick` on"""
    return np.concatenate([outs[k][key][a:a + T] for k, a, T in stream_rows(sc, session, stream, first_tick)])


def _classes_of(codec, decoded):
    """the class of every frame of one Oracle.process_batch result, from its result flags and parameter bits: 'v', 'r', and for the AMBE
    codecs 't', 'i', 'e', 's' (pitch_lattice._ambe_classes)"""
    import oracle_lib
    import pitch_lattice

    flags = decoded["results"]["flags"]
    if ambe(codec):
        return pitch_lattice._ambe_classes(codec, oracle_lib.records_to_bits(decoded["records"], PARAM_BITS[codec]), flags)
    return np.where((flags & pitch_lattice.FLAG_REPEAT) != 0, "r", "v")


def classes(sc, ref):
    """per tick, the class of every frame in the oracle's decode of the script"""
    return [_classes_of(sc.codec, r) for r in ref["ticks"]]


# ---- reference 2: the HIP twin without sessions -----------------------------------------------------------------------------------------------
def _tick_outputs(n, T, records):
    nf = n * T
    o = {"pcm16": np.zeros((nf, 160), np.int16), "pcmf": np.zeros((nf, 160), np.float32), "results": np.zeros(nf, RESULT_DTYPE)}
    if records:
        o["records"] = np.zeros(nf, RECORD_DTYPE)
    for x in o.values():
        x.view(np.uint8).fill(GUARD)
    return o


def run_twin(sc):
    """the script through BatchDecoders on ABI triplets (resident=False), the operations as state_numpy(), a numpy edit, set_state():
    {"ticks": [dict of host arrays per tick], "gets": {(tick, op): (state rows, rng rows)}, "state", "rng": per session}"""
    import torch

    from mbelib_neo_amd import _native, decoder, layout

    L = _native.lib()
    dec = [decoder.BatchDecoder(sc.codec, n) for n in sc.sizes]
    bufs = {"c": sc.given["c"]}
    gets, ticks = {}, []

    def apply(op):
        d = dec[op.session]
        st, rg = d.state_numpy().copy(), d.rng_numpy().copy()
        _apply_numpy(op, st, rg, bufs, layout.init_state, layout.rng_default, layout.rng_seeded)
        d.set_state(st, rg)

    for op in sc.pre:
        apply(op)
    for k, t in enumerate(sc.ticks):
        d = dec[t.session]
        n = t.frames.shape[0]
        frames = np.array(t.frames, copy=True).reshape(-1)
        d_index = None if t.index is None else torch.from_numpy(t.index).to(d.device)
        if t.form == "soft_indexed":
            out = d.decode_soft(t.soft, t.T, want_float=True, stream_index=d_index)
        elif t.form == "keyed":
            out = d.decode(frames, t.T, want_float=True, keystream=t.rows)
        elif t.index is None:
            out = d.decode(frames, t.T, want_float=True)
        else:
            out = d.make_outputs(t.T, True, True, True, streams=n)
            d_frames = d.to_device(frames)
            _native.check(L.mbx_process_batch_indexed(sc.codec, n, t.T, d_index.data_ptr(), d_frames.data_ptr(), d.state.data_ptr(), d.rng.data_ptr(),
                                                      out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(),
                                                      torch.cuda.current_stream().cuda_stream), "mbx_process_batch_indexed")
        torch.cuda.synchronize()
        ticks.append({"pcm16": out["pcm16"].cpu().numpy(), "pcmf": out["pcmf"].cpu().numpy(), "results": decoder.results_numpy(out["results"]),
                      "records": decoder.records_numpy(out["records"])})
        for j, op in enumerate(t.ops):
            apply(op)
            if op.kind == "get" and op.count:
                gets[(k, j)] = bufs[op.buf]
    return {"ticks": ticks, "gets": gets, "state": [d.state_numpy().copy() for d in dec], "rng": [d.rng_numpy().copy() for d in dec]}


# ---- the sessions themselves ---------------------------------------------------------------------------------------------------------------
def _call_op(L, h, op, bufs, sizes):
    """one operation on a session; returns (status, what a get returned or None).  A get writes into buffers one row longer than count,
    pre-filled with GUARD; a set reads the bytes an earlier get of THIS run returned."""
    if op.kind == "streams":
        return (0 if L.mbx_session_streams(h) == op.count else -99), None
    if op.kind == "reset" or (op.kind == "refuse" and op.buf == "reset"):
        return L.mbx_session_reset(h, op.first, op.count), None
    if op.kind == "seed" or (op.kind == "refuse" and op.buf == "seed"):
        seeds = op.seeds if op.seeds is not None else np.arange(max(op.count, 1), dtype=np.uint32)
        return L.mbx_session_seed(h, op.first, op.count, seeds.ctypes.data if op.rng else None), None
    rows = max(op.count, 0) + 1
    if op.kind == "get" or (op.kind == "refuse" and op.buf == "get"):
        st, rg = np.zeros((rows, 3), PARMS_DTYPE), np.zeros(rows, RNG_DTYPE)
        st.view(np.uint8).fill(GUARD)
        rg.view(np.uint8).fill(GUARD)
        rc = L.mbx_session_get_state(h, op.first, op.count, st.ctypes.data if op.state else None, rg.ctypes.data if op.rng else None)
        return rc, (st, rg)
    if op.kind == "refuse":   # set: valid pointers of the right size, so that only the arguments can be the reason
        st, rg = np.zeros((rows, 3), PARMS_DTYPE), np.zeros(rows, RNG_DTYPE)
    else:
        st, rg = (None if x is None else np.ascontiguousarray(x[: max(op.count, 1)]) for x in bufs[op.buf])
    assert (st is not None or not op.state) and (rg is not None or not op.rng), op
    return L.mbx_session_set_state(h, op.first, op.count, st.ctypes.data if op.state else None, rg.ctypes.data if op.rng else None), None


def run_session(sc, log=None):
    """the script through two real sessions created with all three outputs, inputs and outputs in pageable memory.  Outputs are copied
    the moment the first operation behind a submit returns (or, with no operation, after the next wait): a submit the operation did
    not complete leaves GUARD bytes there.  Returns {"ticks": [...], "gets": {(tick, op): (state [count + 1, 3], rng [count + 1])},
    "status": {(tick, op): return value}, "state", "rng": per session, "wait", "destroy": return values}"""
    from mbelib_neo_amd import _native, decoder

    decoder.ensure_init(0)
    L = _native.lib()
    hs = []
    for n in sc.sizes:
        h = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(h), sc.codec, n, n * 5, 1 | 2 | 4), "mbx_session_create")
        hs.append(h)
    bufs = {"c": sc.given["c"]}
    gets, status, ticks, live, keep = {}, {}, [None] * len(sc.ticks), [], []
    try:
        def collect(session):   # every submit of the session so far must be complete now: take its outputs as they are
            for item in [x for x in live if x[0] == session]:
                ticks[item[1]] = {k: v.copy() for k, v in item[2].items()}
                live.remove(item)

        for j, op in enumerate(sc.pre):
            status[(-1, j)] = _call_op(L, hs[op.session], op, bufs, sc.sizes)[0]
        for k, t in enumerate(sc.ticks):
            h = hs[t.session]
            n = t.frames.shape[0]
            records = t.form != "submit"
            o = _tick_outputs(n, t.T, records)
            frames = np.array(t.frames, copy=True).reshape(-1)   # pageable: the session stages it before submit returns
            out3 = [o[x].ctypes.data for x in ("pcm16", "pcmf", "results")]
            if t.form == "submit":
                rc = L.mbx_session_submit(h, t.T, frames.ctypes.data, *out3)
            elif t.form in ("indexed", "indexed_perm"):
                rc = L.mbx_session_submit_indexed(h, n, t.T, t.index.ctypes.data, frames.ctypes.data, *out3, o["records"].ctypes.data)
            elif t.form == "soft_indexed":
                rc = L.mbx_session_submit_soft_indexed(h, n, t.T, t.index.ctypes.data, t.soft.ctypes.data, *out3, o["records"].ctypes.data)
            else:
                rc = L.mbx_session_submit_keyed(h, n, t.T, None, frames.ctypes.data, None, t.rows.ctypes.data, *out3, o["records"].ctypes.data)
            _native.check(rc, "submit " + t.form)
            keep.append(frames)
            live.append((t.session, k, o))
            if log is not None:
                log.append((k, t.form, n, t.T, len(live)))
            if t.wait:
                _native.check(L.mbx_session_wait(h), "mbx_session_wait")
            for j, op in enumerate(t.ops):
                rc, got = _call_op(L, hs[op.session], op, bufs, sc.sizes)
                status[(k, j)] = rc
                if j == 0 and op.kind in KINDS and op.count > 0:
                    collect(op.session)
                if op.kind in ("get", "refuse") and got is not None:
                    gets[(k, j)] = got
                    if op.kind == "get" and rc == 0 and op.count:
                        bufs[op.buf] = (got[0][: op.count] if op.state else None, got[1][: op.count] if op.rng else None)
        wait = [L.mbx_session_wait(h) for h in hs]
        for i in range(len(hs)):
            collect(i)
        state, rng = [], []
        for h, n in zip(hs, sc.sizes):
            st, rg = np.zeros((n, 3), PARMS_DTYPE), np.zeros(n, RNG_DTYPE)
            _native.check(L.mbx_session_get_state(h, 0, n, st.ctypes.data, rg.ctypes.data), "mbx_session_get_state")
            state.append(st)
            rng.append(rg)
    except BaseException:
        for h in hs:
            L.mbx_session_destroy(h)
        raise
    destroy = [L.mbx_session_destroy(h) for h in hs]
    return {"ticks": ticks, "gets": gets, "status": status, "state": state, "rng": rng, "wait": wait, "destroy": destroy}


def flatten(run):
    """every array of a run_session result under a name of its own (np.savez; the byte comparison of two runs)"""
    out = {}
    for k, t in enumerate(run["ticks"]):
        for key, v in t.items():
            out[f"tick{k}_{key}"] = v
    for (k, j), (st, rg) in run["gets"].items():
        out[f"get{k}_{j}_state"], out[f"get{k}_{j}_rng"] = st, rg
    for i, (st, rg) in enumerate(zip(run["state"], run["rng"])):
        out[f"final{i}_state"], out[f"final{i}_rng"] = st, rg
    keys = sorted(run["status"])
    out["status_keys"] = np.array(keys, dtype=np.int64).reshape(-1, 2)
    out["status"] = np.array([run["status"][k] for k in keys] + run["wait"] + run["destroy"], dtype=np.int64)
    return out


def child_timeout(S):
    """seconds a fresh process may take for one script: instance_cases.child_timeout for the script's frames (at most S x 38 and SIDE x 25)"""
    import instance_cases

    return instance_cases.child_timeout(instance_cases.Case("churn", "", 0, S + SIDE, 38, 1, "session", {}))


def main():
    codec, S, path = int(sys.argv[1]), int(sys.argv[2]), sys.argv[3]
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    run = run_session(script(codec, S))
    np.savez(path, **flatten(run))
    print(f"ok session churn codec {codec} S {S}: {len(run['ticks'])} ticks, MBX_SESSION_ABI_STATE={os.environ.get('MBX_SESSION_ABI_STATE')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
