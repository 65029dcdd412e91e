"""GPU suite (-m gpu): channel churn in sessions -- mbx_session_reset, mbx_session_seed, mbx_session_get_state and mbx_session_set_state
between the submits of the scripts of tests/session_churn.py (what they hold is tests/test_session_churn_host.py's, on the CPU).  Every
tick of a script is held byte for byte to the HIP twin without sessions (BatchDecoders on ABI triplets, the operations as numpy edits
of their pools) and to the oracle under the bounds of tests/parity.py; every mid-run get_state to both; an operation issued behind a
submit without a wait must itself have completed that submit (the outputs are copied the moment it returns); the source and the
destination of a migration are the same bytes from then on; count = 0 and the refusals change no byte of the state.  The same scripts
run once more with MBX_SESSION_ABI_STATE=1 in a child process of their own (the switch is read when a session is created; one child at
a time, under its own time limit) and must give the resident session's bytes.  One small mixed session takes burst groups around a
reset that spans two codecs."""
import ctypes as C
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
import session_churn as SC

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
KEYS = ("pcm16", "pcmf", "results")
_resident_runs = {}   # (codec, S) -> the flattened arrays of the resident session's run, for the ABI-state twin


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _guard(a):
    return (np.ascontiguousarray(a).view(np.uint8) == SC.GUARD).all()


def _op(sc, k, j):
    return sc.pre[j] if k < 0 else sc.ticks[k].ops[j]


def _resident_run(codec, S):
    if (codec, S) not in _resident_runs:
        _resident_runs[(codec, S)] = SC.run_session(SC.script(codec, S))
    return _resident_runs[(codec, S)]


@pytest.mark.parametrize("S", SC.SIZES)
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_a_session_under_churn_is_the_twin_byte_for_byte_and_the_oracle_in_tolerance(mbx, codec, S):
    from mbelib_neo_amd import _native

    L = _native.lib()
    sc, ref = SC.script(codec, S), SC.reference(codec, S)
    # the instances the plain hard submits of the script are planned to: a one-frame resident step of a small batch is the staged *_res1
    # form, above the small-batch limit the one-launch form (IMBE 7100x4400: its fused one); T = 5 is above the LDS threshold
    names = SC.instance_names(L, sc)
    print("INSTANCES", f"codec {codec} S {S}:", {f"{form} {n} x {T}": name for (form, n, T), name in sorted(names.items())})
    one, five = names[("submit", S, 1)], names[("submit", S, 5)]
    assert five.endswith("_stream_kernel_res"), five
    if S <= 256:
        assert one.endswith("_stream_kernel_res1"), one
    else:
        assert one.endswith("_one_launch_kernel_res") or (codec == 2 and one == "imbe7100_stream_kernel_res1_fused"), one
    got = _resident_run(codec, S)
    twin = SC.run_twin(sc)
    what = f"codec {codec} S {S}"
    # ---- every call's return value
    assert got["wait"] == [0, 0] and got["destroy"] == [0, 0]
    for (k, j), rc in sorted(got["status"].items()):
        op = _op(sc, k, j)
        assert rc == (SC.INVALID if op.kind == "refuse" else 0), f"{what}: tick {k} operation {j} {op[:5]} returned {rc}"
    # ---- every tick: the twin's bytes, the oracle within the project's bounds
    for k, (t, g, w, r) in enumerate(zip(sc.ticks, got["ticks"], twin["ticks"], ref["ticks"])):
        at = f"{what}: tick {k} (session {t.session}, {t.form}, {t.frames.shape[0]} x {t.T})"
        streams = t.index
        for key in KEYS + (("records",) if "records" in g else ()):
            assert not _guard(g[key][-1:]), f"{at}: {key} was not written when the operation behind the submit returned"
            parity.check_exact(w[key], g[key], f"{at}: {key} against the twin", t.T, streams)
        if "records" in g:
            parity.check_exact(r["records"], g["records"], f"{at}: records against the oracle", t.T, streams)
        with parity.located(t.T, streams):
            parity.check_results(r["results"], g["results"], f"{at}: results")
        parity.check_pcm_located(r["pcmf"], g["pcmf"], r["pcm16"], g["pcm16"], t.T, streams, what=f"{at}: pcm", peak=r["peak"])
    # ---- every get_state: the twin's rows, the oracle's in tolerance, the guard row and an unasked buffer untouched
    checked = 0
    for (k, j), (st, rg) in sorted(got["gets"].items()):
        op = _op(sc, k, j)
        at = f"{what}: tick {k} operation {j} {op[:5]}"
        if op.kind == "refuse" or op.count == 0:
            assert _guard(st) and _guard(rg), f"{at}: a refused or empty get_state wrote to its buffers"
            continue
        w_st, w_rg = twin["gets"][(k, j)]
        r_st, r_rg = ref["gets"][(k, j)]
        assert _guard(st[op.count:]) and _guard(rg[op.count:]), f"{at}: the row behind the range was written"
        if op.state:
            assert st[:op.count].tobytes() == w_st.tobytes(), f"{at}: state against the twin"
            parity.check_state(r_st, st[:op.count], what=f"{at}: state against the oracle")
        else:
            assert _guard(st), f"{at}: state = NULL, and the buffer was written"
        if op.rng:
            parity.check_exact(w_rg, rg[:op.count], f"{at}: rng against the twin")
            parity.check_exact(r_rg, rg[:op.count], f"{at}: rng against the oracle")
        else:
            assert _guard(rg), f"{at}: rng = NULL, and the buffer was written"
        checked += 1
    assert checked >= 8
    # ---- count = 0 and the refusals, between two reads of the whole session: no byte changed
    whole = {_op(sc, k, j).buf: v for (k, j), v in got["gets"].items() if _op(sc, k, j).buf in ("whole0", "whole1")}
    assert whole["whole0"][0].tobytes() == whole["whole1"][0].tobytes() and whole["whole0"][1].tobytes() == whole["whole1"][1].tobytes(), \
        f"{what}: a call with count = 0 or a refused call changed the state"
    # ---- the end: the twin's state, the oracle's in tolerance
    for i in range(2):
        assert got["state"][i].tobytes() == twin["state"][i].tobytes(), f"{what}: final state of session {i} against the twin"
        parity.check_exact(twin["rng"][i], got["rng"][i], f"{what}: final rng of session {i} against the twin")
        parity.check_state(ref["state"][i], got["state"][i], what=f"{what}: final state of session {i}")
        parity.check_exact(ref["rng"][i], got["rng"][i], f"{what}: final rng of session {i} against the oracle")
    # ---- migrations (a) and (b): source and destination are the same bytes from the set_state on
    moves = {"a": (0, SC.MIG_A, 0, SC.MIG_A_TO), "b": (0, SC.MIG_B, 1, SC.MIG_B_TO)}
    for name, (i_from, (first, count), i_to, (to, _)) in moves.items():
        k_set = [k for k, t in enumerate(sc.ticks) for op in t.ops if op.kind == "set" and op.buf == name and op.count][0]
        for j in range(count):
            for key in KEYS:
                a = SC.stream_output(sc, got["ticks"], key, i_from, first + j, k_set + 1)
                b = SC.stream_output(sc, got["ticks"], key, i_to, to + j, k_set + 1)
                assert a.shape[0] >= 20 and a.tobytes() == b.tobytes(), f"{what}: migration ({name}), stream {first + j} -> {to + j}: {key} differs"
            assert got["state"][i_from][first + j].tobytes() == got["state"][i_to][to + j].tobytes(), f"{what}: migration ({name}): final state"
            assert got["rng"][i_from][first + j].tobytes() == got["rng"][i_to][to + j].tobytes(), f"{what}: migration ({name}): final rng"


@pytest.mark.parametrize("codec", [0, 1])
def test_the_abi_state_session_gives_the_resident_sessions_bytes(mbx, tmp_path, codec):
    """MBX_SESSION_ABI_STATE=1 (switches): the session keeps ABI triplets and passes d_resident = NULL down every submit
    form.  One codec of each family at S = 96, in a fresh child process, one at a time."""
    S = SC.SIZES[0]
    want = SC.flatten(_resident_run(codec, S))
    path = str(tmp_path / f"abi_state_{codec}.npz")
    keep = ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MBX_") or k in keep}
    env["MBX_SESSION_ABI_STATE"] = "1"
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "session_churn.py"), str(codec), str(S), path], capture_output=True, text=True,
                           timeout=SC.child_timeout(S), env=env)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"session churn codec {codec}: the child process did not finish in {e.timeout} s -- nothing more is started on the card", returncode=3)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"session churn codec {codec}: the child process ended with status {r.returncode} (a signal, an abort or a fault) -- nothing "
                    f"more is started on the card\n{tail}", returncode=3)
    assert r.returncode == 0, f"exit status {r.returncode}\n{tail}"
    assert "MBX_SESSION_ABI_STATE=1" in r.stdout.strip().splitlines()[-1]
    with np.load(path) as child:
        assert sorted(child.files) == sorted(want)
        for name in sorted(want):
            a, b = want[name], child[name]
            assert a.shape == b.shape and np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"codec {codec}: {name} differs under MBX_SESSION_ABI_STATE=1"


# ---- a mixed session: burst groups around a reset that spans two codecs -----------------------------------------------------------------------
MIXED = 40
# one group per codec, ten streams each: (codec, F, form, sequence, streams, bursts per stream, extra stride)
MIXED_GROUPS = ((0, 2, 0, False, 10, 1, 0), (1, 3, 2, True, 10, 2, 1), (2, 1, 0, False, 10, 1, 0), (3, 1, 1, False, 10, 1, 0))
MIXED_FRAMES = 20 + 60 + 10 + 10
MIXED_RESET, MIXED_GET = (7, 6), (27, 6)   # slots 7..12: IMBE 7200x4400 and AMBE 3600x2450; slots 27..32: IMBE 7100x4400 and AMBE 3600x2400


def test_a_mixed_session_takes_a_reset_across_two_codecs_between_its_burst_groups(mbx, oracle):
    """mbx_session_reset hands the AMBE slots 10..12 the IMBE-default triplet, exactly as mbe_initMbeParms does, so the kernels' AMBE
    re-initialisation on the first frame (mbx_stream.hip: mutingThreshold against MBE_MUTING_THRESHOLD_AMBE) is reached mid-run; both
    operations follow a submit without a wait.  Against decode_burst_groups on a twin pool edited the same way, byte for byte, and
    against the oracle, group by group at its codec."""
    import burst_group_cases as G
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder, layout
    from mbelib_neo_amd.layout import PARMS_DTYPE, RECORD_DTYPE, RESULT_DTYPE, RNG_DTYPE

    L = _native.lib()
    codec_of = np.repeat(np.arange(4, dtype=np.uint8), 10)
    assert len({int(codec_of[s]) for s in range(*np.cumsum(MIXED_RESET))}) == 2 and len({int(codec_of[s]) for s in range(*np.cumsum(MIXED_GET))}) == 2
    slots = [np.flatnonzero(codec_of == g[0]).astype(np.int32) for g in MIXED_GROUPS]
    scheds = G.schedules(MIXED_GROUPS, 51)
    seeds = (np.arange(MIXED) * 3 + 5).astype(np.uint32)
    h = C.c_void_p()
    _native.check(L.mbx_session_create_mixed(C.byref(h), MIXED, codec_of.ctypes.data, MIXED_FRAMES, 1 | 2 | 4), "create_mixed")
    twin = decoder.BatchDecoder(0, MIXED, seeds=seeds)
    state, rng = oracle.init_state(MIXED), oracle.rng_seeded(seeds)
    try:
        assert L.mbx_session_streams(h) == MIXED
        _native.check(L.mbx_session_seed(h, 0, MIXED, seeds.ctypes.data), "seed")
        for tick in range(3):
            order = np.random.default_rng(60 + tick)
            groups = G.make_groups(MIXED_GROUPS, scheds, False, 70 + tick, tag=tick + 1, slots=[order.permutation(s) for s in slots])
            arr, keep = G.group_array(L, groups)
            o = [np.zeros((MIXED_FRAMES, 160), np.int16), np.zeros((MIXED_FRAMES, 160), np.float32), np.zeros(MIXED_FRAMES, RESULT_DTYPE)]
            for x in o:
                x.view(np.uint8).fill(SC.GUARD)
            _native.check(L.mbx_session_submit_burst_groups(h, arr, 4, 0, *[x.ctypes.data for x in o]), "submit_burst_groups")
            want = twin.decode_burst_groups(G.on_device(groups), soft=False, want_float=True)
            torch.cuda.synchronize()
            if tick == 1:   # no wait: the reset completes the submit, then the read of another range
                first, count = MIXED_RESET
                assert L.mbx_session_reset(h, first, count) == 0
                got = [x.copy() for x in o]
                st, rg = twin.state_numpy().copy(), twin.rng_numpy().copy()
                st[first:first + count], rg[first:first + count] = layout.init_state(count), layout.rng_default(count)
                twin.set_state(st, rg)
                first, count = MIXED_GET
                part, part_rng = np.zeros((count + 1, 3), PARMS_DTYPE), np.zeros(count + 1, RNG_DTYPE)
                part.view(np.uint8).fill(SC.GUARD)
                part_rng.view(np.uint8).fill(SC.GUARD)
                assert L.mbx_session_get_state(h, first, count, part.ctypes.data, part_rng.ctypes.data) == 0
                assert _guard(part[count:]) and _guard(part_rng[count:])
                assert part[:count].tobytes() == st[first:first + count].tobytes() and part_rng[:count].tobytes() == rg[first:first + count].tobytes()
            else:
                _native.check(L.mbx_session_wait(h), "wait")
                got = o
            for key, x in zip(KEYS, got):
                y = want[key].cpu().numpy()
                assert x.tobytes() == (decoder.results_numpy(want[key]) if key == "results" else y).tobytes(), f"tick {tick}: {key} against the twin"
            rows = B.group_rows(groups)
            for g, first in zip(groups, rows[:-1]):
                s, at = g.schedule, g.slots()
                T = g.bursts_per_stream * s.frames_per_burst
                ref = oracle.process_batch(s.codec, g.n_streams, T, B.apply_schedule(s, g.bursts, burst_stride=g.burst_stride), state[at], rng[at])
                state[at], rng[at] = ref["state"], ref["rng"]
                cut = slice(int(first), int(first) + g.frames)
                what = f"tick {tick} codec {s.codec}"
                with parity.located(T, at):
                    parity.check_results(ref["results"], got[2][cut], what + ": results")
                parity.check_pcm_located(ref["pcmf"], got[1][cut], ref["pcm16"], got[0][cut], T, at, what=what + ": pcm", peak=ref["peak"])
            if tick == 1:   # (the oracle's pool takes the reset behind its decode of the tick)
                first, count = MIXED_RESET
                state[first:first + count], rng[first:first + count] = oracle.init_state(count), oracle.rng_default(count)
        st, rg = np.zeros((MIXED, 3), PARMS_DTYPE), np.zeros(MIXED, RNG_DTYPE)
        _native.check(L.mbx_session_get_state(h, 0, MIXED, st.ctypes.data, rg.ctypes.data), "get_state")
        assert st.tobytes() == twin.state_numpy().tobytes() and rg.tobytes() == twin.rng_numpy().tobytes()
        parity.check_state(state, st, what="final state")
        parity.check_exact(rng, rg, "final rng")
        assert L.mbx_session_wait(h) == 0
    finally:
        assert L.mbx_session_destroy(h) == 0
        for s in scheds:
            s.close()
