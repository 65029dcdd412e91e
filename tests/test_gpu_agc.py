"""GPU suite (-m gpu) for levelled rows (include/mbx_agc.h): mbx_pcm_agc held bit for bit to the numpy definition
(mbelib_neo_amd.agc.step) over the frame script of tests/agc_cases.py, call by call, rows and the state read back with
mbx_agc_state_get -- entry counts on either side of a wave's four entries and of a workgroup's sixteen, one and three frames a call,
out of place and in place, every device buffer between guard bands at exactly 16 bytes; a stream index onto a larger state, with
entries outside it; the identities of the header on the device; one captured graph replayed three times; the state calls and every
refusal with a state in hand; behind decodes; and the sessions' mbx_session_next_agc held to numpy of the int16 PCM a twin session
without it delivered, with every int16-derived output of one submit and the rules of the attachment.  Nothing here starts a child
process."""
import ctypes as C
import functools

import numpy as np
import pytest

import agc_cases as A
import burst_group_cases as G
import edge_mix
import guarded
from mbelib_neo_amd import agc, bursts as B, levels, mixdown, pcm8
from test_gpu_mixdown import FILL, INVALID, _Host, _Plans, _session, _untouched

pytestmark = pytest.mark.gpu

PCM16, PCMF, RESULTS, PCM8, MIX, LEVELS = 1, 2, 4, pcm8.SESSION_PCM8, mixdown.SESSION_MIXDOWN, levels.SESSION_LEVELS
NMAX = 67
CASES = (("voice", 0), ("voice", 5), ("extreme", 2), ("extreme", 7))
VOICE = dict(A.SETS["voice"])


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _agc(a, state, index_ptr, n, T, in_ptr, out_ptr, stream=None):
    from mbelib_neo_amd import _native

    return _native.lib().mbx_pcm_agc(None if a is None else C.addressof(a), state.handle if state is not None else None, index_ptr, n, T, in_ptr, out_ptr,
                                     _stream() if stream is None else stream)


@functools.lru_cache(maxsize=None)
def _wide():
    """the script spread over NMAX entries: entry i has the rows of script stream i % 8, every other eight of them back to front (the
    ramp then meets other samples); int16 [FRAMES, NMAX, 160]"""
    x = A.script()
    out = np.stack([x[:, i % A.STREAMS, ::-1] if (i // A.STREAMS) & 1 else x[:, i % A.STREAMS] for i in range(NMAX)], axis=1)
    out = np.ascontiguousarray(out)
    out.setflags(write=False)
    return out


def _rows(first, T, n):
    """frames first .. first + T - 1 of the first n entries as the rows of one call, stream-major"""
    return np.array(_wide()[first:first + T, :n].transpose(1, 0, 2).reshape(n * T, 160))   # (a copy: writable, contiguous)


@functools.lru_cache(maxsize=None)
def _expected(name, ramp, T):
    """numpy, once, for NMAX entries (entries do not depend on each other: the first n of them are the answer for n): per call
    (rows [NMAX, T, 160], state after [NMAX])"""
    a = A.params(name, ramp)
    st = agc.fresh_state(NMAX)
    calls = []
    for k in range(A.FRAMES // T):
        out, st, _ = agc.step(_rows(k * T, T, NMAX), T, a, st)
        calls.append((out.reshape(NMAX, T, 160), st))
    return tuple(calls)


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, NMAX])
def test_the_rows_and_the_state_are_those_of_numpy_after_every_call_out_of_place_and_in_place(mbx, n, T):
    import torch
    from mbelib_neo_amd import _native

    arena = guarded.Arena([guarded.buf("in", 320 * n * T, "stage", True), guarded.buf("out", 320 * n * T, "stage")], where="cuda", seed=11 + n)
    assert arena.ptr("in") % 32 == 16 and arena.ptr("out") % 32 == 16
    with agc.AgcState(n) as state:
        assert state.streams == n and state.get().tobytes() == agc.fresh_state(n).tobytes()
        for name, ramp in CASES:
            a = A.params(name, ramp)
            for in_place in (False, True):
                state.reset(stream=_stream())
                for k, (want, want_state) in enumerate(_expected(name, ramp, T)):
                    x = _rows(k * T, T, n)
                    if in_place:
                        arena.load("out", x)
                    else:
                        arena.load("in", x)
                        arena.prefill("out")
                    src = arena.ptr("out" if in_place else "in")
                    assert _agc(a, state, None, n, T, src, arena.ptr("out")) == 0, _native.lib().mbx_last_error()
                    torch.cuda.synchronize()
                    got = arena.read("out").view(np.int16).reshape(n, T, 160)
                    bad = np.flatnonzero((got != want[:n]).any(axis=(1, 2)))
                    assert got.tobytes() == want[:n].tobytes(), (name, ramp, in_place, k, "entries", bad[:8])
                    st = state.get(stream=_stream())
                    assert st.tobytes() == want_state[:n].tobytes(), (name, ramp, in_place, k, np.flatnonzero(st != want_state[:n])[:8])
                if not in_place:
                    arena.check(f"{name}, ramp_log2 {ramp}, n {n}, T {T}")
        arena.load("in", _rows(0, T, n))   # (the last rows loaded into the read-only buffer are what check() compares it with)
        arena.check(f"n {n}, T {T}, at the end")


# ---- the stream index ------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
def test_a_stream_index_onto_a_larger_state_moves_only_its_records_and_passes_entries_outside_it_through(mbx, T):
    import torch
    from mbelib_neo_amd import _native

    n, streams = 7, 12
    index = np.array([9, -1, 11, 0, streams, 7, 4], dtype=np.int32)   # a permutation of 5 records, and two entries outside the state
    a = A.params("voice", 4)
    arena = guarded.Arena([guarded.buf("in", 320 * n * T, "stage", True), guarded.buf("out", 320 * n * T, "stage"), guarded.buf("index", 4 * n, "index", True)],
                          where="cuda", seed=5)
    arena.load("index", index)
    with agc.AgcState(streams) as state:
        planted = agc.fresh_state(streams)
        planted[[2, 3, 9]] = [(4000, 900), (777, 32768), (2048, 300)]   # two records no entry names, and one that one does
        state.set(planted, stream=_stream())
        st = planted
        for k in range(4):
            x = _rows(k * T, T, n)
            arena.load("in", x)
            arena.prefill("out")
            assert _agc(a, state, arena.ptr("index"), n, T, arena.ptr("in"), arena.ptr("out")) == 0, _native.lib().mbx_last_error()
            torch.cuda.synchronize()
            want, st, events = agc.step(x, T, a, st, index)
            got = arena.read("out").view(np.int16).reshape(n * T, 160)
            assert got.tobytes() == want.tobytes(), (T, k)
            outside = got.reshape(n, T, 160)[[1, 4]]
            assert outside.tobytes() == x.reshape(n, T, 160)[[1, 4]].tobytes(), "the rows of an entry outside the state come back bit for bit"
            assert (events.reshape(n, T)[[1, 4]] == agc.PASSED).all() and not (events.reshape(n, T)[[0, 2, 3, 5, 6]] == agc.PASSED).any()
            assert state.get(stream=_stream()).tobytes() == st.tobytes(), (T, k)
        untouched = np.setdiff1d(np.arange(streams), index)
        assert st[untouched].tobytes() == planted[untouched].tobytes() and planted[2].tolist() == (4000, 900)
        assert not (st[[9, 11, 0, 7, 4]] == planted[[9, 11, 0, 7, 4]]).all()
        arena.check(f"stream index, T {T}")
        # in place with the index, and an index of nothing but entries outside the state: nothing moves at all
        nowhere = np.array([-1, streams, -5, streams + 100, 2 ** 31 - 1, -2 ** 31, streams], dtype=np.int32)
        arena.load("index", nowhere)
        arena.load("out", x)
        assert _agc(a, state, arena.ptr("index"), n, T, arena.ptr("out"), arena.ptr("out")) == 0
        torch.cuda.synchronize()
        assert arena.read("out").tobytes() == x.tobytes() and state.get(stream=_stream()).tobytes() == st.tobytes()
        arena.check(f"entries outside the state, T {T}")


# ---- the identities --------------------------------------------------------------------------------------------------------------------------
def test_the_identities_on_the_device_and_three_frames_in_one_launch_are_three_launches_of_one(mbx):
    import torch

    n = 21
    d = torch.zeros((n * 3, 160), dtype=torch.int16, device="cuda")
    out = torch.full((n * 3, 160), 0x5A5A, dtype=torch.int16, device="cuda")

    def run(a, state, T, x):
        rows = x.shape[0]
        d[:rows].copy_(torch.from_numpy(x.copy()))
        assert _agc(a, state, None, rows // T, T, d.data_ptr(), out.data_ptr()) == 0
        torch.cuda.synchronize()
        return out[:rows].cpu().numpy()

    with agc.AgcState(n) as state, agc.AgcState(n) as other:
        for ramp in (0, 3, 7):
            # min = max = 1024 on a fresh state: the input bit for bit
            state.reset(stream=_stream())
            unity = agc.Agc(8000, 200, 1024, 1024, 64, 32, ramp, 0)
            for f in (0, 12, 13):
                x = _rows(f, 1, n)
                assert run(unity, state, 1, x).tobytes() == x.tobytes(), (ramp, f)
            assert (state.get(stream=_stream())["gain_q10"] == 1024).all()
            # min = max = G on a state at G: the static gain
            for gain in (1, 5000, 32768):
                at = agc.fresh_state(n)
                at["gain_q10"] = gain
                state.set(at, stream=_stream())
                static = agc.Agc(8000, 200, gain, gain, 64, 32, ramp, 0)
                for f in (12, 13):
                    x = _rows(f, 1, n)
                    want = np.clip((x.astype(np.int64) * gain + 512) >> 10, -32768, 32767).astype(np.int16)
                    assert run(static, state, 1, x).tobytes() == want.tobytes(), (ramp, gain, f)
                assert (state.get(stream=_stream())["gain_q10"] == gain).all()
            # rise_q8 = 0 never raises a gain
            state.reset(stream=_stream())
            never = agc.Agc(8000, 200, 512, 8192, 64, 0, ramp, 0)
            before = state.get(stream=_stream())
            for f in range(6):
                run(never, state, 1, _rows(f, 1, n))
                after = state.get(stream=_stream())
                assert (after["gain_q10"] <= before["gain_q10"]).all(), (ramp, f)
                before = after
            assert (before["gain_q10"] < 1024).any()
            # T = 3 in one launch against three launches of T = 1 on the regathered rows
            a = A.params("voice", ramp)
            state.reset(stream=_stream())
            other.reset(stream=_stream())
            for k in range(3):
                three = run(a, state, 3, _rows(3 * k, 3, n)).reshape(n, 3, 160)
                for t in range(3):
                    assert run(a, other, 1, _rows(3 * k + t, 1, n)).tobytes() == np.ascontiguousarray(three[:, t]).tobytes(), (ramp, k, t)
                assert state.get(stream=_stream()).tobytes() == other.get(stream=_stream()).tobytes(), (ramp, k)
            assert not (state.get(stream=_stream()) == agc.fresh_state(n)).all()


# ---- a graph -------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_replayed_three_times_advances_the_state_three_frames(mbx):
    """one mbx_pcm_agc captured once on a side stream (a linear graph); new rows are loaded into the same buffer between the replays.
    Nothing about the state was decided on the host at capture time."""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    n, name, ramp = 21, "voice", 5
    a = A.params(name, ramp)
    d = torch.zeros((n, 160), dtype=torch.int16, device="cuda")
    out = torch.full((n, 160), 0x5A5A, dtype=torch.int16, device="cuda")
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with agc.AgcState(n) as state:
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc = L.mbx_pcm_agc(C.addressof(a), state.handle, None, n, 1, d.data_ptr(), out.data_ptr(), side.cuda_stream)
        assert rc == 0, L.mbx_last_error()
        torch.cuda.synchronize()
        assert state.get(stream=_stream()).tobytes() == agc.fresh_state(n).tobytes() and (out.cpu().numpy() == 0x5A5A).all(), "a capture runs nothing"
        for f, (want, want_state) in enumerate(_expected(name, ramp, 1)[:3]):
            d.copy_(torch.from_numpy(_rows(f, 1, n)))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == want[:n].tobytes(), f
            assert state.get(stream=_stream()).tobytes() == want_state[:n].tobytes(), f
        assert not (want_state[:n] == agc.fresh_state(n)).all()


# ---- the state calls and the refusals ----------------------------------------------------------------------------------------------------------
def test_reset_set_and_get_and_every_refusal_with_a_state_in_hand(mbx):
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    n = 16
    a = A.params("voice", 3)
    g = C.addressof(a)
    arena = guarded.Arena([guarded.buf("in", 320 * n, "stage", True), guarded.buf("out", 320 * n, "stage")], where="cuda", seed=3)
    arena.load("in", _rows(5, 1, n))
    with agc.AgcState(n) as state:
        # set / get round trip, whole and over a sub-range; reset over a sub-range
        planted = agc.fresh_state(n)
        planted["gain_q10"] = np.arange(n) * 2000 + 1
        planted["env"] = 32768 - np.arange(n) * 7
        state.set(planted, stream=_stream())
        assert state.get(stream=_stream()).tobytes() == planted.tobytes()
        assert state.get(3, 5, stream=_stream()).tobytes() == planted[3:8].tobytes() and state.get(n, 0).size == 0
        state.set(np.array([(32768, 0), (1, 32768)], dtype=agc.RECORD_DTYPE), first=14, stream=_stream())
        planted[14:] = [(32768, 0), (1, 32768)]
        state.reset(4, 6, stream=_stream())
        planted[4:10] = (1024, 0)
        state.reset(0, 0, stream=_stream())
        assert state.get(stream=_stream()).tobytes() == planted.tobytes()

        def refused(part, call, *args):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert call(*args) == INVALID, part
            assert part in L.mbx_last_error(), L.mbx_last_error()

        # set: a bad record anywhere in the range, nothing written; ranges outside the records
        for record in ((0, 0), (32769, 0), (1024, 32769), (65535, 65535)):
            wrong = planted.copy()
            wrong[n - 1] = record
            refused(b"mbx_agc_state_set: a state record", L.mbx_agc_state_set, state.handle, 0, n, wrong.ctypes.data, _stream())
        host = agc.fresh_state(n + 1)
        for first, count in ((-1, 2), (0, n + 1), (n, 1), (1, n), (0, -1)):
            refused(b"mbx_agc_state_set: first and count", L.mbx_agc_state_set, state.handle, first, count, host.ctypes.data, _stream())
            refused(b"mbx_agc_state_get: first and count", L.mbx_agc_state_get, state.handle, first, count, host.ctypes.data, _stream())
            refused(b"mbx_agc_state_reset: first and count", L.mbx_agc_state_reset, state.handle, first, count, _stream())
        refused(b"mbx_agc_state_set: host memory", L.mbx_agc_state_set, state.handle, 0, n, None, _stream())
        refused(b"mbx_agc_state_get: host memory", L.mbx_agc_state_get, state.handle, 0, n, None, _stream())
        assert state.get(stream=_stream()).tobytes() == planted.tobytes() and host.tobytes() == agc.fresh_state(n + 1).tobytes()
        # the launcher, a state in hand
        i, o = arena.ptr("in"), arena.ptr("out")
        bad = lambda **kw: agc.Agc(**{**VOICE, "ramp_log2": 3, "zero": 0, **kw})
        for part, args in ((b"agc is needed", (None, state, None, n, 1, i, o)), (b"state is needed", (a, None, None, n, 1, i, o)),
                           (b"target_peak", (bad(target_peak=0), state, None, n, 1, i, o)), (b"target_peak", (bad(target_peak=32768), state, None, n, 1, i, o)),
                           (b"floor_peak", (bad(floor_peak=0), state, None, n, 1, i, o)), (b"floor_peak", (bad(floor_peak=32769), state, None, n, 1, i, o)),
                           (b"1 .. 32768", (bad(min_gain_q10=0), state, None, n, 1, i, o)), (b"1 .. 32768", (bad(max_gain_q10=32769), state, None, n, 1, i, o)),
                           (b"min_gain_q10 is above max_gain_q10", (bad(min_gain_q10=8193), state, None, n, 1, i, o)),
                           (b"MBX_AGC_MAX_RAMP_LOG2", (bad(ramp_log2=8), state, None, n, 1, i, o)), (b"zero", (bad(zero=1), state, None, n, 1, i, o)),
                           (b"negative", (a, state, None, -1, 1, i, o)), (b"negative", (a, state, None, n, -1, i, o)),
                           (b"2^31-1", (a, state, None, 65536, 32768, i, i)), (b"rows in and out", (a, state, None, n, 1, None, o)),
                           (b"rows in and out", (a, state, None, n, 1, i, None)), (b"alignment", (a, state, None, n, 1, i + 8, o)),
                           (b"alignment", (a, state, None, n, 1, i, o + 2)), (b"overlap", (a, state, None, n, 1, o + 320, o)),
                           (b"overlap", (a, state, None, n, 1, o, o + 16))):
            refused(b"mbx_pcm_agc: ", _agc, *args)
            assert part in L.mbx_last_error(), (part, L.mbx_last_error())
        assert _agc(a, state, None, 0, 1, i, o) == 0 and _agc(a, state, None, n, 0, i, o) == 0   # nothing to do
        torch.cuda.synchronize()
        arena.check("refused launches")
        assert arena.read("out").tobytes() == arena.prefill_bytes("out").tobytes(), "a refused call launched something"
        assert state.get(stream=_stream()).tobytes() == planted.tobytes(), "a refused call advanced the state"
        assert L.mbx_agc_state_streams(state.handle) == n
    # a state without records: every entry is outside it
    with agc.AgcState(0) as none:
        assert none.streams == 0 and none.get().size == 0
        none.reset()
        none.set(agc.fresh_state(0))
        assert _agc(a, none, None, n, 1, arena.ptr("in"), arena.ptr("out")) == 0
        torch.cuda.synchronize()
        assert arena.read("out").tobytes() == arena.read("in").tobytes()
        arena.check("a state without records")


# ---- behind a decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1])
def test_behind_three_decodes_the_levelled_rows_are_those_of_numpy_on_their_pcm16(mbx, codec):
    import torch
    from mbelib_neo_amd import decoder

    S, T = 37, 2
    dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) * 7 + 3)
    a = A.params("voice", 5)
    with agc.AgcState(S) as state:
        steps = []
        for k in range(3):
            out = dec.decode(edge_mix.frames(codec, S, T, 1 + k).reshape(S * T, -1), T)
            raw = out["pcm16"].clone()
            steps.append((raw, dec.agc(out["pcm16"], T, state, a, out=out["pcm16"] if k == 1 else None)))   # on the decode's stream; once in place
        torch.cuda.synchronize()
        st = agc.fresh_state(S)
        seen = set()
        for k, (raw, got) in enumerate(steps):
            raw = raw.cpu().numpy()
            assert len(np.unique(raw)) > 100, "the decode gave no audio to level"
            want, st, events = agc.step(raw, T, a, st)
            seen |= set(events.tolist())
            assert got.cpu().numpy().tobytes() == want.tobytes(), (codec, k)
        assert state.get(stream=_stream()).tobytes() == st.tobytes()
        assert seen - {agc.FREEZE} and (st["gain_q10"] != 1024).any(), "the decodes moved no gain"
        with pytest.raises(Exception, match="MBX_AGC_MAX_RAMP_LOG2"):
            dec.agc(steps[0][0], T, state, agc.Agc(8000, 200, 512, 8192, 64, 32, 8, 0))


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
def _next_agc(L, s, a, state):
    return L.mbx_session_next_agc(s, None if a is None else C.addressof(a), state.handle if state is not None else None)


def _frames(codec, S, T, seed):
    return np.ascontiguousarray(edge_mix.frames(codec, S, T, seed).reshape(S * T, -1))


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_four_submits_in_flight_advance_the_state_in_submit_order(mbx, pinned):
    """four submits before the first wait, T and the parameters changing; the int16 rows of each are numpy's of the rows a twin session
    without an AGC delivered, under the state the submits before it left"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec, S = 0, 70
    a, b = _session(L, codec, S, S * 2, PCM16), _session(L, codec, S, S * 2, PCM16)
    host = _Host(L, pinned)
    try:
        with agc.AgcState(S + 3) as state:
            steps = []
            for k, T in enumerate((1, 2, 1, 1)):
                frames = _frames(codec, S, T, 2 + k)
                p = A.params("voice", (3, 7, 0, 5)[k])
                own, twin = host.array((S * T, 160), np.int16), np.zeros((S * T, 160), np.int16)
                _native.check(_next_agc(L, a, p, state), "next_agc")
                _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, own.ctypes.data, None, None), "submit")
                _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin.ctypes.data, None, None), "submit (twin)")
                steps.append((T, p, own, twin))
            _native.check(L.mbx_session_wait(a), "wait")
            _native.check(L.mbx_session_wait(b), "wait (twin)")
            st = agc.fresh_state(S + 3)
            for k, (T, p, own, twin) in enumerate(steps):
                assert len(np.unique(twin)) > 100, k
                want, st, _ = agc.step(twin, T, p, st, np.arange(S))
                assert own.tobytes() == want.tobytes(), f"submit {k}"
            assert state.get().tobytes() == st.tobytes() and (st["gain_q10"][:S] != 1024).any() and st[S:].tobytes() == agc.fresh_state(3).tobytes()
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)
        host.close()


def test_an_indexed_submit_of_5_of_16_streams_moves_exactly_those_five_records(mbx):
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec, S, T = 0, 16, 2
    a, b = _session(L, codec, S, S * T, PCM16), _session(L, codec, S, S * T, PCM16)
    index = np.array([1, 15, 4, 9, 12], dtype=np.int32)
    p = A.params("voice", 4)
    try:
        with agc.AgcState(S) as state:
            st = agc.fresh_state(S)
            for k in range(2):
                frames = _frames(codec, 5, T, 11 + k)
                own, twin = np.zeros((5 * T, 160), np.int16), np.zeros((5 * T, 160), np.int16)
                _native.check(_next_agc(L, a, p, state), "next_agc")
                _native.check(L.mbx_session_submit_indexed(a, 5, T, index.ctypes.data, frames.ctypes.data, own.ctypes.data, None, None, None), "submit")
                _native.check(L.mbx_session_submit_indexed(b, 5, T, index.ctypes.data, frames.ctypes.data, twin.ctypes.data, None, None, None), "submit (twin)")
                _native.check(L.mbx_session_wait(a), "wait")
                _native.check(L.mbx_session_wait(b), "wait (twin)")
                assert len(np.unique(twin)) > 100
                want, st, _ = agc.step(twin, T, p, st, index)
                assert own.tobytes() == want.tobytes(), k
                assert state.get().tobytes() == st.tobytes(), k
            others = np.setdiff1d(np.arange(S), index)
            assert st[others].tobytes() == agc.fresh_state(S - 5).tobytes() and (st[index]["env"] > 0).any()
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)


def test_one_submit_delivers_every_int16_derived_output_of_the_levelled_rows_and_pcmf_untouched(mbx):
    """pcm16, next_pcm8, next_levels and next_mixdown_gated together: the numpy chain agc.step -> pcm8.compand / levels.measure /
    levels.mix_gated; pcmf and the results are those of the submit without an AGC"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec, S, T = 0, 70, 2
    bits = PCM16 | PCMF | RESULTS | PCM8 | MIX | LEVELS
    a, b = _session(L, codec, S, S * T, bits), _session(L, codec, S, S * T, PCM16 | PCMF | RESULTS)
    plans = _Plans()
    p = A.params("voice", 6)
    gate = levels.Gate(600, 3)
    try:
        plan, off, row, gain = plans.of(S * T)
        with agc.AgcState(S) as state:
            st = agc.fresh_state(S)
            for k in range(2):
                frames = _frames(codec, S, T, 21 + k)
                form, law = mixdown.FORMS[k], k
                own16, ownf, ownr = np.zeros((S * T, 160), np.int16), np.zeros((S * T, 160), np.float32), np.zeros((S * T, 5), np.int32)
                twin16, twinf, twinr = np.zeros((S * T, 160), np.int16), np.zeros((S * T, 160), np.float32), np.zeros((S * T, 5), np.int32)
                out8 = np.full((S * T, 160), FILL, np.uint8)
                lv = np.zeros(S * T, dtype=levels.LEVEL_DTYPE)
                buses = np.full((13, 160), FILL, mixdown.out_dtype(form))
                _native.check(_next_agc(L, a, p, state), "next_agc")
                _native.check(L.mbx_session_next_pcm8(a, law, out8.ctypes.data), "next_pcm8")
                _native.check(L.mbx_session_next_levels(a, lv.ctypes.data), "next_levels")
                _native.check(L.mbx_session_next_mixdown_gated(a, plan.handle, form, C.addressof(gate), buses.ctypes.data), "next_mixdown_gated")
                _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, own16.ctypes.data, ownf.ctypes.data, ownr.ctypes.data), "submit")
                _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin16.ctypes.data, twinf.ctypes.data, twinr.ctypes.data), "submit (twin)")
                _native.check(L.mbx_session_wait(a), "wait")
                _native.check(L.mbx_session_wait(b), "wait (twin)")
                assert len(np.unique(twin16)) > 100
                want, st, _ = agc.step(twin16, T, p, st)
                assert own16.tobytes() == want.tobytes() and want.tobytes() != twin16.tobytes(), k
                assert out8.tobytes() == pcm8.compand(want, law).tobytes(), k
                assert lv.tobytes() == levels.measure(want).tobytes(), k
                assert buses.tobytes() == levels.mix_gated(want, off, row, gain, form, 600, 3).tobytes(), k
                assert ownf.tobytes() == twinf.tobytes() and ownr.tobytes() == twinr.tobytes(), k
                assert state.get().tobytes() == st.tobytes(), k
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)
        plans.close()


def test_the_attachment_lasts_one_submit_and_a_refused_submit_leaves_the_state(mbx):
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec, S, F = 0, 70, 2
    frames = {T: _frames(codec, S, T, 30 + T) for T in (1, 3)}
    s = _session(L, codec, S, S * 2, PCM16 | RESULTS)
    twin = _session(L, codec, S, S * 2, PCM16 | RESULTS)
    bare = _session(L, codec, S, S * 2, RESULTS)
    p = A.params("voice", 3)
    try:
        with agc.AgcState(S) as state, agc.AgcState(S - 1) as short:
            def submit(h, T, pcm16, results=None):
                return L.mbx_session_submit(h, T, frames[T].ctypes.data, None if pcm16 is None else pcm16.ctypes.data, None,
                                            None if results is None else results.ctypes.data)

            def both(T, pcm16, raw):
                assert submit(s, T, pcm16) == 0 and submit(twin, T, raw) == 0 and L.mbx_session_wait(s) == 0 and L.mbx_session_wait(twin) == 0

            def refused(part, *args):
                L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
                assert _next_agc(L, *args) == INVALID, part
                assert b"mbx_session_next_agc: " + part in L.mbx_last_error(), L.mbx_last_error()

            pcm16, raw = np.zeros((S * 2, 160), np.int16), np.zeros((S * 2, 160), np.int16)
            refused(b"an agc is needed", s, None, state)
            refused(b"ramp_log2 is above MBX_AGC_MAX_RAMP_LOG2", s, agc.Agc(8000, 200, 512, 8192, 64, 32, 8, 0), state)
            refused(b"min_gain_q10 is above max_gain_q10", s, agc.Agc(8000, 200, 8193, 8192, 64, 32, 3, 0), state)
            refused(b"the zero field is not 0", s, agc.Agc(8000, 200, 512, 8192, 64, 32, 3, 1), state)
            refused(b"the state holds fewer records than the session has streams", s, p, short)
            refused(b"the session was created without an output that has int16 rows", bare, p, state)
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and len(np.unique(raw)) > 100   # none of them left anything
            fresh = agc.fresh_state(S)
            assert state.get().tobytes() == fresh.tobytes()
            # queued: levelled once and the state advanced once; the submit after it is plain and leaves the state
            _native.check(_next_agc(L, s, p, state), "next_agc")
            both(1, pcm16, raw)
            want, st, _ = agc.step(raw[:S], 1, p, fresh)
            assert pcm16[:S].tobytes() == want.tobytes() and want.tobytes() != raw[:S].tobytes() and state.get().tobytes() == st.tobytes()
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and state.get().tobytes() == st.tobytes()
            # refused (T beyond max_frames_per_submit): used up, nothing queued, the state as it was
            _native.check(_next_agc(L, s, p, state), "next_agc")
            assert submit(s, 3, pcm16) == INVALID
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and state.get().tobytes() == st.tobytes()
            # a NULL state clears it
            _native.check(_next_agc(L, s, p, state), "next_agc")
            assert _next_agc(L, s, p, None) == 0 and _next_agc(L, s, None, None) == 0
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and state.get().tobytes() == st.tobytes()
            # only the results asked for: the state advances all the same, by the rows nobody took
            res, res_twin = np.zeros((S, 5), np.int32), np.zeros((S, 5), np.int32)
            _native.check(_next_agc(L, s, p, state), "next_agc")
            assert submit(s, 1, None, res) == 0 and submit(twin, 1, raw, res_twin) == 0 and L.mbx_session_wait(s) == 0 and L.mbx_session_wait(twin) == 0
            _, st, _ = agc.step(raw[:S], 1, p, st)
            assert res.tobytes() == res_twin.tobytes() and state.get().tobytes() == st.tobytes()
            # a burst-group submit refuses an attached AGC with a text of its own and uses it up
            shapes = ((codec, F, B.FORM_PACKED, False, 3, 1, 0),)
            scheds = G.schedules(shapes, 17)
            try:
                groups = G.make_groups(shapes, scheds, False, 18, tag=2, slots=[np.array([66, 2, 40], dtype=np.int32)])
                arr, keep = G.group_array(L, groups)
                _native.check(_next_agc(L, s, p, state), "next_agc")
                out6 = np.full((3 * F, 160), 0x5A5A, np.int16)
                assert L.mbx_session_submit_burst_groups(s, arr, 1, 0, out6.ctypes.data, None, None) == INVALID
                assert b"mbx_session_submit_burst_groups: an AGC is attached" in L.mbx_last_error(), L.mbx_last_error()
                assert (out6 == 0x5A5A).all() and L.mbx_session_wait(s) == 0 and state.get().tobytes() == st.tobytes()
                assert L.mbx_session_submit_burst_groups(s, arr, 1, 0, out6.ctypes.data, None, None) == 0 and L.mbx_session_wait(s) == 0
                assert not (out6 == 0x5A5A).all() and state.get().tobytes() == st.tobytes()
                del keep
            finally:
                for sc in scheds:
                    sc.close()
    finally:
        for h in (s, twin, bare):
            L.mbx_session_destroy(h)
