"""GPU suite (-m gpu) for limited buses (include/mbx_limit.h): mbx_bus_limit held bit for bit to the numpy definition
(mbelib_neo_amd.limit.step) over the frame script of tests/limit_cases.py, call by call, rows and the records read back with
mbx_limit_state_get -- bus counts on either side of a wave's four buses and of a workgroup's sixteen, one and three frames a call, all
three forms, every device buffer between guard bands at exactly its alignment; the three sums launches against the int64 numpy sums
over short buses of 0, 1, 2 and 5 inputs and buses of 11, 12 and 13 inputs forced long, their clamp equal to the PCM16 rows of their
parents; one captured graph of sums + limit replayed three times; and the sessions' mbx_session_next_limit behind an AGC and held
buses, held to the numpy chain, with the two refusals of a submit, and on the buses of a burst-group submit.  Nothing here starts a child
process."""
import ctypes as C
import functools

import numpy as np
import pytest

import edge_mix
import guarded
import limit_cases as A
from mbelib_neo_amd import agc, hold, levels, limit, mixdown, pcm8
from test_gpu_mixdown import INVALID, _session

pytestmark = pytest.mark.gpu

PCM16, MIX, LEVELS = 1, mixdown.SESSION_MIXDOWN, levels.SESSION_LEVELS
NMAX = 65
CASES = (("bridge", 0), ("bridge", 5), ("rails", 2), ("rails", 7))


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


def _compand(y, form):
    return y if form == mixdown.PCM16 else pcm8.compand(y, pcm8.LAW_ULAW if form == mixdown.ULAW else pcm8.LAW_ALAW)


@functools.lru_cache(maxsize=None)
def _wide():
    """the script spread over NMAX buses: bus i has the rows of script bus i % 8, every other eight of them back to front (n* and the
    ramp then meet other samples); int32 [FRAMES, NMAX, 160]"""
    x = A.script()
    out = np.ascontiguousarray(np.stack([x[:, i % A.BUSES, ::-1] if (i // A.BUSES) & 1 else x[:, i % A.BUSES] for i in range(NMAX)], axis=1))
    out.setflags(write=False)
    return out


def _rows(first, T, n):
    """frames first .. first + T - 1 of the first n buses as the rows of one call, bus-major"""
    return np.array(_wide()[first:first + T, :n].transpose(1, 0, 2).reshape(n * T, 160))


@functools.lru_cache(maxsize=None)
def _expected(name, ramp, T):
    """numpy, once, for NMAX buses (buses do not depend on each other: the first n of them are the answer for n): per call
    (int16 rows [NMAX, T, 160], records after [NMAX])"""
    p = A.params(name, ramp)
    st = limit.fresh_state(NMAX)
    calls = []
    for k in range(A.FRAMES // T):
        out, st, _ = limit.step(_rows(k * T, T, NMAX), T, p, st)
        calls.append((out.reshape(NMAX, T, 160), st))
    return tuple(calls)


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 3, 4, 5, NMAX])
def test_the_rows_and_the_records_are_those_of_numpy_after_every_call_in_all_three_forms(mbx, n, T):
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    arena = guarded.Arena([guarded.buf("sums", 640 * n * T, "stage", True), guarded.buf("out16", 320 * n * T, "stage"), guarded.buf("out8", 160 * n * T, "rng")],
                          where="cuda", seed=17 + n)
    assert arena.ptr("sums") % 32 == 16 and arena.ptr("out16") % 32 == 16 and arena.ptr("out8") % 16 == 8
    with limit.LimitState(n) as state:
        assert state.buses == n and state.get().tobytes() == limit.fresh_state(n).tobytes() and state.sums_ptr() % 16 == 0
        for at, (name, ramp) in enumerate(CASES):
            p = A.params(name, ramp)
            form = mixdown.FORMS[at % 3]
            dst = "out16" if form == mixdown.PCM16 else "out8"
            state.reset(stream=_stream())
            for k, (want, want_state) in enumerate(_expected(name, ramp, T)):
                arena.load("sums", _rows(k * T, T, n))
                arena.prefill("out16", "out8")
                rc = L.mbx_bus_limit(C.addressof(p), state.handle, n, T, arena.ptr("sums"), form, arena.ptr(dst), _stream())
                assert rc == 0, L.mbx_last_error()
                torch.cuda.synchronize()
                got = arena.read(dst).view(mixdown.out_dtype(form)).reshape(n, T, 160)
                wanted = _compand(want[:n], form)
                bad = np.flatnonzero((got != wanted).any(axis=(1, 2)))
                assert got.tobytes() == wanted.tobytes(), (name, ramp, form, k, "buses", bad[:8])
                st = state.get(stream=_stream())
                assert st.tobytes() == want_state[:n].tobytes(), (name, ramp, form, k, np.flatnonzero(st != want_state[:n])[:8])
                other = "out8" if dst == "out16" else "out16"
                assert arena.read(other).tobytes() == arena.prefill_bytes(other).tobytes()
            arena.check(f"{name}, ramp_log2 {ramp}, form {form}, n {n}, T {T}")
        # a launch over fewer buses than the state has moves only their records; n above the state is refused with nothing launched
        if n > 1:
            before = state.get(stream=_stream())
            arena.prefill("out16")
            assert L.mbx_bus_limit(C.addressof(p), state.handle, n - 1, 1, arena.ptr("sums"), 0, arena.ptr("out16"), _stream()) == 0
            torch.cuda.synchronize()
            after = state.get(stream=_stream())
            assert after[n - 1:].tobytes() == before[n - 1:].tobytes()
            assert arena.read("out16")[320 * (n - 1):].tobytes() == arena.prefill_bytes("out16", 320 * (n - 1)).tobytes()
        before = state.get(stream=_stream())
        arena.prefill("out16")
        assert L.mbx_bus_limit(C.addressof(p), state.handle, n + 1, 1, arena.ptr("sums"), 0, arena.ptr("out16"), _stream()) == INVALID
        assert b"mbx_bus_limit: n is above the buses of the state" in L.mbx_last_error()
        torch.cuda.synchronize()
        assert state.get(stream=_stream()).tobytes() == before.tobytes() and arena.read("out16").tobytes() == arena.prefill_bytes("out16").tobytes()
        arena.check(f"n {n}, T {T}, at the end")


def test_set_get_and_reset_of_the_records(mbx):
    from mbelib_neo_amd import _native

    L = _native.lib()
    n = 9
    with limit.LimitState(n) as state:
        planted = limit.fresh_state(n)
        planted["gain_q15"] = np.arange(n) * 4000 + 8
        planted["hold_left"] = 255 - np.arange(n) * 30
        state.set(planted, stream=_stream())
        assert state.get(stream=_stream()).tobytes() == planted.tobytes() and state.get(3, 4, stream=_stream()).tobytes() == planted[3:7].tobytes()
        state.reset(2, 3, stream=_stream())
        planted[2:5] = (32768, 0)
        assert state.get(stream=_stream()).tobytes() == planted.tobytes()
        for record in ((0, 0), (32769, 0), (32768, 256)):
            wrong = planted.copy()
            wrong[n - 1] = record
            assert L.mbx_limit_state_set(state.handle, 0, n, wrong.ctypes.data, _stream()) == INVALID and b"mbx_limit_state_set: a state record" in L.mbx_last_error()
        for first, count in ((-1, 2), (0, n + 1), (n, 1), (0, -1)):
            assert L.mbx_limit_state_get(state.handle, first, count, planted.ctypes.data, _stream()) == INVALID and b"first and count" in L.mbx_last_error()
            assert L.mbx_limit_state_reset(state.handle, first, count, _stream()) == INVALID and b"first and count" in L.mbx_last_error()
        assert state.get(stream=_stream()).tobytes() == planted.tobytes()
    with limit.LimitState(0) as none:
        assert none.buses == 0 and none.get().size == 0
        none.reset()


# ---- the sums ------------------------------------------------------------------------------------------------------------------------------
ROWS = 40
PLANS = {"short": ((0, 1, 2, 5, 3), None), "long": ((11, 0, 12, 2, 13, 1), 2)}   # inputs per bus, long_above


def _plan_arrays(counts, seed):
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    row = rng.integers(0, ROWS, size=int(off[-1])).astype(np.int32)
    row[-1] = ROWS - 1
    gain = rng.integers(-8192, 8193, size=int(off[-1])).astype(np.int16)
    loud = int(np.argmax(counts))
    gain[off[loud]:off[loud + 1]] = 6000          # one bus far beyond the rails: the sums must not be clamped
    return off, row, gain


def _frames_of_rows(seed):
    """three frames of int16 rows [3, ROWS, 160]: full range, every third row quiet so that a gate closes on it"""
    rng = np.random.default_rng(seed)
    x = rng.integers(-32768, 32768, size=(3, ROWS, 160)).astype(np.int16)
    x[:, ::3] //= 50
    x[0, 1], x[1, 1] = 32767, -32768
    return x


@pytest.mark.parametrize("which", sorted(PLANS))
def test_the_sums_are_the_int64_sums_and_their_clamp_is_the_parents_pcm16(mbx, which):
    import torch
    from mbelib_neo_amd import decoder

    counts, long_above = PLANS[which]
    off, row, gain = _plan_arrays(counts, 3 + len(counts))
    n_buses = len(counts)
    x = _frames_of_rows(9)
    dec = decoder.BatchDecoder(0, 1)
    arena = guarded.Arena([guarded.buf("pcm16", 320 * ROWS, "stage", True), guarded.buf("sums", 640 * n_buses, "stage"), guarded.buf("bus16", 320 * n_buses, "stage")],
                          where="cuda", seed=29)
    pcm = arena.tensor("pcm16", torch.int16, ROWS, 160)
    sums = arena.tensor("sums", torch.int32, n_buses, 160)
    bus16 = arena.tensor("bus16", torch.int16, n_buses, 160)
    assert sums.data_ptr() % 32 == 16
    h = hold.Hold(2000, 1000, 1, 2, 3)
    with mixdown.Plan(off, row, gain, long_above=long_above) as plan:
        assert plan.long_buses == (3 if which == "long" else 0) and plan.buses == n_buses
        with hold.GateState(plan) as gs_sums, hold.GateState(plan) as gs_parent:
            st_np = hold.zero_state(int(off[-1]))
            for f in range(3):
                arena.load("pcm16", x[f])
                lv = dec.levels(pcm)
                runs = [("plain", lambda: dec.mixdown_sums(pcm, plan, out=sums), lambda: dec.mixdown(pcm, plan, 0, out=bus16), limit.sums(x[f], off, row, gain))]
                for t in (0, 2000):
                    runs.append((f"gated {t}", lambda t=t: dec.mixdown_gated_sums(pcm, plan, t, 2, levels=lv, out=sums),
                                 lambda t=t: dec.mixdown_gated(pcm, plan, 0, t, 2, levels=lv, out=bus16), limit.sums_gated(x[f], off, row, gain, t, 2)))
                want_held, st_np = limit.sums_held(x[f], off, row, gain, h, st_np)
                runs.append(("held", lambda: dec.mixdown_held_sums(pcm, plan, gs_sums, h, levels=lv, out=sums),
                             lambda: dec.mixdown_held(pcm, plan, gs_parent, h, 0, levels=lv, out=bus16), want_held))
                for name, run_sums, run_parent, want in runs:
                    arena.prefill("sums", "bus16")
                    run_sums()
                    run_parent()
                    torch.cuda.synchronize()
                    got = arena.read("sums").view(np.int32).reshape(n_buses, 160)
                    assert got.tobytes() == want.tobytes(), (which, name, f, np.flatnonzero((got != want).any(axis=1)))
                    assert np.clip(got, -32768, 32767).astype(np.int16).tobytes() == arena.read("bus16").tobytes(), (which, name, f)
                    arena.check(f"{which}, {name}, frame {f}")
                assert gs_sums.get(stream=_stream()).tobytes() == gs_parent.get(stream=_stream()).tobytes() == st_np.tobytes(), f
            assert np.abs(limit.sums(x[2], off, row, gain).astype(np.int64)).max() > 40000, "a bus beyond the rails"
            assert st_np["on"].any() and not st_np["on"].all()


# ---- a graph -------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_of_sums_and_limit_replayed_three_times_advances_the_records_three_frames(mbx):
    """mbx_mixdown_sums into the state's scratch, then mbx_bus_limit, captured once on a side stream: a linear chain, no parallel
    branches; new rows are loaded into the same buffer between the replays.  Nothing about the records was decided at capture time."""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    counts, long_above = PLANS["long"]
    off, row, gain = _plan_arrays(counts, 5)
    n_buses = len(counts)
    x = _frames_of_rows(13)
    p = A.params("bridge", 4)
    d = torch.zeros((ROWS, 160), dtype=torch.int16, device="cuda")
    out = torch.full((n_buses, 160), 0x5A5A, dtype=torch.int16, device="cuda")
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with mixdown.Plan(off, row, gain, long_above=long_above) as plan, limit.LimitState(n_buses) as state:
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc1 = L.mbx_mixdown_sums(plan.handle, d.data_ptr(), ROWS, state.sums_ptr(), side.cuda_stream)
            rc2 = L.mbx_bus_limit(C.addressof(p), state.handle, n_buses, 1, state.sums_ptr(), 0, out.data_ptr(), side.cuda_stream)
        assert rc1 == 0 and rc2 == 0, L.mbx_last_error()
        torch.cuda.synchronize()
        assert state.get(stream=_stream()).tobytes() == limit.fresh_state(n_buses).tobytes() and (out.cpu().numpy() == 0x5A5A).all(), "a capture runs nothing"
        st = limit.fresh_state(n_buses)
        for f in range(3):
            d.copy_(torch.from_numpy(x[f].copy()))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            want, st, _ = limit.step(limit.sums(x[f], off, row, gain), 1, p, st)
            assert out.cpu().numpy().tobytes() == want.tobytes(), f
            assert state.get(stream=_stream()).tobytes() == st.tobytes(), f
        assert (st["gain_q15"] < limit.UNITY).any() and int(np.abs(want.astype(np.int64)).max()) <= 24000


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
def test_a_session_with_agc_held_buses_and_a_limiter_delivers_the_numpy_chain_and_refuses_two_submits(mbx):
    """8 IMBE streams x 1 frame, four submits: agc.step of the int16 rows a twin session delivered -> limit.sums_held -> limit.step;
    then a submit with a limiter and no buses, and one whose plan has more buses than the limiter's state: both refuse before
    anything is queued, use the attachments up and leave the three states as they were."""
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec, S = 0, 8
    a, b = _session(L, codec, S, S, PCM16 | MIX | LEVELS), _session(L, codec, S, S, PCM16)
    off = np.array([0, 3, 8, 16], dtype=np.int32)
    row = np.array([0, 1, 2, 3, 4, 5, 6, 7, 0, 1, 2, 3, 4, 5, 6, 7], dtype=np.int32)
    gain = np.array([4096] * 3 + [6000] * 5 + [8000] * 8, dtype=np.int16)
    ag = agc.Agc(8000, 200, 512, 8192, 64, 32, 3, 0)
    h = hold.Hold(600, 300, 1, 3, 4)
    lim = limit.Limit(20000, 64, 1, 5)
    frames = [np.ascontiguousarray(edge_mix.frames(codec, S, 1, 41 + k).reshape(S, -1)) for k in range(6)]

    def attach(session, plan, gate_state, agc_state, limit_state, form, buses):
        _native.check(L.mbx_session_next_agc(session, C.addressof(ag), agc_state.handle), "next_agc")
        if buses is not None:
            _native.check(L.mbx_session_next_mixdown_held(session, plan.handle, form, C.addressof(h), gate_state.handle, buses.ctypes.data), "next_mixdown_held")
        _native.check(L.mbx_session_next_limit(session, C.addressof(lim), limit_state.handle), "next_limit")

    try:
        with mixdown.Plan(off, row, gain) as plan, hold.GateState(plan) as gs, agc.AgcState(S) as ast, limit.LimitState(3) as ls, limit.LimitState(2) as short:
            st_agc, st_gate, st_lim = agc.fresh_state(S), hold.zero_state(16), limit.fresh_state(3)
            limited = 0
            for k in range(4):
                form = mixdown.FORMS[k % 3]
                own, twin = np.zeros((S, 160), np.int16), np.zeros((S, 160), np.int16)
                buses = np.full((3, 160), 0x5A, mixdown.out_dtype(form))
                attach(a, plan, gs, ast, ls, form, buses)
                _native.check(L.mbx_session_submit(a, 1, frames[k].ctypes.data, own.ctypes.data, None, None), "submit")
                _native.check(L.mbx_session_submit(b, 1, frames[k].ctypes.data, twin.ctypes.data, None, None), "submit (twin)")
                _native.check(L.mbx_session_wait(a), "wait")
                _native.check(L.mbx_session_wait(b), "wait (twin)")
                assert len(np.unique(twin)) > 100, k
                levelled, st_agc, _ = agc.step(twin, 1, ag, st_agc)
                sums, st_gate = limit.sums_held(levelled, off, row, gain, h, st_gate)
                want, st_lim, events = limit.step(sums, 1, lim, st_lim, form)
                limited += int((np.abs(sums.astype(np.int64)).max(axis=1) > 20000).sum())
                assert own.tobytes() == levelled.tobytes(), k
                assert buses.tobytes() == want.tobytes(), (k, form)
                assert ast.get().tobytes() == st_agc.tobytes() and gs.get().tobytes() == st_gate.tobytes() and ls.get().tobytes() == st_lim.tobytes(), k
            assert limited > 0 and (st_lim["gain_q15"] < limit.UNITY).any(), "no bus ever reached the ceiling"
            # a limiter and no buses
            own = np.full((S, 160), 0x5A5A, np.int16)
            attach(a, plan, gs, ast, ls, 0, None)
            assert L.mbx_session_submit(a, 1, frames[4].ctypes.data, own.ctypes.data, None, None) == INVALID
            assert b"mbx_session_submit: a limiter is attached (mbx_session_next_limit) and no buses are" in L.mbx_last_error(), L.mbx_last_error()
            # a plan of three buses on a state of two
            buses = np.full((3, 160), 0x5A5A, np.int16)
            attach(a, plan, gs, ast, short, 0, buses)
            assert L.mbx_session_submit(a, 1, frames[4].ctypes.data, own.ctypes.data, None, None) == INVALID
            assert b"mbx_session_submit: the plan has more buses than the limiter's state" in L.mbx_last_error(), L.mbx_last_error()
            assert L.mbx_session_wait(a) == 0 and (own == 0x5A5A).all() and (buses == 0x5A5A).all()
            assert ast.get().tobytes() == st_agc.tobytes() and gs.get().tobytes() == st_gate.tobytes() and ls.get().tobytes() == st_lim.tobytes()
            assert short.get().tobytes() == limit.fresh_state(2).tobytes()
            # both used their attachments up: the next submit is plain, and the twin follows it
            twin = np.zeros((S, 160), np.int16)
            assert L.mbx_session_submit(a, 1, frames[4].ctypes.data, own.ctypes.data, None, None) == 0 and L.mbx_session_wait(a) == 0
            assert L.mbx_session_submit(b, 1, frames[4].ctypes.data, twin.ctypes.data, None, None) == 0 and L.mbx_session_wait(b) == 0
            assert own.tobytes() == twin.tobytes() and ls.get().tobytes() == st_lim.tobytes() and ast.get().tobytes() == st_agc.tobytes()
            # a NULL state clears the attachment; the session call's own refusals
            bad = limit.Limit(1000, 64, 1, 5)
            assert L.mbx_session_next_limit(a, C.addressof(bad), ls.handle) == INVALID and b"mbx_session_next_limit: ceiling is 1024 .. 32767" in L.mbx_last_error()
            assert L.mbx_session_next_limit(a, None, ls.handle) == INVALID and b"a limit is needed" in L.mbx_last_error()
            _native.check(L.mbx_session_next_limit(a, C.addressof(lim), ls.handle), "next_limit")
            assert L.mbx_session_next_limit(a, None, None) == 0
            assert L.mbx_session_submit(a, 1, frames[5].ctypes.data, own.ctypes.data, None, None) == 0 and L.mbx_session_wait(a) == 0
            assert ls.get().tobytes() == st_lim.tobytes()
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)


def test_a_burst_group_submit_takes_a_limiter_on_its_buses(mbx):
    """buses have no T: the rows a group submit delivered, summed and limited by numpy, are the buses it delivered beside them"""
    import burst_group_cases as G
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    codec, S, F = 0, 70, 2
    s = _session(L, codec, S, S * 2, PCM16 | MIX)
    off = np.array([0, 4, 6], dtype=np.int32)
    row = np.array([0, 1, 2, 3, 4, 5], dtype=np.int32)
    gain = np.array([8000, 8000, 8000, 8000, 4096, -4096], dtype=np.int16)
    lim = limit.Limit(12000, 128, 0, 3)
    shapes = ((codec, F, B.FORM_PACKED, False, 3, 1, 0),)
    scheds = G.schedules(shapes, 17)
    try:
        groups = G.make_groups(shapes, scheds, False, 18, tag=2, slots=[np.array([66, 2, 40], dtype=np.int32)])
        arr, keep = G.group_array(L, groups)
        with mixdown.Plan(off, row, gain) as plan, limit.LimitState(2) as ls:
            st = limit.fresh_state(2)
            for k in range(2):
                rows6 = np.full((3 * F, 160), 0x5A5A, np.int16)
                buses = np.full((2, 160), 0x5A5A, np.int16)
                _native.check(L.mbx_session_next_mixdown(s, plan.handle, 0, buses.ctypes.data), "next_mixdown")
                _native.check(L.mbx_session_next_limit(s, C.addressof(lim), ls.handle), "next_limit")
                assert L.mbx_session_submit_burst_groups(s, arr, 1, 0, rows6.ctypes.data, None, None) == 0, L.mbx_last_error()
                assert L.mbx_session_wait(s) == 0
                assert len(np.unique(rows6)) > 100, k
                want, st, _ = limit.step(limit.sums(rows6, off, row, gain), 1, lim, st)
                assert buses.tobytes() == want.tobytes() and ls.get().tobytes() == st.tobytes(), k
                assert int(np.abs(want.astype(np.int64)).max()) <= 12000
            # a limiter and no buses: refused under the group submit's own name, nothing queued, the records as they were
            rows6 = np.full((3 * F, 160), 0x5A5A, np.int16)
            _native.check(L.mbx_session_next_limit(s, C.addressof(lim), ls.handle), "next_limit")
            assert L.mbx_session_submit_burst_groups(s, arr, 1, 0, rows6.ctypes.data, None, None) == INVALID
            assert b"mbx_session_submit_burst_groups: a limiter is attached" in L.mbx_last_error(), L.mbx_last_error()
            assert L.mbx_session_wait(s) == 0 and (rows6 == 0x5A5A).all() and ls.get().tobytes() == st.tobytes()
        del keep
    finally:
        for sc in scheds:
            sc.close()
        L.mbx_session_destroy(s)
