"""GPU suite (-m gpu) for wide rows (include/mbx_resample.h): mbx_pcm_resample held bit for bit to the numpy definition
(mbelib_neo_amd.resample.step) over the script of tests/resample_cases.py, call by call, rows and the records read back with
mbx_resample_state_get -- 1, 5 and 9 entries (one entry; a wave's four rows plus one; two waves and a bit; at T = 3 also more than a
workgroup's sixteen rows), one and three frames a call, L in 2, 3, 4, 6 x K in 2, 16, 32, under the designed filter and under the rail
taps that drive the sum to the corner of its bound, every device buffer between guard bands at exactly its alignment and the records
of the call between two records of a known pattern; three calls of T = 1 against one of T = 3 on the device; an index that is a
permutation with one entry outside the state; n = 0 and T = 0; one captured graph replayed three times; set, get and reset; and the
sessions' mbx_session_next_resample behind plain buses and behind held and limited ones, into pinned and into pageable memory, with the
refusals of a submit, and on the buses of a burst-group submit.  Nothing here starts a child process.

The refusal of a state of ANOTHER DEVICE needs two devices: it is checked where torch sees two, and its half that needs none (the
order of the checks, on the host) is in tests/test_resample_host.py."""
import ctypes as C

import numpy as np
import pytest

import edge_mix
import guarded
import resample_cases as A
from mbelib_neo_amd import hold, levels, limit, mixdown, resample
from test_gpu_mixdown import INVALID, _Host, _session

pytestmark = pytest.mark.gpu

PCM16, MIX, LEVELS = 1, mixdown.SESSION_MIXDOWN, levels.SESSION_LEVELS
NS = (1, 5, 9)


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


def _pattern(n, seed):
    """n records no launch writes: every byte a function of its place and the seed"""
    return (np.arange(n * 64, dtype=np.int64) * 37 + seed * 11 + 5).astype(np.uint8).view(resample.RECORD_DTYPE)


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", A.KS)
@pytest.mark.parametrize("L", A.FACTORS)
def test_the_wide_rows_and_the_records_are_those_of_numpy_after_every_call(mbx, L, K):
    """the records of the n entries are records 1 .. n of a state of n + 2: record 0 and record n + 1 are the 64 bytes in front of
    and behind what the launch may write of the state"""
    import torch
    from mbelib_neo_amd import _native

    lib = _native.lib()
    for T in (1, 3):
        for n in NS:
            arena = guarded.Arena([guarded.buf("in", 320 * n * T, "stage", True), guarded.buf("out", 320 * L * n * T, "stage"), guarded.buf("index", 4 * n, "index", True)],
                                  where="cuda", seed=3 + n + 16 * T)
            assert arena.ptr("in") % 32 == 16 and arena.ptr("out") % 32 == 16
            arena.load("index", np.arange(1, n + 1, dtype=np.int32))
            fence = _pattern(2, n + T)
            with resample.ResampleState(n + 2) as state:
                assert state.streams == n + 2 and not state.get().view(np.uint8).any()
                for kind in ("design", "rail"):
                    rs = A.filt(kind, L, K)
                    state.reset(stream=_stream())
                    state.set(fence[:1], 0, stream=_stream())
                    state.set(fence[1:], n + 1, stream=_stream())
                    for c, (want, want_state) in enumerate(A.expected(kind, L, K, T)):
                        arena.load("in", A.call_rows(n, T, c))
                        arena.prefill("out")
                        rc = lib.mbx_pcm_resample(C.addressof(rs), state.handle, arena.ptr("index"), n, T, arena.ptr("in"), arena.ptr("out"), _stream())
                        assert rc == 0, lib.mbx_last_error()
                        torch.cuda.synchronize()
                        got = arena.read("out").view(np.int16).reshape(n * T, 160 * L)
                        wanted = want[:n * T]
                        bad = np.flatnonzero((got != wanted).any(axis=1))
                        assert got.tobytes() == wanted.tobytes(), (kind, L, K, T, n, c, "rows", bad[:8], "first sample", np.flatnonzero(got[bad[0]] != wanted[bad[0]])[:8])
                        st = state.get(stream=_stream())
                        assert st[1:-1].tobytes() == want_state[:n].tobytes(), (kind, L, K, T, n, c, np.flatnonzero((st[1:-1] != want_state[:n]))[:8])
                        assert st[0].tobytes() == fence[0].tobytes() and st[-1].tobytes() == fence[1].tobytes(), (kind, L, K, T, n, c, "the records beside the call's")
                        arena.check(f"{kind}, L {L}, K {K}, T {T}, n {n}, call {c}")
    want = A.expected("rail", L, K, 1)
    assert (want[0][0][1] == -32768).all() and (want[1][0][1, 2 * L:] == 32767).all(), "the clamp fired at both rails"


def test_three_calls_of_one_frame_are_one_call_of_three_and_the_delay_reads_across_frames_and_calls(mbx):
    import torch
    from mbelib_neo_amd import decoder

    dec = decoder.BatchDecoder(0, 1)
    n = 5
    for L, K in ((2, 32), (3, 2), (6, 16)):
        rs = A.filt("delay", L, K)
        with resample.ResampleState(n) as one, resample.ResampleState(n) as three:
            ext = np.zeros((n, 32), np.int16)
            for c in range(2):
                x = A.call_rows(n, 3, c)
                out3 = dec.resample(torch.from_numpy(x).cuda(), 3, three, rs)
                singles = [dec.resample(torch.from_numpy(np.ascontiguousarray(x[t::3])).cuda(), 1, one, rs) for t in range(3)]
                torch.cuda.synchronize()
                got3 = out3.cpu().numpy()
                assert got3.shape == (n * 3, 160 * L)
                assert np.stack([s.cpu().numpy() for s in singles], axis=1).reshape(n * 3, 160 * L).tobytes() == got3.tobytes(), (L, K, c)
                assert one.get().tobytes() == three.get().tobytes(), (L, K, c)
                # the delay identity: y[n*L+p] == x_ext[n - (K-1)], the samples in front of the call's first out of the record
                ext = np.concatenate([ext, x.reshape(n, 480)], axis=1)
                wanted = np.repeat(ext[:, 32 - (K - 1):32 - (K - 1) + 480].reshape(n * 3, 160), L, axis=1)
                assert got3.tobytes() == wanted.tobytes(), (L, K, c)
                ext = ext[:, -32:]
                assert three.get()["hist"].tobytes() == ext.tobytes(), (L, K, c)
    # the hold identity: the input bit for bit
    x = A.call_rows(9, 1, 2)
    with resample.ResampleState(9) as st:
        out = dec.resample(torch.from_numpy(x).cuda(), 1, st, A.filt("hold", 4, 16))
        assert out.cpu().numpy().tobytes() == np.repeat(x, 4, axis=1).tobytes()


def test_an_index_that_is_a_permutation_with_one_entry_outside_the_state(mbx):
    import torch
    from mbelib_neo_amd import decoder

    dec = decoder.BatchDecoder(0, 1)
    rs = A.filt("design", 3, 16)
    index = np.array([6, 2, 9, 0, 11, 5, 12, 1, 4], dtype=np.int32)   # 12 is outside a state of 12 records
    d_index = torch.from_numpy(index).cuda()
    planted = _pattern(12, 4)
    with resample.ResampleState(12) as state:
        state.set(planted, stream=_stream())
        st_np = planted.copy()
        for c in range(A.CALLS):
            x = A.call_rows(9, 3, c)
            out = dec.resample(torch.from_numpy(x).cuda(), 3, state, rs, stream_index=d_index)
            torch.cuda.synchronize()
            want, st_np = resample.step(rs, st_np, 3, x, index)
            got = out.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (c, np.flatnonzero((got != want).any(axis=1)))
            assert state.get(stream=_stream()).tobytes() == st_np.tobytes(), c
            zero, _ = resample.step(rs, resample.fresh_state(1), 3, x[18:21])
            assert got[18:21].tobytes() == zero.tobytes(), "the entry outside ran over a zero history"
        untouched = np.setdiff1d(np.arange(12), index)
        after = state.get(stream=_stream())
        assert after[untouched].tobytes() == planted[untouched].tobytes(), "the records no entry names are intact"
        assert after["hist"][6].tobytes() == x[2, 128:].tobytes() and after["hist"][4].tobytes() == x[26, 128:].tobytes()
        # a negative entry, and one far outside
        index2 = index.copy()
        index2[[0, 3]] = (-1, 2 ** 31 - 1)
        out = dec.resample(torch.from_numpy(x).cuda(), 3, state, rs, stream_index=torch.from_numpy(index2).cuda())
        torch.cuda.synchronize()
        want, st_np = resample.step(rs, st_np, 3, x, index2)
        assert out.cpu().numpy().tobytes() == want.tobytes() and state.get(stream=_stream()).tobytes() == st_np.tobytes()
        assert st_np[[6, 0]].tobytes() == after[[6, 0]].tobytes()


def test_no_entries_and_no_frames_launch_nothing_and_the_records_can_be_set_read_and_reset(mbx):
    import torch
    from mbelib_neo_amd import _native

    lib = _native.lib()
    n = 9
    rs = A.filt("design", 2, 16)
    arena = guarded.Arena([guarded.buf("in", 320 * n, "stage", True), guarded.buf("out", 640 * n, "stage")], where="cuda", seed=23)
    arena.load("in", A.call_rows(n, 1, 0))
    planted = _pattern(n, 9)
    with resample.ResampleState(n) as state:
        state.set(planted, stream=_stream())
        for nn, T in ((0, 1), (n, 0), (0, 0)):
            arena.prefill("out")
            assert lib.mbx_pcm_resample(C.addressof(rs), state.handle, None, nn, T, arena.ptr("in"), arena.ptr("out"), _stream()) == 0, lib.mbx_last_error()
            torch.cuda.synchronize()
            assert arena.read("out").tobytes() == arena.prefill_bytes("out").tobytes() and state.get(stream=_stream()).tobytes() == planted.tobytes(), (nn, T)
        arena.check("nothing to do")
        # a launch over fewer entries than the state has moves only their records
        arena.prefill("out")
        assert lib.mbx_pcm_resample(C.addressof(rs), state.handle, None, n - 2, 1, arena.ptr("in"), arena.ptr("out"), _stream()) == 0
        torch.cuda.synchronize()
        after = state.get(stream=_stream())
        want, want_state = resample.step(rs, planted, 1, A.call_rows(n - 2, 1, 0), np.arange(n - 2))
        assert after.tobytes() == want_state.tobytes() and after[n - 2:].tobytes() == planted[n - 2:].tobytes()
        assert arena.read("out")[:640 * (n - 2)].tobytes() == want.tobytes() and arena.read("out")[640 * (n - 2):].tobytes() == arena.prefill_bytes("out", 640 * (n - 2)).tobytes()
        arena.check("seven of nine")
        # set, get, reset: every int16 is a sample, so no record is refused; the ranges are
        extremes = resample.fresh_state(n)
        extremes["hist"][:, ::2], extremes["hist"][:, 1::2] = -32768, 32767
        state.set(extremes, stream=_stream())
        assert state.get(stream=_stream()).tobytes() == extremes.tobytes() and state.get(3, 4, stream=_stream()).tobytes() == extremes[3:7].tobytes()
        state.reset(2, 3, stream=_stream())
        extremes[2:5] = resample.fresh_state(3)
        assert state.get(stream=_stream()).tobytes() == extremes.tobytes()
        for first, count in ((-1, 2), (0, n + 1), (n, 1), (0, -1)):
            assert lib.mbx_resample_state_get(state.handle, first, count, planted.ctypes.data, _stream()) == INVALID and b"first and count" in lib.mbx_last_error()
            assert lib.mbx_resample_state_set(state.handle, first, count, planted.ctypes.data, _stream()) == INVALID and b"first and count" in lib.mbx_last_error()
            assert lib.mbx_resample_state_reset(state.handle, first, count, _stream()) == INVALID and b"first and count" in lib.mbx_last_error()
        assert lib.mbx_resample_state_get(state.handle, 0, 1, None, _stream()) == INVALID and b"host memory" in lib.mbx_last_error()
        assert state.get(stream=_stream()).tobytes() == extremes.tobytes()
    with resample.ResampleState(0) as none:
        assert none.streams == 0 and none.get().size == 0
        none.reset()


# ---- a graph -------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_replayed_three_times_advances_the_records_three_frames(mbx):
    """one mbx_pcm_resample captured on a side stream: a single node, no parallel branches; new rows are loaded into the same buffer
    between the replays.  The filter went into the node by value and nothing about the records was decided at capture time."""
    import torch
    from mbelib_neo_amd import _native

    lib = _native.lib()
    n, L, K = 9, 6, 32
    rs = A.filt("design", L, K)
    d = torch.zeros((n, 160), dtype=torch.int16, device="cuda")
    out = torch.full((n, 160 * L), 0x5A5A, dtype=torch.int16, device="cuda")
    plain_out = torch.empty((n, 160 * L), dtype=torch.int16, device="cuda")
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with resample.ResampleState(n) as state, resample.ResampleState(n) as plain:
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc = lib.mbx_pcm_resample(C.addressof(rs), state.handle, None, n, 1, d.data_ptr(), out.data_ptr(), side.cuda_stream)
        assert rc == 0, lib.mbx_last_error()
        torch.cuda.synchronize()
        assert not state.get(stream=_stream()).view(np.uint8).any() and (out.cpu().numpy() == 0x5A5A).all(), "a capture runs nothing"
        rs.taps[0] = 0   # the caller's structure may change behind the capture: the node has its own copy
        rs = A.filt("design", L, K)
        for f in range(3):
            x = A.call_rows(n, 1, f)
            d.copy_(torch.from_numpy(x))
            torch.cuda.synchronize()
            g.replay()
            assert lib.mbx_pcm_resample(C.addressof(rs), plain.handle, None, n, 1, d.data_ptr(), plain_out.data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            want, want_state = A.expected("design", L, K, 1)[f]
            assert out.cpu().numpy().tobytes() == plain_out.cpu().numpy().tobytes() == want[:n].tobytes(), f
            assert state.get(stream=_stream()).tobytes() == plain.get(stream=_stream()).tobytes() == want_state[:n].tobytes(), f


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
S, BUSES = 40, 5
OFF = np.arange(0, S + 1, 8, dtype=np.int32)
ROW = np.arange(S, dtype=np.int32)
GAIN = np.array([4096, 3000, -4096, 6000, 2048, 4096, 5000, 4096] * BUSES, dtype=np.int16)


def _frames(k):
    return np.ascontiguousarray(edge_mix.frames(0, S, 1, 61 + k).reshape(S, -1))


@pytest.mark.parametrize("pinned", [False, True])
@pytest.mark.parametrize("chain", ["plain", "held and limited"])
def test_a_session_delivers_its_buses_at_48_khz_beside_the_buses_themselves(mbx, chain, pinned):
    """40 IMBE streams into 5 buses of 8, L = 6, three submits: the wide buses are resample.step over the int16 buses the same submit
    returned, the history carried from submit to submit"""
    from mbelib_neo_amd import _native

    lib = _native.lib()
    a = _session(lib, 0, S, S, PCM16 | MIX | LEVELS)
    rs = A.filt("design", 6, 16)
    h = hold.Hold(600, 300, 1, 3, 4)
    lim = limit.Limit(12000, 64, 1, 5)
    host = _Host(lib, pinned)
    try:
        with mixdown.Plan(OFF, ROW, GAIN) as plan, hold.GateState(plan) as gs, limit.LimitState(BUSES) as ls, resample.ResampleState(BUSES + 1) as state:
            st = resample.fresh_state(BUSES + 1)
            for k in range(3):
                own = host.array((S, 160), np.int16)
                buses = host.array((BUSES, 160), np.int16)
                wide = host.array((BUSES, 960), np.int16)
                if chain == "plain":
                    _native.check(lib.mbx_session_next_mixdown(a, plan.handle, 0, buses.ctypes.data), "next_mixdown")
                else:
                    _native.check(lib.mbx_session_next_mixdown_held(a, plan.handle, 0, C.addressof(h), gs.handle, buses.ctypes.data), "next_mixdown_held")
                    _native.check(lib.mbx_session_next_limit(a, C.addressof(lim), ls.handle), "next_limit")
                _native.check(lib.mbx_session_next_resample(a, C.addressof(rs), state.handle, wide.ctypes.data), "next_resample")
                _native.check(lib.mbx_session_submit(a, 1, _frames(k).ctypes.data, own.ctypes.data, None, None), "submit")
                _native.check(lib.mbx_session_wait(a), "wait")
                assert len(np.unique(own)) > 100 and len(np.unique(buses)) > 100, k
                if chain == "plain":
                    assert buses.tobytes() == mixdown.mix(own, OFF, ROW, GAIN).tobytes(), k
                else:
                    assert int(np.abs(buses.astype(np.int64)).max()) <= 12000, k
                want, st = resample.step(rs, st, 1, np.array(buses), np.arange(BUSES))
                assert wide.tobytes() == want.tobytes(), (chain, pinned, k, np.flatnonzero((wide != want).any(axis=1)))
                assert state.get().tobytes() == st.tobytes(), k
            assert st[:BUSES].view(np.uint8).any() and not st[BUSES:].view(np.uint8).any(), "the record behind the buses is no bus's"
    finally:
        lib.mbx_session_destroy(a)
        host.close()


def test_a_session_refuses_a_resampler_without_int16_buses_or_on_a_short_state_and_uses_the_attachment_up(mbx):
    import torch
    from mbelib_neo_amd import _native, decoder

    lib = _native.lib()
    a = _session(lib, 0, S, S, PCM16 | MIX | LEVELS)
    rs = A.filt("design", 6, 16)
    planted = _pattern(BUSES, 2)
    try:
        with mixdown.Plan(OFF, ROW, GAIN) as plan, resample.ResampleState(BUSES) as state, resample.ResampleState(BUSES - 1) as short:
            state.set(planted)
            short.set(planted[:BUSES - 1])
            own = np.full((S, 160), 0x5A5A, np.int16)
            wide = np.full((BUSES, 960), 0x5A5A, np.int16)
            buses16 = np.full((BUSES, 160), 0x5A5A, np.int16)
            buses8 = np.full((BUSES, 160), 0x5A, np.uint8)

            def attach(st, form=None, buses=None):
                if buses is not None:
                    _native.check(lib.mbx_session_next_mixdown(a, plan.handle, form, buses.ctypes.data), "next_mixdown")
                _native.check(lib.mbx_session_next_resample(a, C.addressof(rs), st.handle, wide.ctypes.data), "next_resample")

            def refused(part):
                assert lib.mbx_session_submit(a, 1, _frames(0).ctypes.data, own.ctypes.data, None, None) == INVALID
                assert b"mbx_session_submit: " + part in lib.mbx_last_error(), lib.mbx_last_error()
                assert lib.mbx_session_wait(a) == 0
                assert (own == 0x5A5A).all() and (wide == 0x5A5A).all() and (buses16 == 0x5A5A).all() and (buses8 == 0x5A).all(), "nothing was queued"
                assert state.get().tobytes() == planted.tobytes() and short.get().tobytes() == planted[:BUSES - 1].tobytes(), "the states as they were"

            attach(state)
            refused(b"a resampler is attached (mbx_session_next_resample) and no buses are")
            for form in (mixdown.ULAW, mixdown.ALAW):
                attach(state, form, buses8)
                refused(b"a resampler is attached (mbx_session_next_resample) and the buses are not MBX_MIXDOWN_PCM16")
            attach(short, mixdown.PCM16, buses16)
            refused(b"the plan has more buses than the resampler's state")
            # every refusal used its attachment up: the next submit is plain and moves no record
            assert lib.mbx_session_submit(a, 1, _frames(0).ctypes.data, own.ctypes.data, None, None) == 0 and lib.mbx_session_wait(a) == 0
            assert len(np.unique(own)) > 100 and (wide == 0x5A5A).all() and state.get().tobytes() == planted.tobytes()
            # the attach call's own refusals; a NULL state clears the attachment
            bad = resample.Resample.of(6, 16, A.taps("design", 6, 16))
            bad.K = 15
            assert lib.mbx_session_next_resample(a, C.addressof(bad), state.handle, wide.ctypes.data) == INVALID
            assert b"mbx_session_next_resample: K is even, 2 .. 32" in lib.mbx_last_error()
            assert lib.mbx_session_next_resample(a, None, state.handle, wide.ctypes.data) == INVALID and b"a resampler is needed" in lib.mbx_last_error()
            assert lib.mbx_session_next_resample(a, C.addressof(rs), state.handle, None) == INVALID and b"no place for the wide buses" in lib.mbx_last_error()
            attach(state, mixdown.PCM16, buses16)
            assert lib.mbx_session_next_resample(a, None, None, None) == 0
            assert lib.mbx_session_submit(a, 1, _frames(1).ctypes.data, own.ctypes.data, None, None) == 0 and lib.mbx_session_wait(a) == 0
            assert (wide == 0x5A5A).all() and not (buses16 == 0x5A5A).all() and state.get().tobytes() == planted.tobytes(), "cleared: the buses came, the wide ones did not"
            if torch.cuda.device_count() > 1:   # a state of another device: refused where it is attached, so no submit ever sees it
                decoder.ensure_init(1)
                with torch.cuda.device(1):
                    other = resample.ResampleState(BUSES)
                try:
                    assert lib.mbx_session_next_resample(a, C.addressof(rs), other.handle, wide.ctypes.data) == INVALID
                    assert b"a state of another device than the session" in lib.mbx_last_error()
                    assert lib.mbx_session_submit(a, 1, _frames(2).ctypes.data, own.ctypes.data, None, None) == 0 and lib.mbx_session_wait(a) == 0
                    assert (wide == 0x5A5A).all()
                finally:
                    with torch.cuda.device(1):
                        other.close()
    finally:
        lib.mbx_session_destroy(a)


def test_a_burst_group_submit_takes_a_resampler_on_its_buses(mbx):
    """buses have no T: the buses a group submit delivered, resampled by numpy, are the wide buses it delivered beside them"""
    import burst_group_cases as G
    from mbelib_neo_amd import _native, bursts as B

    lib = _native.lib()
    codec, streams, F = 0, 70, 2
    s = _session(lib, codec, streams, streams * 2, PCM16 | MIX)
    off = np.array([0, 4, 6], dtype=np.int32)
    row = np.array([0, 1, 2, 3, 4, 5], dtype=np.int32)
    gain = np.array([4096, 4096, 4096, 4096, 4096, -4096], dtype=np.int16)
    rs = A.filt("design", 4, 32)
    shapes = ((codec, F, B.FORM_PACKED, False, 3, 1, 0),)
    scheds = G.schedules(shapes, 17)
    try:
        groups = G.make_groups(shapes, scheds, False, 18, tag=2, slots=[np.array([66, 2, 40], dtype=np.int32)])
        arr, keep = G.group_array(lib, groups)
        with mixdown.Plan(off, row, gain) as plan, resample.ResampleState(2) as state:
            st = resample.fresh_state(2)
            for k in range(2):
                rows6 = np.full((3 * F, 160), 0x5A5A, np.int16)
                buses = np.full((2, 160), 0x5A5A, np.int16)
                wide = np.full((2, 640), 0x5A5A, np.int16)
                _native.check(lib.mbx_session_next_mixdown(s, plan.handle, 0, buses.ctypes.data), "next_mixdown")
                _native.check(lib.mbx_session_next_resample(s, C.addressof(rs), state.handle, wide.ctypes.data), "next_resample")
                assert lib.mbx_session_submit_burst_groups(s, arr, 1, 0, rows6.ctypes.data, None, None) == 0, lib.mbx_last_error()
                assert lib.mbx_session_wait(s) == 0
                assert len(np.unique(rows6)) > 100 and buses.tobytes() == mixdown.mix(rows6, off, row, gain).tobytes(), k
                want, st = resample.step(rs, st, 1, buses)
                assert wide.tobytes() == want.tobytes() and state.get().tobytes() == st.tobytes(), k
            # a resampler and no buses: refused under the group submit's own name, nothing queued, the records as they were
            rows6 = np.full((3 * F, 160), 0x5A5A, np.int16)
            _native.check(lib.mbx_session_next_resample(s, C.addressof(rs), state.handle, wide.ctypes.data), "next_resample")
            assert lib.mbx_session_submit_burst_groups(s, arr, 1, 0, rows6.ctypes.data, None, None) == INVALID
            assert b"mbx_session_submit_burst_groups: a resampler is attached" in lib.mbx_last_error(), lib.mbx_last_error()
            assert lib.mbx_session_wait(s) == 0 and (rows6 == 0x5A5A).all() and state.get().tobytes() == st.tobytes()
        del keep
    finally:
        for sc in scheds:
            sc.close()
        lib.mbx_session_destroy(s)
