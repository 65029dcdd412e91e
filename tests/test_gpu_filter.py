"""GPU suite (-m gpu) for filtered rows (include/mbx_filter.h): mbx_pcm_filter held bit for bit to the numpy definition
(mbelib_neo_amd.filters.step) over the script of tests/filter_cases.py, call by call, rows and the records read back with
mbx_filter_state_get -- 1, 5, 65 and 130 entries (one entry; a few; one more than the 64 a wave and a workgroup of the lane-per-entry
kernel take; two workgroups and a bit), one and three frames a call, S in 1, 2, 4, the designed high-pass, the integrators that reach
both rails, the delays and the sections at the corner of the bound, out of place and in place, every device buffer between guard bands
at exactly its alignment and the records of the call between two fence records of a known pattern; three calls of T = 1 against one of
T = 3 on the device, the delay reading across frames and calls; an index that is a permutation with one entry outside the state and a
negative one; n = 0 and T = 0; fewer entries than records; set, get and reset and their refusals; one captured graph replayed three
times; and the sessions' mbx_session_next_filter held to numpy over the int16 rows a twin session without it delivered, alone and in
front of an AGC with every int16-derived output of the submit, with the rules of the attachment.  Nothing here starts a child process.

The refusal of a state of ANOTHER DEVICE needs two devices: it is checked where torch sees two, and its half that needs none (the
order of the checks, on the host) is in tests/test_filter_host.py."""
import ctypes as C

import numpy as np
import pytest

import agc_cases
import burst_group_cases as G
import edge_mix
import filter_cases as A
import guarded
from mbelib_neo_amd import agc, bursts as B, filters, levels, mixdown, pcm8
from test_gpu_mixdown import FILL, INVALID, _Host, _Plans, _session

pytestmark = pytest.mark.gpu

PCM16, PCMF, RESULTS, PCM8, MIX, LEVELS = 1, 2, 4, pcm8.SESSION_PCM8, mixdown.SESSION_MIXDOWN, levels.SESSION_LEVELS
NS = (1, 5, 65, 130)


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
    """n records no launch writes and mbx_filter_state_set takes: every sample a function of its place and the seed, every e a fraction"""
    st = filters.fresh_state(n)
    v = (np.arange(n * 10, dtype=np.int64) * 2671 + seed * 977 + 5).astype(np.int16).reshape(n, 10)
    st["x1"], st["x2"], st["sec"]["y1"], st["sec"]["y2"] = v[:, 0], v[:, 1], v[:, 2:6], v[:, 6:10]
    st["sec"]["e"] = (np.arange(n * 4).reshape(n, 4) * 613 + seed * 31 + 7) % 16384
    return st


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", A.SECTIONS)
@pytest.mark.parametrize("kind", A.KINDS)
def test_the_rows_and_the_records_are_those_of_numpy_after_every_call_out_of_place_and_in_place(mbx, kind, S):
    """the records of the n entries are records 1 .. n of a state of n + 2: record 0 and record n + 1 are the 32 bytes in front of and
    behind what the launch may write of the state"""
    import torch
    from mbelib_neo_amd import _native

    lib = _native.lib()
    f = A.filt(kind, S)
    for T in A.FRAMES:
        for n in NS:
            arena = guarded.Arena([guarded.buf("in", 320 * n * T, "stage", True), guarded.buf("out", 320 * n * T, "stage"), guarded.buf("index", 4 * n, "index", True)],
                                  where="cuda", seed=5 + n + 16 * T)
            assert arena.ptr("in") % 32 == 16 and arena.ptr("out") % 32 == 16
            arena.load("index", np.arange(1, n + 1, dtype=np.int32))
            fence = _pattern(2, n + T)
            with filters.FilterState(n + 2) as state:
                assert state.streams == n + 2 and not state.get().view(np.uint8).any()
                for in_place in (False, True):
                    state.reset(stream=_stream())
                    state.set(fence[:1], 0, stream=_stream())
                    state.set(fence[1:], n + 1, stream=_stream())
                    for c, (want, want_state) in enumerate(A.expected(kind, S, T)):
                        x = A.call_rows(kind, n, T, c)
                        if in_place:
                            arena.load("out", x)
                        else:
                            arena.load("in", x)
                            arena.prefill("out")
                        src = arena.ptr("out" if in_place else "in")
                        rc = lib.mbx_pcm_filter(C.addressof(f), state.handle, arena.ptr("index"), n, T, src, arena.ptr("out"), _stream())
                        assert rc == 0, lib.mbx_last_error()
                        torch.cuda.synchronize()
                        got = arena.read("out").view(np.int16).reshape(n * T, 160)
                        wanted = want[:n * T]
                        bad = np.flatnonzero((got != wanted).any(axis=1))
                        assert got.tobytes() == wanted.tobytes(), (kind, S, T, n, in_place, c, "rows", bad[:8], "first sample", np.flatnonzero(got[bad[0]] != wanted[bad[0]])[:8])
                        st = state.get(stream=_stream())
                        assert st[1:-1].tobytes() == want_state[:n].tobytes(), (kind, S, T, n, in_place, c, np.flatnonzero(st[1:-1] != want_state[:n])[:8])
                        assert st[0].tobytes() == fence[0].tobytes() and st[-1].tobytes() == fence[1].tobytes(), (kind, S, T, n, c, "the records beside the call's")
                    arena.check(f"{kind}, S {S}, T {T}, n {n}, in place {in_place}")
    if kind == "rail":
        want = A.expected("rail", S, 1)
        assert (want[0][0][:, -1] == 32767).all() and (want[1][0][:, -1] == -32768).all(), "both rails were reached"


def test_three_calls_of_one_frame_are_one_call_of_three_and_the_delay_reads_across_frames_and_calls(mbx):
    import torch
    from mbelib_neo_amd import decoder

    dec = decoder.BatchDecoder(0, 1)
    n = 65
    for kind, S in (("delay", 1), ("delay", 4), ("design", 2), ("corner", 4)):
        f = A.filt(kind, S)
        with filters.FilterState(n) as one, filters.FilterState(n) as three:
            line = np.zeros((n, 2 * S), np.int16)
            for c in range(2):
                x = A.call_rows(kind, n, 3, c)
                out3 = dec.filter(torch.from_numpy(x).cuda(), 3, three, f)
                singles = [dec.filter(torch.from_numpy(np.ascontiguousarray(x[t::3])).cuda(), 1, one, f) for t in range(3)]
                torch.cuda.synchronize()
                got3 = out3.cpu().numpy()
                assert got3.shape == (n * 3, 160)
                assert np.stack([s.cpu().numpy() for s in singles], axis=1).reshape(n * 3, 160).tobytes() == got3.tobytes(), (kind, S, c)
                assert one.get().tobytes() == three.get().tobytes(), (kind, S, c)
                if kind == "delay":   # y[k] = x[k - 2 S], the samples in front of the call's first out of the record
                    line = np.concatenate([line, x.reshape(n, 480)], axis=1)
                    assert got3.tobytes() == np.ascontiguousarray(line[:, :480]).tobytes(), (S, c)
                    line = line[:, -2 * S:]
    # the unity identity: the input bit for bit, in place
    x = A.call_rows("design", 130, 1, 2)
    with filters.FilterState(130) as st:
        d = torch.from_numpy(x).cuda()
        out = dec.filter(d, 1, st, filters.Filter.of([(16384, 0, 0, 0, 0)] * 3), out=d)
        assert out.data_ptr() == d.data_ptr() and out.cpu().numpy().tobytes() == x.tobytes()


def test_an_index_that_is_a_permutation_with_one_entry_outside_the_state_and_a_negative_one(mbx):
    import torch
    from mbelib_neo_amd import decoder

    dec = decoder.BatchDecoder(0, 1)
    f = A.filt("design", 2)
    index = np.array([6, 2, 9, 0, 11, 5, 12, 1, -1], dtype=np.int32)   # 12 is outside a state of 12 records
    d_index = torch.from_numpy(index).cuda()
    planted = _pattern(12, 4)
    with filters.FilterState(12) as state:
        state.set(planted, stream=_stream())
        st_np = planted.copy()
        for c in range(A.CALLS):
            x = A.call_rows("design", 9, 3, c)
            out = dec.filter(torch.from_numpy(x).cuda(), 3, state, f, stream_index=d_index)
            torch.cuda.synchronize()
            want, st_np = filters.step(f, st_np, 3, x, index)
            got = out.cpu().numpy()
            assert got.tobytes() == want.tobytes(), (c, np.flatnonzero((got != want).any(axis=1)))
            assert state.get(stream=_stream()).tobytes() == st_np.tobytes(), c
            for entry in (6, 8):
                zero, _ = filters.step(f, filters.fresh_state(1), 3, x[3 * entry:3 * entry + 3])
                assert got[3 * entry:3 * entry + 3].tobytes() == zero.tobytes(), "the entry outside ran over a zero record"
        untouched = np.setdiff1d(np.arange(12), index)
        after = state.get(stream=_stream())
        assert after[untouched].tobytes() == planted[untouched].tobytes(), "the records no entry names are intact"
        assert after["sec"][:, 2:].tobytes() == planted["sec"][:, 2:].tobytes(), "the sections the filter does not have are intact"
        assert after["x1"][6] == x[2, 159] and after["x2"][6] == x[2, 158] and after["x1"][11] == x[14, 159]
        # one far outside
        index2 = index.copy()
        index2[[0, 3]] = (-2 ** 31, 2 ** 31 - 1)
        out = dec.filter(torch.from_numpy(x).cuda(), 3, state, f, stream_index=torch.from_numpy(index2).cuda())
        torch.cuda.synchronize()
        want, st_np = filters.step(f, st_np, 3, x, index2)
        assert out.cpu().numpy().tobytes() == want.tobytes() and state.get(stream=_stream()).tobytes() == st_np.tobytes()
        assert st_np[[6, 0]].tobytes() == after[[6, 0]].tobytes()


def test_no_entries_and_no_frames_launch_nothing_and_the_records_can_be_set_read_and_reset(mbx):
    import torch
    from mbelib_neo_amd import _native

    lib = _native.lib()
    n = 9
    f = A.filt("design", 4)
    arena = guarded.Arena([guarded.buf("in", 320 * n, "stage", True), guarded.buf("out", 320 * n, "stage")], where="cuda", seed=23)
    arena.load("in", A.call_rows("design", n, 1, 0))
    planted = _pattern(n, 9)
    with filters.FilterState(n) as state:
        state.set(planted, stream=_stream())
        for nn, T in ((0, 1), (n, 0), (0, 0)):
            arena.prefill("out")
            assert lib.mbx_pcm_filter(C.addressof(f), state.handle, None, nn, T, arena.ptr("in"), arena.ptr("out"), _stream()) == 0, lib.mbx_last_error()
            torch.cuda.synchronize()
            assert arena.read("out").tobytes() == arena.prefill_bytes("out").tobytes() and state.get(stream=_stream()).tobytes() == planted.tobytes(), (nn, T)
        arena.check("nothing to do")
        # a launch over fewer entries than the state has moves only their records
        arena.prefill("out")
        assert lib.mbx_pcm_filter(C.addressof(f), state.handle, None, n - 2, 1, arena.ptr("in"), arena.ptr("out"), _stream()) == 0
        torch.cuda.synchronize()
        after = state.get(stream=_stream())
        want, want_state = filters.step(f, planted, 1, A.call_rows("design", n - 2, 1, 0), np.arange(n - 2))
        assert after.tobytes() == want_state.tobytes() and after[n - 2:].tobytes() == planted[n - 2:].tobytes()
        assert arena.read("out")[:320 * (n - 2)].tobytes() == want.tobytes() and arena.read("out")[320 * (n - 2):].tobytes() == arena.prefill_bytes("out", 320 * (n - 2)).tobytes()
        arena.check("seven of nine")
        # set, get, reset: every int16 is a sample and every e up to 16383 a fraction; the ranges and the records are refused
        extremes = filters.fresh_state(n)
        extremes["x1"], extremes["x2"], extremes["sec"]["y1"], extremes["sec"]["y2"], extremes["sec"]["e"] = -32768, 32767, 32767, -32768, 16383
        state.set(extremes, stream=_stream())
        assert state.get(stream=_stream()).tobytes() == extremes.tobytes() and state.get(3, 4, stream=_stream()).tobytes() == extremes[3:7].tobytes()
        state.reset(2, 3, stream=_stream())
        extremes[2:5] = filters.fresh_state(3)
        assert state.get(stream=_stream()).tobytes() == extremes.tobytes()
        for first, count in ((-1, 2), (0, n + 1), (n, 1), (0, -1)):
            assert lib.mbx_filter_state_get(state.handle, first, count, planted.ctypes.data, _stream()) == INVALID and b"first and count" in lib.mbx_last_error()
            assert lib.mbx_filter_state_set(state.handle, first, count, planted.ctypes.data, _stream()) == INVALID and b"first and count" in lib.mbx_last_error()
            assert lib.mbx_filter_state_reset(state.handle, first, count, _stream()) == INVALID and b"first and count" in lib.mbx_last_error()
        assert lib.mbx_filter_state_get(state.handle, 0, 1, None, _stream()) == INVALID and b"host memory" in lib.mbx_last_error()
        for field, value in (("e", 16384), ("zero", 1)):
            wrong = _pattern(3, 1)
            (wrong["sec"]["e"] if field == "e" else wrong["zero"])[2, 1] = value
            assert lib.mbx_filter_state_set(state.handle, 0, 3, wrong.ctypes.data, _stream()) == INVALID and b"state record" in lib.mbx_last_error(), field
        assert state.get(stream=_stream()).tobytes() == extremes.tobytes(), "a refused set writes nothing"
    with filters.FilterState(0) as none:
        assert none.streams == 0 and none.get().size == 0
        none.reset()


# ---- a graph -------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_replayed_three_times_advances_the_records_three_frames(mbx):
    """one mbx_pcm_filter captured on a side stream: a single node, no parallel branches; new rows are loaded into the same buffer
    between the replays.  The filter went into the node by value and nothing about the records was decided at capture time."""
    import torch
    from mbelib_neo_amd import _native

    lib = _native.lib()
    n, S = 65, 4
    f = A.filt("design", S)
    d = torch.zeros((n, 160), dtype=torch.int16, device="cuda")
    out = torch.full((n, 160), 0x5A5A, dtype=torch.int16, device="cuda")
    plain_out = torch.empty((n, 160), dtype=torch.int16, device="cuda")
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with filters.FilterState(n) as state, filters.FilterState(n) as plain:
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc = lib.mbx_pcm_filter(C.addressof(f), state.handle, None, n, 1, d.data_ptr(), out.data_ptr(), side.cuda_stream)
        assert rc == 0, lib.mbx_last_error()
        torch.cuda.synchronize()
        assert not state.get(stream=_stream()).view(np.uint8).any() and (out.cpu().numpy() == 0x5A5A).all(), "a capture runs nothing"
        f.sec[0].b0, f.sec[3].a2, f.sections = 0, 0, 1   # the caller's structure may change behind the capture: the node has its own copy
        f = A.filt("design", S)
        for k in range(3):
            x = A.call_rows("design", n, 1, k)
            d.copy_(torch.from_numpy(x))
            torch.cuda.synchronize()
            g.replay()
            assert lib.mbx_pcm_filter(C.addressof(f), plain.handle, None, n, 1, d.data_ptr(), plain_out.data_ptr(), _stream()) == 0
            torch.cuda.synchronize()
            want, want_state = A.expected("design", S, 1)[k]
            assert out.cpu().numpy().tobytes() == plain_out.cpu().numpy().tobytes() == want[:n].tobytes(), k
            assert state.get(stream=_stream()).tobytes() == plain.get(stream=_stream()).tobytes() == want_state[:n].tobytes(), k


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
SS = 40


def _next_filter(L, s, f, state):
    return L.mbx_session_next_filter(s, None if f is None else C.addressof(f), state.handle if state is not None else None)


def _frames(S, T, seed):
    return np.ascontiguousarray(edge_mix.frames(0, S, T, seed).reshape(S * T, -1))


def test_three_submits_deliver_the_filtered_rows_of_a_twin_session_indexed_and_unindexed(mbx):
    """40 IMBE streams: the rows returned with a filter attached are filters.step over the rows a twin session without it returned,
    the state carried from submit to submit; then three indexed submits of 5 of the streams"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    a, b = _session(L, 0, SS, SS * 2, PCM16), _session(L, 0, SS, SS * 2, PCM16)
    f = filters.highpass(200, 2)
    try:
        with filters.FilterState(SS + 3) as state:
            st = filters.fresh_state(SS + 3)
            for k, T in enumerate((1, 2, 1)):
                frames = _frames(SS, T, 2 + k)
                own, twin = np.zeros((SS * T, 160), np.int16), np.zeros((SS * T, 160), np.int16)
                _native.check(_next_filter(L, a, f, state), "next_filter")
                _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, own.ctypes.data, None, None), "submit")
                _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin.ctypes.data, None, None), "submit (twin)")
                _native.check(L.mbx_session_wait(a), "wait")
                _native.check(L.mbx_session_wait(b), "wait (twin)")
                assert len(np.unique(twin)) > 100, k
                want, st = filters.step(f, st, T, twin, np.arange(SS))
                assert own.tobytes() == want.tobytes() and want.tobytes() != twin.tobytes(), f"submit {k}"
                assert state.get().tobytes() == st.tobytes(), k
            assert st[:SS].view(np.uint8).any() and not st[SS:].view(np.uint8).any()
            index = np.array([1, 39, 4, 9, 12], dtype=np.int32)
            before = st.copy()
            for k in range(3):
                frames = _frames(5, 2, 11 + k)
                own, twin = np.zeros((10, 160), np.int16), np.zeros((10, 160), np.int16)
                _native.check(_next_filter(L, a, f, state), "next_filter")
                _native.check(L.mbx_session_submit_indexed(a, 5, 2, index.ctypes.data, frames.ctypes.data, own.ctypes.data, None, None, None), "submit")
                _native.check(L.mbx_session_submit_indexed(b, 5, 2, index.ctypes.data, frames.ctypes.data, twin.ctypes.data, None, None, None), "submit (twin)")
                _native.check(L.mbx_session_wait(a), "wait")
                _native.check(L.mbx_session_wait(b), "wait (twin)")
                want, st = filters.step(f, st, 2, twin, index)
                assert own.tobytes() == want.tobytes() and state.get().tobytes() == st.tobytes(), k
            others = np.setdiff1d(np.arange(SS + 3), index)
            assert st[others].tobytes() == before[others].tobytes() and st[index].tobytes() != before[index].tobytes()
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)


def test_one_submit_delivers_every_int16_derived_output_of_the_filtered_then_levelled_rows_and_pcmf_untouched(mbx):
    """filter + AGC + pcm8 + levels + gated buses attached together: every int16-derived output is that of numpy's chain
    filters.step -> agc.step -> pcm8.compand / levels.measure / levels.mix_gated, which proves the order (a gain in front of the filter
    gives other rows: asserted); pcmf and the results are those of the submit without either"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    T = 1
    bits = PCM16 | PCMF | RESULTS | PCM8 | MIX | LEVELS
    a, b = _session(L, 0, SS, SS * T, bits), _session(L, 0, SS, SS * T, PCM16 | PCMF | RESULTS)
    plans = _Plans()
    f = filters.highpass(300, 2)
    p = agc_cases.params("voice", 6)
    gate = levels.Gate(600, 3)
    try:
        plan, off, row, gain = plans.of(SS * T)
        with filters.FilterState(SS) as fstate, agc.AgcState(SS) as astate:
            fst, ast = filters.fresh_state(SS), agc.fresh_state(SS)
            for k in range(3):
                frames = _frames(SS, T, 21 + k)
                form, law = mixdown.FORMS[k % 2], k % 2
                own16, ownf, ownr = np.zeros((SS * T, 160), np.int16), np.zeros((SS * T, 160), np.float32), np.zeros((SS * T, 5), np.int32)
                twin16, twinf, twinr = np.zeros((SS * T, 160), np.int16), np.zeros((SS * T, 160), np.float32), np.zeros((SS * T, 5), np.int32)
                out8 = np.full((SS * T, 160), FILL, np.uint8)
                lv = np.zeros(SS * T, dtype=levels.LEVEL_DTYPE)
                buses = np.full((13, 160), FILL, mixdown.out_dtype(form))
                _native.check(L.mbx_session_next_agc(a, C.addressof(p), astate.handle), "next_agc")   # (attached first: the order is the library's)
                _native.check(_next_filter(L, a, f, fstate), "next_filter")
                _native.check(L.mbx_session_next_pcm8(a, law, out8.ctypes.data), "next_pcm8")
                _native.check(L.mbx_session_next_levels(a, lv.ctypes.data), "next_levels")
                _native.check(L.mbx_session_next_mixdown_gated(a, plan.handle, form, C.addressof(gate), buses.ctypes.data), "next_mixdown_gated")
                _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, own16.ctypes.data, ownf.ctypes.data, ownr.ctypes.data), "submit")
                _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin16.ctypes.data, twinf.ctypes.data, twinr.ctypes.data), "submit (twin)")
                _native.check(L.mbx_session_wait(a), "wait")
                _native.check(L.mbx_session_wait(b), "wait (twin)")
                assert len(np.unique(twin16)) > 100
                other, _, _ = agc.step(twin16, T, p, ast)
                other, _ = filters.step(f, fst, T, other)
                filtered, fst = filters.step(f, fst, T, twin16)
                want, ast, _ = agc.step(filtered, T, p, ast)
                assert own16.tobytes() == want.tobytes() and want.tobytes() != twin16.tobytes() and want.tobytes() != other.tobytes(), k
                assert out8.tobytes() == pcm8.compand(want, law).tobytes(), k
                assert lv.tobytes() == levels.measure(want).tobytes(), k
                assert buses.tobytes() == levels.mix_gated(want, off, row, gain, form, 600, 3).tobytes(), k
                assert ownf.tobytes() == twinf.tobytes() and ownr.tobytes() == twinr.tobytes(), k
                assert fstate.get().tobytes() == fst.tobytes() and astate.get().tobytes() == ast.tobytes(), k
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)
        plans.close()


def test_the_attachment_lasts_one_submit_and_a_refused_submit_leaves_the_state(mbx):
    import torch
    from mbelib_neo_amd import _native, decoder

    L = _native.lib()
    S, F = 70, 2
    frames = {T: _frames(S, T, 30 + T) for T in (1, 3)}
    s = _session(L, 0, S, S * 2, PCM16 | RESULTS)
    twin = _session(L, 0, S, S * 2, PCM16 | RESULTS)
    bare = _session(L, 0, S, S * 2, RESULTS)
    f = filters.highpass(200, 2)
    try:
        with filters.FilterState(S) as state, filters.FilterState(S - 1) as short:
            def submit(h, T, pcm16, results=None):
                return L.mbx_session_submit(h, T, frames[T].ctypes.data, None if pcm16 is None else pcm16.ctypes.data, None,
                                            None if results is None else results.ctypes.data)

            def both(T, pcm16, raw):
                assert submit(s, T, pcm16) == 0 and submit(twin, T, raw) == 0 and L.mbx_session_wait(s) == 0 and L.mbx_session_wait(twin) == 0

            def refused(part, *args):
                L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
                assert _next_filter(L, *args) == INVALID, part
                assert b"mbx_session_next_filter: " + part in L.mbx_last_error(), L.mbx_last_error()

            pcm16, raw = np.zeros((S * 2, 160), np.int16), np.zeros((S * 2, 160), np.int16)
            over, beyond, many = filters.highpass(200, 2), filters.highpass(200, 2), filters.highpass(200, 2)
            over.sec[1].b0, over.sec[1].b1, over.sec[1].b2 = 32767, -32768, 1
            beyond.sec[2].a1 = 1
            many.sections = 5
            refused(b"a filter is needed", s, None, state)
            refused(b"sections is 1 .. MBX_FILTER_MAX_SECTIONS", s, many, state)
            refused(b"a section whose |b0| + |b1| + |b2| or |a1| + |a2| is above 65535", s, over, state)
            refused(b"a non-zero coefficient beyond sections", s, beyond, state)
            refused(b"the state holds fewer records than the session has streams", s, f, short)
            refused(b"the session was created without an output that has int16 rows", bare, f, state)
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and len(np.unique(raw)) > 100   # none of them left anything
            fresh = filters.fresh_state(S)
            assert state.get().tobytes() == fresh.tobytes()
            # queued: filtered once and the state advanced once; the submit after it is plain and leaves the state
            _native.check(_next_filter(L, s, f, state), "next_filter")
            both(1, pcm16, raw)
            want, st = filters.step(f, fresh, 1, raw[:S])
            assert pcm16[:S].tobytes() == want.tobytes() and want.tobytes() != raw[:S].tobytes() and state.get().tobytes() == st.tobytes()
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and state.get().tobytes() == st.tobytes()
            # refused (T beyond max_frames_per_submit): used up, nothing queued, the state as it was
            _native.check(_next_filter(L, s, f, state), "next_filter")
            assert submit(s, 3, pcm16) == INVALID
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and state.get().tobytes() == st.tobytes()
            # a NULL state clears it
            _native.check(_next_filter(L, s, f, state), "next_filter")
            assert _next_filter(L, s, f, None) == 0 and _next_filter(L, s, None, None) == 0
            both(1, pcm16, raw)
            assert pcm16.tobytes() == raw.tobytes() and state.get().tobytes() == st.tobytes()
            # only the results asked for: the state advances all the same, by the rows nobody took
            res, res_twin = np.zeros((S, 5), np.int32), np.zeros((S, 5), np.int32)
            _native.check(_next_filter(L, s, f, state), "next_filter")
            assert submit(s, 1, None, res) == 0 and submit(twin, 1, raw, res_twin) == 0 and L.mbx_session_wait(s) == 0 and L.mbx_session_wait(twin) == 0
            _, st = filters.step(f, st, 1, raw[:S])
            assert res.tobytes() == res_twin.tobytes() and state.get().tobytes() == st.tobytes()
            # a burst-group submit refuses an attached filter under its own name and uses it up
            shapes = ((0, F, B.FORM_PACKED, False, 3, 1, 0),)
            scheds = G.schedules(shapes, 17)
            try:
                groups = G.make_groups(shapes, scheds, False, 18, tag=2, slots=[np.array([66, 2, 40], dtype=np.int32)])
                arr, keep = G.group_array(L, groups)
                _native.check(_next_filter(L, s, f, state), "next_filter")
                out6 = np.full((3 * F, 160), 0x5A5A, np.int16)
                assert L.mbx_session_submit_burst_groups(s, arr, 1, 0, out6.ctypes.data, None, None) == INVALID
                assert b"mbx_session_submit_burst_groups: a filter is attached" in L.mbx_last_error(), L.mbx_last_error()
                assert (out6 == 0x5A5A).all() and L.mbx_session_wait(s) == 0 and state.get().tobytes() == st.tobytes()
                assert L.mbx_session_submit_burst_groups(s, arr, 1, 0, out6.ctypes.data, None, None) == 0 and L.mbx_session_wait(s) == 0
                assert not (out6 == 0x5A5A).all() and state.get().tobytes() == st.tobytes()
                del keep
            finally:
                for sc in scheds:
                    sc.close()
            if torch.cuda.device_count() > 1:   # a state of another device: refused where it is attached, so no submit ever sees it
                decoder.ensure_init(1)
                with torch.cuda.device(1):
                    other = filters.FilterState(S)
                try:
                    refused(b"a state of another device than the session", s, f, other)
                    both(1, pcm16, raw)
                    assert pcm16.tobytes() == raw.tobytes() and state.get().tobytes() == st.tobytes()
                finally:
                    with torch.cuda.device(1):
                        other.close()
    finally:
        for h in (s, twin, bare):
            L.mbx_session_destroy(h)
