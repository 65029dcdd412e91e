"""GPU suite (-m gpu) for the held gate (include/mbx_hold.h): mbx_mixdown_held held byte for byte to the numpy definition
(mbelib_neo_amd.hold.step) over the frame script of tests/hold_cases.py, frame by frame, outputs and the state read back with
mbx_gate_state_get -- through both kernel forms (mbx_mixdown_plan_create_split forces every bus size through each), the three output
forms, between guard bands at exactly the alignments of the contract; the two identities of the header on the device against
mbx_mixdown_gated and mbx_mixdown; a hold that changes mid-script, with hundreds of inputs falling at once; the state calls and the
refusals that need a plan; one captured graph replayed over three frames; behind a decode; and the sessions'
mbx_session_next_mixdown_held held to numpy of the int16 PCM the same submits delivered, with the rules of the attachment.  Nothing
here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import edge_mix
import guarded
import hold_cases as H
from mbelib_neo_amd import hold, levels, mixdown
from test_gpu_mixdown import FILL, INVALID, S, _Host, _Plans, _session, _untouched

pytestmark = pytest.mark.gpu

PCM16, MIX, LEVELS = 1, mixdown.SESSION_MIXDOWN, levels.SESSION_LEVELS
ROWS = H.ROWS


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


def _levels(in_ptr, nrows, out_ptr):
    from mbelib_neo_amd import _native

    return _native.lib().mbx_pcm_levels(in_ptr, nrows, out_ptr, _stream())


def _held(plan, h, state, form, in_ptr, nrows, lv_ptr, out_ptr, stream=None):
    from mbelib_neo_amd import _native

    hd = None if h is None else (h if isinstance(h, hold.Hold) else H.hold_of(h))
    return _native.lib().mbx_mixdown_held(plan.handle if plan is not None else None, None if hd is None else C.addressof(hd),
                                          state.handle if state is not None else None, form, in_ptr, nrows, lv_ptr, out_ptr,
                                          _stream() if stream is None else stream)


class _Bench:
    """the script's rows, their records and a bus array per form on the device, plain tensors"""

    def __init__(self, n_buses):
        import torch

        self.d = torch.zeros((ROWS, 160), dtype=torch.int16, device="cuda")
        self.lv = torch.full((ROWS, 16), FILL, dtype=torch.uint8, device="cuda")
        self.out = {form: torch.full((n_buses, 160), FILL, dtype=torch.int16 if form == mixdown.PCM16 else torch.uint8, device="cuda") for form in mixdown.FORMS}

    def frame(self, x):
        import torch

        self.d.copy_(torch.from_numpy(x.copy()))
        assert _levels(self.d.data_ptr(), ROWS, self.lv.data_ptr()) == 0

    def held(self, plan, h, state, form):
        import torch
        from mbelib_neo_amd import _native

        assert _held(plan, h, state, form, self.d.data_ptr(), ROWS, self.lv.data_ptr(), self.out[form].data_ptr()) == 0, _native.lib().mbx_last_error()
        torch.cuda.synchronize()
        return self.out[form].cpu().numpy()


# ---- parity --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [None, 4096, 1], ids=["default-split", "all-short", "all-long"])
def test_both_kernel_forms_give_the_bytes_and_the_state_of_numpy_frame_by_frame(mbx, above):
    """the default split (22), every bus short (long_above = 4096: one lane decides a bus of 4,096), and every bus of two inputs or more
    long (long_above = 1); every hold of the suites, three forms, twelve frames each; rows, records and buses between guard bands at
    16 bytes (8 for the byte buses) and no better"""
    import torch
    from mbelib_neo_amd import _native

    x, off, row, gain, sizes = H.script()
    n_buses = len(sizes)
    arena = guarded.Arena([guarded.buf("pcm16", 320 * ROWS, "stage", True), guarded.buf("levels", 16 * ROWS, "stage"),
                           guarded.buf("bus16", 320 * n_buses, "stage"), guarded.buf("bus8", 160 * n_buses, "rng")], where="cuda", seed=7)
    assert arena.ptr("pcm16") % 32 == 16 and arena.ptr("levels") % 32 == 16 and arena.ptr("bus16") % 32 == 16 and arena.ptr("bus8") % 16 == 8
    with mixdown.Plan(off, row, gain, long_above=above) as plan:
        assert plan.long_buses == {None: sum(s > 22 for s in sizes), 4096: 0, 1: sum(s > 1 for s in sizes)}[above]
        with hold.GateState(plan) as state:
            assert state.inputs == off[-1] and not state.get().view(np.uint32).any()
            for h in H.HOLDS:
                for form in mixdown.FORMS:
                    name = "bus16" if form == mixdown.PCM16 else "bus8"
                    state.reset(_stream())
                    for f, (want_out, want_state) in enumerate(H.expected(h, form)):
                        arena.load("pcm16", x[f])
                        arena.prefill("bus16", "bus8")
                        assert _levels(arena.ptr("pcm16"), ROWS, arena.ptr("levels")) == 0
                        assert _held(plan, h, state, form, arena.ptr("pcm16"), ROWS, arena.ptr("levels"), arena.ptr(name)) == 0, _native.lib().mbx_last_error()
                        torch.cuda.synchronize()
                        got = arena.read(name).view(mixdown.out_dtype(form)).reshape(n_buses, 160)
                        bad = np.flatnonzero((got != want_out).any(axis=1))
                        assert got.tobytes() == want_out.tobytes(), (above, h, form, f, "buses", bad[:8], "of sizes", [sizes[b] for b in bad[:8]])
                        st = state.get(_stream())
                        assert st.tobytes() == want_state.tobytes(), (above, h, form, f, "inputs", np.flatnonzero(st != want_state)[:8])
                    arena.check(f"hold {h}, form {form}, long_above {above}")
                    other = "bus8" if name == "bus16" else "bus16"
                    assert arena.read(other).tobytes() == arena.prefill_bytes(other).tobytes()


# ---- the identities ------------------------------------------------------------------------------------------------------------------------
def test_the_two_identities_on_the_device_against_the_gated_and_the_plain_mix_down(mbx):
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    x, off, row, gain, sizes = H.script()
    bench = _Bench(len(sizes))
    ref = {form: torch.full((len(sizes), 160), FILL, dtype=bench.out[form].dtype, device="cuda") for form in mixdown.FORMS}
    with mixdown.Plan(off, row, gain) as plan, hold.GateState(plan) as state:
        # {t, t, 0, n, 0} on zeroed state: in every frame the bytes of mbx_mixdown_gated under {t, n}
        for t, n in ((H.OPEN, 0), (H.OPEN, 3), (0, 1), (32768, 8)):
            gate = levels.Gate(t, n)
            for form in mixdown.FORMS:
                state.reset(_stream())
                for f in range(4):
                    bench.frame(x[f])
                    got = bench.held(plan, (t, t, 0, n, 0), state, form)
                    assert L.mbx_mixdown_gated(plan.handle, C.addressof(gate), form, bench.d.data_ptr(), ROWS, bench.lv.data_ptr(), ref[form].data_ptr(), _stream()) == 0
                    torch.cuda.synchronize()
                    assert got.tobytes() == ref[form].cpu().numpy().tobytes(), (t, n, form, f)
                    assert got.tobytes() == levels.mix_gated(x[f], off, row, gain, form, t, n).tobytes(), (t, n, form, f)
        # open_peak = 0, loudest_n = 0: the bytes of mbx_mixdown from the second frame on, from the first if ramp_log2 = 0
        for h in ((0, 0, 0, 0, 0), (0, 0, 5, 0, 3), (0, 0, 0, 0, 7)):
            for form in mixdown.FORMS:
                state.reset(_stream())
                for f in range(3):
                    bench.frame(x[f])
                    got = bench.held(plan, h, state, form)
                    assert L.mbx_mixdown(plan.handle, form, bench.d.data_ptr(), ROWS, ref[form].data_ptr(), _stream()) == 0
                    torch.cuda.synchronize()
                    same = got.tobytes() == ref[form].cpu().numpy().tobytes()
                    assert same == (f > 0 or h[4] == 0), (h, form, f)
                assert state.get(_stream())["on"].all()


# ---- a hold that changes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("above", [None, 4096], ids=["default-split", "all-short"])
def test_a_hold_that_changes_mid_script_makes_hundreds_of_inputs_fall_at_once(mbx, above):
    """loudest_n 0 -> 3 -> 0 at ramp_log2 = 3 and 7: in the frame of the change all but 3 of the inputs that were on in the 4,096 bus
    fall, in the long form and in the short one"""
    x, off, row, gain, sizes = H.script()
    bench = _Bench(len(sizes))
    big = sizes.index(4096)
    with mixdown.Plan(off, row, gain, long_above=above) as plan, hold.GateState(plan) as state:
        for ramp, form in ((3, mixdown.PCM16), (7, mixdown.ULAW)):
            holds = [(H.OPEN, H.CLOSE, H.HANG, n, ramp) for n in (0, 0, 0, 3, 3, 3, 0, 0, 1, 8, 0, 0)]
            steps = H.run(holds, form)
            fell = hold.codes(steps[2][1], steps[3][1])[off[big]:off[big + 1]]
            assert (fell == hold.FALLING).sum() > 300, "the script lets several hundred inputs fall at once"
            state.reset(_stream())
            for f, (want_out, want_state) in enumerate(steps):
                bench.frame(x[f])
                got = bench.held(plan, holds[f], state, form)
                bad = np.flatnonzero((got != want_out).any(axis=1))
                assert got.tobytes() == want_out.tobytes(), (above, ramp, f, "buses", bad[:8], "of sizes", [sizes[b] for b in bad[:8]])
                assert state.get(_stream()).tobytes() == want_state.tobytes(), (above, ramp, f)


# ---- the state calls -----------------------------------------------------------------------------------------------------------------------
def test_reset_set_and_get_and_the_refusals_that_need_a_plan(mbx):
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    x, off, row, gain, sizes = H.script()
    bench = _Bench(len(sizes))
    h = (H.OPEN, H.CLOSE, H.HANG, 3, 3)
    with mixdown.Plan(off, row, gain) as plan, mixdown.Plan(off, row, gain) as twin, hold.GateState(plan) as state, hold.GateState(twin) as other:
        want = H.expected(h, mixdown.PCM16)
        for f in range(3):
            bench.frame(x[f])
            bench.held(plan, h, state, mixdown.PCM16)
        assert state.get(_stream()).tobytes() == want[2][1].tobytes() and want[2][1]["on"].any()
        # set: the state after frame 5, then frame 6 -- the state and the bytes of frame 6
        state.set(want[5][1], _stream())
        assert state.get(_stream()).tobytes() == want[5][1].tobytes()
        bench.frame(x[6])
        assert bench.held(plan, h, state, mixdown.PCM16).tobytes() == want[6][0].tobytes()
        assert state.get(_stream()).tobytes() == want[6][1].tobytes()
        # reset: closed, and the script from its start again
        state.reset(_stream())
        assert not state.get(_stream()).view(np.uint32).any()
        bench.frame(x[0])
        assert bench.held(plan, h, state, mixdown.PCM16).tobytes() == want[0][0].tobytes()
        before = state.get(_stream())

        def refused(part, call, *args):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert call(*args) == INVALID, part
            assert part in L.mbx_last_error(), L.mbx_last_error()

        # a bad record: nothing is written
        for record in ((0, 2, 0), (0, 1, 2), (3, 0, 1)):
            wrong = before.copy()
            wrong[off[-1] - 1] = record
            refused(b"mbx_gate_state_set: a state record", L.mbx_gate_state_set, state.handle, wrong.ctypes.data, _stream())
        assert state.get(_stream()).tobytes() == before.tobytes()
        # a state of another plan, although the plans are twins; and what the launcher refuses with a plan in hand
        ptrs = (bench.d.data_ptr(), ROWS, bench.lv.data_ptr(), bench.out[0].data_ptr())
        bench.out[0].fill_(0x5A5A)   # (int16: FILL in either byte)
        for part, args in ((b"mbx_mixdown_held: the state was made for another plan", (plan, h, other, 0, *ptrs)),
                           (b"mbx_mixdown_held: the state was made for another plan", (twin, h, state, 0, *ptrs)),
                           (b"state is needed", (plan, h, None, 0, *ptrs)), (b"hold is needed", (plan, None, state, 0, *ptrs)),
                           (b"close_peak", (plan, (500, 501, 0, 0, 0), state, 0, *ptrs)), (b"MBX_HOLD_MAX_RAMP_LOG2", (plan, (900, 500, 0, 0, 8), state, 0, *ptrs)),
                           (b"MBX_GATE_MAX_LOUDEST", (plan, (900, 500, 0, 9, 0), state, 0, *ptrs)), (b"32768", (plan, (32769, 0, 0, 0, 0), state, 0, *ptrs)),
                           (b"nrows", (plan, h, state, 0, ptrs[0], ROWS - 1, *ptrs[2:])), (b"form", (plan, h, state, 3, *ptrs)),
                           (b"alignment", (plan, h, state, 0, ptrs[0] + 8, *ptrs[1:])), (b"d_levels overlaps", (plan, h, state, 0, ptrs[0], ROWS, ptrs[0] + 16, ptrs[3]))):
            refused(part, _held, *args)
        torch.cuda.synchronize()
        assert _untouched(bench.out[0].cpu().numpy()), "a refused call launched something"
        assert state.get(_stream()).tobytes() == before.tobytes() and not other.get(_stream()).view(np.uint32).any(), "a refused call advanced a state"
        assert L.mbx_gate_state_inputs(state.handle) == off[-1]
    # a plan without inputs has a state without records
    with mixdown.Plan([0, 0, 0], [], None) as empty, hold.GateState(empty) as none:
        assert none.inputs == 0 and none.get(_stream()).size == 0
        none.reset(_stream())
        none.set(hold.zero_state(0), _stream())
        out = torch.full((2, 160), FILL, dtype=torch.uint8, device="cuda")
        assert _held(empty, h, none, mixdown.ALAW, bench.d.data_ptr(), ROWS, bench.lv.data_ptr(), out.data_ptr()) == 0
        torch.cuda.synchronize()
        assert (out.cpu().numpy() == 0xD5).all()


# ---- a graph -------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_graph_replayed_over_three_frames_advances_the_state_three_frames(mbx):
    """the levels launch and the held launches behind it (both kernel forms), captured once on a side stream; new rows are loaded into
    the same buffer between the replays.  Nothing about the state was decided on the host at capture time."""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    x, off, row, gain, sizes = H.script()
    h = (H.OPEN, H.CLOSE, H.HANG, 3, 3)
    hd = H.hold_of(h)
    want = H.expected(h, mixdown.PCM16)
    d = torch.zeros((ROWS, 160), dtype=torch.int16, device="cuda")
    lv = torch.full((ROWS, 16), FILL, dtype=torch.uint8, device="cuda")
    out = torch.full((len(sizes), 160), FILL, dtype=torch.int16, device="cuda")
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with mixdown.Plan(off, row, gain) as plan, hold.GateState(plan) as state:
        assert 0 < plan.long_buses < plan.buses
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc1 = L.mbx_pcm_levels(d.data_ptr(), ROWS, lv.data_ptr(), side.cuda_stream)
            rc2 = L.mbx_mixdown_held(plan.handle, C.addressof(hd), state.handle, mixdown.PCM16, d.data_ptr(), ROWS, lv.data_ptr(), out.data_ptr(), side.cuda_stream)
        assert rc1 == 0 and rc2 == 0, L.mbx_last_error()
        torch.cuda.synchronize()
        assert not state.get(_stream()).view(np.uint32).any(), "a capture runs nothing"
        for f in range(3):
            d.copy_(torch.from_numpy(x[f].copy()))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert lv.cpu().numpy().tobytes() == levels.measure(x[f]).tobytes()
            assert out.cpu().numpy().tobytes() == want[f][0].tobytes(), f
            assert state.get(_stream()).tobytes() == want[f][1].tobytes(), f


# ---- behind a decode -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1])
def test_behind_three_decodes_the_held_buses_are_those_of_their_pcm16(mbx, codec):
    import torch
    from mbelib_neo_amd import decoder

    T = 2
    dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) * 7 + 3)
    plans = _Plans()
    try:
        plan, off, row, gain = plans.of(S * T)
        h = (H.OPEN, H.CLOSE, 1, 3, 5)
        with hold.GateState(plan) as state:
            steps = []
            for k in range(3):
                out = dec.decode(edge_mix.frames(codec, S, T, 1 + k).reshape(S * T, -1), T)
                form = mixdown.FORMS[k]
                steps.append((form, out["pcm16"], dec.mixdown_held(out["pcm16"], plan, state, H.hold_of(h), form)))   # on the decode's stream
            torch.cuda.synchronize()
            st = hold.zero_state(off[-1])
            seen = set()
            for k, (form, pcm16, got) in enumerate(steps):
                pcm16 = pcm16.cpu().numpy()
                assert len(np.unique(pcm16)) > 100, "the decode gave no audio to mix"
                before = st
                want, st = hold.step(pcm16, off, row, gain, form, h, st)
                seen |= set(hold.codes(before, st).tolist())
                assert got.cpu().numpy().tobytes() == want.tobytes(), (codec, k)
            assert state.get(_stream()).tobytes() == st.tobytes()
            assert {hold.STEADY, hold.RISING} <= seen, "the decodes opened no gate"
            with pytest.raises(Exception, match="MBX_HOLD_MAX_RAMP_LOG2"):
                dec.mixdown_held(steps[0][1], plan, state, hold.Hold(900, 500, 0, 0, 8))
    finally:
        plans.close()


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
def _next_held(L, s, plan, form, h, state, buses):
    hd = None if h is None else H.hold_of(h)
    return L.mbx_session_next_mixdown_held(s, plan.handle if plan is not None else None, form, None if hd is None else C.addressof(hd),
                                           state.handle if state is not None else None, None if buses is None else buses.ctypes.data)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_four_submits_in_flight_advance_the_state_in_submit_order(mbx, pinned):
    """four submits of one frame before the first wait, form and hold changing; the buses of each are numpy's of the int16 PCM the same
    submit delivered, under the state the submits before it left"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec = 0
    a = _session(L, codec, S, S * 2, PCM16 | MIX | LEVELS)
    host, plans = _Host(L, pinned), _Plans()
    try:
        plan, off, row, gain = plans.of(S)
        with hold.GateState(plan) as state:
            steps = []
            for k in range(4):
                frames = np.ascontiguousarray(edge_mix.frames(codec, S, 1, 2 + k).reshape(S, -1))
                form, h = mixdown.FORMS[k % 3], (H.OPEN, H.CLOSE, 1, (3, 3, 0, 1)[k], (3, 7, 0, 3)[k])
                pcm16, buses = host.array((S, 160), np.int16), host.array((13, 160), mixdown.out_dtype(form))
                _native.check(_next_held(L, a, plan, form, h, state, buses), "next_mixdown_held")
                _native.check(L.mbx_session_submit(a, 1, frames.ctypes.data, pcm16.ctypes.data, None, None), "submit")
                steps.append((form, h, pcm16, buses))
            _native.check(L.mbx_session_wait(a), "wait")
            st = hold.zero_state(off[-1])
            for k, (form, h, pcm16, buses) in enumerate(steps):
                assert len(np.unique(pcm16)) > 100, k
                want, st = hold.step(pcm16, off, row, gain, form, h, st)
                assert buses.tobytes() == want.tobytes(), f"submit {k}"
            assert state.get(None).tobytes() == st.tobytes() and st["on"].any()
    finally:
        L.mbx_session_destroy(a)
        host.close()
        plans.close()


def test_the_attachment_lasts_one_submit_and_a_refused_submit_leaves_the_state_untouched(mbx):
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec = 0
    frames = {T: np.ascontiguousarray(edge_mix.frames(codec, S, T, 30 + T).reshape(S * T, -1)) for T in (1, 3)}
    sessions = {bits: _session(L, codec, S, S * 2, bits) for bits in (PCM16, PCM16 | MIX, PCM16 | LEVELS, PCM16 | MIX | LEVELS)}
    both = sessions[PCM16 | MIX | LEVELS]
    plans = _Plans()
    try:
        p1, *csr1 = plans.of(S)
        p2, *csr2 = plans.of(S * 2)
        h = (H.OPEN, H.CLOSE, 2, 3, 3)
        with hold.GateState(p1) as state, hold.GateState(p2) as state2:
            def submit(s, T, pcm16):
                return L.mbx_session_submit(s, T, frames[T].ctypes.data, pcm16.ctypes.data, None, None)

            def fresh():
                return np.full((13, 160), 0x5A5A, np.int16)

            def refused(part, *args):
                L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
                assert _next_held(L, *args) == INVALID, part
                assert b"mbx_session_next_mixdown_held: " + part in L.mbx_last_error(), L.mbx_last_error()

            buses, pcm16 = fresh(), np.zeros((S * 2, 160), np.int16)
            refused(b"the session was created without MBX_SESSION_LEVELS", sessions[PCM16 | MIX], p1, 0, h, state, buses)
            for bits in (PCM16, PCM16 | LEVELS):
                refused(b"the session was created without MBX_SESSION_MIXDOWN", sessions[bits], p1, 0, h, state, buses)
            refused(b"a hold is needed", both, p1, 0, None, state, buses)
            refused(b"close_peak is above open_peak", both, p1, 0, (500, 501, 0, 0, 0), state, buses)
            refused(b"open_peak is above 32768", both, p1, 0, (32769, 0, 0, 0, 0), state, buses)
            refused(b"loudest_n is above MBX_GATE_MAX_LOUDEST", both, p1, 0, (900, 500, 0, 9, 0), state, buses)
            refused(b"ramp_log2 is above MBX_HOLD_MAX_RAMP_LOG2", both, p1, 0, (900, 500, 0, 0, 8), state, buses)
            refused(b"a state is needed", both, p1, 0, h, None, buses)
            refused(b"the state was made for another plan", both, p1, 0, h, state2, buses)
            refused(b"form", both, p1, 3, h, state, buses)
            refused(b"no plan", both, None, 0, h, state, buses)
            assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)   # none of them left anything
            assert not state.get(None).view(np.uint32).any()
            # queued: delivered once and the state advanced once; the submit after it delivers nothing and leaves the state
            _native.check(_next_held(L, both, p1, 0, h, state, buses), "next_mixdown_held")
            assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0
            want, st = hold.step(pcm16[:S], *csr1, 0, h, hold.zero_state(csr1[0][-1]))
            assert buses.tobytes() == want.tobytes() and state.get(None).tobytes() == st.tobytes() and st["on"].any()
            buses = fresh()
            assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
            assert state.get(None).tobytes() == st.tobytes()
            # refused (T beyond max_frames_per_submit; rows short of the plan): used up, nothing queued, the state as it was
            for T_bad, plan, its in ((3, p1, state), (1, p2, state2)):
                was = its.get(None)
                _native.check(_next_held(L, both, plan, 0, h, its, buses), "next_mixdown_held")
                assert submit(both, T_bad, pcm16) == INVALID
                assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
                assert its.get(None).tobytes() == was.tobytes()
            # whichever of the three mix-down calls came last holds the buses slot
            gate = levels.Gate(0, 1)
            _native.check(_next_held(L, both, p1, 0, h, state, buses), "next_mixdown_held")
            _native.check(L.mbx_session_next_mixdown(both, p1.handle, 0, buses.ctypes.data), "next_mixdown")
            assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0
            assert buses.tobytes() == mixdown.mix(pcm16[:S], *csr1, 0).tobytes() and state.get(None).tobytes() == st.tobytes()
            _native.check(_next_held(L, both, p1, 0, h, state, buses), "next_mixdown_held")
            _native.check(L.mbx_session_next_mixdown_gated(both, p1.handle, 0, C.addressof(gate), buses.ctypes.data), "next_mixdown_gated")
            assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0
            assert buses.tobytes() == levels.mix_gated(pcm16[:S], *csr1, 0, 0, 1).tobytes() and state.get(None).tobytes() == st.tobytes()
            for first in ("plain", "gated"):
                if first == "plain":
                    _native.check(L.mbx_session_next_mixdown(both, p1.handle, 0, buses.ctypes.data), "next_mixdown")
                else:
                    _native.check(L.mbx_session_next_mixdown_gated(both, p1.handle, 0, C.addressof(gate), buses.ctypes.data), "next_mixdown_gated")
                bytes_ = np.full((13, 160), FILL, np.uint8)
                _native.check(_next_held(L, both, p1, 2, h, state, bytes_), "next_mixdown_held")
                assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0
                want, st = hold.step(pcm16[:S], *csr1, 2, h, st)
                assert bytes_.tobytes() == want.tobytes() and state.get(None).tobytes() == st.tobytes(), first
            # a NULL out clears it
            buses = fresh()
            _native.check(_next_held(L, both, p1, 0, h, state, buses), "next_mixdown_held")
            assert _next_held(L, both, p1, 0, h, state, None) == 0
            assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
            assert state.get(None).tobytes() == st.tobytes()
    finally:
        for s in sessions.values():
            L.mbx_session_destroy(s)
        plans.close()
