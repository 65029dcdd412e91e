"""GPU suite (-m gpu) for levels out and the gated mix-down (include/mbx_levels.h): mbx_pcm_levels held byte for byte to the numpy
definition (mbelib_neo_amd.levels.measure) over row counts on either side of every rows-per-wave and workgroup boundary, between guard
bands at exactly the alignment of its contract; mbx_mixdown_gated held to levels.mix_gated through both kernel forms, the three output
forms, gates of every kind and bus sizes around N, the split and a workgroup, with ties; the launcher's refusals that need a plan;
both behind a decode; and the sessions' mbx_session_next_levels / mbx_session_next_mixdown_gated held to numpy of the int16 PCM the
same submit (or a twin session without the flags) delivered, with the rules of the attachments.  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import burst_cases
import burst_group_cases as G
import edge_mix
import guarded
from mbelib_neo_amd import levels, mixdown, pcm8
from test_gpu_mixdown import FILL, INVALID, S, _Host, _Plans, _session, _untouched

pytestmark = pytest.mark.gpu

PCM16, PCM8, MIX, LEVELS = 1, pcm8.SESSION_PCM8, mixdown.SESSION_MIXDOWN, levels.SESSION_LEVELS
T_OPEN = 900   # the peak gate of most cases: between the quiet and the loud rows of _rows
GATES = [(0, 0), (T_OPEN, 0)] + [(t, n) for n in (1, 3, 8) for t in (0, T_OPEN)]
# 0, 1, 2, N - 1, N, N + 1 for N = 1, 3, 8; either side of the default split (22), of a workgroup of keys (256) and the most
SIZES = [0, 1, 2, 3, 4, 7, 8, 9, 22, 23, 24, 255, 256, 257, 4096]
ROWS = 300


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _rows(rng, rows):
    """rows of very different loudness, full-range ones among them; planted extremes at the first and the last position and behind the
    first: all -32768, all 0, a single 32767, +-1"""
    scale = rng.choice(np.array([3, 40, 700, 5000, 32768]), size=rows)
    x = (rng.integers(-32768, 32768, size=(rows, 160), dtype=np.int64) * scale[:, None] // 32768).astype(np.int16)
    planted = [np.full(160, -32768), np.zeros(160), np.eye(1, 160, 77)[0] * 32767, np.where(np.arange(160) & 1, -1, 1)]
    for r, p in zip((0, rows - 1, 1, 2)[:min(rows, 4)], planted):
        x[r] = p.astype(np.int16)
    return x


def _gate(peak, n):
    return levels.Gate(peak, n)


def _levels(in_ptr, nrows, out_ptr):
    import torch
    from mbelib_neo_amd import _native

    return _native.lib().mbx_pcm_levels(in_ptr, nrows, out_ptr, torch.cuda.current_stream().cuda_stream)


def _gated(plan, gate, form, in_ptr, nrows, lv_ptr, out_ptr):
    import torch
    from mbelib_neo_amd import _native

    return _native.lib().mbx_mixdown_gated(plan.handle if plan is not None else None, C.addressof(gate) if gate is not None else None, form, in_ptr, nrows,
                                           lv_ptr, out_ptr, torch.cuda.current_stream().cuda_stream)


# ---- levels --------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows", [1, 2, 3, 4, 5, 7, 8, 9, 63, 64, 65, 257])
def test_the_records_are_byte_for_byte_those_of_numpy_between_guard_bands(mbx, rows):
    """4 rows are a wave and 16 a workgroup of pcm_levels_kernel (3 and 12 under the other partition); rows and records at 16 bytes and no
    better, the rows read-only, guard bands of tests/guarded.py on every side"""
    import torch

    x = _rows(np.random.default_rng(rows), rows)
    want = levels.measure(x)
    arena = guarded.Arena([guarded.buf("pcm16", 320 * rows, "stage", True), guarded.buf("levels", 16 * rows, "stage")], where="cuda", seed=rows)
    assert arena.ptr("pcm16") % 32 == 16 and arena.ptr("levels") % 32 == 16
    arena.load("pcm16", x)
    arena.prefill("levels")
    assert _levels(arena.ptr("pcm16"), rows, arena.ptr("levels")) == 0
    torch.cuda.synchronize()
    arena.check(f"{rows} rows")
    got = arena.read("levels").view(levels.LEVEL_DTYPE)
    bad = np.flatnonzero(got != want)
    assert got.tobytes() == want.tobytes(), (bad[:8], got[bad[:4]], want[bad[:4]])
    assert want["peak"][0] == 32768 and want["clipped"][0] == 160 and want["energy"][0] == 160 << 30, "the planted first row"
    if rows > 1:
        assert want["energy"][-1] == 0, "the planted last row"
    # no rows: nothing is launched, nothing is written
    arena.prefill("levels")
    assert _levels(arena.ptr("pcm16"), 0, arena.ptr("levels")) == 0
    torch.cuda.synchronize()
    arena.check("no rows")
    assert arena.read("levels").tobytes() == arena.prefill_bytes("levels").tobytes()


# ---- the gated mix-down --------------------------------------------------------------------------------------------------------------------
_CASE = {}


def _case():
    """ROWS rows, one bus of every size of SIZES and the tie buses behind them, and numpy's answer for every gate and form: made once and
    shared (read-only).  Rows 3 .. 9 are quiet (peaks below T_OPEN), row 10 is row 11 negated, row 12 is loud."""
    if not _CASE:
        rng = np.random.default_rng(2024)
        x = _rows(rng, ROWS)
        x[3:10] = rng.integers(-T_OPEN + 1, T_OPEN, size=(7, 160))
        x[11] = np.clip(x[11], -32767, 32767)
        x[10] = -x[11]
        x[12] = rng.integers(-30000, 30001, size=160)
        sizes = list(SIZES)
        row = [rng.integers(0, ROWS, size=n).tolist() for n in sizes]
        ties = [[12] * 6,                                    # one row repeated
                [10, 11], [11, 10, 5],                       # a row beside its negation, either first
                [40, 12, 12, 41, 12, 12, 12, 12, 12, 12, 12, 12, 42],   # more than N inputs share the top energy, for every N
                [3, 4, 5, 6, 7, 8, 9] * 4]                   # quiet rows only: closed by T_OPEN, 28 inputs (long by default)
        row += ties
        sizes += [len(t) for t in ties]
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
        row = np.array([r for bus in row for r in bus], dtype=np.int32)
        row[off[SIZES.index(4096)] + 4095] = ROWS - 1
        gain = rng.integers(-5000, 5001, size=row.size, dtype=np.int64).astype(np.int16)
        gain[rng.integers(0, row.size, size=200)] = rng.choice(np.array([-32768, 32767, 4096, 0], dtype=np.int16), size=200)
        gain[off[len(SIZES)]:] = 4096   # the tie buses at unity
        want = {(gate, form): levels.mix_gated(x, off, row, gain, form, *gate) for gate in GATES for form in mixdown.FORMS}
        lv = levels.measure(x)
        for a in (x, off, row, gain, lv, *want.values()):
            a.setflags(write=False)
        # the cases decide something: the peak gate closes inputs, the ranking drops open ones, the quiet bus is silent under T_OPEN
        taken = {gate: levels.chosen(lv, off, row, *gate) for gate in GATES}
        assert taken[0, 0].all() and 0 < taken[T_OPEN, 0].sum() < row.size and taken[T_OPEN, 3].sum() < taken[0, 3].sum() < taken[0, 8].sum()
        quiet = len(sizes) - 1
        assert not want[(T_OPEN, 0), mixdown.PCM16][quiet].any() and want[(0, 0), mixdown.PCM16][quiet].any()
        assert (want[(T_OPEN, 3), mixdown.ULAW][quiet] == 0xFF).all() and (want[(T_OPEN, 8), mixdown.ALAW][quiet] == 0xD5).all()
        _CASE["it"] = (x, off, row, gain, want, sizes)
    return _CASE["it"]


@pytest.mark.parametrize("above", [None, 4096, 1], ids=["default-split", "all-short", "all-long"])
def test_both_kernel_forms_give_the_bytes_of_the_numpy_definition_under_every_gate(mbx, above):
    """the default split (22), every bus short (long_above = 4096), and every bus of two inputs or more long (long_above = 1: the plan
    has no way to make a bus of one input long); three forms, eight gates; {0, 0} also against mbx_mixdown's bytes"""
    import torch
    from mbelib_neo_amd import _native

    x, off, row, gain, want, sizes = _case()
    n_buses = len(sizes)
    d = torch.from_numpy(x.copy()).cuda()
    lv = torch.full((ROWS, 16), FILL, dtype=torch.uint8, device="cuda")
    assert _levels(d.data_ptr(), ROWS, lv.data_ptr()) == 0
    with mixdown.Plan(off, row, gain, long_above=above) as plan:
        assert plan.long_buses == {None: sum(s > 22 for s in sizes), 4096: 0, 1: sum(s > 1 for s in sizes)}[above]
        for form in mixdown.FORMS:
            dtype = torch.int16 if form == mixdown.PCM16 else torch.uint8
            for gate in GATES:
                out = torch.full((n_buses, 160), FILL, dtype=dtype, device="cuda")
                assert _gated(plan, _gate(*gate), form, d.data_ptr(), ROWS, lv.data_ptr(), out.data_ptr()) == 0, _native.lib().mbx_last_error()
                torch.cuda.synchronize()
                got = out.cpu().numpy()
                bad = np.flatnonzero((got != want[gate, form]).any(axis=1))
                assert got.tobytes() == want[gate, form].tobytes(), (above, form, gate, "buses", bad[:8], "of sizes", [sizes[b] for b in bad[:8]])
            plain = torch.full((n_buses, 160), FILL, dtype=dtype, device="cuda")
            assert _native.lib().mbx_mixdown(plan.handle, form, d.data_ptr(), ROWS, plain.data_ptr(), torch.cuda.current_stream().cuda_stream) == 0
            torch.cuda.synchronize()
            assert plain.cpu().numpy().tobytes() == want[(0, 0), form].tobytes(), "a gate {0, 0} gives the bytes of mbx_mixdown"
    assert np.array_equal(d.cpu().numpy(), x)
    assert lv.cpu().numpy().tobytes() == levels.measure(x).tobytes()


def test_open_peak_at_exactly_a_rows_peak_opens_it_and_one_above_closes_it(mbx):
    import torch

    x, *_ = _case()
    lvn = levels.measure(x)
    d = torch.from_numpy(x.copy()).cuda()
    lv = torch.from_numpy(lvn.view(np.uint8).reshape(-1, 16).copy()).cuda()
    r = 12
    peak = int(lvn["peak"][r])
    assert 0 < peak < 32768
    off, row = np.array([0, 1, 25], dtype=np.int32), np.array([r] * 25, dtype=np.int32)   # a short and a long bus of that row
    with mixdown.Plan(off, row, None) as plan:
        assert plan.long_buses == 1
        for form in mixdown.FORMS:
            for p, n in ((peak, 0), (peak + 1, 0), (peak, 1), (peak + 1, 1), (32768, 0)):
                out = torch.full((2, 160), FILL, dtype=torch.int16 if form == mixdown.PCM16 else torch.uint8, device="cuda")
                assert _gated(plan, _gate(p, n), form, d.data_ptr(), ROWS, lv.data_ptr(), out.data_ptr()) == 0
                torch.cuda.synchronize()
                got, want = out.cpu().numpy(), levels.mix_gated(x, off, row, None, form, p, n)
                assert got.tobytes() == want.tobytes(), (form, p, n)
                if p > peak:
                    assert (got == (0, 0xFF, 0xD5)[form]).all(), "every input closed: the form's silence"
                elif form == mixdown.PCM16:
                    assert got[0].tobytes() == x[r].tobytes()


def test_the_launcher_refuses_what_only_a_plan_can_tell(mbx):
    """with a plan in hand: nrows below the rows it needs, the overlaps, pointers below their alignment, the gate; nothing is launched"""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    rows, n_buses = 64, 3
    off, row = np.array([0, 2, 2, 30], dtype=np.int32), np.concatenate([[63, 0], np.arange(28)]).astype(np.int32)
    mem = torch.full((rows * 320 + rows * 16 + n_buses * 320 + 64,), FILL, dtype=torch.uint8, device="cuda")
    base = (mem.data_ptr() + 15) & ~15
    lv, out = base + rows * 320, base + rows * 320 + rows * 16
    ok = _gate(0, 3)
    with mixdown.Plan(off, row, None) as plan:
        assert plan.rows == rows and plan.long_buses == 1

        def refused(part, gate, form, in_ptr, nrows, lv_ptr, out_ptr, p=plan):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert _gated(p, gate, form, in_ptr, nrows, lv_ptr, out_ptr) == INVALID, part
            assert b"mbx_mixdown_gated:" in L.mbx_last_error() and part in L.mbx_last_error(), L.mbx_last_error()

        refused(b"nrows", ok, 0, base, rows - 1, lv, out)
        refused(b"d_pcm16 and d_out overlap", ok, 0, base, rows, lv, base + 320)
        refused(b"d_levels overlaps", ok, 0, base, rows, base + 16, out)
        refused(b"d_levels overlaps", ok, 0, base, rows, lv - 16, out)
        refused(b"d_levels overlaps", ok, 0, base, rows, out + 16, out)
        refused(b"d_levels overlaps", ok, 1, base, rows, out + n_buses * 160 - 16, out)
        refused(b"d_levels overlaps", ok, 0, base, rows + 1, lv, out)      # the caller's rows count, read or not: the 65th row lies in d_levels
        refused(b"alignment", ok, 0, base + 8, rows, lv, out)
        refused(b"alignment", ok, 0, base, rows, lv + 8, out)
        refused(b"alignment", ok, 0, base, rows, lv, out + 8)
        refused(b"alignment", ok, 2, base, rows, lv, out + 4)
        refused(b"form", ok, 3, base, rows, lv, out)
        refused(b"gate is needed", None, 0, base, rows, lv, out)
        refused(b"MBX_GATE_MAX_LOUDEST", _gate(0, 9), 0, base, rows, lv, out)
        refused(b"32768", _gate(32769, 0), 0, base, rows, lv, out)
        refused(b"needed", ok, 0, base, rows, lv, out, p=None)
        L.mbx_stage_in(0x1008, 0x1000, 16, None)
        assert _levels(base, rows, base + 320) == INVALID and b"mbx_pcm_levels:" in L.mbx_last_error() and b"overlap" in L.mbx_last_error()
        torch.cuda.synchronize()
        assert (mem.cpu().numpy() == FILL).all(), "a refused call launched something"
        assert _levels(base, rows, lv) == 0 and _gated(plan, _gate(32768, 8), 1, base, rows, lv, out + 8) == 0   # the limits of the gate, bytes at 8
        torch.cuda.synchronize()


@pytest.mark.parametrize("codec", [0, 1])
def test_behind_a_decode_the_levels_and_the_gated_buses_are_those_of_its_pcm16(mbx, codec):
    import torch
    from mbelib_neo_amd import decoder

    T = 3
    dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) * 7 + 3)
    plans = _Plans()
    try:
        plan, off, row, gain = plans.of(S * T)
        out = dec.decode(edge_mix.frames(codec, S, T, 1).reshape(S * T, -1), T)
        lv = dec.levels(out["pcm16"])   # on the decode's stream, no synchronisation between
        buses = {(gate, form): dec.mixdown_gated(out["pcm16"], plan, form, *gate, levels=lv) for gate in GATES[1:5] for form in mixdown.FORMS}
        own = dec.mixdown_gated(out["pcm16"], plan, mixdown.ALAW, 0, 3)   # ... measuring for itself
        torch.cuda.synchronize()
        pcm16 = out["pcm16"].cpu().numpy()
        want = levels.measure(pcm16)
        assert len(np.unique(pcm16)) > 100 and len(np.unique(want["peak"])) > 10, "the decode gave no audio to measure"
        assert lv.cpu().numpy().tobytes() == want.tobytes()
        for (gate, form), got in buses.items():
            assert got.cpu().numpy().tobytes() == levels.mix_gated(pcm16, off, row, gain, form, *gate).tobytes(), (gate, form)
        assert own.cpu().numpy().tobytes() == levels.mix_gated(pcm16, off, row, gain, mixdown.ALAW, 0, 3).tobytes()
        with pytest.raises(ValueError):
            dec.levels(out["pcm16"].to(torch.int32))
        with pytest.raises(Exception, match="MBX_GATE_MAX_LOUDEST"):
            dec.mixdown_gated(out["pcm16"], plan, 0, 0, 9)
    finally:
        plans.close()


def test_the_two_launches_are_captured_into_a_graph_and_replayed(mbx):
    """plain launches on the caller's stream: the levels launch and the gated launches behind it (both kernel forms), captured once on a
    side stream and replayed on other rows in the same buffers"""
    import torch

    x, off, row, gain, want, sizes = _case()
    d = torch.zeros((ROWS, 160), dtype=torch.int16, device="cuda")
    lv = torch.full((ROWS, 16), FILL, dtype=torch.uint8, device="cuda")
    out = torch.full((len(sizes), 160), FILL, dtype=torch.int16, device="cuda")
    gate = _gate(T_OPEN, 3)
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with mixdown.Plan(off, row, gain) as plan:
        from mbelib_neo_amd import _native

        L = _native.lib()
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc1 = L.mbx_pcm_levels(d.data_ptr(), ROWS, lv.data_ptr(), side.cuda_stream)
            rc2 = L.mbx_mixdown_gated(plan.handle, C.addressof(gate), mixdown.PCM16, d.data_ptr(), ROWS, lv.data_ptr(), out.data_ptr(), side.cuda_stream)
        assert rc1 == 0 and rc2 == 0, L.mbx_last_error()
        other = np.ascontiguousarray(x[::-1])
        for rows_now in (x, other):
            d.copy_(torch.from_numpy(rows_now.copy()))
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert lv.cpu().numpy().tobytes() == levels.measure(rows_now).tobytes()
            expect = want[(T_OPEN, 3), mixdown.PCM16] if rows_now is x else levels.mix_gated(other, off, row, gain, mixdown.PCM16, T_OPEN, 3)
            assert out.cpu().numpy().tobytes() == expect.tobytes()


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
def _next_gated(L, h, plan, form, gate, buses):
    g = _gate(*gate)
    return L.mbx_session_next_mixdown_gated(h, plan.handle, form, C.addressof(g), None if buses is None else buses.ctypes.data)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_three_submits_in_flight_deliver_the_records_and_the_gated_buses_of_their_own_pcm16(mbx, pinned):
    """T = 1, 2, 1 before the first wait, form and gate changing; the third takes no pcm16 (NULL) and is held to a twin session without
    the flags; the second carries records only"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec = 0
    a, b = _session(L, codec, S, S * 2, PCM16 | MIX | LEVELS), _session(L, codec, S, S * 2, PCM16)
    host, plans = _Host(L, pinned), _Plans()
    try:
        steps = []
        for k, T in enumerate((1, 2, 1)):
            frames = np.ascontiguousarray(edge_mix.frames(codec, S, T, 2 + k).reshape(S * T, -1))
            form, gate = mixdown.FORMS[k], ((T_OPEN, 3), None, (0, 1))[k]
            plan, off, row, gain = plans.of(S * T)
            own16 = host.array((S * T, 160), np.int16) if k < 2 else None
            records, twin16 = host.array((S * T,), levels.LEVEL_DTYPE), np.zeros((S * T, 160), np.int16)
            buses = host.array((13, 160), mixdown.out_dtype(form)) if gate else None
            _native.check(L.mbx_session_next_levels(a, records.ctypes.data), "next_levels")
            if gate:
                _native.check(_next_gated(L, a, plan, form, gate, buses), "next_mixdown_gated")
            _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, None if own16 is None else own16.ctypes.data, None, None), "submit")
            _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin16.ctypes.data, None, None), "submit (twin)")
            steps.append((form, gate, own16, records, buses, twin16, (off, row, gain)))
        _native.check(L.mbx_session_wait(a), "wait")
        _native.check(L.mbx_session_wait(b), "wait (twin)")
        for k, (form, gate, own16, records, buses, twin16, csr) in enumerate(steps):
            assert len(np.unique(twin16)) > 100, k
            if own16 is not None:
                assert own16.tobytes() == twin16.tobytes(), f"submit {k}: pcm16 is no longer what a session without the flags delivers"
            assert records.tobytes() == levels.measure(twin16).tobytes(), f"submit {k}"
            if gate:
                assert buses.tobytes() == levels.mix_gated(twin16, *csr, form, *gate).tobytes(), f"submit {k}"
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)
        host.close()
        plans.close()


def test_frames_indexed_burst_and_burst_group_submits_deliver_both_and_the_bytes_beside_them(mbx):
    """frames (T = 1 and 2), indexed, bursts and burst groups; every other one also carries a pcm8 attachment on the same submit"""
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    codec, F = 0, 2
    h = _session(L, codec, S, S * F, PCM16 | PCM8 | MIX | LEVELS)
    rng = np.random.default_rng(8)
    sched = B.random_schedule(codec, F, F * B.channel_bits(codec) + 120, rng, device=True)
    plans = _Plans()
    count = [0]
    try:
        def run(what, rows, submit):
            k = count[0]
            count[0] += 1
            form, law, gate = mixdown.FORMS[k % 3], k & 1, GATES[1 + k % 7]
            plan, off, row, gain = plans.of(rows)
            pcm16, buses = np.full((rows, 160), 0x5A5A, np.int16), np.full((13, 160), FILL, mixdown.out_dtype(form))
            records = np.full(rows * 16, FILL, np.uint8).view(levels.LEVEL_DTYPE)
            out8 = np.full((rows, 160), FILL, np.uint8)
            _native.check(_next_gated(L, h, plan, form, gate, buses), "next_mixdown_gated")
            _native.check(L.mbx_session_next_levels(h, records.ctypes.data), "next_levels")
            if k % 2:
                _native.check(L.mbx_session_next_pcm8(h, law, out8.ctypes.data), "next_pcm8")
            _native.check(submit(pcm16.ctypes.data), what)
            _native.check(L.mbx_session_wait(h), "wait")
            assert not _untouched(pcm16), what
            assert records.tobytes() == levels.measure(pcm16).tobytes(), what
            assert buses.tobytes() == levels.mix_gated(pcm16, off, row, gain, form, *gate).tobytes(), (what, gate)
            assert out8.tobytes() == pcm8.compand(pcm16, law).tobytes() if k % 2 else _untouched(out8), what

        for T in (1, 2):
            plain = np.ascontiguousarray(edge_mix.frames(codec, S, T, 9 + T).reshape(S * T, -1))
            run(f"frames T={T}", S * T, lambda p: L.mbx_session_submit(h, T, plain.ctypes.data, p, None, None))
        index = np.array([1, 64, 4, 69, 31], dtype=np.int32)
        frames = np.ascontiguousarray(edge_mix.frames(codec, 5, 2, 11).reshape(10, -1))
        run("indexed", 10, lambda p: L.mbx_session_submit_indexed(h, 5, 2, index.ctypes.data, frames.ctypes.data, p, None, None, None))
        carried = edge_mix.frames(codec, S, F, 15).reshape(S * F, -1)
        bursts = np.ascontiguousarray(burst_cases.make_bursts(sched, carried, rng))
        run("bursts", S * F, lambda p: L.mbx_session_submit_bursts(h, sched.handle, S, None, bursts.ctypes.data, sched.burst_bytes, p, None, None))
        shapes = ((codec, F, B.FORM_PACKED, False, 3, 1, 0),)
        scheds = G.schedules(shapes, 17)
        groups = G.make_groups(shapes, scheds, False, 18, tag=2, slots=[np.array([66, 2, 40], dtype=np.int32)])
        arr, keep = G.group_array(L, groups)
        run("burst groups", 3 * F, lambda p: L.mbx_session_submit_burst_groups(h, arr, 1, 0, p, None, None))
        for s in scheds:
            s.close()
    finally:
        L.mbx_session_destroy(h)
        sched.close()
        plans.close()


def test_both_attachments_last_for_one_submit_whether_it_queues_or_refuses(mbx):
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

    L = _native.lib()
    codec = 0
    frames = {T: np.ascontiguousarray(edge_mix.frames(codec, S, T, 30 + T).reshape(S * T, -1)) for T in (1, 2, 3)}
    sessions = {bits: _session(L, codec, S, S * 2, bits) for bits in (PCM16, PCM16 | MIX, PCM16 | LEVELS, PCM16 | MIX | LEVELS, LEVELS)}
    both = sessions[PCM16 | MIX | LEVELS]
    plans = _Plans()
    try:
        p1, *csr1 = plans.of(S)
        p2, *csr2 = plans.of(S * 2)
        ok = _gate(0, 3)

        def submit(h, T, pcm16):
            return L.mbx_session_submit(h, T, frames[T].ctypes.data, None if pcm16 is None else pcm16.ctypes.data, None, None)

        def fresh():
            return np.full((13, 160), 0x5A5A, np.int16), np.full(S * 2 * 16, FILL, np.uint8).view(levels.LEVEL_DTYPE)

        def refused(part, call, *args):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert call(*args) == INVALID
            assert part in L.mbx_last_error(), L.mbx_last_error()

        buses, records = fresh()
        pcm16 = np.zeros((S * 2, 160), np.int16)
        # refusal without the outputs bits, by name
        for bits in (PCM16, PCM16 | MIX):
            refused(b"mbx_session_next_levels: the session was created without MBX_SESSION_LEVELS", L.mbx_session_next_levels, sessions[bits], records.ctypes.data)
        refused(b"mbx_session_next_mixdown_gated: the session was created without MBX_SESSION_LEVELS", L.mbx_session_next_mixdown_gated, sessions[PCM16 | MIX],
                p1.handle, 0, C.addressof(ok), buses.ctypes.data)
        for bits in (PCM16, PCM16 | LEVELS):
            refused(b"mbx_session_next_mixdown_gated: the session was created without MBX_SESSION_MIXDOWN", L.mbx_session_next_mixdown_gated, sessions[bits],
                    p1.handle, 0, C.addressof(ok), buses.ctypes.data)
        nine, loud = _gate(0, 9), _gate(32769, 0)
        refused(b"gate is needed", L.mbx_session_next_mixdown_gated, both, p1.handle, 0, None, buses.ctypes.data)
        refused(b"MBX_GATE_MAX_LOUDEST", L.mbx_session_next_mixdown_gated, both, p1.handle, 0, C.addressof(nine), buses.ctypes.data)
        refused(b"32768", L.mbx_session_next_mixdown_gated, both, p1.handle, 0, C.addressof(loud), buses.ctypes.data)
        refused(b"form", L.mbx_session_next_mixdown_gated, both, p1.handle, 3, C.addressof(ok), buses.ctypes.data)
        refused(b"no plan", L.mbx_session_next_mixdown_gated, both, None, 0, C.addressof(ok), buses.ctypes.data)
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses) and _untouched(records)   # none of them left anything
        # queued: delivered once, and the submit after it delivers nothing
        _native.check(L.mbx_session_next_levels(both, records.ctypes.data), "next_levels")
        _native.check(_next_gated(L, both, p2, 0, (0, 3), buses), "next_mixdown_gated")
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert records.tobytes() == levels.measure(pcm16).tobytes() and buses.tobytes() == levels.mix_gated(pcm16, *csr2, 0, 0, 3).tobytes()
        buses, records = fresh()
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses) and _untouched(records)
        # refused (T beyond max_frames_per_submit; rows short of the plan): used up, nothing queued
        for T_bad, plan in ((3, p1), (1, p2)):
            _native.check(L.mbx_session_next_levels(both, records.ctypes.data), "next_levels")
            _native.check(_next_gated(L, both, plan, 0, (0, 3), buses), "next_mixdown_gated")
            assert submit(both, T_bad, pcm16) == INVALID
            assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses) and _untouched(records)
        # whichever of the two mix-down calls came last holds the buses slot
        _native.check(_next_gated(L, both, p1, 0, (32768, 0), buses), "next_mixdown_gated")
        _native.check(L.mbx_session_next_mixdown(both, p1.handle, 0, buses.ctypes.data), "next_mixdown")
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert buses.tobytes() == mixdown.mix(pcm16[:S], *csr1, 0).tobytes()
        _native.check(L.mbx_session_next_mixdown(both, p1.handle, 0, buses.ctypes.data), "next_mixdown")
        _native.check(_next_gated(L, both, p1, 0, (0, 1), buses), "next_mixdown_gated")
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert buses.tobytes() == levels.mix_gated(pcm16[:S], *csr1, 0, 0, 1).tobytes()
        # NULL clears either, and leaves the other
        buses, records = fresh()
        _native.check(L.mbx_session_next_levels(both, records.ctypes.data), "next_levels")
        _native.check(_next_gated(L, both, p1, 0, (0, 3), buses), "next_mixdown_gated")
        assert _next_gated(L, both, p1, 0, (0, 3), None) == 0
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
        assert records[:S].tobytes() == levels.measure(pcm16[:S]).tobytes() and _untouched(records[S:])
        buses, records = fresh()
        _native.check(L.mbx_session_next_levels(both, records.ctypes.data), "next_levels")
        _native.check(_next_gated(L, both, p1, 0, (0, 3), buses), "next_mixdown_gated")
        assert L.mbx_session_next_levels(both, None) == 0
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(records)
        assert buses.tobytes() == levels.mix_gated(pcm16[:S], *csr1, 0, 0, 3).tobytes()
        # seed, get_state, set_state and reset leave them for the submit
        buses, records = fresh()
        _native.check(L.mbx_session_next_levels(both, records.ctypes.data), "next_levels")
        bytes_ = np.full((13, 160), FILL, np.uint8)
        _native.check(_next_gated(L, both, p2, 2, (T_OPEN, 0), bytes_), "next_mixdown_gated")
        st, rg = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
        seeds = np.arange(S, dtype=np.uint32) + 9
        _native.check(L.mbx_session_reset(both, 0, S), "reset")
        _native.check(L.mbx_session_seed(both, 0, S, seeds.ctypes.data), "seed")
        _native.check(L.mbx_session_get_state(both, 0, S, st.ctypes.data, rg.ctypes.data), "get_state")
        _native.check(L.mbx_session_set_state(both, 0, S, st.ctypes.data, rg.ctypes.data), "set_state")
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert records.tobytes() == levels.measure(pcm16).tobytes() and bytes_.tobytes() == levels.mix_gated(pcm16, *csr2, 2, T_OPEN, 0).tobytes()
        # a session created for the records alone: it has no pcm16 to give, and its records are those of the same frames' pcm16
        only = sessions[LEVELS]
        for h in (both, only):
            _native.check(L.mbx_session_reset(h, 0, S), "reset")
            _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
        assert submit(only, 1, pcm16) == INVALID
        alone = np.full(S * 2 * 16, FILL, np.uint8).view(levels.LEVEL_DTYPE)
        _native.check(L.mbx_session_next_levels(only, alone.ctypes.data), "next_levels")
        assert submit(only, 2, None) == 0 and L.mbx_session_wait(only) == 0
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert alone.tobytes() == levels.measure(pcm16).tobytes() and len(np.unique(pcm16)) > 100
    finally:
        for h in sessions.values():
            L.mbx_session_destroy(h)
        plans.close()
