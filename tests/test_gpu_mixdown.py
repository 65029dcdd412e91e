"""GPU suite (-m gpu) for mix-down out (include/mbx_mixdown.h): mbx_mixdown held byte for byte to the numpy definition
(mbelib_neo_amd.mixdown.mix) -- over row and bus counts on either side of a workgroup and a wave, through both kernel forms and the
default split between them, between guard bands at exactly the alignments of its contract, behind a decode --, and the sessions'
mbx_session_next_mixdown to numpy of the int16 PCM the same submit (or a twin session without the flag) delivered, for every submit
form, with the rules of the attachment.  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import burst_cases
import burst_group_cases as G
import edge_mix
import guarded
import soft_mix
from mbelib_neo_amd import mixdown, pcm8

pytestmark = pytest.mark.gpu

PCM16, PCM8, MIX = 1, pcm8.SESSION_PCM8, mixdown.SESSION_MIXDOWN
S = 70   # streams of the session tests: more than a wave
FILL = 0x5A
INVALID = -1


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _mixdown(plan, form, in_ptr, nrows, out_ptr):
    import torch
    from mbelib_neo_amd import _native

    return _native.lib().mbx_mixdown(plan.handle, form, in_ptr, nrows, out_ptr, torch.cuda.current_stream().cuda_stream)


def _rows(rng, rows):
    """full-range rows; row 0 is quiet but for both extremes, so that a gain of 8 on it saturates at either end and nowhere else"""
    x = rng.integers(-32768, 32768, size=(rows, 160), dtype=np.int64).astype(np.int16)
    x[0] = rng.integers(-100, 101, size=160)
    x[0, [5, 159]] = 32767
    x[0, [0, 77]] = -32768
    return x


def _buses(rng, rows, n_buses, cap=30):
    """n_buses buses over `rows` rows, of seven kinds in turn: a general one (row 0 twice at a gain of 8, then random rows at gains of
    both signs), an empty one, a unity single input, one row twice, row 0 against the last row with opposite polarity (row 0 is in
    many buses), a larger one, and one at the extreme gains"""
    off, row, gain = [0], [], []
    for b in range(n_buses):
        kind = b % 7
        if kind == 0:
            k = int(rng.integers(1, 8))
            r, g = [0, 0] + rng.integers(0, rows, k).tolist(), [32767, 32767] + rng.integers(-3000, 3001, k).tolist()
        elif kind == 1:
            r, g = [], []
        elif kind == 2:
            r, g = [b % rows], [4096]
        elif kind == 3:
            r, g = [(b * 5) % rows] * 2, [4096, 2048]
        elif kind == 4:
            r, g = [0, rows - 1], [-4096, 4096]
        elif kind == 5:
            k = int(rng.integers(13, cap + 1))
            r, g = rng.integers(0, rows, k).tolist(), rng.integers(-1500, 1501, k).tolist()
        else:
            r, g = rng.integers(0, rows, 4).tolist(), [-32768, 32767, 1, -1]
        row += r
        gain += g
        off.append(len(row))
    return np.array(off, dtype=np.int32), np.array(row, dtype=np.int32), np.array(gain, dtype=np.int16)


_CASES = {}


def _case(rows, n_buses):
    """the rows, the buses and numpy's answer in the three forms, made once and shared (read-only)"""
    key = (rows, n_buses)
    if key not in _CASES:
        rng = np.random.default_rng(1000 * rows + n_buses)
        x = _rows(rng, rows)
        off, row, gain = _buses(rng, rows, n_buses)
        want = {form: mixdown.mix(x, off, row, gain, form) for form in mixdown.FORMS}
        for a in (x, off, row, gain, *want.values()):
            a.setflags(write=False)
        assert (want[mixdown.PCM16] == 32767).any() and (want[mixdown.PCM16] == -32768).any(), "both saturations occur"
        _CASES[key] = (x, off, row, gain, want)
    return _CASES[key]


# ---- the launch ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("rows,n_buses", [(1, 1), (3, 3), (64, 13), (257, 70), (1, 70), (257, 3), (3, 13)])
def test_both_kernel_forms_give_the_bytes_of_the_numpy_definition(mbx, rows, n_buses):
    """every case through mbx_mixdown_plan_create_split twice: long_above = 1 (every bus of two inputs or more takes the long form) and
    4096 (every bus the short one); 13 buses x 20 lanes are more than one workgroup, 70 buses more than a wave of them"""
    import torch

    x, off, row, gain, want = _case(rows, n_buses)
    d = torch.from_numpy(x.copy()).cuda()
    sizes = np.diff(off)
    got = {}
    for above in (1, 4096):
        with mixdown.Plan(off, row, gain, long_above=above) as plan:
            assert (plan.buses, plan.rows) == (n_buses, int(row.max()) + 1)
            assert plan.long_buses == (int((sizes > 1).sum()) if above == 1 else 0)
            for form in mixdown.FORMS:
                out = torch.full((n_buses, 160), FILL, dtype=torch.int16 if form == mixdown.PCM16 else torch.uint8, device="cuda")
                assert _mixdown(plan, form, d.data_ptr(), rows, out.data_ptr()) == 0
                torch.cuda.synchronize()
                got[above, form] = out.cpu().numpy()
                bad = np.flatnonzero(got[above, form].reshape(-1) != want[form].reshape(-1))
                assert got[above, form].tobytes() == want[form].tobytes(), (above, form, bad[:8], bad.size)
    for form in mixdown.FORMS:
        assert got[1, form].tobytes() == got[4096, form].tobytes()
    assert np.array_equal(d.cpu().numpy(), x)
    # unity gains through the NULL array
    with mixdown.Plan(off, row, None) as plan:
        out = torch.full((n_buses, 160), FILL, dtype=torch.int16, device="cuda")
        assert _mixdown(plan, mixdown.PCM16, d.data_ptr(), rows, out.data_ptr()) == 0
        torch.cuda.synchronize()
        assert out.cpu().numpy().tobytes() == mixdown.mix(x, off, row, None).tobytes()


def test_the_default_split_sends_buses_above_it_to_the_long_form(mbx):
    """bus sizes long_above and long_above + 1 on either side of the split, one 4,096-input bus, an empty one and a single input, over
    257 rows"""
    import torch

    rows, above = 257, mixdown.LONG_ABOVE
    rng = np.random.default_rng(44)
    x = _rows(rng, rows)
    sizes = [above, above + 1, 4096, 0, 1, above + 1, above, 2]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    row = rng.integers(0, rows, size=int(off[-1]), dtype=np.int64).astype(np.int32)
    gain = rng.integers(-700, 701, size=int(off[-1]), dtype=np.int64).astype(np.int16)
    gain[off[2]:off[3]:3] = 4096   # the all-call bus: a third at unity, so that it saturates in places
    row[-1] = rows - 1
    d = torch.from_numpy(x).cuda()
    with mixdown.Plan(off, row, gain) as plan, mixdown.Plan(off, row, gain, long_above=4096) as short, mixdown.Plan(off, row, gain, long_above=0) as zero:
        assert (plan.buses, plan.rows, plan.long_buses) == (len(sizes), rows, 3)
        assert short.long_buses == 0 and zero.long_buses == 3   # 0 is the library's default
        for form in mixdown.FORMS:
            want = mixdown.mix(x, off, row, gain, form)
            for p in (plan, short):
                out = torch.full((len(sizes), 160), FILL, dtype=torch.int16 if form == mixdown.PCM16 else torch.uint8, device="cuda")
                assert _mixdown(p, form, d.data_ptr(), rows, out.data_ptr()) == 0
                torch.cuda.synchronize()
                assert out.cpu().numpy().tobytes() == want.tobytes(), (form, p.long_buses)
            if form == mixdown.PCM16:
                assert (want[2] == 32767).any() or (want[2] == -32768).any()


@pytest.mark.parametrize("rows,n_buses", [(1, 3), (3, 13), (257, 70)])
def test_nothing_outside_the_payload_changes_at_exactly_the_alignments_of_the_contract(mbx, rows, n_buses):
    """input at 16 and no better, read-only; int16 buses at 16 and bytes at 8 and no better; guard bands of tests/guarded.py on every
    side (the kinds "stage" and "rng" of its table are the ones of 16 and 8 bytes); the default split and all-long"""
    import torch

    x, off, row, gain, want = _case(rows, n_buses)
    arena = guarded.Arena([guarded.buf("pcm16", 320 * rows, "stage", True), guarded.buf("bus16", 320 * n_buses, "stage"),
                           guarded.buf("bus8", 160 * n_buses, "rng")], where="cuda", seed=rows)
    assert arena.ptr("pcm16") % 32 == 16 and arena.ptr("bus16") % 32 == 16 and arena.ptr("bus8") % 16 == 8
    arena.load("pcm16", x)
    for above in (None, 1):
        with mixdown.Plan(off, row, gain, long_above=above) as plan:
            for form in mixdown.FORMS:
                name = "bus16" if form == mixdown.PCM16 else "bus8"
                arena.prefill("bus16", "bus8")
                assert _mixdown(plan, form, arena.ptr("pcm16"), rows, arena.ptr(name)) == 0
                torch.cuda.synchronize()
                arena.check(f"form {form}, {rows} rows, {n_buses} buses, long_above {above}")
                assert arena.read(name).tobytes() == want[form].tobytes(), (form, above)
                other = "bus8" if name == "bus16" else "bus16"
                assert arena.read(other).tobytes() == arena.prefill_bytes(other).tobytes()


def test_the_launcher_refuses_what_only_a_plan_can_tell(mbx):
    """with a plan in hand: nrows below the rows it needs, arrays that overlap, a pointer below its alignment, a form that is none"""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    x, off, row, gain, want = _case(64, 13)
    mem = torch.full((64 * 320 + 13 * 320 + 64,), FILL, dtype=torch.uint8, device="cuda")
    base = (mem.data_ptr() + 15) & ~15
    out = base + 64 * 320
    with mixdown.Plan(off, row, gain) as plan:
        need = plan.rows

        def refused(part, *args):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert _mixdown(plan, *args) == INVALID, args
            assert b"mbx_mixdown:" in L.mbx_last_error() and part in L.mbx_last_error(), L.mbx_last_error()

        refused(b"nrows", 0, base, need - 1, out)
        refused(b"nrows", 1, base, 0, out)
        refused(b"overlap", 0, base, 64, out - 16)
        refused(b"overlap", 2, base, 64, base)
        refused(b"overlap", 0, base, 65, out)         # the caller's rows count, read or not
        refused(b"alignment", 0, base + 8, 64, out)
        refused(b"alignment", 0, base, 64, out + 8)
        refused(b"alignment", 1, base, 64, out + 4)
        refused(b"form", 3, base, 64, out)
        torch.cuda.synchronize()
        assert (mem.cpu().numpy() == FILL).all(), "a refused call launched something"
        assert _mixdown(plan, 1, base, 64, out + 8) == 0   # bytes at 8
        torch.cuda.synchronize()


@pytest.mark.parametrize("codec", [0, 1])
def test_behind_a_decode_the_buses_are_those_of_its_pcm16(mbx, codec):
    import torch
    from mbelib_neo_amd import decoder

    T = 3
    dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) * 7 + 3)
    rng = np.random.default_rng(50 + codec)
    off, row, gain = _buses(rng, S * T, 13)
    with mixdown.Plan(off, row, gain) as plan:
        out = dec.decode(edge_mix.frames(codec, S, T, 1).reshape(S * T, -1), T)
        buses = {form: dec.mixdown(out["pcm16"], plan, form) for form in mixdown.FORMS}   # on the decode's stream, no synchronisation between
        given = torch.full((13, 160), FILL, dtype=torch.uint8, device="cuda")
        assert dec.mixdown(out["pcm16"], plan, mixdown.ALAW, out=given) is given
        torch.cuda.synchronize()
        pcm16 = out["pcm16"].cpu().numpy()
        assert len(np.unique(pcm16)) > 100, "the decode gave no audio to mix"
        for form in mixdown.FORMS:
            assert buses[form].shape == (13, 160) and buses[form].dtype == (torch.int16 if form == mixdown.PCM16 else torch.uint8)
            assert buses[form].cpu().numpy().tobytes() == mixdown.mix(pcm16, off, row, gain, form).tobytes(), form
        assert given.cpu().numpy().tobytes() == mixdown.mix(pcm16, off, row, gain, mixdown.ALAW).tobytes()
        with pytest.raises(ValueError):
            dec.mixdown(out["pcm16"].to(torch.int32), plan, 0)
        with pytest.raises(Exception, match="mbx_mixdown"):
            dec.mixdown(out["pcm16"], plan, 3)
        with pytest.raises(Exception, match="nrows"):
            dec.mixdown(out["pcm16"][:plan.rows - 1], plan, 0)


def test_a_released_stream_takes_its_kernel_name_with_it(mbx):
    """sessions release their compute stream when they go (mbx_release_stream); a stream made later may be given the same handle, and
    must not inherit the name of a launch it never saw (mbx_last_kernel_name)"""
    import torch
    from mbelib_neo_amd import _native, decoder

    L = _native.lib()
    side = torch.cuda.Stream()
    dec = decoder.BatchDecoder(0, S, seeds=np.arange(S) + 1)
    frames = dec.to_device(edge_mix.frames(0, S, 1, 3).reshape(S, -1))
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        dec.decode(frames, 1)
    torch.cuda.synchronize()
    assert L.mbx_last_kernel_name(side.cuda_stream) is not None
    assert L.mbx_release_stream(side.cuda_stream) == 0
    assert L.mbx_last_kernel_name(side.cuda_stream) is None
    assert L.mbx_release_stream(side.cuda_stream) == 0   # twice is harmless


# ---- sessions ------------------------------------------------------------------------------------------------------------------------------
class _Host:
    """destinations in pageable or in pinned (mbx_host_alloc) memory, pre-filled"""

    def __init__(self, L, pinned):
        self.L, self.pinned, self.owned = L, pinned, []

    def array(self, shape, dtype):
        n = int(np.prod(shape)) * np.dtype(dtype).itemsize
        if self.pinned:
            p = self.L.mbx_host_alloc(n)
            assert p
            self.owned.append(p)
            a = np.ctypeslib.as_array((C.c_uint8 * n).from_address(p)).view(dtype).reshape(shape)
        else:
            a = np.empty(shape, dtype=dtype)
        a.view(np.uint8)[...] = FILL
        return a

    def close(self):
        for p in self.owned:
            self.L.mbx_host_free(p)
        self.owned = []


def _session(L, codec, streams, max_frames, outputs, seeds=None):
    from mbelib_neo_amd import _native

    h = C.c_void_p()
    _native.check(L.mbx_session_create(C.byref(h), codec, streams, max_frames, outputs), "create")
    seeds = (np.arange(streams) * 3 + 5).astype(np.uint32) if seeds is None else seeds
    _native.check(L.mbx_session_seed(h, 0, streams, seeds.ctypes.data), "seed")
    return h


def _untouched(a):
    return bool((a.view(np.uint8) == FILL).all())


class _Plans:
    """a plan of 13 buses per row count, over all of the rows (its last input names the last row), kept until close"""

    def __init__(self):
        self.made = {}

    def of(self, rows):
        if rows not in self.made:
            off, row, gain = _buses(np.random.default_rng(rows), rows, 13)
            row[-1] = rows - 1
            self.made[rows] = (mixdown.Plan(off, row, gain), off, row, gain)
            assert self.made[rows][0].rows == rows
        return self.made[rows]

    def close(self):
        for p, *_ in self.made.values():
            p.close()


@pytest.mark.parametrize("codec,pinned", [(0, False), (1, False), (0, True)], ids=["imbe-pageable", "ambe-pageable", "imbe-pinned"])
def test_three_submits_in_flight_deliver_the_buses_of_their_own_pcm16(mbx, codec, pinned):
    """T = 1, 2, 1 before the first wait, the form changing; the third asks for the buses alone (NULL pcm16) and is held to a twin
    session without the flag"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    a, b = _session(L, codec, S, S * 2, PCM16 | MIX), _session(L, codec, S, S * 2, PCM16)
    host, plans = _Host(L, pinned), _Plans()
    try:
        steps = []
        for k, T in enumerate((1, 2, 1)):
            frames = np.ascontiguousarray(edge_mix.frames(codec, S, T, 2 + k).reshape(S * T, -1))
            form = mixdown.FORMS[k]
            plan, off, row, gain = plans.of(S * T)
            own16 = host.array((S * T, 160), np.int16) if k < 2 else None
            buses, twin16 = host.array((13, 160), mixdown.out_dtype(form)), np.zeros((S * T, 160), np.int16)
            _native.check(L.mbx_session_next_mixdown(a, plan.handle, form, buses.ctypes.data), "next_mixdown")
            _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, None if own16 is None else own16.ctypes.data, None, None), "submit")
            _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin16.ctypes.data, None, None), "submit (twin)")
            steps.append((form, own16, buses, twin16, (off, row, gain)))
        _native.check(L.mbx_session_wait(a), "wait")
        _native.check(L.mbx_session_wait(b), "wait (twin)")
        for k, (form, own16, buses, twin16, csr) in enumerate(steps):
            assert len(np.unique(twin16)) > 100, k
            if own16 is not None:
                assert own16.tobytes() == twin16.tobytes(), f"submit {k}: pcm16 is no longer what a session without the flag delivers"
                assert buses.tobytes() == mixdown.mix(own16, *csr, form).tobytes(), f"submit {k}"
            assert buses.tobytes() == mixdown.mix(twin16, *csr, form).tobytes(), f"submit {k}"
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)
        host.close()
        plans.close()


def test_every_submit_form_delivers_the_buses_of_its_pcm16_and_its_bytes_beside_them(mbx):
    """frames (T = 1 and 2), indexed, soft, soft indexed, keyed, bursts, soft bursts and burst groups; every other one also carries a
    pcm8 attachment on the same submit"""
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    codec, F = 0, 2
    h = _session(L, codec, S, S * F, PCM16 | PCM8 | MIX)
    rng = np.random.default_rng(8)
    sched = B.random_schedule(codec, F, F * B.channel_bits(codec) + 120, rng, device=True)
    plans = _Plans()
    count = [0]
    try:
        def run(what, rows, submit):
            k = count[0]
            count[0] += 1
            form, law = mixdown.FORMS[k % 3], k & 1
            plan, off, row, gain = plans.of(rows)
            pcm16, buses = np.full((rows, 160), 0x5A5A, np.int16), np.full((13, 160), FILL, mixdown.out_dtype(form))
            out8 = np.full((rows, 160), FILL, np.uint8)
            _native.check(L.mbx_session_next_mixdown(h, plan.handle, form, buses.ctypes.data), "next_mixdown")
            if k % 2:
                _native.check(L.mbx_session_next_pcm8(h, law, out8.ctypes.data), "next_pcm8")
            _native.check(submit(pcm16.ctypes.data), what)
            _native.check(L.mbx_session_wait(h), "wait")
            assert not _untouched(pcm16), what
            assert buses.tobytes() == mixdown.mix(pcm16, off, row, gain, form).tobytes(), what
            assert out8.tobytes() == pcm8.compand(pcm16, law).tobytes() if k % 2 else _untouched(out8), what

        for T in (1, 2):
            plain = np.ascontiguousarray(edge_mix.frames(codec, S, T, 9 + T).reshape(S * T, -1))
            run(f"frames T={T}", S * T, lambda p: L.mbx_session_submit(h, T, plain.ctypes.data, p, None, None))
        index = np.array([1, 64, 4, 69, 31], dtype=np.int32)   # 5 of the 70 streams, voice among them, across the wave boundary
        frames = np.ascontiguousarray(edge_mix.frames(codec, 5, 2, 11).reshape(10, -1))
        run("indexed", 10, lambda p: L.mbx_session_submit_indexed(h, 5, 2, index.ctypes.data, frames.ctypes.data, p, None, None, None))
        soft = np.ascontiguousarray(soft_mix.frames(codec, S, 1, 12))
        run("soft", S, lambda p: L.mbx_session_submit_soft(h, 1, soft.ctypes.data, p, None, None))
        soft5 = np.ascontiguousarray(soft_mix.frames(codec, 5, 1, 13))
        run("soft indexed", 5, lambda p: L.mbx_session_submit_soft_indexed(h, 5, 1, index.ctypes.data, soft5.ctypes.data, p, None, None, None))
        clear = np.ascontiguousarray(edge_mix.frames(codec, S, 1, 14).reshape(S, -1))
        rows = rng.integers(0, 256, size=(S, 12), dtype=np.uint8)
        rows[::2] = 0   # every other channel in the clear
        run("keyed", S, lambda p: L.mbx_session_submit_keyed(h, S, 1, None, clear.ctypes.data, None, rows.ctypes.data, p, None, None, None))
        carried = edge_mix.frames(codec, S, F, 15).reshape(S * F, -1)
        bursts = np.ascontiguousarray(burst_cases.make_bursts(sched, carried, rng))
        run("bursts", S * F, lambda p: L.mbx_session_submit_bursts(h, sched.handle, S, None, bursts.ctypes.data, sched.burst_bytes, p, None, None))
        cells = soft_mix.frames(codec, S, F, 16)
        soft_bursts = np.ascontiguousarray(burst_cases.make_bursts(sched, cells, rng, soft=True))
        run("soft bursts", S * F, lambda p: L.mbx_session_submit_bursts_soft(h, sched.handle, S, None, soft_bursts.ctypes.data, p, None, None))
        # ... and burst groups on this single-codec session: one group of 3 streams
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


def test_the_attachment_lasts_for_one_submit_whether_it_queues_or_refuses(mbx):
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

    L = _native.lib()
    codec = 0
    frames = {T: np.ascontiguousarray(edge_mix.frames(codec, S, T, 30 + T).reshape(S * T, -1)) for T in (1, 2, 3)}
    plain, both, only = _session(L, codec, S, S * 2, PCM16), _session(L, codec, S, S * 2, PCM16 | MIX), _session(L, codec, S, S * 2, MIX)
    plans = _Plans()
    try:
        p1, *csr1 = plans.of(S)
        p2, *csr2 = plans.of(S * 2)

        def refused(part, h, plan, form, p):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert L.mbx_session_next_mixdown(h, plan, form, p) == INVALID
            assert b"mbx_session_next_mixdown" in L.mbx_last_error() and part in L.mbx_last_error(), L.mbx_last_error()

        def submit(h, T, pcm16):
            return L.mbx_session_submit(h, T, frames[T].ctypes.data, None if pcm16 is None else pcm16.ctypes.data, None, None)

        buses, pcm16 = np.full((13, 160), 0x5A5A, np.int16), np.zeros((S * 2, 160), np.int16)
        refused(b"MBX_SESSION_MIXDOWN", plain, p1.handle, 0, buses.ctypes.data)   # a session made without the flag
        refused(b"form", both, p1.handle, 3, buses.ctypes.data)                   # a form that is none
        refused(b"form", both, p1.handle, -1, buses.ctypes.data)
        refused(b"no plan", both, None, 0, buses.ctypes.data)
        off141 = np.arange(142, dtype=np.int32)   # 141 buses of one input each: more than max_frames_per_submit = 140
        with mixdown.Plan(off141, np.zeros(141, np.int32), None) as wide:
            refused(b"more buses", both, wide.handle, 0, buses.ctypes.data)
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)   # ... and none of them left anything attached
        # a submit with fewer rows than the plan needs is refused, nothing is queued, and the attachment is used up
        _native.check(L.mbx_session_next_mixdown(both, p2.handle, 0, buses.ctypes.data), "next_mixdown")
        pcm16[...] = 0
        assert submit(both, 1, pcm16) == INVALID and b"rows" in L.mbx_last_error() and b"mix-down" in L.mbx_last_error(), L.mbx_last_error()
        assert L.mbx_session_wait(both) == 0 and not pcm16.any() and _untouched(buses)
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses) and len(np.unique(pcm16)) > 100
        # a refused submit uses the attachment up: the next good one leaves the destination alone
        _native.check(L.mbx_session_next_mixdown(both, p1.handle, 0, buses.ctypes.data), "next_mixdown")
        assert submit(both, 3, pcm16) == INVALID        # T beyond max_frames_per_submit
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
        # ... also a burst-group submit that is refused for its group list, before it looks at its session
        _native.check(L.mbx_session_next_mixdown(both, p1.handle, 1, buses.ctypes.data), "next_mixdown")
        assert L.mbx_session_submit_burst_groups(both, None, 1, 0, pcm16.ctypes.data, None, None) == INVALID and b"groups is NULL" in L.mbx_last_error()
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
        # NULL clears it
        _native.check(L.mbx_session_next_mixdown(both, p1.handle, 0, buses.ctypes.data), "next_mixdown")
        assert L.mbx_session_next_mixdown(both, p1.handle, 1, None) == 0 and L.mbx_session_next_mixdown(both, None, 7, None) == 0
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
        # seed, get_state, set_state and reset leave it for the submit
        _native.check(L.mbx_session_next_mixdown(both, p2.handle, 0, buses.ctypes.data), "next_mixdown")
        st, rg = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
        seeds = np.arange(S, dtype=np.uint32) + 9
        _native.check(L.mbx_session_reset(both, 0, S), "reset")
        _native.check(L.mbx_session_seed(both, 0, S, seeds.ctypes.data), "seed")
        _native.check(L.mbx_session_get_state(both, 0, S, st.ctypes.data, rg.ctypes.data), "get_state")
        _native.check(L.mbx_session_set_state(both, 0, S, st.ctypes.data, rg.ctypes.data), "set_state")
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert buses.tobytes() == mixdown.mix(pcm16, *csr2, 0).tobytes()
        # ... once: the submit after it delivers no buses
        buses[...] = 0x5A5A
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(buses)
        # a session created for the buses alone: it has no pcm16 to give, and its buses are those of the same frames' pcm16
        for h in (both, only):
            _native.check(L.mbx_session_reset(h, 0, S), "reset")
            _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
        assert submit(only, 1, pcm16) == INVALID
        bytes_ = np.full((13, 160), FILL, np.uint8)
        _native.check(L.mbx_session_next_mixdown(only, p2.handle, 1, bytes_.ctypes.data), "next_mixdown")
        assert submit(only, 2, None) == 0 and L.mbx_session_wait(only) == 0
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert bytes_.tobytes() == mixdown.mix(pcm16, *csr2, 1).tobytes() and len(np.unique(pcm16)) > 100
    finally:
        for h in (plain, both, only):
            L.mbx_session_destroy(h)
        plans.close()
