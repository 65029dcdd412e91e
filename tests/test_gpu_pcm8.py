"""GPU suite (-m gpu) for companded PCM out (include/mbx_pcm8.h): mbx_pcm_compand held byte for byte to the numpy definition
(mbelib_neo_amd.pcm8) -- over every int16 value, between guard bands at exactly the alignments of its contract, at every phase of the
two addresses, behind a decode --, and the sessions' mbx_session_next_pcm8 to numpy of the int16 PCM the same submit (or a twin session
without the flag) delivered, for every submit form, with the rules of the attachment.  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import burst_cases
import burst_group_cases as G
import edge_mix
import guarded
import soft_mix
from mbelib_neo_amd import pcm8

pytestmark = pytest.mark.gpu

LAWS = (pcm8.LAW_ULAW, pcm8.LAW_ALAW)
PCM16, PCM8 = 1, pcm8.SESSION_PCM8
S = 70   # streams of the session tests: more than a wave
FILL = 0x5A


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _compand(law, in_ptr, nframes, out_ptr):
    import torch
    from mbelib_neo_amd import _native

    return _native.lib().mbx_pcm_compand(law, in_ptr, nframes, out_ptr, torch.cuda.current_stream().cuda_stream)


def _samples(rng, n):
    """random samples with both extremes, zero and the values round them planted"""
    x = rng.integers(-32768, 32768, size=n, dtype=np.int64).astype(np.int16)
    plant = np.array([-32768, 32767, 0, -1, 3, 4, -32768, 32767], dtype=np.int16)
    x[:4] = plant[:4]
    x[-4:] = plant[4:]
    x[rng.integers(0, n, size=8)] = plant
    return x


# ---- the launch ----------------------------------------------------------------------------------------------------------------------------
def test_every_int16_value_gives_the_byte_of_the_numpy_definition(mbx):
    """410 rows hold every int16 value once (in a shuffled order) and 64 padding samples"""
    import torch

    rng = np.random.default_rng(1)
    x = np.concatenate([np.arange(-32768, 32768, dtype=np.int32).astype(np.int16), _samples(rng, 64)])
    x = x[rng.permutation(x.size)].reshape(410, 160)
    d = torch.from_numpy(x).cuda()
    for law in LAWS:
        out = torch.full((410, 160), FILL, dtype=torch.uint8, device="cuda")
        assert _compand(law, d.data_ptr(), 410, out.data_ptr()) == 0
        torch.cuda.synchronize()
        got, want = out.cpu().numpy(), pcm8.compand(x, law)
        assert got.tobytes() == want.tobytes(), (law, np.flatnonzero(got.reshape(-1) != want.reshape(-1))[:8])
    assert np.array_equal(d.cpu().numpy(), x)


@pytest.mark.parametrize("rows", [1, 2, 3, 5, 64, 65, 257])
def test_nothing_outside_the_payload_changes_at_exactly_the_alignments_of_the_contract(mbx, rows):
    """input at 2 and no better, read-only; output at 1 and no better; guard bands of tests/guarded.py on every side"""
    import torch

    x = _samples(np.random.default_rng(10 + rows), rows * 160)
    arena = guarded.Arena([guarded.buf("pcm16", 320 * rows, "pcm16", True), guarded.buf("pcm8", 160 * rows, "frames")], where="cuda", seed=rows)
    assert arena.ptr("pcm16") % 4 == 2 and arena.ptr("pcm8") % 2 == 1
    arena.load("pcm16", x)
    for law in LAWS:
        arena.prefill("pcm8")
        assert _compand(law, arena.ptr("pcm16"), rows, arena.ptr("pcm8")) == 0
        torch.cuda.synchronize()
        arena.check(f"law {law}, {rows} rows")
        assert arena.read("pcm8").tobytes() == pcm8.compand(x, law).tobytes(), (law, rows)


def test_every_phase_of_the_two_addresses_gives_the_same_bytes(mbx):
    """one allocation; the input 0 and 2 bytes past a 16-byte boundary, the output 0 .. 3 bytes past one: the pairs (0, 0) and (2, 1)
    give pieces that are 16-byte aligned in the input where they are 8-byte aligned in the output, the other six do not"""
    import torch

    most = 13 * 160
    mem = torch.empty(16 + 2 * most + 64 + most + 192, dtype=torch.uint8, device="cuda")
    base = (mem.data_ptr() + 15) & ~15
    at_in, at_out = base - mem.data_ptr(), base - mem.data_ptr() + ((2 * most + 64 + 15) & ~15) + 64
    assert (mem.data_ptr() + at_out) % 16 == 0
    rng = np.random.default_rng(5)
    wide = 0
    for rows in (1, 3, 13):
        n = rows * 160
        x = _samples(rng, n)
        for off_in in (0, 2):
            mem[at_in + off_in:at_in + off_in + 2 * n].copy_(torch.from_numpy(x.view(np.uint8).copy()))
            for off_out in (0, 1, 2, 3):
                lo = at_out + off_out
                p_in, p_out = mem.data_ptr() + at_in + off_in, mem.data_ptr() + lo
                head = -p_out % 8
                wide += (p_in + 2 * head) % 16 == 0
                for law in LAWS:
                    mem[lo - 64:lo + n + 64] = FILL
                    assert _compand(law, p_in, rows, p_out) == 0
                    torch.cuda.synchronize()
                    got = mem[lo - 64:lo + n + 64].cpu().numpy()
                    assert got[64:64 + n].tobytes() == pcm8.compand(x, law).tobytes(), (rows, off_in, off_out, law)
                    assert (got[:64] == FILL).all() and (got[64 + n:] == FILL).all(), (rows, off_in, off_out, law)
                    assert _compand(law, p_in, 0, p_out) == 0   # no frames: nothing is launched, nothing changes
                    torch.cuda.synchronize()
                    assert mem[lo - 64:lo + n + 64].cpu().numpy().tobytes() == got.tobytes()
            assert mem[at_in + off_in:at_in + off_in + 2 * n].cpu().numpy().tobytes() == x.tobytes()
    assert wide == 3 * 2   # both instances were reached: two of the eight pairs, for each row count


@pytest.mark.parametrize("codec", [0, 1])
def test_behind_a_decode_the_bytes_are_those_of_its_pcm16(mbx, codec):
    import torch
    from mbelib_neo_amd import decoder

    T = 3
    dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) * 7 + 3)
    out = dec.decode(edge_mix.frames(codec, S, T, 1).reshape(S * T, -1), T)
    bytes_of = {law: dec.compand(out["pcm16"], law) for law in LAWS}   # on the decode's stream, no synchronisation between
    given = torch.full((S * T, 160), FILL, dtype=torch.uint8, device="cuda")
    assert dec.compand(out["pcm16"], pcm8.LAW_ALAW, out=given) is given
    torch.cuda.synchronize()
    pcm16 = out["pcm16"].cpu().numpy()
    assert len(np.unique(pcm16)) > 100, "the decode gave no audio to compand"
    for law in LAWS:
        assert bytes_of[law].shape == (S * T, 160) and bytes_of[law].dtype == torch.uint8
        assert bytes_of[law].cpu().numpy().tobytes() == pcm8.compand(pcm16, law).tobytes(), law
    assert given.cpu().numpy().tobytes() == pcm8.alaw(pcm16).tobytes()
    with pytest.raises(ValueError):
        dec.compand(out["pcm16"].to(torch.int32), 0)
    with pytest.raises(Exception, match="mbx_pcm_compand"):
        dec.compand(out["pcm16"], 2)


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


@pytest.mark.parametrize("codec,pinned", [(0, False), (1, False), (0, True)], ids=["imbe-pageable", "ambe-pageable", "imbe-pinned"])
def test_three_submits_in_flight_deliver_the_bytes_of_their_own_pcm16(mbx, codec, pinned):
    """T = 1, 3, 1 before the first wait, the law alternating; the third asks for the bytes alone and is held to a twin session
    without the flag"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    a, b = _session(L, codec, S, S * 3, PCM16 | PCM8), _session(L, codec, S, S * 3, PCM16)
    host = _Host(L, pinned)
    try:
        steps = []
        for k, T in enumerate((1, 3, 1)):
            frames = np.ascontiguousarray(edge_mix.frames(codec, S, T, 2 + k).reshape(S * T, -1))
            law = LAWS[k & 1]
            own16 = host.array((S * T, 160), np.int16) if k < 2 else None
            own8, twin16 = host.array((S * T, 160), np.uint8), np.zeros((S * T, 160), np.int16)
            _native.check(L.mbx_session_next_pcm8(a, law, own8.ctypes.data), "next_pcm8")
            _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, None if own16 is None else own16.ctypes.data, None, None), "submit")
            _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin16.ctypes.data, None, None), "submit (twin)")
            steps.append((law, frames, own16, own8, twin16))
        _native.check(L.mbx_session_wait(a), "wait")
        _native.check(L.mbx_session_wait(b), "wait (twin)")
        for k, (law, _, own16, own8, twin16) in enumerate(steps):
            assert len(np.unique(twin16)) > 100, k
            if own16 is not None:
                assert own16.tobytes() == twin16.tobytes(), f"submit {k}: pcm16 is no longer what a session without the flag delivers"
                assert own8.tobytes() == pcm8.compand(own16, law).tobytes(), f"submit {k}"
            assert own8.tobytes() == pcm8.compand(twin16, law).tobytes(), f"submit {k}"
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)
        host.close()


def test_every_submit_form_delivers_the_bytes_of_its_pcm16(mbx):
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    codec, F = 0, 2
    h = _session(L, codec, S, S * F, PCM16 | PCM8)
    rng = np.random.default_rng(8)
    sched = B.random_schedule(codec, F, F * B.channel_bits(codec) + 120, rng, device=True)
    try:
        def run(what, rows, law, submit):
            pcm16, out8 = np.full((rows, 160), 0x5A5A, np.int16), np.full((rows, 160), FILL, np.uint8)
            _native.check(L.mbx_session_next_pcm8(h, law, out8.ctypes.data), "next_pcm8")
            _native.check(submit(pcm16.ctypes.data), what)
            _native.check(L.mbx_session_wait(h), "wait")
            assert not _untouched(pcm16), what
            assert out8.tobytes() == pcm8.compand(pcm16, law).tobytes(), what

        index = np.array([1, 64, 4, 69, 31], dtype=np.int32)   # 5 of the 70 streams, voice among them, across the wave boundary
        frames = np.ascontiguousarray(edge_mix.frames(codec, 5, 2, 11).reshape(10, -1))
        run("indexed", 10, 0, lambda p: L.mbx_session_submit_indexed(h, 5, 2, index.ctypes.data, frames.ctypes.data, p, None, None, None))
        soft = np.ascontiguousarray(soft_mix.frames(codec, S, 1, 12))
        run("soft", S, 1, lambda p: L.mbx_session_submit_soft(h, 1, soft.ctypes.data, p, None, None))
        soft5 = np.ascontiguousarray(soft_mix.frames(codec, 5, 1, 13))
        run("soft indexed", 5, 0, lambda p: L.mbx_session_submit_soft_indexed(h, 5, 1, index.ctypes.data, soft5.ctypes.data, p, None, None, None))
        clear = np.ascontiguousarray(edge_mix.frames(codec, S, 1, 14).reshape(S, -1))
        rows = rng.integers(0, 256, size=(S, 12), dtype=np.uint8)
        rows[::2] = 0   # every other channel in the clear
        run("keyed", S, 1, lambda p: L.mbx_session_submit_keyed(h, S, 1, None, clear.ctypes.data, None, rows.ctypes.data, p, None, None, None))
        carried = edge_mix.frames(codec, S, F, 15).reshape(S * F, -1)
        bursts = np.ascontiguousarray(burst_cases.make_bursts(sched, carried, rng))
        run("bursts", S * F, 0, lambda p: L.mbx_session_submit_bursts(h, sched.handle, S, None, bursts.ctypes.data, sched.burst_bytes, p, None, None))
        cells = soft_mix.frames(codec, S, F, 16)
        soft_bursts = np.ascontiguousarray(burst_cases.make_bursts(sched, cells, rng, soft=True))
        run("soft bursts", S * F, 1, lambda p: L.mbx_session_submit_bursts_soft(h, sched.handle, S, None, soft_bursts.ctypes.data, p, None, None))
        # ... and burst groups on this single-codec session: one group of 3 streams
        shapes = ((codec, F, B.FORM_PACKED, False, 3, 1, 0),)
        scheds = G.schedules(shapes, 17)
        groups = G.make_groups(shapes, scheds, False, 18, tag=2, slots=[np.array([66, 2, 40], dtype=np.int32)])
        arr, keep = G.group_array(L, groups)
        run("burst groups", 3 * F, 0, lambda p: L.mbx_session_submit_burst_groups(h, arr, 1, 0, p, None, None))
        for s in scheds:
            s.close()
    finally:
        L.mbx_session_destroy(h)
        sched.close()


def test_a_mixed_session_of_eight_streams_delivers_the_bytes_of_a_burst_group_submit(mbx):
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    codec_of = np.array([0, 1, 2, 3, 3, 2, 1, 0], dtype=np.uint8)
    # (codec, frames per burst, form, inversion sequence, streams, bursts per stream, extra bytes of burst_stride)
    shapes = ((0, 2, B.FORM_PACKED, False, 2, 1, 0), (1, 3, B.FORM_DIBITS, True, 2, 2, 0), (3, 1, B.FORM_BITS, False, 2, 1, 0), (2, 1, B.FORM_PACKED, False, 2, 1, 3))
    total = sum(g[1] * g[4] * g[5] for g in shapes)
    slots = [np.flatnonzero(codec_of == g[0]).astype(np.int32)[::-1].copy() for g in shapes]
    scheds = G.schedules(shapes, 21)
    h, twin = C.c_void_p(), C.c_void_p()
    _native.check(L.mbx_session_create_mixed(C.byref(h), 8, codec_of.ctypes.data, total, PCM8), "create_mixed")
    _native.check(L.mbx_session_create_mixed(C.byref(twin), 8, codec_of.ctypes.data, total, PCM16), "create_mixed (twin)")
    try:
        for tick, law in enumerate(LAWS):
            groups = G.make_groups(shapes, scheds, False, 22 + tick, tag=3 + tick, slots=slots)
            arr, keep = G.group_array(L, groups)
            out8, pcm16 = np.full((total, 160), FILL, np.uint8), np.zeros((total, 160), np.int16)
            _native.check(L.mbx_session_next_pcm8(h, law, out8.ctypes.data), "next_pcm8")
            _native.check(L.mbx_session_submit_burst_groups(h, arr, 4, 0, None, None, None), "submit_burst_groups")   # the bytes alone
            _native.check(L.mbx_session_submit_burst_groups(twin, arr, 4, 0, pcm16.ctypes.data, None, None), "submit_burst_groups (twin)")
            _native.check(L.mbx_session_wait(h), "wait")
            _native.check(L.mbx_session_wait(twin), "wait (twin)")
            assert len(np.unique(pcm16)) > 100
            assert out8.tobytes() == pcm8.compand(pcm16, law).tobytes(), tick
    finally:
        L.mbx_session_destroy(h)
        L.mbx_session_destroy(twin)
        for s in scheds:
            s.close()


def test_the_attachment_lasts_for_one_submit_whether_it_queues_or_refuses(mbx):
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

    L = _native.lib()
    codec, INVALID = 0, -1
    frames = {T: np.ascontiguousarray(edge_mix.frames(codec, S, T, 30 + T).reshape(S * T, -1)) for T in (1, 2, 3)}
    plain, both, only8 = _session(L, codec, S, S * 2, PCM16), _session(L, codec, S, S * 2, PCM16 | PCM8), _session(L, codec, S, S * 2, PCM8)
    try:
        def refused(h, law, p):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert L.mbx_session_next_pcm8(h, law, p) == INVALID
            assert b"mbx_session_next_pcm8" in L.mbx_last_error(), L.mbx_last_error()

        def submit(h, T, pcm16):
            return L.mbx_session_submit(h, T, frames[T].ctypes.data, None if pcm16 is None else pcm16.ctypes.data, None, None)

        out8, pcm16 = np.full((S * 2, 160), FILL, np.uint8), np.zeros((S * 2, 160), np.int16)
        refused(plain, 0, out8.ctypes.data)            # a session made without the flag
        refused(both, 2, out8.ctypes.data)             # a law that is none
        refused(both, -1, out8.ctypes.data)
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(out8)   # ... and neither left anything attached
        # a refused submit uses the attachment up: the next good one leaves the destination alone
        _native.check(L.mbx_session_next_pcm8(both, 0, out8.ctypes.data), "next_pcm8")
        assert submit(both, 3, pcm16) == INVALID        # T beyond max_frames_per_submit
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert _untouched(out8) and len(np.unique(pcm16)) > 100
        # ... also a burst-group submit that is refused for its group list, before it looks at its session
        _native.check(L.mbx_session_next_pcm8(both, 1, out8.ctypes.data), "next_pcm8")
        assert L.mbx_session_submit_burst_groups(both, None, 1, 0, pcm16.ctypes.data, None, None) == INVALID and b"groups is NULL" in L.mbx_last_error()
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(out8)
        # NULL clears it
        _native.check(L.mbx_session_next_pcm8(both, 0, out8.ctypes.data), "next_pcm8")
        assert L.mbx_session_next_pcm8(both, 1, None) == 0
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(out8)
        # seed, get_state, set_state and reset leave it for the submit
        _native.check(L.mbx_session_next_pcm8(both, 1, out8.ctypes.data), "next_pcm8")
        st, rg = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
        seeds = np.arange(S, dtype=np.uint32) + 9
        _native.check(L.mbx_session_reset(both, 0, S), "reset")
        _native.check(L.mbx_session_seed(both, 0, S, seeds.ctypes.data), "seed")
        _native.check(L.mbx_session_get_state(both, 0, S, st.ctypes.data, rg.ctypes.data), "get_state")
        _native.check(L.mbx_session_set_state(both, 0, S, st.ctypes.data, rg.ctypes.data), "set_state")
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert out8.tobytes() == pcm8.alaw(pcm16).tobytes()
        # ... once: the submit after it delivers no bytes
        out8[...] = FILL
        assert submit(both, 1, pcm16) == 0 and L.mbx_session_wait(both) == 0 and _untouched(out8)
        # a session created for the bytes alone: it has no pcm16 to give, and its bytes are those of the same frames' pcm16
        for h in (both, only8):
            _native.check(L.mbx_session_reset(h, 0, S), "reset")
            _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
        assert submit(only8, 1, pcm16) == INVALID
        _native.check(L.mbx_session_next_pcm8(only8, 0, out8.ctypes.data), "next_pcm8")
        assert submit(only8, 2, None) == 0 and L.mbx_session_wait(only8) == 0
        assert submit(both, 2, pcm16) == 0 and L.mbx_session_wait(both) == 0
        assert out8.tobytes() == pcm8.ulaw(pcm16).tobytes() and len(np.unique(pcm16)) > 100
    finally:
        for h in (plain, both, only8):
            L.mbx_session_destroy(h)
