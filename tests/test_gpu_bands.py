"""GPU suite (-m gpu) for band records (include/mbx_bands.h): mbx_pcm_bands held byte for byte to the numpy definition
(mbelib_neo_amd.bands.measure) over row counts on either side of the rows-per-wave and workgroup boundaries and probe counts on either
side of a store round, in both forms, between guard bands at exactly the alignment of its contract; the identities IMPULSE and ZERO; the
synthetic DTMF rows of the host suite; the launcher's refusals that need a bank; behind a decode; captured into a graph and replayed
over changing rows; the sessions' mbx_session_next_bands held to numpy of the int16 PCM the same submit (or a twin session) delivered,
with the rules of the attachment; BatchDecoder.bands.  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import agc_cases
import bands_cases
import burst_cases
import burst_group_cases as G
import edge_mix
import guarded
from mbelib_neo_amd import agc, bands, filters, levels, pcm8
from test_gpu_mixdown import FILL, INVALID, S, _Host, _session, _untouched

pytestmark = pytest.mark.gpu

PCM16, PCMF, RESULTS, PCM8, LEVELS = 1, 2, 4, pcm8.SESSION_PCM8, levels.SESSION_LEVELS
NROWS = [1, 3, 4, 5, 63, 64, 65, 257]   # 4 rows are a wave and 16 a workgroup of pcm_bands_kernel; 257 leaves a tail of one
PROBES = [1, 2, 8, 15, 16, 17, 32]      # lane j keeps probe j: one store round, its edge, two rounds


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


def _bank(probes):
    from mbelib_neo_amd import decoder

    return decoder.Bank(probes)


def _launch(bank, form, in_ptr, nrows, out_ptr):
    from mbelib_neo_amd import _native

    return _native.lib().mbx_pcm_bands(bank.handle if bank is not None else None, form, in_ptr, nrows, out_ptr, _stream())


def _records(bank, form, x):
    """the device's records of the rows x, as numpy [rows, K] of the form's dtype"""
    import torch

    d = torch.from_numpy(np.array(x)).cuda()
    out = torch.full((x.shape[0] * bank.probes * bands.record_bytes(form),), FILL, dtype=torch.uint8, device="cuda")
    assert _launch(bank, form, d.data_ptr(), x.shape[0], out.data_ptr()) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(bands.out_dtype(form)).reshape(x.shape[0], bank.probes)


# ---- 1. parity -------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("K", PROBES)
def test_the_records_are_byte_for_byte_those_of_numpy_between_guard_bands(mbx, K):
    """every row count of NROWS in both forms: random rows and the rail rows (all 32767, all -32768, alternating) against random probes
    at the bound and the sign-aligned probe that reaches +-2,147,450,880; rows and records at 16 bytes and no better, the rows
    read-only, guard bands of tests/guarded.py on every side: nothing is written outside nrows * K * record_bytes"""
    import torch

    reached = 0
    for nrows in NROWS:
        x, p, want = bands_cases.case(nrows, K)
        with _bank(p) as bank:
            assert bank.probes == K
            for form in bands.FORMS:
                per = K * bands.record_bytes(form)
                arena = guarded.Arena([guarded.buf("pcm16", 320 * nrows, "stage", True), guarded.buf("records", per * nrows, "stage")], where="cuda",
                                      seed=nrows * 64 + K * 2 + form)
                assert arena.ptr("pcm16") % 32 == 16 and arena.ptr("records") % 32 == 16
                arena.load("pcm16", x)
                arena.prefill("records")
                assert _launch(bank, form, arena.ptr("pcm16"), nrows, arena.ptr("records")) == 0
                torch.cuda.synchronize()
                arena.check(f"{nrows} rows, {K} probes, form {form}")
                got = arena.read("records").view(bands.out_dtype(form)).reshape(nrows, K)
                bad = np.argwhere(got != want[form])
                assert got.tobytes() == want[form].tobytes(), (nrows, K, form, bad[:8].tolist(), got[tuple(bad[0])], want[form][tuple(bad[0])])
                # no rows: nothing is launched, nothing is written
                arena.prefill("records")
                assert _launch(bank, form, arena.ptr("pcm16"), 0, arena.ptr("records")) == 0
                torch.cuda.synchronize()
                arena.check("no rows")
                assert arena.read("records").tobytes() == arena.prefill_bytes("records").tobytes()
        if nrows >= 2:
            reached += int(abs(int(want[bands.COMPLEX]["re"][1, 0])) == 32768 * 65535)
    assert reached == len(NROWS) - 1, "the sign-aligned probe reaches the bound on the row of -32768"


def test_more_rows_than_one_pass_of_the_grid_and_a_tail(mbx):
    """the workgroups walk the 16-row groups in strides of the grid (2,048): 16 * 2048 * 2 + 16 * 5 + 3 rows make some workgroups walk
    three groups, most two, and the last group holds three rows"""
    nrows = 16 * 2048 * 2 + 16 * 5 + 3
    rng = np.random.default_rng(5)
    x = rng.integers(-32768, 32768, size=(nrows, 160)).astype(np.int16)
    p = bands_cases.bank(rng, 17)
    with _bank(p) as bank:
        for form in bands.FORMS:
            got = _records(bank, form, x)
            assert got.tobytes() == bands.measure(x, p, form).tobytes(), form


# ---- 2. identities ------------------------------------------------------------------------------------------------------------------------------
def test_impulse_and_zero_on_the_device(mbx):
    rng = np.random.default_rng(12)
    x = bands_cases.rows(rng, 70)
    places = [0, 1, 9, 10, 77, 158, 159]   # either end of a lane's ten samples, either end of a row
    p = np.zeros((len(places) + 2, 2, 160), dtype=np.int16)
    for k, m in enumerate(places):
        p[k + 1, 0, m] = 16384   # (probes 0 and the last are zeros)
    with _bank(p) as bank:
        got = _records(bank, bands.COMPLEX, x)
        power = _records(bank, bands.POWER, x)
    for k, m in enumerate(places):
        assert (got["re"][:, k + 1] == 16384 * x[:, m].astype(np.int64)).all() and not got["im"][:, k + 1].any(), m
        assert (power[:, k + 1] == (16384 * x[:, m].astype(np.int64)) ** 2 >> 31).all(), m
    for k in (0, len(places) + 1):
        assert not got["re"][:, k].any() and not got["im"][:, k].any() and not power[:, k].any(), "ZERO"
    assert got["re"].any()


# ---- 3. DTMF ------------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("window", ["rect", "hann"])
def test_the_device_bytes_of_the_dtmf_rows_are_numpys_and_decide_every_digit(mbx, window):
    x, keys = bands_cases.dtmf_rows()
    p = bands.dtmf(window)
    with _bank(p) as bank:
        got = _records(bank, bands.POWER, x)
    assert got.tobytes() == bands.measure(x, p, bands.POWER).tobytes()
    assert bands.dtmf_key(got) == keys


def test_the_launcher_refuses_what_only_a_bank_can_tell(mbx):
    """with a bank in hand: the form, the size, pointers below their alignment, the overlap; nothing is launched"""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    rows, K = 64, 8
    _, p, _ = bands_cases.case(rows, K)
    mem = torch.full((rows * 320 + rows * K * 8 + 64,), FILL, dtype=torch.uint8, device="cuda")
    base = (mem.data_ptr() + 15) & ~15
    out = base + rows * 320
    with _bank(p) as bank:
        def refused(part, form, in_ptr, nrows, out_ptr, b=bank):
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert _launch(b, form, in_ptr, nrows, out_ptr) == INVALID, part
            assert b"mbx_pcm_bands:" in L.mbx_last_error() and part in L.mbx_last_error(), L.mbx_last_error()

        refused(b"needed", 0, base, rows, out, b=None)
        refused(b"needed", 0, None, rows, out)
        refused(b"needed", 0, base, rows, None)
        refused(b"form is MBX_BANDS_COMPLEX or MBX_BANDS_POWER", 2, base, rows, out)
        refused(b"form is", -1, base + 8, 2**40, base + 8)
        refused(b"2^31-1", 0, base + 8, (2**31 - 1) // 64 + 1, base + 8)
        refused(b"2^31-1", 1, base, (2**31 - 1) // 32 + 1, out)
        for off in (2, 4, 8):
            refused(b"alignment", 0, base + off, rows, out)
            refused(b"alignment", 1, base, rows, out + off)
        assert b"mbx_bands.h" in L.mbx_last_error()
        refused(b"d_out overlaps d_pcm16", 0, base, rows, base)
        refused(b"d_out overlaps d_pcm16", 0, base, rows, out - 16)
        refused(b"d_out overlaps d_pcm16", 1, base + rows * K * 4 - 16, rows, base)
        refused(b"d_out overlaps d_pcm16", 0, base, rows + 1, out)   # the caller's rows count: the 65th row lies in d_out
        torch.cuda.synchronize()
        assert (mem.cpu().numpy() == FILL).all(), "a refused call launched something"
        assert _launch(bank, 0, base, rows, out) == 0
        torch.cuda.synchronize()


# ---- 4. behind a decode --------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1])
@pytest.mark.parametrize("T", [1, 2])
def test_behind_a_decode_the_records_are_those_of_its_pcm16(mbx, codec, T):
    import torch
    from mbelib_neo_amd import decoder

    n = 37
    dec = decoder.BatchDecoder(codec, n, seeds=np.arange(n) * 7 + 3)
    p = bands.dtmf("hann")
    with _bank(p) as bank:
        out = dec.decode(edge_mix.frames(codec, n, T, 1).reshape(n * T, -1), T)
        got = {form: dec.bands(out["pcm16"], bank, form) for form in bands.FORMS}   # on the decode's stream, no synchronisation between
        torch.cuda.synchronize()
        pcm16 = out["pcm16"].cpu().numpy()
        assert len(np.unique(pcm16)) > 100, "the decode gave no audio to measure"
        for form in bands.FORMS:
            assert got[form].shape == (n * T, 8 * bands.record_bytes(form))
            assert got[form].cpu().numpy().tobytes() == bands.measure(pcm16, p, form).tobytes(), form


# ---- 5. a graph ----------------------------------------------------------------------------------------------------------------------------------
def test_one_captured_launch_replayed_three_times_gives_the_records_of_the_rows_then_in_place(mbx):
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    nrows, K = 65, 17
    x, p, want = bands_cases.case(nrows, K)
    d = torch.zeros((nrows, 160), dtype=torch.int16, device="cuda")
    out = torch.full((nrows * K * 8,), FILL, dtype=torch.uint8, device="cuda")
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    with _bank(p) as bank:
        torch.cuda.synchronize()
        with torch.cuda.graph(g, stream=side):
            rc = L.mbx_pcm_bands(bank.handle, bands.COMPLEX, d.data_ptr(), nrows, out.data_ptr(), side.cuda_stream)
        assert rc == 0, L.mbx_last_error()
        for rows_now in (np.array(x), np.ascontiguousarray(x[::-1]), np.roll(x, 7, axis=1)):
            d.copy_(torch.from_numpy(rows_now.copy()))
            out.fill_(FILL)
            torch.cuda.synchronize()
            g.replay()
            torch.cuda.synchronize()
            assert out.cpu().numpy().tobytes() == bands.measure(rows_now, p, bands.COMPLEX).tobytes()


# ---- 6. sessions ---------------------------------------------------------------------------------------------------------------------------------
def _next(L, h, bank, form, out):
    return L.mbx_session_next_bands(h, bank.handle if bank is not None else None, form, None if out is None else out.ctypes.data)


@pytest.mark.parametrize("pinned", [False, True], ids=["pageable", "pinned"])
def test_three_submits_in_flight_deliver_the_records_of_their_own_pcm16(mbx, pinned):
    """T = 1, 2, 1 before the first wait, the form and the bank changing -- the second bank has more probes, so the slot's buffer grows;
    the third submit takes no pcm16 (NULL) and is held to a twin session"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec = 0
    a, b = _session(L, codec, S, S * 2, PCM16), _session(L, codec, S, S * 2, PCM16)
    host = _Host(L, pinned)
    p8, p17 = bands.dtmf("rect"), bands_cases.bank(np.random.default_rng(4), 17)
    try:
        with _bank(p8) as b8, _bank(p17) as b17:
            steps = []
            for k, (T, bank, p, form) in enumerate(((1, b8, p8, bands.POWER), (2, b17, p17, bands.COMPLEX), (1, b17, p17, bands.POWER))):
                frames = np.ascontiguousarray(edge_mix.frames(codec, S, T, 2 + k).reshape(S * T, -1))
                own16 = host.array((S * T, 160), np.int16) if k < 2 else None
                records, twin16 = host.array((S * T, bank.probes), bands.out_dtype(form)), np.zeros((S * T, 160), np.int16)
                _native.check(_next(L, a, bank, form, records), "next_bands")
                _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, None if own16 is None else own16.ctypes.data, None, None), "submit")
                _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin16.ctypes.data, None, None), "submit (twin)")
                steps.append((p, form, own16, records, twin16))
            _native.check(L.mbx_session_wait(a), "wait")
            _native.check(L.mbx_session_wait(b), "wait (twin)")
            for k, (p, form, own16, records, twin16) in enumerate(steps):
                assert len(np.unique(twin16)) > 100, k
                if own16 is not None:
                    assert own16.tobytes() == twin16.tobytes(), f"submit {k}: pcm16 is no longer what a session without the attachment delivers"
                assert records.tobytes() == bands.measure(twin16, p, form).tobytes(), f"submit {k}"
            # the same slot again, first with the smaller bank and then with one of 32 probes: the buffer of the slot is made anew
            p32 = bands_cases.bank(np.random.default_rng(6), 32)
            with _bank(p32) as b32:
                for k, (bank, p, form) in enumerate(((b8, p8, bands.COMPLEX), (b32, p32, bands.COMPLEX), (b32, p32, bands.POWER), (b32, p32, bands.COMPLEX))):
                    frames = np.ascontiguousarray(edge_mix.frames(codec, S, 2, 20 + k).reshape(S * 2, -1))
                    pcm16, records = host.array((S * 2, 160), np.int16), host.array((S * 2, bank.probes), bands.out_dtype(form))
                    _native.check(_next(L, a, bank, form, records), "next_bands")
                    _native.check(L.mbx_session_submit(a, 2, frames.ctypes.data, pcm16.ctypes.data, None, None), "submit")
                    _native.check(L.mbx_session_wait(a), "wait")
                    assert records.tobytes() == bands.measure(pcm16, p, form).tobytes(), k
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)
        host.close()


def test_frames_indexed_burst_and_burst_group_submits_deliver_the_records_and_the_levels_beside_them(mbx):
    """frames (T = 1 and 2), indexed, bursts and burst groups; every other one also carries a levels attachment on the same submit"""
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    codec, F = 0, 2
    h = _session(L, codec, S, S * F, PCM16 | LEVELS)
    rng = np.random.default_rng(8)
    sched = B.random_schedule(codec, F, F * B.channel_bits(codec) + 120, rng, device=True)
    p = bands.dtmf("hann")
    count = [0]
    try:
        with _bank(p) as bank:
            def run(what, rows, submit):
                k = count[0]
                count[0] += 1
                form = bands.FORMS[k % 2]
                pcm16 = np.full((rows, 160), 0x5A5A, np.int16)
                records = np.full((rows, 8), FILL, np.uint8).repeat(bands.record_bytes(form), axis=1).view(bands.out_dtype(form))
                lv = np.full(rows * 16, FILL, np.uint8).view(levels.LEVEL_DTYPE)
                _native.check(_next(L, h, bank, form, records), "next_bands")
                if k % 2:
                    _native.check(L.mbx_session_next_levels(h, lv.ctypes.data), "next_levels")
                _native.check(submit(pcm16.ctypes.data), what)
                _native.check(L.mbx_session_wait(h), "wait")
                assert not _untouched(pcm16) and len(np.unique(pcm16)) > 100, what
                assert records.tobytes() == bands.measure(pcm16, p, form).tobytes(), what
                assert lv.tobytes() == levels.measure(pcm16).tobytes() if k % 2 else _untouched(lv), what

            for T in (1, 2):
                plain = np.ascontiguousarray(edge_mix.frames(codec, S, T, 9 + T).reshape(S * T, -1))
                run(f"frames T={T}", S * T, lambda q: L.mbx_session_submit(h, T, plain.ctypes.data, q, None, None))
            index = np.array([1, 64, 4, 69, 31], dtype=np.int32)
            frames = np.ascontiguousarray(edge_mix.frames(codec, 5, 2, 11).reshape(10, -1))
            run("indexed", 10, lambda q: L.mbx_session_submit_indexed(h, 5, 2, index.ctypes.data, frames.ctypes.data, q, None, None, None))
            carried = edge_mix.frames(codec, S, F, 15).reshape(S * F, -1)
            bursts = np.ascontiguousarray(burst_cases.make_bursts(sched, carried, rng))
            run("bursts", S * F, lambda q: L.mbx_session_submit_bursts(h, sched.handle, S, None, bursts.ctypes.data, sched.burst_bytes, q, None, None))
            shapes = ((codec, F, B.FORM_PACKED, False, 3, 1, 0),)
            scheds = G.schedules(shapes, 17)
            groups = G.make_groups(shapes, scheds, False, 18, tag=2, slots=[np.array([66, 2, 40], dtype=np.int32)])
            arr, keep = G.group_array(L, groups)
            run("burst groups", 3 * F, lambda q: L.mbx_session_submit_burst_groups(h, arr, 1, 0, q, None, None))
            for s in scheds:
                s.close()
    finally:
        L.mbx_session_destroy(h)
        sched.close()


def test_a_mixed_session_of_eight_streams_delivers_the_records_of_a_burst_group_submit(mbx):
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    codec_of = np.array([0, 1, 2, 3, 3, 2, 1, 0], dtype=np.uint8)
    # (codec, frames per burst, form, inversion sequence, streams, bursts per stream, extra bytes of burst_stride)
    shapes = ((0, 2, B.FORM_PACKED, False, 2, 1, 0), (1, 3, B.FORM_DIBITS, True, 2, 2, 0), (3, 1, B.FORM_BITS, False, 2, 1, 0), (2, 1, B.FORM_PACKED, False, 2, 1, 3))
    total = sum(g[1] * g[4] * g[5] for g in shapes)
    slots = [np.flatnonzero(codec_of == g[0]).astype(np.int32)[::-1].copy() for g in shapes]
    scheds = G.schedules(shapes, 21)
    p = bands.dtmf("rect")
    h, twin = C.c_void_p(), C.c_void_p()
    _native.check(L.mbx_session_create_mixed(C.byref(h), 8, codec_of.ctypes.data, total, PCM8), "create_mixed")
    _native.check(L.mbx_session_create_mixed(C.byref(twin), 8, codec_of.ctypes.data, total, PCM16), "create_mixed (twin)")
    try:
        with _bank(p) as bank:
            for tick, form in enumerate(bands.FORMS):
                groups = G.make_groups(shapes, scheds, False, 22 + tick, tag=3 + tick, slots=slots)
                arr, keep = G.group_array(L, groups)
                records, pcm16 = np.zeros((total, 8), bands.out_dtype(form)), np.zeros((total, 160), np.int16)
                _native.check(_next(L, h, bank, form, records), "next_bands")
                _native.check(L.mbx_session_submit_burst_groups(h, arr, 4, 0, None, None, None), "submit_burst_groups")   # the records alone
                _native.check(L.mbx_session_submit_burst_groups(twin, arr, 4, 0, pcm16.ctypes.data, None, None), "submit_burst_groups (twin)")
                _native.check(L.mbx_session_wait(h), "wait")
                _native.check(L.mbx_session_wait(twin), "wait (twin)")
                assert len(np.unique(pcm16)) > 100
                assert records.tobytes() == bands.measure(pcm16, p, form).tobytes(), tick
    finally:
        L.mbx_session_destroy(h)
        L.mbx_session_destroy(twin)
        for s in scheds:
            s.close()


def test_behind_a_filter_and_an_agc_the_records_are_of_the_filtered_levelled_rows(mbx):
    """filter + AGC + levels + bands attached together: the records are those of numpy's chain filters.step -> agc.step -> bands.measure,
    and not those of the rows as decoded"""
    from mbelib_neo_amd import _native

    L = _native.lib()
    n, T = 40, 1
    a, b = _session(L, 0, n, n * T, PCM16 | LEVELS), _session(L, 0, n, n * T, PCM16)
    f = filters.highpass(300, 2)
    g = agc_cases.params("voice", 6)
    p = bands.dtmf("hann")
    try:
        with filters.FilterState(n) as fstate, agc.AgcState(n) as astate, _bank(p) as bank:
            fst, ast = filters.fresh_state(n), agc.fresh_state(n)
            for k in range(3):
                frames = np.ascontiguousarray(edge_mix.frames(0, n, T, 21 + k).reshape(n * T, -1))
                form = bands.FORMS[k % 2]
                own16, twin16 = np.zeros((n * T, 160), np.int16), np.zeros((n * T, 160), np.int16)
                records, lv = np.zeros((n * T, 8), bands.out_dtype(form)), np.zeros(n * T, dtype=levels.LEVEL_DTYPE)
                _native.check(_next(L, a, bank, form, records), "next_bands")   # (attached first: the order is the library's)
                _native.check(L.mbx_session_next_agc(a, C.addressof(g), astate.handle), "next_agc")
                _native.check(L.mbx_session_next_filter(a, C.addressof(f), fstate.handle), "next_filter")
                _native.check(L.mbx_session_next_levels(a, lv.ctypes.data), "next_levels")
                _native.check(L.mbx_session_submit(a, T, frames.ctypes.data, own16.ctypes.data, None, None), "submit")
                _native.check(L.mbx_session_submit(b, T, frames.ctypes.data, twin16.ctypes.data, None, None), "submit (twin)")
                _native.check(L.mbx_session_wait(a), "wait")
                _native.check(L.mbx_session_wait(b), "wait (twin)")
                filtered, fst = filters.step(f, fst, T, twin16)
                want, ast, _ = agc.step(filtered, T, g, ast)
                assert own16.tobytes() == want.tobytes() and want.tobytes() != twin16.tobytes(), k
                assert records.tobytes() == bands.measure(want, p, form).tobytes(), k
                assert records.tobytes() != bands.measure(twin16, p, form).tobytes() and records.tobytes() != bands.measure(filtered, p, form).tobytes(), k
                assert lv.tobytes() == levels.measure(want).tobytes(), k
    finally:
        L.mbx_session_destroy(a)
        L.mbx_session_destroy(b)


def test_the_attachment_lasts_for_one_submit_whether_it_queues_or_refuses_and_its_two_refusals(mbx):
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

    L = _native.lib()
    codec = 0
    frames = {T: np.ascontiguousarray(edge_mix.frames(codec, S, T, 30 + T).reshape(S * T, -1)) for T in (1, 2, 3)}
    sessions = {bits: _session(L, codec, S, S * 2, bits) for bits in (PCM16, PCMF, RESULTS, PCMF | RESULTS, PCM8, LEVELS)}
    s = sessions[PCM16]
    p = bands.dtmf("rect")
    try:
        with _bank(p) as bank:
            def submit(h, T, pcm16):
                return L.mbx_session_submit(h, T, frames[T].ctypes.data, None if pcm16 is None else pcm16.ctypes.data, None, None)

            def fresh(form=bands.POWER):
                return np.full((S * 2, 8), FILL, np.uint8).repeat(bands.record_bytes(form), axis=1).view(bands.out_dtype(form))

            def refused(part, *args):
                L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
                assert L.mbx_session_next_bands(*args) == INVALID
                assert b"mbx_session_next_bands: " + part in L.mbx_last_error(), L.mbx_last_error()

            records = fresh()
            pcm16 = np.zeros((S * 2, 160), np.int16)
            # the refusals: a session without an output that has int16 rows; no bank; the form; (a bank of another device: below)
            for bits in (PCMF, RESULTS, PCMF | RESULTS):
                refused(b"the session was created without an output that has int16 rows", sessions[bits], bank.handle, bands.POWER, records.ctypes.data)
            refused(b"no bank", s, None, bands.POWER, records.ctypes.data)
            refused(b"form is MBX_BANDS_COMPLEX or MBX_BANDS_POWER", s, bank.handle, 2, records.ctypes.data)
            assert submit(s, 1, pcm16) == 0 and L.mbx_session_wait(s) == 0 and _untouched(records)   # none of them left anything
            # queued: delivered once, and the submit after it delivers nothing
            _native.check(_next(L, s, bank, bands.POWER, records), "next_bands")
            assert submit(s, 2, pcm16) == 0 and L.mbx_session_wait(s) == 0
            assert records.tobytes() == bands.measure(pcm16, p, bands.POWER).tobytes()
            records = fresh()
            assert submit(s, 1, pcm16) == 0 and L.mbx_session_wait(s) == 0 and _untouched(records)
            # refused (T beyond max_frames_per_submit): used up, nothing queued
            _native.check(_next(L, s, bank, bands.POWER, records), "next_bands")
            assert submit(s, 3, pcm16) == INVALID
            assert submit(s, 2, pcm16) == 0 and L.mbx_session_wait(s) == 0 and _untouched(records)
            # NULL clears it
            _native.check(_next(L, s, bank, bands.POWER, records), "next_bands")
            assert _next(L, s, bank, bands.POWER, None) == 0 and _next(L, s, None, 7, None) == 0
            assert submit(s, 1, pcm16) == 0 and L.mbx_session_wait(s) == 0 and _untouched(records)
            # whichever call came last holds
            first = fresh(bands.COMPLEX)
            _native.check(_next(L, s, bank, bands.COMPLEX, first), "next_bands")
            _native.check(_next(L, s, bank, bands.POWER, records), "next_bands")
            assert submit(s, 1, pcm16) == 0 and L.mbx_session_wait(s) == 0 and _untouched(first)
            assert records[:S].tobytes() == bands.measure(pcm16[:S], p, bands.POWER).tobytes() and _untouched(records[S:])
            # seed, get_state, set_state and reset leave it for the submit
            records = fresh(bands.COMPLEX)
            _native.check(_next(L, s, bank, bands.COMPLEX, records), "next_bands")
            st, rg = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
            seeds = np.arange(S, dtype=np.uint32) + 9
            _native.check(L.mbx_session_reset(s, 0, S), "reset")
            _native.check(L.mbx_session_seed(s, 0, S, seeds.ctypes.data), "seed")
            _native.check(L.mbx_session_get_state(s, 0, S, st.ctypes.data, rg.ctypes.data), "get_state")
            _native.check(L.mbx_session_set_state(s, 0, S, st.ctypes.data, rg.ctypes.data), "set_state")
            assert submit(s, 2, pcm16) == 0 and L.mbx_session_wait(s) == 0
            assert records.tobytes() == bands.measure(pcm16, p, bands.COMPLEX).tobytes()
            # sessions created for the bytes or for the level records alone: they have no pcm16 to give, and their band records are those
            # of the same frames' pcm16
            for bits in (PCM8, LEVELS):
                only = sessions[bits]
                for h in (s, only):
                    _native.check(L.mbx_session_reset(h, 0, S), "reset")
                    _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
                assert submit(only, 1, pcm16) == INVALID
                alone = fresh()
                _native.check(_next(L, only, bank, bands.POWER, alone), "next_bands")
                assert submit(only, 2, None) == 0 and L.mbx_session_wait(only) == 0
                assert submit(s, 2, pcm16) == 0 and L.mbx_session_wait(s) == 0
                assert alone.tobytes() == bands.measure(pcm16, p, bands.POWER).tobytes() and len(np.unique(pcm16)) > 100, bits
    finally:
        for h in sessions.values():
            L.mbx_session_destroy(h)


def test_a_bank_of_another_device_is_refused_by_the_launcher_and_by_the_session(mbx):
    """where two devices are visible: a bank made on device 1 against a launch and a session of device 0"""
    import torch
    from mbelib_neo_amd import _native, decoder

    if torch.cuda.device_count() < 2:
        pytest.skip("one device visible: a bank of another device cannot be made")
    L = _native.lib()
    decoder.ensure_init(1)
    p = bands.dtmf("rect")
    with torch.cuda.device(1):
        other = _bank(p)
    s = None
    try:
        with torch.cuda.device(0):
            decoder.ensure_init(0)
            d = torch.zeros((16, 160), dtype=torch.int16, device="cuda:0")
            out = torch.full((16 * 8 * 4,), FILL, dtype=torch.uint8, device="cuda:0")
            assert _launch(other, bands.POWER, d.data_ptr(), 16, out.data_ptr()) == INVALID
            assert b"mbx_pcm_bands: a bank of another device than the current one" in L.mbx_last_error()
            s = _session(L, 0, 4, 4, PCM16)
            records = np.zeros((4, 8), np.uint32)
            assert _next(L, s, other, bands.POWER, records) == INVALID
            assert b"mbx_session_next_bands: a bank of another device than the session" in L.mbx_last_error()
            torch.cuda.synchronize()
            assert (out.cpu().numpy() == FILL).all()
    finally:
        if s is not None:
            L.mbx_session_destroy(s)
        other.close()


# ---- 7. BatchDecoder.bands ------------------------------------------------------------------------------------------------------------------------
def test_batchdecoder_bands_against_numpy_with_and_without_out(mbx):
    import torch
    from mbelib_neo_amd import decoder

    x, p, want = bands_cases.case(65, 17)
    dec = decoder.BatchDecoder(0, 4)
    d = torch.from_numpy(np.array(x)).cuda()
    with _bank(p) as bank:
        for form in bands.FORMS:
            got = dec.bands(d, bank, form)
            own = torch.full((65, 17 * bands.record_bytes(form)), FILL, dtype=torch.uint8, device="cuda")
            assert dec.bands(d, bank, form=form, out=own) is own
            torch.cuda.synchronize()
            for t in (got, own):
                assert t.dtype == torch.uint8 and t.cpu().numpy().view(bands.out_dtype(form)).reshape(65, 17).tobytes() == want[form].tobytes(), form
        with pytest.raises(ValueError):
            dec.bands(d.to(torch.int32), bank)
        with pytest.raises(ValueError):
            dec.bands(d, bank, form=2)
        with pytest.raises(ValueError):
            dec.bands(d, bank, out=torch.zeros(5, dtype=torch.uint8, device="cuda"))
    with pytest.raises(Exception, match=r"probe 0: the \|c\[n\]\| sum to 65536"):
        over = np.zeros((1, 2, 160), np.int16)
        over[0, 0, :3] = [32767, 32767, 2]
        decoder.Bank(over)
    with pytest.raises(Exception, match="K is 1 .. MBX_BANDS_MAX_PROBES"):
        decoder.Bank(np.zeros((33, 2, 160), np.int16))
