"""GPU suite (-m gpu) for soft bursts as LLRs (include/mbx_burst.h: mbx_burst_schedule_create_llr; include/mbx_llr.h:
mbx_soft_from_llr).  The conversion is the host function mbx_soft_bits_from_llr, which tests/test_llr_bursts_host.py holds to the
reference-made fixture over every value; every LLR path is held, byte for byte, to the same call with the PER-BIT schedule of the
same arrays and sequence on the host-converted cells: the gather alone at every byte phase of its input, the burst launches, the
session submits; the hard calls refuse an LLR schedule; the flat conversion equals the host function at every pointer phase.
Inputs and outputs sit between bands of bytes that must keep what they hold (tests/llr_burst_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import llr_burst_cases as cases
import symbol_burst_cases
from burst_cases import CELLS

pytestmark = pytest.mark.gpu
WIDTH_IDS = {2: "int16", 1: "int8"}


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _sync():
    import torch

    torch.cuda.synchronize()


def _strm():
    import torch

    return torch.cuda.current_stream().cuda_stream


# ---- the gather alone -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("masked", [False, True], ids=["plain", "masked"])
@pytest.mark.parametrize("llr_bytes", [2, 1], ids=["int16", "int8"])
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_gather_of_llr_bursts_is_the_per_bit_gather_of_the_host_converted_cells(mbx, codec, llr_bytes, masked):
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    rng = np.random.default_rng(6000 + 100 * codec + 10 * llr_bytes + masked)
    for F, nbits in cases.gather_shapes(codec):
        mask = rng.integers(0, 2, size=nbits, dtype=np.uint8) if masked else None
        s = B.random_schedule(codec, F, nbits, rng, device=True, form=cases.WIDTHS[llr_bytes], invert=mask)
        per_bit = s.in_form(B.FORM_PACKED, mask, device=True)
        cases.check_accessors(L, s)
        for n in cases.counts(llr_bytes, nbits):
            llr = cases.random_llrs(rng, n, s, llr_bytes)
            cells = cases.host_cells(L, llr)
            want = B.deinterleave(per_bit, cells, soft=True).cpu().numpy()   # the existing <per-bit> instance of the same schedule
            assert want.shape == (n * F, CELLS[codec], 2) and np.array_equal(want, B.apply_schedule(s, llr, soft=True))
            for phase in ((0, 1, 2, 3) if llr_bytes == 1 else (0, 2)):
                src = cases.Guarded(llr.nbytes, phase, rng).load(llr)
                for row_cells in (CELLS[codec], B.MIXED_ROW_CELLS):
                    what = f"codec {codec}, {WIDTH_IDS[llr_bytes]}, F {F}, {nbits} bits, n {n}, input at +{phase}, rows of {row_cells} cells, masked {masked}"
                    out = cases.Guarded(n * F * row_cells * 2, 2, rng)   # (rows at exactly their alignment of 2)
                    _native.check(L.mbx_deinterleave_soft(s.handle, src.ptr, n, out.ptr, row_cells, _strm()), "mbx_deinterleave_soft")
                    _sync()
                    got = out.check(what).reshape(n * F, row_cells, 2)
                    assert np.array_equal(got[:, :CELLS[codec]], want), what
                    assert not got[:, CELLS[codec]:].any(), what + ": the tail of a mixed row is {0, 0}"
                src.check("the LLR bursts", unchanged=True)
        # below its alignment an int16 burst array is refused, an int8 one has none to be below of
        odd = cases.Guarded(2 * nbits, 1, rng)
        out = cases.Guarded(F * CELLS[codec] * 2, 2, rng)
        rc = L.mbx_deinterleave_soft(s.handle, odd.ptr, 1, out.ptr, CELLS[codec], _strm())
        _sync()
        if llr_bytes == 2:
            assert rc == cases.INVALID_ARGUMENT and b"mbx_deinterleave_soft" in L.mbx_last_error() and b"alignment" in L.mbx_last_error()
            out.check("a refused gather", unchanged=True)
        else:
            assert rc == 0
        assert L.mbx_deinterleave_soft(s.handle, odd.ptr + 1, 0, out.ptr, CELLS[codec], _strm()) == 0, "n = 0 launches nothing"
        s.close()
        per_bit.close()


# ---- burst launches ---------------------------------------------------------------------------------------------------------------------
def _launch(L, _native, handle, S, bursts, inputs):
    """mbx_process_bursts_soft on plain allocations: (every output and the state as uint8 arrays by name, the stream-stage instance)"""
    import torch

    mc = symbol_burst_cases.memory_cases
    F = L.mbx_burst_schedule_frames(handle)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda() for k, v in {**inputs, "bursts": bursts}.items()}
    outs = {k: torch.zeros(S * F * mc.OUT_BYTES[k], dtype=torch.uint8, device="cuda") for k in mc.OUT_ORDER}
    ptr = lambda k: dev[k].data_ptr() if k in dev else None   # noqa: E731
    rc = L.mbx_process_bursts_soft(handle, S, ptr("index"), dev["bursts"].data_ptr(), dev["state"].data_ptr(), ptr("resident"), dev["rng"].data_ptr(),
                                   outs["pcm16"].data_ptr(), outs["pcmf"].data_ptr(), outs["results"].data_ptr(), outs["records"].data_ptr(), _strm())
    _native.check(rc, "mbx_process_bursts_soft")
    name = L.mbx_last_kernel_name(_strm())
    _sync()
    return {k: v.cpu().numpy() for k, v in {**outs, **{k: dev[k] for k in ("state", "rng", "resident") if k in dev}}.items()}, name


@pytest.mark.parametrize("S", [1, 65, 300])
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "abi"])
@pytest.mark.parametrize("codec,F", [(0, 3), (1, 1)])
def test_burst_launches_from_llr_bursts_are_the_per_bit_launch(mbx, codec, F, resident, S):
    """(S * F = 3, 195, 900 and 1, 65, 300 frames: both sides of the 256-frame small-batch rule of the launch plan)"""
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    rng = np.random.default_rng(7000 + 100 * codec + 10 * resident + S)
    nbits = F * B.channel_bits(codec) + 59
    arrays = B.random_schedule(codec, F, nbits, rng, invert=rng.integers(0, 2, size=nbits, dtype=np.uint8))
    inputs, _ = symbol_burst_cases.launch_buffers(codec, F, S, S + 20, resident, True, rng)   # with d_stream_index
    assert ("resident" in inputs) == resident and "index" in inputs
    per_bit = arrays.in_form(B.FORM_PACKED, arrays.invert, device=True)
    carried = symbol_burst_cases.carried_bursts(arrays, codec, S, F, True, rng, tag=F)   # per-bit cells as received, valid frames under the schedule
    for llr_bytes, form in cases.WIDTHS.items():
        s = arrays.in_form(form, arrays.invert, device=True)
        llr = cases.llrs_carrying(carried, llr_bytes)
        assert llr.shape == (S, nbits) and llr.dtype == cases.DTYPE[llr_bytes]
        want, name = _launch(L, _native, per_bit.handle, S, cases.host_cells(L, llr), inputs)
        got, got_name = _launch(L, _native, s.handle, S, llr, inputs)
        assert got_name == name and name
        assert set(got) == set(want) and ("resident" in want) == resident
        for k, v in want.items():
            assert np.array_equal(got[k], v), f"{WIDTH_IDS[llr_bytes]}: {k} differs from the per-bit launch"
        # (the launch did decode something; the one frame of S = F = 1 may be a silent one)
        assert want["records"].any() and (S * F == 1 or want["pcm16"].any())
        s.close()
    per_bit.close()


def test_decode_bursts_takes_llr_arrays_and_tensors(mbx):
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder

    L = _native.lib()
    rng = np.random.default_rng(19)
    S, F = 33, 3
    arrays = B.random_schedule(1, F, 301, rng, invert=rng.integers(0, 2, size=301, dtype=np.uint8))
    per_bit = arrays.in_form(B.FORM_PACKED, arrays.invert, device=True)
    carried = symbol_burst_cases.carried_bursts(arrays, 1, S, F, True, rng, tag=1)
    for llr_bytes, form in cases.WIDTHS.items():
        s = arrays.in_form(form, arrays.invert, device=True)
        llr = cases.llrs_carrying(carried, llr_bytes)
        a, b, c = (decoder.BatchDecoder(1, S, seeds=np.arange(S) + 3, resident=True) for _ in range(3))
        out_a = a.decode_bursts(s, llr, soft=True, want_float=True)
        out_b = b.decode_bursts(per_bit, cases.host_cells(L, llr), soft=True, want_float=True)
        out_c = c.decode_bursts(s, torch.from_numpy(llr).cuda(), soft=True, want_float=True)
        torch.cuda.synchronize()
        for k in ("records", "results", "pcm16", "pcmf"):
            assert torch.equal(out_a[k], out_b[k]) and torch.equal(out_c[k], out_b[k]), k
        assert torch.equal(a.state, b.state) and torch.equal(a.rng, b.rng) and torch.equal(a.resident, b.resident)
        with pytest.raises(ValueError):   # one LLR short
            a.decode_bursts(s, llr.reshape(-1)[:-1], soft=True)
        s.close()
    per_bit.close()


# ---- sessions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("llr_bytes", [2, 1], ids=["int16", "int8"])
@pytest.mark.parametrize("codec,F", [(0, 9), (1, 3)])
def test_session_submits_of_llr_bursts_return_the_bytes_of_the_per_bit_submits(mbx, codec, F, llr_bytes):
    from mbelib_neo_amd import _native, bursts as B
    from mbelib_neo_amd.layout import PARMS_DTYPE, RESULT_DTYPE, RNG_DTYPE

    L = _native.lib()
    S, n2 = 41, 40   # 41 streams, room for 40 bursts a submit
    rng = np.random.default_rng(8000 + 10 * codec + llr_bytes)
    nbits = F * B.channel_bits(codec) + 123   # odd: an int8 burst is no whole number of cells
    arrays = B.random_schedule(codec, F, nbits, rng, invert=rng.integers(0, 2, size=nbits, dtype=np.uint8))
    s = arrays.in_form(cases.WIDTHS[llr_bytes], arrays.invert, device=True)
    per_bit = arrays.in_form(B.FORM_PACKED, arrays.invert, device=True)
    seeds = (np.arange(S) * 3 + 5).astype(np.uint32)
    sess = [C.c_void_p(), C.c_void_p()]
    for h in sess:
        _native.check(L.mbx_session_create(C.byref(h), codec, S, n2 * F, 1 | 2 | 4), "create")
        _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
    a, b = sess

    def state_of(h):
        st, rg = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
        _native.check(L.mbx_session_get_state(h, 0, S, st.ctypes.data, rg.ctypes.data), "get_state")
        return st.view(np.uint8).copy(), rg.view(np.uint8).copy()

    def outputs(n):
        return np.zeros((n * F, 160), np.int16), np.zeros((n * F, 160), np.float32), np.zeros(n * F, RESULT_DTYPE)

    pinned = L.mbx_host_alloc(S * nbits * 2 + 64)
    assert pinned
    try:
        for step, pin in enumerate([False, True, True, False]):
            n = n2 if step < 3 else 17   # n * F == max_frames_per_submit is accepted
            index = rng.permutation(S)[:n].astype(np.int32)
            llr = cases.llrs_carrying(symbol_burst_cases.carried_bursts(arrays, codec, n, F, True, rng, tag=step), llr_bytes)
            cells = cases.host_cells(L, llr)
            src = llr
            if pin:   # (submit 2: pinned memory that is not 16-byte aligned is staged, like pageable memory)
                at = 16 * step + (llr_bytes if step == 2 else 0)
                src = np.ctypeslib.as_array((C.c_uint8 * llr.nbytes).from_address(pinned + at))
                src[:] = llr.reshape(-1).view(np.uint8)
            oa, ob = outputs(n), outputs(n)
            pa, pb = [x.ctypes.data for x in oa], [x.ctypes.data for x in ob]
            if step == 0:   # one burst more than max_frames_per_submit holds: refused, nothing queued, nothing moved
                more = np.concatenate([index, [i for i in range(S) if i not in index][:1]]).astype(np.int32)
                big = np.concatenate([llr, llr[:1]])
                ox = outputs(n + 1)
                before = state_of(a)
                assert L.mbx_session_submit_bursts_soft(a, s.handle, n + 1, more.ctypes.data, big.ctypes.data, *[x.ctypes.data for x in ox]) == cases.INVALID_ARGUMENT
                assert b"mbx_session_submit_bursts_soft" in L.mbx_last_error()
                _native.check(L.mbx_session_wait(a), "wait")
                after = state_of(a)
                assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "a refused submit moved the state"
                assert not any(x.view(np.uint8).any() for x in ox), "a refused submit wrote an output"
            _native.check(L.mbx_session_submit_bursts_soft(a, s.handle, n, index.ctypes.data, src.ctypes.data, *pa), "LLR submit")
            _native.check(L.mbx_session_submit_bursts_soft(b, per_bit.handle, n, index.ctypes.data, cells.ctypes.data, *pb), "per-bit submit")
            _native.check(L.mbx_session_wait(a), "wait")
            _native.check(L.mbx_session_wait(b), "wait")
            for u, v, k in zip(oa, ob, ("pcm16", "pcmf", "results")):
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8)) and (k == "results" or u.any()), f"submit {step} (pinned {pin}): {k}"
        sa, sb = state_of(a), state_of(b)
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
        # every LLR is a valid one: the host check says so, and says that an LLR schedule has no hard bursts
        assert L.mbx_burst_validate(s.handle, llr.ctypes.data, 0, n, 1) == 0
        assert L.mbx_burst_validate(s.handle, None, 0, n, 1) == cases.INVALID_ARGUMENT
        assert L.mbx_burst_validate(s.handle, llr.ctypes.data, nbits, n, 0) == cases.INVALID_ARGUMENT
    finally:
        L.mbx_host_free(pinned)
        for h in sess:
            L.mbx_session_destroy(h)
        s.close()
        per_bit.close()


# ---- the hard calls ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("llr_bytes", [2, 1], ids=["int16", "int8"])
def test_the_hard_calls_refuse_an_llr_schedule_and_launch_nothing(mbx, llr_bytes):
    import torch
    from mbelib_neo_amd import _native, bursts as B
    from mbelib_neo_amd.layout import RESULT_DTYPE

    L = _native.lib()
    rng = np.random.default_rng(9000 + llr_bytes)
    codec, F, S, nbits = 1, 3, 5, 300
    s = B.random_schedule(codec, F, nbits, rng, device=True, form=cases.WIDTHS[llr_bytes])
    assert L.mbx_burst_schedule_bytes(s.handle) == 0
    inputs, _ = symbol_burst_cases.launch_buffers(codec, F, S, S, True, False, rng)
    mc = symbol_burst_cases.memory_cases
    sizes = {"bursts": S * nbits * 2, "frames": S * F * 18, **{k: len(v.reshape(-1).view(np.uint8)) for k, v in inputs.items()},
             **{k: S * F * mc.OUT_BYTES[k] for k in mc.OUT_ORDER}}
    g = {k: cases.Guarded(nb, 0, rng) for k, nb in sizes.items()}
    for k, v in inputs.items():
        g[k].load(v)

    def refused(who, rc):
        text = L.mbx_last_error()
        assert rc == cases.INVALID_ARGUMENT and who.encode() in text and b"LLR" in text, (who, rc, text)

    L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
    for stride in (0, 2 * nbits):
        refused("mbx_deinterleave", L.mbx_deinterleave(s.handle, g["bursts"].ptr, stride, S, g["frames"].ptr, 9, _strm()))
        refused("mbx_process_bursts", L.mbx_process_bursts(s.handle, S, None, g["bursts"].ptr, stride, g["state"].ptr, g["resident"].ptr, g["rng"].ptr,
                                                            g["pcm16"].ptr, g["pcmf"].ptr, g["results"].ptr, g["records"].ptr, _strm()))
    torch.cuda.synchronize()
    for k, buf in g.items():
        buf.check(f"{k} after the refused hard calls", unchanged=True)
    h = C.c_void_p()
    _native.check(L.mbx_session_create(C.byref(h), codec, S, S * F, 1 | 2 | 4), "create")
    try:
        host = np.zeros((S, 2 * nbits), dtype=np.uint8)
        out = np.zeros((S * F, 160), np.int16), np.zeros((S * F, 160), np.float32), np.zeros(S * F, RESULT_DTYPE)
        refused("mbx_session_submit_bursts", L.mbx_session_submit_bursts(h, s.handle, S, None, host.ctypes.data, 2 * nbits, *[x.ctypes.data for x in out]))
        _native.check(L.mbx_session_wait(h), "wait")
        assert not any(x.view(np.uint8).any() for x in out), "a refused submit wrote an output"
    finally:
        L.mbx_session_destroy(h)
        s.close()


# ---- the flat conversion ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("llr_bytes", [2, 1], ids=["int16", "int8"])
def test_soft_from_llr_equals_the_host_function_at_every_pointer_phase(mbx, llr_bytes):
    import torch
    from mbelib_neo_amd import _native, decoder

    L = _native.lib()
    rng = np.random.default_rng(9500 + llr_bytes)
    info = np.iinfo(cases.DTYPE[llr_bytes])
    # (184 * 33: three chunks of a workgroup, the last one short; 2048 * 2048 + 4099: more chunks than the grid has workgroups)
    for count in (0, 1, 3, 255, 256, 257, 184 * 33, 2048 * 2048 + 4099):
        big = count > 1 << 20
        llr = np.where(rng.integers(0, 2, size=count) == 1, rng.integers(info.min, info.max + 1, size=count), rng.integers(-300, 301, size=count).clip(info.min, info.max))
        planted = cases.PLANTED[llr_bytes]
        if count >= 2 * len(planted):
            llr[:len(planted)] = planted
            llr[count - len(planted):] = planted
        llr = llr.astype(cases.DTYPE[llr_bytes])
        want = cases.host_cells(L, llr)
        in_phases = (0, 1, 2, 3) if llr_bytes == 1 else (0, 2)
        for in_phase in (in_phases[-1:] if big else in_phases):
            src = cases.Guarded(llr.nbytes, in_phase, rng).load(llr)
            for out_phase in ((2,) if big else (0, 2)):
                what = f"{WIDTH_IDS[llr_bytes]}, count {count}, input at +{in_phase}, output at +{out_phase}"
                out = cases.Guarded(2 * count, out_phase, rng)
                _native.check(L.mbx_soft_from_llr(src.ptr, llr_bytes, count, out.ptr, _strm()), "mbx_soft_from_llr")
                _sync()
                assert np.array_equal(out.check(what).reshape(count, 2), want), what
            src.check("the LLRs", unchanged=True)
    # refusals: a NULL pointer, a width there is none of, a pointer below its alignment -- the call named, nothing written
    src, out = cases.Guarded(64, 0, rng), cases.Guarded(64, 0, rng)
    for args in ((None, llr_bytes, 8, out.ptr), (src.ptr, llr_bytes, 8, None), (src.ptr, 0, 8, out.ptr), (src.ptr, 4, 8, out.ptr), (src.ptr, llr_bytes, 8, out.ptr + 1)) + \
            (((src.ptr + 1, 2, 8, out.ptr),) if llr_bytes == 2 else ()):
        L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
        assert L.mbx_soft_from_llr(*args, _strm()) == cases.INVALID_ARGUMENT and b"mbx_soft_from_llr" in L.mbx_last_error(), args
    _sync()
    out.check("refused conversions", unchanged=True)
    # the wrapper, on frame-shaped LLRs
    frames = rng.integers(info.min, info.max + 1, size=(7, 8, 23)).astype(cases.DTYPE[llr_bytes])
    cells = decoder.soft_from_llr(torch.from_numpy(frames).cuda())
    assert cells.shape == (7, 8, 23, 2) and np.array_equal(cells.cpu().numpy(), cases.host_cells(L, frames))
    assert np.array_equal(decoder.soft_bits_from_llr(frames.astype(np.int16)), cases.host_cells(L, frames))
