"""GPU suite (-m gpu) for burst input in the receiver's forms (include/mbx_burst.h, mbx_burst_schedule_create_form): bursts of bit
bytes, dibit bytes and soft dibit pairs, and a fixed inversion sequence.  Every form is held to the PACKED form, which
tests/test_gpu_bursts.py holds to the oracle, so every comparison here is exact: the gathers against the numpy definition
(bursts.apply_schedule) and against the packed schedule on host-scrambled packed bursts, the launches and the session submits
against the same calls with the packed schedule, and the device entry points between guard bands (tests/symbol_burst_cases.py)."""
import ctypes as C

import numpy as np
import pytest

import symbol_burst_cases as cases
from burst_cases import CELLS

pytestmark = pytest.mark.gpu
FB = {0: 18, 1: 9, 2: 18, 3: 9}


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _at_offset(a, off):
    """the bytes of `a` on the device at an address that is `off` past a 256-byte boundary"""
    import torch

    raw = np.ascontiguousarray(a).reshape(-1).view(np.uint8)
    t = torch.empty(raw.size + 256, dtype=torch.uint8, device="cuda")
    v = t[off:off + raw.size]
    v.copy_(torch.from_numpy(raw.copy()))
    assert v.data_ptr() % 256 == off
    return v


# ---- the gather alone -------------------------------------------------------------------------------------------------------------------
def _check_hard(B, s, n, rng, stride, off):
    import torch

    codec, F = s.codec, s.frames_per_burst
    packed = cases.packed_input(s, n, rng, False)
    bursts = cases.strided(B.to_form(s, packed, junk=rng), stride, rng)
    want = B.apply_schedule(s, bursts, burst_stride=stride)
    assert np.array_equal(want, cases.expected(s, packed, False))
    what = f"hard gather, codec {codec}, form {s.form}, F {F}, {s.burst_bits} bits, n {n}, stride {stride}, input at +{off}"
    d = _at_offset(bursts, off)
    assert np.array_equal(B.deinterleave(s, d, burst_stride=stride).cpu().numpy(), want), what
    # mixed rows at an odd address: an AMBE row keeps its upper nine bytes
    rows = torch.full((n * F * 18 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    B.deinterleave(s, d, burst_stride=stride, mixed_rows=True, out=rows[3:3 + n * F * 18].view(n * F, 18))
    whole = rows.cpu().numpy()
    got = whole[3:3 + n * F * 18].reshape(n * F, 18)
    assert np.array_equal(got[:, :FB[codec]], want) and (got[:, FB[codec]:] == 0xA5).all(), what + ", mixed rows"
    assert (whole[:3] == 0xA5).all() and (whole[3 + n * F * 18:] == 0xA5).all()


def _check_soft(B, s, n, rng, off):
    import torch

    codec, F = s.codec, s.frames_per_burst
    packed = cases.packed_input(s, n, rng, True)
    bursts = B.to_form(s, packed, soft=True, junk=rng)
    want = B.apply_schedule(s, bursts, soft=True)
    assert np.array_equal(want, cases.expected(s, packed, True))
    what = f"soft gather, codec {codec}, form {s.form}, F {F}, {s.burst_bits} bits, n {n}, input at +{off}"
    d = _at_offset(bursts, off)
    assert np.array_equal(B.deinterleave(s, d, soft=True).cpu().numpy(), want), what
    rows = torch.full((n * F * 368 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    B.deinterleave(s, d, soft=True, mixed_rows=True, out=rows[2:2 + n * F * 368].view(n * F, 184, 2))
    whole = rows.cpu().numpy()
    got = whole[2:2 + n * F * 368].reshape(n * F, 184, 2)
    assert np.array_equal(got[:, :CELLS[codec]], want) and not got[:, CELLS[codec]:].any(), what + ", mixed rows"
    assert (whole[:2] == 0xA5).all() and (whole[2 + n * F * 368:] == 0xA5).all()


# (the packed form without a sequence: tests/test_gpu_bursts.py)
GATHERS = [(codec, name, masked) for codec in (0, 1, 2, 3) for name in cases.FORMS for masked in (False, True) if masked or name != "packed"]


@pytest.mark.parametrize("codec,form_name,masked", GATHERS, ids=[f"{c}-{f}-{'masked' if m else 'plain'}" for c, f, m in GATHERS])
def test_gather_of_every_form_equals_the_numpy_definition(mbx, codec, form_name, masked):
    from mbelib_neo_amd import bursts as B

    form = cases.FORMS[form_name]
    rng = np.random.default_rng(2000 + 100 * codec + 10 * form + masked)
    shapes = [(3, 602 if form == B.FORM_DIBITS else 601, (1, 64, 65, 97))]   # 301 dibits: odd, and no multiple of 4
    if codec == 1:
        shapes.append((1, 72, (1, 65)))   # an exact fit: no bit to spare
    if codec == 0:
        shapes.append((B.MAX_FRAMES, B.MAX_BITS, (65,)))   # the largest schedule there is
    for F, nbits, counts in shapes:
        s = B.random_schedule(codec, F, nbits, rng, device=True, form=form, invert=cases.random_mask(rng, nbits) if masked else None)
        for n in counts:
            _check_hard(B, s, n, rng, s.burst_bytes, 0)                 # tight
            _check_hard(B, s, n, rng, s.burst_bytes + 3, 1)             # the byte path, at an odd address
            _check_hard(B, s, n, rng, (s.burst_bytes + 3) & ~3, 0)      # the dword path
            _check_soft(B, s, n, rng, 0)
            _check_soft(B, s, n, rng, 2)                                # the odd-pair head phase
        s.close()


# ---- burst launches ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("resident,indexed", [(True, True), (False, False)], ids=["resident-indexed", "abi"])
@pytest.mark.parametrize("codec,F", [(0, 9), (1, 3), (2, 3), (3, 1)])
def test_burst_launches_from_every_form_are_the_packed_launch(mbx, codec, F, resident, indexed, soft):
    import torch
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    S, pool = 70, 90
    rng = np.random.default_rng(3000 + 100 * codec + 10 * F + 2 * resident + soft)
    nbits = F * B.channel_bits(codec) + 58
    arrays = B.random_schedule(codec, F, nbits, rng)
    inputs, _ = cases.launch_buffers(codec, F, S, pool, resident, indexed, rng)
    # (a soft per-bit schedule without a sequence is the packed one: it carries the sequence here)
    for form, masked in ((B.FORM_BITS, soft), (B.FORM_DIBITS, not soft), (B.FORM_PACKED, True)):
        s = arrays.in_form(form, cases.random_mask(rng, nbits) if masked else None, device=True)
        received = cases.carried_bursts(s, codec, S, F, soft, rng, tag=F)
        want, name = cases.packed_launch(L, _native, strm, s, S, F, soft, received, inputs)
        stride = s.burst_bytes + (form & 1)
        bursts = B.to_form(s, received, soft=soft, junk=rng)
        bursts = bursts if soft else cases.strided(bursts, stride, rng)
        dev = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda() for k, v in {**inputs, "bursts": bursts}.items()}
        outs = {k: torch.zeros(S * F * cases.memory_cases.OUT_BYTES[k], dtype=torch.uint8, device="cuda") for k in cases.memory_cases.OUT_ORDER}
        ptr = lambda k: dev[k].data_ptr() if k in dev else None   # noqa: E731
        tail = (dev["state"].data_ptr(), ptr("resident"), dev["rng"].data_ptr(), outs["pcm16"].data_ptr(), outs["pcmf"].data_ptr(),
                outs["results"].data_ptr(), outs["records"].data_ptr(), strm)
        if soft:
            rc = L.mbx_process_bursts_soft(s.handle, S, ptr("index"), dev["bursts"].data_ptr(), *tail)
        else:
            rc = L.mbx_process_bursts(s.handle, S, ptr("index"), dev["bursts"].data_ptr(), stride, *tail)
        _native.check(rc, "mbx_process_bursts")
        assert L.mbx_last_kernel_name(strm) == name and name
        torch.cuda.synchronize()
        got = {**outs, **{k: dev[k] for k in ("state", "rng", "resident") if k in dev}}
        assert set(got) == set(want) and ("resident" in want) == resident
        for k, v in want.items():
            assert np.array_equal(got[k].cpu().numpy(), v), f"form {form}, masked {masked}: {k} differs from the packed launch"
        assert want["pcm16"].any() and want["records"].any()
        s.close()


def test_decode_bursts_sizes_its_input_from_the_schedule(mbx):
    import torch
    from mbelib_neo_amd import bursts as B, decoder

    rng = np.random.default_rng(9)
    S, F = 33, 3
    dib = B.random_schedule(1, F, 302, rng, device=True, form=B.FORM_DIBITS, invert=cases.random_mask(rng, 302))
    packed = dib.in_form(B.FORM_PACKED, device=True)
    for soft in (False, True):
        received = cases.carried_bursts(dib, 1, S, F, soft, rng, tag=1)
        a, b = (decoder.BatchDecoder(1, S, seeds=np.arange(S) + 3, resident=True) for _ in range(2))
        out_a = a.decode_bursts(dib, B.to_form(dib, received, soft=soft), soft=soft, want_float=True)
        out_b = b.decode_bursts(packed, cases.scrambled(received, dib.invert, soft), soft=soft, want_float=True)
        torch.cuda.synchronize()
        for k in ("records", "results", "pcm16", "pcmf"):
            assert torch.equal(out_a[k], out_b[k]), k
        assert torch.equal(a.state, b.state) and torch.equal(a.rng, b.rng) and torch.equal(a.resident, b.resident)
        with pytest.raises(ValueError):   # a host array is checked: junk above a dibit is refused there ...
            a.decode_bursts(dib, B.to_form(dib, received, soft=soft, junk=rng), soft=soft)
        with pytest.raises(ValueError):   # ... and the packed size is not the dibit size
            a.decode_bursts(dib, cases.scrambled(received, dib.invert, soft), soft=soft)
    dib.close()
    packed.close()


# ---- sessions -------------------------------------------------------------------------------------------------------------------------
def test_burst_validate_on_host_memory(mbx):
    from mbelib_neo_amd import _native, bursts as B

    rng = np.random.default_rng(6)
    cases.validate_matrix(_native.lib(), lambda form: B.random_schedule(1, 3, 602, rng, device=True, form=form))


@pytest.mark.parametrize("codec,F", [(0, 9), (1, 3)])
def test_session_submits_of_dibits_return_the_bytes_of_the_packed_submits(mbx, codec, F):
    from mbelib_neo_amd import _native, bursts as B
    from mbelib_neo_amd.layout import PARMS_DTYPE, RESULT_DTYPE, RNG_DTYPE

    L = _native.lib()
    S, n2 = 120, 77
    rng = np.random.default_rng(4000 + codec)
    nbits = F * B.channel_bits(codec) + 122
    dib = B.random_schedule(codec, F, nbits, rng, device=True, form=B.FORM_DIBITS, invert=cases.random_mask(rng, nbits))
    bit = dib.in_form(B.FORM_BITS, device=True)
    packed = dib.in_form(B.FORM_PACKED, device=True)
    seeds = (np.arange(S) * 3 + 5).astype(np.uint32)
    sess = [C.c_void_p(), C.c_void_p()]
    for h in sess:
        _native.check(L.mbx_session_create(C.byref(h), codec, S, S * F, 1 | 2 | 4), "create")
        _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
    a, b = sess

    def state_of(h):
        st, rg = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
        _native.check(L.mbx_session_get_state(h, 0, S, st.ctypes.data, rg.ctypes.data), "get_state")
        return st.view(np.uint8).copy(), rg.view(np.uint8).copy()

    def outputs(n):
        return np.zeros((n * F, 160), np.int16), np.zeros((n * F, 160), np.float32), np.zeros(n * F, RESULT_DTYPE)

    pinned = L.mbx_host_alloc(S * (nbits * 2 + 64))
    assert pinned
    try:
        for step, (soft, indexed, pin) in enumerate([(False, False, False), (True, False, True), (False, True, True), (True, True, False)]):
            n = n2 if indexed else S
            index = rng.permutation(S)[:n].astype(np.int32) if indexed else None
            ip = index.ctypes.data if indexed else None
            received = cases.carried_bursts(dib, codec, n, F, soft, rng, tag=step)
            clear = cases.scrambled(received, dib.invert, soft)
            stride = dib.burst_bytes + (step & 2)
            bursts = B.to_form(dib, received, soft=soft)
            bursts = bursts if soft else cases.strided(bursts, stride, rng)
            src = bursts
            if pin:
                src = np.ctypeslib.as_array((C.c_uint8 * bursts.size).from_address(pinned))
                src[:] = bursts.reshape(-1)
            oa, ob = outputs(n), outputs(n)
            pa, pb = [x.ctypes.data for x in oa], [x.ctypes.data for x in ob]
            # one byte that is no dibit: refused, nothing queued, nothing moved
            before = state_of(a)
            bad = bursts.copy()
            if soft:
                bad[n // 2, dib.soft_cells - 1, 0] = 4
                assert L.mbx_session_submit_bursts_soft(a, dib.handle, n, ip, bad.ctypes.data, *pa) == cases.INVALID_BITS
            else:
                bad[n // 2, dib.burst_bytes - 1] = 4
                assert L.mbx_session_submit_bursts(a, dib.handle, n, ip, bad.ctypes.data, stride, *pa) == cases.INVALID_BITS
                twos = np.zeros((n, bit.burst_bytes), dtype=np.uint8)
                twos[n - 1, bit.burst_bytes - 1] = 2
                assert L.mbx_session_submit_bursts(a, bit.handle, n, ip, twos.ctypes.data, bit.burst_bytes, *pa) == cases.INVALID_BITS
            after = state_of(a)
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1]), "a refused submit moved the state"
            assert not any(x.view(np.uint8).any() for x in oa), "a refused submit wrote an output"
            if soft:
                _native.check(L.mbx_session_submit_bursts_soft(a, dib.handle, n, ip, src.ctypes.data, *pa), "dibits soft")
                _native.check(L.mbx_session_submit_bursts_soft(b, packed.handle, n, ip, clear.ctypes.data, *pb), "packed soft")
            else:
                _native.check(L.mbx_session_submit_bursts(a, dib.handle, n, ip, src.ctypes.data, stride, *pa), "dibits")
                _native.check(L.mbx_session_submit_bursts(b, packed.handle, n, ip, clear.ctypes.data, packed.burst_bytes, *pb), "packed")
            _native.check(L.mbx_session_wait(a), "wait")
            _native.check(L.mbx_session_wait(b), "wait")
            for u, v, k in zip(oa, ob, ("pcm16", "pcmf", "results")):
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8)) and (k == "results" or u.any()), f"submit {step} (soft {soft}, indexed {indexed}, pinned {pin}): {k}"
        sa, sb = state_of(a), state_of(b)
        assert np.array_equal(sa[0], sb[0]) and np.array_equal(sa[1], sb[1])
    finally:
        L.mbx_host_free(pinned)
        for h in sess:
            L.mbx_session_destroy(h)
        for s in (dib, bit, packed):
            s.close()


# ---- the memory contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", cases.CASES, ids=[c.id for c in cases.CASES])
def test_form_burst_entry_points_between_guard_bands(mbx, case):
    case.fn(**case.args)
