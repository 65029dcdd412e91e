"""GPU suite (-m gpu) for burst input (include/mbx_burst.h).  The gather kernels are held byte for byte to the numpy definition
(bursts.apply_schedule); the burst launches and the session submits byte for byte to the frames calls on the frames the host would
have built, and every stream to the CPU oracle through tests/parity.py; every entry point with a device pointer runs between guard
bands (tests/burst_cases.py).  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import burst_cases
import edge_mix
import parity
import soft_mix
from burst_cases import CELLS, make_bursts

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


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


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
def _check_gather(B, s, n, rng, pad, off):
    import torch

    codec, F = s.codec, s.frames_per_burst
    stride = s.burst_bytes + pad
    bursts = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    want = B.apply_schedule(s, bursts, burst_stride=stride)
    d = _at_offset(bursts, off)
    got = B.deinterleave(s, d, burst_stride=stride)
    assert np.array_equal(got.cpu().numpy(), want), f"hard gather, codec {codec}, n {n}, stride {stride}, input at +{off}"
    # 18-byte rows at an odd address: an AMBE row keeps its upper nine bytes, an IMBE row is the dense case again
    rows = torch.full((n * F * 18 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    out = rows[3:3 + n * F * 18].view(n * F, 18)
    B.deinterleave(s, d, burst_stride=stride, mixed_rows=True, out=out)
    torch.cuda.synchronize()
    whole = rows.cpu().numpy()
    got = whole[3:3 + n * F * 18].reshape(n * F, 18)
    assert np.array_equal(got[:, :FB[codec]], want) and (got[:, FB[codec]:] == 0xA5).all() and (whole[:3] == 0xA5).all() and (whole[3 + n * F * 18:] == 0xA5).all()
    soft = rng.integers(0, 256, size=(n, s.burst_bits, 2), dtype=np.uint8)
    soft[:, :, 0] &= 1
    want = B.apply_schedule(s, soft, soft=True)
    d = _at_offset(soft, off & ~1)
    assert np.array_equal(B.deinterleave(s, d, soft=True).cpu().numpy(), want), f"soft gather, codec {codec}, n {n}"
    rows = torch.full((n * F * 184 * 2 + 256,), 0xA5, dtype=torch.uint8, device="cuda")
    out = rows[2:2 + n * F * 368].view(n * F, 184, 2)
    B.deinterleave(s, d, soft=True, mixed_rows=True, out=out)
    whole = rows.cpu().numpy()
    got = whole[2:2 + n * F * 368].reshape(n * F, 184, 2)
    assert np.array_equal(got[:, :CELLS[codec]], want) and not got[:, CELLS[codec]:].any(), "mixed soft rows: the codec's cells, then zeros"
    assert (whole[:2] == 0xA5).all() and (whole[2 + n * F * 368:] == 0xA5).all()


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_gather_equals_the_numpy_definition_for_random_schedules(mbx, codec):
    from mbelib_neo_amd import bursts as B

    rng = np.random.default_rng(900 + codec)
    for F, extra in ((3, 165), (9, 432 if codec in (0, 2) else 1080)):
        s = B.random_schedule(codec, F, F * B.channel_bits(codec) + extra + (codec & 1), rng, device=True)
        for n in (1, 31, 32, 33, 257, 4099):
            pad, off = ((0, 0), (4 - s.burst_bytes % 4, 0), (5, 1))[n % 3]   # dense, dword path, byte path at an odd address
            _check_gather(B, s, n, rng, pad, off)
        s.close()


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_gather_of_a_schedule_a_person_can_follow(mbx, codec):
    """48 bits that are not voice, then F frames back to back with the bits of each frame in row-major cell order: the frames come
    out as the packers make them from those cells"""
    from mbelib_neo_amd import _native, bursts as B
    from mbelib_neo_amd.layout import FRAME_CELLS, ROW_WIDTHS

    L = _native.lib()
    F, n = 4, 65
    s = B.gap_schedule(codec, F, gap=48, device=True)
    rng = np.random.default_rng(codec)
    bits = rng.integers(0, 2, size=(n, s.burst_bits), dtype=np.uint8)
    rows, stride = FRAME_CELLS[codec]
    cells = np.zeros((n, F, rows, stride), dtype=np.int8)
    at = 48
    for k in range(F):
        for r, w in enumerate(ROW_WIDTHS[codec]):
            cells[:, k, r, :w] = bits[:, at:at + w]
            at += w
    packed = np.zeros((n * F, FB[codec]), dtype=np.uint8)
    pack = {0: L.mbx_pack_imbe7200x4400, 1: L.mbx_pack_ambe3600x2450, 2: L.mbx_pack_imbe7100x4400, 3: L.mbx_pack_ambe3600x2450}[codec]
    assert pack(cells.ctypes.data, n * F, packed.ctypes.data) == 0
    bursts = np.packbits(bits, axis=1)
    assert np.array_equal(B.deinterleave(s, bursts).cpu().numpy(), packed)
    assert np.array_equal(B.apply_schedule(s, bursts), packed)
    soft = np.stack([bits, rng.integers(0, 256, size=bits.shape, dtype=np.uint8)], axis=-1)
    got = B.deinterleave(s, soft, soft=True).cpu().numpy()
    assert np.array_equal(got[:, :, 0].reshape(cells.shape), cells.astype(np.uint8)) and np.array_equal(got, B.apply_schedule(s, soft, soft=True))


# ---- burst launches ---------------------------------------------------------------------------------------------------------------------
def _frames_call(L, dec, codec, n, F, index, d_frames, soft, out, strm):
    ptr = lambda t: t.data_ptr() if t is not None else None   # noqa: E731
    outs = (ptr(out["pcm16"]), ptr(out["pcmf"]), ptr(out["results"]), out["records"].data_ptr(), strm)
    if soft:
        return L.mbx_process_batch_soft_resident(codec, n, F, ptr(index), d_frames.data_ptr(), dec.state.data_ptr(), ptr(dec.resident), dec.rng.data_ptr(), *outs)
    if dec.resident is not None:
        return L.mbx_process_batch_resident(codec, n, F, ptr(index), d_frames.data_ptr(), dec.state.data_ptr(), dec.resident.data_ptr(), dec.rng.data_ptr(), *outs)
    if index is not None:
        return L.mbx_process_batch_indexed(codec, n, F, index.data_ptr(), d_frames.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), *outs)
    return L.mbx_process_batch(codec, n, F, d_frames.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), *outs)


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("resident,indexed", [(True, False), (True, True), (False, False), (False, True)], ids=["resident", "resident-indexed", "abi", "abi-indexed"])
@pytest.mark.parametrize("codec,F", [(0, 1), (0, 9), (1, 3), (1, 1), (2, 3), (3, 1), (3, 3)])
def test_burst_launches_are_the_frames_calls_on_host_built_frames(mbx, oracle, codec, F, resident, indexed, soft):
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    pool, ticks = (300, 3) if F < 9 else (130, 2)
    n = (257 if F < 9 else 97) if indexed else pool
    rng = np.random.default_rng(1000 * codec + 10 * F + 2 * resident + indexed)
    s = B.random_schedule(codec, F, F * B.channel_bits(codec) + 211, rng, device=True)
    seeds = np.arange(pool) * 5 + 17
    a, b = (decoder.BatchDecoder(codec, pool, seeds=seeds, resident=resident) for _ in range(2))
    index = rng.permutation(pool)[:n].astype(np.int32) if indexed else None
    d_index = torch.from_numpy(index).cuda() if indexed else None
    T = ticks * F
    all_frames = soft_mix.frames(codec, n, T, tag=F) if soft else edge_mix.frames(codec, n, T, F).reshape(n * T, -1)
    all_frames = all_frames.reshape(n, ticks, F, *all_frames.shape[1:])
    built_all, got_all = [], []
    for t in range(ticks):
        frames = np.ascontiguousarray(all_frames[:, t]).reshape(n * F, *all_frames.shape[3:])
        stride = s.burst_bytes + t
        bursts = make_bursts(s, frames, rng, soft=soft, burst_stride=stride)
        built = B.apply_schedule(s, bursts, soft=soft, burst_stride=stride)
        if not soft and codec != 2:   # (codec 2: the two bits that pad the last byte come back as zero)
            assert np.array_equal(built, frames)
        out_a = a.decode_bursts(s, bursts, soft=soft, want_float=True, stream_index=d_index, burst_stride=stride)
        name_a = L.mbx_last_kernel_name(strm)
        out_b = b.make_outputs(F, want_float=True, streams=n)
        _native.check(_frames_call(L, b, codec, n, F, d_index, _dev(built), soft, out_b, strm), "frames call")
        name_b = L.mbx_last_kernel_name(strm)
        torch.cuda.synchronize()
        assert name_a == name_b and name_a, (name_a, name_b)
        for k in ("records", "results", "pcm16", "pcmf"):
            assert torch.equal(out_a[k], out_b[k]), f"tick {t}: {k}"
        assert torch.equal(a.state, b.state) and torch.equal(a.rng, b.rng), f"tick {t}: state, rng"
        if resident:
            assert torch.equal(a.resident, b.resident), f"tick {t}: elision words"
        else:   # the ABI triplets are whole after every launch
            assert a.resident is None
        built_all.append(built.reshape(n, F, *built.shape[1:]))
        got_all.append({k: v.cpu().numpy().reshape(n, F, -1) for k, v in out_a.items()})
    # every stream against the oracle, all ticks as one run of T frames
    rows = index if indexed else np.arange(pool)
    fr = np.concatenate(built_all, axis=1).reshape(n * T, *built_all[0].shape[2:])
    ref = oracle.process_batch(codec, n, T, fr, oracle.init_state(n), oracle.rng_seeded(seeds[rows]), soft=soft)
    got = {k: np.ascontiguousarray(np.concatenate([g[k] for g in got_all], axis=1)).reshape(n * T, -1) for k in got_all[0]}
    what = f"bursts codec {codec} F {F}"
    parity.check_exact(ref["records"], got["records"].view(RECORD_DTYPE).reshape(-1), what + ": records", T)
    with parity.located(T):
        parity.check_results(ref["results"], got["results"].view(RESULT_DTYPE).reshape(-1), what + ": results")
    parity.check_pcm_located(ref["pcmf"], got["pcmf"].reshape(-1, 160), ref["pcm16"], got["pcm16"].reshape(-1, 160), T, what=what + ": pcm", peak=ref["peak"])
    parity.check_state_blocks(ref["state"], a.state_numpy()[rows], what=what + ": state")
    parity.check_exact(ref["rng"], a.rng_numpy()[rows], what + ": rng")
    if indexed:   # slots outside the index were left alone
        rest = np.setdiff1d(np.arange(pool), index)
        fresh = decoder.BatchDecoder(codec, pool, seeds=seeds)
        assert np.array_equal(a.state_numpy()[rest], fresh.state_numpy()[rest]) and np.array_equal(a.rng_numpy()[rest], fresh.rng_numpy()[rest])
    s.close()


def test_burst_launch_edges(mbx):
    """S = 0, a reserved workspace, a schedule of another codec, a stride below the burst, pointers below their alignment"""
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder

    L = _native.lib()
    rng = np.random.default_rng(8)
    s = B.random_schedule(0, 9, 1728, rng, device=True)
    strm = torch.cuda.current_stream().cuda_stream
    dec = decoder.BatchDecoder(0, 64, resident=True)
    out = dec.make_outputs(9)
    args = lambda S, bursts, stride, rec: (s.handle, S, None, bursts, stride, dec.state.data_ptr(), dec.resident.data_ptr(), dec.rng.data_ptr(),   # noqa: E731
                                          out["pcm16"].data_ptr(), None, None, rec, strm)
    d = _dev(rng.integers(0, 256, size=(64, 216), dtype=np.uint8))
    assert L.mbx_process_bursts(*args(0, d.data_ptr(), 216, out["records"].data_ptr())) == 0
    assert L.mbx_process_bursts(*args(64, d.data_ptr(), 215, out["records"].data_ptr())) == -1 and b"burst_stride" in L.mbx_last_error()
    assert L.mbx_process_bursts(*args(64, d.data_ptr(), 216, out["records"].data_ptr() + 8)) == -1 and b"alignment" in L.mbx_last_error()
    assert L.mbx_deinterleave(s.handle, d.data_ptr(), 216, 64, out["records"].data_ptr(), 9, strm) == -1 and b"frame_stride" in L.mbx_last_error()
    assert L.mbx_deinterleave_soft(s.handle, d.data_ptr(), 1, out["records"].data_ptr(), 96, strm) == -1 and b"row_cells" in L.mbx_last_error()
    want = 64 * 9 + (64 * 9 * 18 + 255) // 256
    assert L.mbx_burst_workspace_frames(s.handle, 64, 0) == want and L.mbx_burst_workspace_frames(s.handle, 64, 1) == 64 * 9 + (64 * 9 * 368 + 255) // 256
    _native.check(L.mbx_reserve_stream(strm, want), "reserve")
    _native.check(L.mbx_process_bursts(*args(64, d.data_ptr(), 216, out["records"].data_ptr())), "bursts")
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        decoder.BatchDecoder(1, 64).decode_bursts(s, d)
    s.close()


# ---- several air interfaces, one mixed launch -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_two_schedules_gathered_into_one_row_array_feed_one_mixed_launch(mbx, soft):
    import torch
    from mbelib_neo_amd import bursts as B, decoder

    rng = np.random.default_rng(77)
    si = B.random_schedule(0, 9, 1728, rng, device=True)
    sa = B.random_schedule(1, 3, 264, rng, device=True)
    ni, na = 40, 55
    fi = soft_mix.frames(0, ni, 9, tag=9) if soft else edge_mix.frames(0, ni, 9, 9).reshape(ni * 9, -1)
    fa = soft_mix.frames(1, na, 3, tag=3) if soft else edge_mix.frames(1, na, 3, 3).reshape(na * 3, -1)
    bi, ba = make_bursts(si, fi, rng, soft=soft), make_bursts(sa, fa, rng, soft=soft)
    codec = np.array([0] * ni + [1] * na, dtype=np.uint8)
    counts = np.array([9] * ni + [3] * na)
    total = int(counts.sum())
    width = (184, 2) if soft else (18,)
    rows = torch.zeros((total, *width), dtype=torch.uint8, device="cuda")
    B.deinterleave(si, bi, soft=soft, mixed_rows=True, out=rows[:ni * 9])
    B.deinterleave(sa, ba, soft=soft, mixed_rows=True, out=rows[ni * 9:])
    host = [B.apply_schedule(si, bi, soft=soft).reshape(ni, -1)[i] for i in range(ni)] + [B.apply_schedule(sa, ba, soft=soft).reshape(na, -1)[i] for i in range(na)]
    host_rows = decoder.pack_mixed_rows(codec, counts, host, soft)
    assert np.array_equal(rows.cpu().numpy(), host_rows)
    seeds = np.arange(ni + na) + 31
    a, b = (decoder.BatchDecoder(0, ni + na, seeds=seeds, resident=True) for _ in range(2))
    out_a = a.decode_ragged(rows.reshape(-1), counts, soft=soft, want_float=True, codec=codec)
    out_b = b.decode_ragged(host_rows, counts, soft=soft, want_float=True, codec=codec)
    torch.cuda.synchronize()
    for k in ("records", "results", "pcm16", "pcmf"):
        assert torch.equal(out_a[k], out_b[k]), k
    assert torch.equal(a.state, b.state) and torch.equal(a.rng, b.rng) and torch.equal(a.resident, b.resident)


# ---- sessions -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec,F", [(0, 9), (1, 3), (2, 1)])
def test_session_burst_submits_return_the_bytes_of_the_frames_submits(mbx, codec, F):
    from mbelib_neo_amd import _native, bursts as B
    from mbelib_neo_amd.layout import RESULT_DTYPE

    L = _native.lib()
    S, n2 = 200, 77
    rng = np.random.default_rng(40 + codec)
    s = B.random_schedule(codec, F, F * B.channel_bits(codec) + 120, rng, device=True)
    other = B.random_schedule((codec + 1) % 4, F, 18 * 144, rng, device=True)
    seeds = (np.arange(S) * 3 + 5).astype(np.uint32)
    sess = [C.c_void_p(), C.c_void_p()]
    for h in sess:
        _native.check(L.mbx_session_create(C.byref(h), codec, S, S * F, 1 | 2 | 4), "create")
        _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
    a, b = sess
    try:
        def outputs(n):
            return np.zeros((n * F, 160), np.int16), np.zeros((n * F, 160), np.float32), np.zeros(n * F, RESULT_DTYPE)

        def same(x, y, what):
            for u, v, k in zip(x, y, ("pcm16", "pcmf", "results")):
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), f"{what}: {k}"

        pinned = L.mbx_host_alloc(S * (s.burst_bits * 2 + 64))
        assert pinned
        for step, (soft, indexed, pin) in enumerate([(False, False, False), (True, False, True), (False, True, True), (True, True, False), (False, False, True)]):
            n = n2 if indexed else S
            index = rng.permutation(S)[:n].astype(np.int32) if indexed else None
            frames = soft_mix.frames(codec, n, F, tag=step) if soft else edge_mix.frames(codec, n, F, step).reshape(n * F, -1)
            stride = s.burst_bytes + (step & 1)
            bursts = make_bursts(s, frames, rng, soft=soft, burst_stride=stride)
            built = B.apply_schedule(s, bursts, soft=soft, burst_stride=stride)
            src = bursts
            if pin:
                src = np.ctypeslib.as_array((C.c_uint8 * bursts.size).from_address(pinned))
                src[:] = bursts.reshape(-1)
            oa, ob = outputs(n), outputs(n)
            pa, pb = [x.ctypes.data for x in oa], [x.ctypes.data for x in ob]
            ip = index.ctypes.data if indexed else None
            if soft:
                bad = bursts.copy()
                bad[n // 2, 3, 0] = 2
                assert L.mbx_session_submit_bursts_soft(a, s.handle, n, ip, bad.ctypes.data, *pa) == -2   # MBE_STATUS_INVALID_BITS, nothing queued
                _native.check(L.mbx_session_submit_bursts_soft(a, s.handle, n, ip, src.ctypes.data, *pa), "bursts soft")
                if indexed:
                    _native.check(L.mbx_session_submit_soft_indexed(b, n, F, ip, built.ctypes.data, *pb, None), "soft indexed")
                else:
                    _native.check(L.mbx_session_submit_soft(b, F, built.ctypes.data, *pb), "soft")
            else:
                _native.check(L.mbx_session_submit_bursts(a, s.handle, n, ip, src.ctypes.data, stride, *pa), "bursts")
                if indexed:
                    _native.check(L.mbx_session_submit_indexed(b, n, F, ip, built.ctypes.data, *pb, None), "indexed")
                else:
                    _native.check(L.mbx_session_submit(b, F, built.ctypes.data, *pb), "frames")
            _native.check(L.mbx_session_wait(a), "wait")
            _native.check(L.mbx_session_wait(b), "wait")
            same(oa, ob, f"submit {step} (soft {soft}, indexed {indexed}, pinned {pin})")
        L.mbx_host_free(pinned)
        from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

        st = [np.zeros((S, 3), PARMS_DTYPE) for _ in sess]
        rg = [np.zeros(S, RNG_DTYPE) for _ in sess]
        for h, x, y in zip(sess, st, rg):
            _native.check(L.mbx_session_get_state(h, 0, S, x.ctypes.data, y.ctypes.data), "get_state")
        assert np.array_equal(st[0].view(np.uint8), st[1].view(np.uint8)) and np.array_equal(rg[0].view(np.uint8), rg[1].view(np.uint8))
        # refusals: nothing queued
        o = outputs(S)
        po = [x.ctypes.data for x in o]
        one = np.zeros(4096 * 4, dtype=np.uint8)
        assert L.mbx_session_submit_bursts(a, other.handle, S, None, one.ctypes.data, 512, *po) == -1 and b"codec" in L.mbx_last_error()
        assert L.mbx_session_submit_bursts(a, s.handle, S - 1, None, one.ctypes.data, s.burst_bytes, *po) == -1
        if F > 1:
            big = B.random_schedule(codec, F + 1, (F + 1) * 144 + 7, rng, device=True)
            assert L.mbx_session_submit_bursts(a, big.handle, S, None, one.ctypes.data, big.burst_bytes, *po) == -1 and b"max_frames_per_submit" in L.mbx_last_error()
        assert L.mbx_session_submit_bursts(a, s.handle, S, None, one.ctypes.data, s.burst_bytes - 1, *po) == -1
    finally:
        for h in sess:
            L.mbx_session_destroy(h)


# ---- the memory contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", burst_cases.CASES, ids=[c.id for c in burst_cases.CASES])
def test_burst_entry_points_between_guard_bands(mbx, case):
    case.fn(**case.args)
