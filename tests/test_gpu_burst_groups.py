"""GPU suite (-m gpu) for burst groups (include/mbx_burst_groups.h): the bursts of several schedules decoded in one call.  The call is
held byte for byte to the route over the existing calls (mbx_deinterleave[_soft] per group, host-made layout, one
mbx_process_batch[_soft]_mixed: tests/burst_group_cases.py), hard and soft, on resident and on ABI state; to itself with the groups in
another order; per codec to the CPU oracle under the bounds of tests/parity.py; to its buffers between guard bands; the session
submits to the device call; and one captured and replayed call to the eager one.  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import burst_group_cases as G
import parity

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _numpy(out):
    return {k: out[k].cpu().numpy() for k in G.KEYS}


def _kernel_name():
    import torch
    from mbelib_neo_amd import _native

    return (_native.lib().mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream) or b"").decode()


# ---- identity to the existing route, and the oracle ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [True, False], ids=["resident", "abi"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_a_groups_call_is_the_gathers_and_the_mixed_call_it_replaces(mbx, oracle, soft, resident):
    """four groups (165 streams, 405 frames) on 200 permuted slots, two ticks on continuing state"""
    import torch
    from mbelib_neo_amd import bursts as B, decoder
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

    shapes = G.SOFT if soft else G.HARD
    scheds = G.schedules(shapes, 5 + soft)
    seeds = np.arange(G.POOL) * 5 + 17
    a, b = (decoder.BatchDecoder(0, G.POOL, seeds=seeds, resident=resident) for _ in range(2))
    state, rng = oracle.init_state(G.POOL), oracle.rng_seeded(seeds)
    for tick in range(2):
        groups = G.make_groups(shapes, scheds, soft, 40 + tick, tag=3 * tick + 1, junk=tick == 1)
        rows = B.group_rows(groups)
        assert rows.tolist() == [0, 130, 340, 341, G.FRAMES]
        out = a.decode_burst_groups(G.on_device(groups), soft=soft, want_float=True)
        name = _kernel_name()
        torch.cuda.synchronize()
        assert name == "mixed_stream_kernel_ragged" + ("_res" if resident else ""), name
        want, want_name = G.existing_route(b, groups, soft)
        assert want_name == name
        got = _numpy(out)
        for k in G.KEYS:
            assert got[k].tobytes() == want[k].cpu().numpy().tobytes(), f"tick {tick}: {k}"
        assert G.pool_bytes(a) == G.pool_bytes(b), f"tick {tick}: state, RNG state or elision words"
        if not resident:
            assert a.resident is None
        if soft:
            continue
        # the hard case against the oracle, per group at its codec: every stream brings bursts_per_stream * F frames
        for g, first in zip(groups, rows[:-1]):
            s, slots = g.schedule, g.slots()
            T = g.bursts_per_stream * s.frames_per_burst
            frames = B.apply_schedule(s, g.bursts, burst_stride=g.burst_stride)
            ref = oracle.process_batch(s.codec, g.n_streams, T, frames, state[slots], rng[slots])
            state[slots], rng[slots] = ref["state"], ref["rng"]
            at = slice(int(first), int(first) + g.frames)
            what = f"tick {tick} codec {s.codec}"
            parity.check_exact(ref["records"], np.ascontiguousarray(got["records"][at]).view(RECORD_DTYPE).reshape(-1), what + ": records", T)
            with parity.located(T):
                parity.check_results(ref["results"], np.ascontiguousarray(got["results"][at]).view(RESULT_DTYPE).reshape(-1), what + ": results")
            parity.check_pcm_located(ref["pcmf"], got["pcmf"][at], ref["pcm16"], got["pcm16"][at], T, what=what + ": pcm", peak=ref["peak"])
        parity.check_state_blocks(state, a.state_numpy(), what=f"tick {tick}: state")
        parity.check_exact(rng, a.rng_numpy(), f"tick {tick}: rng")
        assert a.state_numpy().tobytes() == b.state_numpy().tobytes(), f"tick {tick}: state bytes"   # (both pools materialised alike)
    for s in scheds:
        s.close()


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_the_order_of_the_groups_changes_no_byte_of_a_stream(mbx, soft):
    """the same groups in another order, with an empty group among them and one group named by first_slot instead of an index"""
    import torch
    from mbelib_neo_amd import bursts as B, decoder

    shapes = G.SOFT if soft else G.HARD
    scheds = G.schedules(shapes, 9 + soft)
    groups = G.make_groups(shapes, scheds, soft, 50, tag=5)
    seeds = np.arange(G.POOL) * 3 + 1
    a, b = (decoder.BatchDecoder(0, G.POOL, seeds=seeds, resident=True) for _ in range(2))
    out_a = _numpy(a.decode_burst_groups(G.on_device(groups), soft=soft, want_float=True))
    rows_a = B.group_rows(groups)
    last = groups[3]
    by_slot = B.BurstGroup(last.schedule, last.bursts, last.n_streams, last.bursts_per_stream, stream_index=None, first_slot=int(last.slots()[0]),
                           burst_stride=last.burst_stride)
    assert np.array_equal(by_slot.slots(), last.slots())
    empty = B.BurstGroup(scheds[1], np.zeros(0, dtype=np.uint8), 0, 2, burst_stride=groups[1].burst_stride)
    order = [2, None, 3, 1, 0]
    other = [empty if i is None else (by_slot if i == 3 else groups[i]) for i in order]
    out_b = _numpy(b.decode_burst_groups(G.on_device(other), soft=soft, want_float=True))
    rows_b = B.group_rows(other)
    torch.cuda.synchronize()
    assert rows_b.tolist() == [0, 1, 1, 65, 275, G.FRAMES]
    for at, i in enumerate(order):
        if i is None:
            continue
        for k in G.KEYS:
            x = out_a[k][int(rows_a[i]):int(rows_a[i + 1])]
            y = out_b[k][int(rows_b[at]):int(rows_b[at + 1])]
            assert x.tobytes() == y.tobytes(), f"group {i}: {k}"
    assert G.pool_bytes(a) == G.pool_bytes(b)
    for s in scheds:
        s.close()


def test_empty_calls_launch_nothing_and_a_captured_call_replays_like_the_eager_one(mbx):
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder

    L = _native.lib()
    side = torch.cuda.Stream()
    scheds = G.schedules(G.HARD, 13)
    seeds = np.arange(G.POOL) + 9
    groups = G.on_device(G.make_groups(G.HARD, scheds, False, 60, tag=7))
    eager = decoder.BatchDecoder(0, G.POOL, seeds=seeds)
    want = []
    for _ in range(2):
        o = eager.decode_burst_groups(groups, want_float=True)
        want.append({k: o[k].clone() for k in G.KEYS})
    torch.cuda.synchronize()
    dec = decoder.BatchDecoder(0, G.POOL, seeds=seeds)
    out = dec.make_outputs(0, want_float=True, total=G.FRAMES)
    d_index = [torch.from_numpy(g.slots()).cuda() for g in groups]
    arr = B.group_structs(groups, [(g.bursts.data_ptr(), i.data_ptr()) for g, i in zip(groups, d_index)])
    tail = (dec.state.data_ptr(), None, dec.rng.data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(),
            out["records"].data_ptr(), side.cuda_stream)
    before = G.pool_bytes(dec)
    none = B.group_structs([B.BurstGroup(s, None, 0) for s in scheds], [(0, 0)] * 4)
    assert L.mbx_process_burst_groups(None, 0, 0, *tail) == 0                 # no group
    assert L.mbx_process_burst_groups(none, 4, 0, *tail) == 0                 # four groups without streams
    assert L.mbx_last_kernel_name(side.cuda_stream) is None, "an empty call launched a stream kernel"
    assert L.mbx_burst_groups_workspace_frames(none, 4, 0) == 0
    torch.cuda.synchronize()
    assert G.pool_bytes(dec) == before
    frames = L.mbx_burst_groups_workspace_frames(arr, 4, 0)
    # the mixed step's own rows, the gathered rows behind them and the layout words
    assert frames >= G.FRAMES + (G.STREAMS + 63) // 64 + 1 + (G.FRAMES * 18 + 9 * G.STREAMS + 4) // L.mbx_workspace_bytes(1)
    _native.check(L.mbx_reserve_stream(side.cuda_stream, frames), "mbx_reserve_stream")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = L.mbx_process_burst_groups(arr, 4, 0, *tail)
    assert rc == 0, L.mbx_last_error()
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        for key in G.KEYS:
            assert torch.equal(out[key], want[k][key]), (k, key)
    assert G.pool_bytes(dec) == G.pool_bytes(eager)
    _native.check(L.mbx_release_stream(side.cuda_stream), "mbx_release_stream")
    for s in scheds:
        s.close()


def test_refusals_that_need_a_schedule_name_the_call_and_launch_nothing(mbx):
    """an LLR schedule in a hard call, a stride below the burst, a group without bursts, more than 2^31-1 frames; and the rows call"""
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder

    L = _native.lib()
    side = torch.cuda.Stream()
    rng = np.random.default_rng(5)
    s = B.random_schedule(1, 3, 264, rng, device=True)
    llr = B.random_schedule(1, 3, 264, rng, device=True, form=B.FORM_LLR8)
    dec = decoder.BatchDecoder(0, 16)
    out = dec.make_outputs(0, total=16 * 6)
    d = torch.zeros(16 * 2 * 34, dtype=torch.uint8, device="cuda")
    tail = (dec.state.data_ptr(), None, dec.rng.data_ptr(), out["pcm16"].data_ptr(), None, None, out["records"].data_ptr(), side.cuda_stream)
    before = G.pool_bytes(dec)

    def refused(why, soft, *groups):
        arr = B.group_structs([g for g, _ in groups], [(p, 0) for _, p in groups])
        L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
        assert L.mbx_process_burst_groups(arr, len(groups), soft, *tail) == -1, why
        text = (L.mbx_last_error() or b"").decode()
        assert "mbx_process_burst_groups" in text and why in text, text
        assert L.mbx_burst_groups_workspace_frames(arr, len(groups), soft) == 0

    good = (B.BurstGroup(s, None, 16, 2, burst_stride=34), d.data_ptr())
    refused("LLR schedule", 0, good, (B.BurstGroup(llr, None, 4, 1, first_slot=16, burst_stride=300), d.data_ptr()))
    refused("burst_stride", 0, (B.BurstGroup(s, None, 16, 2, burst_stride=32), d.data_ptr()))
    refused("without bursts", 0, good, (B.BurstGroup(s, None, 1, 1, first_slot=16, burst_stride=34), 0))
    refused("2^31-1 frames", 0, (B.BurstGroup(s, None, 0x7FFFFFFF // 3 + 1, 1, burst_stride=34), d.data_ptr()))
    refused("2^31-1 frames", 1, (B.BurstGroup(s, None, 0x7FFFFFFF, 0x7FFFFFFF), d.data_ptr()))
    refused("2^31-1 frames", 0, good, (B.BurstGroup(s, None, 0x7FFFFFFF // 3 - 31, 1, first_slot=16, burst_stride=34), d.data_ptr()))
    assert L.mbx_last_kernel_name(side.cuda_stream) is None
    torch.cuda.synchronize()
    assert G.pool_bytes(dec) == before
    # the group boundaries, as the launcher places them
    rows = np.zeros(4, dtype=np.int32)
    arr = B.group_structs([good[0], B.BurstGroup(s, None, 0, 5), B.BurstGroup(llr, None, 7, 1)], [(0, 0)] * 3)
    assert L.mbx_burst_groups_rows(arr, 3, rows.ctypes.data) == 0 and rows.tolist() == [0, 96, 96, 117]
    arr = B.group_structs([B.BurstGroup(s, None, 0x7FFFFFFF // 3 + 1, 1)], [(0, 0)])
    assert L.mbx_burst_groups_rows(arr, 1, rows.ctypes.data) == -1 and b"2^31-1" in L.mbx_last_error()
    # 16 streams x 2 bursts x 3 frames: the good group alone decodes
    arr = B.group_structs([good[0]], [(good[1], 0)])
    _native.check(L.mbx_process_burst_groups(arr, 1, 0, *tail), "mbx_process_burst_groups")
    torch.cuda.synchronize()
    assert L.mbx_last_kernel_name(side.cuda_stream) == b"mixed_stream_kernel_ragged"
    s.close()
    llr.close()


# ---- the memory contract ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.GROUP_CASES, ids=[c.id for c in G.GROUP_CASES])
def test_a_groups_call_between_guard_bands(mbx, case):
    case.fn(**case.args)


# ---- sessions -------------------------------------------------------------------------------------------------------------------------
SESSION = 40
# one group per codec, ten streams each: (codec, F, form, sequence, streams, bursts per stream, extra stride)
SESSION_HARD = ((0, 2, 0, False, 10, 1, 0), (1, 3, 2, True, 10, 2, 1), (2, 1, 0, False, 10, 1, 0), (3, 1, 1, False, 10, 1, 0))
SESSION_SOFT = ((0, 2, 0, True, 10, 1, 0), (1, 3, 2, False, 10, 2, 0), (2, 1, 8, False, 10, 1, 0), (3, 1, 16, False, 10, 1, 0))
SESSION_FRAMES = 20 + 60 + 10 + 10


def _session_state(L, h, n):
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

    st, rg = np.zeros((n, 3), PARMS_DTYPE), np.zeros(n, RNG_DTYPE)
    _native.check(L.mbx_session_get_state(h, 0, n, st.ctypes.data, rg.ctypes.data), "get_state")
    return st, rg


def _outputs(n, fill=0x5A):
    from mbelib_neo_amd.layout import RESULT_DTYPE

    o = [np.zeros((n, 160), np.int16), np.zeros((n, 160), np.float32), np.zeros(n, RESULT_DTYPE)]
    for x in o:
        x.view(np.uint8).fill(fill)
    return o


def _device_call(groups, soft, state, rng):
    """mbx_process_burst_groups on a pool set from the session's state: (pcm16, pcmf, results, state, rng) as bytes"""
    import torch
    from mbelib_neo_amd import decoder

    dec = decoder.BatchDecoder(0, state.shape[0])
    dec.set_state(state, rng)
    out = dec.decode_burst_groups(G.on_device(groups), soft=soft, want_float=True)
    torch.cuda.synchronize()
    return [out[k].cpu().numpy().tobytes() for k in ("pcm16", "pcmf", "results")] + [dec.state_numpy().tobytes(), dec.rng_numpy().tobytes()]


def test_a_mixed_session_takes_burst_groups_from_pageable_and_pinned_memory(mbx):
    from mbelib_neo_amd import _native

    L = _native.lib()
    codec_of = np.repeat(np.arange(4, dtype=np.uint8), 10)[np.random.default_rng(2).permutation(SESSION)]
    slots = [np.flatnonzero(codec_of == g[0]).astype(np.int32) for g in SESSION_HARD]
    hard, soft_s = G.schedules(SESSION_HARD, 31), G.schedules(SESSION_SOFT, 32)
    h = C.c_void_p()
    _native.check(L.mbx_session_create_mixed(C.byref(h), SESSION, codec_of.ctypes.data, SESSION_FRAMES, 1 | 2 | 4), "create_mixed")
    seeds = (np.arange(SESSION) * 3 + 5).astype(np.uint32)
    _native.check(L.mbx_session_seed(h, 0, SESSION, seeds.ctypes.data), "seed")
    pinned = []
    try:
        for tick, (soft, pin) in enumerate([(False, False), (True, True), (False, True)]):
            shapes, scheds = (SESSION_SOFT, soft_s) if soft else (SESSION_HARD, hard)
            rng = np.random.default_rng(70 + tick)
            groups = G.make_groups(shapes, scheds, soft, 80 + tick, tag=tick + 1, slots=[rng.permutation(s) for s in slots])
            if tick == 2:
                groups = groups[::-1]
            arr, keep = G.group_array(L, groups)
            if pin:   # the bursts of every group in pinned memory, 16-byte aligned and not
                for i, g in enumerate(groups):
                    p = L.mbx_host_alloc(g.bursts.size + 16)
                    assert p
                    pinned.append(p)
                    at = p + (0 if i & 1 else 16)
                    C.memmove(at, g.bursts.ctypes.data, g.bursts.size)
                    arr[i].bursts = at
            before = _session_state(L, h, SESSION)
            want = _device_call(groups, soft, *before)
            o = _outputs(SESSION_FRAMES)
            _native.check(L.mbx_session_submit_burst_groups(h, arr, 4, int(soft), *[x.ctypes.data for x in o]), "submit_burst_groups")
            _native.check(L.mbx_session_wait(h), "wait")
            after = _session_state(L, h, SESSION)
            got = [x.tobytes() for x in o] + [after[0].tobytes(), after[1].tobytes()]
            for k, x, y in zip(("pcm16", "pcmf", "results", "state", "rng"), got, want):
                assert x == y, f"tick {tick} (soft {soft}, pinned {pin}): {k}"
        # refusals: nothing is queued, outputs and state keep their bytes
        groups = G.make_groups(SESSION_HARD, hard, False, 90, tag=9, slots=slots)
        before = _session_state(L, h, SESSION)

        def refused(code, why, groups, n=4):
            arr, keep = G.group_array(L, groups)
            o = _outputs(SESSION_FRAMES)
            L.mbx_stage_in(0x1008, 0x1000, 16, None)   # another call's text first
            assert L.mbx_session_submit_burst_groups(h, arr, n, 0, *[x.ctypes.data for x in o]) == code, why
            text = (L.mbx_last_error() or b"").decode()
            assert code == -2 or ("mbx_session_submit_burst_groups" in text and why in text), text
            assert all((x.view(np.uint8) == 0x5A).all() for x in o), why
            after = _session_state(L, h, SESSION)
            assert after[0].tobytes() == before[0].tobytes() and after[1].tobytes() == before[1].tobytes(), why

        from mbelib_neo_amd import bursts as B

        wrong = list(groups)
        wrong[0] = B.BurstGroup(groups[0].schedule, groups[0].bursts, 10, 1, stream_index=slots[2], burst_stride=groups[0].burst_stride)
        refused(-1, "codec", [wrong[0], groups[1], groups[3]], 3)               # a schedule of codec 0 on the streams of codec 2
        twice = list(groups)
        idx = slots[1].copy()
        twice[1] = B.BurstGroup(groups[1].schedule, groups[1].bursts, 10, 2, stream_index=idx, burst_stride=groups[1].burst_stride)
        half = B.BurstGroup(groups[1].schedule, groups[1].bursts, 1, 2, stream_index=idx[4:5], burst_stride=groups[1].burst_stride)
        refused(-1, "listed twice", [groups[0], twice[1], half], 3)              # one slot in two groups
        bad = groups[3].bursts.copy()
        bad[5 * groups[3].burst_stride + 7] = 2                                  # a BITS byte above 1
        refused(-2, "bits", groups[:3] + [B.BurstGroup(groups[3].schedule, bad, 10, 1, stream_index=slots[3], burst_stride=groups[3].burst_stride)])
        # the frames submits are not a mixed session's
        o = _outputs(SESSION)
        frames = np.zeros(SESSION * 18, dtype=np.uint8)
        assert L.mbx_session_submit(h, 1, frames.ctypes.data, *[x.ctypes.data for x in o]) == -1
        assert b"mixed session" in L.mbx_last_error()
        assert L.mbx_session_submit_bursts(h, hard[0].handle, SESSION, None, frames.ctypes.data, hard[0].burst_bytes, *[x.ctypes.data for x in o]) == -1
        assert b"mixed session" in L.mbx_last_error()
    finally:
        L.mbx_session_destroy(h)
        for p in pinned:
            L.mbx_host_free(p)
        for s in hard + soft_s:
            s.close()


def test_a_single_codec_session_takes_groups_of_its_codec(mbx):
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    S = 24
    shapes = ((1, 3, 2, True, 7, 2, 0), (1, 1, 0, False, 9, 1, 2))   # two schedules of ONE codec: 7 streams x 2 bursts of 3 frames, 9 x 1 of 1
    total = 7 * 2 * 3 + 9
    scheds = G.schedules(shapes, 41)
    other = G.schedules(((3, 1, 0, False, 1, 1, 0),), 42)[0]
    h = C.c_void_p()
    _native.check(L.mbx_session_create(C.byref(h), 1, S, total, 1 | 2 | 4), "create")
    try:
        perm = np.random.default_rng(4).permutation(S).astype(np.int32)
        groups = G.make_groups(shapes, scheds, False, 43, tag=4, slots=[perm[:7], perm[7:16]])
        before = _session_state(L, h, S)
        want = _device_call(groups, False, *before)
        arr, keep = G.group_array(L, groups)
        o = _outputs(total)
        _native.check(L.mbx_session_submit_burst_groups(h, arr, 2, 0, *[x.ctypes.data for x in o]), "submit_burst_groups")
        _native.check(L.mbx_session_wait(h), "wait")
        after = _session_state(L, h, S)
        got = [x.tobytes() for x in o] + [after[0].tobytes(), after[1].tobytes()]
        for k, x, y in zip(("pcm16", "pcmf", "results", "state", "rng"), got, want):
            assert x == y, k
        # a schedule of another codec, and more frames than max_frames_per_submit
        stranger = B.BurstGroup(other, np.zeros(other.burst_bytes, dtype=np.uint8), 1, 1, stream_index=perm[20:21])
        arr, keep = G.group_array(L, [stranger])
        assert L.mbx_session_submit_burst_groups(h, arr, 1, 0, *[x.ctypes.data for x in o]) == -1 and b"codec" in L.mbx_last_error()
        more = B.BurstGroup(scheds[1], np.zeros(8 * groups[1].burst_stride, dtype=np.uint8), 8, 1, stream_index=perm[16:24], burst_stride=groups[1].burst_stride)
        arr, keep = G.group_array(L, groups + [more])
        assert L.mbx_session_submit_burst_groups(h, arr, 3, 0, *[x.ctypes.data for x in o]) == -1 and b"max_frames_per_submit" in L.mbx_last_error()
        # the frames submits go on working on it
        frames = np.zeros(S * 9, dtype=np.uint8)
        o = _outputs(S)
        _native.check(L.mbx_session_submit(h, 1, frames.ctypes.data, *[x.ctypes.data for x in o]), "submit")
        _native.check(L.mbx_session_wait(h), "wait")
    finally:
        L.mbx_session_destroy(h)
        for s in scheds + [other]:
            s.close()
