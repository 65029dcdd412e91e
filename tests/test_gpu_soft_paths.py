"""GPU suite (-m gpu) for soft-decision frames on the batched paths: mbx_process_batch_soft and its resident / indexed /
caller-workspace forms, soft submits of sessions, and soft calls in queue mode.  Every comparison is with the
CPU oracle (soft=True) on ALL streams: records, results and RNG state byte for byte, PCM under the int16 bound, state block by
block.  Inputs: tests/soft_mix.py.  Nothing here starts a child process."""
import numpy as np
import pytest

import golden_io
import oracle_lib
import parity
import shim_lib
import soft_mix
from shim_lib import p

pytestmark = pytest.mark.gpu
CELLS = soft_mix.CELLS
NBITS = {0: 88, 1: 49, 2: 88, 3: 49}


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


@pytest.fixture(scope="module")
def mbe(mbx):
    return shim_lib.load()


def _compare(what, ref, got, state, rng, T):
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

    parity.check_exact(ref["records"], np.ascontiguousarray(got["records"]).view(RECORD_DTYPE).reshape(-1), what + ": records", T)
    with parity.located(T):
        parity.check_results(ref["results"], np.ascontiguousarray(got["results"]).view(RESULT_DTYPE).reshape(-1), what + ": results")
    m = parity.check_pcm_located(ref["pcmf"], got["pcmf"].reshape(-1, 160), ref["pcm16"], got["pcm16"].reshape(-1, 160), T,
                                 what=what + ": pcm", peak=ref["peak"])
    parity.check_state_blocks(ref["state"], state, what=what + ": state")
    parity.check_exact(ref["rng"], rng, what + ": rng")
    return m


def _numpy(out):
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


# ---- mbx_process_batch_soft ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
@pytest.mark.parametrize("S,T", [(257, 1), (257, 3), (257, 17), (4096, 1)])
def test_soft_batch_equals_the_oracle_on_every_stream(mbx, oracle, codec, S, T):
    import torch
    from mbelib_neo_amd import _native, decoder

    soft = soft_mix.frames(codec, S, T, tag=T)
    seeds = np.arange(S) * 7 + 3
    dec = decoder.BatchDecoder(codec, S, seeds=seeds)
    out = dec.make_outputs(T, want_float=True)
    d_soft = dec.to_device(soft)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    _native.check(L.mbx_process_batch_soft(codec, S, T, d_soft.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(),
                                           out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(), strm), "soft")
    name = L.mbx_last_kernel_name(strm).decode()
    torch.cuda.synchronize()
    assert "stream_kernel" in name, f"mbx_last_kernel_name reports the stream-stage instance, not {name}"
    ref = oracle.process_batch(codec, S, T, soft, oracle.init_state(S), oracle.rng_seeded(seeds), soft=True)
    print(codec, S, T, name, _compare(f"soft batch codec {codec} {S}x{T}", ref, _numpy(out), dec.state_numpy(), dec.rng_numpy(), T))


def test_soft_batch_reproduces_the_reference_fixtures(mbx):
    """soft_kat.bin: the FEC records of the reference's own soft frames, and its 12-frame soft stream (results exact, PCM)"""
    import torch
    from mbelib_neo_amd import _native, decoder

    kat = golden_io.soft_kat()
    L = _native.lib()
    for codec, key, nbits in ((0, "imbe", 88), (1, "ambe", 49)):
        rows = kat[key]
        n = len(rows)
        dec = decoder.BatchDecoder(codec, n)
        out = dec.make_outputs(1, want_float=True)
        d_soft = dec.to_device(np.ascontiguousarray(rows["soft"]))
        _native.check(L.mbx_process_batch_soft(codec, n, 1, d_soft.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(),
                                               out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(),
                                               torch.cuda.current_stream().cuda_stream), "soft")
        torch.cuda.synchronize()
        rec = decoder.records_numpy(out["records"])
        assert np.array_equal(oracle_lib.records_to_bits(rec, nbits), rows["bits"]), key
    proc = kat["process"]
    T = len(proc)
    dec = decoder.BatchDecoder(0, 1, seeds=[4242])
    out = dec.decode_soft(np.ascontiguousarray(proc["soft"]), T, want_float=True)
    torch.cuda.synchronize()
    res = decoder.results_numpy(out["results"])
    for name in ("c0_errors", "protected_errors", "c4_errors", "total_errors", "flags"):
        assert np.array_equal(res[name], proc["result"][name]), name
    parity.check_pcm(proc["pcmf"], out["pcmf"].cpu().numpy())


# ---- resident state, an index into a larger pool --------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_soft_resident_indexed_launches_carry_state_and_equal_plain_triplets(mbx, oracle, codec):
    """a pool of 2 S slots, an index that permutes the batch over it (another permutation every launch), five launches with the
    elision words carried between them -- T = 1, 1, 3, 1, 17 -- then mbx_resident_materialize; the same frames through
    mbx_process_batch_soft on plain triplets give identical bytes"""
    import torch
    from mbelib_neo_amd import decoder

    S, plan = 300, (1, 1, 3, 1, 17)
    Tt = sum(plan)
    soft = soft_mix.frames(codec, S, Tt, tag=77).reshape(S, Tt, CELLS[codec], 2)
    seeds = np.arange(S) * 5 + 1
    pool = 2 * S
    slots = np.arange(pool - 1, 0, -2)[:S].copy()   # stream s lives in slot slots[s]
    pool_seeds = np.full(pool, 999, dtype=np.int64)
    pool_seeds[slots] = seeds
    res = decoder.BatchDecoder(codec, pool, seeds=pool_seeds, resident=True)
    untouched = res.state_numpy().copy()
    plain = decoder.BatchDecoder(codec, S, seeds=seeds)
    perm_rng = np.random.default_rng(5)
    got = {k: [] for k in ("records", "results", "pcm16", "pcmf")}
    t0 = 0
    for T in plan:
        part = np.ascontiguousarray(soft[:, t0:t0 + T])
        order = perm_rng.permutation(S)      # batch row i = stream order[i]
        d_index = torch.from_numpy(slots[order].astype(np.int32)).cuda()
        out = _numpy(res.decode_soft(np.ascontiguousarray(part[order]), T, want_float=True, stream_index=d_index))
        ref_out = _numpy(plain.decode_soft(part, T, want_float=True))
        torch.cuda.synchronize()
        inv = np.argsort(order)
        for k in got:
            rows = out[k].reshape(S, T, -1)[inv]
            assert rows.tobytes() == ref_out[k].reshape(S, T, -1).tobytes(), f"{k}: resident + index differs from plain triplets at tick {t0}"
            got[k].append(rows)
        t0 += T
    got = {k: np.concatenate(v, axis=1) for k, v in got.items()}
    state, rng = res.state_numpy(), res.rng_numpy()   # (materialises)
    assert state[slots].tobytes() == plain.state_numpy().tobytes() and rng[slots].tobytes() == plain.rng_numpy().tobytes()
    rest = np.setdiff1d(np.arange(pool), slots)
    assert state[rest].tobytes() == untouched[rest].tobytes(), "a slot outside the index changed"
    ref = oracle.process_batch(codec, S, Tt, soft.reshape(S * Tt, -1, 2), oracle.init_state(S), oracle.rng_seeded(seeds), soft=True)
    print(codec, _compare(f"soft resident codec {codec}", ref, got, state[slots], rng[slots], Tt))


@pytest.mark.parametrize("codec", [0, 1])
def test_soft_ws_form_is_captured_into_a_graph_and_replayed(mbx, oracle, codec):
    import torch
    from mbelib_neo_amd import _native, decoder

    S, T = 1024, 1
    soft = soft_mix.frames(codec, S, 2, tag=9).reshape(S, 2, CELLS[codec], 2)
    seeds = np.arange(S) + 40
    dec = decoder.BatchDecoder(codec, S, seeds=seeds)
    out = dec.make_outputs(T, want_float=True)
    L = _native.lib()
    ws = torch.empty(int(L.mbx_workspace_bytes(S * T)), dtype=torch.uint8, device="cuda")
    d_soft = dec.to_device(np.ascontiguousarray(soft[:, 0]))
    assert L.mbx_process_batch_soft_ws(codec, S, T, d_soft.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), None, None, None,
                                       out["records"].data_ptr(), None, 0, None) == -1, "a missing workspace is an argument error"
    graph = torch.cuda.CUDAGraph()
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        with torch.cuda.graph(graph, stream=side):
            _native.check(L.mbx_process_batch_soft_ws(codec, S, T, d_soft.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(),
                                                      out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(),
                                                      out["records"].data_ptr(), ws.data_ptr(), ws.numel(), side.cuda_stream), "soft_ws")
    torch.cuda.synchronize()
    got = {k: [] for k in ("records", "results", "pcm16", "pcmf")}
    for t in range(2):   # the first launch of the graph, then one replay on the next tick's frames
        d_soft.copy_(torch.from_numpy(np.ascontiguousarray(soft[:, t]).reshape(-1)))
        graph.replay()
        torch.cuda.synchronize()
        for k in got:
            got[k].append(out[k].cpu().numpy().reshape(S, 1, -1))
    got = {k: np.concatenate(v, axis=1) for k, v in got.items()}
    ref = oracle.process_batch(codec, S, 2, soft.reshape(S * 2, -1, 2), oracle.init_state(S), oracle.rng_seeded(seeds), soft=True)
    _compare(f"soft ws graph codec {codec}", ref, got, dec.state_numpy(), dec.rng_numpy(), 2)


# ---- sessions -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1])
def test_session_takes_hard_and_soft_submits_in_any_order(mbx, oracle, codec):
    """1,024 streams, 20 ticks of T = 1 alternating hard and soft submits, then one T = 8 indexed soft submit on a subset: the oracle
    is fed the same sequence, state carried from call to call"""
    import ctypes as C

    import edge_mix
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import FRAME_BYTES, PARMS_DTYPE, RECORD_DTYPE, RESULT_DTYPE, RNG_DTYPE

    S, ticks, T2 = 1024, 20, 8
    L = _native.lib()
    hard = edge_mix.frames(codec, S, ticks, tag=31)                                   # [S, ticks, bytes]
    soft = soft_mix.frames(codec, S, ticks, tag=32).reshape(S, ticks, CELLS[codec], 2)
    subset = np.arange(S - 1, 0, -3).astype(np.int32)
    n2 = len(subset)
    soft2 = soft_mix.frames(codec, n2, T2, tag=33)
    seeds = (np.arange(S) + 900).astype(np.uint32)
    sess = C.c_void_p()
    _native.check(L.mbx_session_create(C.byref(sess), codec, S, S * T2, 1 | 2 | 4), "create")
    try:
        _native.check(L.mbx_session_seed(sess, 0, S, seeds.ctypes.data), "seed")
        bad = np.ascontiguousarray(soft[:, 0]).copy()
        bad[S // 2, 5, 0] = 2
        assert L.mbx_session_submit_soft(sess, 1, bad.ctypes.data, None, None, None) == -2   # MBE_STATUS_INVALID_BITS, nothing queued
        assert L.mbx_session_submit_soft(sess, T2 + 1, soft.ctypes.data, None, None, None) == -1   # over max_frames_per_submit
        st, rg = oracle.init_state(S), oracle.rng_seeded(seeds)
        keep = []
        for t in range(ticks):
            is_soft = t % 2 == 1
            frames = np.ascontiguousarray(soft[:, t] if is_soft else hard[:, t])
            pcm16, pcmf = np.zeros((S, 160), np.int16), np.zeros((S, 160), np.float32)
            res = np.zeros(S, RESULT_DTYPE)
            fn = L.mbx_session_submit_soft if is_soft else L.mbx_session_submit
            _native.check(fn(sess, 1, frames.ctypes.data, pcm16.ctypes.data, pcmf.ctypes.data, res.ctypes.data), f"submit {t}")
            keep.append((frames, pcm16, pcmf, res))
        _native.check(L.mbx_session_wait(sess), "wait")
        for t, (frames, pcm16, pcmf, res) in enumerate(keep):
            ref = oracle.process_batch(codec, S, 1, frames.reshape(S, -1, 2) if t % 2 else frames.reshape(S, FRAME_BYTES[codec]), st, rg, soft=t % 2 == 1)
            st, rg = ref["state"], ref["rng"]
            with parity.located(1):
                parity.check_results(ref["results"], res, f"session tick {t}: results")
            parity.check_pcm_located(ref["pcmf"], pcmf, ref["pcm16"], pcm16, 1, what=f"session tick {t}: pcm", peak=ref["peak"])
        pcm16, pcmf = np.zeros((n2 * T2, 160), np.int16), np.zeros((n2 * T2, 160), np.float32)
        res, rec = np.zeros(n2 * T2, RESULT_DTYPE), np.zeros(n2 * T2, RECORD_DTYPE)
        _native.check(L.mbx_session_submit_soft_indexed(sess, n2, T2, subset.ctypes.data, soft2.ctypes.data, pcm16.ctypes.data, pcmf.ctypes.data,
                                                        res.ctypes.data, rec.ctypes.data), "submit indexed")
        state, rng = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
        _native.check(L.mbx_session_get_state(sess, 0, S, state.ctypes.data, rng.ctypes.data), "get_state")
        ref = oracle.process_batch(codec, n2, T2, soft2, st[subset], rg[subset], soft=True)
        _compare("session indexed soft submit", ref, {"records": rec, "results": res, "pcm16": pcm16, "pcmf": pcmf}, state[subset],
                 rng[subset], T2)
        rest = np.setdiff1d(np.arange(S), subset)
        parity.check_state_blocks(st[rest], state[rest], what="session: streams outside the index")
        parity.check_exact(rg[rest], rng[rest], "session: rng outside the index")
    finally:
        L.mbx_session_destroy(sess)


# ---- queue mode of the per-frame library ---------------------------------------------------------------------------------------
SOFT_CALLS = {0: "mbe_processImbe7200x4400SoftFrame", 1: "mbe_processAmbe3600x2450SoftFrame", 2: "mbe_processImbe7100x4400SoftFrame",
              3: "mbe_processAmbe3600x2400SoftFrame"}
HARD_CALLS = {0: "mbe_processImbe7200x4400Framef", 1: "mbe_processAmbe3600x2450Framef"}
MBE_BATCH_QUEUE_SOFT = 0x10
FILL = 0x5A


def _new_state(mbe):
    from mbelib_neo_amd.layout import PARMS_DTYPE

    st = [np.zeros(1, dtype=PARMS_DTYPE) for _ in range(3)]
    mbe.mbe_initMbeParms(p(st[0]), p(st[1]), p(st[2]))
    return st


class _Channel:
    """one channel's frames and output buffers; codec = c % 4, the short call where (c // 4) % 2: all eight entry points in turn"""

    def __init__(self, mbe, c, codec, soft):
        from mbelib_neo_amd.layout import RESULT_DTYPE

        self.c, self.codec, self.soft, self.T, self.t = c, codec, soft, len(soft), 0
        short = (c // 4) % 2 == 1
        self.fn = getattr(mbe, SOFT_CALLS[codec] + ("" if short else "f"))
        self.pcm = np.full((self.T, 160), 0, dtype=np.int16 if short else np.float32)
        self.pcm.view(np.uint8)[...] = FILL
        self.res = np.zeros(self.T, dtype=RESULT_DTYPE)
        self.res.view(np.uint8)[...] = FILL
        self.bits = np.full((self.T, NBITS[codec]), FILL, dtype=np.int8)
        self.st = _new_state(mbe)
        self.rets = []

    def call(self, mbe):
        t = self.t
        if t == 0:
            mbe.mbe_setThreadRngSeed(7000 + self.c)
        self.rets.append(self.fn(p(self.pcm[t]), p(self.res[t:t + 1]), p(self.soft[t]), p(self.bits[t]), p(self.st[0]), p(self.st[1]), p(self.st[2])))
        self.t += 1

    def outputs(self):
        return self.pcm.tobytes(), self.res.tobytes(), self.bits.tobytes(), np.concatenate(self.st).tobytes()


def _channels(mbe, n=64, T=12):
    return [_Channel(mbe, c, c % 4, soft_mix.frames(c % 4, 1, T, tag=200 + c)) for c in range(n)]


@pytest.mark.parametrize("mode", [0, 1])
def test_queue_mode_with_the_flag_queues_soft_calls_and_equals_the_synchronous_calls(mbe, mode):
    """64 channels, four codecs mixed, ragged counts (0..5 frames per channel and flush): nothing is written before mbe_flush(), and
    after it every output and the final structs are byte for byte what the same calls return synchronously"""
    want = _channels(mbe)
    for ch in want:   # synchronous: each channel alone, so that it owns the thread's RNG state like a queued channel owns its copy
        while ch.t < ch.T:
            ch.call(mbe)
        assert all(r >= 0 for r in ch.rets)
    got = _channels(mbe)
    counts = np.random.default_rng(11).integers(0, 6, size=(16, len(got)))
    assert mbe.mbe_batchBegin(mode | MBE_BATCH_QUEUE_SOFT) == 0
    try:
        for row in counts:
            made, touched = 0, []
            for ch, k in zip(got, row):
                first = ch.t
                for _ in range(min(int(k), ch.T - ch.t)):
                    ch.call(mbe)
                    made += 1
                touched.append((ch, first, ch.t))
            assert mbe.mbe_batchPending() == made, "a soft call in queue mode with the flag must queue"
            for ch, a, b in touched:
                for arr in (ch.pcm, ch.res, ch.bits):
                    assert (arr[a:b].view(np.uint8) == FILL).all(), "an output was written before mbe_flush()"
            assert mbe.mbe_flush() == made and mbe.mbe_batchPending() == 0
        # an invalid hard decision: refused at once, nothing queued
        ch = got[0]
        bad = ch.soft[0].copy()
        bad[3, 0] = 2
        out, bits = np.zeros(160, np.float32), np.zeros(88, np.int8)
        assert ch.fn(p(out), None, p(bad), p(bits), p(ch.st[0]), p(ch.st[1]), p(ch.st[2])) == -2 and mbe.mbe_batchPending() == 0
        for ch in got:   # whatever the ragged plan left
            while ch.t < ch.T:
                ch.call(mbe)
    finally:
        assert mbe.mbe_batchEnd() >= 0
    for a, b in zip(want, got):
        assert all(r == 0 for r in b.rets)
        for name, x, y in zip(("pcm", "result", "bits", "state"), a.outputs(), b.outputs()):
            assert x == y, f"channel {a.c} (codec {a.codec}): {name} differs from the synchronous calls"


def test_queue_mode_channel_switches_hard_soft_direct_inside_one_batch(mbe):
    """one channel and flush: two hard frames, two soft frames (the change of input form runs what is queued), then a direct
    mbe_process*Data call (flushes and releases the channel), then soft again -- PCM, bits, results and the final structs equal the
    synchronous sequence.  (The thread's RNG is seeded again before and after the direct call in both legs: a queued channel works
    on its own copy of it, taken at its first queued frame.)"""
    import edge_mix
    from mbelib_neo_amd.layout import RESULT_DTYPE

    for codec in (0, 1):
        nb = NBITS[codec]
        hard = edge_mix.frames(codec, 1, 8, tag=5)[0]
        cells, _ = soft_mix.cells_from_packed(codec, hard)
        cells = cells.astype(np.int8)
        soft = soft_mix.frames(codec, 1, 8, tag=6)
        hard_fn, soft_fn = getattr(mbe, HARD_CALLS[codec]), getattr(mbe, SOFT_CALLS[codec] + "f")
        decode = mbe.mbe_decodeImbe7200x4400Frame if codec == 0 else mbe.mbe_decodeAmbe3600x2450Frame
        data = mbe.mbe_processImbe4400Dataf if codec == 0 else mbe.mbe_processAmbe2450Dataf

        def run(queued):
            st = _new_state(mbe)
            pcm, bits, res = np.zeros((8, 160), np.float32), np.zeros((8, nb), np.int8), np.zeros(8, RESULT_DTYPE)
            mbe.mbe_setThreadRngSeed(4321)
            if queued:
                assert mbe.mbe_batchBegin(1 | MBE_BATCH_QUEUE_SOFT) == 0
            for t in range(8):
                args = (p(bits[t]), p(st[0]), p(st[1]), p(st[2]))
                if t in (0, 1):
                    rc = hard_fn(p(pcm[t]), p(res[t:t + 1]), p(cells[t]), *args)
                elif t == 4:
                    mbe.mbe_setThreadRngSeed(555)
                    assert decode(p(cells[t]), p(bits[t]), p(res[t:t + 1])) >= 0
                    rc = 0 if data(p(pcm[t]), p(res[t:t + 1]), *args) >= 0 else -1
                    mbe.mbe_setThreadRngSeed(556)
                else:
                    rc = soft_fn(p(pcm[t]), p(res[t:t + 1]), p(soft[t]), *args)
                assert rc >= 0
                if queued and t == 2:
                    assert mbe.mbe_batchPending() == 1, "the two hard frames ran when the input form changed"
            if queued:
                assert mbe.mbe_batchEnd() >= 0
            return pcm, bits, res, np.concatenate(st)

        want, got = run(False), run(True)
        for name, x, y in zip(("pcm", "bits", "results", "state"), want, got):
            assert x.tobytes() == y.tobytes(), f"codec {codec}: {name} differs from the synchronous sequence"


def test_queue_mode_without_the_flag_runs_soft_calls_at_once(mbe):
    chans = _channels(mbe, n=4, T=2)
    assert mbe.mbe_batchBegin(1) == 0
    try:
        for ch in chans:
            ch.call(mbe)
            assert mbe.mbe_batchPending() == 0
            assert ch.rets[-1] >= 0 and not (ch.pcm[0].view(np.uint8) == FILL).all()
    finally:
        assert mbe.mbe_batchEnd() >= 0
