"""GPU suite (-m gpu) for ragged batches: mbx_process_batch_ragged / _soft_ragged and BatchDecoder.decode_ragged.  Every stream is
compared with the CPU oracle run with that stream's OWN frame count, and every byte with the per-count launches
(mbx_process_batch_indexed / _resident / _soft_resident, one call per distinct count) a ragged launch replaces.  Inputs: the edge mix
and the soft mix, cut to the counts.  One test starts child processes (fresh ones, one at a time, each under a time limit)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import parity
import ragged_case
from ragged_case import ragged_frames

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
COUNTS = np.array([0, 1, 2, 3, 4, 5, 9, 17, 40])
S = 1003


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
    return {k: v.cpu().numpy() for k, v in out.items() if v is not None}


def _offsets(counts):
    return np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)


def _rows(counts, streams):
    """batch rows of the listed streams of a ragged batch, stream by stream"""
    off = _offsets(counts)
    return np.concatenate([np.arange(off[i], off[i + 1]) for i in streams]) if len(streams) else np.zeros(0, dtype=np.int64)


def _oracle_ragged(oracle, codec, counts, frames, state, rng, soft):
    """every stream with its own T: one oracle batch per distinct count; `state` / `rng` are the rows' own (already gathered)"""
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

    n = int(counts.sum())
    ref = {"pcm16": np.zeros((n, 160), np.int16), "pcmf": np.zeros((n, 160), np.float32), "results": np.zeros(n, RESULT_DTYPE),
           "records": np.zeros(n, RECORD_DTYPE), "peak": np.zeros(n, np.float32), "state": state.copy(), "rng": rng.copy()}
    for T in np.unique(counts[counts > 0]):
        who = np.flatnonzero(counts == T)
        rows = _rows(counts, who)
        r = oracle.process_batch(codec, len(who), int(T), frames[rows], state[who], rng[who], soft=soft)
        for k in ("pcm16", "pcmf", "results", "records", "peak"):
            ref[k][rows] = r[k]
        ref["state"][who] = r["state"]
        ref["rng"][who] = r["rng"]
    return ref


def _per_count_launches(dec, codec, counts, frames, slots, soft):
    """what a ragged launch replaces: one indexed launch per distinct count on the same kind of state, gathered into the ragged layout"""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    n = int(counts.sum())
    got = {"pcm16": np.zeros((n, 160), np.int16), "pcmf": np.zeros((n, 160), np.float32), "results": np.zeros((n, 5), np.int32),
           "records": np.zeros((n, 4), np.int32)}
    for T in np.unique(counts[counts > 0]):
        who = np.flatnonzero(counts == T)
        rows = _rows(counts, who)
        out = dec.make_outputs(int(T), want_float=True, streams=len(who))
        d_in = dec.to_device(frames[rows])
        d_index = torch.from_numpy(slots[who].astype(np.int32)).to(dec.device)
        tail = (dec.rng.data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(), strm)
        if soft or dec.resident is not None:
            fn = L.mbx_process_batch_soft_resident if soft else L.mbx_process_batch_resident
            rc = fn(codec, len(who), int(T), d_index.data_ptr(), d_in.data_ptr(), dec.state.data_ptr(),
                    dec.resident.data_ptr() if dec.resident is not None else None, *tail)
        else:
            rc = L.mbx_process_batch_indexed(codec, len(who), int(T), d_index.data_ptr(), d_in.data_ptr(), dec.state.data_ptr(), *tail)
        _native.check(rc, "per-count launch")
        torch.cuda.synchronize()
        for k in got:
            got[k][rows] = out[k].cpu().numpy()
    return got


def _same_bytes(what, a, b):
    for k in ("records", "results", "pcm16", "pcmf"):
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), f"{what}: {k} differ"


@pytest.mark.parametrize("indexed", [False, True], ids=["identity", "indexed"])
@pytest.mark.parametrize("resident", [False, True], ids=["abi", "resident"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_ragged_launches_equal_the_oracle_and_the_per_count_launches_on_every_stream(mbx, oracle, codec, soft, resident, indexed):
    """two launches on continuing state, different counts per launch (0 among them); the state of a stream without frames, its RNG
    state and its elision word keep their bytes"""
    import torch
    from mbelib_neo_amd import _native, decoder
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

    pool = 2 * S + 3 if indexed else S
    slots = (np.random.default_rng(codec + 11).permutation(pool)[:S] if indexed else np.arange(S)).astype(np.int32)
    seeds = np.arange(pool) * 3 + 17
    dec = decoder.BatchDecoder(codec, pool, seeds=seeds, resident=resident)
    twin = decoder.BatchDecoder(codec, pool, seeds=seeds, resident=resident)   # takes the per-count launches
    d_index = torch.from_numpy(slots).to(dec.device) if indexed else None
    state, rng = oracle.init_state(pool), oracle.rng_seeded(seeds)
    strm = torch.cuda.current_stream().cuda_stream
    want_name = ("imbe", "ambe", "imbe", "ambe2400")[codec] + "_stream_kernel_ragged" + ("_res" if resident else "")
    for launch in range(2):
        counts = COUNTS[np.random.default_rng(100 * codec + launch).integers(0, len(COUNTS), size=S)]
        frames = ragged_frames(codec, counts, tag=launch + 1, soft=soft)
        before = (dec.state.cpu().numpy().copy(), dec.rng.cpu().numpy().copy(), dec.resident.cpu().numpy().copy() if resident else None)
        out = dec.decode_ragged(frames, counts, soft=soft, want_float=True, stream_index=d_index)
        name = _native.lib().mbx_last_kernel_name(strm).decode()
        torch.cuda.synchronize()
        assert name == want_name, name
        assert np.array_equal(out["offsets"].cpu().numpy(), _offsets(counts))
        got = _numpy(out)
        # streams without frames: nothing of their slot was written (raw device bytes, before any materialisation)
        idle = slots[counts == 0]
        after_state = dec.state.cpu().numpy().reshape(pool, -1)
        after_rng = dec.rng.cpu().numpy().reshape(pool, -1)
        assert idle.size and np.array_equal(after_state[idle], before[0].reshape(pool, -1)[idle]), "state of a stream without frames"
        assert np.array_equal(after_rng[idle], before[1].reshape(pool, -1)[idle]), "RNG state of a stream without frames"
        if resident:
            assert np.array_equal(dec.resident.cpu().numpy()[idle], before[2][idle]), "elision word of a stream without frames"
        # the oracle, every stream with its own frame count
        ref = _oracle_ragged(oracle, codec, counts, frames, state[slots], rng[slots], soft)
        state[slots], rng[slots] = ref["state"], ref["rng"]
        what = f"codec {codec} launch {launch}"
        parity.check_exact(ref["records"], np.ascontiguousarray(got["records"]).view(RECORD_DTYPE).reshape(-1), what + ": records")
        parity.check_results(ref["results"], np.ascontiguousarray(got["results"]).view(RESULT_DTYPE).reshape(-1), what + ": results")
        parity.check_pcm(ref["pcmf"], got["pcmf"], ref["pcm16"], got["pcm16"], what=what + ": pcm", peak=ref["peak"])
        parity.check_state_blocks(state, dec.state_numpy(), what=what + ": state")
        parity.check_exact(rng, dec.rng_numpy(), what + ": rng")
        # the bytes of the launches it replaces
        _same_bytes(what, got, _per_count_launches(twin, codec, counts, frames, slots, soft))
        assert dec.state_numpy().tobytes() == twin.state_numpy().tobytes(), what + ": state bytes"
        assert dec.rng_numpy().tobytes() == twin.rng_numpy().tobytes(), what + ": rng bytes"


def test_a_batch_without_frames_launches_nothing(mbx):
    import torch
    from mbelib_neo_amd import _native, decoder

    L = _native.lib()
    side = torch.cuda.Stream()
    dec = decoder.BatchDecoder(1, 64, resident=True)
    state, rng = dec.state.cpu().numpy().copy(), dec.rng.cpu().numpy().copy()
    with torch.cuda.stream(side):
        out = dec.decode_ragged(np.zeros(0, np.uint8), np.zeros(64, np.int64), want_float=True)
        assert out["records"].shape[0] == 0 and out["offsets"].cpu().numpy().tolist() == [0] * 65
        assert L.mbx_last_kernel_name(side.cuda_stream) is None, "an all-zero batch launched a stream kernel"
        d_off = torch.zeros(1, dtype=torch.int32, device=dec.device)
        for fn in (L.mbx_process_batch_ragged, L.mbx_process_batch_soft_ragged):
            assert fn(1, 0, d_off.data_ptr(), 0, None, d_off.data_ptr(), dec.state.data_ptr(), None, dec.rng.data_ptr(), None, None, None,
                      out["records"].data_ptr(), side.cuda_stream) == 0
        assert L.mbx_last_kernel_name(side.cuda_stream) is None, "S == 0 launched a stream kernel"
        assert L.mbx_process_batch_ragged(1, 4, None, 8, None, d_off.data_ptr(), dec.state.data_ptr(), None, dec.rng.data_ptr(), None, None,
                                          None, out["records"].data_ptr(), side.cuda_stream) == -1
    torch.cuda.synchronize()
    assert np.array_equal(dec.state.cpu().numpy(), state) and np.array_equal(dec.rng.cpu().numpy(), rng)
    assert int(dec.resident.abs().sum()) == 0
    _native.check(L.mbx_release_stream(side.cuda_stream), "mbx_release_stream")


@pytest.mark.parametrize("codec", [1, 0])
def test_more_streams_than_wave_slots_skewed_counts_and_the_order_changes_no_byte(mbx, oracle, codec):
    """6,500 streams (more than the resident wave slots of either kernel: the order kernel runs), 97 % with 1..4 frames, 3 % with
    150: the bytes of the per-count launches on all streams, the oracle on every 16th, and the same digest from a fresh child
    process with MBX_RAGGED_ORDER=0"""
    from mbelib_neo_amd import decoder

    assert "MBX_RAGGED_ORDER" not in os.environ, "this test compares the default with MBX_RAGGED_ORDER=0"
    counts = ragged_case.skewed_counts()
    n = len(counts)
    assert n * 0 + int(counts.sum()) <= 330_000 and (counts == ragged_case.LONG).sum() == (3 * n) // 100
    out, dec, name = ragged_case.run_skewed(codec)
    assert name.endswith("_stream_kernel_ragged_res"), name
    got = _numpy(out)
    frames = ragged_frames(codec, counts, tag=4)
    seeds = np.arange(n) * 5 + 1
    twin = decoder.BatchDecoder(codec, n, seeds=seeds, resident=True)
    _same_bytes(f"codec {codec} skewed", got, _per_count_launches(twin, codec, counts, frames, np.arange(n, dtype=np.int32), False))
    assert dec.state_numpy().tobytes() == twin.state_numpy().tobytes() and dec.rng_numpy().tobytes() == twin.rng_numpy().tobytes()
    sample = np.arange(0, n, 16)
    ref = _oracle_ragged(oracle, codec, counts[sample], frames[_rows(counts, sample)], oracle.init_state(n)[sample],
                         oracle.rng_seeded(seeds)[sample], False)
    rows = _rows(counts, sample)
    from mbelib_neo_amd.layout import RESULT_DTYPE

    parity.check_results(ref["results"], np.ascontiguousarray(got["results"][rows]).view(RESULT_DTYPE).reshape(-1), "skewed: results")
    parity.check_pcm(ref["pcmf"], got["pcmf"][rows], ref["pcm16"], got["pcm16"][rows], what="skewed: pcm", peak=ref["peak"])
    parity.check_exact(ref["rng"], dec.rng_numpy()[sample], "skewed: rng")
    # grid order instead of longest first: a fresh process (the switch is read once), nothing else on the card meanwhile
    env = {k: v for k, v in os.environ.items() if not k.startswith("MBX_") or k in ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")}
    env["MBX_RAGGED_ORDER"] = "0"
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "ragged_case.py"), str(codec)], capture_output=True, text=True, timeout=600, env=env)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"ragged_case {codec}: the child process did not finish in {e.timeout} s -- nothing more is started on the card", returncode=3)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"ragged_case {codec}: the child process ended with status {r.returncode} -- nothing more is started on the card\n{tail}",
                    returncode=3)
    assert r.returncode == 0, tail
    assert r.stdout.strip().splitlines()[-1] == f"{name} {ragged_case.digest(out, dec)}", tail


def test_a_captured_ragged_step_replays_like_direct_calls(mbx):
    """one ragged step is a linear chain on the caller's stream (front, expand, order, stream kernel): captured once after
    mbx_reserve_stream(total + (S + 63) / 64) and replayed twice, it leaves what two direct calls leave"""
    import torch
    from mbelib_neo_amd import _native, decoder

    L = _native.lib()
    codec = 1
    counts = ragged_case.skewed_counts()
    n, total = len(counts), int(counts.sum())
    frames = ragged_frames(codec, counts, tag=6)
    seeds = np.arange(n) + 9
    eager = decoder.BatchDecoder(codec, n, seeds=seeds)
    want = []
    for _ in range(2):
        o = eager.decode_ragged(frames, counts, want_float=True)
        want.append((o["pcm16"].clone(), o["pcmf"].clone(), o["results"].clone()))
    torch.cuda.synchronize()
    dec = decoder.BatchDecoder(codec, n, seeds=seeds)
    d_frames = dec.to_device(frames)
    d_off = torch.from_numpy(_offsets(counts).astype(np.int32)).to(dec.device)
    out = dec.make_outputs(0, want_float=True, total=total)
    side = torch.cuda.Stream()
    args = (codec, n, d_off.data_ptr(), total, None, d_frames.data_ptr(), dec.state.data_ptr(), None, dec.rng.data_ptr(), out["pcm16"].data_ptr(),
            out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(), side.cuda_stream)
    _native.check(L.mbx_reserve_stream(side.cuda_stream, total + (n + 63) // 64), "mbx_reserve_stream")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = L.mbx_process_batch_ragged(*args)
    assert rc == 0, L.mbx_last_error()
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["pcm16"], want[k][0]) and torch.equal(out["pcmf"], want[k][1]) and torch.equal(out["results"], want[k][2]), k
    assert dec.state_numpy().tobytes() == eager.state_numpy().tobytes() and dec.rng_numpy().tobytes() == eager.rng_numpy().tobytes()
