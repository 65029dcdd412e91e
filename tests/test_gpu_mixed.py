"""GPU suite (-m gpu) for mixed-codec ragged batches: mbx_process_batch_mixed / _soft_mixed, BatchDecoder.decode_ragged(codec=array) and
the queue mode of the per-frame library on top of them.  Every stream is compared with the CPU oracle at its OWN codec and frame
count, and every byte with one single-codec ragged call per codec present on a second copy of the pool.  One test starts a child
process (a fresh one, under a time limit), and the two queue-mode flush fixtures one each (tests/queue_flush_case.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest

import mixed_case
import parity
import ragged_case
from mixed_case import mixed_frames, rows_of
from queue_channels import MBE_BATCH_QUEUE_SOFT, Channel as _Channel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
S = 2003
COUNTS = np.array([0, 0, 1, 2, 3, 5, 9, 17, 40])
KEYS = ("records", "results", "pcm16", "pcmf")


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
    return {k: out[k].cpu().numpy() for k in KEYS}


def _filled(dec, total, fill=0x5A):
    """output tensors whose every byte is `fill`: rows nobody writes keep it"""
    out = dec.make_outputs(0, want_float=True, total=total)
    for k in KEYS:
        out[k].view(dec.state.dtype).fill_(fill)
    return out


def _per_codec_ragged_calls(twin, codecs, counts, own, slots, soft, like):
    """what a mixed call replaces: one single-codec ragged call per codec present, on the twin's pool; gathered into the mixed layout
    (rows of streams no call covers keep the bytes of `like`)"""
    import torch

    got = {k: like[k].copy() for k in KEYS}
    for c, (who, at, frames) in own.items():
        twin.codec = c
        d_index = torch.from_numpy(slots[who].astype(np.int32)).to(twin.device)
        out = twin.decode_ragged(frames, counts[who], soft=soft, want_float=True, stream_index=d_index)
        torch.cuda.synchronize()
        for k in KEYS:
            got[k][at] = out[k].cpu().numpy()
    return got


def _check_oracle(oracle, own, counts, slots, state, rng, got, soft, what):
    """every stream against the oracle at its own codec and count; advances `state` / `rng` (the oracle's pool)"""
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE
    from test_gpu_ragged import _oracle_ragged

    for c, (who, at, frames) in own.items():
        f = frames
        ref = _oracle_ragged(oracle, c, counts[who], f, state[slots[who]], rng[slots[who]], soft)
        state[slots[who]], rng[slots[who]] = ref["state"], ref["rng"]
        w = f"{what} codec {c}"
        parity.check_exact(ref["records"], np.ascontiguousarray(got["records"][at]).view(RECORD_DTYPE).reshape(-1), w + ": records")
        parity.check_results(ref["results"], np.ascontiguousarray(got["results"][at]).view(RESULT_DTYPE).reshape(-1), w + ": results")
        parity.check_pcm(ref["pcmf"], got["pcmf"][at], ref["pcm16"], got["pcm16"][at], what=w + ": pcm", peak=ref["peak"])


def _same_bytes(what, a, b):
    for k in KEYS:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), f"{what}: {k} differ"


def _pool_bytes(dec):
    return (dec.state.cpu().numpy().tobytes(), dec.rng.cpu().numpy().tobytes(), dec.resident.cpu().numpy().tobytes() if dec.resident is not None else b"")


@pytest.mark.parametrize("indexed", [False, True], ids=["identity", "indexed"])
@pytest.mark.parametrize("resident", [False, True], ids=["abi", "resident"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_a_mixed_batch_equals_the_oracle_on_every_stream_and_the_per_codec_ragged_calls_on_every_byte(mbx, oracle, soft, resident, indexed):
    """~2,000 streams over all four codecs, counts 0..40 with idle streams, two launches on continuing state"""
    import torch
    from mbelib_neo_amd import _native, decoder

    pool = 2 * S + 3 if indexed else S
    slots = (np.random.default_rng(31).permutation(pool)[:S] if indexed else np.arange(S)).astype(np.int32)
    seeds = np.arange(pool) * 3 + 17
    dec = decoder.BatchDecoder(0, pool, seeds=seeds, resident=resident)
    twin = decoder.BatchDecoder(0, pool, seeds=seeds, resident=resident)
    d_index = torch.from_numpy(slots).to(dec.device) if indexed else None
    state, rng = oracle.init_state(pool), oracle.rng_seeded(seeds)
    codecs = mixed_case.codecs_for(S, 5)   # a slot keeps its codec from launch to launch
    assert all((codecs == c).sum() > 300 for c in range(4))
    strm = torch.cuda.current_stream().cuda_stream
    for launch in range(2):
        counts = COUNTS[np.random.default_rng(40 + launch).integers(0, len(COUNTS), size=S)]
        rows, own = mixed_frames(codecs, counts, tag=launch + 1, soft=soft)
        out = dec.decode_ragged(rows, counts, soft=soft, stream_index=d_index, codec=codecs, out=_filled(dec, int(counts.sum())))
        name = _native.lib().mbx_last_kernel_name(strm).decode()
        torch.cuda.synchronize()
        assert name == "mixed_stream_kernel_ragged" + ("_res" if resident else ""), name
        got = _numpy(out)
        what = f"launch {launch}"
        # the bytes of the calls it replaces: outputs, and the pools as the launches left them (before anything is materialised)
        _same_bytes(what, got, _per_codec_ragged_calls(twin, codecs, counts, own, slots, soft, got))
        assert _pool_bytes(dec) == _pool_bytes(twin), what + ": state, RNG state or elision words differ from the per-codec calls"
        # the oracle, every stream at its own codec and count
        _check_oracle(oracle, own, counts, slots, state, rng, got, soft, what)
        parity.check_state_blocks(state, dec.state_numpy(), what=what + ": state")
        parity.check_exact(rng, dec.rng_numpy(), what + ": rng")
        assert dec.state_numpy().tobytes() == twin.state_numpy().tobytes(), what + ": state bytes"


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_a_mixed_batch_of_one_codec_equals_the_ragged_call_of_that_codec(mbx, codec):
    import torch
    from mbelib_neo_amd import decoder

    n = 700
    counts = COUNTS[np.random.default_rng(60 + codec).integers(0, len(COUNTS), size=n)]
    codecs = np.full(n, codec, dtype=np.uint8)
    for soft in (False, True):
        rows, own = mixed_frames(codecs, counts, tag=3, soft=soft)
        dec = decoder.BatchDecoder(codec, n, seeds=np.arange(n) + 2, resident=True)
        twin = decoder.BatchDecoder(codec, n, seeds=np.arange(n) + 2, resident=True)
        got = _numpy(dec.decode_ragged(rows, counts, soft=soft, want_float=True, codec=codecs))
        want = _numpy(twin.decode_ragged(own[codec][2], counts, soft=soft, want_float=True))
        torch.cuda.synchronize()
        _same_bytes(f"codec {codec} soft {soft}", got, want)
        assert _pool_bytes(dec) == _pool_bytes(twin)


def test_more_streams_than_wave_slots_and_the_order_changes_no_byte(mbx, oracle):
    """the 6,500-stream skewed shape over four codecs on resident state (the order kernel runs): the bytes of the per-codec ragged
    calls, the oracle on a sample, and the same digest from a fresh child process with MBX_RAGGED_ORDER=0"""
    from mbelib_neo_amd import decoder

    assert "MBX_RAGGED_ORDER" not in os.environ, "this test compares the default with MBX_RAGGED_ORDER=0"
    out, dec, name, codecs, counts = mixed_case.run_skewed()
    assert name == "mixed_stream_kernel_ragged_res", name
    n = len(counts)
    got = _numpy(out)
    rows, own = mixed_frames(codecs, counts, tag=4)
    seeds = np.arange(n) * 5 + 1
    twin = decoder.BatchDecoder(0, n, seeds=seeds, resident=True)
    slots = np.arange(n, dtype=np.int32)
    _same_bytes("skewed", got, _per_codec_ragged_calls(twin, codecs, counts, own, slots, False, got))
    assert dec.state_numpy().tobytes() == twin.state_numpy().tobytes() and dec.rng_numpy().tobytes() == twin.rng_numpy().tobytes()
    sample = np.arange(0, n, 16)
    _, sown = mixed_frames(codecs[sample], counts[sample], tag=0)   # (the layout of the sample; frames below are the batch's own)
    state, rng = oracle.init_state(n), oracle.rng_seeded(seeds)
    picked = {k: got[k][rows_of(counts, sample)] for k in KEYS}
    for c, (who, at, _f) in sown.items():
        sown[c] = (who, at, rows[rows_of(counts, sample[who])][:, :own[c][2].shape[1]])
    _check_oracle(oracle, sown, counts[sample], sample.astype(np.int32), state, rng, picked, False, "skewed")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MBX_") or k in ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")}
    env["MBX_RAGGED_ORDER"] = "0"
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "mixed_case.py")], capture_output=True, text=True, timeout=600, env=env)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"mixed_case: the child process did not finish in {e.timeout} s -- nothing more is started on the card", returncode=3)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"mixed_case: the child process ended with status {r.returncode} -- nothing more is started on the card\n{tail}", returncode=3)
    assert r.returncode == 0, tail
    assert r.stdout.strip().splitlines()[-1] == f"{name} {ragged_case.digest(out, dec)}", tail


@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_a_codec_byte_that_names_no_codec_leaves_its_stream_alone(mbx, oracle, soft):
    import torch
    from mbelib_neo_amd import decoder

    n = 400
    counts = COUNTS[np.random.default_rng(9).integers(2, len(COUNTS), size=n)]
    codecs = mixed_case.codecs_for(n, 6)
    rows, own = mixed_frames(codecs, counts, tag=2, soft=soft)
    bad = np.array([17, 250])
    sent = codecs.copy()
    sent[bad] = 7
    seeds = np.arange(n) + 40
    dec = decoder.BatchDecoder(0, n, seeds=seeds, resident=True)
    before = _pool_bytes(dec)
    d_rows, d_off = dec.to_device(rows), torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dec.device)
    d_codec = torch.from_numpy(sent).to(dec.device)   # (past the Python face: it refuses such an array on the host)
    out = _filled(dec, int(counts.sum()))
    fn = mbx.lib().mbx_process_batch_soft_mixed if soft else mbx.lib().mbx_process_batch_mixed
    assert fn(n, d_codec.data_ptr(), d_off.data_ptr(), int(counts.sum()), None, d_rows.data_ptr(), dec.state.data_ptr(), dec.resident.data_ptr(),
              dec.rng.data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(), out["records"].data_ptr(),
              torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    got = _numpy(out)
    at = rows_of(counts, bad)
    for k in KEYS:
        assert (np.ascontiguousarray(got[k][at]).view(np.uint8) == 0x5A).all(), f"{k} rows of a stream with a bad codec byte were written"
    after = _pool_bytes(dec)
    psz, rsz = len(before[0]) // n, len(before[1]) // n
    for s in bad:
        assert after[0][s * psz:(s + 1) * psz] == before[0][s * psz:(s + 1) * psz], "state of a stream with a bad codec byte"
        assert after[1][s * rsz:(s + 1) * rsz] == before[1][s * rsz:(s + 1) * rsz] and after[2][4 * s:4 * s + 4] == before[2][4 * s:4 * s + 4]
    # every other stream: the oracle
    good = np.setdiff1d(np.arange(n), bad)
    state, rng = oracle.init_state(n), oracle.rng_seeded(seeds)
    keep = {c: (who[~np.isin(who, bad)], rows_of(counts, who[~np.isin(who, bad)]), f[~np.isin(np.repeat(who, counts[who]), bad)])
            for c, (who, _a, f) in own.items()}
    _check_oracle(oracle, keep, counts, np.arange(n, dtype=np.int32), state, rng, got, soft, "bad codec byte")
    parity.check_exact(rng[good], dec.rng_numpy()[good], "bad codec byte: rng")


def test_empty_mixed_batches_launch_nothing_and_a_captured_step_replays_like_direct_calls(mbx):
    import torch
    from mbelib_neo_amd import _native, decoder

    L = _native.lib()
    side = torch.cuda.Stream()
    n = 1500
    codecs = mixed_case.codecs_for(n, 8)
    counts = COUNTS[np.random.default_rng(12).integers(0, len(COUNTS), size=n)]
    total = int(counts.sum())
    rows, _ = mixed_frames(codecs, counts, tag=6)
    seeds = np.arange(n) + 9
    eager = decoder.BatchDecoder(0, n, seeds=seeds)
    want = []
    for _ in range(2):
        o = eager.decode_ragged(rows, counts, want_float=True, codec=codecs)
        want.append((o["pcm16"].clone(), o["pcmf"].clone(), o["results"].clone()))
    torch.cuda.synchronize()
    dec = decoder.BatchDecoder(0, n, seeds=seeds)
    d_rows, d_codec = dec.to_device(rows), torch.from_numpy(codecs).to(dec.device)
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).to(dec.device)
    out = dec.make_outputs(0, want_float=True, total=total)
    tail = (dec.state.data_ptr(), None, dec.rng.data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(),
            out["records"].data_ptr(), side.cuda_stream)
    before = _pool_bytes(dec)
    for fn in (L.mbx_process_batch_mixed, L.mbx_process_batch_soft_mixed):
        assert fn(0, d_codec.data_ptr(), d_off.data_ptr(), 0, None, d_rows.data_ptr(), *tail) == 0            # S == 0
        assert fn(n, d_codec.data_ptr(), d_off.data_ptr(), 0, None, d_rows.data_ptr(), *tail) == 0            # total_frames == 0
        assert fn(n, None, d_off.data_ptr(), total, None, d_rows.data_ptr(), *tail) == -1                     # no codec array
    assert L.mbx_last_kernel_name(side.cuda_stream) is None, "an empty mixed batch launched a stream kernel"
    torch.cuda.synchronize()
    assert _pool_bytes(dec) == before
    _native.check(L.mbx_reserve_stream(side.cuda_stream, total + (n + 63) // 64 + (total + 255) // 256), "mbx_reserve_stream")
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g, stream=side):
        rc = L.mbx_process_batch_mixed(n, d_codec.data_ptr(), d_off.data_ptr(), total, None, d_rows.data_ptr(), *tail)
    assert rc == 0, L.mbx_last_error()
    for k in range(2):
        g.replay()
        torch.cuda.synchronize()
        assert torch.equal(out["pcm16"], want[k][0]) and torch.equal(out["pcmf"], want[k][1]) and torch.equal(out["results"], want[k][2]), k
    assert dec.state_numpy().tobytes() == eager.state_numpy().tobytes() and dec.rng_numpy().tobytes() == eager.rng_numpy().tobytes()
    _native.check(L.mbx_release_stream(side.cuda_stream), "mbx_release_stream")


# ---- queue mode of the per-frame library ---------------------------------------------------------------------------------------
def _flush_case(scenario, env_extra):
    """tests/queue_flush_case.py in a fresh process under a time limit: {mode: its line}"""
    env = dict(os.environ, **env_extra)
    try:
        r = subprocess.run([sys.executable, os.path.join(HERE, "queue_flush_case.py"), scenario], capture_output=True, text=True, timeout=300, env=env)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"queue_flush_case {scenario}: the child process did not finish in {e.timeout} s -- nothing more is started on the card", returncode=3)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"queue_flush_case {scenario}: the child process ended with status {r.returncode} -- nothing more is started on the card\n{tail}", returncode=3)
    assert r.returncode in (0, 1), tail
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert sorted(lines) == ["0", "1"], tail
    return lines


@pytest.fixture(scope="module")
def dma_flush(mbx):
    return _flush_case("mixed48", {"MBE_NEO_ZERO_COPY_FLUSH": "0"})


@pytest.fixture(scope="module")
def chunked_flush(mbx):
    return _flush_case("chunks", {})


@pytest.mark.parametrize("mode", [0, 1], ids=["writeback", "resident"])
def test_queue_mode_flushes_all_codecs_and_counts_of_an_input_form_as_one_mixed_launch_set(mbx, mode):
    """48 channels of all four codecs, hard and soft, 1..9 pending frames each, ONE mbe_flush: every caller buffer and the final
    structs equal the synchronous per-frame calls.  (Which kernel ran is not visible from outside: the library keeps its stream to
    itself and queue mode gains no export; the flush is 24 (codec, form, count) groups, so both forms take the mixed launch set.)"""
    import shim_lib

    mbe = shim_lib.load()
    want = [_Channel(mbe, c) for c in range(48)]
    pending = 1 + np.arange(48) * 5 % 9
    for ch, k in zip(want, pending):   # synchronous: each channel alone (it owns the thread's RNG state like a queued channel its copy)
        for _ in range(int(k)):
            ch.call(mbe)
    got = [_Channel(mbe, c) for c in range(48)]
    assert mbe.mbe_batchBegin(mode | MBE_BATCH_QUEUE_SOFT) == 0
    try:
        for ch, k in zip(got, pending):
            for _ in range(int(k)):
                ch.call(mbe)
        assert mbe.mbe_batchPending() == int(pending.sum())
        assert mbe.mbe_flush() == int(pending.sum())
    finally:
        assert mbe.mbe_batchEnd() >= 0
    for a, b in zip(want, got):
        assert all(r == 0 for r in b.rets)
        for what, x, y in zip(("pcm", "result", "bits", "state"), a.outputs(), b.outputs()):
            assert x == y, f"channel {a.c} (codec {a.codec}, soft {a.soft}): {what} differs from the synchronous calls"


@pytest.mark.parametrize("mode", [0, 1], ids=["writeback", "resident"])
def test_queue_mode_flush_by_dma_copies_equals_the_synchronous_calls(dma_flush, mode):
    """the 48-channel scenario above in a process with MBE_NEO_ZERO_COPY_FLUSH=0: frames, index, offsets and codecs are uploaded, the
    kernels work on device arrays, results, records and ONE PCM chunk are copied back"""
    assert dma_flush[str(mode)] == "ok", dma_flush[str(mode)]


@pytest.mark.parametrize("mode", [0, 1], ids=["writeback", "resident"])
def test_queue_mode_flush_of_8195_rows_in_four_pcm_chunks_equals_the_synchronous_calls(chunked_flush, mode):
    """8,195 hard rows of 65 channels in three groups (tests/queue_flush_case.py, chunks): four PCM chunks of 2,049, 2,049, 2,049 and
    2,048 rows, int16 and float calls alternating by channel, chunk edges inside channels"""
    assert chunked_flush[str(mode)] == "ok", chunked_flush[str(mode)]
