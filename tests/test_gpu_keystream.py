"""GPU suite (-m gpu) for keystream input (include/mbx_keystream.h): a keyed call decrypts to the clear audio byte for byte, equals
the staged route FEC -> mbx_apply_keystream (or numpy on the host) -> mbx_process_records, follows the reference's split API on the
CPU oracle (tests/keyed_reference.py) under the bounds of tests/parity.py, is the unkeyed call with an all-zero or an absent
keystream, holds on a mixed ragged batch, keeps to its buffers (tests/keystream_cases.py, guarded arenas) and runs through
sessions.  Shapes: tests/keystream_cases.py.  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import keyed_reference
import keystream_cases as KC
import parity
from mbelib_neo_amd import keystream as K

pytestmark = pytest.mark.gpu
KEYS = ("records", "results", "pcm16", "pcmf")
FLAG_TONE, FLAG_ERASURE, FLAG_REPEAT, FLAG_MUTE = 0x10, 0x20, 0x40, 0x80


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _decoder(codec, S, resident, seed0=77):
    from mbelib_neo_amd import decoder

    return decoder.BatchDecoder(codec, S, seeds=np.arange(S) * 3 + seed0, resident=resident)


def _run(codec, S, T, frames, soft, resident, keystream=None):
    """one decoder call on a fresh pool: (output bytes, (state, rng, resident words), the kernel that ran)"""
    dec = _decoder(codec, S, resident)
    if soft:
        out = dec.decode_soft(frames, T, want_float=True, keystream=keystream)
    else:
        out = dec.decode(frames, T, want_float=True, keystream=keystream)
    name = KC.kernel_name()
    return KC.out_bytes(out), KC.pool_bytes(dec), name


def _same(what, a, b):
    for k in KEYS:
        assert a[0][k] == b[0][k], f"{what}: {k} differs"
    for k, x, y in zip(("state", "rng", "resident words"), a[1], b[1]):
        assert x == y, f"{what}: {k} differs"


def _staged_name(codec, T, resident):
    from mbelib_neo_amd import _native

    return _native.lib().mbx_stream_kernel_name(KC.STREAM_CODEC[codec], -T if resident else T).decode()


# ---- 1. decrypts to the clear audio ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("resident", [False, True], ids=["abi", "resident"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("S,T", KC.SHAPES)
@pytest.mark.parametrize("codec", [0, 1, 3])
def test_a_keyed_call_on_encrypted_frames_is_the_unkeyed_call_on_the_clear_frames(mbx, codec, S, T, soft, resident):
    clear, encrypted, rows, flips = KC.clear_and_encrypted(codec, S * T, tag=S + T)
    assert not np.array_equal(clear, encrypted)
    if soft:
        clear, encrypted = KC.soft_cells(codec, clear, 3, flips), KC.soft_cells(codec, encrypted, 3, flips)
    want = _run(codec, S, T, clear, soft, resident)
    got = _run(codec, S, T, encrypted, soft, resident, keystream=rows)
    _same(f"codec {codec} {S} x {T}", want, got)
    from mbelib_neo_amd.layout import RESULT_DTYPE

    res = np.frombuffer(got[0]["results"], dtype=RESULT_DTYPE)
    assert (res["total_errors"] > 0).any(), "the frames carry channel errors: the error context is not all zero"
    wrong = _run(codec, S, T, encrypted, soft, resident)   # (without the keystream the encrypted frames decode to something else)
    assert wrong[0]["records"] != want[0]["records"] and wrong[0]["pcm16"] != want[0]["pcm16"]
    if (S, T) == (257, 1):
        assert got[2] == _staged_name(codec, 1, resident), got[2]
        if not soft:
            assert "one_launch" in want[2] or "fused" in want[2], f"the unkeyed call of 257 x 1 takes a one-launch form, not {want[2]}"
        if codec == 0 and not soft and not resident:
            assert (want[2], got[2]) == ("imbe_one_launch_kernel", "imbe_stream_kernel_one")


# ---- 2. the staged identity -----------------------------------------------------------------------------------------------------------
def _staged(codec, S, T, frames, soft, rows, on_host):
    """mbx_fec_* / mbx_fec_soft, the keystream by mbx_apply_keystream (on_host: by numpy between the calls), mbx_process_records --
    on ABI triplets"""
    import torch
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import RECORD_DTYPE

    L = _native.lib()
    dec = _decoder(codec, S, False)
    out = dec.make_outputs(T, True, True, True)
    strm = torch.cuda.current_stream().cuda_stream
    d_in, n = KC.dev(frames), S * T
    if soft:
        _native.check(L.mbx_fec_soft(codec, d_in.data_ptr(), n, out["records"].data_ptr(), strm), "mbx_fec_soft")
    else:
        fn = {0: L.mbx_fec_imbe7200x4400, 1: L.mbx_fec_ambe3600x2450, 2: L.mbx_fec_imbe7100x4400, 3: L.mbx_fec_ambe3600x2450}[codec]
        _native.check(fn(d_in.data_ptr(), n, out["records"].data_ptr(), strm), "mbx_fec")
    if on_host:
        torch.cuda.synchronize()
        rec = K.apply(out["records"].cpu().numpy().reshape(-1).view(RECORD_DTYPE), rows, codec)
        out["records"].copy_(torch.from_numpy(rec.view(np.int32).reshape(n, 4)))
    else:
        d_key = KC.dev(rows)
        _native.check(L.mbx_apply_keystream(codec, out["records"].data_ptr(), n, d_key.data_ptr(), strm), "mbx_apply_keystream")
    rc = L.mbx_process_records(KC.STREAM_CODEC[codec], S, T, out["records"].data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(),
                               out["pcmf"].data_ptr(), out["results"].data_ptr(), strm)
    _native.check(rc, "mbx_process_records")
    return KC.out_bytes(out), KC.pool_bytes(dec), KC.kernel_name()


@pytest.mark.parametrize("soft,S,T", [(False, 257, 1), (False, 5, 3), (True, 9, 2), (True, 3, 5)])
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_a_keyed_call_is_fec_then_the_keystream_stage_then_process_records(mbx, codec, soft, S, T):
    from mbelib_neo_amd import framegen

    frames = KC.any_frames(codec, S, T, tag=21, soft=soft)
    rows = KC.random_rows(S * T, framegen.rng_for(0x4B5E0000 + codec))
    device_stage = _staged(codec, S, T, frames, soft, rows, on_host=False)
    host_stage = _staged(codec, S, T, frames, soft, rows, on_host=True)
    _same("mbx_apply_keystream against numpy on the host", device_stage, host_stage)
    abi = _run(codec, S, T, frames, soft, False, keystream=rows)
    _same("keyed call on ABI triplets against the staged route", device_stage, abi)
    assert abi[2] == device_stage[2] or (S, T) == (257, 1), (abi[2], device_stage[2])
    res = _run(codec, S, T, frames, soft, True, keystream=rows)
    for k in KEYS:
        assert res[0][k] == device_stage[0][k], f"keyed call on resident state: {k} differs"
    assert res[1][0] == device_stage[1][0] and res[1][1] == device_stage[1][1], "keyed call on resident state: the materialised state or the RNG state differs"
    assert res[2] == _staged_name(codec, T, True), res[2]
    # BatchDecoder.decode(staged=True, keystream=...) is the same staged route
    if not soft:
        dec = _decoder(codec, S, False)
        out = dec.decode(frames, T, want_float=True, staged=True, keystream=rows)
        _same("decode(staged=True, keystream=rows)", device_stage, (KC.out_bytes(out), KC.pool_bytes(dec)))


# ---- 3. the reference's semantics -----------------------------------------------------------------------------------------------------
def _reference_case(oracle, codec, S, T):
    """(encrypted frames with channel errors, keystream rows): the keystream is chosen so that the decrypted stream holds what is
    wanted -- IMBE: all-voiced frames; AMBE: voice, tones and erasure signatures --, and one stream's frames are beyond correction"""
    import imbe7100_frames
    from mbelib_neo_amd import framegen

    rng = framegen.rng_for(0x4B5F0000 + codec)
    n = S * T
    sent = KC.param_bits(0 if codec in (0, 2) else 1, n, rng)            # what is on the air: valid frames of other content
    target = KC.param_bits(0 if codec in (0, 2) else 1, n, rng)          # what the channel carries once decrypted
    if codec in (1, 3):
        for f in range(2 * T, 3 * T):   # stream 2: tone, voice, erasure signature, ... (the bit patterns of tests/edge_mix.py)
            if f % 3 == 0:
                target[f, 0:6] = 1
                target[f, 45:49] = 0
                target[f, 12:20] = [(40 >> (7 - j)) & 1 for j in range(8)]
            elif f % 3 == 2:
                target[f, 0:4] = 1
                target[f, 4] = 0
                target[f, 37] = 0
    if codec == 2:
        frames = imbe7100_frames.encode_imbe7100x4400(sent, oracle)
    else:
        frames = KC.encode(codec, sent)
    clean = frames
    frames = framegen.flip_bits(clean, codec, 0.01, rng)
    if codec in (1, 3):   # stream 1: frames the AMBE decoders answer with a repeat, then a mute (tests/edge_mix.py: three flipped data cells per Golay word)
        cells = np.unpackbits(clean[T:2 * T], axis=1)
        for i in range(T):
            cells[i, rng.choice(12, 3, replace=False)] ^= 1
            cells[i, 24 + rng.choice(12, 3, replace=False)] ^= 1
        frames[T:2 * T] = np.packbits(cells, axis=1)
    else:                 # ... IMBE: heavily damaged frames
        frames[T:2 * T] = framegen.flip_bits(frames[T:2 * T], codec, 0.2, rng)
    from oracle_lib import records_to_bits

    decoded = records_to_bits(oracle.fec_batch(codec, frames), K.NBITS[codec]).astype(np.uint8)
    return frames, K.rows_from_bits(decoded ^ target)


@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_a_keyed_call_follows_the_references_split_api_on_the_oracle(mbx, oracle, codec):
    from mbelib_neo_amd.layout import PARMS_DTYPE, RECORD_DTYPE, RESULT_DTYPE, RNG_DTYPE

    S, T = 4, 6
    frames, rows = _reference_case(oracle, codec, S, T)
    seeds = np.arange(S) * 3 + 77
    ref = keyed_reference.process_batch_keyed(oracle, codec, S, T, frames, rows, oracle.init_state(S), oracle.rng_seeded(seeds))
    flags = ref["results"]["flags"]
    assert (ref["results"]["total_errors"] > 0).any(), "the frames carry channel errors"
    plain = (flags & (FLAG_TONE | FLAG_ERASURE | FLAG_REPEAT | FLAG_MUTE)) == 0
    assert plain.any() and (flags & FLAG_REPEAT).any(), "the decrypted stream holds voice and repeated frames"
    if codec in (1, 3):
        assert (flags & FLAG_TONE).any() and (flags & (FLAG_ERASURE | FLAG_MUTE)).any(), "AMBE: tone frames, and an erasure or a muted frame"
    for resident in (False, True):
        dec = _decoder(codec, S, resident)
        out = dec.decode(frames, T, want_float=True, keystream=rows)
        got = KC.out_bytes(out)
        what = f"codec {codec} resident {resident}"
        parity.check_exact(ref["records"], np.frombuffer(got["records"], dtype=RECORD_DTYPE), what + ": records", T)
        with parity.located(T):
            parity.check_results(ref["results"], np.frombuffer(got["results"], dtype=RESULT_DTYPE), what + ": results")
        # (the per-frame reference calls report no pre-clip peak: every frame is held to the bound of the peak it is known to have
        # reached, the largest reference sample -- never a wider bound than that of the true peak)
        pcmf = np.frombuffer(got["pcmf"], dtype=np.float32).reshape(-1, 160)
        pcm16 = np.frombuffer(got["pcm16"], dtype=np.int16).reshape(-1, 160)
        parity.check_pcm_located(ref["pcmf"], pcmf, ref["pcm16"], pcm16, T, what=what + ": pcm", peak=np.abs(ref["pcmf"]).max(axis=1))
        state = np.frombuffer(KC.pool_bytes(dec)[0], dtype=PARMS_DTYPE).reshape(S, 3)
        parity.check_state(ref["state"], state, what=what + ": state")
        parity.check_exact(ref["rng"], np.frombuffer(KC.pool_bytes(dec)[1], dtype=RNG_DTYPE), what + ": rng")


# ---- 4. zero and absent keys ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
@pytest.mark.parametrize("S,T", [(257, 1), (3, 5)])
@pytest.mark.parametrize("codec", [0, 1])
def test_an_all_zero_keystream_and_no_keystream_are_the_unkeyed_call(mbx, codec, S, T, soft):
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    frames = KC.any_frames(codec, S, T, tag=23, soft=soft)
    for resident in (False, True):
        want = _run(codec, S, T, frames, soft, resident)
        zero = _run(codec, S, T, frames, soft, resident, keystream=np.zeros((S * T, K.ROW_BYTES), dtype=np.uint8))
        _same(f"all-zero keystream, resident {resident}", want, zero)
        # d_keystream = NULL: the unkeyed call of the same form, launch for launch
        dec = _decoder(codec, S, resident)
        out = dec.make_outputs(T, True, True, True)
        d_in = KC.dev(frames)
        rc = L.mbx_process_batch_keyed(codec, S, T, None, None if soft else d_in.data_ptr(), d_in.data_ptr() if soft else None, None, dec.state.data_ptr(),
                                       KC.ptr(dec.resident), dec.rng.data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(),
                                       out["records"].data_ptr(), torch.cuda.current_stream().cuda_stream)
        _native.check(rc, "mbx_process_batch_keyed")
        absent = (KC.out_bytes(out), KC.pool_bytes(dec), KC.kernel_name())
        _same(f"no keystream, resident {resident}", want, absent)
        assert absent[2] == want[2], "no keystream: the unkeyed call's kernel"
        if (S, T) == (257, 1) and not soft:
            assert zero[2] != want[2] and zero[2] == _staged_name(codec, 1, resident)


# ---- 5. mixed ragged --------------------------------------------------------------------------------------------------------------------
def _ragged_call(L, strm, codec, d_codec, S, d_offsets, total, d_index, d_frames, soft, d_key, pool, out):
    from mbelib_neo_amd import _native

    rc = L.mbx_process_batch_ragged_keyed(codec, KC.ptr(d_codec), S, d_offsets.data_ptr(), total, KC.ptr(d_index), None if soft else d_frames.data_ptr(),
                                          d_frames.data_ptr() if soft else None, KC.ptr(d_key), pool["state"].data_ptr(), KC.ptr(pool["resident"]),
                                          pool["rng"].data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(), out["results"].data_ptr(),
                                          out["records"].data_ptr(), strm)
    _native.check(rc, "mbx_process_batch_ragged_keyed")


def _pool(resident):
    import torch
    import memory_cases

    state, rng = memory_cases._initial(KC.MIXED_POOL, 3)
    return {"state": KC.dev(state), "rng": KC.dev(rng), "resident": torch.zeros(KC.MIXED_POOL, dtype=torch.int32, device="cuda") if resident else None}


def _outputs(total):
    import torch

    fill = {"records": (4, torch.int32), "results": (5, torch.int32), "pcm16": (160, torch.int16), "pcmf": (160, torch.float32)}
    return {k: torch.full((total, w), 0x5A, dtype=t, device="cuda") for k, (w, t) in fill.items()}


@pytest.mark.parametrize("resident", [False, True], ids=["abi", "resident"])
@pytest.mark.parametrize("soft", [False, True], ids=["hard", "soft"])
def test_a_keyed_mixed_batch_is_one_keyed_ragged_call_per_codec(mbx, soft, resident):
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    S, total = len(KC.MIXED_COUNTS), int(KC.MIXED_COUNTS.sum())
    rows, key = KC.mixed_batch(9, soft)
    offsets = np.concatenate([[0], np.cumsum(KC.MIXED_COUNTS)]).astype(np.int32)
    # the mixed call
    mixed_pool, mixed_out = _pool(resident), _outputs(total)
    before = {k: v.cpu().numpy().copy() for k, v in mixed_pool.items() if v is not None}
    d_off, d_idx, d_codec, d_rows, d_key = (torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (offsets, KC.MIXED_SLOTS, KC.MIXED_CODECS, rows, key))
    _ragged_call(L, strm, 0, d_codec, S, d_off, total, d_idx, d_rows, soft, d_key, mixed_pool, mixed_out)
    assert KC.kernel_name() == "mixed_stream_kernel_ragged" + ("_res" if resident else "")
    torch.cuda.synchronize()
    # one keyed ragged call per codec present, on one pool
    pool, outs = _pool(resident), {}
    for codec in range(4):
        who, at, own = KC.own_frames(rows, codec, soft)
        off = np.concatenate([[0], np.cumsum(KC.MIXED_COUNTS[who])]).astype(np.int32)
        n = int(off[-1])
        out = _outputs(max(n, 1))
        t = [torch.from_numpy(np.ascontiguousarray(a)).cuda() for a in (off, KC.MIXED_SLOTS[who], own.reshape(-1), key[at].reshape(-1))]
        if n:
            _ragged_call(L, strm, codec, None, len(who), t[0], n, t[1], t[2], soft, t[3], pool, out)
        torch.cuda.synchronize()
        outs[codec] = (at, out)
    for codec, (at, out) in outs.items():
        for k in KEYS:
            assert np.array_equal(mixed_out[k].cpu().numpy()[at], out[k].cpu().numpy()[:len(at)]), f"codec {codec}: {k} differs from the single-codec keyed call"
    for k in ("rng", "resident", "state"):
        if mixed_pool[k] is not None:
            if k == "state" and resident:
                for p_ in (mixed_pool, pool):
                    _native.check(L.mbx_resident_materialize(KC.MIXED_POOL, None, p_["state"].data_ptr(), p_["resident"].data_ptr(), strm), "materialize")
                torch.cuda.synchronize()
            assert mixed_pool[k].cpu().numpy().tobytes() == pool[k].cpu().numpy().tobytes(), f"{k} of the pool differs"
    # the stream whose codec byte names no codec, and the stream without frames, keep every byte
    idle = np.flatnonzero((KC.MIXED_COUNTS == 0) | (KC.MIXED_CODECS >= 4))
    named = KC.MIXED_SLOTS[np.setdiff1d(np.arange(S), idle)]
    rest = np.setdiff1d(np.arange(KC.MIXED_POOL), named)
    assert KC.MIXED_SLOTS[6] in rest and KC.MIXED_SLOTS[0] in rest
    for k in ("state", "rng", "resident"):
        if mixed_pool[k] is not None:
            a, b = mixed_pool[k].cpu().numpy().reshape(KC.MIXED_POOL, -1), before[k].reshape(KC.MIXED_POOL, -1)
            assert a[rest].tobytes() == b[rest].tobytes(), f"{k}: an idle slot changed"
    held = np.concatenate([np.arange(offsets[i], offsets[i + 1]) for i in idle])
    assert held.size == 3
    for k in KEYS:
        got = mixed_out[k].cpu().numpy()[held]
        assert np.array_equal(got, np.full_like(got, 0x5A)), f"{k}: rows of a stream of no codec were written"


# ---- 6. memory contract ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", KC.KEYSTREAM_CASES, ids=[c.id for c in KC.KEYSTREAM_CASES])
def test_a_keyed_call_between_guard_bands(mbx, case):
    case.fn(**case.args)


# ---- 7. sessions ----------------------------------------------------------------------------------------------------------------------
def _submit(L, sess, n, T, index, frames, soft, rows):
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import RECORD_DTYPE, RESULT_DTYPE

    nf = n * T
    got = {"pcm16": np.zeros((nf, 160), np.int16), "pcmf": np.zeros((nf, 160), np.float32), "results": np.zeros(nf, RESULT_DTYPE),
           "records": np.zeros(nf, RECORD_DTYPE)}
    rc = L.mbx_session_submit_keyed(sess, n, T, None if index is None else index.ctypes.data, None if soft else frames, frames if soft else None,
                                    rows, got["pcm16"].ctypes.data, got["pcmf"].ctypes.data, got["results"].ctypes.data, got["records"].ctypes.data)
    _native.check(rc, "mbx_session_submit_keyed")
    _native.check(L.mbx_session_wait(sess), "wait")
    return {k: v.tobytes() for k, v in got.items()}


def _indexed(dec, n, T, index, frames, rows):
    """mbx_process_batch_keyed on n named slots of a decoder's pool: the output bytes"""
    import torch
    from mbelib_neo_amd import _native

    out = dec.make_outputs(T, True, True, True, streams=n)
    d_idx, d_in, d_key = torch.from_numpy(index).cuda(), KC.dev(frames), KC.dev(rows)
    rc = _native.lib().mbx_process_batch_keyed(dec.codec, n, T, d_idx.data_ptr(), d_in.data_ptr(), None, d_key.data_ptr(), dec.state.data_ptr(),
                                               KC.ptr(dec.resident), dec.rng.data_ptr(), out["pcm16"].data_ptr(), out["pcmf"].data_ptr(),
                                               out["results"].data_ptr(), out["records"].data_ptr(), torch.cuda.current_stream().cuda_stream)
    _native.check(rc, "mbx_process_batch_keyed")
    return KC.out_bytes(out)


def test_keyed_submits_of_a_session_are_the_launchers_calls_on_a_pool(mbx):
    from mbelib_neo_amd import _native, framegen
    from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

    L = _native.lib()
    codec, S, T = 1, 64, 2
    rng = framegen.rng_for(0x4B600000)
    hard = [np.ascontiguousarray(KC.any_frames(codec, S, T, tag=31 + i)).reshape(-1) for i in range(3)]
    soft = np.ascontiguousarray(KC.any_frames(codec, S, T, tag=35, soft=True)).reshape(-1)
    keys = [KC.random_rows(S * T, rng) for _ in range(4)]
    subset = np.arange(S - 1, 0, -3)[:17].astype(np.int32)
    assert len(subset) == 17
    sub_frames = np.ascontiguousarray(KC.any_frames(codec, 17, T, tag=36)).reshape(-1)
    seeds = (np.arange(S) * 3 + 77).astype(np.uint32)
    sess = C.c_void_p()
    _native.check(L.mbx_session_create(C.byref(sess), codec, S, S * T, 1 | 2 | 4), "create")
    pinned = []
    try:
        _native.check(L.mbx_session_seed(sess, 0, S, seeds.ctypes.data), "seed")

        def pin(a):   # the same bytes in mbx_host_alloc memory
            p = L.mbx_host_alloc(a.nbytes)
            assert p
            pinned.append(p)
            C.memmove(p, a.ctypes.data, a.nbytes)
            return p

        got = [
            _submit(L, sess, S, T, None, hard[0].ctypes.data, False, keys[0].ctypes.data),        # keyed hard, pageable
            _submit(L, sess, S, T, None, hard[1].ctypes.data, False, None),                       # unkeyed hard
            _submit(L, sess, S, T, None, pin(soft), True, pin(keys[1])),                          # keyed soft, pinned frames and rows
            _submit(L, sess, 17, T, subset, sub_frames.ctypes.data, False, keys[2][:17 * T].ctypes.data),   # keyed, indexed: 17 of the 64
            _submit(L, sess, S, T, None, hard[2].ctypes.data, False, pin(keys[3])),               # keyed hard, rows pinned, frames pageable
        ]
        state, rg = np.zeros((S, 3), PARMS_DTYPE), np.zeros(S, RNG_DTYPE)
        _native.check(L.mbx_session_get_state(sess, 0, S, state.ctypes.data, rg.ctypes.data), "get_state")
    finally:
        L.mbx_session_destroy(sess)
        for p in pinned:
            L.mbx_host_free(p)
    # the same sequence through the launchers on a pool (resident, as a session's)
    import torch

    dec = _decoder(codec, S, True)
    want = [
        KC.out_bytes(dec.decode(hard[0], T, want_float=True, keystream=keys[0])),
        KC.out_bytes(dec.decode(hard[1], T, want_float=True)),
        KC.out_bytes(dec.decode_soft(soft.reshape(S * T, -1, 2), T, want_float=True, keystream=keys[1])),
        _indexed(dec, 17, T, subset, sub_frames, keys[2][:17 * T]),
        KC.out_bytes(dec.decode(hard[2], T, want_float=True, keystream=keys[3])),
    ]
    for i, (g, w) in enumerate(zip(got, want)):
        for k in KEYS:
            assert g[k] == w[k], f"submit {i}: {k} differs from the launcher's bytes"
    assert state.tobytes() == KC.pool_bytes(dec)[0] and rg.tobytes() == KC.pool_bytes(dec)[1]


def test_a_mixed_session_refuses_the_keyed_submit(mbx):
    from mbelib_neo_amd import _native

    L = _native.lib()
    codecs = np.array([0, 1, 2, 3], dtype=np.uint8)
    sess = C.c_void_p()
    _native.check(L.mbx_session_create_mixed(C.byref(sess), 4, codecs.ctypes.data, 8, 1), "create_mixed")
    try:
        frames, rows = np.zeros(4 * 18, dtype=np.uint8), np.zeros(4 * 12, dtype=np.uint8)
        pcm = np.zeros((4, 160), dtype=np.int16)
        assert L.mbx_session_submit_keyed(sess, 4, 1, None, frames.ctypes.data, None, rows.ctypes.data, pcm.ctypes.data, None, None, None) == -1
        assert b"mbx_session_submit_keyed" in L.mbx_last_error() and b"mixed session" in L.mbx_last_error()
    finally:
        L.mbx_session_destroy(sess)
