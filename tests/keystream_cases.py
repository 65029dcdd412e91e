"""Keystream input (include/mbx_keystream.h): what the CPU and GPU suites share.  The shapes, the makers of clear / encrypted frame
pairs and of keystream rows, thin wrappers over the keyed entry points on torch tensors, and the memory-contract cases in
tests/guarded.py arenas (a list of their own, KEYSTREAM_CASES: memory_cases.CASES stays what tests/test_memory_contract_host.py
holds it to).  Importable without a GPU."""
from collections import namedtuple

import numpy as np

import guarded
import memory_cases
import mixed_case
import ragged_case
import soft_mix
from mbelib_neo_amd import framegen
from mbelib_neo_amd import keystream as K
from mbelib_neo_amd.layout import FRAME_BYTES, ROW_WIDTHS

# The smallest shapes at which each piece can go wrong: 257 x 1 -- a block boundary of the 256-thread front, and the first S at which
# the unkeyed call takes a one-launch form; 3 x 5 -- LDS instances, IMBE expands records in the stream kernel; 5 x 3 -- HBM-slot
# instances through the expand launch.  (The soft front also runs at 9 x 2: the staged identity and the guarded cases.)
SHAPES = ((257, 1), (3, 5), (5, 3))
CELLS = soft_mix.CELLS
STREAM_CODEC = {0: 0, 1: 1, 2: 0, 3: 3}          # the codec whose stream stage a codec's records go to
PROTECTED_ROWS = {0: range(7), 1: range(2), 3: range(2)}   # rows of the frame that carry a code word (the rest is sent bare)
# the mixed ragged batch: every codec, a count of 0, a codec byte that names no codec
MIXED_CODECS = np.array([0, 1, 2, 3, 0, 1, 9], dtype=np.uint8)
MIXED_COUNTS = np.array([0, 1, 4, 2, 5, 1, 3], dtype=np.int64)
MIXED_POOL = 11
MIXED_SLOTS = np.array([9, 2, 7, 0, 10, 4, 5], dtype=np.int32)   # a permutation into a pool with slots nobody names


def param_bits(codec, n, rng):
    return framegen.imbe_voiced_param_bits(n, rng) if codec == 0 else framegen.ambe_voice_param_bits(n, rng)


def encode(codec, bits):
    """clean wire frames of parameter bits (codec 3 shares the frame and the FEC of 3600x2450)"""
    return framegen.encode_imbe7200x4400(bits) if codec == 0 else framegen.encode_ambe3600x2450(bits)


def flip_mask(codec, n, rng):
    """[n, frame bytes]: at most one flipped cell per protected row (every code word corrects it), about every other row"""
    widths = ROW_WIDTHS[codec]
    cells = np.zeros((n, 8 * FRAME_BYTES[codec]), dtype=np.uint8)
    off = 0
    for r, w in enumerate(widths):
        if r in PROTECTED_ROWS[codec]:
            hit = rng.integers(0, 2, size=n).astype(bool)
            cells[np.flatnonzero(hit), off + rng.integers(0, w, size=int(hit.sum()))] = 1
        off += w
    return np.packbits(cells, axis=1)


def random_rows(n, rng):
    """keystream rows with every bit random, the ones beyond nbits included (they are ignored)"""
    return rng.integers(0, 256, size=(n, K.ROW_BYTES), dtype=np.uint8)


def clear_and_encrypted(codec, n, tag):
    """(clear frames, encrypted frames, keystream rows, flip mask): clear = encode(b), encrypted = encode(b ^ k), the same cells flipped
    in both"""
    rng = framegen.rng_for(0x4B590000 + 16 * int(tag) + codec)
    b = param_bits(codec, n, rng)
    k = rng.integers(0, 2, size=b.shape, dtype=np.uint8)
    flips = flip_mask(codec, n, rng)
    rows = K.rows_from_bits(k)
    rows[:, -1] = rng.integers(0, 256, size=n, dtype=np.uint8)   # junk beyond bit 88
    if K.NBITS[codec] == 49:
        rows[:, 7:] = rng.integers(0, 256, size=(n, 5), dtype=np.uint8)   # ... and beyond bit 56; bits 49..55 share a byte with the key
        rows[:, 6] |= rng.integers(0, 128, size=n, dtype=np.uint8)
    assert np.array_equal(K.bits_from_rows(rows, codec), k)
    return encode(codec, b) ^ flips, encode(codec, b ^ k) ^ flips, rows, flips


def soft_cells(codec, packed, tag, flips):
    """[n, cells, 2] cells whose hard decisions are the frames' bits.  The reliabilities depend on the cell's place and on `tag` alone,
    so two frame arrays of one shape get the same ones: 128..255, and 1..16 on the cells `flips` (a wire-bit mask as flip_mask makes
    it) names.  The code word that was sent then costs at most 16 and every other one more than 6 x 128 - 16: the search has ONE best
    candidate in every block, and no rule for equal costs -- which may look at the candidates' values -- is asked."""
    hard, used = soft_mix.cells_from_packed(codec, packed)
    weak, _ = soft_mix.cells_from_packed(codec, flips)
    rng = framegen.rng_for(0x4B5A0000 + int(tag))
    rel = np.where(weak == 1, rng.integers(1, 17, size=hard.shape, dtype=np.uint8), rng.integers(128, 256, size=hard.shape, dtype=np.uint8))
    return np.ascontiguousarray(np.stack([np.where(used, hard, 0), np.where(used, rel, 0)], axis=-1).astype(np.uint8))


def any_frames(codec, S, T, tag, soft=False):
    """frames of any of the four codecs, stream-major: the edge mix / soft mix"""
    return ragged_case.ragged_frames(codec, np.full(S, T, dtype=np.int64), tag, soft=soft)


def mixed_batch(tag, soft):
    """(rows of the mixed batch -- [total, 18], soft: [total, 184 * 2] --, keystream rows); the stream whose codec byte names no codec
    brings rows like any other (they must not be looked at)"""
    good = np.where(MIXED_CODECS < 4, MIXED_CODECS, 0).astype(np.uint8)
    rows, _ = mixed_case.mixed_frames(good, MIXED_COUNTS, tag, soft=soft)
    return rows, random_rows(int(MIXED_COUNTS.sum()), framegen.rng_for(0x4B5B0000 + tag))


def own_frames(rows, codec, soft):
    """(streams of `codec` in the mixed batch, their batch rows, their frames cut to the codec's own size)"""
    who = np.flatnonzero(MIXED_CODECS == codec)
    at = mixed_case.rows_of(MIXED_COUNTS, who)
    width = 2 * CELLS[codec] if soft else FRAME_BYTES[codec]
    return who, at, np.ascontiguousarray(rows[at][:, :width])


# ---- the keyed entry points on torch tensors -----------------------------------------------------------------------------------
def ptr(t):
    return t.data_ptr() if t is not None else None


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def kernel_name():
    import torch
    from mbelib_neo_amd import _native

    return (_native.lib().mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream) or b"").decode()


def pool_bytes(dec, materialize=True):
    """(state, rng, resident words) of a decoder as bytes; the elision words as they are BEFORE the state is materialised"""
    import torch

    res = dec.resident.cpu().numpy().tobytes() if dec.resident is not None else b""
    if not materialize:
        torch.cuda.synchronize()
        return dec.state.cpu().numpy().tobytes(), dec.rng_numpy().tobytes(), res
    return dec.state_numpy().tobytes(), dec.rng_numpy().tobytes(), res


def out_bytes(out):
    import torch

    torch.cuda.synchronize()
    return {k: out[k].cpu().numpy().tobytes() for k in ("records", "results", "pcm16", "pcmf") if out.get(k) is not None}


# ---- memory-contract cases -------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id covers fn args")
KEYSTREAM_CASES = []


def _case(cid, covers, fn, **args):
    KEYSTREAM_CASES.append(Case(cid, tuple(covers), fn, args))


def apply_stage(codec):
    """mbx_apply_keystream: 257 records in place, the keystream read-only at exactly 4 bytes; w[3] and the bits beyond nbits keep
    their bytes, the rest is the numpy definition's"""
    L, _native, strm = memory_cases._lib()
    n = 257
    rng = framegen.rng_for(0x4B5C0000 + codec)
    rec = rng.integers(0, 1 << 32, size=(n, 4), dtype=np.uint64).astype(np.uint32)
    rows = random_rows(n, rng)
    specs = [guarded.buf("records", 16 * n, "records"), guarded.buf("keystream", K.ROW_BYTES * n, "index", True)]

    def call(run):
        _native.check(L.mbx_apply_keystream(codec, run.p("records"), n, run.p("keystream"), strm), "mbx_apply_keystream")

    got = memory_cases.twice(f"apply keystream codec {codec}", specs, {"records": rec, "keystream": rows}, call)
    from mbelib_neo_amd.layout import RECORD_DTYPE

    want = K.apply(rec.reshape(-1).view(RECORD_DTYPE), rows, codec)
    assert got["records"].tobytes() == want.tobytes()


def batch(codec, S, T, soft, indexed, resident, skip=None):
    """mbx_process_batch_keyed with every buffer of the call in one guarded arena; skip: an optional output that is NULL"""
    L, _native, strm = memory_cases._lib()
    pool = 2 * S + 3 if indexed else S
    slots = np.arange(pool - 2, 0, -2)[:S].astype(np.int32)
    frames = np.ascontiguousarray(any_frames(codec, S, T, 5, soft)).reshape(-1)
    rows = random_rows(S * T, framegen.rng_for(0x4B5D0000 + codec))
    state, rng = memory_cases._initial(pool, 3)
    want = [k for k in ("pcm16", "pcmf", "results") if k != skip]
    specs = [guarded.buf("frames", frames.size, "soft" if soft else guarded.frames_kind(codec), True),
             guarded.buf("keystream", rows.size, "index", True), guarded.buf("state", state.size, "state"),
             guarded.buf("rng", rng.size, "rng")] + memory_cases._out_specs(S * T, want)
    inputs = {"frames": frames, "keystream": rows, "state": state, "rng": rng}
    if resident:
        specs.append(guarded.buf("resident", 4 * pool, "resident"))
        inputs["resident"] = np.zeros(pool, dtype=np.uint32)
    if indexed:
        specs.append(guarded.buf("index", 4 * S, "index", True))
        inputs["index"] = slots

    def call(run):
        rc = L.mbx_process_batch_keyed(codec, S, T, run.p("index"), None if soft else run.p("frames"), run.p("frames") if soft else None,
                                       run.p("keystream"), run.p("state"), run.p("resident"), run.p("rng"), run.p("pcm16"), run.p("pcmf"),
                                       run.p("results"), run.p("records"), strm)
        _native.check(rc, "mbx_process_batch_keyed")

    return memory_cases.twice(f"keyed batch codec {codec} {S} x {T} soft {soft} indexed {indexed} resident {resident} without {skip}", specs, inputs, call)


def ragged_mixed(soft, resident, skip=None):
    """mbx_process_batch_ragged_keyed, mixed: the 7-stream batch; the stream whose codec byte names no codec and the stream without
    frames keep their slots and their output rows (they still hold the pre-fill)"""
    L, _native, strm = memory_cases._lib()
    S, total = len(MIXED_COUNTS), int(MIXED_COUNTS.sum())
    frames, rows = mixed_batch(7, soft)
    want = [k for k in ("pcm16", "pcmf", "results") if k != skip]
    offsets = np.concatenate([[0], np.cumsum(MIXED_COUNTS)]).astype(np.int32)
    state, rng = memory_cases._initial(MIXED_POOL, 3)
    specs = [guarded.buf("offsets", 4 * (S + 1), "index", True), guarded.buf("frames", frames.size, "soft" if soft else "frames2", True),
             guarded.buf("keystream", rows.size, "index", True), guarded.buf("index", 4 * S, "index", True), guarded.buf("codec", S, "codec", True),
             guarded.buf("state", state.size, "state"), guarded.buf("rng", rng.size, "rng")] + memory_cases._out_specs(total, want)
    inputs = {"offsets": offsets, "frames": frames.reshape(-1), "keystream": rows, "index": MIXED_SLOTS, "codec": MIXED_CODECS, "state": state, "rng": rng}
    if resident:
        specs.append(guarded.buf("resident", 4 * MIXED_POOL, "resident"))
        inputs["resident"] = np.zeros(MIXED_POOL, dtype=np.uint32)
    idle = np.flatnonzero((MIXED_COUNTS == 0) | (MIXED_CODECS >= 4))

    def call(run):
        rc = L.mbx_process_batch_ragged_keyed(0, run.p("codec"), S, run.p("offsets"), total, run.p("index"), None if soft else run.p("frames"),
                                              run.p("frames") if soft else None, run.p("keystream"), run.p("state"), run.p("resident"), run.p("rng"),
                                              run.p("pcm16"), run.p("pcmf"), run.p("results"), run.p("records"), strm)
        _native.check(rc, "mbx_process_batch_ragged_keyed")

    def after(run, got):
        st, rg = got["state"].reshape(MIXED_POOL, -1), got["rng"].reshape(MIXED_POOL, -1)
        rest = np.setdiff1d(np.arange(MIXED_POOL), MIXED_SLOTS[np.setdiff1d(np.arange(S), idle)])
        assert st[rest].tobytes() == state.reshape(MIXED_POOL, -1)[rest].tobytes() and rg[rest].tobytes() == rng.reshape(MIXED_POOL, -1)[rest].tobytes(), \
            "a slot without frames, or of no codec, changed"
        if resident:
            assert not got["resident"].view(np.uint32)[rest].any(), "the elision word of an idle slot changed"
        for k in got:
            if k in memory_cases.OUT_BYTES:
                for i in idle:
                    lo, hi = int(offsets[i]) * memory_cases.OUT_BYTES[k], int(offsets[i + 1]) * memory_cases.OUT_BYTES[k]
                    assert got[k][lo:hi].tobytes() == run.arena.prefill_bytes(k, lo, hi).tobytes(), f"{k}: rows of idle stream {i} were written"
                    got[k][lo:hi] = 0   # (the pre-fill differs between the two runs, as it must)

    return memory_cases.twice(f"keyed mixed ragged soft {soft} resident {resident} without {skip}", specs, inputs, call, after=after)


def misaligned():
    """a keystream pointer at address % 4 == 2 is refused before any launch: every output still holds its pre-fill"""
    import torch

    L, _native, strm = memory_cases._lib()
    S, T, codec = 5, 3, 0
    frames = np.ascontiguousarray(any_frames(codec, S, T, 5)).reshape(-1)
    state, rng = memory_cases._initial(S, 3)
    offsets = (np.arange(S + 1) * T).astype(np.int32)
    specs = [guarded.buf("frames", frames.size, "frames2", True), guarded.buf("keystream", K.ROW_BYTES * S * T + 2, "index", True),
             guarded.buf("offsets", 4 * (S + 1), "index", True), guarded.buf("state", state.size, "state"), guarded.buf("rng", rng.size, "rng")] \
        + memory_cases._out_specs(S * T, ("pcm16", "pcmf", "results"))
    arena = guarded.Arena(specs, where="cuda", seed=5)
    for name, data in (("frames", frames), ("keystream", np.zeros(K.ROW_BYTES * S * T + 2, dtype=np.uint8)), ("offsets", offsets), ("state", state), ("rng", rng)):
        arena.load(name, data)
    p = arena.ptr
    assert (p("keystream") + 2) % 4 == 2
    outs = (p("pcm16"), p("pcmf"), p("results"), p("records"), strm)
    calls = {
        "mbx_apply_keystream": lambda: L.mbx_apply_keystream(codec, p("records"), S * T, p("keystream") + 2, strm),
        "mbx_process_batch_keyed": lambda: L.mbx_process_batch_keyed(codec, S, T, None, p("frames"), None, p("keystream") + 2, p("state"), None, p("rng"), *outs),
        "mbx_process_batch_ragged_keyed": lambda: L.mbx_process_batch_ragged_keyed(codec, None, S, p("offsets"), S * T, None, p("frames"), None, p("keystream") + 2,
                                                                                   p("state"), None, p("rng"), *outs),
    }
    for who, fn in calls.items():
        assert fn() == -1 and who.encode() in L.mbx_last_error() and b"mbx_keystream.h" in L.mbx_last_error(), (who, L.mbx_last_error())
    torch.cuda.synchronize()
    arena.check("misaligned keystream")
    for name in ("pcm16", "pcmf", "results", "records"):
        assert arena.read(name).tobytes() == arena.prefill_bytes(name).tobytes(), f"{name} was written by a refused call"
    assert arena.read("state").tobytes() == state.tobytes() and arena.read("rng").tobytes() == rng.tobytes()


for _codec in (0, 1):
    _case(f"keystream-apply-{_codec}", ["mbx_apply_keystream"], apply_stage, codec=_codec)
_case("keystream-batch-hard", ["mbx_process_batch_keyed"], batch, codec=0, S=257, T=1, soft=False, indexed=False, resident=False)
_case("keystream-batch-hard-ambe", ["mbx_process_batch_keyed"], batch, codec=1, S=5, T=3, soft=False, indexed=False, resident=False)
_case("keystream-batch-soft", ["mbx_process_batch_keyed"], batch, codec=2, S=9, T=2, soft=True, indexed=False, resident=False)
_case("keystream-batch-indexed-resident", ["mbx_process_batch_keyed"], batch, codec=0, S=3, T=5, soft=False, indexed=True, resident=True)
_case("keystream-batch-soft-indexed-resident", ["mbx_process_batch_keyed"], batch, codec=3, S=9, T=2, soft=True, indexed=True, resident=True)
for _skip in ("pcm16", "pcmf", "results"):
    _case(f"keystream-optional-batch-{_skip}", ["mbx_process_batch_keyed"], batch, codec=1, S=5, T=3, soft=False, indexed=True, resident=True, skip=_skip)
for _soft in (False, True):
    for _res in (False, True):
        _case(f"keystream-ragged-mixed-{'soft' if _soft else 'hard'}-{'resident' if _res else 'abi'}", ["mbx_process_batch_ragged_keyed"], ragged_mixed,
              soft=_soft, resident=_res)
for _skip in ("pcm16", "pcmf", "results"):
    _case(f"keystream-optional-ragged-{_skip}", ["mbx_process_batch_ragged_keyed"], ragged_mixed, soft=_skip == "pcmf", resident=True, skip=_skip)
_case("keystream-misaligned", ["mbx_apply_keystream", "mbx_process_batch_keyed", "mbx_process_batch_ragged_keyed"], misaligned)
BY_ID = {c.id: c for c in KEYSTREAM_CASES}
