"""Burst input (include/mbx_burst.h): what the CPU and GPU suites share.  Schedules of a given shape, bursts that carry given
frames (the inverse of apply_schedule, with junk in the bits no entry names), and the memory-contract cases of the burst entry points
in tests/guarded.py arenas.  Importable without a GPU: CASES names, per case, the entry points it puts under guard
(tests/test_bursts_host.py demands one for every function of the header that takes a device pointer)."""
import ctypes as C
from collections import namedtuple

import numpy as np

import guarded
import memory_cases
from mbelib_neo_amd import bursts as B
from mbelib_neo_amd.layout import FRAME_BYTES, FRAME_CELLS

CELLS = {c: FRAME_CELLS[c][0] * FRAME_CELLS[c][1] for c in FRAME_CELLS}


def make_bursts(schedule, frames, rng, soft=False, burst_stride=None):
    """bursts that carry `frames` (hard: uint8 [n * F, frame bytes]; soft: uint8 [n * F, cells, 2]) under `schedule`, every other
    bit / cell / padding byte random (soft: hard decisions stay 0 / 1).  apply_schedule of the result gives the frames back (soft:
    with the cells that are not on the wire zero)."""
    s = schedule
    F, nb = s.frames_per_burst, s.burst_bits
    if soft:
        cells = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, F, CELLS[s.codec], 2)
        out = rng.integers(0, 256, size=(cells.shape[0], nb, 2), dtype=np.uint8)
        out[:, :, 0] &= 1
        stride = FRAME_CELLS[s.codec][1]
        for k in range(F):
            out[:, s.src_bit[k]] = cells[:, k, s.cell_row[k] * stride + s.cell_col[k]]
        return out
    stride = s.burst_bytes if burst_stride is None else burst_stride
    wire = np.unpackbits(np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, F, FRAME_BYTES[s.codec]), axis=2)
    raw = rng.integers(0, 256, size=(wire.shape[0], stride), dtype=np.uint8)
    bits = np.unpackbits(raw[:, :s.burst_bytes], axis=1)
    for k in range(F):
        bits[:, s.src_bit[k]] = wire[:, k, B.wire_bit_of_cell(s.codec, s.cell_row[k], s.cell_col[k])]
    raw[:, :s.burst_bytes] = np.packbits(bits, axis=1)
    return raw


def scatter_like_the_integration_guide(L, schedule, bursts):
    """the host route of INTEGRATION.md: mbx_wire_permutation per frame of the burst, then the per-bit loop"""
    s = schedule
    n = B.channel_bits(s.codec)
    raw = np.ascontiguousarray(bursts, dtype=np.uint8).reshape(-1, s.burst_bytes)
    out = np.zeros((raw.shape[0], s.frames_per_burst, FRAME_BYTES[s.codec]), dtype=np.uint8)
    for k in range(s.frames_per_burst):
        wire = np.zeros(n, dtype=np.int32)
        assert L.mbx_wire_permutation(s.codec, s.cell_row[k].ctypes.data, s.cell_col[k].ctypes.data, n, wire.ctypes.data) == 0
        for i in range(n):
            j = int(s.src_bit[k, i])
            bit = (raw[:, j >> 3] >> (7 - (j & 7))) & 1
            out[:, k, wire[i] >> 3] |= (bit << (7 - (wire[i] & 7))).astype(np.uint8)
    return out.reshape(-1, FRAME_BYTES[s.codec])


# ---- memory-contract cases -------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id covers fn args")
CASES = []


def _case(cid, covers, fn, **args):
    CASES.append(Case(cid, tuple(covers), fn, args))


def _schedule(codec, F, nbits, seed):
    return B.random_schedule(codec, F, nbits, np.random.default_rng(seed), device=True)


def gather(codec, soft, mixed_rows, n=97, F=3, nbits=601):
    """mbx_deinterleave / _soft between guard bands: input read-only, output at alignment 1 (hard) / 2 (soft) exactly; a mixed hard
    row of an AMBE codec keeps bytes 9..17"""
    import torch

    L, _native, strm = memory_cases._lib()
    s = _schedule(codec, F, nbits, 5 + codec)
    rng = np.random.default_rng(50 + codec)
    if soft:
        bursts = rng.integers(0, 256, size=(n, nbits, 2), dtype=np.uint8)
        bursts[:, :, 0] &= 1
        row = B.MIXED_ROW_CELLS if mixed_rows else CELLS[codec]
        specs = [guarded.buf("bursts", bursts.size, "soft", True), guarded.buf("rows", n * F * row * 2, "soft")]
        want = np.zeros((n * F, row, 2), dtype=np.uint8)
        want[:, :CELLS[codec]] = B.apply_schedule(s, bursts, soft=True)

        def call(run):
            _native.check(L.mbx_deinterleave_soft(s.handle, run.p("bursts"), n, run.p("rows"), row, strm), "mbx_deinterleave_soft")

        got = memory_cases.twice(f"deinterleave soft codec {codec}", specs, {"bursts": bursts}, call)
        assert np.array_equal(got["rows"].reshape(want.shape), want)
        return
    stride = s.burst_bytes + 3
    bursts = rng.integers(0, 256, size=(n, stride), dtype=np.uint8)
    row = B.MIXED_ROW_BYTES if mixed_rows else FRAME_BYTES[codec]
    specs = [guarded.buf("bursts", bursts.size, "frames", True), guarded.buf("rows", n * F * row, "frames")]
    want = B.apply_schedule(s, bursts, burst_stride=stride)
    fb = FRAME_BYTES[codec]

    def call(run):
        _native.check(L.mbx_deinterleave(s.handle, run.p("bursts"), stride, n, run.p("rows"), row, strm), "mbx_deinterleave")

    def after(run, got):
        rows = got["rows"].reshape(n * F, row)
        assert np.array_equal(rows[:, :fb], want), "gathered bytes"
        assert np.array_equal(rows[:, fb:], run.arena.prefill_bytes("rows").reshape(n * F, row)[:, fb:]), "bytes 9..17 of a mixed AMBE row are kept"

    memory_cases.twice(f"deinterleave codec {codec} rows of {row}", specs, {"bursts": bursts}, call, after=after, compare=row == fb)
    torch.cuda.synchronize()


def launch(codec, soft, F, S=70, pool=90, resident=True, indexed=True, skip=None, nbits=None):
    """mbx_process_bursts / _soft with every buffer in the arena; skip: an optional output that is NULL.  The first run's bytes equal
    the frames call on the host-built frames (plain torch buffers)."""
    import torch
    import edge_mix
    import soft_mix

    L, _native, strm = memory_cases._lib()
    nbits = nbits or F * B.channel_bits(codec) + 57
    s = _schedule(codec, F, nbits, 9 + codec + F)
    rng = np.random.default_rng(70 + codec)
    frames = soft_mix.frames(codec, S, F, tag=F) if soft else edge_mix.frames(codec, S, F, F).reshape(S * F, -1)
    stride = s.burst_bytes + 1
    bursts = make_bursts(s, frames, rng, soft=soft, burst_stride=stride)
    built = B.apply_schedule(s, bursts, soft=soft, burst_stride=stride)
    index = (rng.permutation(pool)[:S]).astype(np.int32) if indexed else None
    npool = pool if indexed else S
    state0, rng0 = memory_cases._initial(npool, 11)
    want = [k for k in ("pcm16", "pcmf", "results") if k != skip]
    specs = [guarded.buf("bursts", bursts.size, "soft" if soft else "frames", True), guarded.buf("state", state0.size, "state"),
             guarded.buf("rng", rng0.size, "rng")] + memory_cases._out_specs(S * F, want)
    inputs = {"bursts": bursts, "state": state0, "rng": rng0}
    if indexed:
        specs.append(guarded.buf("index", 4 * S, "index", True))
        inputs["index"] = index
    if resident:
        specs.append(guarded.buf("resident", 4 * npool, "resident"))
        inputs["resident"] = np.zeros(npool, dtype=np.uint32)

    def call(run):
        tail = (run.p("state"), run.p("resident"), run.p("rng"), run.p("pcm16"), run.p("pcmf"), run.p("results"), run.p("records"), strm)
        if soft:
            rc = L.mbx_process_bursts_soft(s.handle, S, run.p("index"), run.p("bursts"), *tail)
        else:
            rc = L.mbx_process_bursts(s.handle, S, run.p("index"), run.p("bursts"), stride, *tail)
        _native.check(rc, "mbx_process_bursts")

    got = memory_cases.twice(f"bursts codec {codec} soft {soft} F {F} without {skip}", specs, inputs, call)
    # the same step from the frames the host would have built, on plain allocations
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda() for k, v in inputs.items() if k != "bursts"}
    d_frames = torch.from_numpy(built.reshape(-1).copy()).cuda()
    outs = {k: torch.zeros(S * F * memory_cases.OUT_BYTES[k], dtype=torch.uint8, device="cuda") for k in want + ["records"]}
    ptr = lambda d, k: d[k].data_ptr() if k in d else None   # noqa: E731
    fn = L.mbx_process_batch_soft_resident if soft else L.mbx_process_batch_resident
    if not soft and not resident:
        if indexed:
            rc = L.mbx_process_batch_indexed(codec, S, F, ptr(dev, "index"), d_frames.data_ptr(), dev["state"].data_ptr(), dev["rng"].data_ptr(),
                                             ptr(outs, "pcm16"), ptr(outs, "pcmf"), ptr(outs, "results"), outs["records"].data_ptr(), strm)
        else:
            rc = L.mbx_process_batch(codec, S, F, d_frames.data_ptr(), dev["state"].data_ptr(), dev["rng"].data_ptr(), ptr(outs, "pcm16"),
                                     ptr(outs, "pcmf"), ptr(outs, "results"), outs["records"].data_ptr(), strm)
    else:
        rc = fn(codec, S, F, ptr(dev, "index"), d_frames.data_ptr(), dev["state"].data_ptr(), ptr(dev, "resident"), dev["rng"].data_ptr(),
                ptr(outs, "pcm16"), ptr(outs, "pcmf"), ptr(outs, "results"), outs["records"].data_ptr(), strm)
    _native.check(rc, "frames call")
    torch.cuda.synchronize()
    for k, v in {**outs, **{k: dev[k] for k in ("state", "rng", "resident") if k in dev}}.items():
        assert np.array_equal(got[k], v.cpu().numpy()), f"{k}: the burst launch and the frames call differ"


for _codec in (0, 1, 2, 3):
    _case(f"gather-hard-{_codec}", ["mbx_deinterleave"], gather, codec=_codec, soft=False, mixed_rows=False)
    _case(f"gather-soft-{_codec}", ["mbx_deinterleave_soft"], gather, codec=_codec, soft=True, mixed_rows=False)
    _case(f"gather-hard-mixed-rows-{_codec}", ["mbx_deinterleave"], gather, codec=_codec, soft=False, mixed_rows=True)
    _case(f"gather-soft-mixed-rows-{_codec}", ["mbx_deinterleave_soft"], gather, codec=_codec, soft=True, mixed_rows=True)
    for _F in (1, 3):
        _case(f"launch-hard-{_codec}-F{_F}", ["mbx_process_bursts"], launch, codec=_codec, soft=False, F=_F)
        _case(f"launch-soft-{_codec}-F{_F}", ["mbx_process_bursts_soft"], launch, codec=_codec, soft=True, F=_F)
for _skip in ("pcm16", "pcmf", "results"):
    _case(f"optional-hard-{_skip}", ["mbx_process_bursts"], launch, codec=1, soft=False, F=3, skip=_skip)
    _case(f"optional-soft-{_skip}", ["mbx_process_bursts_soft"], launch, codec=0, soft=True, F=1, skip=_skip)
_case("launch-hard-abi-identity", ["mbx_process_bursts"], launch, codec=0, soft=False, F=9, resident=False, indexed=False)
_case("launch-hard-abi-indexed", ["mbx_process_bursts"], launch, codec=3, soft=False, F=3, resident=False, indexed=True)
_case("launch-soft-abi-identity", ["mbx_process_bursts_soft"], launch, codec=2, soft=True, F=3, resident=False, indexed=False)
