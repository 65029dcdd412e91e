"""Burst groups (include/mbx_burst_groups.h): what the CPU and GPU suites share.  The four groups of the identity case, hard and soft
-- shapes chosen so that group boundaries fall inside a workgroup's 64 bursts and inside an output dword, one group is a single
burst and one fills a workgroup exactly --, the route over the existing calls that a groups call must equal byte for byte
(mbx_deinterleave[_soft] per group into mixed rows, host-made offsets, codecs and index, ONE mbx_process_batch[_soft]_mixed), and the
memory-contract cases in tests/guarded.py arenas (a list of their own, GROUP_CASES: burst_cases.CASES stays what
tests/test_bursts_host.py holds it to).  Importable without a GPU."""
import ctypes as C
from collections import namedtuple

import numpy as np

import guarded
import llr_burst_cases
import memory_cases
import symbol_burst_cases
from mbelib_neo_amd import bursts as B

POOL = 200
KEYS = ("records", "results", "pcm16", "pcmf")
# (codec, frames per burst, form, inversion sequence, streams, bursts per stream, extra bytes of burst_stride)
HARD = ((0, 2, B.FORM_PACKED, False, 65, 1, 0), (1, 3, B.FORM_DIBITS, True, 35, 2, 0), (3, 1, B.FORM_BITS, False, 1, 1, 0),
        (2, 1, B.FORM_PACKED, False, 64, 1, 3))
# the soft twin: per-bit cells with a sequence, dibit pairs, int16 LLRs, int8 LLRs
SOFT = ((0, 2, B.FORM_PACKED, True, 65, 1, 0), (1, 3, B.FORM_DIBITS, False, 35, 2, 0), (3, 1, B.FORM_LLR16, False, 1, 1, 0),
        (2, 1, B.FORM_LLR8, False, 64, 1, 0))
STREAMS, FRAMES = 165, 405
assert sum(g[4] for g in HARD) == STREAMS and sum(g[1] * g[4] * g[5] for g in HARD) == FRAMES
assert [g[:2] + g[4:6] for g in HARD] == [g[:2] + g[4:6] for g in SOFT]
# 65 streams, then 70 bursts: the second group starts at burst 65 of the call -- inside a workgroup's 64 -- and at frame row 130, byte
# 2,340 = 4 * 585 of the wire rows; the third at row 340, byte 6,120; the fourth at row 341, byte 6,138 = 4 * 1,534 + 2: inside a dword
assert (130 * 18) % 4 == 0 and (341 * 18) % 4 == 2


def slots_of_groups(shapes, seed=3, pool=POOL):
    """pool slots of every group's streams: the LAST group a run of consecutive slots (so that it can also be named by first_slot),
    the others a permutation of the rest"""
    last = shapes[-1][4]
    first_slot = 70
    rest = np.setdiff1d(np.arange(pool), np.arange(first_slot, first_slot + last))
    perm = np.random.default_rng(seed).permutation(rest)
    out, at = [], 0
    for g in shapes[:-1]:
        out.append(perm[at:at + g[4]].astype(np.int32))
        at += g[4]
    out.append(np.arange(first_slot, first_slot + last, dtype=np.int32))
    return out


def schedules(shapes, seed, device=True):
    """one schedule per group shape: 57 burst bits (an even number more for the dibit form) that no entry names"""
    rng = np.random.default_rng(seed)
    out = []
    for codec, F, form, masked, *_ in shapes:
        nbits = F * B.channel_bits(codec) + (58 if form == B.FORM_DIBITS else 57)
        mask = symbol_burst_cases.random_mask(rng, nbits) if masked else None
        out.append(B.random_schedule(codec, F, nbits, rng, device=device, form=form, invert=mask))
    return out


def group_bursts(s, shape, soft, rng, tag, junk=False):
    """the bursts of one group in its schedule's form, carrying the frames of tests/edge_mix.py / soft_mix.py: uint8, flat"""
    codec, F, form, _, n, per, pad = shape
    received = symbol_burst_cases.carried_bursts(s, codec, n * per, F, soft, rng, tag)
    if soft and form in B.LLR_DTYPE:
        return llr_burst_cases.llrs_carrying(received, 2 if form == B.FORM_LLR16 else 1).reshape(-1).view(np.uint8)
    bursts = B.to_form(s, received, soft=soft, junk=rng if junk else None)
    if not soft and pad:
        bursts = symbol_burst_cases.strided(bursts, s.burst_bytes + pad, rng)
    return np.ascontiguousarray(bursts).reshape(-1)


def make_groups(shapes, scheds, soft, seed, tag, slots=None, junk=False):
    """BurstGroups with HOST bursts and host slots"""
    rng = np.random.default_rng(seed)
    slots = slots_of_groups(shapes) if slots is None else slots
    return [B.BurstGroup(s, group_bursts(s, g, soft, rng, tag + i, junk), g[4], g[5], stream_index=idx, burst_stride=None if soft else s.burst_bytes + g[6])
            for i, (s, g, idx) in enumerate(zip(scheds, shapes, slots))]


def existing_route(dec, groups, soft):
    """What a groups call replaces, on `dec`'s pool: mbx_deinterleave[_soft] per group into mixed rows at the group's first row,
    host-made frame offsets, codecs and index, one mbx_process_batch[_soft]_mixed.  Returns (outputs, kernel name)."""
    import torch
    from mbelib_neo_amd import _native

    lay = B.apply_groups(groups, soft)
    total = int(lay["row_of_group"][-1])
    rows = torch.zeros((total, B.MIXED_ROW_CELLS, 2) if soft else (total, B.MIXED_ROW_BYTES), dtype=torch.uint8, device=dec.device)
    for g, first in zip(groups, lay["row_of_group"][:-1]):
        if g.n_streams:
            B.deinterleave(g.schedule, np.asarray(g.bursts), soft=soft, mixed_rows=True, burst_stride=None if soft else g.burst_stride,
                           out=rows[int(first):int(first) + g.frames])
    assert np.array_equal(rows.cpu().numpy(), lay["rows"]), "the gathers differ from the numpy definition (bursts.apply_groups)"
    counts = np.diff(lay["frame_offset"])
    d_index = torch.from_numpy(lay["stream_index"]).to(dec.device)
    out = dec.decode_ragged(rows.reshape(-1), counts, soft=soft, want_float=True, stream_index=d_index, codec=lay["stream_codec"])
    name = _native.lib().mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream)
    torch.cuda.synchronize()
    return out, (name or b"").decode()


def on_device(groups):
    """the same groups with their bursts as device tensors (the caller's to check: the decoder does not validate them)"""
    import torch

    return [B.BurstGroup(g.schedule, torch.from_numpy(np.ascontiguousarray(g.bursts).reshape(-1).copy()).cuda(), g.n_streams, g.bursts_per_stream,
                         stream_index=g.stream_index, first_slot=g.first_slot, burst_stride=g.burst_stride) for g in groups]


def pool_bytes(dec):
    return (dec.state.cpu().numpy().tobytes(), dec.rng.cpu().numpy().tobytes(), dec.resident.cpu().numpy().tobytes() if dec.resident is not None else b"")


# ---- memory-contract cases -------------------------------------------------------------------------------------------------------------
Case = namedtuple("Case", "id covers fn args")
GROUP_CASES = []


def _case(cid, covers, fn, **args):
    GROUP_CASES.append(Case(cid, tuple(covers), fn, args))


def launch(soft, resident, skip=None):
    """mbx_process_burst_groups with every buffer of the call -- each group's bursts and index, the pools, the outputs -- in ONE
    guarded arena: inputs read-only, nothing written outside the total_frames rows of each output, the call twice under two patterns
    with the same bytes; skip: an optional output that is NULL.  The first run's outputs and pools are those of the decoder route."""
    import torch
    from mbelib_neo_amd import decoder

    L, _native, strm = memory_cases._lib()
    shapes = SOFT if soft else HARD
    scheds = schedules(shapes, 21 + soft)
    groups = make_groups(shapes, scheds, soft, 23, tag=2, junk=True)
    state0, rng0 = memory_cases._initial(POOL, 11)
    want = [k for k in ("pcm16", "pcmf", "results") if k != skip]
    specs = [guarded.buf("state", state0.size, "state"), guarded.buf("rng", rng0.size, "rng")] + memory_cases._out_specs(FRAMES, want)
    inputs = {"state": state0, "rng": rng0}
    for i, g in enumerate(groups):
        # (soft bursts: 16-bit pieces; int8 LLRs and hard bursts: bytes)
        kind = "soft" if soft and g.schedule.form != B.FORM_LLR8 else "frames"
        specs += [guarded.buf(f"bursts{i}", g.bursts.size, kind, True), guarded.buf(f"index{i}", 4 * g.n_streams, "index", True)]
        inputs[f"bursts{i}"], inputs[f"index{i}"] = g.bursts, g.slots()
    if resident:
        specs.append(guarded.buf("resident", 4 * POOL, "resident"))
        inputs["resident"] = np.zeros(POOL, dtype=np.uint32)
    names = []

    def call(run):
        arr = B.group_structs(groups, [(run.p(f"bursts{i}"), run.p(f"index{i}")) for i in range(len(groups))])
        rc = L.mbx_process_burst_groups(arr, len(groups), int(soft), run.p("state"), run.p("resident"), run.p("rng"), run.p("pcm16"), run.p("pcmf"),
                                        run.p("results"), run.p("records"), strm)
        _native.check(rc, "mbx_process_burst_groups")
        names.append(L.mbx_last_kernel_name(strm).decode())

    got = memory_cases.twice(f"burst groups soft {soft} resident {resident} without {skip}", specs, inputs, call)
    assert names == ["mixed_stream_kernel_ragged" + ("_res" if resident else "")] * 2, names
    # the same call through the decoder, on plain torch allocations
    dec = decoder.BatchDecoder(0, POOL, resident=resident)
    dec.set_state(state0, rng0)
    out = dec.decode_burst_groups(on_device(groups), soft=soft, want_float=True)
    torch.cuda.synchronize()
    for k in want + ["records"]:
        assert np.array_equal(got[k], out[k].cpu().numpy().reshape(-1).view(np.uint8)), k
    assert got["state"].tobytes() == pool_bytes(dec)[0] and got["rng"].tobytes() == pool_bytes(dec)[1]
    if resident:
        assert got["resident"].tobytes() == pool_bytes(dec)[2]
    for s in scheds:
        s.close()


for _soft in (False, True):
    for _res in (True, False):
        _case(f"groups-{'soft' if _soft else 'hard'}-{'resident' if _res else 'abi'}", ["mbx_process_burst_groups"], launch, soft=_soft, resident=_res)
for _skip in ("pcm16", "pcmf", "results"):
    _case(f"groups-optional-hard-{_skip}", ["mbx_process_burst_groups"], launch, soft=False, resident=True, skip=_skip)
    _case(f"groups-optional-soft-{_skip}", ["mbx_process_burst_groups"], launch, soft=True, resident=False, skip=_skip)


def group_array(L, groups, host=True):
    """(ctypes array of mbx_burst_group, the arrays it points into) for groups with HOST bursts and indices: the session's form"""
    keep = [(np.ascontiguousarray(g.bursts).reshape(-1), None if g.stream_index is None else g.slots()) for g in groups]
    arr = B.group_structs(groups, [(b.ctypes.data if b.size else 0, None if i is None else i.ctypes.data) for b, i in keep])
    return arr, keep
