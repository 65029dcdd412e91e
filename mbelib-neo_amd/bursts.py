"""Burst input (include/mbx_burst.h): a caller's de-interleave schedule applied on the device.

A received air-interface burst carries F frames of one stream, their channel bits interleaved with each other and with bits that
are not voice at all.  The caller states ONCE where every channel bit sits -- for frame k and its i-th channel bit: received bit
``src_bit[k, i]`` of the burst goes to cell ``[cell_row[k, i]][cell_col[k, i]]`` of that frame's imbe_fr / ambe_fr array -- and the
library applies that to every burst: ``deinterleave`` (the gather alone), ``BatchDecoder.decode_bursts`` (gather + decode).

A schedule also says in which FORM the receiver holds its bursts (FORM_PACKED: 8 bits per byte, MSB first; FORM_BITS: one byte per
bit; FORM_DIBITS: one byte per dibit, and for soft input one {dibit, reliability} pair per dibit) and, optionally, which received
bits arrive inverted (``invert``: a fixed descrambling sequence, one 0 / 1 per received bit).  ``src_bit`` counts received BITS in
every form.  ``to_form`` turns packed bursts into the form of a schedule.

FORM_LLR16 / FORM_LLR8 are SOFT-ONLY forms: one signed log-likelihood ratio per received bit, int16 or int8, as a soft demodulator
emits them; the gather converts them (``cells_from_llr`` is the conversion in numpy) and the hard calls refuse such a schedule.

``apply_schedule`` is the same thing in numpy, on the host: the definition, and what the tests expect of the kernels.  No
air-interface table of any standard is written here; ``random_schedule`` and ``gap_schedule`` make schedules of a given SHAPE.

``BurstGroup`` (include/mbx_burst_groups.h) is the bursts of ONE schedule in one tick -- n_streams streams with bursts_per_stream
consecutive bursts each, every stream named by a pool slot; ``BatchDecoder.decode_burst_groups`` decodes up to MAX_GROUPS of them in
one call, and ``apply_groups`` is its numpy definition: the mixed rows, offsets, codecs and index that one mixed ragged step takes.
"""
import ctypes as C

import numpy as np

from . import _native
from .layout import FRAME_BYTES, FRAME_CELLS, ROW_WIDTHS

MAX_FRAMES, MAX_BITS = 18, 4096          # MBX_BURST_MAX_FRAMES, MBX_BURST_MAX_BITS
MIXED_ROW_BYTES, MIXED_ROW_CELLS = 18, 184
MAX_GROUPS = 8                           # MBX_BURST_MAX_GROUPS (include/mbx_burst_groups.h)
FORM_PACKED, FORM_BITS, FORM_DIBITS = 0, 1, 2   # MBX_BURST_FORM_*
FORM_LLR16, FORM_LLR8 = 16, 8                   # MBX_BURST_FORM_LLR*: soft bursts of one int16 / int8 LLR per received bit
LLR_DTYPE = {FORM_LLR16: np.int16, FORM_LLR8: np.int8}


def channel_bits(codec):
    """channel bits of one frame: 144 / 72 / 142 / 72"""
    return int(sum(ROW_WIDTHS[codec]))


def wire_bit_of_cell(codec, row, col):
    """numpy form of mbx_wire_bit_of_cell: where cell [row][col] sits in the packed wire frame (arrays in, array out; the cells
    must be on the wire)"""
    widths = np.asarray(ROW_WIDTHS[codec])
    start = np.concatenate(([0], np.cumsum(widths)[:-1]))
    row, col = np.asarray(row), np.asarray(col)
    return start[row] + widths[row] - 1 - col


def cells_from_llr(llr):
    """numpy form of the conversion (mbx_soft_bits_from_llr, and what the LLR gathers and mbx_soft_from_llr do on the device):
    integer LLRs [...] -> uint8 [..., 2] cells, bit = v > 0, reliability = min(|v|, 255) with |v| taken in a wider type"""
    v = np.asarray(llr).astype(np.int32)
    return np.stack([v > 0, np.minimum(np.abs(v), 255)], axis=-1).astype(np.uint8)


def llr_from_cells(cells, form=FORM_LLR16):
    """per-bit cells uint8 [..., 2] -> the LLRs of the form's type that convert to exactly them: +-reliability.  ValueError for a
    cell no LLR gives: {1, 0}, and for int8 a reliability above 127 ({1, .}) / 128 ({0, .})"""
    c = np.asarray(cells, dtype=np.uint8)
    bit, rel = c[..., 0].astype(np.int32), c[..., 1].astype(np.int32)
    v = np.where(bit & 1, rel, -rel)
    info = np.iinfo(LLR_DTYPE[form])
    if ((bit > 1) | ((bit == 1) & (rel == 0)) | (v < info.min) | (v > info.max)).any():
        raise ValueError("a cell that no LLR of this width converts to")
    return v.astype(LLR_DTYPE[form])


def as_bytes(schedule, bursts, soft=False):
    """bursts (host array or device tensor) as the uint8 bytes the library reads: soft bursts of an LLR schedule may come as int16 /
    int8 (any integer array is cast to the form's type; a uint8 one is taken as the bytes themselves), everything else is uint8"""
    dtype = LLR_DTYPE.get(schedule.form) if soft else None
    if isinstance(bursts, np.ndarray):
        if dtype is not None and bursts.dtype != np.uint8:
            return np.ascontiguousarray(bursts, dtype=dtype).reshape(-1).view(np.uint8)
        return np.ascontiguousarray(bursts, dtype=np.uint8)
    import torch

    if dtype is not None and bursts.dtype == {np.int16: torch.int16, np.int8: torch.int8}[dtype] and bursts.is_contiguous():
        return bursts.reshape(-1).view(torch.uint8)
    return bursts


class ScheduleArrays:
    """The three integer arrays of a schedule, [frames_per_burst, channel_bits(codec)] each, on the host, the form of its bursts and
    its inversion sequence (None, or burst_bits values of 0 / 1).  Checks shapes only: whether the schedule is a valid one is the
    library's to say (mbx_burst_schedule_create_form)."""

    def __init__(self, codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col, form=FORM_PACKED, invert=None):
        self.codec, self.frames_per_burst, self.burst_bits = int(codec), int(frames_per_burst), int(burst_bits)
        if self.codec not in FRAME_BYTES:
            raise ValueError("no such codec")
        shape = (self.frames_per_burst, channel_bits(self.codec))
        self.src_bit, self.cell_row, self.cell_col = (np.ascontiguousarray(a, dtype=np.int32).reshape(shape) for a in (src_bit, cell_row, cell_col))
        self.form = int(form)
        self.invert = None if invert is None else np.ascontiguousarray(invert, dtype=np.uint8).reshape(self.burst_bits)

    @property
    def packed_bytes(self):
        """bytes of one hard burst in the packed form, whatever the schedule's own"""
        return (self.burst_bits + 7) // 8

    @property
    def burst_bytes(self):
        """the smallest burst_stride of a hard burst in the schedule's form (mbx_burst_schedule_bytes)"""
        return {FORM_BITS: self.burst_bits, FORM_DIBITS: self.burst_bits // 2, FORM_LLR16: 0, FORM_LLR8: 0}.get(self.form, self.packed_bytes)

    @property
    def soft_cells(self):
        """mbe_soft_bit-sized cells of one soft burst (mbx_burst_schedule_soft_cells); LLR8: 0, its bursts need not be whole cells"""
        return {FORM_DIBITS: self.burst_bits // 2, FORM_LLR8: 0}.get(self.form, self.burst_bits)

    @property
    def soft_bytes(self):
        """bytes of one soft burst (mbx_burst_schedule_soft_bytes)"""
        return self.burst_bits if self.form == FORM_LLR8 else 2 * self.soft_cells

    def in_form(self, form=FORM_PACKED, invert=None, device=False):
        """the same three arrays as a schedule of another form / inversion sequence"""
        return (BurstSchedule if device else ScheduleArrays)(self.codec, self.frames_per_burst, self.burst_bits, self.src_bit, self.cell_row,
                                                            self.cell_col, form, invert)


class BurstSchedule(ScheduleArrays):
    """A schedule on the device (mbx_burst_schedule_create_form, for an LLR form mbx_burst_schedule_create_llr, on the current
    device, which must have been initialised: decoder.ensure_init).  Owns the native handle; immutable."""

    def __init__(self, codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col, form=FORM_PACKED, invert=None):
        super().__init__(codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col, form, invert)
        self.handle = None
        h = C.c_void_p()
        L = _native.lib()
        create, form = (L.mbx_burst_schedule_create_llr, self.form // 8) if self.form in LLR_DTYPE else (L.mbx_burst_schedule_create_form, self.form)
        rc = create(C.byref(h), self.codec, self.frames_per_burst, self.burst_bits, self.src_bit.ctypes.data, self.cell_row.ctypes.data,
                    self.cell_col.ctypes.data, form, None if self.invert is None else self.invert.ctypes.data)
        _native.check(rc, "mbx_burst_schedule_create_llr" if self.form in LLR_DTYPE else "mbx_burst_schedule_create_form")
        self.handle = h

    def close(self):
        if self.handle is not None:
            _native.lib().mbx_burst_schedule_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:   # interpreter shutdown
            pass


def _received_bits(s, raw):
    """[n, burst_bits] 0 / 1 of hard bursts [n, >= burst_bytes] in the schedule's form, as the device reads them"""
    if s.form == FORM_BITS:
        return raw[:, :s.burst_bits] & 1
    if s.form == FORM_DIBITS:
        d = raw[:, :s.burst_bits // 2]
        return np.stack([(d >> 1) & 1, d & 1], axis=-1).reshape(raw.shape[0], -1)
    return np.unpackbits(raw[:, :s.packed_bytes], axis=1)[:, :s.burst_bits]


def apply_schedule(schedule, bursts, soft=False, burst_stride=None):
    """What the gather kernels do, in numpy.  schedule: ScheduleArrays (or BurstSchedule).
    hard: bursts = uint8, n bursts of burst_stride bytes (default schedule.burst_bytes) in the schedule's form -- PACKED: bit j at
          byte j >> 3, mask 0x80 >> (j & 7); BITS: bit j = byte j & 1; DIBITS: bits 2d, 2d + 1 = bits 1, 0 of byte d
          -> uint8 [n * F, FRAME_BYTES[codec]] packed wire frames, frame k of burst b at row b * F + k
    soft: bursts = uint8 [n, soft_cells, 2] -- (bit, reliability) per bit, DIBITS: (dibit, reliability) per dibit, both bits of the
          dibit with its reliability; LLR16 / LLR8: [n, burst_bits] int16 / int8 (or their bytes as uint8), converted by
          cells_from_llr first -> uint8 [n * F, cells, 2] cell arrays in the reference's shape, cells that are not on the wire {0, 0}
    schedule.invert: the received bits with a 1 are flipped (soft: the hard decision; the reliability stays)"""
    s = schedule
    F, B, nbits = s.frames_per_burst, s.burst_bits, channel_bits(s.codec)
    rows, stride = FRAME_CELLS[s.codec]
    if s.form in LLR_DTYPE and not soft:
        raise ValueError("an LLR schedule has soft bursts only")
    if soft:
        if s.form in LLR_DTYPE:
            cells = cells_from_llr(as_bytes(s, np.asarray(bursts), True).view(LLR_DTYPE[s.form]).reshape(-1, B))
        else:
            cells = np.ascontiguousarray(bursts, dtype=np.uint8).reshape(-1, s.soft_cells, 2)
        if s.form == FORM_DIBITS:
            d, rel = cells[:, :, 0], cells[:, :, 1]
            cells = np.stack([np.stack([(d >> 1) & 1, d & 1], axis=-1).reshape(-1, B), np.repeat(rel, 2, axis=1)], axis=-1)
        if s.invert is not None:
            cells = cells.copy()
            cells[:, :, 0] ^= s.invert
        out = np.zeros((cells.shape[0], F, rows * stride, 2), dtype=np.uint8)
        for k in range(F):
            out[:, k, s.cell_row[k] * stride + s.cell_col[k]] = cells[:, s.src_bit[k]]
        return out.reshape(-1, rows * stride, 2)
    burst_stride = s.burst_bytes if burst_stride is None else int(burst_stride)
    raw = np.ascontiguousarray(bursts, dtype=np.uint8).reshape(-1, burst_stride)[:, :s.burst_bytes]
    bits = _received_bits(s, raw)
    if s.invert is not None:
        bits = bits ^ s.invert
    out = np.zeros((raw.shape[0], F, FRAME_BYTES[s.codec] * 8), dtype=np.uint8)
    for k in range(F):
        out[:, k, wire_bit_of_cell(s.codec, s.cell_row[k], s.cell_col[k])] = bits[:, s.src_bit[k]]
    assert nbits <= out.shape[2]
    return np.packbits(out, axis=2).reshape(-1, FRAME_BYTES[s.codec])


def to_form(schedule, packed_bursts, soft=False, junk=None):
    """Bursts in the packed form -> the same received bits in the schedule's form, at the tight stride.
    hard: packed_bursts = uint8 [n, >= ceil(burst_bits / 8)], MSB first -> uint8 [n, schedule.burst_bytes]
    soft: packed_bursts = uint8 [n, burst_bits, 2] (bit, reliability) per bit -> uint8 [n, schedule.soft_cells, 2]; for the dibit form
          the two bits of a dibit must come with ONE reliability (ValueError otherwise); LLR16 / LLR8: int16 / int8 [n, burst_bits],
          the LLRs +-reliability that convert to exactly these cells (llr_from_cells: ValueError for a cell no LLR gives)
    junk: an rng (numpy Generator) that fills the bits of every byte which the DEVICE does not read -- bits 1..7 of a bit byte, bits
          2..7 of a dibit byte or dibit cell, the bits of the last packed byte behind burst_bits.  Such bursts are what the device
          calls mask; mbx_burst_validate and the session submits refuse them.
    The inversion sequence plays no part: it says how the bits ARRIVE."""
    s = schedule
    B = s.burst_bits
    if soft:
        cells = np.ascontiguousarray(packed_bursts, dtype=np.uint8).reshape(-1, B, 2)
        if s.form in LLR_DTYPE:
            return llr_from_cells(cells, s.form)
        if s.form != FORM_DIBITS:
            return cells.copy()
        pairs = cells.reshape(-1, B // 2, 2, 2)
        if not np.array_equal(pairs[:, :, 0, 1], pairs[:, :, 1, 1]):
            raise ValueError("soft dibits: the two bits of a dibit must have one reliability")
        d = ((pairs[:, :, 0, 0] & 1) << 1) | (pairs[:, :, 1, 0] & 1)
        if junk is not None:
            d = d | (junk.integers(0, 64, size=d.shape, dtype=np.uint8) << 2)
        return np.stack([d, pairs[:, :, 0, 1]], axis=-1)
    if s.form in LLR_DTYPE:
        raise ValueError("an LLR schedule has soft bursts only")
    raw = np.ascontiguousarray(packed_bursts, dtype=np.uint8)
    raw = raw.reshape(-1, s.packed_bytes) if raw.ndim != 2 else raw[:, :s.packed_bytes]
    bits = np.unpackbits(raw, axis=1)
    if s.form == FORM_BITS:
        out = bits[:, :B].copy()
        if junk is not None:
            out |= junk.integers(0, 128, size=out.shape, dtype=np.uint8) << 1
        return out
    if s.form == FORM_DIBITS:
        out = (bits[:, 0:B:2] << 1) | bits[:, 1:B:2]
        if junk is not None:
            out |= junk.integers(0, 64, size=out.shape, dtype=np.uint8) << 2
        return out
    if junk is not None:
        bits[:, B:] = junk.integers(0, 2, size=bits[:, B:].shape, dtype=np.uint8)
    else:
        bits[:, B:] = 0
    return np.packbits(bits, axis=1)


def _wire_cells(codec):
    """(row, col) of every wire cell, in wire order"""
    rows = np.concatenate([np.full(w, r) for r, w in enumerate(ROW_WIDTHS[codec])])
    cols = np.concatenate([np.arange(w - 1, -1, -1) for w in ROW_WIDTHS[codec]])
    return rows, cols


def random_schedule(codec, frames_per_burst, burst_bits, rng, device=False, form=FORM_PACKED, invert=None):
    """A random valid schedule of the given shape: the channel bits of the F frames at random distinct places of the burst, the
    cells of each frame in random order.  device=True: a BurstSchedule."""
    nbits = channel_bits(codec)
    src = rng.permutation(burst_bits)[:frames_per_burst * nbits].reshape(frames_per_burst, nbits)
    rows, cols = _wire_cells(codec)
    order = np.stack([rng.permutation(nbits) for _ in range(frames_per_burst)])
    return (BurstSchedule if device else ScheduleArrays)(codec, frames_per_burst, burst_bits, src, rows[order], cols[order], form, invert)


def gap_schedule(codec, frames_per_burst, gap=48, device=False):
    """The schedule a person can follow: `gap` bits that are not voice, then the F frames back to back, the bits of each frame in
    row-major cell order (row 0 cell 0, row 0 cell 1, ...)."""
    nbits = channel_bits(codec)
    rows = np.concatenate([np.full(w, r) for r, w in enumerate(ROW_WIDTHS[codec])])
    cols = np.concatenate([np.arange(w) for w in ROW_WIDTHS[codec]])
    src = gap + np.arange(frames_per_burst * nbits).reshape(frames_per_burst, nbits)
    tile = (frames_per_burst, 1)
    return (BurstSchedule if device else ScheduleArrays)(codec, frames_per_burst, gap + frames_per_burst * nbits, src, np.tile(rows, tile), np.tile(cols, tile))


def deinterleave(schedule, bursts, soft=False, mixed_rows=False, burst_stride=None, out=None):
    """The gather alone, on the device (mbx_deinterleave / mbx_deinterleave_soft on the current torch stream).  bursts: uint8 device
    tensor (or host array, uploaded) of n bursts in the schedule's form -- hard: burst_stride bytes each (default
    schedule.burst_bytes); soft: [n, schedule.soft_cells, 2], of an LLR schedule [n, burst_bits] int16 / int8 (array or tensor, or their
    bytes as uint8).  Returns uint8 [n * F, row] wire frames (soft: [n * F, row, 2] cells); mixed_rows=True: rows of
    MIXED_ROW_BYTES bytes / MIXED_ROW_CELLS cells, as mbx_process_batch_mixed takes them (bytes 9..17 of an AMBE wire row are not
    written: zero in a tensor made here, kept in `out`)."""
    import torch

    s = schedule
    bursts = as_bytes(s, bursts, soft)
    if isinstance(bursts, np.ndarray):
        bursts = torch.from_numpy(bursts.reshape(-1)).cuda()
    if bursts.dtype != torch.uint8 or not bursts.is_contiguous():
        raise ValueError("bursts must be a contiguous uint8 tensor")
    per = s.soft_bytes if soft else (s.burst_bytes if burst_stride is None else int(burst_stride))
    if per < 1 or bursts.numel() % per:
        raise ValueError("bursts must hold whole bursts")
    n = bursts.numel() // per
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    if soft:
        row = MIXED_ROW_CELLS if mixed_rows else FRAME_CELLS[s.codec][0] * FRAME_CELLS[s.codec][1]
        if out is None:
            out = torch.empty((n * s.frames_per_burst, row, 2), dtype=torch.uint8, device=bursts.device)
        _native.check(L.mbx_deinterleave_soft(s.handle, bursts.data_ptr(), n, out.data_ptr(), row, strm), "mbx_deinterleave_soft")
    else:
        row = MIXED_ROW_BYTES if mixed_rows else FRAME_BYTES[s.codec]
        if out is None:
            out = torch.zeros((n * s.frames_per_burst, row), dtype=torch.uint8, device=bursts.device)
        _native.check(L.mbx_deinterleave(s.handle, bursts.data_ptr(), per, n, out.data_ptr(), row, strm), "mbx_deinterleave")
    return out


class BurstGroup:
    """The bursts of ONE schedule in one tick (mbx_burst_group): n_streams streams x bursts_per_stream consecutive bursts, stream-major.
    bursts: uint8 array or device tensor in the schedule's form -- hard: burst_stride bytes each (default schedule.burst_bytes); soft:
    dense, schedule.soft_bytes each (LLRs may come as int16 / int8).  stream_index: the pool slot of each stream (sequence, int32
    array or int32 device tensor); None: slots first_slot .. first_slot + n_streams - 1."""

    def __init__(self, schedule, bursts, n_streams, bursts_per_stream=1, stream_index=None, first_slot=0, burst_stride=None):
        self.schedule, self.bursts = schedule, bursts
        self.n_streams, self.bursts_per_stream, self.first_slot = int(n_streams), int(bursts_per_stream), int(first_slot)
        self.stream_index = stream_index
        self.burst_stride = schedule.burst_bytes if burst_stride is None else int(burst_stride)

    @property
    def n_bursts(self):
        return self.n_streams * self.bursts_per_stream

    @property
    def frames(self):
        return self.n_bursts * self.schedule.frames_per_burst

    def slots(self):
        """the pool slots of the group's streams, int32 on the host"""
        if self.stream_index is None:
            return np.arange(self.first_slot, self.first_slot + self.n_streams, dtype=np.int32)
        idx = self.stream_index
        if not isinstance(idx, (np.ndarray, list, tuple, range)):
            idx = idx.cpu().numpy()
        return np.ascontiguousarray(idx, dtype=np.int32).reshape(-1)


def group_rows(groups):
    """first frame row of every group and the total behind them (mbx_burst_groups_rows): int32 [len(groups) + 1]"""
    rows = np.zeros(len(groups) + 1, dtype=np.int64)
    np.cumsum([g.frames for g in groups], out=rows[1:])
    if rows[-1] > 0x7FFFFFFF:
        raise ValueError("more than 2^31-1 frames in one call")
    return rows.astype(np.int32)


def apply_groups(groups, soft=False):
    """What one burst-groups call decodes, in numpy: the numpy gather (apply_schedule) of every group into mixed rows, group after
    group, and the layout of the ONE mixed ragged step over them.  groups: BurstGroups with HOST bursts.  Returns a dict:
      rows          uint8 [total, MIXED_ROW_BYTES] wire rows (bytes behind an AMBE frame zero); soft: [total, MIXED_ROW_CELLS, 2]
      frame_offset  int32 [S + 1]: stream row s owns rows frame_offset[s] .. frame_offset[s + 1] - 1, bursts_per_stream * F of them
      stream_codec  uint8 [S]: the codec of the stream's group's schedule
      stream_index  int32 [S]: its pool slot
      row_of_group  int32 [len(groups) + 1]"""
    if len(groups) > MAX_GROUPS:
        raise ValueError("at most MAX_GROUPS groups in one call")
    row_of_group = group_rows(groups)
    total = int(row_of_group[-1])
    rows = np.zeros((total, MIXED_ROW_CELLS, 2) if soft else (total, MIXED_ROW_BYTES), dtype=np.uint8)
    counts, codecs, index = [], [], []
    for g, first in zip(groups, row_of_group[:-1]):
        s = g.schedule
        if g.n_streams < 0 or g.bursts_per_stream < 1:
            raise ValueError("a group has n_streams >= 0 streams of bursts_per_stream >= 1 bursts")
        slots = g.slots()
        if slots.size != g.n_streams:
            raise ValueError("stream_index must hold one slot per stream of the group")
        if g.n_streams:
            raw = as_bytes(s, np.asarray(g.bursts), soft).reshape(-1)[:g.n_bursts * (s.soft_bytes if soft else g.burst_stride)]
            got = apply_schedule(s, raw, soft=True) if soft else apply_schedule(s, raw, burst_stride=g.burst_stride)
            rows[first:first + g.frames, :got.shape[1]] = got
        counts += [g.bursts_per_stream * s.frames_per_burst] * g.n_streams
        codecs += [s.codec] * g.n_streams
        index.append(slots)
    frame_offset = np.zeros(len(counts) + 1, dtype=np.int32)
    np.cumsum(counts, out=frame_offset[1:])
    return {"rows": rows, "frame_offset": frame_offset, "stream_codec": np.asarray(codecs, dtype=np.uint8),
            "stream_index": np.concatenate(index).astype(np.int32) if index else np.zeros(0, dtype=np.int32), "row_of_group": row_of_group}


def group_structs(groups, pointers):
    """the ctypes array of mbx_burst_group for `groups`; pointers: one (bursts, stream_index) address pair per group (0 / None: NULL)"""
    arr = (_native.BurstGroupStruct * max(len(groups), 1))()
    for a, g, (bursts, index) in zip(arr, groups, pointers):
        a.sched, a.bursts, a.burst_stride = g.schedule.handle, bursts or None, g.burst_stride
        a.n_streams, a.bursts_per_stream, a.stream_index, a.first_slot = g.n_streams, g.bursts_per_stream, index or None, g.first_slot
    return arr
