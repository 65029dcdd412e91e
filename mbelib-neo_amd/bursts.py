"""Burst input (include/mbx_burst.h): a caller's de-interleave schedule applied on the device.

A received air-interface burst carries F frames of one stream, their channel bits interleaved with each other and with bits that
are not voice at all.  The caller states ONCE where every channel bit sits -- for frame k and its i-th channel bit: received bit
``src_bit[k, i]`` of the burst goes to cell ``[cell_row[k, i]][cell_col[k, i]]`` of that frame's imbe_fr / ambe_fr array -- and the
library applies that to every burst: ``deinterleave`` (the gather alone), ``BatchDecoder.decode_bursts`` (gather + decode).

``apply_schedule`` is the same thing in numpy, on the host: the definition, and what the tests expect of the kernels.  No
air-interface table of any standard is written here; ``random_schedule`` and ``gap_schedule`` make schedules of a given SHAPE.
"""
import ctypes as C

import numpy as np

from . import _native
from .layout import FRAME_BYTES, FRAME_CELLS, ROW_WIDTHS

MAX_FRAMES, MAX_BITS = 18, 4096          # MBX_BURST_MAX_FRAMES, MBX_BURST_MAX_BITS
MIXED_ROW_BYTES, MIXED_ROW_CELLS = 18, 184


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


class ScheduleArrays:
    """The three integer arrays of a schedule, [frames_per_burst, channel_bits(codec)] each, on the host.  Checks shapes only: whether
    the schedule is a valid one is the library's to say (mbx_burst_schedule_create)."""

    def __init__(self, codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col):
        self.codec, self.frames_per_burst, self.burst_bits = int(codec), int(frames_per_burst), int(burst_bits)
        if self.codec not in FRAME_BYTES:
            raise ValueError("no such codec")
        shape = (self.frames_per_burst, channel_bits(self.codec))
        self.src_bit, self.cell_row, self.cell_col = (np.ascontiguousarray(a, dtype=np.int32).reshape(shape) for a in (src_bit, cell_row, cell_col))

    @property
    def burst_bytes(self):
        return (self.burst_bits + 7) // 8


class BurstSchedule(ScheduleArrays):
    """A schedule on the device (mbx_burst_schedule_create on the current device, which must have been initialised:
    decoder.ensure_init).  Owns the native handle; immutable."""

    def __init__(self, codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col):
        super().__init__(codec, frames_per_burst, burst_bits, src_bit, cell_row, cell_col)
        self.handle = None
        h = C.c_void_p()
        rc = _native.lib().mbx_burst_schedule_create(C.byref(h), self.codec, self.frames_per_burst, self.burst_bits, self.src_bit.ctypes.data,
                                                     self.cell_row.ctypes.data, self.cell_col.ctypes.data)
        _native.check(rc, "mbx_burst_schedule_create")
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


def apply_schedule(schedule, bursts, soft=False, burst_stride=None):
    """What the gather kernels do, in numpy.  schedule: ScheduleArrays (or BurstSchedule).
    hard: bursts = uint8, n bursts of burst_stride bytes (default ceil(burst_bits / 8)), bit j at byte j >> 3, mask 0x80 >> (j & 7)
          -> uint8 [n * F, FRAME_BYTES[codec]] packed wire frames, frame k of burst b at row b * F + k
    soft: bursts = uint8 [n, burst_bits, 2] (bit, reliability) -> uint8 [n * F, cells, 2] cell arrays in the reference's shape,
          cells that are not on the wire {0, 0}"""
    s = schedule
    F, B, nbits = s.frames_per_burst, s.burst_bits, channel_bits(s.codec)
    rows, stride = FRAME_CELLS[s.codec]
    if soft:
        cells = np.ascontiguousarray(bursts, dtype=np.uint8).reshape(-1, B, 2)
        out = np.zeros((cells.shape[0], F, rows * stride, 2), dtype=np.uint8)
        for k in range(F):
            out[:, k, s.cell_row[k] * stride + s.cell_col[k]] = cells[:, s.src_bit[k]]
        return out.reshape(-1, rows * stride, 2)
    burst_stride = s.burst_bytes if burst_stride is None else int(burst_stride)
    raw = np.ascontiguousarray(bursts, dtype=np.uint8).reshape(-1, burst_stride)[:, :s.burst_bytes]
    bits = np.unpackbits(raw, axis=1)[:, :B]
    out = np.zeros((raw.shape[0], F, FRAME_BYTES[s.codec] * 8), dtype=np.uint8)
    for k in range(F):
        out[:, k, wire_bit_of_cell(s.codec, s.cell_row[k], s.cell_col[k])] = bits[:, s.src_bit[k]]
    assert nbits <= out.shape[2]
    return np.packbits(out, axis=2).reshape(-1, FRAME_BYTES[s.codec])


def _wire_cells(codec):
    """(row, col) of every wire cell, in wire order"""
    rows = np.concatenate([np.full(w, r) for r, w in enumerate(ROW_WIDTHS[codec])])
    cols = np.concatenate([np.arange(w - 1, -1, -1) for w in ROW_WIDTHS[codec]])
    return rows, cols


def random_schedule(codec, frames_per_burst, burst_bits, rng, device=False):
    """A random valid schedule of the given shape: the channel bits of the F frames at random distinct places of the burst, the
    cells of each frame in random order.  device=True: a BurstSchedule."""
    nbits = channel_bits(codec)
    src = rng.permutation(burst_bits)[:frames_per_burst * nbits].reshape(frames_per_burst, nbits)
    rows, cols = _wire_cells(codec)
    order = np.stack([rng.permutation(nbits) for _ in range(frames_per_burst)])
    return (BurstSchedule if device else ScheduleArrays)(codec, frames_per_burst, burst_bits, src, rows[order], cols[order])


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
    tensor (or host array, uploaded) of n bursts -- hard: burst_stride bytes each (default ceil(burst_bits / 8)); soft:
    [n, burst_bits, 2].  Returns uint8 [n * F, row] wire frames (soft: [n * F, row, 2] cells); mixed_rows=True: rows of
    MIXED_ROW_BYTES bytes / MIXED_ROW_CELLS cells, as mbx_process_batch_mixed takes them (bytes 9..17 of an AMBE wire row are not
    written: zero in a tensor made here, kept in `out`)."""
    import torch

    s = schedule
    if isinstance(bursts, np.ndarray):
        bursts = torch.from_numpy(np.ascontiguousarray(bursts, dtype=np.uint8).reshape(-1)).cuda()
    if bursts.dtype != torch.uint8 or not bursts.is_contiguous():
        raise ValueError("bursts must be a contiguous uint8 tensor")
    per = s.burst_bits * 2 if soft else (s.burst_bytes if burst_stride is None else int(burst_stride))
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
