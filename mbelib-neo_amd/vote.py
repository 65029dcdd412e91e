"""Voted streams (include/mbx_vote.h) in numpy: the definition the host functions (mbx_vote_select_host, mbx_vote_combine_host) and the
kernels (vote_select_kernel, vote_combine_kernel) are held to, the Plan wrapper of the C handle, and the makers of test candidates.

cand_offset holds S + 1 ascending offsets, cand_offset[0] = 0 and C = cand_offset[S]; voted stream s owns candidate rows
cand_offset[s] .. cand_offset[s + 1] - 1 (1 .. 32 of them).  A candidate batch is C rows of T frames; present is uint8 [C, T] or None
(all present).  select() works on records (uint32 [C, T, 4]), combine() on soft cells (uint8 [C, T, cells, 2] = (bit, reliability)).
The numpy part needs neither torch nor the native library."""
import ctypes as C

import numpy as np

from .layout import FRAME_BYTES, FRAME_CELLS, ROW_WIDTHS

MAX_CANDIDATES = 32      # MBX_VOTE_MAX_CANDIDATES
NONE = 0xFF              # MBX_VOTE_NONE
COMBINED = 0xFE          # MBX_VOTE_COMBINED
SELECT, COMBINE = 0, 1   # MBX_VOTE_SELECT, MBX_VOTE_COMBINE
ROW_CELLS = (184, 168, 96)
VOTE_DTYPE = np.dtype([("winner", "u1"), ("present", "u1"), ("best", "u1"), ("second", "u1"), ("agree", "<u4")])   # mbx_vote_record
assert VOTE_DTYPE.itemsize == 8
_ABSENT = np.uint64(0xFFFFFFFF)


def check_offsets(cand_offset):
    """raises ValueError with the library's wording for what mbx_vote_plan_create refuses; returns the offsets as int32 [S + 1]"""
    off = np.asarray(cand_offset)
    if off.ndim != 1 or off.size < 1 or not np.issubdtype(off.dtype, np.integer):
        raise ValueError("cand_offset is S + 1 integers")
    if off.size < 2:
        raise ValueError("S is at least 1")
    if off[0] != 0:
        raise ValueError("cand_offset[0] is 0")
    sizes = np.diff(off.astype(np.int64))
    for s in np.nonzero((sizes < 1) | (sizes > MAX_CANDIDATES))[0]:
        raise ValueError(f"stream {s}: {sizes[s]} candidates (offsets {off[s]} .. {off[s + 1]}), a group has 1 .. MBX_VOTE_MAX_CANDIDATES (32)")
    return off.astype(np.int32)


def _present(present, n_cand, T):
    if present is None:
        return np.ones((n_cand, T), dtype=bool)
    p = np.asarray(present)
    if p.dtype != np.uint8:
        raise TypeError("present is uint8")
    return p.reshape(n_cand, T) != 0


def select(records, present, cand_offset, T):
    """THE definition of the select rule: records uint32 [C, T, 4] (or anything of C * T * 4 words) -> (voted uint32 [S, T, 4], votes
    VOTE_DTYPE [S, T]).  Key of a present candidate j: (c0 + protected) << 16 | c0 << 8 | j, the smallest wins."""
    off = check_offsets(cand_offset)
    S, n_cand = off.size - 1, int(off[-1])
    r = np.asarray(records)
    if r.dtype != np.uint32:
        raise TypeError("records are uint32 words")
    r = r.reshape(n_cand, T, 4)
    there = _present(present, n_cand, T)
    voted = np.empty((S, T, 4), dtype=np.uint32)
    votes = np.zeros((S, T), dtype=VOTE_DTYPE)
    for s in range(S):
        g, th = r[off[s]:off[s + 1]], there[off[s]:off[s + 1]]
        n = g.shape[0]
        c0 = (g[:, :, 3] & 0xFF).astype(np.uint64)
        prot = ((g[:, :, 3] >> 8) & 0xFF).astype(np.uint64)
        key = ((c0 + prot) << np.uint64(16)) | (c0 << np.uint64(8)) | np.arange(n, dtype=np.uint64)[:, None]
        key = np.where(th, key, _ABSENT)
        order = np.sort(key, axis=0)
        key1 = order[0]
        key2 = order[1] if n > 1 else np.full(T, _ABSENT)
        none = key1 == _ABSENT
        won = np.where(none, 0, key1 & np.uint64(0xFF)).astype(np.int64)
        voted[s] = g[won, np.arange(T)]
        equal = (g[:, :, :3] == voted[s][None, :, :3]).all(axis=2) & th
        agree = (equal.astype(np.uint64) << np.arange(n, dtype=np.uint64)[:, None]).sum(axis=0)
        votes["winner"][s] = np.where(none, NONE, won)
        votes["present"][s] = th.sum(axis=0)
        votes["best"][s] = np.where(none, 255, np.minimum(key1 >> np.uint64(16), 255))
        votes["second"][s] = np.where(key2 == _ABSENT, 255, np.minimum(key2 >> np.uint64(16), 255))
        votes["agree"][s] = np.where(none, 0, agree)
    return voted, votes


def combine(cells, present, cand_offset, T):
    """THE definition of the combine rule: cells uint8 [C, T, row_cells, 2] -> (combined uint8 [S, T, row_cells, 2], votes VOTE_DTYPE
    [S, T]).  V = sum over the present of (bit ? +reliability : -reliability); the cell is (V > 0 ? 1 : V < 0 ? 0 : the bit byte of the
    lowest-index present candidate, min(|V|, 255)); with nobody present, candidate 0's cells."""
    off = check_offsets(cand_offset)
    S, n_cand = off.size - 1, int(off[-1])
    c = np.asarray(cells)
    if c.dtype != np.uint8:
        raise TypeError("cells are uint8 (bit, reliability) pairs")
    c = c.reshape(n_cand, T, -1, 2)
    row_cells = c.shape[2]
    if row_cells not in ROW_CELLS:
        raise ValueError("row_cells is 184, 168 or 96")
    there = _present(present, n_cand, T)
    out = np.empty((S, T, row_cells, 2), dtype=np.uint8)
    votes = np.zeros((S, T), dtype=VOTE_DTYPE)
    for s in range(S):
        g, th = c[off[s]:off[s + 1]], there[off[s]:off[s + 1]]
        n = g.shape[0]
        v = np.where(g[..., 0] != 0, 1, -1) * g[..., 1].astype(np.int64) * th[:, :, None]
        V = v.sum(axis=0)                                     # [T, row_cells]
        first = np.argmax(th, axis=0)                         # lowest-index present candidate (0 where there is none)
        first_bit = g[first, np.arange(T), :, 0]
        bit = np.where(V > 0, 1, np.where(V < 0, 0, first_bit)).astype(np.uint8)
        comb = np.stack([bit, np.minimum(np.abs(V), 255).astype(np.uint8)], axis=-1)
        none = ~th.any(axis=0)
        out[s] = np.where(none[:, None, None], g[0], comb)
        mask = (th.astype(np.uint64) << np.arange(n, dtype=np.uint64)[:, None]).sum(axis=0)
        votes["winner"][s] = np.where(none, NONE, COMBINED)
        votes["present"][s] = th.sum(axis=0)
        votes["best"][s] = 255
        votes["second"][s] = 255
        votes["agree"][s] = mask
    return out, votes


class Plan:
    """mbx_vote_plan: the grouping on the current device, immutable; `handle` is what the C calls take.  Needs mbx_init() for the device."""

    def __init__(self, cand_offset):
        from . import _native

        self.offsets = check_offsets(cand_offset)
        self._lib = _native.lib()
        h = C.c_void_p()
        _native.check(self._lib.mbx_vote_plan_create(C.byref(h), self.offsets.ctypes.data, self.offsets.size - 1), "mbx_vote_plan_create")
        self.handle = h

    @property
    def streams(self):
        return int(self.offsets.size - 1)

    @property
    def candidates(self):
        return int(self.offsets[-1])

    def workspace_frames(self, codec, mode, T):
        return int(self._lib.mbx_vote_workspace_frames(self.handle, int(codec), int(mode), int(T)))

    def close(self):
        if self.handle is not None:
            self._lib.mbx_vote_plan_destroy(self.handle)
            self.handle = None

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _wire_bits(codec):
    return sum(ROW_WIDTHS[int(codec)])


def noisy_sites(frames, codec, ber_per_site, rng):
    """test candidates: uint8 [sites, n, frame_bytes], copies of the clean packed wire frames [n, frame_bytes] with independent bit flips
    at rate ber_per_site[k] over the channel bits of site k (the padding bits of a 142-bit frame stay)"""
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, FRAME_BYTES[int(codec)])
    nbits = _wire_bits(codec)
    out = []
    for ber in ber_per_site:
        flips = np.zeros((f.shape[0], f.shape[1] * 8), dtype=np.uint8)
        flips[:, :nbits] = rng.random((f.shape[0], nbits)) < ber
        out.append(f ^ np.packbits(flips, axis=1))
    return np.stack(out)


def cells_of_frames(frames, codec):
    """(bits int64 [n, cells], used bool [cells]): packed wire frames in the reference's array shape, the first wire bit of a row its highest cell"""
    codec = int(codec)
    f = np.ascontiguousarray(frames, dtype=np.uint8).reshape(-1, FRAME_BYTES[codec])
    rows, cols = FRAME_CELLS[codec]
    wire = np.unpackbits(f, axis=1)
    bits = np.zeros((f.shape[0], rows, cols), dtype=np.int64)
    used = np.zeros((rows, cols), dtype=bool)
    at = 0
    for r, w in enumerate(ROW_WIDTHS[codec]):
        bits[:, r, :w] = wire[:, at:at + w][:, ::-1]
        used[r, :w] = True
        at += w
    return bits.reshape(f.shape[0], rows * cols), used.reshape(-1)


def noisy_soft_sites(frames, codec, ber_per_site, rng):
    """test candidates for the soft forms: uint8 [sites, n, cells, 2] = (bit, reliability).  Site k sees every channel bit flipped with
    probability ber_per_site[k], independently of the other sites; a bit that came through has a reliability drawn from 64 .. 255, a
    flipped one from 0 .. 127 (a soft demodulator is less sure of what it gets wrong); unused cells are 0 / 0"""
    bits, used = cells_of_frames(frames, codec)
    out = []
    for ber in ber_per_site:
        flip = (rng.random(bits.shape) < ber) & used
        rel = np.where(flip, rng.integers(0, 128, size=bits.shape), rng.integers(64, 256, size=bits.shape))
        hard = (bits ^ flip) * used
        out.append(np.stack([hard, rel * used], axis=-1).astype(np.uint8))
    return np.stack(out)
