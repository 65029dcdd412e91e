"""Guard bands round the buffers of ONE call: every buffer the call is handed lies in one uint8 allocation (device memory, pageable
host memory or pinned host memory), at EXACTLY the alignment its contract states and no better, at its exact size, with at least
GUARD bytes of its own in front and behind.  Guards and outputs are pre-filled with a pattern that is a function of the byte's
absolute offset in the arena and of a seed -- no memset, no copy of zeros and no copy of neighbouring bytes reproduces it -- and
check() regenerates it where the arena lives (nothing but the changed offsets is copied to the host) and raises an AssertionError
that names the buffer, the side, the distance of the first and last changed byte from the payload and their number.  Buffers
registered read-only are compared whole with what was loaded into them.

Nothing here ever places a buffer against unmapped memory: every guard is allocated memory, and a store outside a payload shows as
changed bytes, not as a fault.  Importable without a GPU (tests/test_memory_contract_host.py holds the helper to planted bytes in a
numpy arena, and ALIGN to the table in include/mbx.h)."""
import ctypes
from collections import namedtuple

import numpy as np

GUARD = 16384   # bytes: more than a stream's state triplet (7,812 B) and more than a wave's widest store (64 x 16 B)

# the alignment in bytes each kind of pointer needs: the table "Alignment" of include/mbx.h, line for line
ALIGN = {
    "frames": 1,        # wire frames of the AMBE codecs (byte loads), packed frames out
    "frames2": 2,       # wire frames of the IMBE codecs and the rows of a mixed batch: read in 16-bit pieces
    "frames4": 4,       # IMBE frames where the one-launch and fused instances are wanted (dword loads)
    "codec": 1,         # d_stream_codec
    "cells": 4,         # the 0/1 chars of mbx_pack_cells, read four at a time
    "soft": 2,          # mbe_soft_bit cells: (bit, reliability) pairs are loaded as one 16-bit word
    "pcm16": 2,
    "pcmf": 4,
    "results": 4,
    "state": 4,
    "resident": 4,
    "index": 4,         # d_stream_index, d_frame_offset, d_status, d_errs, d_rc, d_done, words of the ECC calls
    "rng": 8,
    "hist": 8,
    "records": 16,
    "workspace": 16,
    "stage": 16,        # both buffers of mbx_stage_in
    "f2s_in": 8,        # mbx_floattoshort: float pairs in ...
    "f2s_out": 4,       # ... one dword of two samples out
}


def frames_kind(codec, one_frame=False):
    """the kind of a hard-frame array of `codec` (None: the rows of a mixed batch); one_frame: the T = 1 IMBE instances are wanted"""
    if codec in (1, 3):
        return "frames"
    return "frames4" if one_frame and codec is not None else "frames2"


Buf = namedtuple("Buf", "name nbytes kind readonly")


def buf(name, nbytes, kind, readonly=False):
    assert kind in ALIGN, kind
    return Buf(name, int(nbytes), kind, bool(readonly))


def _mix(off, seed):
    """the pattern byte of absolute offset(s) `off` (int64 numpy array or torch tensor): every product stays below 2^63"""
    x = (off * 0x3C6EF35F + (int(seed) * 0x47502933 + 0x1234567) % 0x7FFFFFFF) & 0xFFFFFFFF
    x = x ^ (x >> 15)
    x = (x * 0x2C1B3C6D) & 0xFFFFFFFF
    x = x ^ (x >> 13)
    return x & 0xFF


def pattern_numpy(lo, hi, seed):
    return _mix(np.arange(lo, hi, dtype=np.int64), seed).astype(np.uint8)


def pattern_torch(lo, hi, seed, device):
    import torch

    return _mix(torch.arange(lo, hi, dtype=torch.int64, device=device), seed).to(torch.uint8)


Slot = namedtuple("Slot", "name start end front back kind readonly")   # payload [start, end), its own guards [front, start) and [end, back)


def plan(specs, base_address, guard=GUARD):
    """Offsets for the payloads of `specs` (Buf) in an arena that starts at base_address: payload i at an address that is a multiple
    of its alignment a and NOT of 2 a, guard bytes of its own on either side (never shared with a neighbour: the guard behind one
    payload ends where the guard in front of the next begins).  Returns (slots, total bytes)."""
    slots, at = [], 0
    for s in specs:
        a = ALIGN[s.kind]
        front = at
        start = front + guard
        start += (-(base_address + start)) % a
        if (base_address + start) % (2 * a) == 0:
            start += a
        end = start + s.nbytes
        back = end + guard
        slots.append(Slot(s.name, start, end, front, back, s.kind, s.readonly))
        at = back
    return slots, at


def plan_bytes(specs, guard=GUARD):
    """an upper bound of what plan() needs whatever the base address is"""
    return sum(s.nbytes + 2 * guard + 2 * ALIGN[s.kind] for s in specs) + 64


class GuardError(AssertionError):
    pass


class Arena:
    """where = "numpy" (pageable host memory), "pinned" (host memory from `pinned_alloc(nbytes)` -> address, e.g. mbx_host_alloc) or
    "cuda" (a torch uint8 tensor on the current device)."""

    def __init__(self, specs, where="numpy", seed=1, guard=GUARD, pinned_alloc=None, pinned_free=None):
        self.where, self.seed, self.guard = where, int(seed), guard
        names = [s.name for s in specs]
        assert len(set(names)) == len(names), "buffer names must be unique"
        size = plan_bytes(specs, guard)
        self._free = None
        if where == "cuda":
            import torch

            self.mem = torch.empty(size, dtype=torch.uint8, device="cuda")
            self.base = self.mem.data_ptr()
        elif where == "pinned":
            p = pinned_alloc(size)
            assert p, "no pinned memory"
            self._free = (pinned_free, p)
            self.mem = np.ctypeslib.as_array((ctypes.c_uint8 * size).from_address(p))
            self.base = p
        else:
            assert where == "numpy", where
            self.mem = np.empty(size, dtype=np.uint8)
            self.base = self.mem.ctypes.data
        self.slots, self.used = plan(specs, self.base, guard)
        assert self.used <= size
        self.by_name = {s.name: s for s in self.slots}
        self.expected = {}   # read-only buffers: the bytes loaded into them (numpy)
        self.fill(0, self.used)

    def close(self):
        if self._free:
            fn, p = self._free
            self.mem = None
            fn(p)
            self._free = None

    # -- the pattern -----------------------------------------------------------------------------------------------------------
    def _pattern(self, lo, hi):
        if self.where == "cuda":
            return pattern_torch(lo, hi, self.seed, self.mem.device)
        return pattern_numpy(lo, hi, self.seed)

    def fill(self, lo, hi, step=1 << 24):
        for a in range(lo, hi, step):
            b = min(hi, a + step)
            if self.where == "cuda":
                self.mem[a:b].copy_(self._pattern(a, b))
            else:
                self.mem[a:b] = self._pattern(a, b)

    def prefill(self, *names):
        """the payloads of `names` hold the pattern again (outputs, before every launch)"""
        for n in names:
            s = self.by_name[n]
            self.fill(s.start, s.end)

    def prefill_bytes(self, name, lo=0, hi=None):
        """what prefill() put into bytes [lo, hi) of a payload, as a numpy array (rows a launch must leave alone)"""
        s = self.by_name[name]
        hi = s.end - s.start if hi is None else hi
        return pattern_numpy(s.start + lo, s.start + hi, self.seed)

    # -- access ----------------------------------------------------------------------------------------------------------------
    def view(self, name):
        s = self.by_name[name]
        return self.mem[s.start:s.end]

    def ptr(self, name):
        return self.base + self.by_name[name].start

    def nbytes(self, name):
        s = self.by_name[name]
        return s.end - s.start

    def tensor(self, name, dtype, *shape):
        """cuda arenas: the payload as a tensor of `dtype` (a view: the alignment of every kind is at least its element size)"""
        return self.view(name).view(dtype).view(*shape)

    def array(self, name, dtype, *shape):
        """host arenas: the payload as a numpy view"""
        return self.view(name).view(dtype).reshape(*shape)

    def load(self, name, data):
        """bytes into a payload of exactly their size; a read-only buffer is from now on compared with them"""
        s = self.by_name[name]
        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert raw.size == s.end - s.start, f"{name}: {raw.size} bytes for a payload of {s.end - s.start}"
        if self.where == "cuda":
            import torch

            self.mem[s.start:s.end].copy_(torch.from_numpy(raw.copy()))
        else:
            self.mem[s.start:s.end] = raw
        if s.readonly:
            self.expected[name] = raw.copy()

    def read(self, name):
        """the payload's bytes as a numpy copy"""
        v = self.view(name)
        return v.cpu().numpy() if self.where == "cuda" else v.copy()

    # -- the check ---------------------------------------------------------------------------------------------------------------
    def _changed(self, lo, hi, want=None):
        """offsets in [lo, hi) whose byte differs from the pattern (or from `want`): (count, first, last) relative to lo"""
        if hi <= lo:
            return 0, -1, -1
        if self.where == "cuda":
            import torch

            ref = self._pattern(lo, hi) if want is None else torch.from_numpy(want).to(self.mem.device)
            bad = torch.nonzero(self.mem[lo:hi] != ref).reshape(-1)
            n = int(bad.numel())
            return (n, int(bad[0]), int(bad[-1])) if n else (0, -1, -1)
        ref = self._pattern(lo, hi) if want is None else want
        bad = np.flatnonzero(self.mem[lo:hi] != ref)
        return (bad.size, int(bad[0]), int(bad[-1])) if bad.size else (0, -1, -1)

    def check(self, what=""):
        """after the caller has synchronised: every guard against the regenerated pattern, every read-only payload against what was
        loaded; raises GuardError (an AssertionError) listing every finding"""
        found = []
        for s in self.slots:
            n, first, last = self._changed(s.front, s.start)
            if n:   # distance 1 = the byte just in front of the payload
                found.append(f"{s.name}: {n} guard byte(s) changed IN FRONT OF the payload, {s.start - s.front - last} .. {s.start - s.front - first} "
                             f"bytes before its first byte")
            n, first, last = self._changed(s.end, s.back)
            if n:   # distance 0 = the first byte behind the payload
                found.append(f"{s.name}: {n} guard byte(s) changed BEHIND the payload of {s.end - s.start} bytes, {first} .. {last} bytes past its end")
            if s.readonly:
                assert s.name in self.expected, f"{s.name}: read-only but never loaded"
                n, first, last = self._changed(s.start, s.end, self.expected[s.name])
                if n:
                    found.append(f"{s.name}: read-only input changed: {n} byte(s), first at offset {first}, last at offset {last} of {s.end - s.start}")
        if found:
            raise GuardError((what + ": " if what else "") + "; ".join(found))
