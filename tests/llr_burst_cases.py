"""Soft bursts as LLRs (include/mbx_burst.h, mbx_burst_schedule_create_llr; include/mbx_llr.h, mbx_soft_from_llr): what the CPU and
GPU suites share.  Every LLR path is defined by equivalence: the conversion is the host function mbx_soft_bits_from_llr (held to
the reference-made fixture and to the oracle by tests/test_llr_bursts_host.py), and a gather, launch or submit of LLR bursts is the
same call with the PER-BIT schedule of the same arrays and the same inversion sequence on the host-converted cells, which
tests/test_gpu_bursts.py and tests/test_gpu_symbol_bursts.py hold to the oracle.  So every comparison is exact.  Importable without
a GPU."""
import ctypes as C

import numpy as np

from mbelib_neo_amd import bursts as B

WIDTHS = {2: B.FORM_LLR16, 1: B.FORM_LLR8}   # llr_bytes -> form
DTYPE = {2: np.int16, 1: np.int8}
INVALID_ARGUMENT = -1
# the values where the conversion changes its mind: the sign, the saturation of the magnitude, the ends of each type
PLANTED = {2: (0, 1, -1, 254, -254, 255, -255, 256, -256, 32767, -32768), 1: (0, 1, -1, 127, -128)}
STAGE_BYTES, MOST_BURSTS = 32768, {2: 16, 1: 32}   # kSoftStageBytes, and the cap of each width (mbx_burst.hip)


def bursts_per_workgroup(llr_bytes, burst_bits):
    """how many bursts a workgroup of the LLR gather stages: mbx_burst_schedule_create_llr's rule"""
    return min(MOST_BURSTS[llr_bytes], max(1, STAGE_BYTES // (burst_bits * llr_bytes)))


def counts(llr_bytes, burst_bits):
    """burst counts that end inside the first workgroup, at its end, one behind it, and some workgroups on"""
    nb = bursts_per_workgroup(llr_bytes, burst_bits)
    return sorted({1, nb, nb + 1, 97})


def gather_shapes(codec):
    """(frames per burst, burst bits): an odd length (int8 bursts start at every byte phase, int16 bursts at both dword phases), an
    LDU-sized one for IMBE, and the exact fit without a bit to spare"""
    shapes = [(3, 601)]
    if codec == 0:
        shapes.append((9, 1728 + 431))
    shapes.append((1, B.channel_bits(codec)))
    return shapes


def random_llrs(rng, n, schedule, llr_bytes):
    """[n, burst_bits] LLRs of the width: half of them anywhere in the type, half near zero where an int16 does not saturate, and
    PLANTED on received bits that an entry names, each value on an inverted and on a plain bit where the sequence has both"""
    info = np.iinfo(DTYPE[llr_bytes])
    nbits = schedule.burst_bits
    wide = rng.integers(info.min, info.max + 1, size=(n, nbits))
    near = rng.integers(-300, 301, size=(n, nbits)).clip(info.min, info.max)
    out = np.where(rng.integers(0, 2, size=(n, nbits)) == 1, wide, near)
    named = np.unique(schedule.src_bit)
    inv = schedule.invert if schedule.invert is not None else np.zeros(nbits, dtype=np.uint8)
    groups = [g for g in (named[inv[named] == 0], named[inv[named] == 1]) if g.size]
    for g in groups:
        for i, v in enumerate(PLANTED[llr_bytes]):
            out[(3 * i) % n, g[(7 * i) % g.size]] = v
            out[n - 1 - (i % n), g[g.size - 1 - (5 * i) % g.size]] = v
    return out.astype(DTYPE[llr_bytes])


def host_cells(L, llr):
    """mbx_soft_bits_from_llr, the pinned host conversion, of integer LLRs of any width -> uint8 [..., 2]"""
    wide = np.ascontiguousarray(llr, dtype=np.int16)
    out = np.zeros(wide.shape + (2,), dtype=np.uint8)
    assert L.mbx_soft_bits_from_llr(wide.ctypes.data, out.ctypes.data, wide.size) == 0
    return out


def old_conversion(llr):
    """the loop mbx_soft_bits_from_llr was before the conversion got a function of its own, in numpy"""
    v = np.asarray(llr, dtype=np.int16).astype(np.int64)
    mag = np.where(v < 0, -v, v)
    return np.stack([(v > 0).astype(np.uint8), np.where(mag > 255, 255, mag).astype(np.uint8)], axis=-1)


def llrs_carrying(cells, llr_bytes):
    """LLRs of the width that say what per-bit cells [..., 2] say, as far as an LLR can: the sign from the hard decision, the
    magnitude from the reliability, at least 1 and at most what the type holds (the frames a burst carries stay decodable)"""
    c = np.asarray(cells, dtype=np.uint8)
    mag = np.clip(c[..., 1].astype(np.int32), 1, np.iinfo(DTYPE[llr_bytes]).max)
    return np.where(c[..., 0] & 1, mag, -mag).astype(DTYPE[llr_bytes])


def create_llr(L, codec, F, nbits, src, row, col, llr_bytes, invert):
    h = C.c_void_p()
    a = [np.ascontiguousarray(x, dtype=np.int32) for x in (src, row, col)]
    inv = None if invert is None else np.ascontiguousarray(invert, dtype=np.uint8)
    rc = L.mbx_burst_schedule_create_llr(C.byref(h), codec, F, nbits, *(x.ctypes.data for x in a), llr_bytes, None if inv is None else inv.ctypes.data)
    return rc, h, (L.mbx_last_error() or b"").decode()


def check_accessors(L, s):
    """form, bits, bytes, soft_cells and soft_bytes of a BurstSchedule of any form against the Python model and the header's rules"""
    nbits = s.burst_bits
    want = {B.FORM_PACKED: ((nbits + 7) // 8, nbits, 2 * nbits), B.FORM_BITS: (nbits, nbits, 2 * nbits), B.FORM_DIBITS: (nbits // 2, nbits // 2, nbits),
            B.FORM_LLR16: (0, nbits, 2 * nbits), B.FORM_LLR8: (0, 0, nbits)}[s.form]
    got = (L.mbx_burst_schedule_bytes(s.handle), L.mbx_burst_schedule_soft_cells(s.handle), L.mbx_burst_schedule_soft_bytes(s.handle))
    assert got == want == (s.burst_bytes, s.soft_cells, s.soft_bytes), (s.form, got, want)
    assert (L.mbx_burst_schedule_form(s.handle), L.mbx_burst_schedule_bits(s.handle), L.mbx_burst_schedule_frames(s.handle), L.mbx_burst_schedule_codec(s.handle)) == \
        (s.form, nbits, s.frames_per_burst, s.codec)


class Guarded:
    """`nbytes` of device memory at an address that is `phase` past a 256-byte boundary, between two bands of random bytes that
    check() wants unchanged; the payload starts as random bytes too (load() replaces them)"""
    BAND = 4096

    def __init__(self, nbytes, phase, rng):
        import torch

        self.lo = self.BAND + phase
        self.n = int(nbytes)
        self.before = rng.integers(0, 256, size=self.lo + self.n + self.BAND, dtype=np.uint8)
        self.mem = torch.from_numpy(self.before.copy()).cuda()
        assert self.mem.data_ptr() % 256 == 0
        self.ptr = self.mem.data_ptr() + self.lo

    def load(self, data):
        import torch

        raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
        assert raw.size == self.n
        self.before[self.lo:self.lo + self.n] = raw
        self.mem[self.lo:self.lo + self.n].copy_(torch.from_numpy(raw.copy()))
        return self

    def check(self, what, unchanged=False):
        """the payload (after a synchronise); the bands, and with unchanged=True the payload, hold what they held"""
        now = self.mem.cpu().numpy()
        hi = self.lo + self.n
        assert np.array_equal(now[:self.lo], self.before[:self.lo]), f"{what}: bytes in front of the buffer changed"
        assert np.array_equal(now[hi:], self.before[hi:]), f"{what}: bytes behind the buffer changed"
        if unchanged:
            assert np.array_equal(now[self.lo:hi], self.before[self.lo:hi]), f"{what}: the buffer changed"
        return now[self.lo:hi]
