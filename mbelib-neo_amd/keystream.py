"""Keystream input (include/mbx_keystream.h) -- the numpy definition of a keystream row and of what the library does with it.

A host that serves an encrypted channel XORs its cipher's keystream onto the parameter bits between FEC and parameter decode
(the reference's split API: mbe_decode*Frame, the XOR on imbe_d / ambe_d, mbe_process*Dataf).  The library applies a caller's
keystream at that place on the device; it owns no cipher.  One row of ROW_BYTES bytes per frame whatever the codec: parameter
bit i is XORed with bit 7 - (i & 7) of byte i >> 3 -- keystream octets MSB first --, bits at and beyond NBITS[codec] are ignored,
and w[3] of a record (error counts and flags) has no keystream.  Host only, numpy only: tests hold the library to this."""
import numpy as np

from .layout import RECORD_DTYPE

ROW_BYTES = 12
NBITS = {0: 88, 1: 49, 2: 88, 3: 49}   # a 7100x4400 record (codec 2) is keyed in 7200x4400 order, as it leaves the front end


def rows_from_bits(bits):
    """[n, nbits] 0/1 keystream bits (nbits <= 96; 88 for the IMBE codecs, 49 for the AMBE ones) -> [n, 12] uint8 rows."""
    bits = np.asarray(bits)
    if bits.ndim != 2 or bits.shape[1] > 8 * ROW_BYTES:
        raise ValueError("bits must be [n, nbits] with nbits <= 96")
    if bits.size and (bits.min() < 0 or bits.max() > 1):
        raise ValueError("keystream bits must be 0 or 1")
    padded = np.zeros((bits.shape[0], 8 * ROW_BYTES), dtype=np.uint8)
    padded[:, :bits.shape[1]] = bits
    return np.packbits(padded, axis=1)   # MSB first: bit i of a row's 96 in bit 7 - (i & 7) of byte i >> 3


def bits_from_rows(rows, codec):
    """[n, 12] uint8 rows -> the [n, NBITS[codec]] 0/1 bits that count."""
    rows = _rows(rows)
    return np.unpackbits(rows, axis=1)[:, :NBITS[int(codec)]]


def words(rows, codec):
    """[n, 12] rows -> uint32 [n, 3]: what is XORed onto w[0..2] of the records (bits beyond NBITS[codec] masked off)."""
    rows = _rows(rows)
    nbits = NBITS[int(codec)]
    be = rows.reshape(-1, 3, 4).astype(np.uint32)
    w = (be[:, :, 0] << 24) | (be[:, :, 1] << 16) | (be[:, :, 2] << 8) | be[:, :, 3]
    for j in range(3):
        kept = min(max(nbits - 32 * j, 0), 32)
        w[:, j] &= np.uint32((0xFFFFFFFF << (32 - kept)) & 0xFFFFFFFF)
    return w


def apply(records, rows, codec):
    """A copy of `records` (RECORD_DTYPE [n]) with row i applied to record i: what mbx_keystream_apply_host, mbx_apply_keystream
    and the front launch of every keyed call do."""
    rec = np.array(records, dtype=RECORD_DTYPE, copy=True).reshape(-1)
    w = words(rows, codec)
    if w.shape[0] != rec.size:
        raise ValueError("one keystream row per record")
    rec["w"][:, :3] ^= w
    return rec


def _rows(rows):
    rows = np.ascontiguousarray(rows)
    if rows.dtype != np.uint8 or rows.ndim != 2 or rows.shape[1] != ROW_BYTES:
        raise ValueError("keystream rows must be uint8 [n, 12]")
    return rows
