"""Clean IMBE 7100x4400 wire frames for the tests.  framegen has no encoder for this codec: `encode_imbe7100x4400` is the inverse
of the oracle's front end (bit order of the 7100 -> 7200 conversion, Golay(23,12), the codec's own Hamming(15,11) table read off the
oracle, pseudo-random modulation), and `check_encoder` of tests/silent_store_cases.py holds it to that front end frame by frame.
Shared by tests/silent_store_cases.py and tests/pitch_lattice.py.
Test infrastructure: imported without a GPU; nothing in the package uses it."""
import math

import numpy as np

from mbelib_neo_amd import framegen
from mbelib_neo_amd.layout import ROW_WIDTHS


def _k_of_b0(b0):   # K(b0) as the 7100 -> 7200 conversion computes it (float fundamental, double quotient)
    w0 = float(np.float32(np.float32(4.0 * math.pi) / np.float32(b0 + 39.5)))
    L = int(0.9254 * int((math.pi / w0) + 0.25))
    return int(np.float32(L + 2) / np.float32(3)) if L < 37 else 12


def _source_index_7100(K):
    """src[j]: the 7100-order position of 7200-order bit j (the conversion is d7200[j] = d7100[src[j]])"""
    src = np.zeros(88, dtype=np.int64)
    src[87] = 0
    src[48 + K] = 42
    src[49 + K] = 43
    for i in range(K):
        src[48 + i] = 44 + i
    j, k = 0, 1
    while j < 87:
        src[j] = k
        j += 1
        if j == 48:
            j += K + 2
        k += 1
        if k == 42:
            k += K + 2
    return src


_hamming7100_words = None


def _hamming7100_encode(data11, oracle):
    """the 15-bit word of the 7100x4400 Hamming code that carries data11 in bits 14..4 without an error (table from the oracle)"""
    global _hamming7100_words
    if _hamming7100_words is None:
        table = np.zeros(2048, dtype=np.uint32)
        for cw in range(1 << 15):
            fixed, errs = oracle.hamming7100(cw)
            if errs == 0:
                table[(fixed >> 4) & 0x7FF] = fixed
        _hamming7100_words = table
    return _hamming7100_words[np.asarray(data11, dtype=np.int64)]


_k_table = None


def encode_imbe7100x4400(bits7200, oracle):
    """[n, 88] parameter bits in the 7200x4400 order -> clean IMBE 7100x4400 wire frames [n, 18].  The bit order depends on the
    frame's K(b0) alone, so the frames are reordered group by group of equal K (twelve at the most), not one by one."""
    global _k_table
    if _k_table is None:
        _k_table = np.array([_k_of_b0(b0) for b0 in range(256)], dtype=np.int64)
    b = np.asarray(bits7200, dtype=np.uint8)
    toi = framegen._bits_to_int
    b0 = (toi(b, 0, 6).astype(np.int64) << 2) | (b[:, 85].astype(np.int64) << 1) | b[:, 86].astype(np.int64)
    K = _k_table[b0]
    d = np.zeros_like(b)
    for k in np.unique(K):
        rows = np.flatnonzero(K == k)
        d[rows[:, None], _source_index_7100(int(k))[None, :]] = b[rows]
    u0 = toi(d, 0, 7)
    masks = framegen.pr_masks(u0, (24, 23, 23, 15, 15))
    rows = [(framegen.golay2312_encode(u0) & 0x3FFFF) << 1,
            (framegen.golay2312_encode(toi(d, 7, 19)) << 1) ^ masks[0],
            framegen.golay2312_encode(toi(d, 19, 31)) ^ masks[1],
            framegen.golay2312_encode(toi(d, 31, 43)) ^ masks[2],
            _hamming7100_encode(toi(d, 43, 54), oracle) ^ masks[3],
            _hamming7100_encode(toi(d, 54, 65), oracle) ^ masks[4],
            toi(d, 65, 88)]
    return framegen._pack_rows(rows, ROW_WIDTHS[2])
