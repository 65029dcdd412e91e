"""The reference's semantics of an encrypted channel, frame by frame on the CPU oracle: what a host written against the split API
does -- the FEC half (mbe_decodeImbe7200x4400Frame / mbe_decodeAmbe3600x2450Frame and the 7100x4400 one: parameter bits and the
error context in *result), the host's own XOR of its keystream onto imbe_d / ambe_d, then mbe_processImbe4400Dataf /
mbe_processAmbe2450Dataf / mbe_processAmbe2400Dataf with the decode's result as context -- for S streams x T frames in stream
order.  Binds mbxo_record_to_bits, mbxo_record_to_result and the three *_dataf calls from the loaded oracle handle (precedent:
Oracle.process_ambe2400_data).  Test infrastructure: imported without a GPU."""
import ctypes as C

import numpy as np

from mbelib_neo_amd import keystream as K
from mbelib_neo_amd.layout import PARMS_DTYPE, RECORD_DTYPE, RESULT_DTYPE, RNG_DTYPE

_vp = C.c_void_p


def _bind(o):
    h = o.h
    h.mbxo_record_to_bits.restype = None
    h.mbxo_record_to_bits.argtypes = [_vp, C.c_int, _vp]
    h.mbxo_record_to_result.restype = None
    h.mbxo_record_to_result.argtypes = [_vp, _vp]
    for name in ("mbxo_process_imbe4400_dataf", "mbxo_process_ambe2450_dataf", "mbxo_process_ambe2400_dataf"):
        getattr(h, name).restype = C.c_int
        getattr(h, name).argtypes = [_vp] * 7
    return h


def process_batch_keyed(o, codec, S, T, frames, rows, state, rng, soft=False):
    """frames: packed wire frames [S*T, 18|9] (soft: cells [S*T, cells, 2]); rows: keystream rows [S*T, 12]; state [S, 3] and rng [S]
    as Oracle.init_state / rng_seeded make them (copied).  Returns the dict of Oracle.process_batch without "peak": the records hold
    the bits AFTER the keystream and the FEC's own w[3]."""
    h = _bind(o)
    n = S * T
    nbits = K.NBITS[codec]
    dataf = {0: h.mbxo_process_imbe4400_dataf, 2: h.mbxo_process_imbe4400_dataf, 1: h.mbxo_process_ambe2450_dataf,
             3: h.mbxo_process_ambe2400_dataf}[codec]
    fec = o.fec_soft_batch(codec, np.asarray(frames).reshape(n, -1, 2)) if soft else o.fec_batch(codec, frames)   # the FEC half, frame by frame
    key_bits = K.bits_from_rows(rows, codec).astype(np.int8)
    state = np.ascontiguousarray(state).copy()
    rng = np.ascontiguousarray(rng).copy()
    pcmf = np.zeros((n, 160), dtype=np.float32)
    results = np.zeros(n, dtype=RESULT_DTYPE)
    records = np.zeros(n, dtype=RECORD_DTYPE)
    bits = np.zeros(88, dtype=np.int8)
    for s in range(S):
        cur, prev, enh = (state.ctypes.data + (3 * s + j) * PARMS_DTYPE.itemsize for j in range(3))
        for t in range(T):
            f = s * T + t
            h.mbxo_record_to_bits(fec[f:f + 1].ctypes.data, nbits, bits.ctypes.data)
            h.mbxo_record_to_result(fec[f:f + 1].ctypes.data, results[f:f + 1].ctypes.data)
            bits[:nbits] ^= key_bits[f]   # the host's XOR, between the reference's two calls
            dataf(pcmf[f].ctypes.data, results[f:f + 1].ctypes.data, bits.ctypes.data, cur, prev, enh, rng.ctypes.data + s * RNG_DTYPE.itemsize)
            w = fec["w"][f].copy()   # the FEC's record with the keyed bits toggled one by one: w[3] and the bits beyond nbits as they were
            for i in np.flatnonzero(key_bits[f]):
                w[i >> 5] ^= np.uint32(1 << (31 - (int(i) & 31)))
            records["w"][f] = w
    return {"pcm16": o.floattoshort(pcmf), "pcmf": pcmf, "results": results, "records": records, "state": state, "rng": rng}
