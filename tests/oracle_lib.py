"""ctypes access to the CPU oracle (oracle/liboracle.so).  TEST INFRASTRUCTURE: only tests/,
__graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module."""
import ctypes as C
import os
import subprocess
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.environ.get("MBX_ORACLE_LIBRARY") or os.path.join(ROOT, "oracle", "liboracle.so")   # (override: the sanitizer build, oracle/Makefile)
TABLES = os.path.join(ROOT, "mbelib-neo_amd", "data", "mbx_tables.bin")

import sys

sys.path.insert(0, ROOT)
from mbelib_neo_amd.layout import PARMS_DTYPE, RECORD_DTYPE, RESULT_DTYPE, RNG_DTYPE, FRAME_BYTES, PARAM_BITS  # noqa: E402

_vp = C.c_void_p
SOFT_CELLS = {0: 184, 1: 96, 2: 168, 3: 96}   # (bit, reliability) pairs per soft-decision frame, by codec
MAX_THREADS = 32             # Oracle.process_batch: most ranges of streams decoded side by side
SMALL_BATCH_FRAMES = 16384   # ... and below this many frames ONE thread: a pool costs more than it saves there, and bench.py's
                             # cpu_baseline leg times this function as "cores: 1" on batches of at most 8,192 frames


def default_threads(frames):
    """threads Oracle.process_batch uses for a batch of `frames` frames when the caller does not say"""
    return 1 if frames < SMALL_BATCH_FRAMES else min(len(os.sched_getaffinity(0)), MAX_THREADS)


class Oracle:
    def __init__(self, handle):
        self.h = handle
        h = handle
        h.mbxo_load_tables.restype = C.c_int
        h.mbxo_load_tables.argtypes = [_vp, C.c_size_t]
        blob = open(TABLES, "rb").read()
        assert h.mbxo_load_tables(blob, len(blob)) == 0, "oracle rejected the table blob"
        h.mbxo_golay2312_word.restype = C.c_int
        h.mbxo_golay2312_word.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        h.mbxo_hamming1511_word.restype = C.c_int
        h.mbxo_hamming1511_word.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        for name in ("mbxo_pack_imbe_frame", "mbxo_pack_ambe_frame"):
            getattr(h, name).restype = C.c_int
            getattr(h, name).argtypes = [_vp, _vp]
        for name in ("mbxo_decode_imbe7200x4400_frame", "mbxo_decode_ambe3600x2450_frame"):
            getattr(h, name).restype = C.c_int
            getattr(h, name).argtypes = [_vp, _vp, _vp]
        for name in ("mbxo_decode_imbe4400_parms",):
            getattr(h, name).restype = C.c_int
            getattr(h, name).argtypes = [_vp, _vp, _vp]
        h.mbxo_decode_ambe2450_parms.restype = C.c_int
        h.mbxo_decode_ambe2450_parms.argtypes = [_vp, _vp, _vp, C.c_int]
        for name in ("mbxo_process_imbe4400_dataf", "mbxo_process_ambe2450_dataf", "mbxo_process_ambe2400_dataf"):
            getattr(h, name).restype = C.c_int
            getattr(h, name).argtypes = [_vp] * 7
        for name in ("mbxo_process_imbe7200x4400_framef", "mbxo_process_ambe3600x2450_framef"):
            getattr(h, name).restype = C.c_int
            getattr(h, name).argtypes = [_vp] * 8
        h.mbxo_process_batch.restype = C.c_int
        h.mbxo_process_batch.argtypes = [C.c_int, C.c_int, C.c_int] + [_vp] * 7
        h.mbxo_process_batch_soft.restype = C.c_int
        h.mbxo_process_batch_soft.argtypes = [C.c_int, C.c_int, C.c_int] + [_vp] * 7
        h.mbxo_fec_batch.restype = C.c_int
        h.mbxo_fec_batch.argtypes = [C.c_int, C.c_size_t, _vp, _vp]
        h.mbxo_floattoshort_batch.restype = None
        h.mbxo_floattoshort_batch.argtypes = [_vp, _vp, C.c_size_t]
        h.mbxo_synthesize_speech_batch.restype = None
        h.mbxo_synthesize_speech_batch.argtypes = [C.c_int, _vp, _vp, _vp, _vp]
        h.mbxo_spectral_amp_enhance.restype = C.c_float
        h.mbxo_spectral_amp_enhance.argtypes = [_vp]
        h.mbxo_adaptive_smoothing.restype = None
        h.mbxo_adaptive_smoothing.argtypes = [_vp, _vp]
        h.mbxo_comfort_noisef.restype = None
        h.mbxo_comfort_noisef.argtypes = [_vp, _vp]
        h.mbxo_init_parms.restype = None
        h.mbxo_init_parms.argtypes = [_vp, _vp, _vp]
        h.mbxo_rng_default.restype = None
        h.mbxo_rng_default.argtypes = [_vp]
        h.mbxo_rng_seed.restype = None
        h.mbxo_rng_seed.argtypes = [_vp, C.c_uint32]
        h.mbxo_set_tones.restype = None
        h.mbxo_set_tones.argtypes = [C.c_int]
        h.mbxo_set_preclip_peaks.restype = None
        h.mbxo_set_preclip_peaks.argtypes = [C.c_void_p]
        h.mbxo_set_fft_float.restype = None
        h.mbxo_set_fft_float.argtypes = [C.c_int]
        h.mbxo_fnv1a32.restype = C.c_uint32
        h.mbxo_fnv1a32.argtypes = [_vp, C.c_size_t]
        h.mbxo_tonef.restype = None
        h.mbxo_tonef.argtypes = [_vp, _vp, _vp]
        h.mbxo_tone_dstarf.restype = None
        h.mbxo_tone_dstarf.argtypes = [_vp, _vp, C.c_int]
        # IMBE 7100x4400 front end
        h.mbxo_pack_imbe7100_frame.restype = C.c_int
        h.mbxo_pack_imbe7100_frame.argtypes = [_vp, _vp]
        h.mbxo_hamming1511_7100_word.restype = C.c_int
        h.mbxo_hamming1511_7100_word.argtypes = [C.c_uint32, C.POINTER(C.c_uint32)]
        h.mbxo_convert_imbe7100to7200.restype = C.c_int
        h.mbxo_convert_imbe7100to7200.argtypes = [_vp]
        h.mbxo_decode_imbe7100x4400_frame.restype = C.c_int
        h.mbxo_decode_imbe7100x4400_frame.argtypes = [_vp, _vp, _vp]
        # soft-decision front end
        h.mbxo_decode_imbe7100x4400_soft_frame.restype = C.c_int
        h.mbxo_decode_imbe7100x4400_soft_frame.argtypes = [_vp, _vp, _vp]
        for name in ("mbxo_golay2312_soft", "mbxo_hamming1511_soft", "mbxo_hamming1511_7100_soft"):
            getattr(h, name).restype = C.c_int
            getattr(h, name).argtypes = [_vp, _vp]
        for name in ("mbxo_decode_imbe7200x4400_soft_frame", "mbxo_decode_ambe3600x2450_soft_frame"):
            getattr(h, name).restype = C.c_int
            getattr(h, name).argtypes = [_vp, _vp, _vp]
        h.mbxo_fec_soft_batch.restype = C.c_int
        h.mbxo_fec_soft_batch.argtypes = [C.c_int, C.c_size_t, _vp, _vp]
        h.mbxo_soft_bits_from_llr.restype = C.c_int
        h.mbxo_soft_bits_from_llr.argtypes = [_vp, _vp, C.c_size_t]
        h.mbxo_soft_bits_from_hard.restype = C.c_int
        h.mbxo_soft_bits_from_hard.argtypes = [_vp, _vp, C.c_size_t, C.c_uint8]

    # ---- small wrappers -----------------------------------------------------------------
    def golay(self, cw):
        out = C.c_uint32(0)
        errs = self.h.mbxo_golay2312_word(int(cw), C.byref(out))
        return out.value, errs

    def hamming(self, cw):
        out = C.c_uint32(0)
        errs = self.h.mbxo_hamming1511_word(int(cw), C.byref(out))
        return out.value, errs

    def init_state(self, streams):
        """[streams, 3] (cur, prev, enh) as mbxo_init_parms leaves them: one call, repeated for every stream"""
        one = np.zeros((1, 3), dtype=PARMS_DTYPE)
        self.h.mbxo_init_parms(one[0, 0:1].ctypes.data, one[0, 1:2].ctypes.data, one[0, 2:3].ctypes.data)
        return np.repeat(one, streams, axis=0)

    def rng_seeded(self, seeds):
        r = np.zeros(len(seeds), dtype=RNG_DTYPE)
        base, step = r.ctypes.data, RNG_DTYPE.itemsize
        for i, s in enumerate(seeds):
            self.h.mbxo_rng_default(base + i * step)
            self.h.mbxo_rng_seed(base + i * step, int(s) & 0xFFFFFFFF)
        return r

    def rng_default(self, n):
        one = np.zeros(1, dtype=RNG_DTYPE)
        self.h.mbxo_rng_default(one.ctypes.data)
        return np.repeat(one, n)

    def pack(self, codec, cells):
        """cells: [n, 184|96] int8 -> (rc list, packed [n, 18|9])"""
        cells = np.ascontiguousarray(cells, dtype=np.int8)
        n = cells.shape[0]
        out = np.zeros((n, FRAME_BYTES[codec]), dtype=np.uint8)
        fn = {0: self.h.mbxo_pack_imbe_frame, 1: self.h.mbxo_pack_ambe_frame, 2: self.h.mbxo_pack_imbe7100_frame,
              3: self.h.mbxo_pack_ambe_frame}[codec]
        rcs = [fn(cells[i].ctypes.data, out[i].ctypes.data) for i in range(n)]
        return rcs, out

    def fec_batch(self, codec, frames):
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        n = frames.size // FRAME_BYTES[codec]
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        self.h.mbxo_fec_batch(codec, n, frames.ctypes.data, rec.ctypes.data)
        return rec

    def hamming7100(self, cw):
        out = C.c_uint32(0)
        errs = self.h.mbxo_hamming1511_7100_word(int(cw), C.byref(out))
        return out.value, errs

    def convert7100(self, bits88):
        d = np.ascontiguousarray(bits88, dtype=np.int8).copy()
        assert self.h.mbxo_convert_imbe7100to7200(d.ctypes.data) == 0
        return d

    def decode_imbe7100_frame(self, cells168):
        cells = np.ascontiguousarray(cells168, dtype=np.int8)
        d = np.zeros(88, dtype=np.int8)
        res = np.zeros(1, dtype=RESULT_DTYPE)
        ret = self.h.mbxo_decode_imbe7100x4400_frame(cells.ctypes.data, d.ctypes.data, res.ctypes.data)
        return d, ret, res[0]

    def process_ambe2400_data(self, bits49, total_errors, state3, rng1, plus2=False):
        """one mbe_processAmbe2400Dataf (plus2: mbe_processAmbe2450Dataf) call: state3 = (cur, prev, enh) array of 3, updated in place"""
        d = np.ascontiguousarray(bits49, dtype=np.int8)
        res = np.zeros(1, dtype=RESULT_DTYPE)
        res[0]["total_errors"] = int(total_errors)
        pcm = np.zeros(160, dtype=np.float32)
        fn = self.h.mbxo_process_ambe2450_dataf if plus2 else self.h.mbxo_process_ambe2400_dataf
        ret = fn(
            pcm.ctypes.data, res.ctypes.data, d.ctypes.data, state3[0:1].ctypes.data, state3[1:2].ctypes.data,
            state3[2:3].ctypes.data, rng1.ctypes.data,
        )
        return pcm, ret, res[0]

    def fec_soft_batch(self, codec, soft):
        """soft: [n, 184|96, 2] uint8 (bit, reliability) in the reference's array order -> records"""
        soft = np.ascontiguousarray(soft, dtype=np.uint8)
        n = soft.shape[0]
        rec = np.zeros(n, dtype=RECORD_DTYPE)
        self.h.mbxo_fec_soft_batch(codec, n, soft.ctypes.data, rec.ctypes.data)
        return rec

    def golay_soft(self, soft23):
        soft23 = np.ascontiguousarray(soft23, dtype=np.uint8)
        out = np.zeros(23, dtype=np.int8)
        ret = self.h.mbxo_golay2312_soft(soft23.ctypes.data, out.ctypes.data)
        return out, ret

    def hamming_soft(self, soft15, variant7100=False):
        soft15 = np.ascontiguousarray(soft15, dtype=np.uint8)
        out = np.zeros(15, dtype=np.int8)
        fn = self.h.mbxo_hamming1511_7100_soft if variant7100 else self.h.mbxo_hamming1511_soft
        ret = fn(soft15.ctypes.data, out.ctypes.data)
        return out, ret

    def decode_soft_frame(self, codec, soft):
        soft = np.ascontiguousarray(soft, dtype=np.uint8)
        d = np.zeros(49 if codec == 1 else 88, dtype=np.int8)
        res = np.zeros(1, dtype=RESULT_DTYPE)
        fn = {0: self.h.mbxo_decode_imbe7200x4400_soft_frame, 1: self.h.mbxo_decode_ambe3600x2450_soft_frame,
              2: self.h.mbxo_decode_imbe7100x4400_soft_frame}[codec]
        ret = fn(soft.ctypes.data, d.ctypes.data, res.ctypes.data)
        return d, ret, res[0]

    def soft_from_llr(self, llr):
        llr = np.ascontiguousarray(llr, dtype=np.int16)
        out = np.zeros((llr.size, 2), dtype=np.uint8)
        assert self.h.mbxo_soft_bits_from_llr(llr.ctypes.data, out.ctypes.data, llr.size) == 0
        return out

    def process_batch(self, codec, S, T, frames, state, rng, soft=False, threads=None):
        """frames: packed wire frames, or with soft=True uint8 [S*T, 184|96, 2] soft-decision frames.
        threads: how many contiguous ranges of streams decode side by side (streams are independent, ctypes releases the GIL,
        every range writes its own slices of the same arrays, so the result does not depend on it); None = one per CPU this
        process may run on, at most MAX_THREADS, and one for batches below SMALL_BATCH_FRAMES frames."""
        frames = np.ascontiguousarray(frames, dtype=np.uint8)
        state = np.ascontiguousarray(state).copy()
        rng = np.ascontiguousarray(rng).copy()
        n = S * T
        pcm16 = np.zeros((n, 160), dtype=np.int16)
        pcmf = np.zeros((n, 160), dtype=np.float32)
        results = np.zeros(n, dtype=RESULT_DTYPE)
        records = np.zeros(n, dtype=RECORD_DTYPE)
        peak = np.zeros(n, dtype=np.float32)   # largest |sample| before the soft clip, per frame (parity.int16_bound)
        fn = self.h.mbxo_process_batch_soft if soft else self.h.mbxo_process_batch
        if threads is None:
            threads = default_threads(n)
        threads = max(1, min(int(threads), S))
        frame_bytes = 2 * SOFT_CELLS[codec] if soft else FRAME_BYTES[codec]

        def run(a, b):   # streams [a, b): every pointer moved to stream a, the peak pointer bound to THIS thread (mbx_oracle.h)
            f = a * T
            self.h.mbxo_set_preclip_peaks(peak.ctypes.data + f * 4)
            try:
                return fn(
                    codec, b - a, T, frames.ctypes.data + f * frame_bytes, state.ctypes.data + a * 3 * PARMS_DTYPE.itemsize,
                    rng.ctypes.data + a * RNG_DTYPE.itemsize, pcm16.ctypes.data + f * 320, pcmf.ctypes.data + f * 640,
                    results.ctypes.data + f * RESULT_DTYPE.itemsize, records.ctypes.data + f * RECORD_DTYPE.itemsize,
                )
            finally:
                self.h.mbxo_set_preclip_peaks(None)

        if threads == 1:
            rcs = [run(0, S)]
        else:
            cuts = [S * i // threads for i in range(threads + 1)]
            with ThreadPoolExecutor(max_workers=threads) as pool:
                rcs = list(pool.map(run, cuts[:-1], cuts[1:]))
        assert all(rc == 0 for rc in rcs), rcs
        return {"pcm16": pcm16, "pcmf": pcmf, "results": results, "records": records, "state": state, "rng": rng, "peak": peak}

    def synthesize_speech(self, cur, prev, rng):
        cur = np.ascontiguousarray(cur).copy()
        prev = np.ascontiguousarray(prev).copy()
        rng = np.ascontiguousarray(rng).copy()
        S = cur.shape[0]
        pcmf = np.zeros((S, 160), dtype=np.float32)
        self.h.mbxo_synthesize_speech_batch(S, cur.ctypes.data, prev.ctypes.data, rng.ctypes.data, pcmf.ctypes.data)
        return pcmf, cur, prev, rng

    def floattoshort(self, pcmf):
        pcmf = np.ascontiguousarray(pcmf, dtype=np.float32).reshape(-1, 160)
        out = np.zeros(pcmf.shape, dtype=np.int16)
        self.h.mbxo_floattoshort_batch(pcmf.ctypes.data, out.ctypes.data, pcmf.shape[0])
        return out

    def set_tones(self, on):
        """0: the restatement of the reference's NOTONES build (tone frames = silence); 1 (default): tones synthesised"""
        self.h.mbxo_set_tones(1 if on else 0)

    def set_fft_float(self, on):
        """1: the unvoiced FFT as FFTPACK's float real transform (what the reference's PFFFT runs: float PCM identical to the
        reference's to the last bit); 0 (the default every HIP comparison uses): double precision"""
        self.h.mbxo_set_fft_float(1 if on else 0)

    def fnv(self, arr):
        arr = np.ascontiguousarray(arr)
        return self.h.mbxo_fnv1a32(arr.ctypes.data, arr.nbytes)


def records_to_bits(records, nbits):
    w = records["w"].astype(np.uint32)
    out = np.zeros((w.shape[0], nbits), dtype=np.int8)
    for i in range(nbits):
        out[:, i] = (w[:, i >> 5] >> np.uint32(31 - (i & 31))) & 1
    return out


def records_to_results(records):
    w3 = records["w"][:, 3].astype(np.uint32)
    r = np.zeros(w3.shape[0], dtype=RESULT_DTYPE)
    r["c0_errors"] = w3 & 0xFF
    r["protected_errors"] = (w3 >> 8) & 0xFF
    r["c4_errors"] = (w3 >> 16) & 0xFF
    r["total_errors"] = r["c0_errors"] + r["protected_errors"]
    r["flags"] = (w3 >> 24) & 0xFF
    return r


_cached = None


def load():
    global _cached
    if _cached is None:
        if not os.path.exists(LIB):
            subprocess.check_call(["make", "-C", os.path.join(ROOT, "oracle"), "oracle"])
        _cached = Oracle(C.CDLL(LIB))
    return _cached
