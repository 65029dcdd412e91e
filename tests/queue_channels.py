"""Channels of the per-frame library for the queue-mode tests (tests/test_gpu_mixed.py, tests/queue_flush_case.py): one channel is
its three structs, its frames and the buffers the mbe_process*Frame[f] calls fill, so that the same frames can go through the
synchronous calls and through a queued flush and be compared byte for byte.  Test infrastructure."""
import numpy as np

import soft_mix

HARD_CALLS = {0: "mbe_processImbe7200x4400Frame", 1: "mbe_processAmbe3600x2450Frame", 2: "mbe_processImbe7100x4400Frame",
              3: "mbe_processAmbe3600x2400Frame"}
SOFT_CALLS = {c: n.replace("Frame", "SoftFrame") for c, n in HARD_CALLS.items()}
NBITS = {0: 88, 1: 49, 2: 88, 3: 49}
MBE_BATCH_QUEUE_SOFT = 0x10
WHAT = ("pcm", "result", "bits", "state")


class Channel:
    """channel c: codec c % 4, soft input where (c // 4) % 2, the short call where (c // 8) % 2; 9 frames -- unless the caller says
    otherwise (`cells`: the channel's frames as soft cells [T, cells, 2]; a hard channel sends their hard decisions)"""

    def __init__(self, mbe, c, codec=None, soft=None, short=None, cells=None):
        import ctypes as C

        from mbelib_neo_amd.layout import PARMS_DTYPE, RESULT_DTYPE

        self.c, self.codec, self.t = c, c % 4 if codec is None else codec, 0
        self.soft = (c // 4) % 2 == 1 if soft is None else soft
        short = (c // 8) % 2 == 1 if short is None else short
        if cells is None:
            cells = soft_mix.frames(self.codec, 1, 9, tag=300 + c)
        self.T = len(cells)
        self.frames = np.ascontiguousarray(cells) if self.soft else np.ascontiguousarray(cells[..., 0]).astype(np.int8)
        self.fn = getattr(mbe, (SOFT_CALLS if self.soft else HARD_CALLS)[self.codec] + ("" if short else "f"))
        self.pcm = np.zeros((self.T, 160), dtype=np.int16 if short else np.float32)
        self.res = np.zeros(self.T, dtype=RESULT_DTYPE)
        self.bits = np.zeros((self.T, NBITS[self.codec]), dtype=np.int8)
        self.st = [np.zeros(1, dtype=PARMS_DTYPE) for _ in range(3)]
        self.p = lambda a: a.ctypes.data_as(C.c_void_p)
        mbe.mbe_initMbeParms(self.p(self.st[0]), self.p(self.st[1]), self.p(self.st[2]))
        self.rets = []

    def call(self, mbe):
        t, p = self.t, self.p
        if t == 0:
            mbe.mbe_setThreadRngSeed(9000 + self.c)
        self.rets.append(self.fn(p(self.pcm[t]), p(self.res[t:t + 1]), p(self.frames[t]), p(self.bits[t]), p(self.st[0]), p(self.st[1]), p(self.st[2])))
        self.t += 1

    def outputs(self):
        return self.pcm.tobytes(), self.res.tobytes(), self.bits.tobytes(), np.concatenate(self.st).tobytes()
