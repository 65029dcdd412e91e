"""Queue-mode flushes that only a fresh process can set up, for tests/test_gpu_mixed.py: the library reads MBE_NEO_ZERO_COPY_FLUSH once
per process.  `python queue_flush_case.py SCENARIO` sends the scenario's frames through the synchronous per-frame calls once, then
through ONE queued flush in each state mode (write-back, resident), and prints one line per mode: `MODE ok`, or `MODE differs: ...`
naming every channel and buffer that is not the synchronous calls' byte for byte.  Scenarios:

mixed48  48 channels of all four codecs, hard and soft, 1..9 pending frames (the scenario of the mixed-launch-set test).  With
         MBE_NEO_ZERO_COPY_FLUSH=0 in the environment this small flush takes the copy path: uploads, one PCM chunk.
chunks   8,195 rows, the smallest flush above the 8,192-row threshold whose four PCM chunks end in a shorter one (2,049, 2,049,
         2,049, 2,048): 43 IMBE 7200x4400 channels x 128 frames, 21 AMBE 3600x2450 channels x 128 frames and one IMBE channel x 3
         frames, all hard input (three groups, one mixed launch set), the short and the float call alternating by channel, queued
         frame by frame across the channels.  Chunk edges fall inside channels.
Test infrastructure."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for d in (HERE, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

import shim_lib  # noqa: E402
import soft_mix  # noqa: E402
from queue_channels import MBE_BATCH_QUEUE_SOFT, WHAT, Channel  # noqa: E402

CHUNK_ROWS = 8195


def mixed48(mbe):
    chans = [Channel(mbe, c) for c in range(48)]
    pending = 1 + np.arange(48) * 5 % 9
    return chans, [int(k) for k in pending], False


def chunks(mbe):
    imbe = soft_mix.frames(0, 44, 128, tag=71).reshape(44, 128, -1, 2)
    ambe = soft_mix.frames(1, 21, 128, tag=72).reshape(21, 128, -1, 2)
    chans = [Channel(mbe, c, codec=0, soft=False, short=c % 2 == 1, cells=imbe[c]) for c in range(43)]
    chans += [Channel(mbe, 43 + k, codec=1, soft=False, short=(43 + k) % 2 == 1, cells=ambe[k]) for k in range(21)]
    chans.append(Channel(mbe, 64, codec=0, soft=False, short=False, cells=imbe[43, :3]))
    pending = [ch.T for ch in chans]
    assert sum(pending) == CHUNK_ROWS and -(-CHUNK_ROWS // 4) * 3 + 2048 == CHUNK_ROWS
    return chans, pending, True


SCENARIOS = {"mixed48": mixed48, "chunks": chunks}


def main(name):
    mbe = shim_lib.load()
    want, pending, round_robin = SCENARIOS[name](mbe)
    for ch, k in zip(want, pending):   # synchronous: each channel alone (it owns the thread's RNG state like a queued channel its copy)
        for _ in range(k):
            ch.call(mbe)
    status = 0
    for mode in (0, 1):
        got, _, _ = SCENARIOS[name](mbe)
        assert mbe.mbe_batchBegin(mode | MBE_BATCH_QUEUE_SOFT) == 0
        try:
            if round_robin:   # frame t of every channel that has one, then frame t + 1
                for t in range(max(pending)):
                    for ch, k in zip(got, pending):
                        if t < k:
                            ch.call(mbe)
            else:
                for ch, k in zip(got, pending):
                    for _ in range(k):
                        ch.call(mbe)
            assert mbe.mbe_batchPending() == sum(pending)
            assert mbe.mbe_flush() == sum(pending)
        finally:
            assert mbe.mbe_batchEnd() >= 0
        bad = [f"channel {a.c} (codec {a.codec}, soft {a.soft}) {what}" for a, b in zip(want, got)
               for what, x, y in zip(WHAT, a.outputs(), b.outputs()) if x != y]
        bad += [f"channel {b.c} returned {sorted(set(b.rets))}" for b in got if any(r != 0 for r in b.rets)]
        print(mode, "ok" if not bad else "differs: " + "; ".join(bad), flush=True)
        status |= bool(bad)
    return status


if __name__ == "__main__":
    sys.exit(main(sys.argv[1]))
