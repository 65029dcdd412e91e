"""Queue mode over several shards, for tests/test_gpu_queue_shards.py: the library reads MBX_DEVICES once per process, so every case
runs in a fresh one.  `python queue_shards_case.py CASE SHARDS` expects MBX_DEVICES to name device 0 SHARDS times, sends the case's
frames through the synchronous per-frame calls once and then through queue mode, and prints one line per state mode it covers:
`MODE ok`, or `MODE differs: ...` naming everything that is not as it should be -- a caller buffer or struct that is not the
synchronous calls' byte for byte, a channel on another shard than (home + k) % SHARDS, a census that does not add up.  Cases:

mixed48  the 48-channel scenario of tests/queue_flush_case.py (four codecs, hard and soft, 1..9 pending frames), ONE flush per state
         mode: channel c on shard c % SHARDS, every shard one flush pass and 48 / SHARDS channels, the rows summing to the frames.
reentry  twelve channels, nine frames each, round-robin in three ticks of three frames with a flush after each, both state modes:
         channel 4 is touched by a direct call after tick 1 (released; it comes back as the 13th channel created), channel 10 is
         released by mbe_batchRelease after tick 2 (back as the 14th), and channel 7 -- a soft channel -- sends the middle frame of
         tick 2 through the hard call, so that the whole batch is flushed twice inside that tick.
threads  four host threads in resident mode, six channels each (ids 100 * t + c), three flushes of three frames: four different
         home shards, channel k of a thread on (home + k) % SHARDS, every thread's bytes those of the synchronous calls.
Test infrastructure."""
import ctypes as C
import os
import sys
import threading

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for d in (HERE, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

import shim_lib  # noqa: E402
from queue_channels import HARD_CALLS, MBE_BATCH_QUEUE_SOFT, WHAT, Channel  # noqa: E402
from queue_flush_case import SCENARIOS  # noqa: E402


class Census(C.Structure):   # mbq_census, include/mbe_neo_shards.h
    _fields_ = [("flush_passes", C.c_longlong), ("rows", C.c_longlong), ("channels", C.c_int), ("resident", C.c_int)]


def bind(mbe):
    """the five reporting functions of include/mbe_neo_shards.h on a library loaded by shim_lib.load()"""
    for name, args in (("mbq_shard_count", []), ("mbq_shard_device", [C.c_int]), ("mbq_thread_home", []), ("mbq_channel_shard", [C.c_void_p]),
                       ("mbq_shard_census", [C.c_int, C.POINTER(Census)])):
        getattr(mbe, name).restype = C.c_int
        getattr(mbe, name).argtypes = args
    return mbe


def census(mbe, shard):
    c = Census()
    assert mbe.mbq_shard_census(shard, C.byref(c)) == 0
    return c.flush_passes, c.rows, c.channels, c.resident


def shard_of(mbe, ch):
    return mbe.mbq_channel_shard(ch.p(ch.st[0]))


def differences(want, got, queued=True):
    bad = [f"channel {a.c} (codec {a.codec}, soft {a.soft}) {what}" for a, b in zip(want, got)
           for what, x, y in zip(WHAT, a.outputs(), b.outputs()) if x != y]
    if queued:
        bad += [f"channel {b.c} returned {sorted(set(b.rets))}" for b in got if any(r != 0 for r in b.rets)]
    return bad


def mixed48(mbe, n):
    want, pending, _ = SCENARIOS["mixed48"](mbe)
    total = sum(pending)
    for ch, k in zip(want, pending):   # synchronous: each channel alone (it owns the thread's RNG state like a queued channel its copy)
        for _ in range(k):
            ch.call(mbe)
    status = 0
    for mode in (0, 1):
        got, _, _ = SCENARIOS["mixed48"](mbe)
        bad = []
        assert mbe.mbe_batchBegin(mode | MBE_BATCH_QUEUE_SOFT) == 0
        try:
            for ch, k in zip(got, pending):   # channel c is the c-th the thread creates
                for _ in range(k):
                    ch.call(mbe)
            where = [shard_of(mbe, ch) for ch in got]
            if where != [c % n for c in range(48)]:
                bad.append(f"channels sit on shards {where}")
            if mbe.mbe_batchPending() != total:
                bad.append(f"{mbe.mbe_batchPending()} frames pending, not {total}")
            ran = mbe.mbe_flush()
            if ran != total:
                bad.append(f"mbe_flush returned {ran}, not {total}")
            seen = [census(mbe, i) for i in range(n)]
            expect = [(1, sum(pending[i::n]), 48 // n, 48 // n if mode == 1 else 0) for i in range(n)]
            if seen != expect or sum(c[1] for c in seen) != total:
                bad.append(f"census {seen}, expected {expect}")
        finally:
            assert mbe.mbe_batchEnd() >= 0
        if any(shard_of(mbe, ch) != -1 for ch in got):
            bad.append("a channel is still known after mbe_batchEnd")
        bad += differences(want, got)
        print(mode, "ok" if not bad else "differs: " + "; ".join(bad), flush=True)
        status |= bool(bad)
    return status


FORM_CHANGE = (7, 4)   # channel 7 sends its frame 4 -- the middle one of tick 2 -- through the hard call


def call_hard(ch, mbe, keep):
    """the next frame of a SOFT channel through the hard-decision call of its codec, on the cells' hard decisions"""
    t, p = ch.t, ch.p
    fn = getattr(mbe, HARD_CALLS[ch.codec] + ("f" if ch.pcm.dtype == np.float32 else ""))
    cells = np.ascontiguousarray(ch.frames[t][..., 0]).astype(np.int8)
    keep.append(cells)
    ch.rets.append(fn(p(ch.pcm[t]), p(ch.res[t:t + 1]), p(cells), p(ch.bits[t]), p(ch.st[0]), p(ch.st[1]), p(ch.st[2])))
    ch.t += 1


def reentry_call(ch, mbe, keep):
    if (ch.c, ch.t) == FORM_CHANGE:
        call_hard(ch, mbe, keep)
    else:
        ch.call(mbe)


def reentry(mbe, n):
    assert n == 3
    from mbelib_neo_amd.layout import PARMS_DTYPE

    keep = []
    want = [Channel(mbe, c) for c in range(12)]
    assert want[FORM_CHANGE[0]].soft
    for ch in want:   # synchronous: each channel alone
        for _ in range(9):
            reentry_call(ch, mbe, keep)
    status = 0
    for mode in (0, 1):
        got = [Channel(mbe, c) for c in range(12)]
        scratch = np.zeros(1, dtype=PARMS_DTYPE)
        bad = []

        def expect_shards(when, where):
            seen = {ch.c: shard_of(mbe, ch) for ch in got}
            if seen != where:
                bad.append(f"{when}: channels sit on shards {seen}, expected {where}")

        where = {c: c % 3 for c in range(12)}
        assert mbe.mbe_batchBegin(mode | MBE_BATCH_QUEUE_SOFT) == 0
        try:
            for tick in range(3):
                ran = 0
                for _ in range(3):
                    for ch in got:
                        before = mbe.mbe_batchPending()
                        reentry_call(ch, mbe, keep)
                        after = mbe.mbe_batchPending()
                        if after != before + 1:   # the call ran what was pending first: the WHOLE batch
                            if after != 1 or ch.c != FORM_CHANGE[0]:
                                bad.append(f"tick {tick}: {before} frames pending before a call of channel {ch.c}, {after} after")
                            ran += before
                expect_shards(f"tick {tick}, queued", where)
                ran += mbe.mbe_flush()
                if ran != 36:
                    bad.append(f"tick {tick}: {ran} frames ran, not 36")
                if tick == 0:   # a direct call on a struct of channel 4 (shard 1): the channel leaves the batch
                    mbe.mbe_moveMbeParms(got[4].p(got[4].st[0]), got[4].p(scratch))
                    where[4] = -1
                    expect_shards("after the direct call", where)
                    where[4] = 12 % 3   # the 13th channel the thread creates
                if tick == 1:
                    if mbe.mbe_batchRelease(got[10].p(got[10].st[0])) != 0:
                        bad.append("mbe_batchRelease failed")
                    where[10] = -1
                    expect_shards("after mbe_batchRelease", where)
                    where[10] = 13 % 3
            seen = [census(mbe, i) for i in range(3)]
            # tick 0: one pass per shard; tick 1: three (two forced by channel 7, one mbe_flush), every shard having frames each time; tick 2: one
            if [c[0] for c in seen] != [5, 5, 5] or sum(c[1] for c in seen) != 108 or sum(c[2] for c in seen) != 12:
                bad.append(f"census {seen}")
        finally:
            assert mbe.mbe_batchEnd() >= 0
        bad += differences(want, got, queued=False)
        bad += [f"channel {b.c} returned {sorted(set(b.rets))}" for b in got if any(r != 0 for r in b.rets)]
        print(mode, "ok" if not bad else "differs: " + "; ".join(bad), flush=True)
        status |= bool(bad)
    return status


def threads(mbe, n):
    assert n == 4
    ids = [[100 * t + c for c in range(6)] for t in range(4)]
    want = [[Channel(mbe, i) for i in mine] for mine in ids]
    for mine in want:   # synchronous, on this thread (the first to use the library: thread 0, home shard 0)
        for ch in mine:
            for _ in range(9):
                ch.call(mbe)
    got = [[Channel(mbe, i) for i in mine] for mine in ids]
    report = [None] * 4

    def work(t):
        bad = []
        try:
            home = mbe.mbq_thread_home()
            assert mbe.mbe_batchBegin(1 | MBE_BATCH_QUEUE_SOFT) == 0
            try:
                for tick in range(3):
                    for _ in range(3):
                        for ch in got[t]:
                            ch.call(mbe)
                    where = [shard_of(mbe, ch) for ch in got[t]]
                    if where != [(home + k) % n for k in range(6)]:
                        bad.append(f"tick {tick}: home {home}, channels on shards {where}")
                    ran = mbe.mbe_flush()
                    if ran != 18:
                        bad.append(f"tick {tick}: mbe_flush returned {ran}")
                seen = [census(mbe, i) for i in range(n)]
                if sum(c[1] for c in seen) != 54 or sum(c[2] for c in seen) != 6 or sum(c[3] for c in seen) != 6:
                    bad.append(f"census {seen}")
            finally:
                assert mbe.mbe_batchEnd() >= 0
            report[t] = (home, bad)
        except BaseException as e:   # (reported by the main thread)
            report[t] = (-1, bad + [f"{type(e).__name__}: {e}"])

    pool = [threading.Thread(target=work, args=(t,)) for t in range(4)]
    for th in pool:
        th.start()
    for th in pool:
        th.join()
    bad = [f"thread {t}: {b}" for t in range(4) for b in report[t][1]]
    homes = sorted(r[0] for r in report)
    if homes != [0, 1, 2, 3]:
        bad.append(f"home shards {[r[0] for r in report]}")
    if mbe.mbq_thread_home() != 0:
        bad.append("the first thread's home is not shard 0")
    for t in range(4):
        bad += [f"thread {t}: {b}" for b in differences(want[t], got[t])]
    print(1, "ok" if not bad else "differs: " + "; ".join(bad), flush=True)
    return int(bool(bad))


CASES = {"mixed48": mixed48, "reentry": reentry, "threads": threads}


def main(name, shards):
    mbe = bind(shim_lib.load())
    n = mbe.mbq_shard_count()
    assert n == shards, f"{n} shards, not {shards}: MBX_DEVICES={os.environ.get('MBX_DEVICES')!r}"
    assert [mbe.mbq_shard_device(i) for i in range(-1, n + 1)] == [-1] + [0] * n + [-1]
    return CASES[name](mbe, n)


if __name__ == "__main__":
    sys.exit(main(sys.argv[1], int(sys.argv[2])))
