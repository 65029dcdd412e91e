#!/usr/bin/env python3
"""llr_gather_bench.py [--gathers | --sessions] [--streams S] [--steps N] [--rounds R] -- what soft bursts as LLRs cost next to per-bit
soft bursts (include/mbx_burst.h, mbx_burst_schedule_create_llr).

The two SHAPES of tools/burst_bench.py: "dmr" = AMBE+2, 3 frames in 264 bits; "ldu" = IMBE, 9 frames in 1,728 bits; random
schedules without an inversion sequence, S bursts (default 65,536).  The same received LLRs in three forms: host-converted per-bit
cells (the instance burst_gather_soft_kernel<kCellBit, false>), int16 LLRs (<kCellLlr16, true>) and int8 LLRs (<kCellLlr8, true>;
the int16 values clipped to int8, so its cells differ: its gather is held to the per-bit gather of ITS converted cells).

--gathers   HIP-event time of mbx_deinterleave_soft alone, `steps` launches a window, the three forms' windows alternating, `rounds`
            rounds: per form the best, the median and the spread (worst - best) over the rounds, and the bytes a launch reads.
--sessions  frames/s of sessions fed with soft bursts of each form (mbx_session_submit_bursts_soft; pinned input, int16 PCM out),
            1 and 8 host threads, each thread with its own session of S / threads streams; the forms' windows alternate, the better
            of two each.
Needs a GPU; prints one JSON line per measurement.  Development aid."""
import argparse
import ctypes as C
import json
import os
import sys
import threading
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPES = {"dmr": (1, 3, 264), "ldu": (0, 9, 1728)}
FORMS = ("per-bit", "llr16", "llr8")


def make(shape, n, seed=1):
    """{form: (schedule, bursts as the form's array)} of one random schedule and one set of received LLRs"""
    from mbelib_neo_amd import bursts as B, decoder

    codec, F, bits = SHAPES[shape]
    rng = np.random.default_rng(seed)
    arrays = B.random_schedule(codec, F, bits, rng)
    llr16 = rng.integers(-400, 401, size=(n, bits)).astype(np.int16)
    llr8 = llr16.clip(-128, 127).astype(np.int8)
    return {"per-bit": (arrays.in_form(B.FORM_PACKED, device=True), decoder.soft_bits_from_llr(llr16)),
            "llr16": (arrays.in_form(B.FORM_LLR16, device=True), llr16),
            "llr8": (arrays.in_form(B.FORM_LLR8, device=True), llr8)}


def timed(step, steps):
    import torch

    for _ in range(3):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def gathers(S, steps, rounds):
    import torch
    from mbelib_neo_amd import bursts as B, decoder

    decoder.ensure_init(0)
    for shape in SHAPES:
        made = make(shape, S)
        d_in = {f: torch.from_numpy(np.ascontiguousarray(made[f][1]).reshape(-1).view(np.uint8)).cuda() for f in FORMS}
        want = B.deinterleave(made["per-bit"][0], d_in["per-bit"], soft=True)
        assert torch.equal(B.deinterleave(made["llr16"][0], d_in["llr16"], soft=True), want)
        cells8 = torch.from_numpy(decoder.soft_bits_from_llr(made["llr8"][1].astype(np.int16)).reshape(-1)).cuda()
        assert torch.equal(B.deinterleave(made["llr8"][0], d_in["llr8"], soft=True), B.deinterleave(made["per-bit"][0], cells8, soft=True))
        out = torch.empty_like(want)
        step = {f: (lambda f=f: B.deinterleave(made[f][0], d_in[f], soft=True, out=out)) for f in FORMS}
        times = {f: [] for f in FORMS}
        for _ in range(rounds):
            for f in FORMS:
                times[f].append(timed(step[f], steps))
        for f in FORMS:
            t = sorted(times[f])
            print(json.dumps({"mode": "gathers", "shape": shape, "form": f, "bursts": S, "bytes_read_per_launch": int(d_in[f].numel()),
                              "bytes_written_per_launch": int(out.numel()), "best_us": round(1e3 * t[0], 2), "median_us": round(1e3 * t[len(t) // 2], 2),
                              "spread_us": round(1e3 * (t[-1] - t[0]), 2), "rounds": rounds, "launches_per_round": steps}), flush=True)
            made[f][0].close()


def sessions(S, steps):
    from mbelib_neo_amd import _native, decoder

    decoder.ensure_init(0)
    L = _native.lib()
    for shape in SHAPES:
        codec, F, _ = SHAPES[shape]
        for threads in (1, 8):
            per = S // threads
            made = make(shape, per)
            rates = {}
            for f in FORMS + FORMS:   # (twice: the better of two windows)
                sched, data = made[f]
                raw = np.ascontiguousarray(data).reshape(-1).view(np.uint8)
                work = []
                for _ in range(threads):
                    h = C.c_void_p()
                    _native.check(L.mbx_session_create(C.byref(h), codec, per, per * F, 1), "create")
                    pin = L.mbx_host_alloc(raw.size)
                    np.ctypeslib.as_array((C.c_uint8 * raw.size).from_address(pin))[:] = raw
                    pcm = L.mbx_host_alloc(per * F * 320)
                    work.append((h, pin, pcm))

                def run(h, pin, pcm, count):
                    import torch

                    torch.cuda.set_device(0)
                    for _ in range(count):
                        _native.check(L.mbx_session_submit_bursts_soft(h, sched.handle, per, None, pin, pcm, None, None), "submit")
                    _native.check(L.mbx_session_wait(h), "wait")

                for w in work:
                    run(*w, 2)
                ts = [threading.Thread(target=run, args=(*w, steps)) for w in work]
                t0 = time.perf_counter()
                for t in ts:
                    t.start()
                for t in ts:
                    t.join()
                rates[f] = max(rates.get(f, 0.0), threads * per * F * steps / (time.perf_counter() - t0))
                for h, pin, pcm in work:
                    L.mbx_session_destroy(h)
                    L.mbx_host_free(pin)
                    L.mbx_host_free(pcm)
            print(json.dumps({"mode": "sessions", "shape": shape, "streams": per * threads, "host_threads": threads,
                              **{f + "_Mframes_per_s": round(rates[f] / 1e6, 2) for f in FORMS},
                              **{f + "_input_bytes_per_burst": int(np.ascontiguousarray(made[f][1]).nbytes // per) for f in FORMS}}), flush=True)
            for f in FORMS:
                made[f][0].close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--gathers", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=400)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if a.gathers or not a.sessions:
        gathers(a.streams, a.steps, a.rounds)
    if a.sessions:
        sessions(a.streams, a.steps)
