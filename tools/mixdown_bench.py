#!/usr/bin/env python3
"""mixdown_bench.py [--kernel | --sessions] [--rows N] [--sizes a,b,..] [--steps N] [--submits N] [--rounds R] -- what mix-down out
(include/mbx_mixdown.h) costs and what it saves.

--kernel    HIP-event time of mbx_mixdown alone over `rows` int16 rows (65,536), all three output forms.  The rows are dealt at random
            into buses of one size -- 2, 8, 32 and sizes round the library's default split (mixdown.LONG_ABOVE) --, every row in
            exactly one bus, gains random; each size through BOTH kernel forms (mbx_mixdown_plan_create_split: long_above = 4096, all
            short; long_above = 1, all long), which is how the split is found.  Then one 4,096-input bus beside buses of 8 ("allcall"):
            the default split against all short.  Next to them mbx_pcm_compand and mbx_floattoshort on the same rows.  `steps`
            launches a window, the windows alternating, `rounds` rounds: per form the best, the median and the spread (worst - best)
            over the rounds.  The first buses of every plan are compared with mixdown.mix first.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, `submits` submits a window, pinned
            buffers in and out; int16 rows out only (a session made without MBX_SESSION_MIXDOWN: the path of a library without the
            feature) against buses out only (8 and 32 rows per bus, as int16 and as mu-law; the submit's pcm16 is NULL), windows
            alternating in one process, `rounds` rounds: median, best and spread of each form's windows.
Needs a GPU; prints one JSON line per measurement.  Development aid."""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FORM_NAMES = {0: "pcm16", 1: "ulaw", 2: "alaw"}


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


def summary(times):
    t = sorted(times)
    return {"best_us": round(1e3 * t[0], 2), "median_us": round(1e3 * statistics.median(t), 2), "spread_us": round(1e3 * (t[-1] - t[0]), 2)}


def dealt(rng, rows, size):
    """every row in exactly one bus of `size` rows (the last rows left over are in none), at random, with random gains"""
    n = rows // size
    row = rng.permutation(rows)[:n * size].astype(np.int32)
    off = (np.arange(n + 1, dtype=np.int64) * size).astype(np.int32)
    gain = rng.integers(-8192, 8193, size=row.size, dtype=np.int64).astype(np.int16)
    return off, row, gain


def allcall(rng, rows):
    """one bus of 4,096 rows in front of buses of 8 over the others"""
    off, row, gain = dealt(rng, rows - 4096, 8)
    every = rng.permutation(rows)[:4096].astype(np.int32)
    return (np.concatenate([[0], off + 4096]).astype(np.int32), np.concatenate([every, row]),
            np.concatenate([rng.integers(-600, 601, size=4096, dtype=np.int64).astype(np.int16), gain]))


def kernel(rows, sizes, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, mixdown, pcm8

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    n = rows * 160
    pcmf = (torch.rand(n, device="cuda") - 0.5) * 9000.0   # (mbe_floattoshort scales by 7: the whole int16 range, clipping included)
    pcm16 = torch.empty(n, dtype=torch.int16, device="cuda")
    out16 = torch.empty(n, dtype=torch.int16, device="cuda")
    out8 = torch.empty(n, dtype=torch.uint8, device="cuda")
    _native.check(L.mbx_floattoshort(pcmf.data_ptr(), pcm16.data_ptr(), rows, strm), "mbx_floattoshort")
    torch.cuda.synchronize()
    host = pcm16.cpu().numpy().reshape(rows, 160)
    rng = np.random.default_rng(7)
    step, info, plans = {}, {}, []
    step["floattoshort"] = lambda: L.mbx_floattoshort(pcmf.data_ptr(), pcm16.data_ptr(), rows, strm)
    step["compand ulaw"] = lambda: L.mbx_pcm_compand(pcm8.LAW_ULAW, pcm16.data_ptr(), rows, out8.data_ptr(), strm)
    info["floattoshort"], info["compand ulaw"] = {"bytes_moved_per_launch": 6 * n}, {"bytes_moved_per_launch": 3 * n}

    def add(name, csr, above, forms):
        off, row, gain = csr
        plan = mixdown.Plan(off, row, gain, long_above=above)
        plans.append(plan)
        check = min(plan.buses, 48)
        for form in forms:
            out = out16 if form == mixdown.PCM16 else out8
            _native.check(L.mbx_mixdown(plan.handle, form, pcm16.data_ptr(), rows, out.data_ptr(), strm), "mbx_mixdown")
            torch.cuda.synchronize()
            got = out[:check * 160].cpu().numpy().reshape(check, 160)
            assert got.tobytes() == mixdown.mix(host, off[:check + 1], row, gain, form).tobytes(), (name, form)
            key = f"{name} {FORM_NAMES[form]}"
            step[key] = lambda plan=plan, form=form, out=out: L.mbx_mixdown(plan.handle, form, pcm16.data_ptr(), rows, out.data_ptr(), strm)
            info[key] = {"buses": plan.buses, "long_buses": plan.long_buses, "inputs": int(off[-1]),
                         "bytes_moved_per_launch": int(off[-1]) * 320 + plan.buses * 160 * (2 if form == mixdown.PCM16 else 1)}

    for size in sizes:
        csr = dealt(rng, rows, size)
        for kind, above in (("short", 4096), ("long", 1)):
            # every form at the sizes the issue names, int16 alone at the sizes that only look for the split
            add(f"size {size} {kind}", csr, above, mixdown.FORMS if size in (2, 8, 32) else (mixdown.PCM16,))
    csr = allcall(rng, rows)
    add("allcall default", csr, None, mixdown.FORMS)
    add("allcall short", csr, 4096, (mixdown.PCM16,))
    times = {f: [] for f in step}
    for _ in range(rounds):
        for f in step:
            times[f].append(timed(step[f], steps))
    for f in step:
        print(json.dumps({"mode": "kernel", "form": f, "rows": rows, **info[f], **summary(times[f]), "rounds": rounds, "launches_per_round": steps}), flush=True)
    for p in plans:
        p.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, decoder, framegen, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    rng = np.random.default_rng(9)
    # name: (outputs, rows per bus or None, form)
    forms = {"pcm16 rows": (1, None, 0), "buses of 8 pcm16": (16, 8, 0), "buses of 32 pcm16": (16, 32, 0), "buses of 8 ulaw": (16, 8, 1)}
    work = {}
    for f, (outputs, per, form) in forms.items():
        h = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(h), 0, S, S, outputs), "create")
        plan = mixdown.Plan(*dealt(rng, S, per)) if per else None
        out_bytes = S * 320 if not per else plan.buses * 160 * (2 if form == 0 else 1)
        work[f] = (h, plan, form, L.mbx_host_alloc(out_bytes), out_bytes)

    def window(f, count):
        h, plan, form, out, _ = work[f]
        t0 = time.perf_counter()
        for _ in range(count):
            if plan:
                _native.check(L.mbx_session_next_mixdown(h, plan.handle, form, out), "next_mixdown")
                _native.check(L.mbx_session_submit(h, 1, pin, None, None, None), "submit")
            else:
                _native.check(L.mbx_session_submit(h, 1, pin, out, None, None), "submit")
        _native.check(L.mbx_session_wait(h), "wait")
        return S * count / (time.perf_counter() - t0)

    rates = {f: [] for f in forms}
    for f in forms:
        window(f, 4)
    for _ in range(rounds):
        for f in forms:
            rates[f].append(window(f, submits))
    for f in forms:
        r = sorted(rates[f])
        print(json.dumps({"mode": "sessions", "form": f, "streams": S, "submits_per_window": submits, "host_threads": 1,
                          "bytes_out_per_submit": work[f][4], "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2),
                          "best_Mframes_per_s": round(r[-1] / 1e6, 2), "spread_Mframes_per_s": round((r[-1] - r[0]) / 1e6, 2), "rounds": rounds}), flush=True)
    for h, plan, _, out, _ in work.values():
        L.mbx_session_destroy(h)
        if plan:
            plan.close()
        L.mbx_host_free(out)
    L.mbx_host_free(pin)


if __name__ == "__main__":
    from mbelib_neo_amd import mixdown as _m

    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--sizes", default=",".join(str(s) for s in sorted({2, 4, 8, 12, 16, 24, 32, _m.LONG_ABOVE, _m.LONG_ABOVE + 1, 64, 96, 128, 256})))
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--submits", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.kernel or not a.sessions:
        kernel(a.rows, [int(s) for s in a.sizes.split(",")], a.steps, a.rounds)
    if a.sessions:
        sessions(a.rows, a.submits, a.rounds)
