#!/usr/bin/env python3
"""resample_bench.py [--kernel | --sessions] [--rows N] [--steps N] [--submits N] [--rounds R] -- what wide rows
(include/mbx_resample.h) cost beside the launch they are measured against.  Built like agc_bench.py, whose rows and helpers it uses.

The reference is mbx_pcm_compand of the same library on the same rows, measured in the same process: windows alternate, `rounds`
rounds, per form the best, the median and the spread (worst - best).

--kernel    HIP-event times, `steps` launches a window: mbx_pcm_resample at rows x 1 (65,536) for L in 2, 6 and K in 16, 32, at
            rows / 8 x 1 (8,192: bus-sized) and at rows / 16 x 16 (4,096 x 16), beside mbx_pcm_compand on the same rows.  The launch
            moves 320 + 320 L bytes per row where compand moves 480: the yardstick is (320 + 320 L) / 480 x compand's median plus the
            spread of compand's own windows, and every resample line says whether it is inside it.  The first rows of every shape are
            compared with resample.step first.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, pinned buffers in and out; held and
            limited buses of 8 out only, at 8 kHz, against the same buses delivered at 48 kHz beside them.
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
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from levels_bench import device_rows, summary, timed  # noqa: E402
from mixdown_bench import dealt  # noqa: E402


def kernel(rows, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, pcm8, resample

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    step, info, keep, yard = {}, {}, [], {}
    shapes = [(rows, 1, f, k) for f in (2, 6) for k in (16, 32)] + [(max(rows // 8, 1), 1, 6, 16), (max(rows // 16, 1), 16, 6, 16), (max(rows // 16, 1), 16, 2, 16)]
    inputs = {}
    for n, T, factor, K in shapes:
        total = n * T
        if total not in inputs:
            inputs[total] = (device_rows(total), torch.empty(total * 160, dtype=torch.uint8, device="cuda"))
        x, out8 = inputs[total]
        rs = resample.Resample.of(factor, K, resample.design(factor, K))
        y = torch.empty((total, 160 * factor), dtype=torch.int16, device="cuda")
        state = resample.ResampleState(n)
        keep.extend((state, rs))
        check = min(n, 64)
        _native.check(L.mbx_pcm_resample(C.addressof(rs), state.handle, None, n, T, x.data_ptr(), y.data_ptr(), strm), "mbx_pcm_resample")
        torch.cuda.synchronize()
        want, st = resample.step(rs, resample.fresh_state(check), T, x[:check * T].cpu().numpy())
        assert y[:check * T].cpu().numpy().tobytes() == want.tobytes() and state.get(0, check, strm).tobytes() == st.tobytes(), (n, T, factor, K)
        shape = f"{n} x {T}"
        name = f"resample L {factor} K {K} {shape}"
        step[name] = lambda n=n, T=T, x=x, y=y, s=state, rs=rs: L.mbx_pcm_resample(C.addressof(rs), s.handle, None, n, T, x.data_ptr(), y.data_ptr(), strm)
        info[name] = {"rows": total, "entries": n, "frames_per_entry": T, "L": factor, "K": K, "bytes_moved_per_launch": (320 + 320 * factor) * total + 128 * n,
                      "dot_products_per_input_sample": K * factor // 2}
        yard[name] = (f"compand ulaw {shape}", (320 + 320 * factor) / 480.0)
        step[f"compand ulaw {shape}"] = lambda total=total, x=x, o=out8: L.mbx_pcm_compand(pcm8.LAW_ULAW, x.data_ptr(), total, o.data_ptr(), strm)
        info[f"compand ulaw {shape}"] = {"rows": total, "bytes_moved_per_launch": 480 * total}
    times = {f: [] for f in step}
    for _ in range(rounds):
        for f in step:
            times[f].append(timed(step[f], steps))
    got = {f: summary(times[f]) for f in step}
    for f in step:
        line = {"mode": "kernel", "form": f, **info[f], **got[f], "rounds": rounds, "launches_per_round": steps}
        if f in yard:
            ref, ratio = yard[f]
            limit_us = got[ref]["median_us"] * ratio + got[ref]["spread_us"]
            line["yardstick_us"] = round(limit_us, 2)
            line["inside_yardstick"] = bool(got[f]["median_us"] <= limit_us)
        print(json.dumps(line), flush=True)
    for k in reversed(keep):
        if hasattr(k, "close"):
            k.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, decoder, framegen, hold, limit, mixdown, resample

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    plan = mixdown.Plan(*dealt(np.random.default_rng(9), S, 8))
    h, lim = hold.Hold(1000, 500, 3, 3, 5), limit.Limit(20000, 64, 1, 5)
    rs = resample.Resample.of(6, 16, resample.design(6, 16))
    forms = ("buses of 8 held and limited, 8 kHz", "buses of 8 held and limited, 8 kHz and 48 kHz")
    out = L.mbx_host_alloc(plan.buses * 320)
    wide = L.mbx_host_alloc(plan.buses * 320 * 6)

    def run(s, f, count, gs, ls, st):
        for _ in range(count):
            _native.check(L.mbx_session_next_mixdown_held(s, plan.handle, 0, C.addressof(h), gs.handle, out), "next_mixdown_held")
            _native.check(L.mbx_session_next_limit(s, C.addressof(lim), ls.handle), "next_limit")
            if "48 kHz" in f:
                _native.check(L.mbx_session_next_resample(s, C.addressof(rs), st.handle, wide), "next_resample")
            _native.check(L.mbx_session_submit(s, 1, pin, None, None, None), "submit")
        _native.check(L.mbx_session_wait(s), "wait")

    def window(f, count):
        """ONE session alive at a time, made for its window (hold_bench.py says why)"""
        s = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(s), 0, S, S, 16 | 32), "create")
        with hold.GateState(plan) as gs, limit.LimitState(plan.buses) as ls, resample.ResampleState(plan.buses) as st:
            run(s, f, 4, gs, ls, st)
            t0 = time.perf_counter()
            run(s, f, count, gs, ls, st)
            rate = S * count / (time.perf_counter() - t0)
            L.mbx_session_destroy(s)
        return rate

    rates = {f: [] for f in forms}
    for _ in range(rounds):
        for f in forms:
            rates[f].append(window(f, submits))
    for f in forms:
        r = sorted(rates[f])
        print(json.dumps({"mode": "sessions", "form": f, "streams": S, "submits_per_window": submits, "host_threads": 1,
                          "bytes_out_per_submit": plan.buses * 320 * (7 if "48 kHz" in f else 1), "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2),
                          "best_Mframes_per_s": round(r[-1] / 1e6, 2), "spread_Mframes_per_s": round((r[-1] - r[0]) / 1e6, 2), "rounds": rounds}), flush=True)
    L.mbx_host_free(wide)
    L.mbx_host_free(out)
    plan.close()
    L.mbx_host_free(pin)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--submits", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    a_ = ap.parse_args()
    if a_.kernel or not a_.sessions:
        kernel(a_.rows, a_.steps, a_.rounds)
    if a_.sessions:
        sessions(a_.rows, a_.submits, a_.rounds)
