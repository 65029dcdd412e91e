#!/usr/bin/env python3
"""agc_bench.py [--kernel | --sessions] [--rows N] [--steps N] [--submits N] [--rounds R] -- what levelled rows (include/mbx_agc.h)
cost beside the two launches they sit next to behind a step.  Built like hold_bench.py, whose rows and helpers it uses.

The references are mbx_pcm_compand and mbx_pcm_levels of the same library on the same rows, measured in the same process: windows
alternate, `rounds` rounds, per form the best, the median and the spread (worst - best).

--kernel    HIP-event times, `steps` launches a window: mbx_pcm_agc out of place and in place at rows x 1 (65,536), rows / 16 x 16 and
            16 * rows x 1 (1,048,576), beside mbx_pcm_compand and mbx_pcm_levels on the same rows.  The launch moves 640 B per row where compand
            moves 480: the yardstick is 1.33 x compand's median plus the spread of compand's own windows.  The first rows of every
            shape are compared with agc.step first.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, pinned buffers in and out; levelled
            int16 rows out only against plain int16 rows out only, and levelled gated buses of 8 out only against unlevelled ones.
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

from levels_bench import T_OPEN, device_rows, report  # noqa: E402
from mixdown_bench import dealt  # noqa: E402

LOUDEST = 3


def _agc():
    from mbelib_neo_amd import agc

    return agc.Agc(8000, 200, 512, 8192, 64, 32, 5, 0)


def kernel(rows, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, agc, decoder, pcm8

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    a = _agc()
    step, info, keep = {}, {}, []
    for n, T in ((rows, 1), (max(rows // 16, 1), 16), (rows * 16, 1)):
        total = n * T
        x = device_rows(total)
        y = torch.empty_like(x)
        scratch = x.clone()   # the in-place launches level their own copy over and over
        out8 = torch.empty(total * 160, dtype=torch.uint8, device="cuda")
        lv = torch.empty((total, 16), dtype=torch.uint8, device="cuda")
        state = agc.AgcState(n)
        keep.append(state)
        check = min(n, 64)
        _native.check(L.mbx_pcm_agc(C.addressof(a), state.handle, None, n, T, x.data_ptr(), y.data_ptr(), strm), "mbx_pcm_agc")
        torch.cuda.synchronize()
        want, st, _ = agc.step(x[:check * T].cpu().numpy(), T, a, agc.fresh_state(check))
        assert y[:check * T].cpu().numpy().tobytes() == want.tobytes() and state.get(0, check, strm).tobytes() == st.tobytes(), (n, T)
        shape = f"{n} x {T}"
        step[f"agc {shape}"] = lambda n=n, T=T, x=x, y=y, s=state: L.mbx_pcm_agc(C.addressof(a), s.handle, None, n, T, x.data_ptr(), y.data_ptr(), strm)
        step[f"agc in place {shape}"] = lambda n=n, T=T, z=scratch, s=state: L.mbx_pcm_agc(C.addressof(a), s.handle, None, n, T, z.data_ptr(), z.data_ptr(), strm)
        step[f"compand ulaw {shape}"] = lambda total=total, x=x, o=out8: L.mbx_pcm_compand(pcm8.LAW_ULAW, x.data_ptr(), total, o.data_ptr(), strm)
        step[f"levels {shape}"] = lambda total=total, x=x, o=lv: L.mbx_pcm_levels(x.data_ptr(), total, o.data_ptr(), strm)
        for f, per_row in (("agc", 640), ("agc in place", 640), ("compand ulaw", 480), ("levels", 336)):
            info[f"{f} {shape}"] = {"rows": total, "entries": n, "frames_per_entry": T, "bytes_moved_per_launch": per_row * total + (8 * n if "agc" in f else 0)}
    report("kernel", step, info, steps, rounds)
    for k in reversed(keep):
        k.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, agc, decoder, framegen, levels, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    plan = mixdown.Plan(*dealt(np.random.default_rng(9), S, 8))
    state = agc.AgcState(S)
    a, gate = _agc(), levels.Gate(T_OPEN, LOUDEST)
    forms = ("pcm16 rows", "pcm16 rows levelled", "buses of 8 pcm16 gated {t,3}", "buses of 8 pcm16 gated {t,3} levelled")
    out = L.mbx_host_alloc(S * 320)

    def run(s, f, count):
        for _ in range(count):
            if "levelled" in f:
                _native.check(L.mbx_session_next_agc(s, C.addressof(a), state.handle), "next_agc")
            if "buses" in f:
                _native.check(L.mbx_session_next_mixdown_gated(s, plan.handle, 0, C.addressof(gate), out), "next_mixdown_gated")
            _native.check(L.mbx_session_submit(s, 1, pin, None if "buses" in f else out, None, None), "submit")
        _native.check(L.mbx_session_wait(s), "wait")

    def window(f, count):
        """ONE session alive at a time, made for its window (hold_bench.py says why)"""
        s = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(s), 0, S, S, (16 | 32) if "buses" in f else 1), "create")
        run(s, f, 4)
        t0 = time.perf_counter()
        run(s, f, count)
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
                          "bytes_out_per_submit": plan.buses * 320 if "buses" in f else S * 320, "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2),
                          "best_Mframes_per_s": round(r[-1] / 1e6, 2), "spread_Mframes_per_s": round((r[-1] - r[0]) / 1e6, 2), "rounds": rounds}), flush=True)
    L.mbx_host_free(out)
    state.close()
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
