#!/usr/bin/env python3
"""filter_bench.py [--kernel | --sessions] [--rows N] [--steps N] [--submits N] [--rounds R] -- what filtered rows
(include/mbx_filter.h) cost beside the launch they are measured against.  Built like agc_bench.py, whose rows and helpers it uses.

The references are mbx_pcm_agc and mbx_pcm_compand of the same library on the same rows, measured in the same process: windows
alternate, `rounds` rounds, per form the best, the median and the spread (worst - best).

--kernel    HIP-event times, `steps` launches a window: mbx_pcm_filter at S = 1, 2, 4 (highpass(200, S)), out of place and in place,
            at rows x 1 (65,536), rows / 16 x 16, 16 * rows x 1 (1,048,576) and rows / 8 x 1 (8,192: a bus-sized launch), beside
            mbx_pcm_agc and mbx_pcm_compand on the same rows.  The AGC moves the same bytes with the same walk over T: what the filter
            adds over it is its serial chain, 160 T S section steps a lane.  The first rows of every shape are compared with
            filters.step first.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, pinned buffers in and out; int16
            rows out only, filtered rows out only, and filtered + levelled gated buses of 8 out only against unfiltered ones.
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

from agc_bench import LOUDEST, _agc  # noqa: E402
from levels_bench import T_OPEN, device_rows, report  # noqa: E402
from mixdown_bench import dealt  # noqa: E402

SECTIONS = (1, 2, 4)


def kernel(rows, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, agc, decoder, filters, pcm8

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    a = _agc()
    filts = {S: filters.highpass(200, S) for S in SECTIONS}
    step, info, keep = {}, {}, []
    for n, T in ((rows, 1), (max(rows // 16, 1), 16), (rows * 16, 1), (max(rows // 8, 1), 1)):
        total = n * T
        x = device_rows(total)
        y = torch.empty_like(x)
        scratch = x.clone()   # the in-place launches filter their own copy over and over
        out8 = torch.empty(total * 160, dtype=torch.uint8, device="cuda")
        shape = f"{n} x {T}"
        check = min(n, 130)
        for S in SECTIONS:
            f = filts[S]
            state = filters.FilterState(n)
            keep.append(state)
            _native.check(L.mbx_pcm_filter(C.addressof(f), state.handle, None, n, T, x.data_ptr(), y.data_ptr(), strm), "mbx_pcm_filter")
            torch.cuda.synchronize()
            want, st = filters.step(f, filters.fresh_state(check), T, x[:check * T].cpu().numpy())
            assert y[:check * T].cpu().numpy().tobytes() == want.tobytes() and state.get(0, check, strm).tobytes() == st.tobytes(), (n, T, S)
            step[f"filter S={S} {shape}"] = lambda n=n, T=T, x=x, y=y, s=state, f=f: L.mbx_pcm_filter(C.addressof(f), s.handle, None, n, T, x.data_ptr(), y.data_ptr(), strm)
            step[f"filter S={S} in place {shape}"] = lambda n=n, T=T, z=scratch, s=state, f=f: L.mbx_pcm_filter(C.addressof(f), s.handle, None, n, T, z.data_ptr(),
                                                                                                               z.data_ptr(), strm)
            for name in (f"filter S={S} {shape}", f"filter S={S} in place {shape}"):
                info[name] = {"rows": total, "entries": n, "frames_per_entry": T, "sections": S, "bytes_moved_per_launch": 640 * total + 64 * n,
                              "section_steps_per_lane": 160 * T * S}
        astate = agc.AgcState(n)
        keep.append(astate)
        step[f"agc {shape}"] = lambda n=n, T=T, x=x, y=y, s=astate: L.mbx_pcm_agc(C.addressof(a), s.handle, None, n, T, x.data_ptr(), y.data_ptr(), strm)
        step[f"compand ulaw {shape}"] = lambda total=total, x=x, o=out8: L.mbx_pcm_compand(pcm8.LAW_ULAW, x.data_ptr(), total, o.data_ptr(), strm)
        info[f"agc {shape}"] = {"rows": total, "entries": n, "frames_per_entry": T, "bytes_moved_per_launch": 640 * total + 8 * n}
        info[f"compand ulaw {shape}"] = {"rows": total, "entries": n, "frames_per_entry": T, "bytes_moved_per_launch": 480 * total}
    report("kernel", step, info, steps, rounds)
    for k in reversed(keep):
        k.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, agc, decoder, filters, framegen, levels, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    plan = mixdown.Plan(*dealt(np.random.default_rng(9), S, 8))
    fstate, astate = filters.FilterState(S), agc.AgcState(S)
    f, a, gate = filters.highpass(200, 2), _agc(), levels.Gate(T_OPEN, LOUDEST)
    forms = ("pcm16 rows", "pcm16 rows filtered", "buses of 8 pcm16 gated {t,3} levelled", "buses of 8 pcm16 gated {t,3} filtered and levelled")
    out = L.mbx_host_alloc(S * 320)

    def run(s, form, count):
        for _ in range(count):
            if "filtered" in form:
                _native.check(L.mbx_session_next_filter(s, C.addressof(f), fstate.handle), "next_filter")
            if "levelled" in form:
                _native.check(L.mbx_session_next_agc(s, C.addressof(a), astate.handle), "next_agc")
            if "buses" in form:
                _native.check(L.mbx_session_next_mixdown_gated(s, plan.handle, 0, C.addressof(gate), out), "next_mixdown_gated")
            _native.check(L.mbx_session_submit(s, 1, pin, None if "buses" in form else out, None, None), "submit")
        _native.check(L.mbx_session_wait(s), "wait")

    def window(form, count):
        """ONE session alive at a time, made for its window (hold_bench.py says why)"""
        s = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(s), 0, S, S, (16 | 32) if "buses" in form else 1), "create")
        run(s, form, 4)
        t0 = time.perf_counter()
        run(s, form, count)
        rate = S * count / (time.perf_counter() - t0)
        L.mbx_session_destroy(s)
        return rate

    rates = {form: [] for form in forms}
    for _ in range(rounds):
        for form in forms:
            rates[form].append(window(form, submits))
    for form in forms:
        r = sorted(rates[form])
        print(json.dumps({"mode": "sessions", "form": form, "streams": S, "submits_per_window": submits, "host_threads": 1,
                          "bytes_out_per_submit": plan.buses * 320 if "buses" in form else S * 320, "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2),
                          "best_Mframes_per_s": round(r[-1] / 1e6, 2), "spread_Mframes_per_s": round((r[-1] - r[0]) / 1e6, 2), "rounds": rounds}), flush=True)
    L.mbx_host_free(out)
    fstate.close()
    astate.close()
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
