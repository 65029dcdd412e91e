#!/usr/bin/env python3
"""hold_bench.py [--kernel | --sessions] [--rows N] [--steps N] [--submits N] [--rounds R] -- what the held gate (include/mbx_hold.h)
costs beside the stateless gate it extends (include/mbx_levels.h).  Built like levels_bench.py, whose rows and helpers it uses.

The reference is mbx_mixdown_gated of the same library, measured in the same process: windows alternate, `rounds` rounds, per form the
best, the median and the spread (worst - best).

--kernel    HIP-event times, `steps` launches a window.  `rows` rows (65,536) dealt into buses of 8 and of 32 (the default split: short
            and long kernel form) under "open at t, the 3 loudest", and one 4,096-input bus beside buses of 8 ("allcall") under "the 3
            loudest": mbx_pcm_levels + mbx_mixdown_gated against mbx_pcm_levels + mbx_mixdown_held {t, t / 2, 2, 3, 5}, and either
            mix-down launch set alone.  Held runs twice: on the same rows every launch (after the first every input is steady or off:
            no ramp is computed), and on two sets of rows in turn whose talkers differ ("churn": inputs rise and fall in every launch).
            The first buses of every case are compared with hold.step first.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, pinned buffers in and out; held buses
            of 8 out only against gated buses of 8 out only.
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
from mixdown_bench import allcall, dealt  # noqa: E402

HANG, RAMP_LOG2, LOUDEST = 2, 5, 3


def kernel(rows, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, hold, levels, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    pcm16 = device_rows(rows)
    other = torch.roll(pcm16, 1, 0).contiguous()   # every bus gets other talkers
    out16 = torch.empty(rows * 160, dtype=torch.int16, device="cuda")
    lv, lv_other = (torch.empty((rows, 16), dtype=torch.uint8, device="cuda") for _ in range(2))
    host = pcm16.cpu().numpy()
    rng = np.random.default_rng(7)
    step, info, keep = {}, {}, []
    cases = {"buses of 8": (dealt(rng, rows, 8), T_OPEN), "buses of 32": (dealt(rng, rows, 32), T_OPEN), "allcall": (allcall(rng, rows), 0)}
    for name, ((off, row, gain), t) in cases.items():
        plan = mixdown.Plan(off, row, gain)
        state = hold.GateState(plan)
        keep += [plan, state]
        g, h = levels.Gate(t, LOUDEST), hold.Hold(t, t // 2, HANG, LOUDEST, RAMP_LOG2)
        check = min(plan.buses, 48)
        n_in = int(off[check])
        _native.check(L.mbx_pcm_levels(pcm16.data_ptr(), rows, lv.data_ptr(), strm), "mbx_pcm_levels")
        _native.check(L.mbx_mixdown_held(plan.handle, C.addressof(h), state.handle, 0, pcm16.data_ptr(), rows, lv.data_ptr(), out16.data_ptr(), strm), "mbx_mixdown_held")
        torch.cuda.synchronize()
        want, st = hold.step(host, off[:check + 1], row[:n_in], gain[:n_in], 0, h, hold.zero_state(n_in))
        assert out16[:check * 160].cpu().numpy().tobytes() == want.tobytes() and state.get(strm)[:n_in].tobytes() == st.tobytes(), name

        def gated(plan=plan, g=g):
            return L.mbx_mixdown_gated(plan.handle, C.addressof(g), 0, pcm16.data_ptr(), rows, lv.data_ptr(), out16.data_ptr(), strm)

        def held(plan=plan, h=h, state=state, x=pcm16, l=lv):
            return L.mbx_mixdown_held(plan.handle, C.addressof(h), state.handle, 0, x.data_ptr(), rows, l.data_ptr(), out16.data_ptr(), strm)

        def pair(mix, x=pcm16, l=lv):
            L.mbx_pcm_levels(x.data_ptr(), rows, l.data_ptr(), strm)
            return mix()

        turn = [0]

        def churn(held=held):
            turn[0] ^= 1
            x, l = (other, lv_other) if turn[0] else (pcm16, lv)
            L.mbx_pcm_levels(x.data_ptr(), rows, l.data_ptr(), strm)
            return held(x=x, l=l)

        base = {"rows": rows, "buses": plan.buses, "long_buses": plan.long_buses, "inputs": int(off[-1]), "open_peak": t, "loudest_n": LOUDEST}
        step[f"{name}: gated alone"], step[f"{name}: held alone"] = gated, held
        step[f"{name}: levels + gated"] = lambda gated=gated, pair=pair: pair(gated)
        step[f"{name}: levels + held"] = lambda held=held, pair=pair: pair(held)
        step[f"{name}: levels + held, churn"] = churn
        for f in ("gated alone", "held alone", "levels + gated", "levels + held", "levels + held, churn"):
            info[f"{name}: {f}"] = {**base, "launches": (plan.long_buses > 0) + (plan.long_buses < plan.buses) * (2 if "held" in f else 1) + ("levels" in f)}
    report("kernel", step, info, steps, rounds)
    for k in reversed(keep):
        k.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, decoder, framegen, hold, levels, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    plan = mixdown.Plan(*dealt(np.random.default_rng(9), S, 8))
    state = hold.GateState(plan)
    gate, h = levels.Gate(T_OPEN, LOUDEST), hold.Hold(T_OPEN, T_OPEN // 2, HANG, LOUDEST, RAMP_LOG2)
    forms = ("buses of 8 pcm16 gated {t,3}", "buses of 8 pcm16 held {t,t/2,2,3,5}")
    out = L.mbx_host_alloc(S * 320)

    def run(s, f, count):
        for _ in range(count):
            if "held" in f:
                _native.check(L.mbx_session_next_mixdown_held(s, plan.handle, 0, C.addressof(h), state.handle, out), "next_mixdown_held")
            else:
                _native.check(L.mbx_session_next_mixdown_gated(s, plan.handle, 0, C.addressof(gate), out), "next_mixdown_gated")
            _native.check(L.mbx_session_submit(s, 1, pin, None, None, None), "submit")
        _native.check(L.mbx_session_wait(s), "wait")

    def window(f, count):
        """ONE session alive at a time, made for its window: with both alive the streams of the second share hardware queues (4 by
        default) with those of the first, and its copy out no longer runs beside its next step -- 230 M frames/s where 300 M are
        measured alone, whichever form comes second"""
        s = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(s), 0, S, S, 16 | 32), "create")
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
                          "bytes_out_per_submit": plan.buses * 320, "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2),
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
    a = ap.parse_args()
    if a.kernel or not a.sessions:
        kernel(a.rows, a.steps, a.rounds)
    if a.sessions:
        sessions(a.rows, a.submits, a.rounds)
