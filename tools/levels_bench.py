#!/usr/bin/env python3
"""levels_bench.py [--kernel | --plain | --sessions] [--rows N] [--steps N] [--submits N] [--rounds R] -- what levels out and the gated
mix-down (include/mbx_levels.h) cost and what they save.  Built like mixdown_bench.py, whose helpers it uses.

The rows: three channels in four idle (comfort noise, peaks of a few tens), one in four talking (peaks of thousands); the peak gate
of the gated cases, `t` = 1000, lies between the two.

--kernel    HIP-event times, `steps` launches a window, the windows alternating in one process, `rounds` rounds: per form the best, the
            median and the spread (worst - best).
              mbx_pcm_levels against mbx_pcm_compand on `rows` rows (65,536) and on 16 x as many;
              `rows` rows dealt into buses of 8 and of 32 (the default split: short and long kernel form): mbx_mixdown against
              mbx_pcm_levels + mbx_mixdown_gated under {0,0}, {t,0} and {t,3}, and the gated launch alone;
              one 4,096-input bus beside buses of 8 ("allcall"): mbx_mixdown against mbx_pcm_levels + mbx_mixdown_gated under {0,3}.
            The first buses of every case are compared with levels.mix_gated first.
--plain     mbx_mixdown alone on the same cases: what a library of the parent commit can run as well (MBX_HIP_LIBRARY=... with
            MBX_HIP_LIBRARY_ALLOW_OLDER=1), to hold the old path of this build against it.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, pinned buffers in and out; level
            records out only against int16 rows out only against buses of 8 out only (ungated, and {t,3} with its levels launch).
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

from mixdown_bench import FORM_NAMES, allcall, dealt, summary, timed  # noqa: E402

T_OPEN = 1000


def device_rows(rows):
    """int16 [rows, 160] on the device: one row in four a talker, the others idle"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(11)
    talk = torch.rand(rows, 1, device="cuda", generator=g) < 0.25
    amp = torch.where(talk, torch.tensor(9000.0, device="cuda"), torch.tensor(30.0, device="cuda"))
    return ((torch.rand(rows, 160, device="cuda", generator=g) - 0.5) * 2.0 * amp).to(torch.int16).contiguous()


def cases(rng, rows):
    return {"buses of 8": (dealt(rng, rows, 8), ((0, 0), (T_OPEN, 0), (T_OPEN, 3))), "buses of 32": (dealt(rng, rows, 32), ((0, 0), (T_OPEN, 0), (T_OPEN, 3))),
            "allcall": (allcall(rng, rows), ((0, 3),))}


def report(mode, step, info, steps, rounds):
    times = {f: [] for f in step}
    for _ in range(rounds):
        for f in step:
            times[f].append(timed(step[f], steps))
    for f in step:
        print(json.dumps({"mode": mode, "form": f, **info.get(f, {}), **summary(times[f]), "rounds": rounds, "launches_per_round": steps}), flush=True)


def kernel(rows, steps, rounds, plain):
    import torch
    from mbelib_neo_amd import _native, decoder, mixdown, pcm8

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    pcm16 = device_rows(rows)
    out16 = torch.empty(rows * 160, dtype=torch.int16, device="cuda")
    host = pcm16.cpu().numpy()
    rng = np.random.default_rng(7)
    step, info, plans = {}, {}, []
    if not plain:
        from mbelib_neo_amd import levels

        lv = torch.empty((rows, 16), dtype=torch.uint8, device="cuda")
        for scale in (1, 16):
            big = pcm16 if scale == 1 else device_rows(rows * scale)
            n = rows * scale
            big_lv, big8 = torch.empty((n, 16), dtype=torch.uint8, device="cuda"), torch.empty(n * 160, dtype=torch.uint8, device="cuda")
            step[f"levels {n} rows"] = lambda big=big, n=n, o=big_lv: L.mbx_pcm_levels(big.data_ptr(), n, o.data_ptr(), strm)
            step[f"compand ulaw {n} rows"] = lambda big=big, n=n, o=big8: L.mbx_pcm_compand(pcm8.LAW_ULAW, big.data_ptr(), n, o.data_ptr(), strm)
            info[f"levels {n} rows"], info[f"compand ulaw {n} rows"] = {"bytes_moved_per_launch": 336 * n}, {"bytes_moved_per_launch": 480 * n}
        _native.check(L.mbx_pcm_levels(pcm16.data_ptr(), rows, lv.data_ptr(), strm), "mbx_pcm_levels")
        torch.cuda.synchronize()
        host_lv = levels.measure(host)
        assert lv.cpu().numpy().tobytes() == host_lv.tobytes()
    for name, ((off, row, gain), gates) in cases(rng, rows).items():
        plan = mixdown.Plan(off, row, gain)
        plans.append(plan)
        check = min(plan.buses, 48)
        base = {"rows": rows, "buses": plan.buses, "long_buses": plan.long_buses, "inputs": int(off[-1])}
        step[f"{name}: mixdown"] = lambda plan=plan: L.mbx_mixdown(plan.handle, 0, pcm16.data_ptr(), rows, out16.data_ptr(), strm)
        info[f"{name}: mixdown"] = base
        if plain:
            continue
        for gate in gates:
            g = levels.Gate(*gate)
            _native.check(L.mbx_mixdown_gated(plan.handle, C.addressof(g), 0, pcm16.data_ptr(), rows, lv.data_ptr(), out16.data_ptr(), strm), "mbx_mixdown_gated")
            torch.cuda.synchronize()
            got = out16[:check * 160].cpu().numpy().reshape(check, 160)
            assert got.tobytes() == levels.mix_gated(host, off[:check + 1], row, gain, 0, *gate).tobytes(), (name, gate)
            taken = levels.chosen(host_lv, off, row, *gate)

            def gated(plan=plan, g=g):
                return L.mbx_mixdown_gated(plan.handle, C.addressof(g), 0, pcm16.data_ptr(), rows, lv.data_ptr(), out16.data_ptr(), strm)

            def both(gated=gated):
                L.mbx_pcm_levels(pcm16.data_ptr(), rows, lv.data_ptr(), strm)
                return gated()

            key = "{%s,%d}" % ("t" if gate[0] else "0", gate[1])
            step[f"{name}: gated {key} alone"], step[f"{name}: levels + gated {key}"] = gated, both
            info[f"{name}: gated {key} alone"] = info[f"{name}: levels + gated {key}"] = {**base, "inputs_chosen": int(taken.sum())}
    report("plain" if plain else "kernel", step, info, steps, rounds)
    for p in plans:
        p.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, decoder, framegen, levels, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    rng = np.random.default_rng(9)
    plan = mixdown.Plan(*dealt(rng, S, 8))
    gate = levels.Gate(T_OPEN, 3)
    # name: (outputs, what is attached, bytes out)
    forms = {"pcm16 rows": (1, None, S * 320), "level records": (32, "levels", S * 16), "buses of 8 pcm16": (16, "buses", plan.buses * 320),
             "buses of 8 pcm16 gated {t,3}": (16 | 32, "gated", plan.buses * 320), "gated {t,3} + level records": (16 | 32, "both", plan.buses * 320 + S * 16)}
    work = {}
    for f, (outputs, what, out_bytes) in forms.items():
        h = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(h), 0, S, S, outputs), "create")
        work[f] = (h, what, L.mbx_host_alloc(S * 320), L.mbx_host_alloc(S * 16), out_bytes)

    def window(f, count):
        h, what, out, rec, _ = work[f]
        t0 = time.perf_counter()
        for _ in range(count):
            if what in ("levels", "both"):
                _native.check(L.mbx_session_next_levels(h, rec), "next_levels")
            if what == "buses":
                _native.check(L.mbx_session_next_mixdown(h, plan.handle, 0, out), "next_mixdown")
            if what in ("gated", "both"):
                _native.check(L.mbx_session_next_mixdown_gated(h, plan.handle, 0, C.addressof(gate), out), "next_mixdown_gated")
            _native.check(L.mbx_session_submit(h, 1, pin, None if what else out, None, None), "submit")
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
    for h, _, out, rec, _ in work.values():
        L.mbx_session_destroy(h)
        L.mbx_host_free(out)
        L.mbx_host_free(rec)
    plan.close()
    L.mbx_host_free(pin)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--plain", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--submits", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    if a.kernel or a.plain or not a.sessions:
        kernel(a.rows, a.steps, a.rounds, a.plain)
    if a.sessions:
        sessions(a.rows, a.submits, a.rounds)
