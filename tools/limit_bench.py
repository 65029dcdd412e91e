#!/usr/bin/env python3
"""limit_bench.py [--kernel | --sums | --sessions] [--parents-only] [--rows N] [--steps N] [--submits N] [--rounds R] -- what limited
buses (include/mbx_limit.h) cost beside the launches they sit next to.  Built like agc_bench.py, whose helpers it uses.

Every reference is measured in the same process on the same rows: windows alternate, `rounds` rounds, per form the best, the median
and the spread (worst - best).

--kernel    HIP-event times, `steps` launches a window: mbx_bus_limit (T = 1, all three forms) at rows / 8 (8,192) and rows (65,536) bus
            rows beside mbx_pcm_compand on as many int16 rows.  The launch moves 960 B a row (640 in, 320 out as int16) where compand
            moves 480: the yardstick is 2 x compand's median plus the spread of compand's own windows.  The first rows of every shape
            are compared with limit.step first.
--sums      the three sums launches beside their PCM16 parents, `rows` rows dealt into buses of 8 and of 32, in one process.
            --parents-only measures the parents alone: run it once on this library and once with MBX_HIP_LIBRARY naming the library of
            the parent commit (MBX_HIP_LIBRARY_ALLOW_OLDER=1) to hold the 18 old bus-kernel instances to their old times.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, pinned buffers in and out; limited
            gated buses of 8 out only against unlimited ones.
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


def _limit():
    from mbelib_neo_amd import limit

    return limit.Limit(24000, 64, 2, 5)


def device_sums(rows):
    """int32 [rows, 160] on the device: one bus in four beyond the ceiling, the others inside it"""
    import torch

    g = torch.Generator(device="cuda").manual_seed(13)
    hot = torch.rand(rows, 1, device="cuda", generator=g) < 0.25
    amp = torch.where(hot, torch.tensor(60000.0, device="cuda"), torch.tensor(9000.0, device="cuda"))
    return ((torch.rand(rows, 160, device="cuda", generator=g) - 0.5) * 2.0 * amp).to(torch.int32).contiguous()


def kernel(rows, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, limit, pcm8

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    p = _limit()
    step, info, keep = {}, {}, []
    for n in (max(rows // 8, 1), rows):
        s = device_sums(n)
        x = device_rows(n)
        out16 = torch.empty((n, 160), dtype=torch.int16, device="cuda")
        out8 = torch.empty((n, 160), dtype=torch.uint8, device="cuda")
        state = limit.LimitState(n)
        keep.append(state)
        check = min(n, 64)
        for form, out in ((0, out16), (1, out8), (2, out8)):
            state.reset(stream=strm)
            _native.check(L.mbx_bus_limit(C.addressof(p), state.handle, n, 1, s.data_ptr(), form, out.data_ptr(), strm), "mbx_bus_limit")
            torch.cuda.synchronize()
            want, st, _ = limit.step(s[:check].cpu().numpy(), 1, p, limit.fresh_state(check), form)
            assert out[:check].cpu().numpy().tobytes() == want.tobytes() and state.get(0, check, strm).tobytes() == st.tobytes(), (n, form)
        for form, name, out in ((0, "pcm16", out16), (1, "ulaw", out8), (2, "alaw", out8)):
            step[f"limit {name} {n} rows"] = lambda n=n, s=s, o=out, st=state, form=form: L.mbx_bus_limit(C.addressof(p), st.handle, n, 1, s.data_ptr(), form,
                                                                                                            o.data_ptr(), strm)
            info[f"limit {name} {n} rows"] = {"rows": n, "bytes_moved_per_launch": (640 + (320 if form == 0 else 160) + 8) * n}
        step[f"compand ulaw {n} rows"] = lambda n=n, x=x, o=out8: L.mbx_pcm_compand(pcm8.LAW_ULAW, x.data_ptr(), n, o.data_ptr(), strm)
        info[f"compand ulaw {n} rows"] = {"rows": n, "bytes_moved_per_launch": 480 * n}
    report("kernel", step, info, steps, rounds)
    for k in reversed(keep):
        k.close()


def sums(rows, steps, rounds, parents_only):
    import torch
    from mbelib_neo_amd import _native, decoder, hold, levels, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    pcm16 = device_rows(rows)
    lv = torch.empty((rows, 16), dtype=torch.uint8, device="cuda")
    _native.check(L.mbx_pcm_levels(pcm16.data_ptr(), rows, lv.data_ptr(), strm), "mbx_pcm_levels")
    gate, h = levels.Gate(T_OPEN, LOUDEST), hold.Hold(T_OPEN, T_OPEN // 2, 2, LOUDEST, 5)
    rng = np.random.default_rng(7)
    step, info, keep = {}, {}, []
    for size in (8, 32):
        plan = mixdown.Plan(*dealt(rng, rows, size))
        gs = hold.GateState(plan)
        keep += [gs, plan]
        out16 = torch.empty((plan.buses, 160), dtype=torch.int16, device="cuda")
        out32 = torch.empty((plan.buses, 160), dtype=torch.int32, device="cuda")
        tag = f"buses of {size}"
        a = (pcm16.data_ptr(), rows)
        step[f"mixdown pcm16 {tag}"] = lambda pl=plan, o=out16: L.mbx_mixdown(pl.handle, 0, *a, o.data_ptr(), strm)
        step[f"gated pcm16 {tag}"] = lambda pl=plan, o=out16: L.mbx_mixdown_gated(pl.handle, C.addressof(gate), 0, *a, lv.data_ptr(), o.data_ptr(), strm)
        step[f"held pcm16 {tag}"] = lambda pl=plan, o=out16, g=gs: L.mbx_mixdown_held(pl.handle, C.addressof(h), g.handle, 0, *a, lv.data_ptr(), o.data_ptr(), strm)
        if not parents_only:
            step[f"mixdown sums {tag}"] = lambda pl=plan, o=out32: L.mbx_mixdown_sums(pl.handle, *a, o.data_ptr(), strm)
            step[f"gated sums {tag}"] = lambda pl=plan, o=out32: L.mbx_mixdown_gated_sums(pl.handle, C.addressof(gate), *a, lv.data_ptr(), o.data_ptr(), strm)
            step[f"held sums {tag}"] = lambda pl=plan, o=out32, g=gs: L.mbx_mixdown_held_sums(pl.handle, C.addressof(h), g.handle, *a, lv.data_ptr(), o.data_ptr(), strm)
        for f in list(step):
            if f.endswith(tag):
                info[f] = {"rows": rows, "buses": plan.buses}
    for f in step:
        _native.check(step[f](), f)
    torch.cuda.synchronize()
    report("sums", step, info, steps, rounds)
    for k in keep:
        k.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, decoder, framegen, levels, limit, mixdown

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    plan = mixdown.Plan(*dealt(np.random.default_rng(9), S, 8))
    state = limit.LimitState(plan.buses)
    p, gate = _limit(), levels.Gate(T_OPEN, LOUDEST)
    forms = ("buses of 8 pcm16 gated {t,3}", "buses of 8 pcm16 gated {t,3} limited")
    out = L.mbx_host_alloc(S * 320)

    def run(s, f, count):
        for _ in range(count):
            _native.check(L.mbx_session_next_mixdown_gated(s, plan.handle, 0, C.addressof(gate), out), "next_mixdown_gated")
            if "limited" in f:
                _native.check(L.mbx_session_next_limit(s, C.addressof(p), state.handle), "next_limit")
            _native.check(L.mbx_session_submit(s, 1, pin, None, None, None), "submit")
        _native.check(L.mbx_session_wait(s), "wait")

    def window(f, count):
        """ONE session alive at a time, made for its window (hold_bench.py says why)"""
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
        print(json.dumps({"mode": "sessions", "form": f, "streams": S, "submits_per_window": submits, "host_threads": 1, "bytes_out_per_submit": plan.buses * 320,
                          "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2), "best_Mframes_per_s": round(r[-1] / 1e6, 2),
                          "spread_Mframes_per_s": round((r[-1] - r[0]) / 1e6, 2), "rounds": rounds}), flush=True)
    L.mbx_host_free(out)
    state.close()
    plan.close()
    L.mbx_host_free(pin)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--sums", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--parents-only", action="store_true")
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--submits", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=7)
    a_ = ap.parse_args()
    if a_.kernel or not (a_.sums or a_.sessions):
        kernel(a_.rows, a_.steps, a_.rounds)
    if a_.sums:
        sums(a_.rows, a_.steps, a_.rounds, a_.parents_only)
    if a_.sessions:
        sessions(a_.rows, a_.submits, a_.rounds)
