#!/usr/bin/env python3
"""bands_bench.py [--kernel | --sessions] [--rows N] [--steps N] [--submits N] [--rounds R] -- what band records (include/mbx_bands.h)
cost beside the launches they are measured against.  Built like filter_bench.py, whose helpers it uses.

The references are mbx_pcm_levels and mbx_pcm_compand of the same library on the same rows, measured in the same process: windows
alternate, `rounds` rounds, per form the best, the median and the spread (worst - best).

--kernel    HIP-event times, `steps` launches a window: mbx_pcm_bands at K = 8 (bands.dtmf) and K = 32 (a coarse spectrum: 32 Hann tones), in
            both forms, over rows (65,536) and 16 * rows (1,048,576), beside mbx_pcm_levels and mbx_pcm_compand on the same rows.  The
            yardstick of the earlier stages: compand's median times the ratio of bytes moved, (320 + K * record_bytes) / 480, plus
            compand's own spread in this run; every form says whether it is inside.  The first rows of every shape are compared with
            bands.measure first.
--sessions  frames/s of one session, one host thread: IMBE, S = rows streams x T = 1 per submit, pinned buffers in and out, one session
            alive at a time: DTMF power records out only (32 B a row), level records out only (16 B), int16 rows out only (320 B).
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

PROBES = (8, 32)


def kernel(rows, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, bands, decoder, pcm8

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    probes = {8: bands.dtmf("hann"), 32: np.stack([bands.tone(200 + 110 * k, "hann") for k in range(32)])}
    banks = {K: decoder.Bank(p) for K, p in probes.items()}
    step, info = {}, {}
    for n in (rows, rows * 16):
        x = device_rows(n)
        out = torch.empty(n * 32 * 8, dtype=torch.uint8, device="cuda")
        out8 = torch.empty(n * 160, dtype=torch.uint8, device="cuda")
        lv = torch.empty((n, 16), dtype=torch.uint8, device="cuda")
        check = min(n, 300)
        for K in PROBES:
            for form in bands.FORMS:
                name = f"bands K={K} {'complex' if form == bands.COMPLEX else 'power'} {n} rows"
                _native.check(L.mbx_pcm_bands(banks[K].handle, form, x.data_ptr(), n, out.data_ptr(), strm), "mbx_pcm_bands")
                torch.cuda.synchronize()
                per = K * bands.record_bytes(form)
                assert out[:check * per].cpu().numpy().tobytes() == bands.measure(x[:check].cpu().numpy(), probes[K], form).tobytes(), name
                step[name] = lambda K=K, form=form, x=x, n=n, o=out: L.mbx_pcm_bands(banks[K].handle, form, x.data_ptr(), n, o.data_ptr(), strm)
                info[name] = {"rows": n, "probes": K, "bytes_moved_per_launch": (320 + per) * n, "against": f"compand ulaw {n} rows", "byte_ratio": (320 + per) / 480}
        step[f"levels {n} rows"] = lambda x=x, n=n, o=lv: L.mbx_pcm_levels(x.data_ptr(), n, o.data_ptr(), strm)
        step[f"compand ulaw {n} rows"] = lambda x=x, n=n, o=out8: L.mbx_pcm_compand(pcm8.LAW_ULAW, x.data_ptr(), n, o.data_ptr(), strm)
        info[f"levels {n} rows"] = {"rows": n, "bytes_moved_per_launch": 336 * n}
        info[f"compand ulaw {n} rows"] = {"rows": n, "bytes_moved_per_launch": 480 * n}
    times = {f: [] for f in step}
    for _ in range(rounds):
        for f in step:
            times[f].append(timed(step[f], steps))
    done = {f: summary(times[f]) for f in step}
    for f in step:
        line = {"mode": "kernel", "form": f, **{k: v for k, v in info[f].items() if k not in ("against", "byte_ratio")}, **done[f], "rounds": rounds,
                "launches_per_round": steps}
        if "against" in info[f]:
            ref = done[info[f]["against"]]
            us = [k for k in ref if k.startswith("median")][0]
            spread = [k for k in ref if k.startswith("spread")][0]
            line["yardstick_us"] = round(ref[us] * info[f]["byte_ratio"] + ref[spread], 2)
            line["inside_yardstick"] = bool(done[f][us] <= line["yardstick_us"])
        print(json.dumps(line), flush=True)
    for b in banks.values():
        b.close()


def sessions(S, submits, rounds):
    from mbelib_neo_amd import _native, bands, decoder, framegen

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    bank = decoder.Bank(bands.dtmf("hann"))
    forms = {"pcm16 rows": (1, 320), "level records": (32, 16), "dtmf power records": (1, 32)}   # (outputs of the session, bytes out per row)
    out = L.mbx_host_alloc(S * 320)

    def run(s, form, count):
        for _ in range(count):
            if form == "level records":
                _native.check(L.mbx_session_next_levels(s, out), "next_levels")
            if form == "dtmf power records":
                _native.check(L.mbx_session_next_bands(s, bank.handle, bands.POWER, out), "next_bands")
            _native.check(L.mbx_session_submit(s, 1, pin, out if form == "pcm16 rows" else None, None, None), "submit")
        _native.check(L.mbx_session_wait(s), "wait")

    def window(form, count):
        """ONE session alive at a time, made for its window (hold_bench.py says why)"""
        s = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(s), 0, S, S, forms[form][0]), "create")
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
                          "bytes_out_per_submit": S * forms[form][1], "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2),
                          "best_Mframes_per_s": round(r[-1] / 1e6, 2), "spread_Mframes_per_s": round((r[-1] - r[0]) / 1e6, 2), "rounds": rounds}), flush=True)
    L.mbx_host_free(out)
    bank.close()
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
