#!/usr/bin/env python3
"""pcm8_bench.py [--kernel | --share | --sessions | --ab NAME] [--streams S] [--steps N] [--rounds R] -- what companded PCM out
(include/mbx_pcm8.h) costs and what it saves.

--kernel    HIP-event time of mbx_pcm_compand alone, both laws, next to mbx_floattoshort on the same rows (float in, int16 out: twice
            the bytes) at 65,536 and 1,048,576 rows; `steps` launches a window, the forms' windows alternating, `rounds` rounds: per
            form the best, the median and the spread (worst - best) over the rounds, and the bytes a launch moves.
--share     the compand launch as a share of the resident IMBE x 1 step (BatchDecoder(resident=True).decode, T = 1) at S streams,
            windows alternating as above.
--sessions  frames/s of one session, one host thread: IMBE, S streams x T = 1 per submit, `submits` submits a window (40, as
            tools/src/host_bench.c), pinned buffers in and out; three forms -- int16 PCM out only (a session made without
            MBX_SESSION_PCM8: the path of a library without the feature), bytes out only, both --, windows alternating, `rounds`
            rounds: median, best and spread of each form's windows.  --forms pcm16: that form alone (a library of an earlier commit);
            --forms pcm16,pcm8,both,none adds submits that bring nothing back: the rate the input side and the step allow.
--ab NAME   the pcm16 form of --sessions in child processes that alternate between the library in the tree and
            mbelib-neo_amd/variants/libmbx_hip_NAME.so (as tools/abx.sh does for bench.py), `rounds` alternations: the median of the
            children's medians and their spread, per library.
Needs a GPU; prints one JSON line per measurement.  Development aid."""
import argparse
import ctypes as C
import json
import os
import statistics
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


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


def kernel(steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, pcm8

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    for rows in (65536, 1048576):
        n = rows * 160
        pcmf = (torch.rand(n, device="cuda") - 0.5) * 9000.0   # (mbe_floattoshort scales by 7: the whole int16 range, clipping included)
        pcm16 = torch.empty(n, dtype=torch.int16, device="cuda")
        out8 = torch.empty(n, dtype=torch.uint8, device="cuda")
        _native.check(L.mbx_floattoshort(pcmf.data_ptr(), pcm16.data_ptr(), rows, strm), "mbx_floattoshort")
        host = pcm16[:160 * 4096].cpu().numpy()
        for law in (pcm8.LAW_ULAW, pcm8.LAW_ALAW):
            _native.check(L.mbx_pcm_compand(law, pcm16.data_ptr(), rows, out8.data_ptr(), strm), "mbx_pcm_compand")
            assert out8[:160 * 4096].cpu().numpy().tobytes() == pcm8.compand(host, law).tobytes()
        step = {"floattoshort": lambda: L.mbx_floattoshort(pcmf.data_ptr(), pcm16.data_ptr(), rows, strm),
                "ulaw": lambda: L.mbx_pcm_compand(pcm8.LAW_ULAW, pcm16.data_ptr(), rows, out8.data_ptr(), strm),
                "alaw": lambda: L.mbx_pcm_compand(pcm8.LAW_ALAW, pcm16.data_ptr(), rows, out8.data_ptr(), strm)}
        moved = {"floattoshort": 6 * n, "ulaw": 3 * n, "alaw": 3 * n}
        times = {f: [] for f in step}
        per = max(20, steps // (rows // 65536))
        for _ in range(rounds):
            for f in step:
                times[f].append(timed(step[f], per))
        for f in step:
            s = summary(times[f])
            print(json.dumps({"mode": "kernel", "form": f, "rows": rows, "bytes_moved_per_launch": moved[f], **s,
                              "GB_per_s_at_median": round(moved[f] / (s["median_us"] * 1e3), 1), "rounds": rounds, "launches_per_round": per}), flush=True)
        del pcmf, pcm16, out8
        torch.cuda.empty_cache()


def share(S, steps, rounds):
    import torch
    from mbelib_neo_amd import decoder, framegen, pcm8

    dec = decoder.BatchDecoder(0, S, resident=True)
    frames = dec.to_device(framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)))
    out = dec.make_outputs(1, want_results=False)
    out8 = torch.empty((S, 160), dtype=torch.uint8, device="cuda")
    step = {"step": lambda: dec.decode(frames, 1, out=out), "compand": lambda: dec.compand(out["pcm16"], pcm8.LAW_ULAW, out=out8),
            "step+compand": lambda: (dec.decode(frames, 1, out=out), dec.compand(out["pcm16"], pcm8.LAW_ULAW, out=out8))}
    times = {f: [] for f in step}
    for _ in range(rounds):
        for f in step:
            times[f].append(timed(step[f], steps))
    s = {f: summary(times[f]) for f in step}
    print(json.dumps({"mode": "share", "streams": S, **{f: s[f] for f in step},
                      "compand_share_of_step": round(s["compand"]["median_us"] / s["step"]["median_us"], 4), "rounds": rounds, "launches_per_round": steps}), flush=True)


# session outputs, int16 asked for, bytes asked for ("none": a submit that brings nothing back -- what the input side and the step alone allow)
FORMS = {"pcm16": (1, True, False), "pcm8": (8, False, True), "both": (1 | 8, True, True), "none": (1, False, False)}


def sessions(S, submits, rounds, forms):
    from mbelib_neo_amd import _native, decoder, framegen

    decoder.ensure_init(0)
    L = _native.lib()
    frames = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(7)).reshape(-1)
    pin = L.mbx_host_alloc(frames.size)
    np.ctypeslib.as_array((C.c_uint8 * frames.size).from_address(pin))[:] = frames
    work = {}
    for f in forms:
        outputs, want16, want8 = FORMS[f]
        h = C.c_void_p()
        _native.check(L.mbx_session_create(C.byref(h), 0, S, S, outputs), "create")
        work[f] = (h, L.mbx_host_alloc(S * 320) if want16 else None, L.mbx_host_alloc(S * 160) if want8 else None)

    def window(f, count):
        h, p16, p8 = work[f]
        t0 = time.perf_counter()
        for k in range(count):
            if p8:
                _native.check(L.mbx_session_next_pcm8(h, k & 1, p8), "next_pcm8")
            _native.check(L.mbx_session_submit(h, 1, pin, p16, None, None), "submit")
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
                          "bytes_out_per_frame": 320 * FORMS[f][1] + 160 * FORMS[f][2], "median_Mframes_per_s": round(statistics.median(r) / 1e6, 2),
                          "best_Mframes_per_s": round(r[-1] / 1e6, 2), "spread_Mframes_per_s": round((r[-1] - r[0]) / 1e6, 2), "rounds": rounds,
                          "library": os.path.basename(_native.library_path())}), flush=True)
    for h, p16, p8 in work.values():
        L.mbx_session_destroy(h)
        L.mbx_host_free(p16)
        L.mbx_host_free(p8)
    L.mbx_host_free(pin)


def ab(name, S, submits, rounds):
    libs = {"product": None, name: os.path.join(ROOT, "mbelib-neo_amd", "variants", f"libmbx_hip_{name}.so")}
    medians = {k: [] for k in libs}
    for _ in range(rounds):
        for k, path in libs.items():
            env = dict(os.environ)
            if path:
                env["MBX_HIP_LIBRARY"], env["MBX_HIP_LIBRARY_ALLOW_OLDER"] = path, "1"
            run = subprocess.run([sys.executable, os.path.abspath(__file__), "--sessions", "--forms", "pcm16", "--streams", str(S), "--submits", str(submits),
                                  "--rounds", "9"], env=env, capture_output=True, text=True, timeout=300)
            if run.returncode != 0:
                print(k, "FAILED", run.stderr[-600:])
                sys.exit(1)
            medians[k].append(json.loads(run.stdout.strip().splitlines()[-1])["median_Mframes_per_s"])
    for k, v in medians.items():
        print(json.dumps({"mode": "ab", "library": k, "form": "pcm16", "streams": S, "median_of_medians_Mframes_per_s": round(statistics.median(v), 2),
                          "spread_Mframes_per_s": round(max(v) - min(v), 2), "children": v}), flush=True)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--share", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--ab", default=None, metavar="NAME")
    ap.add_argument("--forms", default="pcm16,pcm8,both")
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=200)
    ap.add_argument("--submits", type=int, default=40)
    ap.add_argument("--rounds", type=int, default=9)
    a = ap.parse_args()
    if a.kernel or not (a.share or a.sessions or a.ab):
        kernel(a.steps, a.rounds)
    if a.share:
        share(a.streams, a.steps, a.rounds)
    if a.sessions:
        sessions(a.streams, a.submits, a.rounds, a.forms.split(","))
    if a.ab:
        ab(a.ab, a.streams, a.submits, a.rounds)
