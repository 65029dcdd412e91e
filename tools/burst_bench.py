#!/usr/bin/env python3
"""burst_bench.py [--kernels | --sessions] [--form FORM] [--streams S] [--steps N] -- what burst input (include/mbx_burst.h) costs and saves.

Two SHAPES, random bijections with the right frame count and burst length (no air-interface table is written down anywhere):
"dmr" = AMBE+2, 3 frames in 264 bits; "ldu" = IMBE, 9 frames in 1,728 bits.  Hard and soft, S streams (default 65,536), resident state.

--kernels   per shape: HIP-event time of one mbx_process_bursts[_soft] step against the mbx_process_batch[_soft]_resident step on
            frames that are already there.  Run it under `rocprofv3 --kernel-trace --stats -- python tools/burst_bench.py --kernels`
            for the gather kernels' own times next to their step's kernels (instances of burst_gather_kernel<form, invert> and
            burst_gather_soft_kernel<cell, flip>).  Soft bursts as LLRs: tools/llr_gather_bench.py.
--sessions  frames/s of sessions fed with bursts (mbx_session_submit_bursts[_soft]) against the same sessions fed with frames the
            host scatters first (numpy apply_schedule, vectorised over the batch -- kinder to the host than the per-bit C loop of
            INTEGRATION.md), 1 and 8 host threads, each thread with its own session of S / threads streams; pinned input, int16 PCM out.
--form      packed (default) | bits | dibits: the form of the bursts (mbx_burst_schedule_create_form).  With another form than packed
            every measurement is made for the packed form AND for that form in the same process, their windows alternating:
            --kernels adds the form's step and both gathers alone, --sessions replaces the scatter route by the packed bursts.
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
FORMS = {"packed": 0, "bits": 1, "dibits": 2}


def make(shape, n, soft, seed=1, form="packed"):
    """(schedule, bursts): the same random schedule and the same received bits for every form"""
    from mbelib_neo_amd import bursts as B

    codec, F, bits = SHAPES[shape]
    rng = np.random.default_rng(seed)
    s = B.random_schedule(codec, F, bits, rng, device=True, form=FORMS[form])
    if soft:
        bursts = rng.integers(0, 256, size=(n, bits, 2), dtype=np.uint8)
        bursts[:, :, 0] &= 1
        bursts[:, 1::2, 1] = bursts[:, 0::2, 1]   # one reliability per symbol
    else:
        bursts = rng.integers(0, 256, size=(n, (bits + 7) // 8), dtype=np.uint8)
    return s, B.to_form(s, bursts, soft=soft)


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


def kernels(S, steps, form="packed"):
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder

    decoder.ensure_init(0)
    L = _native.lib()
    forms = ["packed"] + ([form] if form != "packed" else [])
    for shape in SHAPES:
        for soft in (False, True):
            codec, F, _ = SHAPES[shape]
            dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) + 1, resident=True)
            out = dec.make_outputs(F)
            made = {f: make(shape, S, soft, form=f) for f in forms}
            d_bursts = {f: dec.to_device(made[f][1]) for f in forms}
            d_frames = B.deinterleave(made["packed"][0], d_bursts["packed"], soft=soft).reshape(-1)
            for f in forms:
                assert torch.equal(B.deinterleave(made[f][0], d_bursts[f], soft=soft).reshape(-1), d_frames), f
                _native.check(L.mbx_reserve_stream(torch.cuda.current_stream().cuda_stream, L.mbx_burst_workspace_frames(made[f][0].handle, S, int(soft))), "reserve")
            from_bursts = {f: (lambda f=f: dec.decode_bursts(made[f][0], d_bursts[f], soft=soft, out=out)) for f in forms}
            gather = {f: (lambda f=f: B.deinterleave(made[f][0], d_bursts[f], soft=soft, out=d_frames)) for f in forms}
            from_frames = (lambda: dec.decode_soft(d_frames, F, out=out)) if soft else (lambda: dec.decode(d_frames, F, out=out))
            t_frames, t_bursts, t_gather = 1e9, dict.fromkeys(forms, 1e9), dict.fromkeys(forms, 1e9)
            for _ in range(3):   # interleaved, the better of three each: the first measurement of a process runs on a cold clock
                t_frames = min(t_frames, timed(from_frames, steps))
                for f in forms:
                    t_bursts[f] = min(t_bursts[f], timed(from_bursts[f], steps))
            for _ in range(3):
                for f in forms:
                    t_gather[f] = min(t_gather[f], timed(gather[f], steps))
            for f in forms:
                print(json.dumps({"mode": "kernels", "shape": shape, "soft": soft, "form": f, "streams": S, "frames_per_burst": F,
                                  "input_bytes_per_burst": int(made[f][1].size // S), "step_from_bursts_ms": round(t_bursts[f], 4),
                                  "step_from_frames_ms": round(t_frames, 4), "gather_alone_ms": round(t_gather[f], 4),
                                  "gather_share_of_step": round((t_bursts[f] - t_frames) / t_frames, 4)}), flush=True)
                made[f][0].close()


def sessions(S, steps, form="packed"):
    from mbelib_neo_amd import _native, bursts as B, decoder

    decoder.ensure_init(0)
    L = _native.lib()
    for shape in SHAPES:
        codec, F, _ = SHAPES[shape]
        for soft in (False, True):
            for threads in (1, 8):
                per = S // threads
                s, bursts = make(shape, per, soft)
                formed = make(shape, per, soft, form=form) if form != "packed" else None
                rates = {}
                for route in ("bursts", "scatter") if formed is None else ("bursts", "form", "bursts", "form"):   # (twice: the better of two windows)
                    sched, data = (s, bursts) if route != "form" else formed
                    work = []
                    for _ in range(threads):
                        h = C.c_void_p()
                        _native.check(L.mbx_session_create(C.byref(h), codec, per, per * F, 1), "create")
                        pin = L.mbx_host_alloc(data.size)
                        np.ctypeslib.as_array((C.c_uint8 * data.size).from_address(pin))[:] = data.reshape(-1)
                        pcm = L.mbx_host_alloc(per * F * 320)
                        work.append((h, pin, pcm))

                    def run(h, pin, pcm, count):
                        import torch

                        torch.cuda.set_device(0)
                        src = np.ctypeslib.as_array((C.c_uint8 * data.size).from_address(pin)).reshape(data.shape)
                        for _ in range(count):
                            if route != "scatter":
                                rc = (L.mbx_session_submit_bursts_soft(h, sched.handle, per, None, pin, pcm, None, None) if soft else
                                      L.mbx_session_submit_bursts(h, sched.handle, per, None, pin, sched.burst_bytes, pcm, None, None))
                            else:
                                frames = B.apply_schedule(s, src, soft=soft)
                                rc = (L.mbx_session_submit_soft if soft else L.mbx_session_submit)(h, F, frames.ctypes.data, pcm, None, None)
                            _native.check(rc, "submit")
                        _native.check(L.mbx_session_wait(h), "wait")

                    for w in work:
                        run(*w, 2)
                    ts = [threading.Thread(target=run, args=(*w, steps)) for w in work]
                    t0 = time.perf_counter()
                    for t in ts:
                        t.start()
                    for t in ts:
                        t.join()
                    rates[route] = max(rates.get(route, 0.0), threads * per * F * steps / (time.perf_counter() - t0))
                    for h, pin, pcm in work:
                        L.mbx_session_destroy(h)
                        L.mbx_host_free(pin)
                        L.mbx_host_free(pcm)
                line = {"mode": "sessions", "shape": shape, "soft": soft, "streams": per * threads, "host_threads": threads,
                        "bursts_in_Mframes_per_s": round(rates["bursts"] / 1e6, 2)}
                if formed is None:
                    line["scatter_then_frames_Mframes_per_s"] = round(rates["scatter"] / 1e6, 2)
                else:
                    line[form + "_in_Mframes_per_s"] = round(rates["form"] / 1e6, 2)
                    formed[0].close()
                print(json.dumps(line), flush=True)
                s.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernels", action="store_true")
    ap.add_argument("--sessions", action="store_true")
    ap.add_argument("--form", choices=sorted(FORMS), default="packed")
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=20)
    a = ap.parse_args()
    if a.kernels or not a.sessions:
        kernels(a.streams, a.steps, a.form)
    if a.sessions:
        sessions(a.streams, a.steps, a.form)
