#!/usr/bin/env python3
"""keystream_bench.py [--streams S] [--steps K] [--rounds R] -- what a keyed step (include/mbx_keystream.h) costs next to the unkeyed
step of the same shape, and what mbx_apply_keystream costs alone.

Three workloads on resident state: S x 1 IMBE 7200x4400, S x 1 AMBE+2 3600x2450 and S x 16 IMBE 7200x4400 (default S = 65,536).
Per workload the windows alternate in one process:

  keyed    mbx_process_batch_keyed on ENCRYPTED frames encode(b ^ k) with the keystream k
  unkeyed  the same call without a keystream on the CLEAR frames encode(b): the same decoded content, so the stream stage does the
           same work in both (the outputs of the two are compared byte for byte first)
  apply    mbx_apply_keystream alone on S * T records

A keyed T = 1 step takes the staged launches; the unkeyed T = 1 step takes a one-launch form unless MBX_FUSE_ONE=0, and the switch
is read once per process.  So the program runs itself twice as a child process: once under MBX_FUSE_ONE=0, where `unkeyed` is the
same launches as `keyed` but for the front kernel, and once with the switch unset, where `unkeyed` is the default step.  Each child
interleaves its own windows; the two children run one after the other.

HIP-event time per call, `steps` calls a window, `rounds` rounds: per line the best, the median and the spread (worst - best) over
the rounds.  Needs a GPU; prints one JSON line per measurement.  Development aid."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

WORKLOADS = (("imbe7200x4400", 0, 1), ("ambe3600x2450", 1, 1), ("imbe7200x4400", 0, 16))


def timed(step, steps):
    import torch

    for _ in range(2):
        step()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(steps):
        step()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / steps


def child(S, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, framegen, keystream as K

    L = _native.lib()
    fuse = os.environ.get("MBX_FUSE_ONE", "unset")
    strm = torch.cuda.current_stream().cuda_stream
    for name, codec, T in WORKLOADS:
        rng = framegen.rng_for(0x4B610000 + 16 * T + codec)
        b = framegen.imbe_voiced_param_bits(S, rng) if codec == 0 else framegen.ambe_voice_param_bits(S, rng)
        k = rng.integers(0, 2, size=b.shape, dtype=np.uint8)
        enc = framegen.encode_imbe7200x4400 if codec == 0 else framegen.encode_ambe3600x2450
        # (one frame per stream, repeated over the T ticks of a launch: S distinct frames)
        clear, encrypted, rows = (np.ascontiguousarray(np.repeat(a, T, axis=0)) for a in (enc(b), enc(b ^ k), K.rows_from_bits(k)))
        decs = [decoder.BatchDecoder(codec, S, resident=True) for _ in range(2)]
        outs = [d.make_outputs(T, want_pcm16=True, want_results=False) for d in decs]
        d_clear, d_enc, d_key = (torch.from_numpy(a.reshape(-1)).cuda() for a in (clear, encrypted, rows))

        def call(i, frames, key):
            d, o = decs[i], outs[i]
            _native.check(L.mbx_process_batch_keyed(codec, S, T, None, frames.data_ptr(), None, key.data_ptr() if key is not None else None,
                                                    d.state.data_ptr(), d.resident.data_ptr(), d.rng.data_ptr(), o["pcm16"].data_ptr(), None, None,
                                                    o["records"].data_ptr(), strm), "mbx_process_batch_keyed")
            return (L.mbx_last_kernel_name(strm) or b"").decode()

        kernels = {"keyed": call(0, d_enc, d_key), "unkeyed": call(1, d_clear, None)}
        torch.cuda.synchronize()
        assert torch.equal(outs[0]["pcm16"], outs[1]["pcm16"]) and torch.equal(outs[0]["records"], outs[1]["records"]), "keyed and unkeyed differ"
        assert torch.equal(decs[0].state, decs[1].state) and torch.equal(decs[0].rng, decs[1].rng)
        spare = outs[0]["records"].clone()
        runs = {"keyed": lambda: call(0, d_enc, d_key), "unkeyed": lambda: call(1, d_clear, None),
                "apply": lambda: _native.check(L.mbx_apply_keystream(codec, spare.data_ptr(), S * T, d_key.data_ptr(), strm), "mbx_apply_keystream")}
        times = {w: [] for w in runs}
        for _ in range(rounds):
            for w, fn in runs.items():
                times[w].append(timed(fn, steps))
        for w in runs:
            t = sorted(times[w])
            print(json.dumps({"workload": f"{S} x {T} {name}", "what": w, "MBX_FUSE_ONE": fuse, "kernel": kernels.get(w, "keystream_apply_kernel"),
                              "best_us": round(1e3 * t[0], 2), "median_us": round(1e3 * t[len(t) // 2], 2), "spread_us": round(1e3 * (t[-1] - t[0]), 2),
                              "rounds": rounds, "calls_per_round": steps}), flush=True)
        del decs, outs, d_clear, d_enc, d_key, spare
        torch.cuda.empty_cache()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--streams", type=int, default=65536)
    ap.add_argument("--steps", type=int, default=400)   # (windows of 20 calls, 3 ms at T = 1, spread by 30 us: too short to tell 2 us)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--child", action="store_true", help="measure in this process, under the environment it was started in")
    a = ap.parse_args()
    if a.child:
        child(a.streams, a.steps, a.rounds)
    else:
        for fuse in ("0", None):
            env = {k: v for k, v in os.environ.items() if k != "MBX_FUSE_ONE"}
            if fuse is not None:
                env["MBX_FUSE_ONE"] = fuse
            rc = subprocess.call([sys.executable, os.path.abspath(__file__), "--child", "--streams", str(a.streams), "--steps", str(a.steps),
                                  "--rounds", str(a.rounds)], env=env)
            if rc != 0:
                sys.exit(rc)
