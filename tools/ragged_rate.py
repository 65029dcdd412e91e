#!/usr/bin/env python3
"""ragged_rate.py [--steps N] [--streams S] -- what one ragged launch is worth: frames/s of REAL frames for IMBE and AMBE+2, S streams
(default 8,192) with (a) counts uniform in 1..128 and (b) 95 % in 1..4, 5 % in 100..200 (fixed seed), decoded four ways on
resident state: one mbx_process_batch_ragged call (streams ordered longest first), the same with MBX_RAGGED_ORDER=0 (a fresh
child process: the switch is read once), the per-count mbx_process_batch_resident launches it replaces, and every stream padded
to the longest.  HIP events around whole steps, warm, >= 20 steps.  Needs a GPU; prints one table.  Development aid.
--mixed: streams of all four codecs instead -- (i) four equal codec groups, (ii) one large group and three of 300 streams, counts
(a) and (b) -- decoded by ONE mbx_process_batch_mixed call and by one mbx_process_batch_ragged call per codec."""
import argparse
import json
import os
import subprocess
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def counts_of(kind, S):
    rng = np.random.default_rng(0xA66ED)
    if kind == "a":
        return rng.integers(1, 129, size=S)
    c = rng.integers(1, 5, size=S)
    long = rng.choice(S, size=S // 20, replace=False)
    c[long] = rng.integers(100, 201, size=long.size)
    return c


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
    return a.elapsed_time(b) / steps   # ms per step


def measure(codec, kind, S, steps, only_ragged):
    import torch
    from mbelib_neo_amd import _native, decoder, framegen

    L = _native.lib()
    counts = counts_of(kind, S)
    total, Tmax = int(counts.sum()), int(counts.max())
    frames = framegen.random_frames(codec, total, framegen.rng_for(7 + codec))
    dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) + 1, resident=True)
    d_frames = dec.to_device(frames)
    out = dec.make_outputs(0, total=total)
    _native.check(L.mbx_reserve(S * Tmax + S), "mbx_reserve")
    res = {"real_frames": total, "padded_frames": S * Tmax}
    strm = torch.cuda.current_stream().cuda_stream
    off = np.concatenate([[0], np.cumsum(counts)])
    d_off = torch.from_numpy(off.astype(np.int32)).to(dec.device)

    def ragged():
        _native.check(L.mbx_process_batch_ragged(codec, S, d_off.data_ptr(), total, None, d_frames.data_ptr(), dec.state.data_ptr(),
                                                 dec.resident.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(), None,
                                                 out["results"].data_ptr(), out["records"].data_ptr(), strm), "mbx_process_batch_ragged")

    res["ragged_ms"] = timed(ragged, steps)
    if only_ragged:
        return res
    # the per-count launches: frames grouped by count, one indexed resident launch each
    groups = []
    for T in np.unique(counts):
        who = np.flatnonzero(counts == T)
        rows = np.concatenate([np.arange(off[i], off[i + 1]) for i in who])
        groups.append((int(T), len(who), torch.from_numpy(who.astype(np.int32)).to(dec.device), dec.to_device(frames[rows]),
                       dec.make_outputs(int(T), streams=len(who))))

    def per_count():
        for T, n, index, fr, o in groups:
            _native.check(L.mbx_process_batch_resident(codec, n, T, index.data_ptr(), fr.data_ptr(), dec.state.data_ptr(), dec.resident.data_ptr(),
                                                       dec.rng.data_ptr(), o["pcm16"].data_ptr(), None, o["results"].data_ptr(),
                                                       o["records"].data_ptr(), strm), "per-count launch")

    res["per_count_ms"] = timed(per_count, steps)
    res["per_count_launch_sets"] = len(groups)
    del groups
    padded = dec.to_device(framegen.random_frames(codec, S * Tmax, framegen.rng_for(8)))
    pout = dec.make_outputs(Tmax)
    res["padded_ms"] = timed(lambda: dec.decode(padded, Tmax, out=pout), steps)
    return res


def measure_mixed(shape, kind, S, steps):
    """the same streams decoded by ONE mbx_process_batch_mixed call and by one mbx_process_batch_ragged call per codec, alternating
    windows on one resident pool.  shape (i): four equal codec groups; (ii): one large group (IMBE) and three of 300 streams each."""
    import torch
    from mbelib_neo_amd import _native, decoder, framegen

    L = _native.lib()
    counts = counts_of(kind, S)
    rng = np.random.default_rng(0xC0DEC)
    codecs = (np.arange(S) % 4 if shape == "i" else np.concatenate([np.repeat([1, 2, 3], 300), np.zeros(S - 900, dtype=np.int64)])).astype(np.uint8)
    rng.shuffle(codecs)
    total = int(counts.sum())
    off = np.concatenate([[0], np.cumsum(counts)])
    dec = decoder.BatchDecoder(0, S, seeds=np.arange(S) + 1, resident=True)
    rows = np.zeros((total, decoder.MIXED_ROW_BYTES), np.uint8)
    per_codec = []
    for c in range(4):
        who = np.flatnonzero(codecs == c)
        at = np.concatenate([np.arange(off[i], off[i + 1]) for i in who])
        f = framegen.random_frames(c, len(at), framegen.rng_for(7 + c)).reshape(len(at), -1)
        rows[at, :f.shape[1]] = f
        coff = np.concatenate([[0], np.cumsum(counts[who])]).astype(np.int32)
        per_codec.append((c, len(who), len(at), torch.from_numpy(coff).to(dec.device), torch.from_numpy(who.astype(np.int32)).to(dec.device),
                          dec.to_device(f), dec.make_outputs(0, total=len(at))))
    d_rows, d_codec = dec.to_device(rows), torch.from_numpy(codecs).to(dec.device)
    d_off = torch.from_numpy(off.astype(np.int32)).to(dec.device)
    out = dec.make_outputs(0, total=total)
    _native.check(L.mbx_reserve(total + S + total // 256 + 8), "mbx_reserve")
    strm = torch.cuda.current_stream().cuda_stream

    def mixed():
        _native.check(L.mbx_process_batch_mixed(S, d_codec.data_ptr(), d_off.data_ptr(), total, None, d_rows.data_ptr(), dec.state.data_ptr(),
                                                dec.resident.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(), None,
                                                out["results"].data_ptr(), out["records"].data_ptr(), strm), "mbx_process_batch_mixed")

    def per_codec_calls():
        for c, n, tot, coff, index, fr, o in per_codec:
            _native.check(L.mbx_process_batch_ragged(c, n, coff.data_ptr(), tot, index.data_ptr(), fr.data_ptr(), dec.state.data_ptr(),
                                                     dec.resident.data_ptr(), dec.rng.data_ptr(), o["pcm16"].data_ptr(), None,
                                                     o["results"].data_ptr(), o["records"].data_ptr(), strm), "mbx_process_batch_ragged")

    ms = {"mixed": [], "per_codec": []}
    for _ in range(3):   # alternating windows: the spread between them is the noise of the box
        ms["mixed"].append(timed(mixed, steps))
        ms["per_codec"].append(timed(per_codec_calls, steps))
    return {"real_frames": total, "streams_per_codec": [int((codecs == c).sum()) for c in range(4)], **ms}


def main_mixed(args):
    print(f"{'shape':6} {'counts':6} {'streams per codec':>24} {'real frames':>11} {'one mixed call':>22} {'one ragged call per codec':>28}   "
          "(M real frames/s: median [min .. max] of 3 alternating windows)")
    for shape in ("i", "ii"):
        for kind in ("a", "b"):
            r = measure_mixed(shape, kind, args.streams, args.steps)
            cell = lambda v: "%.1f [%.1f .. %.1f]" % tuple(r["real_frames"] / x / 1e3 for x in (sorted(v)[1], max(v), min(v)))
            print(f"({shape:2})   ({kind})    {str(r['streams_per_codec']):>24} {r['real_frames']:>11} {cell(r['mixed']):>22} {cell(r['per_codec']):>28}",
                  flush=True)
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--mixed", action="store_true", help="one mixed-codec call against one ragged call per codec, on the same streams")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--streams", type=int, default=8192)
    ap.add_argument("--child", nargs=2, metavar=("CODEC", "KIND"), help="internal: ragged only, one JSON line")
    args = ap.parse_args()
    if args.mixed:
        return main_mixed(args)
    if args.child:
        print(json.dumps(measure(int(args.child[0]), args.child[1], args.streams, args.steps, True)))
        return 0
    print(f"{'codec':8} {'counts':6} {'real frames':>11} {'ragged':>12} {'ragged, grid order':>18} {'per count':>16} {'padded to max':>14}   (M real frames/s)")
    for codec, label in ((0, "IMBE"), (1, "AMBE+2")):
        for kind in ("a", "b"):
            r = measure(codec, kind, args.streams, args.steps, False)
            env = dict(os.environ, MBX_RAGGED_ORDER="0")
            child = subprocess.run([sys.executable, os.path.abspath(__file__), "--steps", str(args.steps), "--streams", str(args.streams),
                                    "--child", str(codec), kind], capture_output=True, text=True, timeout=600, env=env)
            if child.returncode != 0:
                sys.stderr.write(child.stdout[-2000:] + child.stderr[-2000:])
                return child.returncode if child.returncode > 0 else 1
            grid = json.loads(child.stdout.strip().splitlines()[-1])
            rate = lambda ms: r["real_frames"] / ms / 1e3
            print(f"{label:8} ({kind})    {r['real_frames']:>11} {rate(r['ragged_ms']):>12.1f} {rate(grid['ragged_ms']):>18.1f} "
                  f"{rate(r['per_count_ms']):>9.1f} ({r['per_count_launch_sets']:>3} sets) {rate(r['padded_ms']):>14.1f}", flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
