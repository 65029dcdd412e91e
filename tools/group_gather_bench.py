#!/usr/bin/env python3
"""group_gather_bench.py [--bursts N] [--steps K] [--rounds R] -- what ONE gather launch over four burst groups costs next to the four
mbx_deinterleave launches it replaces (include/mbx_burst_groups.h).

Four groups of N bursts each (default 16,384), one burst per stream, in the two hard SHAPES of tools/burst_bench.py and mixed forms:
"dmr" = AMBE+2, 3 frames in 264 bits, once packed and once as dibit bytes with an inversion sequence; "ldu" = IMBE, 9 frames in
1,728 bits, once packed and once as bit bytes.  The groups gather has no entry point of its own, so it is timed inside its call:

  groups   mbx_process_burst_groups: ONE gather launch (which also writes the step's layout words), then the mixed step
  four     the route it replaces: four mbx_deinterleave launches into mixed rows, then mbx_process_batch_mixed on layout arrays that
           were uploaded ONCE, outside the timed windows (a host doing this per tick pays three more uploads)
  gathers  the four mbx_deinterleave launches alone
  step     mbx_process_batch_mixed alone, on rows gathered before

HIP-event time per call, `steps` calls a window, the four windows alternating, `rounds` rounds, in one process: per line the best, the
median and the spread (worst - best) over the rounds.  groups - step against gathers is one launch against four; groups against four is
what a host sees.  The outputs of `groups` and `four` are compared byte for byte first.  Needs a GPU; prints one JSON line per
measurement.  Development aid."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

# (codec, frames per burst, burst bits, form, inversion sequence)
GROUPS = ((1, 3, 264, "packed", False), (1, 3, 264, "dibits", True), (0, 9, 1728, "packed", False), (0, 9, 1728, "bits", False))


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


def main(N, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, bursts as B, decoder

    L = _native.lib()
    forms = {"packed": B.FORM_PACKED, "bits": B.FORM_BITS, "dibits": B.FORM_DIBITS}
    rng = np.random.default_rng(1)
    S = len(GROUPS) * N
    decs = [decoder.BatchDecoder(0, S, resident=True) for _ in range(2)]
    strm = torch.cuda.current_stream().cuda_stream
    groups = []
    for i, (codec, F, bits, form, masked) in enumerate(GROUPS):
        mask = rng.integers(0, 2, size=bits, dtype=np.uint8) if masked else None
        s = B.random_schedule(codec, F, bits, rng, device=True, form=forms[form], invert=mask)
        raw = B.to_form(s, rng.integers(0, 256, size=(N, s.packed_bytes), dtype=np.uint8))
        groups.append(B.BurstGroup(s, torch.from_numpy(np.ascontiguousarray(raw).reshape(-1)).cuda(), N, 1, first_slot=i * N))
    rows_of = B.group_rows(groups)
    total = int(rows_of[-1])
    out = [d.make_outputs(0, want_pcm16=True, want_results=False, total=total) for d in decs]
    arr = B.group_structs(groups, [(g.bursts.data_ptr(), 0) for g in groups])
    # the route it replaces: rows, and the layout arrays a host builds and uploads
    rows = torch.zeros((total, B.MIXED_ROW_BYTES), dtype=torch.uint8, device="cuda")
    counts = np.concatenate([np.full(N, g.schedule.frames_per_burst) for g in groups])
    d_off = torch.from_numpy(np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)).cuda()
    d_codec = torch.from_numpy(np.concatenate([np.full(N, g.schedule.codec, dtype=np.uint8) for g in groups])).cuda()

    def tail(k):
        d, o = decs[k], out[k]
        return (d.state.data_ptr(), d.resident.data_ptr(), d.rng.data_ptr(), o["pcm16"].data_ptr(), None, None, o["records"].data_ptr(), strm)

    def run_groups():
        _native.check(L.mbx_process_burst_groups(arr, len(groups), 0, *tail(0)), "mbx_process_burst_groups")

    def run_gathers():
        for g, first in zip(groups, rows_of[:-1]):
            _native.check(L.mbx_deinterleave(g.schedule.handle, g.bursts.data_ptr(), g.burst_stride, N, rows[int(first):].data_ptr(), B.MIXED_ROW_BYTES, strm),
                          "mbx_deinterleave")

    def run_step():
        _native.check(L.mbx_process_batch_mixed(S, d_codec.data_ptr(), d_off.data_ptr(), total, None, rows.data_ptr(), *tail(1)), "mbx_process_batch_mixed")

    def run_four():
        run_gathers()
        run_step()

    run_groups()
    run_four()
    torch.cuda.synchronize()
    assert torch.equal(out[0]["pcm16"], out[1]["pcm16"]) and torch.equal(out[0]["records"], out[1]["records"]), "the two routes differ"
    assert torch.equal(decs[0].state, decs[1].state) and torch.equal(decs[0].rng, decs[1].rng)
    runs = {"groups": run_groups, "four": run_four, "gathers": run_gathers, "step": run_step}
    times = {k: [] for k in runs}
    for _ in range(rounds):
        for k, fn in runs.items():
            times[k].append(timed(fn, steps))
    for k in runs:
        t = sorted(times[k])
        print(json.dumps({"what": k, "groups": len(groups), "bursts_per_group": N, "frames": total, "best_us": round(1e3 * t[0], 2),
                          "median_us": round(1e3 * t[len(t) // 2], 2), "spread_us": round(1e3 * (t[-1] - t[0]), 2), "rounds": rounds,
                          "calls_per_round": steps}), flush=True)
    for g in groups:
        g.schedule.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--bursts", type=int, default=16384)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    a = ap.parse_args()
    main(a.bursts, a.steps, a.rounds)
