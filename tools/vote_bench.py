#!/usr/bin/env python3
"""vote_bench.py [--step | --kernel] [--candidates N] [--group G] [--steps N] [--rounds R] -- what voted streams (include/mbx_vote.h)
cost beside what a multi-site host runs today.  Built like bands_bench.py, whose helpers it uses.

Windows alternate in one process, `rounds` rounds, per form the best, the median and the spread (worst - best) of HIP-event times over
`steps` launches a window.

--step      IMBE x 1 on resident state: `candidates` (65,536) candidate frames in groups of `group` (4) sites.
              voted hard      mbx_process_batch_voted: the FEC launch over all candidates, select, the stream stage of candidates / group
                              voted streams
              voted soft      mbx_process_batch_soft_voted under MBX_VOTE_SELECT and under MBX_VOTE_COMBINE
              all candidates  mbx_process_batch_resident (and, "soft", mbx_process_batch_soft_resident) over all candidates as streams of
                              their own: what a host must run today before it can vote (on the PCM, on the host)
            Every voted line carries its ratio to the all-candidates step of its input form.
--kernel    mbx_vote_select alone over candidates / group voted frames beside mbx_pcm_levels on as many rows; mbx_vote_combine alone (184
            cells) beside the project's usual yardstick: the median of mbx_pcm_compand on `candidates` rows times the ratio of bytes moved,
            plus compand's own spread in this run; the line says whether it is inside.  The first frames are compared with the numpy
            definition (mbelib_neo_amd.vote) first.
Needs a GPU; prints one JSON line per measurement.  Development aid."""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from levels_bench import device_rows, summary, timed  # noqa: E402


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _sites(n_cand, group):
    """(hard candidates [n_cand, 18], soft candidates [n_cand, 184, 2]): voted stream s owns rows s * group ..., sites at 1 .. 4 % bit errors"""
    from mbelib_neo_amd import framegen, vote

    S = n_cand // group
    clean = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(0x566F7E00))
    ber = np.linspace(0.01, 0.04, group)
    rng = framegen.rng_for(0x566F7E01)
    hard = np.ascontiguousarray(vote.noisy_sites(clean, 0, ber, rng).transpose(1, 0, 2)).reshape(n_cand, 18)
    soft = np.ascontiguousarray(vote.noisy_soft_sites(clean, 0, ber, rng).transpose(1, 0, 2, 3)).reshape(n_cand, 184, 2)
    return hard, soft


def _report(mode, step, info, steps, rounds, against=None):
    times = {f: [] for f in step}
    for _ in range(rounds):
        for f in step:
            times[f].append(timed(step[f], steps))
    done = {f: summary(times[f]) for f in step}
    for f in step:
        line = {"mode": mode, "form": f, **{k: v for k, v in info.get(f, {}).items() if k not in ("yardstick_of", "byte_ratio")}, **done[f], "rounds": rounds,
                "launches_per_round": steps}
        if against and f in against:
            line["ratio_to_" + against[f].replace(" ", "_")] = round(done[f]["median_us"] / done[against[f]]["median_us"], 3)
        if "yardstick_of" in info.get(f, {}):
            ref = done[info[f]["yardstick_of"]]
            line["byte_ratio"] = round(info[f]["byte_ratio"], 3)
            line["yardstick_us"] = round(ref["median_us"] * info[f]["byte_ratio"] + ref["spread_us"], 2)
            line["inside_yardstick"] = bool(done[f]["median_us"] <= line["yardstick_us"])
        print(json.dumps(line), flush=True)


def whole_step(n_cand, group, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, vote
    from mbelib_neo_amd.layout import init_state, rng_seeded

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    S = n_cand // group
    hard, soft = _sites(n_cand, group)
    d_hard, d_soft = _dev(hard), _dev(soft)
    plan = vote.Plan(np.arange(S + 1, dtype=np.int64) * group)

    def pool(n):
        one = torch.from_numpy(init_state(1).reshape(-1).view(np.uint8).copy()).cuda()
        return {"state": one.repeat(n), "rng": _dev(rng_seeded(np.arange(n) + 1)), "resident": torch.zeros(n, dtype=torch.int32, device="cuda"),
                "pcm16": torch.empty((n, 160), dtype=torch.int16, device="cuda"), "results": torch.empty((n, 5), dtype=torch.int32, device="cuda"),
                "records": torch.empty((n, 4), dtype=torch.int32, device="cuda")}

    voted, every = pool(S), pool(n_cand)
    votes = torch.empty((S, 8), dtype=torch.uint8, device="cuda")
    _native.check(L.mbx_reserve_stream(strm, max(plan.workspace_frames(0, vote.SELECT, 1), plan.workspace_frames(0, vote.COMBINE, 1), n_cand)), "reserve")

    def tail(p, v):
        return (None, p["state"].data_ptr(), p["resident"].data_ptr(), p["rng"].data_ptr(), p["pcm16"].data_ptr(), None, p["results"].data_ptr(), p["records"].data_ptr(),
                v, strm)

    step = {
        "voted hard": lambda: _native.check(L.mbx_process_batch_voted(plan.handle, 0, 1, None, d_hard.data_ptr(), *tail(voted, votes.data_ptr())), "voted"),
        "voted soft select": lambda: _native.check(L.mbx_process_batch_soft_voted(plan.handle, 0, vote.SELECT, 1, None, d_soft.data_ptr(), *tail(voted, votes.data_ptr())), "voted"),
        "voted soft combine": lambda: _native.check(L.mbx_process_batch_soft_voted(plan.handle, 0, vote.COMBINE, 1, None, d_soft.data_ptr(), *tail(voted, votes.data_ptr())), "voted"),
        "all candidates": lambda: _native.check(L.mbx_process_batch_resident(0, n_cand, 1, None, d_hard.data_ptr(), every["state"].data_ptr(), every["resident"].data_ptr(),
                                                                             every["rng"].data_ptr(), every["pcm16"].data_ptr(), None, every["results"].data_ptr(),
                                                                             every["records"].data_ptr(), strm), "resident"),
        "all candidates soft": lambda: _native.check(L.mbx_process_batch_soft_resident(0, n_cand, 1, None, d_soft.data_ptr(), every["state"].data_ptr(),
                                                                                       every["resident"].data_ptr(), every["rng"].data_ptr(), every["pcm16"].data_ptr(), None,
                                                                                       every["results"].data_ptr(), every["records"].data_ptr(), strm), "soft resident"),
    }
    info = {f: {"candidates": n_cand, "group": group, "streams": n_cand if f.startswith("all candidates") else S} for f in step}
    for f in step:   # the kernel that ran, once
        step[f]()
        torch.cuda.synchronize()
        info[f]["stream_kernel"] = L.mbx_last_kernel_name(strm).decode()
    _report("step", step, info, steps, rounds, against={"voted hard": "all candidates", "voted soft select": "all candidates soft", "voted soft combine": "all candidates soft"})
    plan.close()


def kernel(n_cand, group, steps, rounds):
    import torch
    from mbelib_neo_amd import _native, decoder, pcm8, vote

    decoder.ensure_init(0)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream
    S = n_cand // group
    off = np.arange(S + 1, dtype=np.int64) * group
    plan = vote.Plan(off)
    rng = np.random.default_rng(3)
    rec = rng.integers(0, 2**32, size=(n_cand, 1, 4), dtype=np.uint32)
    rec[..., 3] = rng.integers(0, 4, size=(n_cand, 1)) | (rng.integers(0, 4, size=(n_cand, 1)) << 8)
    _, soft = _sites(n_cand, group)
    d_rec, d_soft = _dev(rec), _dev(soft)
    out_rec = torch.empty((S, 4), dtype=torch.int32, device="cuda")
    out_soft = torch.empty(S * 368, dtype=torch.uint8, device="cuda")
    votes = torch.empty((S, 8), dtype=torch.uint8, device="cuda")
    check = min(S, 300)
    _native.check(L.mbx_vote_select(plan.handle, 1, d_rec.data_ptr(), None, out_rec.data_ptr(), votes.data_ptr(), strm), "select")
    torch.cuda.synchronize()
    want, want_votes = vote.select(rec[:check * group], None, off[:check + 1], 1)
    assert out_rec[:check].cpu().numpy().tobytes() == want.tobytes() and votes[:check].cpu().numpy().tobytes() == want_votes.tobytes(), "select"
    _native.check(L.mbx_vote_combine(plan.handle, 184, 1, d_soft.data_ptr(), None, out_soft.data_ptr(), votes.data_ptr(), strm), "combine")
    torch.cuda.synchronize()
    want, want_votes = vote.combine(soft[:check * group].reshape(check * group, 1, 184, 2), None, off[:check + 1], 1)
    assert out_soft[:check * 368].cpu().numpy().tobytes() == want.tobytes() and votes[:check].cpu().numpy().tobytes() == want_votes.tobytes(), "combine"
    x_s, x_c = device_rows(S), device_rows(n_cand)
    lv = torch.empty((S, 16), dtype=torch.uint8, device="cuda")
    out8 = torch.empty(n_cand * 160, dtype=torch.uint8, device="cuda")
    compand = f"compand ulaw {n_cand} rows"
    step = {
        f"select {S} frames of {group}": lambda: L.mbx_vote_select(plan.handle, 1, d_rec.data_ptr(), None, out_rec.data_ptr(), votes.data_ptr(), strm),
        f"levels {S} rows": lambda: L.mbx_pcm_levels(x_s.data_ptr(), S, lv.data_ptr(), strm),
        f"combine {S} frames of {group}": lambda: L.mbx_vote_combine(plan.handle, 184, 1, d_soft.data_ptr(), None, out_soft.data_ptr(), votes.data_ptr(), strm),
        compand: lambda: L.mbx_pcm_compand(pcm8.LAW_ULAW, x_c.data_ptr(), n_cand, out8.data_ptr(), strm),
    }
    moved = n_cand * 368 + S * 368 + S * 8
    info = {
        f"select {S} frames of {group}": {"bytes_moved_per_launch": n_cand * 16 + S * 24},
        f"levels {S} rows": {"bytes_moved_per_launch": 336 * S},
        f"combine {S} frames of {group}": {"bytes_moved_per_launch": moved, "yardstick_of": compand, "byte_ratio": moved / (480 * n_cand)},
        compand: {"bytes_moved_per_launch": 480 * n_cand},
    }
    _report("kernel", step, info, steps, rounds)
    plan.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--candidates", type=int, default=65536)
    ap.add_argument("--group", type=int, default=4)
    ap.add_argument("--steps", type=int, default=100)
    ap.add_argument("--rounds", type=int, default=7)
    a_ = ap.parse_args()
    if a_.step or not a_.kernel:
        whole_step(a_.candidates, a_.group, a_.steps, a_.rounds)
    if a_.kernel or not a_.step:
        kernel(a_.candidates, a_.group, a_.steps, a_.rounds)
