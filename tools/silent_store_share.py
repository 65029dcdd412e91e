#!/usr/bin/env python3
"""silent_store_share.py [streams=512] [ticks=12] -- how often the one-frame instances' silent-store rule can apply, counted on the
CPU oracle (no GPU needed): per bench workload's frame generator, `streams` streams x `ticks` ticks of T = 1, the first two ticks
left out.  `after` = share of frames whose cur_mp.previousUw is 256 dwords of 0x00000000 after the frame; `skip` = share of frames
where it was that before the frame too (the store of cur_mp.previousUw is then a store of zeros over zeros: store_parms / UwSkip in
csrc/mbx_stream.hip).  Synthetic generators only: the share in real speech is not measured by this."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import bench  # noqa: E402
import oracle_lib  # noqa: E402


def main():
    S = int(sys.argv[1]) if len(sys.argv) > 1 else 512
    ticks = int(sys.argv[2]) if len(sys.argv) > 2 else 12
    o = oracle_lib.load()
    for name in ("imbe_voiced", "ambe_fec", "ambe_stream", "imbe_mixed"):
        codec = bench.WORKLOADS[name][0]
        frames = bench.make_frames(name, codec, S, ticks, 0).reshape(S, ticks, -1)
        state, rng = o.init_state(S), o.rng_seeded(np.arange(S) + 1)
        zero_before = np.zeros(S, dtype=bool)
        after = skip = total = 0
        for t in range(ticks):
            ref = o.process_batch(codec, S, 1, frames[:, t], state, rng)
            state, rng = ref["state"], ref["rng"]
            zero = ~ref["state"][:, 0]["previousUw"].view(np.uint32).any(axis=1)
            if t >= 2:
                after += int(zero.sum())
                skip += int((zero & zero_before).sum())
                total += S
            zero_before = zero
        print(f"{name:12s} frames {total:6d}  after {after / total:.3f}  skip {skip / total:.3f}")


if __name__ == "__main__":
    main()
