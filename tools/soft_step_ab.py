#!/usr/bin/env python3
"""soft_step_ab.py <rounds> <names...> -- GPU box: interleaved A/B of the SOFT batch step (mbx_process_batch_soft, 65,536 x T = 1,
framegen.soft_frames_coded) between variant libraries (mbelib-neo_amd/variants/libmbx_hip_<name>.so, tools/variant.sh / mkbase.sh;
"product" = the library in the tree), the way tools/abx.sh compares bench workloads -- bench.py has no workload on this entry point.
Every measurement is a fresh child process under a time limit of its own (steady state: 50 untimed launches, then 400 between two
events); the first child that fails ends the run.  Prints the median step time per codec and variant, relative to the first name.
Development aid."""
import os
import statistics
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(codec):
    import numpy as np
    import torch

    sys.path.insert(0, ROOT)
    from mbelib_neo_amd import _native, decoder, framegen

    S, T = 65536, 1
    soft = framegen.soft_frames_coded(codec, S * T, framegen.rng_for(99 + codec))
    dec = decoder.BatchDecoder(codec, S, seeds=np.arange(S) + 1)
    d = dec.to_device(soft)
    out = dec.make_outputs(T)
    L = _native.lib()
    strm = torch.cuda.current_stream().cuda_stream

    def go():
        rc = L.mbx_process_batch_soft(codec, S, T, d.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), out["pcm16"].data_ptr(), None,
                                      out["results"].data_ptr(), out["records"].data_ptr(), strm)
        assert rc == 0, rc

    for _ in range(50):
        go()
    torch.cuda.synchronize()
    n = 400
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(n):
        go()
    b.record()
    torch.cuda.synchronize()
    print(f"RESULT {a.elapsed_time(b) / n:.5f} {out['pcm16'].to(torch.int64).sum().item()}")


def main():
    if sys.argv[1] == "--child":
        return child(int(sys.argv[2]))
    rounds, names = int(sys.argv[1]), sys.argv[2:]
    res, digest = {}, {}
    for _ in range(rounds):
        for codec in (0, 1):
            for name in names:
                env = dict(os.environ)
                if name != "product":
                    env["MBX_HIP_LIBRARY"] = os.path.join(ROOT, "mbelib-neo_amd", "variants", f"libmbx_hip_{name}.so")
                    env["MBX_HIP_LIBRARY_ALLOW_OLDER"] = "1"
                out = subprocess.run([sys.executable, os.path.abspath(__file__), "--child", str(codec)], env=env, capture_output=True, text=True,
                                     timeout=180)
                if out.returncode != 0:
                    print("FAILED", codec, name, out.returncode, out.stderr[-1500:])
                    return 1
                _, ms, pcm = out.stdout.strip().splitlines()[-1].split()
                res.setdefault((codec, name), []).append(float(ms))
                digest.setdefault(codec, set()).add(pcm)
    for codec in (0, 1):
        base = statistics.median(res[(codec, names[0])])
        for name in names:
            v = res[(codec, name)]
            print(f"codec {codec} {name:10s} median {statistics.median(v):.4f} ms  min {min(v):.4f}  ({statistics.median(v) / base - 1:+.2%} vs {names[0]})  {v}")
        print(f"codec {codec} PCM digests of all variants equal: {len(digest[codec]) == 1}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
