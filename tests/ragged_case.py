"""The skewed ragged batch of tests/test_gpu_ragged.py, runnable as a child process: more streams than the device has resident wave
slots, 97 % of them with 1..4 frames and 3 % with 150, decoded by ONE mbx_process_batch_ragged call on resident state.
`python ragged_case.py <codec>` prints a SHA-256 over every output, the state and the RNG state (under the environment it was
started in: the parent compares MBX_RAGGED_ORDER=0 with the default).  Test infrastructure."""
import hashlib
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for d in (HERE, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

S_SKEWED, LONG = 6500, 150


def skewed_counts(S=S_SKEWED):
    rng = np.random.default_rng(0x5EED)
    counts = rng.integers(1, 5, size=S)
    counts[rng.choice(S, size=(3 * S) // 100, replace=False)] = LONG
    return counts


def ragged_frames(codec, counts, tag, soft=False):
    """frames of stream i = the first counts[i] frames of stream i of the edge mix (soft: of the soft mix), concatenated"""
    import edge_mix
    import soft_mix

    S, Tmax = len(counts), int(max(counts.max(initial=0), 1))
    if soft:
        full = soft_mix.frames(codec, S, Tmax, tag).reshape(S, Tmax, -1)
    else:
        full = edge_mix.frames(codec, S, Tmax, tag).reshape(S, Tmax, -1)
    keep = np.arange(Tmax)[None, :] < np.asarray(counts)[:, None]
    return np.ascontiguousarray(full[keep])


def digest(out, dec):
    h = hashlib.sha256()
    for k in ("records", "results", "pcm16", "pcmf"):
        h.update(out[k].cpu().numpy().tobytes())
    h.update(dec.state_numpy().tobytes())
    h.update(dec.rng_numpy().tobytes())
    return h.hexdigest()


def run_skewed(codec):
    import torch
    from mbelib_neo_amd import _native, decoder

    counts = skewed_counts()
    dec = decoder.BatchDecoder(codec, len(counts), seeds=np.arange(len(counts)) * 5 + 1, resident=True)
    out = dec.decode_ragged(ragged_frames(codec, counts, tag=4), counts, want_float=True)
    name = _native.lib().mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream).decode()
    torch.cuda.synchronize()
    return out, dec, name


if __name__ == "__main__":
    out, dec, name = run_skewed(int(sys.argv[1]))
    print(name, digest(out, dec))
