"""Mixed-codec ragged batches for tests/test_gpu_mixed.py: every stream row brings a codec (all four) and a frame count of its own.
Frames are those of tests/ragged_case.py per codec (edge mix / soft mix, cut to the counts), packed into rows of one size.
`python mixed_case.py` decodes the skewed batch (more streams than resident wave slots) by ONE mbx_process_batch_mixed call on
resident state and prints the kernel that ran and a SHA-256 over every output, the state and the RNG state, under the environment it
was started in: the parent compares MBX_RAGGED_ORDER=0 with the default.  Test infrastructure."""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for d in (HERE, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

import ragged_case  # noqa: E402

ROW_BYTES, ROW_CELLS = 18, 184


def codecs_for(S, seed):
    return np.random.default_rng(seed).integers(0, 4, size=S).astype(np.uint8)


def rows_of(counts, streams):
    off = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    return np.concatenate([np.arange(off[i], off[i + 1]) for i in streams]) if len(streams) else np.zeros(0, dtype=np.int64)


def mixed_frames(codecs, counts, tag, soft=False):
    """(rows, own): rows = uint8 [total, 18] (soft: [total, 184 * 2]) as the mixed calls take them; own[c] = (streams of codec c, their
    batch rows, their frames in the codec's own size: what a single-codec ragged call and the oracle take)"""
    counts = np.asarray(counts)
    rows = np.zeros((int(counts.sum()), ROW_CELLS * 2 if soft else ROW_BYTES), dtype=np.uint8)
    own = {}
    for c in range(4):
        who = np.flatnonzero(codecs == c)
        if who.size == 0:
            continue
        f = ragged_case.ragged_frames(c, counts[who], tag, soft=soft)
        f = f.reshape(f.shape[0], -1)
        at = rows_of(counts, who)
        rows[at, :f.shape[1]] = f
        own[c] = (who, at, f)
    return rows, own


def run_skewed():
    import torch
    from mbelib_neo_amd import _native, decoder

    counts = ragged_case.skewed_counts()
    codecs = codecs_for(len(counts), 77)
    rows, _ = mixed_frames(codecs, counts, tag=4)
    dec = decoder.BatchDecoder(0, len(counts), seeds=np.arange(len(counts)) * 5 + 1, resident=True)
    out = dec.decode_ragged(rows, counts, want_float=True, codec=codecs)
    name = _native.lib().mbx_last_kernel_name(torch.cuda.current_stream().cuda_stream).decode()
    torch.cuda.synchronize()
    return out, dec, name, codecs, counts


if __name__ == "__main__":
    out, dec, name, _, _ = run_skewed()
    print(name, ragged_case.digest(out, dec))
