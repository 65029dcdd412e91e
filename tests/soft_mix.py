"""Soft-decision edge streams for the soft batch paths: the hard-decision edge mix (tests/edge_mix.py: voice, random bits, runs of
uncorrectable frames into repeat and mute, all-zero / all-one frames, AMBE tones and erasures) turned into mbe_soft_bit cells in
the reference's array shapes, with a reliability script per frame that visits what the soft search has rules for."""
import numpy as np

import edge_mix
from mbelib_neo_amd import framegen
from mbelib_neo_amd.layout import FRAME_CELLS, ROW_WIDTHS

CELLS = {0: 184, 1: 96, 2: 168, 3: 96}


def cells_from_packed(codec, packed):
    """packed wire frames [n, 18|9] -> hard decisions [n, cells] in the reference's [rows][cols] order and the mask of used cells
    (the first wire bit of a row is its highest cell, as in framegen.soft_frames_coded)"""
    rows, cols = FRAME_CELLS[codec]
    wire = np.unpackbits(np.ascontiguousarray(packed, dtype=np.uint8), axis=1)
    bits = np.zeros((len(packed), rows, cols), dtype=np.uint8)
    used = np.zeros((rows, cols), dtype=bool)
    off = 0
    for r, w in enumerate(ROW_WIDTHS[codec]):
        bits[:, r, :w] = wire[:, off:off + w][:, ::-1]
        used[r, :w] = True
        off += w
    return bits.reshape(len(packed), rows * cols), used.reshape(-1)


def frames(codec, S, T, tag):
    """uint8 [S * T, cells, 2] = (bit, reliability), stream-major.  Frame f follows reliability script f % 6:
    0 a noisy observation (wrong hard decisions carry low confidence: the search corrects what the hard decoder cannot),
    1 all-zero reliability (every candidate costs 0: the tie rules alone decide), 2 all 255, 3 three-level confidences (many
    equal costs), 4 random confidences on the clean hard decisions, 5 a noisy observation with unused cells set to junk."""
    rng = framegen.rng_for(0x50F70000 + 64 * int(tag) + codec)
    packed = edge_mix.frames(codec, S, T, tag).reshape(S * T, -1)
    hard, used = cells_from_packed(codec, packed)
    n, cells = hard.shape
    obs = (2.0 * hard - 1.0) * 1.6 + rng.normal(0.0, 1.0, size=hard.shape)
    noisy_hard = (obs > 0).astype(np.uint8)
    noisy_rel = np.clip(np.abs(obs) * 40.0, 0, 255).astype(np.uint8)
    script = np.arange(n) % 6
    bit = np.where(np.isin(script, (0, 3, 5))[:, None], noisy_hard, hard)
    rel = noisy_rel.copy()
    rel[script == 1] = 0
    rel[script == 2] = 255
    rel[script == 3] = (rel[script == 3] // 96) * 96
    rel[script == 4] = rng.integers(0, 256, size=(int((script == 4).sum()), cells), dtype=np.uint8)
    junk = (script == 5)[:, None] & ~used[None, :]
    bit = np.where(junk, rng.integers(0, 2, size=bit.shape, dtype=np.uint8), np.where(used[None, :], bit, 0))
    rel = np.where(junk, rng.integers(0, 256, size=rel.shape, dtype=np.uint8), np.where(used[None, :], rel, 0))
    return np.ascontiguousarray(np.stack([bit, rel], axis=-1).astype(np.uint8))
