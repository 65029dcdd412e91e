"""Shared cases of the voted-stream tests (tests/test_vote_host.py on the CPU, tests/test_gpu_vote.py on the device): the grouping of
every shape test, records crafted for every clause of the select rule with their answers written out by hand, random records and cells,
the three forms of the present bytes, and the four noisy sites of the decoding experiment.  numpy only; what is made once is handed
out read-only."""
import numpy as np

from mbelib_neo_amd import framegen, vote

OFFSETS = np.array([0, 1, 3, 6, 22, 54], dtype=np.int32)   # S = 5 groups of 1, 2, 3, 16 and 32 candidates: C = 54
S, C = 5, 54
FRAMES = (1, 3)                                              # T
CELLS = {0: 184, 1: 96, 2: 168, 3: 96}                       # row_cells by codec


def w3(c0, prot, c4=0, flags=0):
    return np.uint32(c0 | (prot << 8) | (c4 << 16) | (flags << 24))


def crafted_select():
    """(records uint32 [C, 1, 4], present uint8 [C, 1], offsets, answers): one group per clause of the rule, T = 1.  answers[s] is
    (row of the winner's record in `records`, winner, present, best, second, agree), written out by hand."""
    groups = []   # per group: list of (w0, c0, prot, present)
    answers = []
    # 0: a tie on the total (3) broken by c0: candidate 1 has the smaller c0
    groups.append([(10, 2, 1, 1), (11, 1, 2, 1)])
    answers.append((1, 1, 2, 3, 3, 0b10))
    # 1: a tie on both broken by the lower index; all three hold the same words: agree is the mask of the present
    groups.append([(20, 1, 1, 1), (20, 1, 1, 1), (20, 1, 1, 1)])
    answers.append((0, 0, 3, 2, 2, 0b111))
    # 2: the winner is the last of 32
    groups.append([(30 + j, 2, 3, 1) for j in range(31)] + [(99, 0, 0, 1)])
    answers.append((31, 31, 32, 0, 5, 1 << 31))
    # 3: absent candidates are skipped: candidate 0 has no error and is not there
    groups.append([(40, 0, 0, 0), (41, 1, 3, 1), (42, 2, 0, 1)])
    answers.append((2, 2, 2, 2, 4, 0b100))
    # 4: nobody is there: candidate 0's record as it stands, MBX_VOTE_NONE
    groups.append([(50, 7, 7, 0), (51, 0, 0, 0), (52, 0, 0, 0)])
    answers.append((0, vote.NONE, 0, 255, 255, 0))
    # 5: agree and second by hand: the winner is candidate 2; 0 and 3 hold its words, 3 is absent, 1 holds others and is the runner-up
    groups.append([(60, 1, 2, 1), (61, 1, 0, 1), (60, 0, 0, 1), (60, 0, 0, 0)])
    answers.append((2, 2, 3, 0, 1, 0b0101))
    # 6: one candidate with more than 255 errors: best saturates, there is no runner-up
    groups.append([(70, 200, 100, 1)])
    answers.append((0, 0, 1, 255, 255, 0b1))
    off = np.concatenate([[0], np.cumsum([len(g) for g in groups])]).astype(np.int32)
    rec = np.zeros((off[-1], 1, 4), dtype=np.uint32)
    present = np.zeros((off[-1], 1), dtype=np.uint8)
    at = 0
    for g in groups:
        for (w0, c0, prot, there) in g:
            rec[at, 0] = (w0, w0 * 3 + 1, w0 ^ 0xABCD, w3(c0, prot, c4=at & 3, flags=2))
            present[at, 0] = there * (1 + at)   # (non-zero means present: any value)
            at += 1
    rows = [(int(off[s]) + a[0],) + a[1:] for s, a in enumerate(answers)]
    return rec, present, off, rows


def random_records(rng, n_cand, T):
    """records with error counts small enough to tie often, words that repeat inside a group now and then"""
    rec = rng.integers(0, 2**32, size=(n_cand, T, 4), dtype=np.uint32)
    c0 = rng.integers(0, 3, size=(n_cand, T)).astype(np.uint32)
    prot = rng.integers(0, 4, size=(n_cand, T)).astype(np.uint32)
    big = rng.random((n_cand, T)) < 0.05
    c0 = np.where(big, 255, c0).astype(np.uint32)
    prot = np.where(big, rng.integers(0, 256, size=(n_cand, T)), prot).astype(np.uint32)
    rec[..., 3] = c0 | (prot << 8) | (rec[..., 3] & 0xFFFF0000)
    same = rng.random((n_cand, T)) < 0.4   # copies of the candidate in front: equal words with other error counts
    for c in range(1, n_cand):
        rec[c, :, :3] = np.where(same[c, :, None], rec[c - 1, :, :3], rec[c, :, :3])
    return rec


def random_cells(rng, n_cand, T, row_cells):
    """valid cells: bits 0 / 1, reliabilities of every size, a share of zeros so that V = 0 happens"""
    cells = np.empty((n_cand, T, row_cells, 2), dtype=np.uint8)
    cells[..., 0] = rng.integers(0, 2, size=cells.shape[:-1])
    rel = rng.integers(0, 256, size=cells.shape[:-1])
    rel = np.where(rng.random(cells.shape[:-1]) < 0.3, rng.integers(0, 3, size=cells.shape[:-1]), rel)
    cells[..., 1] = rel
    return cells


PRESENT_FORMS = ("null", "random", "stream-gone")


def present_of(form, rng, T, off=OFFSETS):
    """None | random bytes, a little over half of them non-zero | everybody there but every candidate of stream 3 at every frame"""
    n_cand = int(off[-1])
    if form == "null":
        return None
    if form == "random":
        return (rng.integers(1, 256, size=(n_cand, T)) * (rng.random((n_cand, T)) < 0.6)).astype(np.uint8)
    assert form == "stream-gone"
    p = np.ones((n_cand, T), dtype=np.uint8)
    p[off[3]:off[4]] = 0
    return p


# ---- the decoding experiment: 200 clean voiced IMBE 7200x4400 frames heard by four sites ---------------------------------------------
SITE_BER = (0.02, 0.02, 0.02, 0.02)   # four sites of equal quality: the case a voter exists for (with one site always best there is nothing to vote on)
N_FRAMES = 200
_SITES = {}


def sites():
    """(clean wire frames [200, 18], hard candidates uint8 [4, 200, 18], soft candidates uint8 [4, 200, 184, 2]); generators
    framegen.rng_for(2001) for the frames and rng_for(2002) for the sites, the hard sites drawn first"""
    if not _SITES:
        clean = framegen.imbe_clean_voiced_frames(N_FRAMES, framegen.rng_for(2001))
        rng = framegen.rng_for(2002)
        hard = vote.noisy_sites(clean, 0, SITE_BER, rng)
        soft = vote.noisy_soft_sites(clean, 0, SITE_BER, rng)
        for a in (clean, hard, soft):
            a.setflags(write=False)
        _SITES["it"] = (clean, hard, soft)
    return _SITES["it"]


def same_parameters(records, clean_records):
    """frames whose parameter bits (w[0..2]) equal the clean ones"""
    a, b = np.asarray(records).reshape(-1, 4), np.asarray(clean_records).reshape(-1, 4)
    return int((a[:, :3] == b[:, :3]).all(axis=1).sum())
