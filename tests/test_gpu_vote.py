"""GPU suite (-m gpu) for voted streams (include/mbx_vote.h).  Shapes: S = 5 voted streams in groups of 1, 2, 3, 16 and 32 candidates
(C = 54), T = 1 and 3, all four codecs, the present bytes absent, random, or all zero for one stream (tests/vote_cases.py).
mbx_vote_select and mbx_vote_combine are held byte for byte to the numpy definition (mbelib_neo_amd.vote) between guard bands at exactly
the alignment of their contract; the whole steps -- hard voted, soft voted under select, soft voted under combine -- byte for byte to
the same pool run through the existing front call (mbx_fec_* / mbx_fec_soft), numpy's select or combine on the host, and
mbx_process_records or its resident form on the chosen records, with identity and with d_stream_index, on ABI triplets and on resident
state; one voted IMBE and one voted AMBE+2 batch to the CPU oracle on the winners' frames under the bounds of tests/parity.py; a
captured voted step replayed twice; the launchers' refusals that need a plan; the decoding experiment of the CPU suite through
mbx_fec_host / mbx_fec_soft_host.  Nothing here starts a child process."""

import numpy as np
import pytest

import guarded
import parity
import vote_cases as VC
from mbelib_neo_amd import framegen, vote
from mbelib_neo_amd.layout import FRAME_BYTES, PARMS_DTYPE, RECORD_DTYPE, RESULT_DTYPE, RNG_DTYPE, init_state, rng_seeded

pytestmark = pytest.mark.gpu
INVALID = -1
STREAM_CODEC = {0: 0, 1: 1, 2: 0, 3: 3}
POOL = 9                                   # slots of the indexed pool
INDEX = np.array([7, 0, 4, 2, 8], dtype=np.int32)   # voted stream s works on slot INDEX[s]; slots 1, 3, 5, 6 stay as they are
FORMS = ("hard", "soft-select", "soft-combine")


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


def _L():
    from mbelib_neo_amd import _native

    return _native.lib()


def _stream():
    import torch

    return torch.cuda.current_stream().cuda_stream


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a).reshape(-1).view(np.uint8).copy()).cuda()


def _ptr(t):
    return None if t is None else t.data_ptr()


@pytest.fixture(scope="module")
def plan(mbx):
    with vote.Plan(VC.OFFSETS) as p:
        assert (p.streams, p.candidates) == (VC.S, VC.C)
        L = _L()
        assert L.mbx_vote_plan_streams(p.handle) == VC.S and L.mbx_vote_plan_candidates(p.handle) == VC.C
        yield p


# ---- 1. launch parity ---------------------------------------------------------------------------------------------------------------------
def _select_between_guards(p, n_streams, n_cand, T, rec, present, with_votes, seed):
    import torch

    specs = [guarded.buf("cand", 16 * n_cand * T, "records", True), guarded.buf("records", 16 * n_streams * T, "records"), guarded.buf("votes", 8 * n_streams * T, "rng")]
    if present is not None:
        specs.append(guarded.buf("present", n_cand * T, "frames", True))
    arena = guarded.Arena(specs, where="cuda", seed=seed)
    assert arena.ptr("cand") % 32 == 16 and arena.ptr("records") % 32 == 16 and arena.ptr("votes") % 16 == 8
    arena.load("cand", rec)
    if present is not None:
        arena.load("present", present)
    arena.prefill("records", "votes")
    rc = _L().mbx_vote_select(p.handle, T, arena.ptr("cand"), arena.ptr("present") if present is not None else None, arena.ptr("records"),
                              arena.ptr("votes") if with_votes else None, _stream())
    assert rc == 0, _L().mbx_last_error()
    torch.cuda.synchronize()
    arena.check(f"select T {T} votes {with_votes}")
    return arena.read("records"), arena.read("votes"), arena.prefill_bytes("votes")


@pytest.mark.parametrize("form", VC.PRESENT_FORMS)
@pytest.mark.parametrize("T", VC.FRAMES)
def test_select_is_numpy_byte_for_byte_between_guard_bands(mbx, plan, T, form):
    """random records with ties and repeated words; the candidates and the present bytes read-only, guard bands on every side.  With
    d_votes NULL the voted records are the same and not a byte of the vote array is written."""
    rng = np.random.default_rng(300 + 10 * T + len(form))
    rec = VC.random_records(rng, VC.C, T)
    present = VC.present_of(form, rng, T)
    want, want_votes = vote.select(rec, present, VC.OFFSETS, T)
    got, got_votes, _ = _select_between_guards(plan, VC.S, VC.C, T, rec, present, True, seed=T * 8 + len(form))
    assert got.tobytes() == want.tobytes(), np.argwhere(got.view(np.uint32).reshape(want.shape) != want)[:4].tolist()
    assert got_votes.tobytes() == want_votes.tobytes(), (got_votes.view(vote.VOTE_DTYPE), want_votes.reshape(-1))
    got, got_votes, untouched = _select_between_guards(plan, VC.S, VC.C, T, rec, present, False, seed=T * 8 + len(form) + 1)
    assert got.tobytes() == want.tobytes() and got_votes.tobytes() == untouched.tobytes(), "d_votes NULL writes nothing else differently"
    if form == "stream-gone":
        assert (want_votes["winner"][3] == vote.NONE).all() and (want_votes["winner"][[0, 1, 2, 4]] != vote.NONE).all()


def test_select_on_the_crafted_records_of_the_cpu_cases(mbx):
    rec, present, off, rows = VC.crafted_select()
    want, want_votes = vote.select(rec, present, off, 1)
    with vote.Plan(off) as p:
        got, got_votes, _ = _select_between_guards(p, 7, 48, 1, rec, present, True, seed=77)
    assert got.tobytes() == want.tobytes() and got_votes.tobytes() == want_votes.tobytes()
    votes = got_votes.view(vote.VOTE_DTYPE)
    for s, (row, winner, there, best, second, agree) in enumerate(rows):
        assert got.view(np.uint32).reshape(7, 4)[s].tobytes() == rec[row, 0].tobytes(), s
        assert tuple(int(x) for x in votes[s]) == (winner, there, best, second, agree), (s, votes[s])


@pytest.mark.parametrize("form", VC.PRESENT_FORMS)
@pytest.mark.parametrize("cells", vote.ROW_CELLS)
def test_combine_is_numpy_byte_for_byte_between_guard_bands(mbx, plan, cells, form):
    """every row length, T = 1 and 3 (15 x 23 = 345 pieces: two workgroups, the second part-empty); cells and rows at 16 bytes and no better"""
    import torch

    for T in VC.FRAMES:
        rng = np.random.default_rng(500 + cells + T)
        c = VC.random_cells(rng, VC.C, T, cells)
        present = VC.present_of(form, rng, T)
        want, want_votes = vote.combine(c, present, VC.OFFSETS, T)
        for with_votes in (True, False):
            specs = [guarded.buf("cand", c.size, "stage", True), guarded.buf("soft", want.size, "stage"), guarded.buf("votes", 8 * VC.S * T, "rng")]
            if present is not None:
                specs.append(guarded.buf("present", VC.C * T, "frames", True))
            arena = guarded.Arena(specs, where="cuda", seed=cells + T + int(with_votes))
            assert arena.ptr("cand") % 32 == 16 and arena.ptr("soft") % 32 == 16
            arena.load("cand", c)
            if present is not None:
                arena.load("present", present)
            arena.prefill("soft", "votes")
            rc = _L().mbx_vote_combine(plan.handle, cells, T, arena.ptr("cand"), arena.ptr("present") if present is not None else None, arena.ptr("soft"),
                                       arena.ptr("votes") if with_votes else None, _stream())
            assert rc == 0, _L().mbx_last_error()
            torch.cuda.synchronize()
            arena.check(f"combine {cells} cells T {T}")
            got = arena.read("soft")
            assert got.tobytes() == want.tobytes(), (cells, T, np.argwhere(got.reshape(want.shape) != want)[:4].tolist())
            votes = arena.read("votes")
            assert votes.tobytes() == (want_votes.tobytes() if with_votes else arena.prefill_bytes("votes").tobytes())
        assert want[0].tobytes() == np.ascontiguousarray(c[0]).tobytes() or form == "random", "identity ONE on the device's answer too"


def test_the_launchers_refuse_what_needs_a_plan_and_launch_nothing_at_T_0(mbx, plan):
    import torch

    L = _L()
    a = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    base = (a.data_ptr() + 63) & ~63
    out = base + 32768

    def refused(part, rc):
        assert rc == INVALID
        assert part in L.mbx_last_error(), L.mbx_last_error()

    refused(b"T is not negative", L.mbx_vote_select(plan.handle, -1, base, None, out, None, None))
    refused(b"C * T is above 2^31-1", L.mbx_vote_select(plan.handle, (2**31 - 1) // 54 + 1, base, None, out, None, None))
    refused(b"include/mbx_vote.h, Alignment", L.mbx_vote_select(plan.handle, 1, base + 8, None, out, None, None))
    refused(b"include/mbx_vote.h, Alignment", L.mbx_vote_select(plan.handle, 1, base, None, out, out + 1024 + 4, None))
    refused(b"overlaps", L.mbx_vote_select(plan.handle, 1, base, None, base + 16 * 53, None, None))
    refused(b"row_cells is 184, 168 or 96", L.mbx_vote_combine(plan.handle, 72, 1, base, None, out, None, None))
    refused(b"include/mbx_vote.h, Alignment", L.mbx_vote_combine(plan.handle, 96, 1, base + 2, None, out, None, None))
    refused(b"overlaps", L.mbx_vote_combine(plan.handle, 96, 1, base, None, base + 192 * 53, None, None))
    refused(b"codec is one of", L.mbx_process_batch_voted(plan.handle, 9, 1, None, base, None, base, None, base, None, None, None, out, None, None))
    refused(b"mode is MBX_VOTE_SELECT or MBX_VOTE_COMBINE", L.mbx_process_batch_soft_voted(plan.handle, 0, 2, 1, None, base, None, base, None, base, None, None, None, out, None, None))
    refused(b"Alignment", L.mbx_process_batch_soft_voted(plan.handle, 0, 1, 1, None, base + 2, None, base, None, base, None, None, None, out, None, None))
    refused(b"Alignment", L.mbx_process_batch_voted(plan.handle, 0, 1, None, base, None, base, None, base, None, None, None, out + 8, None, None))
    a.fill_(0x5A)
    assert L.mbx_vote_select(plan.handle, 0, base, None, out, out + 4096, None) == 0 and L.mbx_vote_combine(plan.handle, 96, 0, base, None, out, None, None) == 0
    assert L.mbx_process_batch_voted(plan.handle, 0, 0, None, base, None, base, None, base, None, None, None, out, None, None) == 0
    torch.cuda.synchronize()
    assert bool((a == 0x5A).all()), "T = 0 launches nothing"
    assert L.mbx_vote_workspace_frames(plan.handle, 0, vote.SELECT, 3) >= (54 * 3 * 16 + 255) // 256
    assert L.mbx_vote_workspace_frames(plan.handle, 0, vote.COMBINE, 3) >= (5 * 3 * 368 + 255) // 256


# ---- 2. whole steps ---------------------------------------------------------------------------------------------------------------------
_CLEAN = {}


def _clean_frames(codec, T):
    """S x T clean fixture frames of `codec` (framegen's encoders; 7100x4400 through tests/imbe7100_frames.py): made once per shape"""
    if (codec, T) not in _CLEAN:
        rng = framegen.rng_for(0x566F7400 + 16 * codec + T)
        n = VC.S * T
        if codec == 0:
            f = framegen.imbe_clean_voiced_frames(n, rng)
        elif codec == 2:
            import imbe7100_frames
            import oracle_lib

            f = imbe7100_frames.encode_imbe7100x4400(framegen.imbe_voiced_param_bits(n, rng), oracle_lib.load())
        else:
            f = framegen.encode_ambe3600x2450(framegen.ambe_voice_param_bits(n, rng))
        f = f.reshape(VC.S, T, FRAME_BYTES[codec])
        f.setflags(write=False)
        _CLEAN[codec, T] = f
    return _CLEAN[codec, T]


def _candidates(codec, T, soft, tag):
    """the C x T candidates of the five groups: every candidate of stream s a copy of its clean frames with bit flips of its own, at a
    rate of its own between 0 and 6 %"""
    clean = _clean_frames(codec, T)
    rng = framegen.rng_for(0x566F7500 + tag)
    make = vote.noisy_soft_sites if soft else vote.noisy_sites
    parts = []
    for s in range(VC.S):
        n = int(VC.OFFSETS[s + 1] - VC.OFFSETS[s])
        parts.append(make(clean[s], codec, rng.uniform(0.0, 0.06, size=n), rng))
    return np.ascontiguousarray(np.concatenate(parts))


def _front(codec, soft, d_in, n):
    """the existing front call: n frames -> records, as numpy uint32 [n, 4]"""
    import torch

    L = _L()
    rec = torch.zeros((n, 4), dtype=torch.int32, device="cuda")
    if soft:
        rc = L.mbx_fec_soft(codec, d_in.data_ptr(), n, rec.data_ptr(), _stream())
    else:
        fn = {0: L.mbx_fec_imbe7200x4400, 1: L.mbx_fec_ambe3600x2450, 2: L.mbx_fec_imbe7100x4400, 3: L.mbx_fec_ambe3600x2450}[codec]
        rc = fn(d_in.data_ptr(), n, rec.data_ptr(), _stream())
    assert rc == 0, L.mbx_last_error()
    torch.cuda.synchronize()
    return rec.cpu().numpy().view(np.uint32)


class _Pool:
    def __init__(self, slots, resident):
        import torch

        self.state = _dev(init_state(slots))
        self.rng = _dev(rng_seeded(np.arange(slots) * 5 + 31))
        self.resident = torch.zeros(slots, dtype=torch.int32, device="cuda") if resident else None

    def numpy(self):
        return (self.state.cpu().numpy().view(PARMS_DTYPE).reshape(-1, 3), self.rng.cpu().numpy().view(RNG_DTYPE),
                None if self.resident is None else self.resident.cpu().numpy())


class _Out:
    def __init__(self, n):
        import torch

        self.records = torch.full((n, 4), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.pcm16 = torch.full((n, 160), 0x5A5A, dtype=torch.int16, device="cuda")
        self.pcmf = torch.full((n, 160), 7.0, dtype=torch.float32, device="cuda")
        self.results = torch.full((n, 5), 0x5A5A5A5A, dtype=torch.int32, device="cuda")
        self.votes = torch.full((n, 8), 0x5A, dtype=torch.uint8, device="cuda")

    def bytes(self):
        return {k: getattr(self, k).cpu().numpy().tobytes() for k in ("records", "pcm16", "pcmf", "results")}


def _voted_call(plan, codec, form, T, d_index, d_cand, d_present, pool, out, stream=None):
    L = _L()
    tail = (_ptr(d_present), pool.state.data_ptr(), _ptr(pool.resident), pool.rng.data_ptr(), out.pcm16.data_ptr(), out.pcmf.data_ptr(), out.results.data_ptr(),
            out.records.data_ptr(), out.votes.data_ptr(), _stream() if stream is None else stream)
    if form == "hard":
        return L.mbx_process_batch_voted(plan.handle, codec, T, _ptr(d_index), d_cand.data_ptr(), *tail)
    mode = vote.COMBINE if form == "soft-combine" else vote.SELECT
    return L.mbx_process_batch_soft_voted(plan.handle, codec, mode, T, _ptr(d_index), d_cand.data_ptr(), *tail)


def _reference(codec, form, T, cand, present, resident):
    """the existing calls: front over the candidates (or over numpy's combined cells), numpy's select on the host, then
    mbx_process_records -- or mbx_expand_records + mbx_stream_expanded_resident -- on a fresh identity pool of S streams whose slots
    hold what slot INDEX[s] of the voted pool holds.  -> (output bytes, votes, state, rng, resident words, kernel name)"""
    import torch

    L = _L()
    n = VC.S * T
    if form == "soft-combine":
        combined, votes = vote.combine(cand, present, VC.OFFSETS, T)
        chosen = _front(codec, True, _dev(combined), n)
    else:
        rec = _front(codec, form != "hard", _dev(cand), VC.C * T)
        chosen, votes = vote.select(rec.reshape(VC.C, T, 4), present, VC.OFFSETS, T)
    pool = _Pool(POOL, resident)
    pick = torch.from_numpy(INDEX.astype(np.int64)).cuda()
    pool.state = pool.state.view(POOL, -1)[pick].contiguous().view(-1)
    pool.rng = pool.rng.view(POOL, -1)[pick].contiguous().view(-1)
    if resident:
        pool.resident = pool.resident[pick].contiguous()
    out = _Out(n)
    out.records.copy_(torch.from_numpy(np.ascontiguousarray(chosen).reshape(n, 4).view(np.int32)))
    sc = STREAM_CODEC[codec]
    if resident:
        assert L.mbx_expand_records(sc, out.records.data_ptr(), n, _stream()) == 0, L.mbx_last_error()
        rc = L.mbx_stream_expanded_resident(sc, VC.S, T, out.records.data_ptr(), pool.state.data_ptr(), pool.resident.data_ptr(), pool.rng.data_ptr(),
                                            out.pcm16.data_ptr(), out.pcmf.data_ptr(), out.results.data_ptr(), _stream())
    else:
        rc = L.mbx_process_records(sc, VC.S, T, out.records.data_ptr(), pool.state.data_ptr(), pool.rng.data_ptr(), out.pcm16.data_ptr(), out.pcmf.data_ptr(),
                                   out.results.data_ptr(), _stream())
    assert rc == 0, L.mbx_last_error()
    torch.cuda.synchronize()
    name = L.mbx_last_kernel_name(_stream()).decode()
    return (out.bytes(), votes) + pool.numpy() + (name,)


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("codec", [0, 1, 2, 3])
def test_a_voted_step_is_the_front_call_numpy_and_the_records_step_byte_for_byte(mbx, plan, codec, form):
    """PCM, results, records, vote records, state, RNG state and elision words; T = 1 and 3; the present bytes absent, random and all
    zero for one stream; identity and d_stream_index; ABI triplets and resident state.  The candidates stay as they were, and the slots
    of the pool no voted stream names stay as they were."""
    import torch

    L = _L()
    soft = form != "hard"
    for T in VC.FRAMES:
        cand = _candidates(codec, T, soft, tag=32 * codec + 4 * T + FORMS.index(form))
        d_cand = _dev(cand)
        for k, pform in enumerate(VC.PRESENT_FORMS):
            present = VC.present_of(pform, np.random.default_rng(40 + k + T), T)
            d_present = None if present is None else _dev(present)
            for resident in (False, True):
                want, want_votes, want_state, want_rng, want_res, want_name = _reference(codec, form, T, cand, present, resident)
                for indexed in (False, True):
                    what = f"codec {codec} {form} T {T} present {pform} resident {resident} indexed {indexed}"
                    pool = _Pool(POOL, resident)
                    before = pool.numpy()
                    out = _Out(VC.S * T)
                    if not indexed:   # identity: the voted streams' slots are 0 .. S-1; they start as the reference's do
                        pick = torch.from_numpy(INDEX.astype(np.int64)).cuda()
                        pool.state.view(POOL, -1)[:VC.S] = pool.state.view(POOL, -1)[pick]
                        pool.rng.view(POOL, -1)[:VC.S] = pool.rng.view(POOL, -1)[pick]
                        before = pool.numpy()
                    d_index = _dev(INDEX).view(torch.int32) if indexed else None
                    rc = _voted_call(plan, codec, form, T, d_index, d_cand, d_present, pool, out)
                    assert rc == 0, (what, L.mbx_last_error())
                    torch.cuda.synchronize()
                    assert L.mbx_last_kernel_name(_stream()).decode() == want_name, (what, want_name)
                    got = out.bytes()
                    for key in ("records", "results", "pcm16", "pcmf"):
                        assert got[key] == want[key], f"{what}: {key} differs"
                    assert out.votes.cpu().numpy().tobytes() == want_votes.tobytes(), f"{what}: vote records differ"
                    state, rng, res = pool.numpy()
                    slots = INDEX if indexed else np.arange(VC.S)
                    assert state[slots].tobytes() == want_state.tobytes(), f"{what}: state differs"
                    assert rng[slots].tobytes() == want_rng.tobytes(), f"{what}: RNG state differs"
                    rest = np.setdiff1d(np.arange(POOL), slots)
                    assert state[rest].tobytes() == before[0][rest].tobytes() and rng[rest].tobytes() == before[1][rest].tobytes(), f"{what}: a slot no stream names changed"
                    if resident:
                        assert res[slots].tobytes() == want_res.tobytes() and not res[rest].any(), f"{what}: elision words differ"
                    assert d_cand.cpu().numpy().tobytes() == cand.tobytes(), f"{what}: the candidates changed"
        if form != "soft-combine":
            assert (want_votes["winner"] != vote.NONE).any()


def test_the_stream_stage_of_a_voted_step_is_the_records_step_of_its_shape(mbx):
    """more than 256 voted streams at T = 1: the IMBE records step takes the expand launch and its one-frame instance, and so does the
    voted step; the kernel mbx_last_kernel_name reports is the one mbx_process_records leaves there"""
    import torch

    L = _L()
    S = 300
    off = np.arange(S + 1, dtype=np.int32) * 2
    clean = framegen.imbe_clean_voiced_frames(S, framegen.rng_for(0x566F7600))
    cand = np.ascontiguousarray(vote.noisy_sites(clean, 0, (0.01, 0.03), framegen.rng_for(0x566F7601)).transpose(1, 0, 2))   # [S, 2, 18]: candidate rows 2 s, 2 s + 1
    assert L.mbx_uses_expand_launch(0, S, 1) == 1 and L.mbx_uses_expand_launch(0, 5, 1) == 0
    with vote.Plan(off) as p:
        pool, out, d_cand = _Pool(S, False), _Out(S), _dev(cand)
        assert _voted_call(p, 0, "hard", 1, None, d_cand, None, pool, out) == 0, L.mbx_last_error()
        torch.cuda.synchronize()
        voted_name = L.mbx_last_kernel_name(_stream()).decode()
        rec = _front(0, False, _dev(cand), 2 * S)
        chosen, votes = vote.select(rec.reshape(2 * S, 1, 4), None, off, 1)
        ref_pool, ref = _Pool(S, False), _Out(S)
        ref.records.copy_(torch.from_numpy(np.ascontiguousarray(chosen).reshape(S, 4).view(np.int32)))
        assert L.mbx_process_records(0, S, 1, ref.records.data_ptr(), ref_pool.state.data_ptr(), ref_pool.rng.data_ptr(), ref.pcm16.data_ptr(), ref.pcmf.data_ptr(),
                                     ref.results.data_ptr(), _stream()) == 0
        torch.cuda.synchronize()
        assert voted_name == L.mbx_last_kernel_name(_stream()).decode()
        assert out.bytes() == ref.bytes() and out.votes.cpu().numpy().tobytes() == votes.tobytes()
        assert pool.state.cpu().numpy().tobytes() == ref_pool.state.cpu().numpy().tobytes()
        assert len(set(votes["winner"].reshape(-1).tolist())) == 2, "both sites win somewhere"


# ---- 3. the oracle ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("codec", [0, 1], ids=["imbe", "ambe+2"])
def test_a_voted_batch_follows_the_cpu_oracle_on_the_winners_frames(mbx, plan, oracle, codec):
    """the hard voted step, T = 3, all five groups: the records and the results exact, PCM and state under the project's one bound
    (tests/parity.py), against oracle.process_batch on the frames of the winners the vote records name"""
    import torch

    T = 3
    cand = _candidates(codec, T, False, tag=900 + codec)
    pool, out = _Pool(VC.S, False), _Out(VC.S * T)
    seeds = np.arange(VC.S) * 5 + 31
    d_cand = _dev(cand)
    assert _voted_call(plan, codec, "hard", T, None, d_cand, None, pool, out) == 0, _L().mbx_last_error()
    torch.cuda.synchronize()
    votes = out.votes.cpu().numpy().view(vote.VOTE_DTYPE).reshape(VC.S, T)
    assert (votes["winner"] < np.diff(VC.OFFSETS)[:, None]).all() and (votes["present"] == np.diff(VC.OFFSETS)[:, None]).all()
    rows = VC.OFFSETS[:-1, None] + votes["winner"].astype(np.int64)
    winners = cand[rows, np.arange(T)[None, :]]   # [S, T, frame bytes]
    ref = oracle.process_batch(codec, VC.S, T, np.ascontiguousarray(winners).reshape(VC.S * T, -1), oracle.init_state(VC.S), oracle.rng_seeded(seeds))
    parity.check_exact(ref["records"], out.records.cpu().numpy().reshape(-1).view(RECORD_DTYPE), "records", T)
    with parity.located(T):
        parity.check_results(ref["results"], out.results.cpu().numpy().reshape(-1).view(RESULT_DTYPE))
    parity.check_pcm_located(ref["pcmf"], out.pcmf.cpu().numpy(), ref["pcm16"], out.pcm16.cpu().numpy(), T, what="pcm", peak=ref["peak"])
    parity.check_state(ref["state"], pool.numpy()[0], what="state")
    assert (ref["results"]["total_errors"] > 0).any(), "the winners still carry channel errors"


# ---- 4. a graph -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", FORMS)
def test_a_captured_voted_step_replayed_twice_on_fresh_state_gives_the_bytes_of_two_plain_calls(mbx, plan, form):
    """captured after mbx_reserve_stream(stream, mbx_vote_workspace_frames(...)), the default number of hardware queues: two frames
    per stream one after the other, the candidates of the second replay copied into the captured buffer between the replays"""
    import torch

    L = _L()
    codec, T = 0, 1
    soft = form != "hard"
    first, second = (_candidates(codec, T, soft, tag=700 + k) for k in (0, 1))
    plain_pool, plain = _Pool(VC.S, True), []
    for c in (first, second):
        out, d_c = _Out(VC.S * T), _dev(c)
        assert _voted_call(plan, codec, form, T, None, d_c, None, plain_pool, out) == 0, L.mbx_last_error()
        torch.cuda.synchronize()
        plain.append((out.bytes(), out.votes.cpu().numpy().tobytes()))
    side, g = torch.cuda.Stream(), torch.cuda.CUDAGraph()
    mode = vote.COMBINE if form == "soft-combine" else vote.SELECT
    need = L.mbx_vote_workspace_frames(plan.handle, codec, mode, T)
    assert need > 0 and L.mbx_reserve_stream(side.cuda_stream, need) == 0, L.mbx_last_error()
    pool, out, d_cand = _Pool(VC.S, True), _Out(VC.S * T), _dev(first)
    torch.cuda.synchronize()
    with torch.cuda.graph(g, stream=side):
        rc = _voted_call(plan, codec, form, T, None, d_cand, None, pool, out, stream=side.cuda_stream)
    assert rc == 0, L.mbx_last_error()
    for c, want in zip((first, second), plain):
        d_cand.copy_(_dev(c))
        torch.cuda.synchronize()
        g.replay()
        torch.cuda.synchronize()
        assert (out.bytes(), out.votes.cpu().numpy().tobytes()) == want
    assert pool.state.cpu().numpy().tobytes() == plain_pool.state.cpu().numpy().tobytes() and pool.rng.cpu().numpy().tobytes() == plain_pool.rng.cpu().numpy().tobytes()
    assert pool.resident.cpu().numpy().tobytes() == plain_pool.resident.cpu().numpy().tobytes()
    assert L.mbx_release_stream(side.cuda_stream) == 0


# ---- 5. the decoding experiment on the device's FEC ---------------------------------------------------------------------------------------
def test_vote_and_combine_help_decoding_through_the_host_fec_calls(mbx):
    """tests/test_vote_host.py::test_vote_and_combine_against_the_oracle with n(x) through mbx_fec_host / mbx_fec_soft_host, and the
    voted records through mbx_vote_select_host / mbx_vote_combine_host: n(combine) >= n(select) >= n(best single site), the same counts
    as on the CPU oracle (hard sites 157, 150, 161, 158; select 170; combine 200)."""
    L = _L()
    clean, hard, soft = VC.sites()

    def fec(frames, is_soft):
        a = np.ascontiguousarray(frames)
        n = a.shape[0]
        rec = np.zeros((n, 4), dtype=np.uint32)
        rc = L.mbx_fec_soft_host(0, a.ctypes.data, n, rec.ctypes.data) if is_soft else L.mbx_fec_host(0, a.ctypes.data, n, rec.ctypes.data)
        assert rc == 0, L.mbx_last_error()
        return rec

    clean_rec = fec(clean, False)
    off = np.array([0, 4], dtype=np.int32)
    hard_rec = np.stack([fec(h, False) for h in hard])
    n_site = [VC.same_parameters(r, clean_rec) for r in hard_rec]
    voted = np.zeros((200, 4), dtype=np.uint32)
    assert L.mbx_vote_select_host(off.ctypes.data, 1, 200, hard_rec.ctypes.data, None, voted.ctypes.data, None) == 0
    n_select = VC.same_parameters(voted, clean_rec)
    combined = np.zeros((200, 184, 2), dtype=np.uint8)
    assert L.mbx_vote_combine_host(off.ctypes.data, 1, 184, 200, np.ascontiguousarray(soft).ctypes.data, None, combined.ctypes.data, None) == 0
    n_combine = VC.same_parameters(fec(combined, True), clean_rec)
    print(f"hard sites {n_site} select {n_select} combine {n_combine}")
    assert 20 <= 200 - max(n_site) <= 100
    assert n_combine >= n_select >= max(n_site), (n_combine, n_select, n_site)
    assert (n_site, n_select, n_combine) == ([157, 150, 161, 158], 170, 200), "the device's FEC is the oracle's: the counts of the CPU suite"
