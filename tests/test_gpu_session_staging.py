"""GPU suite (-m gpu) for the roads a session's inputs and outputs take between host memory and the slot (mbx_session.hip): pageable
memory through the slot's pinned staging, pinned 16-byte aligned memory in place, pinned memory at an odd offset staged again -- for
the frames, for the keystream rows and for the bursts of a submit and of each group --, the burst buffers of a slot growing, being
reused while large enough, and growing again, and either output into pinned and into pageable memory.  A twin session fed the same
bytes purely from pageable numpy arrays gives the same bytes: two runs of one library, so np.array_equal and no tolerance.
Schedules and inputs: tests/burst_cases.py, keystream_cases.py, burst_group_cases.py.  Nothing here starts a child process."""
import ctypes as C

import numpy as np
import pytest

import burst_cases
import burst_group_cases as G
import keystream_cases as KC

pytestmark = pytest.mark.gpu

S, MAX_FRAMES, OUTPUTS = 5, 10, 1 | 4   # MBX_SESSION_PCM16 | MBX_SESSION_RESULTS; 5 streams: 90 (IMBE) and 45 (AMBE) bytes per tick


@pytest.fixture(scope="module")
def mbx():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    return m


class Pins:
    """mbx_host_alloc memory, freed at the end: put(a, off) is the bytes of `a` at `off` past the allocation's start"""

    def __init__(self, L):
        self.L, self.all = L, []

    def put(self, a, off=0):
        a = np.ascontiguousarray(a)
        p = self.L.mbx_host_alloc(a.nbytes + 16)
        assert p and p % 16 == 0
        self.all.append(p)
        C.memmove(p + off, a.ctypes.data, a.nbytes)
        return p + off

    def out(self, like):
        """a pinned output of the shape of `like`, as a numpy view"""
        p = self.L.mbx_host_alloc(like.nbytes)
        assert p
        self.all.append(p)
        a = np.ctypeslib.as_array((C.c_uint8 * like.nbytes).from_address(p)).view(like.dtype).reshape(like.shape)
        a.view(np.uint8).fill(0x5A)
        return a

    def free(self):
        for p in self.all:
            self.L.mbx_host_free(p)


def _state(L, h, n):
    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import PARMS_DTYPE, RNG_DTYPE

    st, rg = np.zeros((n, 3), PARMS_DTYPE), np.zeros(n, RNG_DTYPE)
    _native.check(L.mbx_session_get_state(h, 0, n, st.ctypes.data, rg.ctypes.data), "get_state")
    return st.tobytes() + rg.tobytes()


def _outputs(nf):
    from mbelib_neo_amd.layout import RESULT_DTYPE

    return np.full((nf, 160), 0x5A5A, np.int16), np.zeros(nf, RESULT_DTYPE)


# what each of the seven submits is: slot 0 of the three takes submits 0, 3 and 6, the burst submits
#   (kind, T, where the frames / bursts are, where the keystream rows are, extra bytes of burst_stride)
# where: None pageable, else the offset into mbx_host_alloc memory
SUBMITS = (("bursts", 2, None, None, 8),     # the slot's burst buffers, device and pinned staging, are made
           ("frames", 2, 0, None, 0),        # frames pinned and aligned: read in place
           ("keyed", 1, None, None, 0),      # frames pageable, rows pageable
           ("bursts", 2, 0, None, 0),        # a smaller burst submit on slot 0, read in place: both buffers stay
           ("keyed", 2, 2, 0, 0),            # frames pinned at +2: staged; rows pinned and aligned
           ("keyed", 1, 0, 4, 0),            # rows pinned at +4: staged
           ("bursts", 2, 1, None, 40))       # a larger one on slot 0, pinned at +1: staged, both buffers grow again


@pytest.mark.parametrize("codec", [0, 1], ids=["imbe7200x4400", "ambe3600x2450"])
def test_every_road_into_and_out_of_a_slot_gives_the_bytes_of_the_pageable_road(mbx, codec):
    from mbelib_neo_amd import _native, bursts as B

    L = _native.lib()
    rng = np.random.default_rng(900 + codec)
    sched = B.random_schedule(codec, 2, 2 * B.channel_bits(codec) + 57, rng, device=True)
    seeds = (np.arange(S) * 7 + 3).astype(np.uint32)
    a, b = C.c_void_p(), C.c_void_p()
    pins = Pins(L)
    try:
        for h in (a, b):
            _native.check(L.mbx_session_create(C.byref(h), codec, S, MAX_FRAMES, OUTPUTS), "create")
            _native.check(L.mbx_session_seed(h, 0, S, seeds.ctypes.data), "seed")
        got, want, keep = [], [], []
        for step, (kind, T, where, rows_where, pad) in enumerate(SUBMITS):
            frames = np.ascontiguousarray(KC.any_frames(codec, S, T, tag=60 + step)).reshape(-1)
            stride = sched.burst_bytes + pad
            data = burst_cases.make_bursts(sched, frames, rng, burst_stride=stride).reshape(-1) if kind == "bursts" else frames
            rows = KC.random_rows(S * T, rng) if kind == "keyed" else None
            keep += [data, rows]
            # pcm16 into pinned memory and results into pageable memory, then the other way round
            o16, ores = _outputs(S * T)
            oa = (pins.out(o16), ores) if step % 2 == 0 else (o16, pins.out(ores))
            ob = _outputs(S * T)
            for h, out, paged in ((a, oa, False), (b, ob, True)):
                src = data.ctypes.data if paged or where is None else pins.put(data, where)
                p16, pres = out[0].ctypes.data, out[1].ctypes.data
                if kind == "bursts":
                    rc = L.mbx_session_submit_bursts(h, sched.handle, S, None, src, stride, p16, None, pres)
                elif kind == "keyed":
                    key = rows.ctypes.data if paged or rows_where is None else pins.put(rows, rows_where)
                    rc = L.mbx_session_submit_keyed(h, S, T, None, src, None, key, p16, None, pres, None)
                else:
                    rc = L.mbx_session_submit(h, T, src, p16, None, pres)
                _native.check(rc, f"submit {step} ({kind})")
            got.append(oa)
            want.append(ob)
        # (no wait in between: the fourth and the seventh submit finish the batch their slot held and hand its staged outputs over)
        _native.check(L.mbx_session_wait(a), "wait")
        _native.check(L.mbx_session_wait(b), "wait")
        for step, (x, y) in enumerate(zip(got, want)):
            for u, v, k in zip(x, y, ("pcm16", "results")):
                assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), f"submit {step} {SUBMITS[step]}: {k}"
        assert any(w[0].any() for w in want), "the twin decoded nothing but silence"
        assert _state(L, a, S) == _state(L, b, S)
    finally:
        for h in (a, b):
            L.mbx_session_destroy(h)
        pins.free()
        sched.close()


def test_groups_from_pinned_memory_aligned_and_not_give_the_bytes_of_pageable_groups(mbx):
    from mbelib_neo_amd import _native

    L = _native.lib()
    streams = 8
    shapes = ((1, 3, 2, True, 3, 2, 0), (1, 1, 0, False, 4, 1, 2))   # two schedules of ONE codec: 3 streams x 2 bursts of 3 frames, 4 x 1 of 1
    total = 3 * 2 * 3 + 4
    scheds = G.schedules(shapes, 51)
    perm = np.random.default_rng(6).permutation(streams).astype(np.int32)
    groups = G.make_groups(shapes, scheds, False, 53, tag=5, slots=[perm[:3], perm[3:7]])
    a, b = C.c_void_p(), C.c_void_p()
    pins = Pins(L)
    try:
        outs = []
        for h, paged in ((a, False), (b, True)):
            _native.check(L.mbx_session_create(C.byref(h), 1, streams, total, OUTPUTS), "create")
            arr, keep = G.group_array(L, groups)
            if not paged:   # one group pinned and 16-byte aligned, one pinned at +1
                for i, g in enumerate(groups):
                    arr[i].bursts = pins.put(g.bursts, i)
            o = _outputs(total)
            _native.check(L.mbx_session_submit_burst_groups(h, arr, 2, 0, o[0].ctypes.data, None, o[1].ctypes.data), "submit_burst_groups")
            _native.check(L.mbx_session_wait(h), "wait")
            outs.append(o)
        for u, v, k in zip(outs[0], outs[1], ("pcm16", "results")):
            assert np.array_equal(u.view(np.uint8), v.view(np.uint8)), k
        assert outs[1][0].any() and _state(L, a, streams) == _state(L, b, streams)
    finally:
        for h in (a, b):
            L.mbx_session_destroy(h)
        pins.free()
        for s in scheds:
            s.close()
