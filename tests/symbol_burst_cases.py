"""Burst input in the receiver's forms (include/mbx_burst.h, mbx_burst_schedule_create_form): what the CPU and GPU suites share.
Every form is defined by equivalence to the packed form, which tests/test_gpu_bursts.py holds to the oracle: here are the packed
bursts, their image in a schedule's form (bursts.to_form, with junk in the bits the device does not read), the expectation built
from the PACKED schedule of the same arrays on the packed bursts with the inversion sequence XORed on by the host, the matrix of
mbx_burst_validate, and the memory-contract cases in tests/guarded.py arenas.  Importable without a GPU."""
from collections import namedtuple

import numpy as np

import guarded
import memory_cases
from burst_cases import CELLS, make_bursts
from mbelib_neo_amd import bursts as B
from mbelib_neo_amd.layout import FRAME_BYTES

FORMS = {"packed": B.FORM_PACKED, "bits": B.FORM_BITS, "dibits": B.FORM_DIBITS}
INVALID_ARGUMENT, INVALID_BITS = -1, -2


def random_mask(rng, burst_bits):
    return rng.integers(0, 2, size=burst_bits, dtype=np.uint8)


def one_reliability_per_dibit(soft):
    """per-bit soft bursts [n, burst_bits, 2] whose two bits of a dibit share the reliability of the first (a copy)"""
    out = np.array(soft, dtype=np.uint8)
    even = out.shape[1] & ~1
    out[:, 1:even:2, 1] = out[:, 0:even:2, 1]
    return out


def packed_input(schedule, n, rng, soft):
    """random bursts in the packed form: hard uint8 [n, packed_bytes]; soft uint8 [n, burst_bits, 2] with hard decisions 0 / 1 and
    one reliability per dibit"""
    if soft:
        out = rng.integers(0, 256, size=(n, schedule.burst_bits, 2), dtype=np.uint8)
        out[:, :, 0] &= 1
        return one_reliability_per_dibit(out)
    return rng.integers(0, 256, size=(n, schedule.packed_bytes), dtype=np.uint8)


def scrambled(packed, mask, soft):
    """the packed bursts with the inversion sequence XORed on (None: as they are)"""
    if mask is None:
        return packed
    out = packed.copy()
    if soft:
        out[:, :, 0] ^= mask
    else:
        out ^= np.packbits(np.concatenate([mask, np.zeros(-mask.size % 8, dtype=np.uint8)]))
    return out


def expected(schedule, packed, soft):
    """what a gather of `schedule` must give for bursts that are to_form(schedule, packed): the PACKED schedule of the same arrays,
    without inversion, applied to the packed bursts on which the host has XORed the sequence"""
    return B.apply_schedule(schedule.in_form(B.FORM_PACKED), scrambled(packed, schedule.invert, soft), soft=soft)


def strided(bursts, stride, rng):
    """hard bursts [n, w] -> [n, stride] with random bytes in the padding"""
    out = rng.integers(0, 256, size=(bursts.shape[0], stride), dtype=np.uint8)
    out[:, :bursts.shape[1]] = bursts
    return out


def validate_matrix(L, make):
    """mbx_burst_validate for every form, hard and soft: what is accepted, what is refused, that the padding of the stride is not
    looked at and the last byte / cell that a gather reads is.  make(form) -> a BurstSchedule of codec 1, F = 3, 602 bits."""
    rng = np.random.default_rng(12)
    n = 5
    assert L.mbx_burst_validate(None, b"\0" * 8, 8, 1, 0) == INVALID_ARGUMENT
    for form in FORMS.values():
        s = make(form)
        assert (L.mbx_burst_schedule_form(s.handle), L.mbx_burst_schedule_bytes(s.handle), L.mbx_burst_schedule_soft_cells(s.handle)) == \
            (form, s.burst_bytes, s.soft_cells) == (form, {0: 76, 1: 602, 2: 301}[form], {0: 602, 1: 602, 2: 301}[form])
        assert L.mbx_burst_validate(s.handle, None, s.burst_bytes, n, 0) == INVALID_ARGUMENT
        assert L.mbx_burst_validate(s.handle, None, 0, n, 1) == INVALID_ARGUMENT
        stride = s.burst_bytes + 5
        good = strided(B.to_form(s, packed_input(s, n, rng, False)), stride, rng)   # padding: any bytes
        check = lambda a, soft=0, st=stride: L.mbx_burst_validate(s.handle, a.ctypes.data, st, n, soft)   # noqa: E731
        assert check(good) == 0
        assert check(good, st=s.burst_bytes - 1) == INVALID_ARGUMENT
        most = {B.FORM_PACKED: None, B.FORM_BITS: 1, B.FORM_DIBITS: 3}[form]
        for row, col in ((0, 0), (n - 1, s.burst_bytes - 1), (2, 77)):
            bad = good.copy()
            bad[row, col] = 255 if most is None else most + 1
            assert check(bad) == (0 if most is None else INVALID_BITS), (form, row, col)
            if most is not None:
                bad[row, col] = most
                assert check(bad) == 0
        soft = B.to_form(s, packed_input(s, n, rng, True), soft=True)
        assert soft.shape == (n, s.soft_cells, 2) and check(soft, 1, 0) == 0
        most = 3 if form == B.FORM_DIBITS else 1
        for row, col in ((0, 0), (n - 1, s.soft_cells - 1), (3, 100)):
            bad = soft.copy()
            bad[row, col, 0] = most + 1
            assert check(bad, 1, 0) == INVALID_BITS, (form, row, col)
            bad[row, col] = (most, 255)   # any reliability
            assert check(bad, 1, 0) == 0
        s.close()


# ---- memory-contract cases: the four device entry points with BITS and DIBITS schedules --------------------------------------------
Case = namedtuple("Case", "id covers fn args")
CASES = []


def _case(cid, covers, fn, **args):
    CASES.append(Case(cid, tuple(covers), fn, args))


def _schedule(codec, F, form, masked, seed):
    rng = np.random.default_rng(seed)
    nbits = 602 if form == B.FORM_DIBITS else 601   # 301 dibits: odd, and no multiple of 4
    return B.random_schedule(codec, F, nbits, rng, device=True, form=form, invert=random_mask(rng, nbits) if masked else None)


def gather(codec, form, soft, masked, n=97, F=3):
    """mbx_deinterleave / _soft between guard bands: the bursts read-only at alignment 1 (hard, tight stride: the byte path, and
    the last burst ends where the guard begins) / exactly 2 (soft: the odd-pair head phase), the rows exact, the same bytes under
    two fills of the guards"""
    L, _native, strm = memory_cases._lib()
    s = _schedule(codec, F, form, masked, 300 + 10 * codec + form)
    rng = np.random.default_rng(310 + codec)
    packed = packed_input(s, n, rng, soft)
    bursts = B.to_form(s, packed, soft=soft, junk=rng)
    want = expected(s, packed, soft)
    if soft:
        specs = [guarded.buf("bursts", bursts.size, "soft", True), guarded.buf("rows", n * F * CELLS[codec] * 2, "soft")]
        call = lambda run: _native.check(L.mbx_deinterleave_soft(s.handle, run.p("bursts"), n, run.p("rows"), CELLS[codec], strm), "mbx_deinterleave_soft")   # noqa: E731
    else:
        assert bursts.shape == (n, s.burst_bytes)
        specs = [guarded.buf("bursts", bursts.size, "frames", True), guarded.buf("rows", n * F * FRAME_BYTES[codec], "frames")]
        call = lambda run: _native.check(L.mbx_deinterleave(s.handle, run.p("bursts"), s.burst_bytes, n, run.p("rows"), FRAME_BYTES[codec], strm), "mbx_deinterleave")   # noqa: E731
    got = memory_cases.twice(f"deinterleave codec {codec} form {form} soft {soft}", specs, {"bursts": bursts}, call)
    assert np.array_equal(got["rows"].reshape(want.shape), want)
    s.close()


def launch_buffers(codec, F, S, pool, resident, indexed, rng):
    """(inputs by name, guarded specs without the bursts) of a burst launch"""
    npool = pool if indexed else S
    state0, rng0 = memory_cases._initial(npool, 11)
    specs = [guarded.buf("state", state0.size, "state"), guarded.buf("rng", rng0.size, "rng")] + memory_cases._out_specs(S * F, ("pcm16", "pcmf", "results"))
    inputs = {"state": state0, "rng": rng0}
    if indexed:
        specs.append(guarded.buf("index", 4 * S, "index", True))
        inputs["index"] = rng.permutation(pool)[:S].astype(np.int32)
    if resident:
        specs.append(guarded.buf("resident", 4 * npool, "resident"))
        inputs["resident"] = np.zeros(npool, dtype=np.uint32)
    return inputs, specs


def packed_launch(L, _native, strm, s, S, F, soft, packed, inputs):
    """mbx_process_bursts[_soft] with the packed schedule of the same arrays on the packed bursts, on plain torch allocations:
    (every output and the state as uint8 arrays by name, the stream-stage instance)"""
    import torch

    ps = s.in_form(B.FORM_PACKED, device=True)
    data = scrambled(packed, s.invert, soft)
    dev = {k: torch.from_numpy(np.ascontiguousarray(v).reshape(-1).view(np.uint8).copy()).cuda() for k, v in inputs.items()}
    d_bursts = torch.from_numpy(np.ascontiguousarray(data).reshape(-1).copy()).cuda()
    outs = {k: torch.zeros(S * F * memory_cases.OUT_BYTES[k], dtype=torch.uint8, device="cuda") for k in memory_cases.OUT_ORDER}
    ptr = lambda k: dev[k].data_ptr() if k in dev else None   # noqa: E731
    tail = (dev["state"].data_ptr(), ptr("resident"), dev["rng"].data_ptr(), outs["pcm16"].data_ptr(), outs["pcmf"].data_ptr(), outs["results"].data_ptr(),
            outs["records"].data_ptr(), strm)
    if soft:
        rc = L.mbx_process_bursts_soft(ps.handle, S, ptr("index"), d_bursts.data_ptr(), *tail)
    else:
        rc = L.mbx_process_bursts(ps.handle, S, ptr("index"), d_bursts.data_ptr(), ps.burst_bytes, *tail)
    _native.check(rc, "packed burst launch")
    name = L.mbx_last_kernel_name(strm)
    torch.cuda.synchronize()
    ps.close()
    got = {k: v.cpu().numpy() for k, v in {**outs, **{k: dev[k] for k in ("state", "rng", "resident") if k in dev}}.items()}
    return got, name


def carried_bursts(s, codec, S, F, soft, rng, tag):
    """packed bursts AS RECEIVED that carry the frames of tests/edge_mix.py / soft_mix.py under the schedule: the sequence is on them"""
    import edge_mix
    import soft_mix

    frames = soft_mix.frames(codec, S, F, tag=tag) if soft else edge_mix.frames(codec, S, F, tag).reshape(S * F, -1)
    clear = make_bursts(s.in_form(B.FORM_PACKED), frames, rng, soft=soft)
    if soft:
        clear = one_reliability_per_dibit(clear)
    return scrambled(clear, s.invert, soft)   # (XOR twice is the identity: scrambled(received) is `clear` again)


def launch(codec, form, soft, masked, resident=True, indexed=True, S=97, F=3, pool=120):
    """mbx_process_bursts / _soft with every buffer in the arena, n = 97 bursts at the tight stride; the first run's bytes are those
    of the packed launch on plain allocations"""
    L, _native, strm = memory_cases._lib()
    s = _schedule(codec, F, form, masked, 400 + 10 * codec + form)
    rng = np.random.default_rng(410 + codec)
    received = carried_bursts(s, codec, S, F, soft, rng, tag=F)
    bursts = B.to_form(s, received, soft=soft, junk=rng)
    inputs, specs = launch_buffers(codec, F, S, pool, resident, indexed, rng)
    specs = [guarded.buf("bursts", bursts.size, "soft" if soft else "frames", True)] + specs
    names = []

    def call(run):
        tail = (run.p("state"), run.p("resident"), run.p("rng"), run.p("pcm16"), run.p("pcmf"), run.p("results"), run.p("records"), strm)
        if soft:
            rc = L.mbx_process_bursts_soft(s.handle, S, run.p("index"), run.p("bursts"), *tail)
        else:
            rc = L.mbx_process_bursts(s.handle, S, run.p("index"), run.p("bursts"), s.burst_bytes, *tail)
        _native.check(rc, "mbx_process_bursts")
        names.append(L.mbx_last_kernel_name(strm))

    got = memory_cases.twice(f"bursts codec {codec} form {form} soft {soft}", specs, {**inputs, "bursts": bursts}, call)
    want, name = packed_launch(L, _native, strm, s, S, F, soft, received, inputs)
    assert names == [name, name] and name
    for k, v in want.items():
        assert np.array_equal(got[k], v), f"{k}: the launch from form {form} and the packed launch differ"
    s.close()


for _form_name, _form in (("bits", B.FORM_BITS), ("dibits", B.FORM_DIBITS)):
    for _soft in (False, True):
        _kind = "soft" if _soft else "hard"
        _entry = "_soft" if _soft else ""
        # (a soft per-bit schedule without a sequence is the packed one: its cases carry a sequence)
        _case(f"gather-{_kind}-{_form_name}-1", ["mbx_deinterleave" + _entry], gather, codec=1, form=_form, soft=_soft, masked=_soft and _form == B.FORM_BITS)
        _case(f"gather-{_kind}-{_form_name}-2-masked", ["mbx_deinterleave" + _entry], gather, codec=2, form=_form, soft=_soft, masked=True)
        _case(f"launch-{_kind}-{_form_name}", ["mbx_process_bursts" + _entry], launch, codec=3 if _soft else 0, form=_form, soft=_soft,
              masked=_soft == (_form == B.FORM_BITS))
