"""One oracle case per row of kInstances (mbelib-neo_amd/csrc/mbx_api.hip): every stream-stage kernel instance is run BY NAME --
after each launch mbx_last_kernel_name must report the case's instance -- on the edge mix of its codec (tests/edge_mix.py) and
held to the oracle on every stream: records, results and RNG state exact, PCM under the int16 bound of each frame's pre-clip
peak, state in tolerance.  Shapes sit on the edges: S not a multiple of 8 or 64, 257 and 256 around the small-batch limit, T = 2, 3,
4 (the LDS threshold) and 17 (AMBE expands eight frames at a time: two blocks and one), slices of 16, 16 and 8 frames over groups
that do not divide S, more chunks than the front blocks' lead, an index into a larger pool; several launches on continuing state,
so both walking directions and the hand-over of the state are under the oracle.

Importable without a GPU (tests/test_host_logic.py holds CASES to the table).  Cases without switches run inside the GPU suite's
process when its environment holds no MBX_* switch; a case with environment switches -- the library reads them once per process --
and every case of a suite that itself runs under switches runs as `python tests/instance_cases.py <id>` in a fresh child with
exactly the case's switches: exit status 0 = passed, 1 = a mismatch (printed).  `python tests/instance_cases.py <id> --guarded`
(tests/test_gpu_memory_contract.py): the same case twice with every buffer in a guarded arena (run_guarded)."""
import os
import sys
from collections import namedtuple

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

# entry: batch = mbx_process_batch; batch_ws = mbx_process_batch_ws (caller workspace); batch_indexed = mbx_process_batch_indexed
# (the batch's streams are every second slot, backwards, of a pool of 2 S + 3); resident = mbx_process_batch_resident; resident_indexed
# = the same through that index; staged = mbx_fec_* + mbx_process_records
Case = namedtuple("Case", "id name codec S T launches entry env")


def _c(name, codec, S, T, launches, entry, env=None, tag=""):
    return Case(name + ("-" + tag if tag else ""), name, codec, S, T, launches, entry, dict(env or {}))


CASES = [
    # T = 2, 3: the plain looped instances (state in its HBM slots every frame)
    _c("imbe_stream_kernel", 0, 1003, 3, 2, "batch"),
    _c("ambe_stream_kernel", 1, 1001, 2, 3, "batch"),
    _c("ambe2400_stream_kernel", 3, 517, 3, 2, "batch_indexed"),
    _c("imbe_stream_kernel", 2, 300, 2, 3, "batch", tag="imbe7100"),
    # T = 1 behind the FEC (and expansion) launches: the staged calls, a small batch, a caller workspace
    _c("imbe_stream_kernel_one", 0, 257, 1, 6, "staged"),
    _c("imbe_stream_kernel_one", 0, 256, 1, 6, "batch", tag="small"),
    _c("ambe_stream_kernel_one", 1, 1003, 1, 6, "batch_ws"),
    _c("ambe2400_stream_kernel_one", 3, 257, 1, 6, "staged"),
    # T >= 4: prev_mp / prev_mp_enhanced stay in LDS for the launch
    _c("imbe_stream_kernel_lds", 0, 2051, 4, 2, "batch"),
    _c("ambe_stream_kernel_lds", 1, 1001, 17, 2, "batch"),
    _c("ambe2400_stream_kernel_lds", 3, 1003, 17, 2, "batch_indexed"),
    # resident state, several frames and one
    _c("imbe_stream_kernel_res", 0, 1001, 3, 2, "resident"),
    _c("ambe_stream_kernel_res", 1, 1003, 17, 2, "resident_indexed"),
    _c("ambe2400_stream_kernel_res", 3, 517, 4, 2, "resident"),
    _c("imbe_stream_kernel_res1", 0, 256, 1, 6, "resident"),
    _c("ambe_stream_kernel_res1", 1, 1003, 1, 6, "resident", env={"MBX_FUSE_ONE": "0"}),
    _c("ambe2400_stream_kernel_res1", 3, 203, 1, 6, "resident_indexed"),
    # sliced launches: three groups of streams that do not divide S.  Two cases with the slice length set by switch, T = 40 = slices
    # of 16, 16 and a tail of 8; one sliced by the launcher's OWN rule, which needs more streams than the device has wave slots for
    # the kernel -- 5,125 on the 5,120 of a whole MI355X (256 CUs x 4 SIMDs x 5 waves; on a partitioned device the launch would not be
    # sliced and the name assertion says so) -- and T >= 32: T = 32 (16 + 16) keeps that case at 328,000 frames
    _c("imbe_stream_kernel_lds_slice", 0, 1000, 40, 2, "batch", env={"MBX_SLICE": "16"}),
    _c("ambe_stream_kernel_lds_slice", 1, 5125, 32, 2, "batch"),
    _c("ambe2400_stream_kernel_lds_slice", 3, 1001, 40, 2, "batch", env={"MBX_SLICE": "16"}),
    # the T = 1 step as ONE launch: front blocks and stream blocks in one grid (S = 257: the last chunk of eight holds one stream)
    _c("imbe_one_launch_kernel", 0, 257, 1, 6, "batch"),
    _c("imbe_one_launch_kernel", 0, 1003, 1, 6, "batch_indexed", env={"MBX_FRONT_LEAD": "64"}, tag="lead64"),   # 126 chunks, lead 64
    _c("ambe_one_launch_kernel", 1, 4099, 1, 6, "batch"),
    _c("ambe2400_one_launch_kernel", 3, 257, 1, 6, "batch"),
    _c("imbe_one_launch_kernel_res", 0, 4099, 1, 6, "resident"),
    _c("ambe_one_launch_kernel_res", 1, 257, 1, 6, "resident"),
    _c("ambe2400_one_launch_kernel_res", 3, 1003, 1, 6, "resident_indexed"),
    # ... and with the front end in the stream's own wave
    _c("imbe_stream_kernel_one_fused", 0, 1003, 1, 6, "batch_ws"),
    _c("imbe_stream_kernel_one_fused", 0, 257, 1, 6, "batch", env={"MBX_FUSE_ONE": "1"}, tag="switch"),
    _c("imbe7100_stream_kernel_one_fused", 2, 1003, 1, 6, "batch"),
    _c("imbe_stream_kernel_res1_fused", 0, 1003, 1, 6, "resident", env={"MBX_FUSE_ONE": "1"}),
    _c("imbe7100_stream_kernel_res1_fused", 2, 257, 1, 6, "resident_indexed"),
]
BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def child_timeout(case):
    """seconds a fresh process may take for a case: start-up of the runtime plus its frames at a cautious rate"""
    return 180 + case.S * case.T * case.launches // 2000


class PlainBuffers:
    """the buffers of a case as torch allocates them (what the instance tests have always run on)"""

    trace = None
    OUTPUTS = ("records", "results", "pcm16", "pcmf")

    def layout(self, specs):
        import torch

        self.bufs = {s.name: torch.empty(s.nbytes, dtype=torch.uint8, device="cuda") for s in specs}
        return self.bufs

    def load(self, name, bufs, data):
        import torch

        bufs[name].copy_(torch.from_numpy(np.ascontiguousarray(data).reshape(-1).view(np.uint8)))

    def before_launch(self):
        for n in self.OUTPUTS:   # (the outputs are reused from launch to launch: a row a launch leaves unwritten must not hold the last launch's)
            self.bufs[n].fill_(0xA5)

    def after_launch(self, what):
        pass

    def note(self, label, data):
        pass


class GuardedBuffers(PlainBuffers):
    """the same buffers in ONE guarded arena (tests/guarded.py): each at exactly the alignment of its kind, exact size, guard bands on
    both sides, outputs pre-filled with the arena's pattern before every launch, guards and read-only inputs checked after every
    launch; `trace` keeps the bytes of every output of every launch and of the final state for the two-run comparison"""

    def __init__(self, seed):
        self.seed, self.trace, self.arena = seed, [], None

    def layout(self, specs):
        import guarded

        self.arena = guarded.Arena(specs, where="cuda", seed=self.seed)
        return {s.name: self.arena.view(s.name) for s in specs}

    def load(self, name, bufs, data):
        self.arena.load(name, data)

    def before_launch(self):
        self.arena.prefill(*[n for n in self.OUTPUTS if n in self.arena.by_name])

    def after_launch(self, what):
        self.arena.check(what)

    def note(self, label, data):
        self.trace.append((label, np.ascontiguousarray(data).reshape(-1).view(np.uint8).copy()))


def compare_traces(first, second, what):
    """two runs of one case from the same inputs, under different guard and pre-fill patterns: byte-identical outputs of every launch,
    state, RNG state and elision words -- every output byte was written, and nothing outside the inputs was read into a result"""
    assert [a for a, _ in first] == [a for a, _ in second], what
    for (label, a), (_, b) in zip(first, second):
        assert a.size == b.size, (what, label)
        bad = np.flatnonzero(a != b)
        assert bad.size == 0, (f"{what}: {label} differs between two runs that differ only in the pre-fill of the outputs and in the guard bytes: "
                               f"{bad.size} byte(s), first at offset {int(bad[0])}, last at offset {int(bad[-1])} of {a.size}")


class EdgeMixWorkload:
    """the workload of every case of CASES: the edge mix of the case's codec (tests/edge_mix.py), decoded by the oracle for the case.
    Another workload (tests/pitch_lattice.py) brings the same five things: the frames [S, T x launches, bytes], the oracle's decode of
    them from the initial state under the case's seeds, the assertion of what the decode must hold, a context manager that may
    say more about the streams a failed comparison names, and a report of figures that asserts nothing."""

    def frames(self, case):
        import edge_mix

        return edge_mix.frames(case.codec, case.S, case.T * case.launches, tag=sum(case.id.encode()) & 0xFFF)

    def reference(self, case, frames, seeds):
        import oracle_lib

        o = oracle_lib.load()
        Tt = case.T * case.launches
        return o.process_batch(case.codec, case.S, Tt, frames.reshape(case.S * Tt, -1), o.init_state(case.S), o.rng_seeded(seeds))

    def assert_classes(self, codec, ref):
        import edge_mix

        edge_mix.assert_classes(codec, ref)

    state_block = None   # streams per block of parity.check_state_blocks; None: parity.check_state over all streams at once

    def naming(self, case):
        import contextlib

        return contextlib.nullcontext()

    def report(self, case, ref, got):
        """figures a workload wants of the run (got: records, results, pcm16, pcmf as [S, T x launches, ...]), taken before anything is asserted"""

    # optional: checkpoint(case, launch, state) -- called behind every launch with the state [S, 3] of the case's slots as that launch
    # left it (slot_state); the workloads here do not define it (tests/error_lattice.py does)


def slot_state(dec, slots):
    """the state [S, 3] of the given slots as the last launch left it, taken from a COPY of the pool: for a resident decoder the copy is
    materialised (mbx_resident_materialize on the copied structs and elision words), the decoder's own buffers stay as the launch left
    them, elided structs and all"""
    import torch

    from mbelib_neo_amd import _native
    from mbelib_neo_amd.layout import PARMS_DTYPE

    state = dec.state.clone()
    if dec.resident is not None:
        words = dec.resident.clone()
        _native.check(_native.lib().mbx_resident_materialize(dec.streams, None, state.data_ptr(), words.data_ptr(), torch.cuda.current_stream().cuda_stream),
                      "mbx_resident_materialize")
    return state.cpu().numpy().view(PARMS_DTYPE).reshape(dec.streams, 3)[slots]


def run_case(case, mem=None, oracle=True, workload=None):
    """Runs the case on the current device and compares with the oracle; raises AssertionError on the first mismatch.  The process's
    environment must already hold case.env (the library reads its switches once).
    workload: the frames of the case and what the oracle's decode of them must hold (EdgeMixWorkload by default); the launches, the
    buffers, the name assertions and every comparison are the same for any workload.  A workload with a `checkpoint` method is also
    called behind every launch, with the launch index and the state of the case's slots (slot_state).
    mem: where the buffers of the case live (PlainBuffers by default; GuardedBuffers: every buffer the launches are handed -- frames,
    records, state pool, RNG pool, elision words, index, PCM, results, caller workspace -- in one guarded arena, checked after every
    launch).  oracle=False: the launches and the checks of `mem` only (the second of two runs, compared with the first by trace)."""
    import torch

    import parity
    from mbelib_neo_amd import _native, decoder
    from mbelib_neo_amd.layout import FRAME_BYTES, RECORD_DTYPE, RESULT_DTYPE

    for k, v in case.env.items():
        assert os.environ.get(k) == v, f"{case.id}: needs {k}={v} in the environment of a fresh process"
    codec, S, T, n_launch = case.codec, case.S, case.T, case.launches
    fb, Tt = FRAME_BYTES[codec], case.T * case.launches
    workload = workload if workload is not None else EdgeMixWorkload()
    frames = workload.frames(case)
    assert frames.shape == (S, Tt, fb) and frames.dtype == np.uint8, (case.id, frames.shape)
    seeds = np.arange(S) * 3 + 11
    indexed = case.entry.endswith("_indexed")
    resident = case.entry.startswith("resident")
    pool = 2 * S + 3 if indexed else S
    slots = np.arange(pool - 2, 0, -2)[:S] if indexed else np.arange(S)   # every second slot of the pool, walked backwards
    assert len(slots) == S and len(set(slots.tolist())) == S
    pool_seeds = np.full(pool, 999, dtype=np.int64)
    pool_seeds[slots] = seeds
    import guarded

    mem = mem if mem is not None else PlainBuffers()
    L = _native.lib()
    dec = decoder.BatchDecoder(codec, pool, seeds=pool_seeds, resident=resident)
    untouched_state, untouched_rng = dec.state_numpy().copy(), dec.rng_numpy().copy()
    strm = torch.cuda.current_stream().cuda_stream
    n = S * T
    # (IMBE frames are read in 16-bit pieces, and the one-launch and fused instances are selected only for frames on a 4-byte
    # boundary: exactly that, no better; AMBE frames are read byte by byte and sit on an odd address)
    specs = [guarded.buf("frames", n * fb, guarded.frames_kind(codec, one_frame=T == 1), readonly=True), guarded.buf("records", n * 16, "records"),
             guarded.buf("state", dec.state.numel(), "state"), guarded.buf("rng", dec.rng.numel(), "rng"),
             guarded.buf("pcm16", n * 320, "pcm16"), guarded.buf("pcmf", n * 640, "pcmf"), guarded.buf("results", n * 20, "results")]
    if resident:
        specs.append(guarded.buf("resident", pool * 4, "resident"))
    if indexed:
        specs.append(guarded.buf("index", S * 4, "index", readonly=True))
    if case.entry == "batch_ws":
        specs.append(guarded.buf("workspace", int(L.mbx_workspace_bytes(n)), "workspace"))   # EXACTLY the documented need
    bufs = mem.layout(specs)
    bufs["state"].copy_(dec.state)
    bufs["rng"].copy_(dec.rng)
    dec.state, dec.rng = bufs["state"], bufs["rng"]   # (plain tensor attributes: every launch and state_numpy() go through them)
    if resident:
        bufs["resident"].copy_(dec.resident.view(torch.uint8))
        dec.resident = bufs["resident"].view(torch.int32)
    if indexed:
        mem.load("index", bufs, slots.astype(np.int32))
    d_index = bufs["index"] if indexed else None
    ws = bufs.get("workspace")
    out = {"records": bufs["records"].view(torch.int32).view(n, 4), "results": bufs["results"].view(torch.int32).view(n, 5),
           "pcm16": bufs["pcm16"].view(torch.int16).view(n, 160), "pcmf": bufs["pcmf"].view(torch.float32).view(n, 160)}
    got = {k: [] for k in ("records", "results", "pcm16", "pcmf")}
    for k in range(n_launch):
        part = np.ascontiguousarray(frames[:, k * T:(k + 1) * T])
        mem.load("frames", bufs, part)
        d_frames = bufs["frames"]
        mem.before_launch()
        if case.entry in ("batch", "staged") or (case.entry == "resident"):
            dec.decode(d_frames, T, want_float=True, staged=case.entry == "staged", out=out)
        else:
            o = [out[x].data_ptr() for x in ("pcm16", "pcmf", "results", "records")]
            if case.entry == "batch_ws":
                rc = L.mbx_process_batch_ws(codec, S, T, d_frames.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), *o, ws.data_ptr(), ws.numel(), strm)
            elif case.entry == "batch_indexed":
                rc = L.mbx_process_batch_indexed(codec, S, T, d_index.data_ptr(), d_frames.data_ptr(), dec.state.data_ptr(), dec.rng.data_ptr(), *o, strm)
            else:
                assert case.entry == "resident_indexed", case.entry
                rc = L.mbx_process_batch_resident(codec, S, T, d_index.data_ptr(), d_frames.data_ptr(), dec.state.data_ptr(), dec.resident.data_ptr(),
                                                  dec.rng.data_ptr(), *o, strm)
            _native.check(rc, case.entry)
        ran = L.mbx_last_kernel_name(strm)
        assert ran is not None and ran.decode() == case.name, f"{case.id}: launch {k} ran {ran!r}, the case is for {case.name}"
        if case.entry in ("batch", "batch_indexed", "resident", "resident_indexed"):   # (the calls the prediction is made for: same plan, same name)
            predicted = L.mbx_batch_kernel_name(codec, S, T, 1 if resident else 0)
            assert predicted == ran, f"{case.id}: launch {k} ran {ran!r}, mbx_batch_kernel_name predicts {predicted!r}"
        torch.cuda.synchronize()
        mem.after_launch(f"{case.id}: launch {k}")
        for x in got:
            got[x].append(out[x].cpu().numpy().reshape(S, T, -1))
            mem.note(f"launch {k}: {x}", got[x][-1])
        if oracle and hasattr(workload, "checkpoint"):
            workload.checkpoint(case, k, slot_state(dec, slots))
    if mem.trace is not None:   # the state as the launches left it, elision words and all, before anything materialises it
        mem.note("state as left", dec.state.cpu().numpy())
        if resident:
            mem.note("elision words", dec.resident.cpu().numpy())
    got = {x: np.concatenate(v, axis=1) for x, v in got.items()}   # [S, Tt, ...]
    state, rng = dec.state_numpy(), dec.rng_numpy()   # (resident: mbx_resident_materialize on the same buffers)
    torch.cuda.synchronize()
    mem.after_launch(f"{case.id}: materialize")
    mem.note("state", state)
    mem.note("rng", rng)
    if not oracle:
        return None

    ref = workload.reference(case, frames, seeds)
    workload.assert_classes(codec, ref)
    what = case.id
    with workload.naming(case):
        workload.report(case, ref, got)
        parity.check_exact(ref["records"], np.ascontiguousarray(got["records"]).view(RECORD_DTYPE).reshape(-1), what + ": records", Tt)
        with parity.located(Tt):
            parity.check_results(ref["results"], np.ascontiguousarray(got["results"]).view(RESULT_DTYPE).reshape(-1), what + ": results")
            m = parity.check_pcm(ref["pcmf"], got["pcmf"].reshape(-1, 160), ref["pcm16"], got["pcm16"].reshape(-1, 160), what=what + ": pcm", peak=ref["peak"])
        if workload.state_block:   # (the same fields under the same bound, block by block)
            parity.check_state_blocks(ref["state"], state[slots], block=workload.state_block, what=what + ": state (rows are streams)")
        else:
            parity.check_state(ref["state"], state[slots], what=what + ": state (rows are streams)")
        parity.check_exact(ref["rng"], rng[slots], what + ": rng")
    if indexed:   # the slots of the pool the index does not name are as they were
        rest = np.setdiff1d(np.arange(pool), slots)
        assert state[rest].tobytes() == untouched_state[rest].tobytes() and rng[rest].tobytes() == untouched_rng[rest].tobytes(), what + ": a slot outside the index changed"
    return m


def run_guarded(case):
    """the case twice from the same inputs, every buffer in a guarded arena (GuardedBuffers), under two patterns: the first run against
    the oracle as run_case always does, the second against the first run's bytes"""
    import torch

    first = GuardedBuffers(seed=1)
    m = run_case(case, mem=first)
    first.arena = None
    torch.cuda.empty_cache()
    second = GuardedBuffers(seed=2)
    run_case(case, mem=second, oracle=False)
    compare_traces(first.trace, second.trace, case.id)
    return m


def main():
    case = BY_ID[sys.argv[1]]
    guarded_run = len(sys.argv) > 2 and sys.argv[2] == "--guarded"
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)
    try:
        m = run_guarded(case) if guarded_run else run_case(case)
    except AssertionError as e:
        print(f"MISMATCH {case.id}: {e}")
        return 1
    print(f"ok {case.id}: {m}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
