"""The memory-contract cases of the launch forms outside the kernel-instance table (tests/test_gpu_memory_contract.py): every buffer of
a call in ONE guarded arena (tests/guarded.py) -- exact size, exactly the alignment of its kind, guard bands on both sides, outputs
pre-filled with the arena's pattern -- the call run TWICE from the same inputs under two patterns.  After each run the guards and the
read-only inputs must be intact; between the runs every output, the state, the RNG state and the elision words must be byte-identical
(every output byte was written, nothing outside the inputs was read into a result); and rows the header says a launch leaves alone
still hold the pre-fill.  Values are held to the oracle elsewhere (the parity suites, on torch's own buffers); here the first run is
additionally compared, byte for byte, with the same call on plain torch allocations where a case says so.

Importable without a GPU: CASES names, per case, the entry points of include/mbx.h it puts under guard
(tests/test_memory_contract_host.py requires every exported function with a device pointer, and every *_host call, to be named here,
by an instance case or by the exemption table)."""
import os
import sys
from collections import namedtuple

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
for d in (HERE, os.path.dirname(HERE)):
    if d not in sys.path:
        sys.path.insert(0, d)

import guarded  # noqa: E402

Case = namedtuple("Case", "id covers fn args")
CASES = []


def _case(cid, covers, fn, **args):
    CASES.append(Case(cid, tuple(covers), fn, args))


FB = {0: 18, 1: 9, 2: 18, 3: 9}
CELLS = {0: 184, 1: 96, 2: 168, 3: 96}
OUT_BYTES = {"records": 16, "results": 20, "pcm16": 320, "pcmf": 640}
OUT_ORDER = ("pcm16", "pcmf", "results", "records")


def _initial(pool, seed0):
    from mbelib_neo_amd.layout import init_state, rng_seeded

    return init_state(pool).view(np.uint8).reshape(-1), rng_seeded(np.arange(pool) * 7 + seed0).view(np.uint8).reshape(-1)


class Run:
    """one guarded arena per run; call(run) issues the launches; `scratch` buffers (workspaces) are guarded but not compared"""

    def __init__(self, specs, seed, scratch=(), where="cuda"):
        self.arena = guarded.Arena(specs, where=where, seed=seed)
        self.scratch = set(scratch)

    def p(self, name):
        return self.arena.ptr(name) if name in self.arena.by_name else None

    def finish(self, what):
        import torch

        torch.cuda.synchronize()
        self.arena.check(what)
        return {s.name: self.arena.read(s.name) for s in self.arena.slots if not s.readonly and s.name not in self.scratch}


def twice(what, specs, inputs, call, scratch=(), after=None, where="cuda", compare=True):
    """the call under two patterns; returns the first run's buffers (name -> uint8 array).  after(run, got): further assertions that
    need the arena (rows left alone).  where="numpy": the buffers are HOST memory (the *_host calls).  compare=False: a call that must
    write nothing -- the payloads then legitimately differ between the runs (they hold the pre-fill)"""
    import torch

    results = []
    for seed in (1, 2):
        run = Run(specs, seed, scratch, where)
        for name, data in inputs.items():
            run.arena.load(name, data)
        call(run)
        got = run.finish(f"{what} (pattern {seed})")
        if after:
            after(run, got)
        results.append(got)
        del run
        torch.cuda.empty_cache()
    a, b = results
    for name in a if compare else ():
        bad = np.flatnonzero(a[name] != b[name])
        assert bad.size == 0, (f"{what}: {name} differs between two runs that differ only in the pre-fill of the outputs and in the guard bytes: "
                               f"{bad.size} byte(s), first at offset {int(bad[0])}, last at offset {int(bad[-1])} of {a[name].size}")
    return a


def _lib():
    import torch

    from mbelib_neo_amd import _native, decoder

    decoder.ensure_init(0)
    return _native.lib(), _native, torch.cuda.current_stream().cuda_stream


def _out_specs(n, want):
    return [guarded.buf(k, n * OUT_BYTES[k], k) for k in ("records", "results", "pcm16", "pcmf") if k == "records" or k in want]


# ---- ragged and mixed batches ----------------------------------------------------------------------------------------------------
# streams without frames first, in the middle and last; total_frames odd and not a multiple of 8
RAGGED_COUNTS = np.array([0, 3, 1, 0, 0, 5, 2, 1, 4, 0, 1, 3, 2, 0, 7, 1, 1, 2, 0, 3, 1, 0], dtype=np.int64)
assert RAGGED_COUNTS.sum() % 2 == 1 and RAGGED_COUNTS.sum() % 8 != 0


def ragged(codec, soft, resident, indexed, mixed, want=("pcm16", "pcmf", "results")):
    import mixed_case
    import ragged_case

    L, _native, strm = _lib()
    counts = np.tile(RAGGED_COUNTS, 3)[:65]   # 65 streams: one more than a wave's lanes, one more than the 64 of an order word's frame
    counts[-1] = 0
    counts[-2] += 1
    S, total = len(counts), int(counts.sum())
    assert total % 2 == 1 and total % 8 != 0
    pool = 2 * S + 3 if indexed else S
    slots = np.arange(pool - 2, 0, -2)[:S] if indexed else np.arange(S)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    codecs = None
    if mixed:
        codecs = mixed_case.codecs_for(S, 5)
        codecs[7] = 200   # no MBX_CODEC_* value: its stream is a stream without frames, its rows keep their bytes
        assert counts[7] > 0
        good = np.where(codecs < 4, codecs, 0).astype(np.uint8)
        rows, _ = mixed_case.mixed_frames(good, counts, tag=9, soft=soft)
    else:
        rows = ragged_case.ragged_frames(codec, counts, tag=9, soft=soft)
    rows = np.ascontiguousarray(rows).reshape(-1)
    state, rng = _initial(pool, 3)
    specs = [guarded.buf("offsets", 4 * (S + 1), "index", True), guarded.buf("frames", rows.size, "soft" if soft else guarded.frames_kind(None if mixed else codec), True),
             guarded.buf("state", state.size, "state"), guarded.buf("rng", rng.size, "rng")] + _out_specs(total, want)
    inputs = {"offsets": offsets, "frames": rows, "state": state, "rng": rng}
    if resident:
        specs.append(guarded.buf("resident", 4 * pool, "resident"))
        inputs["resident"] = np.zeros(pool, dtype=np.uint32)
    if indexed:
        specs.append(guarded.buf("index", 4 * S, "index", True))
        inputs["index"] = slots.astype(np.int32)
    if mixed:
        specs.append(guarded.buf("codec", S, "codec", True))
        inputs["codec"] = codecs
    names = []

    def call(run):
        tail = (run.p("offsets"), total, run.p("index"), run.p("frames"), run.p("state"), run.p("resident"), run.p("rng"),
                run.p("pcm16"), run.p("pcmf"), run.p("results"), run.p("records"), strm)
        if mixed:
            rc = (L.mbx_process_batch_soft_mixed if soft else L.mbx_process_batch_mixed)(S, run.p("codec"), *tail)
        else:
            rc = (L.mbx_process_batch_soft_ragged if soft else L.mbx_process_batch_ragged)(codec, S, *tail)
        _native.check(rc, "ragged")
        names.append(L.mbx_last_kernel_name(strm).decode())

    idle = np.flatnonzero((counts == 0) | ((codecs >= 4) if mixed else False))

    def after(run, got):
        # a stream without frames (or with a codec byte that names no codec) is not touched: state, RNG state and elision word keep
        # their bytes, and so do its rows of every output (they still hold the pre-fill)
        st, rg = got["state"].reshape(pool, -1), got["rng"].reshape(pool, -1)
        rest = np.setdiff1d(np.arange(pool), slots[np.setdiff1d(np.arange(S), idle)])
        assert st[rest].tobytes() == state.reshape(pool, -1)[rest].tobytes() and rg[rest].tobytes() == rng.reshape(pool, -1)[rest].tobytes(), \
            "a slot without frames changed"
        if resident:
            assert not got["resident"].view(np.uint32)[rest].any(), "the elision word of a slot without frames changed"
        for k in got:
            if k in OUT_BYTES:
                for i in idle:
                    lo, hi = int(offsets[i]) * OUT_BYTES[k], int(offsets[i + 1]) * OUT_BYTES[k]
                    assert got[k][lo:hi].tobytes() == run.arena.prefill_bytes(k, lo, hi).tobytes(), f"{k}: rows of idle stream {i} were written"
                    got[k][lo:hi] = 0   # (the pre-fill differs between the two runs, as it must)

    got = twice("ragged", specs, inputs, call, after=after)
    assert len(set(names)) == 1
    got["kernel"] = names[0]
    return got


for _soft in (False, True):
    for _form, _res, _idx in (("plain", False, False), ("resident", True, False), ("indexed", False, True), ("resident_indexed", True, True)):
        _case(f"ragged-{'soft' if _soft else 'hard'}-{_form}", ["mbx_process_batch_soft_ragged" if _soft else "mbx_process_batch_ragged"], ragged,
              codec=1 if _form == "plain" else 0, soft=_soft, resident=_res, indexed=_idx, mixed=False)
        _case(f"mixed-{'soft' if _soft else 'hard'}-{_form}", ["mbx_process_batch_soft_mixed" if _soft else "mbx_process_batch_mixed"], ragged,
              codec=0, soft=_soft, resident=_res, indexed=_idx, mixed=True)


# ---- S x T batches: hard and soft, every entry point -------------------------------------------------------------------------------
def batch(entry, codec, S, T, want=("pcm16", "pcmf", "results")):
    """entry: batch | batch_ws | indexed | resident | soft | soft_ws | soft_resident | records | records_ws | expanded_ws"""
    import edge_mix
    import soft_mix

    L, _native, strm = _lib()
    soft = entry.startswith("soft")
    n = S * T
    frames = (soft_mix.frames(codec, S, T, 3) if soft else edge_mix.frames(codec, S, T, tag=3)).reshape(-1)
    indexed = entry in ("indexed", "soft_resident")
    resident = entry in ("resident", "soft_resident")
    pool = 2 * S + 3 if indexed else S
    slots = np.arange(pool - 2, 0, -2)[:S]
    state, rng = _initial(pool, 5)
    specs = [guarded.buf("frames", frames.size, "soft" if soft else guarded.frames_kind(codec, one_frame=T == 1), True),
             guarded.buf("state", state.size, "state"), guarded.buf("rng", rng.size, "rng")] + _out_specs(n, want)
    inputs = {"frames": frames, "state": state, "rng": rng}
    scratch = []
    if resident:
        specs.append(guarded.buf("resident", 4 * pool, "resident"))
        inputs["resident"] = np.zeros(pool, dtype=np.uint32)
    if indexed:
        specs.append(guarded.buf("index", 4 * S, "index", True))
        inputs["index"] = slots.astype(np.int32)
    if entry.endswith("_ws"):
        specs.append(guarded.buf("workspace", int(L.mbx_workspace_bytes(n)), "workspace"))   # EXACTLY the documented need
        scratch.append("workspace")
    names = []
    stream_codec = 0 if codec == 2 else codec
    fec = {0: L.mbx_fec_imbe7200x4400, 1: L.mbx_fec_ambe3600x2450, 2: L.mbx_fec_imbe7100x4400, 3: L.mbx_fec_ambe3600x2450}[codec]

    def call(run):
        o = tuple(run.p(k) for k in OUT_ORDER)
        sr = (run.p("state"), run.p("rng"))
        ws = (run.p("workspace"), run.arena.nbytes("workspace")) if "workspace" in run.arena.by_name else None
        if entry == "batch":
            rc = L.mbx_process_batch(codec, S, T, run.p("frames"), *sr, *o, strm)
        elif entry == "batch_ws":
            rc = L.mbx_process_batch_ws(codec, S, T, run.p("frames"), *sr, *o, *ws, strm)
        elif entry == "indexed":
            rc = L.mbx_process_batch_indexed(codec, S, T, run.p("index"), run.p("frames"), *sr, *o, strm)
        elif entry == "resident":
            rc = L.mbx_process_batch_resident(codec, S, T, None, run.p("frames"), run.p("state"), run.p("resident"), run.p("rng"), *o, strm)
        elif entry == "soft":
            rc = L.mbx_process_batch_soft(codec, S, T, run.p("frames"), *sr, *o, strm)
        elif entry == "soft_ws":
            rc = L.mbx_process_batch_soft_ws(codec, S, T, run.p("frames"), *sr, *o, *ws, strm)
        elif entry == "soft_resident":
            rc = L.mbx_process_batch_soft_resident(codec, S, T, run.p("index"), run.p("frames"), run.p("state"), run.p("resident"), run.p("rng"), *o, strm)
        else:   # the staged calls: the FEC launch, then the stream stage from the records
            _native.check(fec(run.p("frames"), n, run.p("records"), strm), "mbx_fec")
            if entry == "records":
                rc = L.mbx_process_records(stream_codec, S, T, run.p("records"), *sr, *o[:3], strm)
            elif entry == "records_ws":
                rc = L.mbx_process_records_ws(stream_codec, S, T, run.p("records"), *sr, *o[:3], *ws, strm)
            else:
                assert entry == "expanded_ws", entry
                _native.check(L.mbx_expand_records_ws(stream_codec, run.p("records"), n, *ws, strm), "mbx_expand_records_ws")
                rc = L.mbx_stream_expanded_ws(stream_codec, S, T, run.p("records"), run.p("state"), None, run.p("rng"), *o[:3], *ws, strm)
        _native.check(rc, entry)
        names.append(L.mbx_last_kernel_name(strm).decode())

    got = twice(f"{entry} codec {codec} {S} x {T}", specs, inputs, call, scratch=scratch)
    assert len(set(names)) == 1, names
    got["kernel"] = names[0]
    return got


_case("soft-plain", ["mbx_process_batch_soft"], batch, entry="soft", codec=0, S=65, T=3)
_case("soft-ws", ["mbx_process_batch_soft_ws"], batch, entry="soft_ws", codec=1, S=257, T=1)
_case("soft-resident-indexed", ["mbx_process_batch_soft_resident"], batch, entry="soft_resident", codec=3, S=63, T=2)
_case("soft-plain-7100", ["mbx_process_batch_soft"], batch, entry="soft", codec=2, S=257, T=1)
_case("records", ["mbx_process_records", "mbx_fec_imbe7200x4400"], batch, entry="records", codec=0, S=257, T=1)
_case("records-ambe", ["mbx_process_records", "mbx_fec_ambe3600x2450"], batch, entry="records", codec=1, S=65, T=3)
_case("records-ws", ["mbx_process_records_ws", "mbx_fec_imbe7100x4400"], batch, entry="records_ws", codec=2, S=257, T=1)
_case("expanded-ws", ["mbx_expand_records_ws", "mbx_stream_expanded_ws"], batch, entry="expanded_ws", codec=3, S=63, T=2)


# ---- optional outputs: each of d_pcm16, d_pcmf, d_results NULL in turn, and all three ------------------------------------------------
def optional_outputs(form, instance, **args):
    fn = form
    full = fn(**args)
    assert full["kernel"] == instance, f"the launch ran {full['kernel']}, this family's case is for {instance}"
    for want in (("pcmf", "results"), ("pcm16", "results"), ("pcm16", "pcmf"), ()):
        part = fn(want=want, **args)
        assert part["kernel"] == full["kernel"], (want, part["kernel"], full["kernel"])
        for k, v in part.items():
            if k != "kernel":
                assert v.tobytes() == full[k].tobytes(), f"outputs {want or 'none'}: {k} differs from the launch with every output"
        assert not (set(OUT_BYTES) - {"records"} - set(want)) & set(part)


for _fam, _inst, _fn, _args in (
        ("stream", "ambe_stream_kernel", batch, dict(entry="batch", codec=1, S=65, T=3)),
        ("one-launch", "imbe_one_launch_kernel", batch, dict(entry="batch", codec=0, S=257, T=1)),
        ("fused", "imbe7100_stream_kernel_one_fused", batch, dict(entry="batch", codec=2, S=257, T=1)),
        ("resident", "ambe2400_stream_kernel_res", batch, dict(entry="resident", codec=3, S=65, T=4)),
        ("indexed", "imbe_stream_kernel", batch, dict(entry="indexed", codec=0, S=63, T=2)),
        ("ragged", "ambe_stream_kernel_ragged_res", ragged, dict(codec=1, soft=False, resident=True, indexed=False, mixed=False)),
        ("mixed", "mixed_stream_kernel_ragged", ragged, dict(codec=0, soft=False, resident=False, indexed=True, mixed=True)),
        ("soft", "imbe_stream_kernel_one", batch, dict(entry="soft", codec=0, S=65, T=1)),
        ("records", "imbe_stream_kernel", batch, dict(entry="records", codec=0, S=65, T=2))):
    _case(f"optional-{_fam}", [], optional_outputs, form=_fn, instance=_inst, **_args)


# ---- single stages at counts on the edges ----------------------------------------------------------------------------------------------
COUNTS = (1, 63, 64, 65, 257)


def stage_in():
    """mbx_stage_in, pinned host memory -> device memory, at byte counts round the 16-byte pieces and their hand-written tail"""
    L, _native, strm = _lib()
    for nbytes in (0, 1, 15, 16, 17, 9 * 7, 9 * 257):
        src_specs = [guarded.buf("src", max(nbytes, 1), "stage", True)]
        data = np.random.default_rng(nbytes).integers(0, 256, size=max(nbytes, 1), dtype=np.uint8)
        host = guarded.Arena(src_specs, where="pinned", seed=3, pinned_alloc=L.mbx_host_alloc, pinned_free=L.mbx_host_free)
        try:
            host.load("src", data)

            def call(run):
                _native.check(L.mbx_stage_in(run.p("dst"), host.ptr("src"), nbytes, strm), "mbx_stage_in")

            def after(run, got):
                assert got["dst"][:nbytes].tobytes() == data[:nbytes].tobytes()
                assert got["dst"][nbytes:].tobytes() == run.arena.prefill_bytes("dst", nbytes, None).tobytes(), "bytes behind the count were written"

            twice(f"mbx_stage_in {nbytes} bytes", [guarded.buf("dst", max(nbytes, 1), "stage")], {}, call, after=after, compare=nbytes > 0)
            host.check(f"mbx_stage_in {nbytes} bytes: host side")
        finally:
            host.close()


_case("stage-in", ["mbx_stage_in"], stage_in)


def floattoshort():
    L, _native, strm = _lib()
    for n in COUNTS:
        pcmf = (np.random.default_rng(n).normal(0, 3000, size=n * 160)).astype(np.float32)

        def call(run):
            _native.check(L.mbx_floattoshort(run.p("in"), run.p("out"), n, strm), "mbx_floattoshort")

        got = twice(f"mbx_floattoshort {n} frames", [guarded.buf("in", n * 640, "f2s_in", True), guarded.buf("out", n * 320, "f2s_out")], {"in": pcmf}, call)
        top = np.float32(32767.0 * 0.95)   # (values against the oracle: tests/test_gpu_parity.py; here: every sample is of THIS input)
        want = np.trunc(np.clip(np.float32(7.0) * pcmf, -top, top)).astype(np.int16)
        assert np.abs(got["out"].view(np.int16).astype(np.int32) - want).max() <= 1


_case("floattoshort", ["mbx_floattoshort"], floattoshort)


def fec_stages():
    """the FEC calls alone (hard and soft) at counts round a block of 256 threads / a wave per frame, and the result histogram over
    results of the edge mix"""
    import edge_mix
    import soft_mix

    L, _native, strm = _lib()
    for n in COUNTS:
        for codec, fn in ((0, L.mbx_fec_imbe7200x4400), (1, L.mbx_fec_ambe3600x2450), (2, L.mbx_fec_imbe7100x4400)):
            frames = edge_mix.frames(codec, n, 1, tag=n & 0xFF).reshape(-1)

            def call(run):
                _native.check(fn(run.p("frames"), n, run.p("records"), strm), "mbx_fec")

            hard = twice(f"mbx_fec codec {codec} x {n}", [guarded.buf("frames", frames.size, guarded.frames_kind(codec), True), guarded.buf("records", 16 * n, "records")],
                         {"frames": frames}, call)
            assert hard["records"].any()
        for codec in (0, 1, 2):
            cells = soft_mix.frames(codec, n, 1, n & 0xFF).reshape(-1)

            def call(run):
                _native.check(L.mbx_fec_soft(codec, run.p("soft"), n, run.p("records"), strm), "mbx_fec_soft")

            twice(f"mbx_fec_soft codec {codec} x {n}", [guarded.buf("soft", cells.size, "soft", True), guarded.buf("records", 16 * n, "records")],
                  {"soft": cells}, call)


_case("fec-stages", ["mbx_fec_imbe7200x4400", "mbx_fec_ambe3600x2450", "mbx_fec_imbe7100x4400", "mbx_fec_soft"], fec_stages)


def materialize():
    """mbx_resident_materialize with and without an index, on the state a resident launch left: the listed slots' third struct is
    written, no other slot and nothing outside the pool"""
    L, _native, strm = _lib()
    for n in COUNTS:
        first = batch("resident", 1, n, 2, want=())
        state, words = first["state"], first["resident"]
        pool = n
        for index in (None, np.arange(n - 1, -1, -2).astype(np.int32)):
            specs = [guarded.buf("state", state.size, "state"), guarded.buf("resident", words.size, "resident")]
            inputs = {"state": state, "resident": words}
            if index is not None:
                specs.append(guarded.buf("index", index.size * 4, "index", True))
                inputs["index"] = index
            m = n if index is None else index.size

            def call(run):
                _native.check(L.mbx_resident_materialize(m, run.p("index"), run.p("state"), run.p("resident"), strm), "mbx_resident_materialize")

            got = twice(f"mbx_resident_materialize {n}", specs, inputs, call)
            named = np.arange(n) if index is None else index
            rest = np.setdiff1d(np.arange(pool), named)
            st0, st1 = state.reshape(pool, 3, -1), got["state"].reshape(pool, 3, -1)
            assert st1[rest].tobytes() == st0[rest].tobytes() and st1[:, :2].tobytes() == st0[:, :2].tobytes()
            assert got["resident"].view(np.uint32)[rest].tobytes() == words.view(np.uint32)[rest].tobytes()
            assert not got["resident"].view(np.uint32)[named].any()
            elided = named[words.view(np.uint32)[named] != 0]
            assert elided.size > 0 or n < 63, "the resident launch left no struct elided: nothing for materialize to write"
            assert st1[elided, 2].tobytes() == st0[elided, 0].tobytes()


_case("materialize", ["mbx_resident_materialize", "mbx_process_batch_resident"], materialize)


def histogram():
    L, _native, strm = _lib()
    for n in COUNTS:
        res = np.random.default_rng(n).integers(0, 9, size=(n, 5)).astype(np.int32)

        def call(run):
            _native.check(L.mbx_result_histogram(run.p("results"), n, run.p("hist"), strm), "mbx_result_histogram")

        got = twice(f"mbx_result_histogram {n}", [guarded.buf("results", 20 * n, "results", True), guarded.buf("hist", 14 * 8, "hist")],
                    {"results": res, "hist": np.zeros(14, dtype=np.uint64)}, call)
        assert int(got["hist"].view(np.uint64)[0]) == n


_case("histogram", ["mbx_result_histogram"], histogram)


def process_frame():
    """one frame of one stream as one launch (mbx_process_frame), every buffer in device memory, per codec; each output NULL in turn"""
    import edge_mix

    L, _native, strm = _lib()
    for codec in range(4):
        frame = edge_mix.frames(codec, 3, 1, tag=1).reshape(3, -1)[1]
        state, rng = _initial(1, 9)
        full = None
        for want in (("pcm16", "pcmf", "results"), ("pcmf", "results"), ("pcm16", "results"), ("pcm16", "pcmf"), ()):
            specs = [guarded.buf("frame", frame.size, guarded.frames_kind(codec), True), guarded.buf("state", state.size, "state"),
                     guarded.buf("rng", rng.size, "rng"), guarded.buf("done", 4, "index")] + _out_specs(1, want)

            def call(run):
                _native.check(L.mbx_process_frame(codec, run.p("frame"), run.p("state"), run.p("rng"), run.p("pcm16"), run.p("pcmf"), run.p("results"),
                                                  run.p("records"), run.p("done"), 0x5A5A1234, strm), "mbx_process_frame")

            got = twice(f"mbx_process_frame codec {codec} outputs {want}", specs, {"frame": frame, "state": state, "rng": rng}, call)
            assert int(got["done"].view(np.uint32)[0]) == 0x5A5A1234
            full = full or got
            for k in got:
                assert got[k].tobytes() == full[k].tobytes(), (codec, want, k)
        # ... and with a device copy of the state (mbx_process_frame_shadow): the same outputs, the copy written whole
        specs = [guarded.buf("frame", frame.size, guarded.frames_kind(codec), True), guarded.buf("state", state.size, "state"),
                 guarded.buf("rng", rng.size, "rng"), guarded.buf("done", 4, "index"), guarded.buf("shadow_state", state.size, "state"),
                 guarded.buf("shadow_rng", rng.size, "rng"), guarded.buf("shadow_ok", 4, "index")] + _out_specs(1, ("pcm16", "pcmf", "results"))

        def call_shadow(run):
            _native.check(L.mbx_process_frame_shadow(codec, run.p("frame"), run.p("state"), run.p("rng"), run.p("pcm16"), run.p("pcmf"), run.p("results"),
                                                     run.p("records"), run.p("done"), 7, run.p("shadow_state"), run.p("shadow_rng"), run.p("shadow_ok"), 0,
                                                     None, strm), "mbx_process_frame_shadow")

        got = twice(f"mbx_process_frame_shadow codec {codec}", specs, {"frame": frame, "state": state, "rng": rng, "shadow_state": state, "shadow_rng": rng},
                    call_shadow)
        for k in full:
            if k != "done":
                assert got[k].tobytes() == full[k].tobytes(), (codec, "shadow", k)
        assert got["shadow_rng"].tobytes() == got["rng"].tobytes() and int(got["shadow_ok"].view(np.uint32)[0]) in (0, 1)
        if int(got["shadow_ok"].view(np.uint32)[0]) == 1:
            assert got["shadow_state"].tobytes() == got["state"].tobytes()


_case("process-frame", ["mbx_process_frame", "mbx_process_frame_shadow"], process_frame)


def single_stages():
    """the single stages of the public API, batched, at counts round a wave and a block: one wavefront or one thread per element"""
    import edge_mix
    import soft_mix
    L, _native, strm = _lib()
    for n in COUNTS:
        state, rng = _initial(n, 21)
        trip = state.reshape(n, 3, -1)
        # a cur / prev pair with a decoded frame in it: the state an AMBE launch of two frames leaves
        after = batch("batch", 1, n, 2, want=())["state"].reshape(n, 3, -1)
        cur, prev = np.ascontiguousarray(after[:, 0]), np.ascontiguousarray(after[:, 1])
        S1 = [guarded.buf("cur", cur.size, "state"), guarded.buf("prev", prev.size, "state")]
        pcm = [guarded.buf("pcmf", 640 * n, "pcmf"), guarded.buf("pcm16", 320 * n, "pcm16")]

        twice(f"mbx_synthesize_speech {n}", S1 + [guarded.buf("rng", rng.size, "rng")] + pcm, {"cur": cur, "prev": prev, "rng": rng},
              lambda r: _native.check(L.mbx_synthesize_speech(n, r.p("cur"), r.p("prev"), r.p("rng"), r.p("pcmf"), r.p("pcm16"), strm), "speech"))
        twice(f"mbx_spectral_amp_enhance {n}", S1[:1], {"cur": cur},
              lambda r: _native.check(L.mbx_spectral_amp_enhance(n, r.p("cur"), strm), "enhance"))
        twice(f"mbx_adaptive_smoothing {n}", [S1[0], guarded.buf("prev", prev.size, "state", True)], {"cur": cur, "prev": prev},
              lambda r: _native.check(L.mbx_adaptive_smoothing(n, r.p("cur"), r.p("prev"), strm), "smoothing"))
        twice(f"mbx_comfort_noise {n}", [guarded.buf("rng", rng.size, "rng")] + pcm, {"rng": rng},
              lambda r: _native.check(L.mbx_comfort_noise(n, r.p("rng"), r.p("pcmf"), r.p("pcm16"), strm), "noise"))
        got = twice(f"mbx_state_copy {n}", [guarded.buf("state", state.size, "state")], {"state": state},
                    lambda r: _native.check(L.mbx_state_copy(n, r.p("state"), strm), "state_copy"))
        assert got["state"].tobytes() == state.tobytes()
        ids = np.random.default_rng(n).integers(0, 256, size=n).astype(np.int32)
        twice(f"mbx_synthesize_tone {n}", [guarded.buf("ids", 4 * n, "index", True), S1[0]] + pcm, {"ids": ids, "cur": np.ascontiguousarray(trip[:, 0])},
              lambda r: _native.check(L.mbx_synthesize_tone(n, None, r.p("ids"), r.p("cur"), r.p("pcmf"), r.p("pcm16"), strm), "tone"))
        words = np.random.default_rng(n + 1).integers(0, 1 << 23, size=n).astype(np.uint32)
        for kind in (0, 1, 2):
            twice(f"mbx_ecc_words {kind} x {n}", [guarded.buf("in", 4 * n, "index", True), guarded.buf("out", 4 * n, "index"), guarded.buf("errs", 4 * n, "index")],
                  {"in": words}, lambda r: _native.check(L.mbx_ecc_words(kind, r.p("in"), n, r.p("out"), r.p("errs"), strm), "ecc"))
            width = 23 if kind == 0 else 15
            cells = np.random.default_rng(n + kind).integers(0, 256, size=(n, width, 2)).astype(np.uint8)
            cells[:, :, 0] &= 1
            twice(f"mbx_ecc_soft_words {kind} x {n}", [guarded.buf("in", cells.size, "soft", True), guarded.buf("out", 4 * n, "index"), guarded.buf("errs", 4 * n, "index")],
                  {"in": cells}, lambda r: _native.check(L.mbx_ecc_soft_words(kind, r.p("in"), n, r.p("out"), r.p("errs"), strm), "ecc soft"))
        for codec in (0, 1, 2):
            hard, _ = soft_mix.cells_from_packed(codec, edge_mix.frames(codec, n, 1, tag=2).reshape(n, -1))
            hard = np.ascontiguousarray(hard, dtype=np.uint8)
            hard[n // 2, 3] = 2   # one frame with a cell outside {0, 1}
            got = twice(f"mbx_pack_cells {codec} x {n}", [guarded.buf("cells", hard.size, "cells", True), guarded.buf("packed", FB[codec] * n, "frames"),
                                                          guarded.buf("status", 4 * n, "index")], {"cells": hard},
                        lambda r: _native.check(L.mbx_pack_cells(codec, r.p("cells"), n, r.p("packed"), r.p("status"), strm), "pack"))
            assert np.flatnonzero(got["status"].view(np.int32)).tolist() == [n // 2]
        # the sub-stages of the frame decode (packed frames in, packed frames or records out) and the parameter decode alone
        for codec in (0, 1, 2):
            frames = edge_mix.frames(codec, n, 1, tag=6).reshape(-1)
            fin = guarded.buf("in", frames.size, "frames", True)
            twice(f"mbx_fec_stage C0 {codec} x {n}", [fin, guarded.buf("out", frames.size, "frames")], {"in": frames},
                  lambda r: _native.check(L.mbx_fec_stage(codec, 1, r.p("in"), n, r.p("out"), None, strm), "fec_stage"))
            twice(f"mbx_fec_stage DATA {codec} x {n}", [fin, guarded.buf("records", 16 * n, "records")], {"in": frames},
                  lambda r: _native.check(L.mbx_fec_stage(codec, 4, r.p("in"), n, None, r.p("records"), strm), "fec_stage"))
        recs = batch("batch", 3, n, 1, want=())["records"]
        twice(f"mbx_decode_parms {n}", [guarded.buf("records", recs.size, "records", True)] + S1 + [guarded.buf("rc", 4 * n, "index")],
              {"records": recs, "cur": np.ascontiguousarray(trip[:, 0]), "prev": np.ascontiguousarray(trip[:, 1])},
              lambda r: _native.check(L.mbx_decode_parms(3, r.p("records"), n, r.p("cur"), r.p("prev"), r.p("rc"), strm), "decode_parms"))
        # the two halves of mbx_process_records through the stream's own workspace, on ABI triplets and on resident state
        for res in (False, True):
            specs = [guarded.buf("records", recs.size, "records", True), guarded.buf("state", state.size, "state"), guarded.buf("rng", rng.size, "rng")] + \
                _out_specs(n, ("pcm16", "pcmf", "results"))[1:] + ([guarded.buf("resident", 4 * n, "resident")] if res else [])
            inputs = {"records": recs, "state": state, "rng": rng}
            if res:
                inputs["resident"] = np.zeros(n, dtype=np.uint32)

            def halves(r):
                _native.check(L.mbx_expand_records(3, r.p("records"), n, strm), "mbx_expand_records")
                o = (r.p("pcm16"), r.p("pcmf"), r.p("results"))
                if res:
                    rc = L.mbx_stream_expanded_resident(3, n, 1, r.p("records"), r.p("state"), r.p("resident"), r.p("rng"), *o, strm)
                else:
                    rc = L.mbx_stream_expanded(3, n, 1, r.p("records"), r.p("state"), r.p("rng"), *o, strm)
                _native.check(rc, "mbx_stream_expanded")

            twice(f"mbx_expand_records + mbx_stream_expanded{'_resident' if res else ''} {n}", specs, inputs, halves)


_case("single-stages", ["mbx_synthesize_speech", "mbx_spectral_amp_enhance", "mbx_adaptive_smoothing", "mbx_comfort_noise", "mbx_state_copy",
                        "mbx_synthesize_tone", "mbx_ecc_words", "mbx_ecc_soft_words", "mbx_pack_cells", "mbx_fec_stage", "mbx_decode_parms",
                        "mbx_expand_records", "mbx_stream_expanded", "mbx_stream_expanded_resident"], single_stages)


def host_calls():
    """the *_host conveniences: caller arrays in pageable HOST memory, guarded the same way (the library stages through device
    buffers of its own)"""
    import edge_mix
    import soft_mix

    L, _native, _ = _lib()
    for codec, S, T in ((0, 65, 1), (1, 63, 2)):
        n = S * T
        frames = edge_mix.frames(codec, S, T, tag=8).reshape(-1)
        cells = soft_mix.frames(codec, S, T, 8).reshape(-1)
        state, rng = _initial(S, 13)
        outs = [guarded.buf(k, n * OUT_BYTES[k], k) for k in OUT_ORDER]
        sr = [guarded.buf("state", state.size, "state"), guarded.buf("rng", rng.size, "rng")]
        twice(f"mbx_process_batch_host {codec}", [guarded.buf("frames", frames.size, guarded.frames_kind(codec), True)] + sr + outs,
              {"frames": frames, "state": state, "rng": rng}, where="numpy",
              call=lambda r: _native.check(L.mbx_process_batch_host(codec, S, T, r.p("frames"), r.p("state"), r.p("rng"), *[r.p(k) for k in OUT_ORDER]), "host"))
        twice(f"mbx_process_batch_soft_host {codec}", [guarded.buf("soft", cells.size, "soft", True)] + sr + outs,
              {"soft": cells, "state": state, "rng": rng}, where="numpy",
              call=lambda r: _native.check(L.mbx_process_batch_soft_host(codec, S, T, r.p("soft"), r.p("state"), r.p("rng"), *[r.p(k) for k in OUT_ORDER]), "host"))
        twice(f"mbx_fec_host {codec}", [guarded.buf("frames", frames.size, guarded.frames_kind(codec), True), guarded.buf("records", 16 * n, "records")],
              {"frames": frames}, where="numpy", call=lambda r: _native.check(L.mbx_fec_host(codec, r.p("frames"), n, r.p("records")), "host"))
        twice(f"mbx_fec_soft_host {codec}", [guarded.buf("soft", cells.size, "soft", True), guarded.buf("records", 16 * n, "records")],
              {"soft": cells}, where="numpy", call=lambda r: _native.check(L.mbx_fec_soft_host(codec, r.p("soft"), n, r.p("records")), "host"))
        pcmf = np.random.default_rng(n).normal(0, 3000, size=n * 160).astype(np.float32)
        twice(f"mbx_floattoshort_host {n}", [guarded.buf("in", pcmf.size * 4, "f2s_in", True), guarded.buf("out", pcmf.size * 2, "f2s_out")],
              {"in": pcmf}, where="numpy", call=lambda r: _native.check(L.mbx_floattoshort_host(r.p("in"), r.p("out"), n), "host"))
        trip = state.reshape(S, 3, -1)
        twice(f"mbx_synthesize_speech_host {S}", [guarded.buf("cur", trip[:, 0].size, "state"), guarded.buf("prev", trip[:, 1].size, "state"),
                                                  guarded.buf("rng", rng.size, "rng"), guarded.buf("pcmf", 640 * S, "pcmf"), guarded.buf("pcm16", 320 * S, "pcm16")],
              {"cur": np.ascontiguousarray(trip[:, 0]), "prev": np.ascontiguousarray(trip[:, 1]), "rng": rng}, where="numpy",
              call=lambda r: _native.check(L.mbx_synthesize_speech_host(S, r.p("cur"), r.p("prev"), r.p("rng"), r.p("pcmf"), r.p("pcm16")), "host"))
        soft23 = np.random.default_rng(S).integers(0, 256, size=(n, 23, 2)).astype(np.uint8)
        soft23[:, :, 0] &= 1
        twice(f"mbx_ecc_soft_words_host {n}", [guarded.buf("in", soft23.size, "soft", True), guarded.buf("out", 4 * n, "index"), guarded.buf("errs", 4 * n, "index")],
              {"in": soft23}, where="numpy", call=lambda r: _native.check(L.mbx_ecc_soft_words_host(0, r.p("in"), n, r.p("out"), r.p("errs")), "host"))


_case("host-calls", ["mbx_process_batch_host", "mbx_process_batch_soft_host", "mbx_fec_host", "mbx_fec_soft_host", "mbx_floattoshort_host",
                     "mbx_synthesize_speech_host", "mbx_ecc_soft_words_host"], host_calls)

BY_ID = {c.id: c for c in CASES}
assert len(BY_ID) == len(CASES)


def run(case_id):
    c = BY_ID[case_id]
    return c.fn(**c.args)


if __name__ == "__main__":
    run(sys.argv[1])
    print("ok", sys.argv[1])
