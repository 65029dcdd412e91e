"""GPU suite (-m gpu): where the kernels write and read.  Every buffer a launch is handed lies in one guarded arena (tests/guarded.py:
exact size, exactly the alignment include/mbx.h states for its kind and no better, 16 KB of patterned guard of its own on both sides,
outputs pre-filled with the pattern), and every case runs twice from the same inputs under two patterns: guards and read-only inputs
intact after every launch, every output / state / RNG / elision byte identical between the runs, rows a launch must leave alone still
holding the pre-fill.
  * every row of the kernel-instance table: tests/instance_cases.py, run through GuardedBuffers -- the oracle comparison and the
    mbx_last_kernel_name assertion run on the guarded buffers, on the very launches the guards watch; cases with environment switches
    in a fresh child, as in tests/test_gpu_instances.py;
  * the other launch forms, the optional outputs and the single stages: tests/memory_cases.py.
No kernel is ever built or asked to write out of bounds: the checker is shown to bite by a torch write into a guard."""
import os
import subprocess
import sys

import numpy as np
import pytest

import guarded
import instance_cases
import memory_cases

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))


@pytest.fixture(scope="module")
def device():
    import mbelib_neo_amd as m

    m.lib()   # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)


def test_the_checker_finds_a_planted_byte_on_the_device(device):
    """one guard byte and one byte of a read-only input, changed by a torch write into the arena (nothing else: no kernel writes out
    of bounds on purpose): check() names the buffer, the side and the distance"""
    specs = [guarded.buf("frames", 18 * 257, "frames4", True), guarded.buf("pcm16", 320 * 257, "pcm16"), guarded.buf("records", 16 * 257, "records")]
    a = guarded.Arena(specs, where="cuda", seed=1)
    a.load("frames", np.arange(18 * 257, dtype=np.uint8))
    for s in a.slots:
        al = guarded.ALIGN[s.kind]
        assert (a.base + s.start) % al == 0 and (a.base + s.start) % (2 * al) == al and s.start - s.front >= guarded.GUARD and s.back - s.end >= guarded.GUARD
    a.check()
    s = a.by_name["pcm16"]
    keep = a.mem[s.end + 318].clone()
    a.mem[s.end + 318] ^= 0x40   # sample 159 of the row behind the last one
    with pytest.raises(guarded.GuardError, match=r"pcm16: 1 guard byte\(s\) changed BEHIND the payload of 82240 bytes, 318 \.\. 318 bytes past its end"):
        a.check()
    a.mem[s.end + 318] = keep
    a.check()
    a.mem[s.start - 2] ^= 1
    with pytest.raises(guarded.GuardError, match=r"pcm16: 1 guard byte\(s\) changed IN FRONT OF the payload, 2 \.\. 2 bytes before its first byte"):
        a.check()
    a.mem[s.start - 2] ^= 1
    f = a.by_name["frames"]
    a.mem[f.start + 4000] ^= 0x80
    with pytest.raises(guarded.GuardError, match=r"frames: read-only input changed: 1 byte\(s\), first at offset 4000, last at offset 4000 of 4626"):
        a.check()
    a.mem[f.start + 4000] ^= 0x80
    a.check()
    # the pre-fill of an output is the pattern of ITS offsets under THIS seed: a second arena's differs
    b = guarded.Arena(specs, where="cuda", seed=2)
    assert a.read("pcm16").tobytes() == a.prefill_bytes("pcm16").tobytes() != b.read("pcm16").tobytes()


def _child(argv, switches, timeout, what):
    keep = ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")
    env = {k: v for k, v in os.environ.items() if not k.startswith("MBX_") or k in keep}
    env.update(switches)
    try:
        r = subprocess.run([sys.executable] + argv, capture_output=True, text=True, timeout=timeout, env=env)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"{what}: the child process did not finish in {e.timeout} s -- nothing more is started on the card", returncode=3)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"{what}: the child process ended with status {r.returncode} (a signal, an abort or a fault) -- nothing more is "
                    f"started on the card\n{tail}", returncode=3)
    assert r.returncode == 0, f"{what}: exit status {r.returncode}\n{tail}"
    print(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("case_id", [c.id for c in instance_cases.CASES])
def test_instance_row_stays_inside_its_buffers_and_runs_twice_to_the_same_bytes(device, case_id):
    case = instance_cases.BY_ID[case_id]
    keep = ("MBX_HIP_LIBRARY", "MBX_ORACLE_LIBRARY")
    if not case.env and not any(k.startswith("MBX_") and k not in keep for k in os.environ):
        print(case_id, instance_cases.run_guarded(case))
        return
    _child([os.path.join(HERE, "instance_cases.py"), case_id, "--guarded"], case.env, 2 * instance_cases.child_timeout(case), case_id)


@pytest.mark.parametrize("case_id", [c.id for c in memory_cases.CASES])
def test_launch_form_stays_inside_its_buffers_and_runs_twice_to_the_same_bytes(device, case_id):
    memory_cases.run(case_id)


def test_a_guarded_batch_equals_the_same_batch_on_plain_allocations(device):
    """the weakest legal alignment changes no byte: the guarded runs of the S x T entry points against BatchDecoder on torch's buffers"""
    import edge_mix
    from mbelib_neo_amd import decoder

    for codec, S, T in ((1, 65, 3), (0, 257, 1)):
        got = memory_cases.batch("batch", codec, S, T)
        dec = decoder.BatchDecoder(codec, S)
        state, rng = memory_cases._initial(S, 5)
        import torch

        dec.state.copy_(torch.from_numpy(state))
        dec.rng.copy_(torch.from_numpy(rng))
        out = dec.decode(edge_mix.frames(codec, S, T, tag=3).reshape(-1, memory_cases.FB[codec]), T, want_float=True)
        torch.cuda.synchronize()
        for k in ("records", "results", "pcm16", "pcmf"):
            assert out[k].cpu().numpy().tobytes() == got[k].tobytes(), (codec, S, T, k)
        assert dec.state.cpu().numpy().tobytes() == got["state"].tobytes() and dec.rng.cpu().numpy().tobytes() == got["rng"].tobytes()


def test_every_launcher_refuses_a_pointer_below_its_alignment_before_it_launches(device):
    """MBE_STATUS_INVALID_ARGUMENT and a message that names the call, from the host-side check: nothing is ever launched on a
    misaligned pointer (every buffer still holds its zeros afterwards)"""
    import torch
    from mbelib_neo_amd import _native

    L = _native.lib()
    S, T = 4, 1
    t = {k: torch.zeros(n + 64, dtype=torch.uint8, device="cuda") for k, n in
         (("frames", 18 * S), ("state", 7812 * S), ("rng", 24 * S), ("pcm16", 320 * S), ("pcmf", 640 * S), ("results", 20 * S), ("records", 16 * S),
          ("ws", 256 * S), ("index", 4 * S), ("resident", 4 * S), ("hist", 14 * 8), ("soft", 368 * S))}
    torch.cuda.synchronize()
    ok = {k: v.data_ptr() for k, v in t.items()}
    strm = torch.cuda.current_stream().cuda_stream

    def refused(who, fn, *args):
        assert L.mbx_stage_in(ok["ws"] + 8, ok["ws"], 16, strm) == -1 and b"mbx_stage_in" in L.mbx_last_error()   # (another call's text first ...)
        assert fn(*args) == -1, who
        text = L.mbx_last_error()
        assert b"align" in text and who.encode() in text, (who, text)   # ... so this text is this call's

    for name, by in (("records", 8), ("rng", 4), ("pcm16", 1), ("pcmf", 2), ("results", 2), ("state", 2), ("index", 2), ("resident", 2), ("ws", 8), ("frames", 1)):
        a = dict(ok)
        a[name] += by
        out = (a["pcm16"], a["pcmf"], a["results"], a["records"])
        if name not in ("ws", "index", "resident"):
            refused("mbx_process_batch_ws", L.mbx_process_batch_ws, 0, S, T, a["frames"], a["state"], a["rng"], *out, ok["ws"], 256 * S, strm)
            refused("mbx_process_frame", L.mbx_process_frame, 0, a["frames"], a["state"], a["rng"], *out, None, 0, strm)
        if name not in ("ws", "index", "resident", "frames"):
            refused("mbx_process_records", L.mbx_process_records, 0, S, T, a["records"], a["state"], a["rng"], *out[:3], strm)
            refused("mbx_stream_expanded_ws", L.mbx_stream_expanded_ws, 0, S, T, a["records"], a["state"], None, a["rng"], *out[:3], ok["ws"], 256 * S, strm)
        if name == "ws":
            refused("mbx_process_batch_ws", L.mbx_process_batch_ws, 0, S, T, a["frames"], a["state"], a["rng"], *out, a["ws"], 256 * S, strm)
            refused("mbx_expand_records_ws", L.mbx_expand_records_ws, 0, a["records"], S, a["ws"], 256 * S, strm)
        else:
            refused("mbx_process_batch_resident", L.mbx_process_batch_resident, 0, S, T, a["index"], a["frames"], a["state"], a["resident"], a["rng"], *out, strm)
    assert L.mbx_process_batch(1, S, T, ok["frames"] + 1, ok["state"], ok["rng"], None, None, None, ok["records"], strm) == 0   # AMBE frames may sit anywhere
    refused("mbx_fec", L.mbx_fec_imbe7200x4400, ok["frames"] + 1, S, ok["records"], strm)
    refused("mbx_fec", L.mbx_fec_imbe7100x4400, ok["frames"], S, ok["records"] + 8, strm)
    refused("mbx_fec_soft", L.mbx_fec_soft, 0, ok["soft"] + 1, S, ok["records"], strm)
    refused("mbx_fec_stage", L.mbx_fec_stage, 0, 4, ok["frames"], S, None, ok["records"] + 4, strm)
    refused("mbx_result_histogram", L.mbx_result_histogram, ok["results"], S, ok["hist"] + 4, strm)
    refused("mbx_resident_materialize", L.mbx_resident_materialize, S, None, ok["state"] + 2, ok["resident"], strm)
    refused("mbx_decode_parms", L.mbx_decode_parms, 0, ok["records"] + 8, S, ok["state"], ok["state"], ok["index"], strm)
    refused("mbx_pack_cells", L.mbx_pack_cells, 0, ok["soft"] + 2, 1, ok["frames"], None, strm)
    refused("mbx_ecc_words", L.mbx_ecc_words, 0, ok["index"] + 2, S, ok["index"], None, strm)
    refused("mbx_synthesize_speech", L.mbx_synthesize_speech, S, ok["state"], ok["state"], ok["rng"] + 4, ok["pcmf"], None, strm)
    refused("mbx_floattoshort", L.mbx_floattoshort, ok["pcmf"] + 4, ok["pcm16"], 1, strm)
    refused("mbx_floattoshort", L.mbx_floattoshort, ok["pcmf"], ok["pcm16"] + 2, 1, strm)
    torch.cuda.synchronize()
    for k, v in t.items():
        if k not in ("state", "rng", "records"):   # (the one accepted AMBE call above decoded into these)
            assert not v.any(), k   # nothing else ran
