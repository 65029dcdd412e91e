"""GPU suite (-m gpu): the one-frame stream instances leave an all-zero previousUw unstored where the slot already holds zeros
(store_parms / UwSkip, mbx_stream.hip).  That may not change a byte: everything here is compared as bytes, never within the
tolerances of parity.check_state.  Workloads and runners: tests/silent_store_cases.py."""
import numpy as np
import pytest

import silent_store_cases as cases

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def device():
    import mbelib_neo_amd as m

    m.lib()   # raises NativeLibraryError if the HIP extension is missing
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    from mbelib_neo_amd import decoder

    decoder.ensure_init(0)


_scripted = {}


def scripted(codec, oracle):
    """the scripted history of a codec, made and classified once (on the CPU, before anything runs on the GPU)"""
    if codec not in _scripted:
        cases.check_encoder(codec, oracle)
        frames, state, seeds = cases.scripted(codec, oracle)
        cls = cases.classes(codec, oracle, frames, state, seeds)
        missing = {a + b for a in cases.CLASSES for b in cases.CLASSES} - cases.pairs_seen(cls)
        assert not missing, f"codec {codec}: the scripts never bring {sorted(missing)} as (frame, next frame)"
        _scripted[codec] = (frames, state, seeds)
    return _scripted[codec]


@pytest.mark.parametrize("codec,resident", [(0, False), (2, False), (0, True)])
def test_scripted_history_tick_by_tick_equals_one_long_launch(device, oracle, codec, resident):
    """67 streams x six T = 1 launches (mbx_process_batch; mbx_process_batch_resident + materialize), every ordered pair of
    {all-voiced, unvoiced, repeat, mute} among them: after every tick state, RNG, results and PCM are byte-identical to one
    launch of T = k, in both walking orders."""
    frames, state, seeds = scripted(codec, oracle)
    cases.run_history(codec, frames, state, seeds, resident=resident)


def test_repeat_after_unvoiced_frames_stores_the_repeated_previousUw(device, oracle):
    """unvoiced, unvoiced, repeat, all-voiced: the repeat replaces cur_mp's registers with prev_mp's struct, so what the cur_mp slot
    holds must have been read off the registers as loaded -- the fourth tick would otherwise leave old bytes in cur_mp."""
    frames, state, seeds = cases.scripted(0, oracle, scripts=(("UUXV", False),), tag=1)
    cls = cases.classes(0, oracle, frames, state, seeds)
    assert (cls == np.array(list("UURV"))[None, :]).all(axis=1).sum() >= cases.S // 2, cls[:8]
    cases.run_history(0, frames, state, seeds)


@pytest.mark.parametrize("codec,resident", [(0, False), (2, False), (0, True)])
def test_planted_previousUw_is_overwritten_or_rightly_left(device, oracle, codec, resident):
    """One all-voiced tick over previousUw planted through dec.state: zeros over zeros (the skipped store), zeros over values,
    -0.0f, a NaN, a single dword at either end, and a prev_mp_enhanced whose unread lower half is set."""
    from mbelib_neo_amd import decoder, framegen
    from mbelib_neo_amd.layout import init_state

    n = cases.S
    seeds = np.arange(n) + 77
    frames = cases.frames_of(codec, "V" * n, framegen.rng_for(0x51E72000 + codec), oracle)
    ref = oracle.process_batch(codec, n, 1, frames, oracle.init_state(n), oracle.rng_seeded(seeds))
    assert not (ref["results"]["flags"] & (cases.FLAG_REPEAT | cases.FLAG_MUTE)).any()
    patterns = cases.planted_patterns()
    dec = decoder.BatchDecoder(codec, n, seeds=seeds, resident=resident)
    staged = decoder.BatchDecoder(codec, n, seeds=seeds)
    cases.plant(dec, patterns)
    cases.plant(staged, patterns)
    dec.decode(frames, 1)
    cases.staged_step(staged, frames)
    got, got_rng = cases._snapshot(dec)
    want, want_rng = cases._snapshot(staged)
    uw = got["previousUw"].view(np.uint32)
    assert not uw[:, 0].any(), f"cur_mp.previousUw not all +0 in streams {np.flatnonzero(uw[:, 0].any(axis=1))}"
    assert not uw[:, 2].any(), f"prev_mp_enhanced.previousUw not all +0 in streams {np.flatnonzero(uw[:, 2].any(axis=1))}"
    planted = np.zeros((n, 256), dtype=np.uint32)
    for s, (cur, _) in zip(cases.PLANTED_STREAMS, patterns.values()):
        planted[s] = cur
    assert np.array_equal(uw[:, 1], planted), "prev_mp.previousUw is not what cur_mp held before the frame"
    assert got.tobytes() == want.tobytes() and got_rng.tobytes() == want_rng.tobytes(), "differs from the staged one-frame path"
    assert np.array_equal(init_state(1)["previousUw"].view(np.uint32), np.zeros((1, 3, 256), dtype=np.uint32))
