"""CPU suite (-m "not gpu"): the model lattices of tests/model_lattice.py hold what they claim.  Every lattice builds the same bytes
twice; its composition holds in the ORACLE's answer (the oracle is the checker of these lattices: no fixture); outside the
non-finite classes the oracle's PCM is finite; at least 90 % of each synthesis lattice's structs stay below the soft clip; and the
oracle with the reference's own float FFT differs from the double-precision default by less than a tenth of parity.PCM_REL_RMS in
every group the GPU tests apply that bound to, so the bound is about the kernels and not about the checker."""
import numpy as np
import pytest

import model_lattice
import oracle_lib
import parity


@pytest.mark.parametrize("name", model_lattice.NAMES)
def test_lattice_builds_the_same_bytes_twice(name):
    a, b = model_lattice.lattice_bytes(name), model_lattice.lattice_bytes(name)
    assert a == b and len(a) > 0
    lat = model_lattice.build(name)
    n = lat.cur.shape[0]
    assert n <= model_lattice.MAX_STRUCTS and len(lat.text) == n and lat.cls.shape == (n,)
    assert all(t.startswith(f"{name}[{s}] class {lat.cls[s]}:") for s, t in enumerate(lat.text))
    covered = np.concatenate([idx for _, idx in model_lattice.groups(name)])
    assert sorted(covered.tolist()) == list(range(n)) and max(len(i) for _, i in model_lattice.groups(name)) <= model_lattice.GROUP


@pytest.mark.parametrize("name", model_lattice.NAMES)
def test_composition_holds_in_the_oracle(name):
    print("COMPOSITION", name, model_lattice.composition(name))


@pytest.mark.parametrize("codec", model_lattice.TONE_STREAM_CODECS)
def test_tone_streams_hold_every_id(codec):
    f = model_lattice.tone_stream_frames(codec)
    assert f.shape == (256, 4, 9) and f.tobytes() == model_lattice.tone_stream_frames.__wrapped__(codec).tobytes()
    print("COMPOSITION tone streams", codec, model_lattice.tone_stream_composition(codec))


@pytest.mark.parametrize("name", model_lattice.SYNTHESIS)
def test_synthesis_lattice_is_finite_and_below_the_clip(name):
    ref = model_lattice.oracle(name, "speech")
    assert np.isfinite(ref["pcmf"]).all(), f"{name}: the oracle's PCM is not finite"
    for x in ("cur", "prev"):
        for field in ("Ml", "PHIl", "PSIl", "localEnergy", "previousUw"):
            assert np.isfinite(ref[x][field]).all(), f"{name}: {x}.{field} is not finite in the oracle's answer"
    share = float(np.mean(model_lattice.below_clip(ref["pcmf"])))
    print("BELOW_CLIP", name, round(share, 4))
    assert share >= model_lattice.MIN_SHARE_BELOW_CLIP, f"{name}: only {share:.3f} of the structs stay below the soft clip"


def test_float_fft_and_double_fft_agree_on_the_lattices():
    o = oracle_lib.load()
    worst = {}
    for name in model_lattice.SYNTHESIS:
        lat = model_lattice.build(name)
        default = model_lattice.oracle(name, "speech")
        o.set_fft_float(1)
        try:
            pcmf, cur, prev, rng = o.synthesize_speech(lat.cur, lat.prev, lat.rng)
        finally:
            o.set_fft_float(0)
        assert rng.tobytes() == default["rng"].tobytes()
        for cls, idx in model_lattice.groups(name):
            total, frame, _ = parity.pcm_float_stats(default["pcmf"][idx], pcmf[idx])
            worst[name] = max(worst.get(name, 0.0), total)
            assert total < 0.1 * parity.PCM_REL_RMS, f"{name} class {cls}: the oracle's two transforms differ by {total:.3e} relative RMS"
            assert frame < 0.1 * parity.PCM_WORST_FRAME, f"{name} class {cls}: the oracle's two transforms differ by {frame:.3e} in one frame"
            for x, got in (("cur", cur), ("prev", prev)):
                parity.check_state(default[x][idx], got[idx], rel=0.1 * parity.STATE_REL_RMS, what=f"{name} class {cls}: {x} under the float FFT")
    print("FFT_FLOAT_VS_DOUBLE", {k: float(f"{v:.3e}") for k, v in worst.items()})
