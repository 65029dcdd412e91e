"""GPU suite (-m gpu) for the per-frame library on several shards (MBX_DEVICES, include/mbe_neo_shards.h): queue mode spread over
the entries of the device list must hand back the bytes of the synchronous calls, place every channel on (home + k) % shards and
account for every row.  The GPU machine has one card for this, so every list names device 0, several times: independent shards --
streams, pools, launch sets -- on one device.  The library reads the variable once per process: every case but the unset one runs in
a fresh child (tests/queue_shards_case.py) under a time limit, and the last one runs the existing queue-mode tests of
tests/test_gpu_shim_api.py in a child with four shards."""
import os
import re
import subprocess
import sys
import time

import numpy as np
import pytest

from queue_channels import MBE_BATCH_QUEUE_SOFT, Channel

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _child(what, argv, env_extra, timeout, cwd=None):
    """a fresh process under a time limit; one that does not end, or ends by a signal, ends the session: nothing more is started on the card"""
    env = dict(os.environ, **env_extra)
    try:
        r = subprocess.run(argv, capture_output=True, text=True, timeout=timeout, env=env, cwd=cwd)
    except subprocess.TimeoutExpired as e:
        pytest.exit(f"{what}: the child process did not finish in {e.timeout} s -- nothing more is started on the card", returncode=3)
    tail = (r.stdout or "")[-3000:] + (r.stderr or "")[-3000:]
    if r.returncode < 0 or r.returncode in (124, 134, 137, 139):
        pytest.exit(f"{what}: the child process ended with status {r.returncode} -- nothing more is started on the card\n{tail}", returncode=3)
    return r, tail


def _shards_case(case, shards, env_extra=None, modes=("0", "1")):
    """tests/queue_shards_case.py with device 0 named `shards` times: {mode: its line}"""
    env = dict(env_extra or {}, MBX_DEVICES=",".join(["0"] * shards))
    r, tail = _child(f"queue_shards_case {case}", [sys.executable, os.path.join(HERE, "queue_shards_case.py"), case, str(shards)], env, 300)
    assert r.returncode in (0, 1), tail
    lines = dict(line.split(" ", 1) for line in r.stdout.strip().splitlines())
    assert sorted(lines) == sorted(modes), tail
    return lines


@pytest.fixture(scope="module")
def mbe():
    import mbelib_neo_amd as m

    m.lib()
    import torch

    assert torch.cuda.is_available(), "GPU tests need a HIP device"
    import shim_lib
    from queue_shards_case import bind

    return bind(shim_lib.load())


@pytest.fixture(scope="module")
def four_shards(mbe):
    return _shards_case("mixed48", 4)


@pytest.fixture(scope="module")
def three_shards_by_dma(mbe):
    return _shards_case("mixed48", 3, {"MBE_NEO_ZERO_COPY_FLUSH": "0"})


@pytest.fixture(scope="module")
def reentry(mbe):
    return _shards_case("reentry", 3)


@pytest.mark.parametrize("mode", [0, 1], ids=["writeback", "resident"])
def test_48_channels_over_four_shards_equal_the_synchronous_calls(four_shards, mode):
    """MBX_DEVICES=0,0,0,0: channel c on shard c % 4, one flush pass and 12 channels per shard, the rows summing to the frames queued;
    PCM, results, parameter bits and the three structs of every channel the synchronous calls' bytes"""
    assert four_shards[str(mode)] == "ok", four_shards[str(mode)]


@pytest.mark.parametrize("mode", [0, 1], ids=["writeback", "resident"])
def test_48_channels_over_three_shards_by_dma_copies_equal_the_synchronous_calls(three_shards_by_dma, mode):
    """MBX_DEVICES=0,0,0 with MBE_NEO_ZERO_COPY_FLUSH=0: three shards of 16 channels, each flushing through uploads and copies"""
    assert three_shards_by_dma[str(mode)] == "ok", three_shards_by_dma[str(mode)]


@pytest.mark.parametrize("mode", [0, 1], ids=["writeback", "resident"])
def test_channels_that_leave_and_come_back_move_on_to_the_next_shard(reentry, mode):
    """MBX_DEVICES=0,0,0, twelve channels in three ticks: a channel released by a direct call comes back on shard 12 % 3, one released
    by mbe_batchRelease on 13 % 3, a channel that changes its input form flushes the whole batch; every byte as by synchronous calls"""
    assert reentry[str(mode)] == "ok", reentry[str(mode)]


def test_four_host_threads_have_four_homes_and_the_synchronous_bytes(mbe):
    """MBX_DEVICES=0,0,0,0, resident mode: four threads with six channels each, three flushes of three frames"""
    lines = _shards_case("threads", 4, modes=("1",))
    assert lines["1"] == "ok", lines["1"]


def test_without_the_variable_there_is_one_shard_and_one_flush_pass(mbe):
    assert "MBX_DEVICES" not in os.environ, "this test is about the library without MBX_DEVICES"
    from queue_shards_case import census

    assert mbe.mbq_shard_count() == 1
    assert mbe.mbq_shard_device(0) == int(os.environ.get("MBX_DEVICE", "0")) and mbe.mbq_shard_device(1) == -1 and mbe.mbq_shard_device(-1) == -1
    assert mbe.mbq_thread_home() == 0
    chans = [Channel(mbe, c) for c in range(48)]
    pending = [int(k) for k in 1 + np.arange(48) * 5 % 9]
    assert mbe.mbq_channel_shard(chans[0].p(chans[0].st[0])) == -1
    assert mbe.mbe_batchBegin(1 | MBE_BATCH_QUEUE_SOFT) == 0
    try:
        assert census(mbe, 0) == (0, 0, 0, 0)
        for ch, k in zip(chans, pending):
            for _ in range(k):
                ch.call(mbe)
        assert [mbe.mbq_channel_shard(ch.p(ch.st[0])) for ch in chans] == [0] * 48
        assert mbe.mbe_flush() == sum(pending)
        assert census(mbe, 0) == (1, sum(pending), 48, 48)
        assert mbe.mbq_shard_census(1, None) == -1
    finally:
        assert mbe.mbe_batchEnd() >= 0
    assert all(r == 0 for ch in chans for r in ch.rets)


def test_the_existing_queue_mode_tests_pass_on_four_shards(mbe):
    """tests/test_gpu_shim_api.py -k queue_mode -- four test functions, one of them in both state modes: five cases -- in a child with
    MBX_DEVICES=0,0,0,0"""
    t0 = time.monotonic()
    r, tail = _child("the queue-mode tests on four shards", [sys.executable, "-m", "pytest", "tests/test_gpu_shim_api.py", "-m", "gpu", "-k", "queue_mode", "-q"],
                     {"MBX_DEVICES": "0,0,0,0"}, 600, cwd=ROOT)
    print(f"the queue-mode tests on four shards took {time.monotonic() - t0:.1f} s")
    assert r.returncode == 0, tail
    summary = r.stdout.strip().splitlines()[-1]
    assert re.search(r"\b5 passed\b", summary) and not re.search(r"failed|error|skipped", summary), tail
