"""Everything the library acquires on the GPU (device buffers, pinned host buffers, streams,
events) is held by an owner object and released with its handle: tg_live_resources(), the count
of those owners in the process, returns to its earlier value after tg_destroy, after a failed
tg_create and after a refused tg_set_groups.  Other tests' fixtures may hold handles, so every
check compares against the count at its own start (after a garbage collection, so that no
dropped handle of an earlier test is destroyed in between).  The default level throughout."""
import ctypes
import gc
import random

import numpy as np
import pytest
import torch

from test_gpu_parity import assert_bits, run_gpu
from test_policy_mlp_host import seeded_params

pytestmark = pytest.mark.gpu


def live(tg):
    return tg._lib.load().tg_live_resources()


@pytest.fixture
def base(tg):
    gc.collect()
    return live(tg)


def compact_rollout(vec, policy="uniform"):
    return vec.rollout(4, policy=policy, obs=False, actions=False)


def test_everything_a_handle_allocates_is_released(tg, base):
    """8,192 envs (the smallest batch two groups accept) with every lazily allocated resource
    driven once: the timing records, the obs scratch, two groups' steppers, streams and events,
    the flow structures, the actor's parameters and action scratch, the renderer's tables at
    full size and at one scale, a resized episode queue, read_state's staging buffer.  Twice."""
    sprites = tg.synthetic_sprites()
    params = tg.pack_mlp_params(seeded_params(16, 316))
    for cycle in range(2):
        vec = tg.TreasureGameVec(8192, seed=11, autoreset=True)
        held = live(tg) - base
        assert held > 0
        vec.reset()
        for t in range(2):
            vec.step(vec.policy_actions(t, policy="masked"))
        vec.set_timing(1)
        compact_rollout(vec)
        vec.set_groups(2)
        assert live(tg) - base > held  # the groups' steppers, streams and events
        compact_rollout(vec)
        vec.set_groups(1)
        vec.set_mode("flow")
        compact_rollout(vec)
        vec.set_mode("compact")
        vec.set_policy_mlp(params)
        compact_rollout(vec, "mlp")
        vec.render_init(sprites)
        assert vec.render(count=4).shape[0] == 4
        assert vec.render(count=4, scale=4, gray=True).shape[0] == 4
        vec.set_episode_capacity(1 << 12)
        vec.write_state(vec.read_state(mt=True))
        assert vec.stats()["timed_launches"] > 0
        assert vec.errors() == 0
        vec.close()
        assert live(tg) == base, cycle


def test_one_env_handle_releases_its_buffers_and_server(tg, base):
    """The N = 1 handle's own resources: the result row, the Python-stream state and cache, the
    server's mailbox, stream and events (a step starts it); with serving off, the pinned mask
    and the row again.  A shared-stream env is closed while its server is resident."""
    env = tg.TreasureGame(seed=3)
    env.step(0)
    mask = env.available_mask
    env.reset()
    env._vec.set_serve(False)
    env.step(1)
    assert env.available_mask is not None and mask is not None
    assert live(tg) > base
    env.close()
    assert live(tg) == base
    saved = random.getstate()
    try:
        env = tg.TreasureGame()  # draws from Python's global stream
        env.step(0)
        env.step(1)
        assert live(tg) > base
        env.close()  # (its server still resident)
    finally:
        random.setstate(saved)
    assert live(tg) == base


def test_a_failed_create_holds_nothing(tg, oracle, base):
    """tg_create of 2^40 envs: every per-env array is at least 8 TB, so an allocation fails
    whatever their order: TG_E_NOMEM, a null handle and nothing held; the library then works as
    before (256 envs' 8 masked steps equal the oracle's, bit for bit)."""
    L = tg._lib.load()
    h = ctypes.c_void_p()
    dev = torch.cuda.current_device()
    rc = L.tg_create(ctypes.byref(h), 2**40, 0, 0, dev, None, None, None)
    assert rc == tg._lib.TG_E_NOMEM, L.tg_last_error()
    assert not h.value
    assert live(tg) == base
    n, steps, a0 = 256, 8, 0x51
    got = run_gpu(tg, 0, 0, n, steps, a0, 1, False)
    ref = oracle.run(0, 0, n, steps, a0, 1, False)
    for key in ("obs", "reward", "valid", "done"):
        assert_bits(got[key], ref[key], key)
    np.testing.assert_array_equal(got["hash"], ref["hash"])
    assert got["errors"] == 0
    got["vec"].close()
    assert live(tg) == base


def test_a_refused_regrouping_changes_nothing(tg, base):
    """two groups need 8,192 envs: on 4,096 tg_set_groups returns TG_E_INVAL, the handle still
    steps and holds what it held"""
    vec = tg.TreasureGameVec(4096, seed=2, autoreset=True)
    vec.reset()
    held = live(tg)
    rc = tg._lib.load().tg_set_groups(vec.handle, 2, 0)
    assert rc == tg._lib.TG_E_INVAL
    assert live(tg) == held
    for t in range(2):
        vec.step(vec.policy_actions(t, policy="masked"))
    assert vec.stats()["steps"] == 2 * 4096 and vec.errors() == 0
    assert live(tg) == held
    vec.close()
    assert live(tg) == base
