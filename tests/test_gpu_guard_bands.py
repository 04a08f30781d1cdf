"""Nothing a rollout kernel writes lands outside its buffers (GPU): every trajectory and h-DQN output sits between
two 4-KiB bands of byte 0xA5 (tests/guard_bands.py), and after a launch the bands are intact, the
final_observation rows of steps that ended no episode still hold their prefill, the mask words carry no bit at or
past n, and every tensor equals -- torch.equal -- that of an unguarded twin env run from the same state.

Sizes: one env, one wave and a lane (65), one 512-env group / block and an env (513); T = 1 and 3. Every clock is at
most two steps short of the timeout, so steps that end an episode and steps that do not are both in every run
longer than one env-step.
"""

import os

import numpy as np
import pytest

import guard_bands as gb
from conftest import ROOT

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
KERNELS = ["random", "qnet-none", "qnet-uniform", "qnet-self", "qnet-other", "hdqn-none", "hdqn-self", "rainbow-none",
           "rainbow-self"]
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf", "_ep_stats")


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def nets(torch):
    import rainbow_ref as R
    from merging_gym.policy import NUM_GOALS, QNet
    from merging_gym.rainbow import RainbowNet
    from test_gpu_hdqn import _net

    f = np.load(os.path.join(ROOT, "tests", "golden", "dqn_checkpoints.npz"))
    out = {key: QNet.from_state_dict({name.split("/", 1)[1]: f[name] for name in f.files if name.startswith(key + "/")},
                                     device=DEV) for key in ("l1", "l3")}
    rng = np.random.default_rng(21)
    out["meta"] = QNet.from_state_dict(_net(rng, 10, NUM_GOALS), device=DEV)
    out["lower"] = QNet.from_state_dict(_net(rng, 11, 5), device=DEV)
    out["rainbow"] = RainbowNet.from_state_dict(R.state_dict(3, False), device=DEV)
    return out


def _env(torch, n):
    """n envs after 20 random steps, the clocks of the even ones at the step that times out and of the odd ones one
    step before it (timeout_steps = 2,501: the step acting at 2,500 ends the episode)."""
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(n, device=DEV)
    env.rollout_random(20, 3, first_step=0)
    clock = (2500 - torch.arange(n, device=DEV) % 2).to(torch.int16)
    env.tf.copy_((env.tf & ~env._nat.TF_STEPS_MASK) | clock)
    return env


def _launch(env, kind, T, nets, ring, **outputs):
    fam, _, opponent = kind.partition("-")
    if fam == "random":
        return env.rollout_random(T, 5, first_step=101, **outputs)
    if fam == "qnet":
        return env.rollout_qnet(T, nets["l1"], 5, opponent=nets["l3"] if opponent == "other" else opponent,
                                first_step=101, **outputs)
    if fam == "hdqn":
        return env.rollout_hdqn(T, nets["meta"], nets["lower"], 5, opponent=opponent, first_step=101, ring=ring,
                                goal_memory=True, **outputs)
    return env.rollout_rainbow(T, nets["rainbow"], opponent=opponent, **outputs)


def _run(torch, nets, kind, n, T, final_observation=True, won_mask=True):
    from merging_gym import ReplayRing

    hdqn = kind.startswith("hdqn")
    env, twin = _env(torch, n), _env(torch, n)
    for name in STATE:
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    # the fused goal ring: 7 rows, fewer than one step of 65 envs stores
    ring, ring_t = (ReplayRing(7, device=DEV, goal=True), ReplayRing(7, device=DEV, goal=True)) if hdqn else (None, None)
    g = gb.install(env, T, final_observation, won_mask, hdqn=hdqn)
    outputs = dict(final_observation=final_observation, won_mask=won_mask)
    out = _launch(env, kind, T, nets, ring, **outputs)
    ref = _launch(twin, kind, T, nets, ring_t, **outputs)
    torch.cuda.synchronize()
    assert out["flags"].data_ptr() == g.raw["flags"][0].data_ptr() + gb.BAND  # the launch wrote the guarded buffers
    if hdqn:
        assert out["goal"].data_ptr() == g.raw["goal"][0].data_ptr() + gb.BAND
    g.assert_bands_intact()
    done = out["done"]
    assert bool(done.any()) and (n * T == 1 or not bool(done.all()))
    if final_observation:
        fo = out["final_observation"].view(torch.int32)
        assert torch.equal(fo[~done], gb.prefill_bits(torch, out["final_observation"])[~done])
        assert torch.equal(fo[done], ref["final_observation"].view(torch.int32)[done])
    else:
        assert out["final_observation"] is None and ref["final_observation"] is None
    for key in ("won_mask", "no_break"):
        if out.get(key) is not None:
            gb.assert_no_bits_past_n(out[key], n)
    assert (out["won_mask"] is None) == (not won_mask)
    assert set(out) == set(ref)
    for key, v in ref.items():
        if v is not None and key != "final_observation":
            assert torch.equal(out[key], v), key
    for name in STATE + (("hdqn_goal", "hdqn_ext") if hdqn else ()) + (("hdqn_goal_op",) if kind == "hdqn-self" else ()):
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    if hdqn:
        assert ring.memory_counter == ring_t.memory_counter == n * T
        assert torch.equal(ring.memory, ring_t.memory)


@pytest.mark.parametrize("T", [1, 3])
@pytest.mark.parametrize("n", [1, 65, 513])
@pytest.mark.parametrize("kind", KERNELS)
def test_rollout_writes_stay_inside_their_buffers(torch, nets, kind, n, T):
    _run(torch, nets, kind, n, T)


@pytest.mark.parametrize("kind", ["random", "qnet-self", "hdqn-self", "rainbow-self"])
def test_rollout_without_the_optional_outputs(torch, nets, kind):
    """final_observation and won_mask off (NULL in mg_traj): the rest is still right and nothing is written around it."""
    _run(torch, nets, kind, 65, 3, final_observation=False, won_mask=False)
