"""MergeVecEnv.rollout_rainbow(T, net, opponent=<another RainbowNet>) (mg_rollout_rainbow_vs, rainbow_rollout_kernel's
OPP 3 instance): the ego acts with its net on the state, the opponent with ITS net on state[3:] + state[:3].

The launch against the same steps composed from RainbowNet.act (rotate 0 with the ego, rotate 3 with the opponent)
and MergeVecEnv.step with torch.equal, every action against the tests' restatement of the forward, its transitions
against the C oracle. The ego is the recorded net of seed 3 (it picks actions 0 / 1) and the opponent the soft net
of seed 1 (always action 4), so the two never agree and a kernel that forwards the ego's net twice, or swaps the
two, cannot pass.
"""

import ctypes

import numpy as np
import pytest

import merge_oracle as mo
import params_cases as pc
import rainbow_ref as R
from test_gpu_rainbow import OBS_TOL, STATE, _fresh_env

pytestmark = pytest.mark.gpu

EGO, OPP = (3, False), (1, True)  # (seed, soft) of the recorded nets


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def ego(torch):
    from merging_gym.rainbow import RainbowNet

    return RainbowNet.from_state_dict(R.state_dict(*EGO), device="cuda:0")


@pytest.fixture(scope="module")
def opp(torch):
    from merging_gym.rainbow import RainbowNet

    return RainbowNet.from_state_dict(R.state_dict(*OPP), device="cuda:0")


def _same(torch, a, b):
    if a.is_floating_point():
        a, b = torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)
    return torch.equal(a, b)


@pytest.mark.parametrize("n,case", [(17, "A"), (65, "A"), (577, None)])
def test_rollout_vs_equals_composition_restatement_and_oracle(torch, coracle, ego, opp, n, case):
    """Two consecutive launches of T = 5 (the state carried): below one wave, just past one wave, two blocks with
    a partial last wave. (a) The launch equals the composition ego.act(obs, 0), opp.act(obs, 3), twin.step; (b)
    a1 / a2 are the restatement's choices with the ego's / the opponent's effective weights; (c) the C oracle's
    step on those actions gives the flags and the fp64 state bit for bit, the observations after one fp32
    rounding; (d) a rerun from the same state gives identical outputs. An episode ends inside the checked steps,
    and on the first step a2 differs from what the ego's own net would have chosen on the rotated view."""
    T, launches, seed = 5, 2, 11
    eff_ego, eff_opp = R.effective_ref(R.state_dict(*EGO)), R.effective_ref(R.state_dict(*OPP))
    params = None if case is None else pc.CASES[case]
    env = _fresh_env(torch, coracle, n, case, seed)      # the fused launches
    twin = _fresh_env(torch, coracle, n, case, seed)     # the composition
    again = _fresh_env(torch, coracle, n, case, seed)    # the fused launches once more
    for name in STATE:
        assert torch.equal(getattr(env, name), getattr(twin, name)), name
    envs = mo.oracle_envs_from(coracle, env, params=params)
    obs_in = env.observe().clone()
    assert torch.equal(obs_in, twin.observe())
    finished = 0
    for launch in range(launches):
        traj = {k: (v.clone() if v is not None else None) for k, v in env.rollout_rainbow(T, ego, opponent=opp).items()}
        rerun = again.rollout_rainbow(T, ego, opponent=opp)
        for k, v in traj.items():
            if v is not None:
                assert _same(torch, v, rerun[k]), ("rerun", k)
        for t in range(T):
            # (a) the composition
            a1 = ego.act(obs_in, rotate=0)
            a2 = opp.act(obs_in, rotate=3)
            if launch == 0 and t == 0:
                assert not torch.equal(a2, ego.act(obs_in, rotate=3)), "the two nets agree: the test shows nothing"
            c_obs, c_rew, c_done, c_info = twin.step(a1, a2)
            assert torch.equal(traj["a1"][t], a1), (launch, t)
            assert torch.equal(traj["a2"][t], a2), (launch, t)
            assert torch.equal(traj["obs"][t], c_obs), (launch, t)
            assert torch.equal(traj["rew"][t], c_rew), (launch, t)
            assert torch.equal(traj["done"][t], c_done), (launch, t)
            assert torch.equal(traj["collision"][t], c_info["collision"]), (launch, t)
            d = c_done
            assert torch.equal(traj["final_observation"][t][d], c_info["final_observation"][d]), (launch, t)
            assert torch.equal(traj["won_mask"][t], twin.won_mask), (launch, t)
            # (b) the restatement on the observation the kernel acted on
            x = obs_in.cpu().numpy()
            np.testing.assert_array_equal(traj["a1"][t].cpu().numpy(), R.forward_ref(eff_ego, x, 0)[2],
                                          err_msg=f"{launch} {t}")
            np.testing.assert_array_equal(traj["a2"][t].cpu().numpy(), R.forward_ref(eff_opp, x, 3)[2],
                                          err_msg=f"{launch} {t}")
            # (c) the C oracle on the actions taken
            o_obs, o_rew, o_done, o_coll, _, o_fobs, err = coracle.step(
                envs, traj["a1"][t].cpu().numpy(), traj["a2"][t].cpu().numpy(), autoreset=True, final_obs=True,
                params=params)
            assert err == 0
            np.testing.assert_array_equal(traj["done"][t].cpu().numpy(), o_done.astype(bool))
            np.testing.assert_array_equal(traj["collision"][t].cpu().numpy(), o_coll.astype(bool))
            np.testing.assert_allclose(traj["obs"][t].cpu().numpy(), o_obs.astype(np.float32), **OBS_TOL)
            np.testing.assert_allclose(traj["rew"][t].cpu().numpy(), o_rew.astype(np.float32), **OBS_TOL)
            dn = o_done.astype(bool)
            np.testing.assert_allclose(traj["final_observation"][t].cpu().numpy()[dn], o_fobs[dn].astype(np.float32),
                                       **OBS_TOL)
            finished += int(dn.sum())
            obs_in = traj["obs"][t]
        # the state and the episode records after the launch
        for name in STATE:
            assert torch.equal(getattr(env, name), getattr(twin, name)), (launch, name)
            assert torch.equal(getattr(env, name), getattr(again, name)), (launch, "rerun", name)
        for name, key in (("p1", "pos1"), ("v1", "vel1"), ("p2", "pos2"), ("v2", "vel2"), ("ret1", "r1_acc"),
                          ("ret2", "r2_acc")):
            np.testing.assert_array_equal(getattr(env, name).cpu().numpy(), envs[key], err_msg=name)
        np.testing.assert_array_equal(env.steps.cpu().numpy(), envs["steps"])
        np.testing.assert_array_equal(env.winner.cpu().numpy(), envs["winner"])
    assert finished >= 1, "no env finished and was reset inside the checked steps"


def _pair(torch, coracle, n=65):
    return _fresh_env(torch, coracle, n, "A", 11), _fresh_env(torch, coracle, n, "A", 11)


def test_the_ego_as_its_own_opponent_is_self_play_bit_for_bit(torch, coracle, ego):
    """opponent=<the ego's RainbowNet> goes through mg_rollout_rainbow_vs and gives what opponent="self" gives."""
    vs, own = _pair(torch, coracle)
    got = vs.rollout_rainbow(6, ego, opponent=ego)
    want = own.rollout_rainbow(6, ego, opponent="self")
    assert bool(want["done"].any())
    for k, v in want.items():
        assert (v is None) == (got[k] is None), k
        if v is not None:
            assert _same(torch, got[k], v), k
    for name in STATE:
        assert torch.equal(getattr(vs, name), getattr(own, name)), name


def test_swapping_the_roles_swaps_the_actions(torch, coracle, ego, opp):
    """Which net is the ego: rollout_rainbow(T, opp, opponent=ego) acts otherwise than the unswapped call."""
    a, b = _pair(torch, coracle)
    plain = a.rollout_rainbow(6, ego, opponent=opp)
    swapped = b.rollout_rainbow(6, opp, opponent=ego)
    assert not torch.equal(plain["a1"], swapped["a1"])
    obs0 = _fresh_env(torch, coracle, 65, "A", 11).observe()
    assert torch.equal(plain["a1"][0], ego.act(obs0, rotate=0)) and torch.equal(plain["a2"][0], opp.act(obs0, rotate=3))
    assert torch.equal(swapped["a1"][0], opp.act(obs0, rotate=0))
    assert torch.equal(swapped["a2"][0], ego.act(obs0, rotate=3))


def test_refusals(torch, ego):
    from merging_gym import MergeVecEnv, _native

    env = MergeVecEnv(64, device="cuda:0")
    buf = env._traj(2, True, True)
    rc = _native.lib.mg_rollout_rainbow_vs(env._p_ref, env._s_ref, ctypes.byref(buf["_traj"]), env._st_ref, 64, 2,
                                           ego.packed.data_ptr(), None, env._flags, None)
    assert rc != 0 and _native.lib.mg_last_error().startswith(b"mg_rollout_rainbow_vs: opponent must be")
    with pytest.raises(KeyError):
        env.rollout_rainbow(2, ego, opponent="uniform")
