"""Rainbow acting on the device (GPU): mg_rainbow_forward and mg_rollout_rainbow against the tests' own
restatement (tests/rainbow_ref.py: the C oracle's MFMA chains in the packed k order, the plain-C head) bit for
bit, the fused rollout against the same steps composed from RainbowNet.forward and MergeVecEnv.step, and its
transitions against the C oracle."""

import ctypes

import numpy as np
import pytest

import merge_oracle as mo
import params_cases as pc
import rainbow_ref as R

pytestmark = pytest.mark.gpu

OBS_TOL = dict(rtol=1e-6, atol=1e-5)  # one fp32 rounding of the oracle's fp64 values (tests/test_gpu_qnet.py)
NETS = {"default": (3, False), "soft": (1, True)}  # (seed, soft) of the recorded nets used here
SIZES = [1, 15, 16, 17, 63, 64, 65, 577]  # the tile edges of 16 and 64, a ragged tail over three blocks
SENTINEL = -12345.0


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def nets(torch):
    from merging_gym.rainbow import RainbowNet

    return {k: RainbowNet.from_state_dict(R.state_dict(seed, soft), device="cuda:0") for k, (seed, soft) in NETS.items()}


def _rows(n):
    """n fixture observations spread over the whole recorded trajectory."""
    return np.linspace(0, len(R.observations()) - 1, n).astype(np.int64)


@pytest.mark.parametrize("rotate", [0, 3])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("fam", ["default", "soft"])
def test_forward_equals_the_restatement_bit_for_bit(torch, nets, fam, n, rotate):
    seed, soft = NETS[fam]
    idx = _rows(n)
    lg_ref, q_ref, a_ref = (a[idx] for a in R.forward_fixture(seed, soft, rotate))
    obs = torch.from_numpy(R.observations()[idx]).to("cuda:0")
    q, act, lg = nets[fam].forward(obs, rotate=rotate, logits=True)
    np.testing.assert_array_equal(R.bits(lg.cpu().numpy()), R.bits(lg_ref))
    np.testing.assert_array_equal(R.bits(q.cpu().numpy()), R.bits(q_ref))
    np.testing.assert_array_equal(act.cpu().numpy(), a_ref)


@pytest.mark.parametrize("n", [17, 577])
def test_forward_writes_only_what_was_requested(torch, nets, n):
    """Each output alone gives the bits of the call with all three, a NULL output is accepted, and no
    output is written past row n."""
    from merging_gym import _native

    net = nets["soft"]
    obs = torch.from_numpy(R.observations()[_rows(n)]).to("cuda:0")
    q_all, a_all, lg_all = net.forward(obs, rotate=3, logits=True)
    pad = 64
    bufs = {"logits": torch.full((n + pad, R.LOGITS), SENTINEL, device="cuda:0"),
            "q": torch.full((n + pad, R.ACTIONS), SENTINEL, device="cuda:0"),
            "action": torch.full((n + pad,), 99, dtype=torch.int8, device="cuda:0")}
    want = {"logits": lg_all, "q": q_all, "action": a_all}
    for only in ("logits", "q", "action"):
        for b in bufs.values():
            b.fill_(99 if b.dtype == torch.int8 else SENTINEL)
        ptr = {k: (bufs[k].data_ptr() if k == only else None) for k in bufs}
        _native.check(_native.lib.mg_rainbow_forward(net.packed.data_ptr(), obs.data_ptr(), 3, ptr["logits"], ptr["q"],
                                                     ptr["action"], n, None), "mg_rainbow_forward")
        torch.cuda.synchronize()
        assert torch.equal(bufs[only][:n], want[only]), only
        for k, b in bufs.items():
            fresh = 99 if b.dtype == torch.int8 else SENTINEL
            assert bool((b[n:] == fresh).all()), (only, k)
            if k != only:
                assert bool((b == fresh).all()), (only, k)


def _warmup_steps(coracle, n, seed, horizon=10):
    """The warm-up length, chosen with the C oracle on the CPU: the multiple of `horizon` random-play steps
    after which the most episodes end inside the next `horizon` steps (of random play; the test then asserts
    what the policy itself finished)."""
    envs = coracle.new_envs(n)
    coracle.reset(envs)
    ret_sum, counts = mo.new_stats(n)
    ends, k = [], 0
    for _ in range(40):
        before = int(counts[:, 0].sum())
        coracle.rollout_random(envs, horizon, seed, k, True, stats=(ret_sum, counts))
        ends.append(int(counts[:, 0].sum()) - before)
        k += horizon
    return horizon * int(np.argmax(ends))


def _fresh_env(torch, coracle, n, case, seed):
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(n, device="cuda:0", won_mask=True)
    if case is None:
        env.rollout_random(_warmup_steps(coracle, n, seed), seed, first_step=0)
    else:
        pc.fill_native(env.params, case)
        env.reset()
        pc.load_scattered_device(env, case, np.random.default_rng(n))
    return env


STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf", "_ep_stats")


@pytest.mark.parametrize("opponent", ["none", "self"])
@pytest.mark.parametrize("n,case", [(577, None), (1000, None), (577, "A"), (17, "A"), (65, "A")])
def test_rollout_equals_composition_restatement_and_oracle(torch, coracle, nets, n, case, opponent):
    """Two consecutive launches of T = 5 (the state carried) on a mid-episode batch. (a) The launch equals,
    with torch.equal, the same steps composed from RainbowNet.forward (rotate 0 and 3) and MergeVecEnv.step;
    (b) every action is the restatement's choice on the observation the kernel acted on; (c) the C oracle's
    step on those actions gives the flags and the fp64 state bit for bit and the observations after one fp32
    rounding; (d) a second run from the same state gives identical outputs. (17, "A") and (65, "A"): below and
    just past one wave, from case A's scattered states; two of the 17 end an episode inside the ten steps."""
    T, launches, seed = 5, 2, 11
    net = nets["default"]
    eff = R.effective_ref(R.state_dict(*NETS["default"]))
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
        traj = {k: (v.clone() if v is not None else None) for k, v in env.rollout_rainbow(T, net, opponent=opponent).items()}
        rerun = again.rollout_rainbow(T, net, opponent=opponent)
        for k, v in traj.items():
            if v is not None:
                eq = torch.equal(torch.nan_to_num(v, nan=7.0), torch.nan_to_num(rerun[k], nan=7.0)) if v.is_floating_point() \
                    else torch.equal(v, rerun[k])
                assert eq, ("rerun", k)
        for t in range(T):
            # (a) the composition
            a1 = net.act(obs_in, rotate=0)
            a2 = net.act(obs_in, rotate=3) if opponent == "self" else None
            c_obs, c_rew, c_done, c_info = twin.step(a1, a2)
            assert torch.equal(traj["a1"][t], a1), (launch, t)
            assert torch.equal(traj["a2"][t], a2 if a2 is not None else torch.full_like(a1, -1)), (launch, t)
            assert torch.equal(traj["obs"][t], c_obs), (launch, t)
            assert torch.equal(traj["rew"][t], c_rew), (launch, t)
            assert torch.equal(traj["done"][t], c_done), (launch, t)
            assert torch.equal(traj["collision"][t], c_info["collision"]), (launch, t)
            d = c_done
            assert torch.equal(traj["final_observation"][t][d], c_info["final_observation"][d]), (launch, t)
            assert torch.equal(traj["won_mask"][t], twin.won_mask), (launch, t)
            # (b) the restatement on the observation the kernel acted on
            x = obs_in.cpu().numpy()
            np.testing.assert_array_equal(traj["a1"][t].cpu().numpy(), R.forward_ref(eff, x, 0)[2], err_msg=f"{launch} {t}")
            if opponent == "self":
                np.testing.assert_array_equal(traj["a2"][t].cpu().numpy(), R.forward_ref(eff, x, 3)[2])
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
        # the state and the episode statistics after the launch
        for name in STATE:
            assert torch.equal(getattr(env, name), getattr(twin, name)), (launch, name)
            assert torch.equal(getattr(env, name), getattr(again, name)), (launch, "rerun", name)
        for name, key in (("p1", "pos1"), ("v1", "vel1"), ("p2", "pos2"), ("v2", "vel2"), ("ret1", "r1_acc"),
                          ("ret2", "r2_acc")):
            np.testing.assert_array_equal(getattr(env, name).cpu().numpy(), envs[key], err_msg=name)
        np.testing.assert_array_equal(env.steps.cpu().numpy(), envs["steps"])
        np.testing.assert_array_equal(env.winner.cpu().numpy(), envs["winner"])
    assert finished >= 1, "no env finished and was reset inside the checked steps"
    assert bool((env.q_eval == 0).all())  # the script logs no q_eval: left unchanged


def test_rollout_refuses_what_it_cannot_run(torch, nets):
    from merging_gym import MergeVecEnv, _native

    env = MergeVecEnv(64, device="cuda:0")
    buf = env._traj(2, True, True)
    rc = _native.lib.mg_rollout_rainbow(env._p_ref, env._s_ref, ctypes.byref(buf["_traj"]), env._st_ref, 64, 2,
                                        nets["default"].packed.data_ptr(), 1, env._flags, None)
    assert rc != 0 and b"opponent_mode must be 0 (None) or 2" in _native.lib.mg_last_error()
    with pytest.raises(KeyError):
        env.rollout_rainbow(2, nets["default"], opponent="uniform")
