"""MergeVecEnv.rollout_rainbow_many (mg_rollout_rainbow_many, rainbow_rollout_kernel's MANY instances): every
member's slice of every output is bit for bit what a lone MergeVecEnv(n_member).rollout_rainbow gives with the
member's net from the slice's state -- observations, rewards, the flag bytes, final observations, the member's
won-mask words, the env state and the episode records.

Every member has its own net, and member 0's lone actions under net 0 differ from those under net 1, so a wrong
member -> net mapping cannot pass. The batch starts from params case "A" with scattered mid-episode states, and in
every member's slice one env stands one step and one four steps before its timeout, so episodes end (and envs
reset) inside every member's rollout whatever its net does.
"""
import numpy as np
import pytest

import params_cases as pc
import rainbow_ref as R

pytestmark = pytest.mark.gpu

CASE = "A"
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf", "_ep_stats")
# (seed, soft) of the recorded nets: the first two act differently on every observation (seed 3 picks actions 0 / 1,
# seed 1 with linear1 / 1024 always action 4)
BASES = ((3, False), (1, True), (2, False), (1, False), (3, True), (2, True))
# (M, n_member): one live wave per block; two blocks per member, the second with one live wave, member 1 starting
# mid-block of the whole batch; the full member table; the lone call on the whole env
SHAPES = [(3, 64), (2, 576), (64, 64), (1, 1024)]


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


@pytest.fixture(scope="module")
def nets(torch):
    """64 distinct nets: the recorded ones, then the same with the noise of a counter-based stream per member."""
    from merging_gym.rainbow import RainbowNet

    out = []
    for m in range(64):
        seed, soft = BASES[m % len(BASES)]
        net = RainbowNet.from_state_dict(R.state_dict(seed, soft), device="cuda:0")
        if m >= len(BASES):
            net.reset_noise(seed=1000 + m)
        out.append(net)
    packed = [net.packed for net in out]
    for a in range(len(BASES) + 2):  # the recorded ones and the first redrawn ones really differ
        for b in range(a):
            assert not torch.equal(packed[a], packed[b]), (a, b)
    return out


def _env(n):
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(n, device="cuda:0", won_mask=True)
    pc.fill_native(env.params, CASE)
    env.reset()
    return env


def _batch_env(torch, M, n_member):
    """The whole batch in scattered states; env 1 and env 3 of every slice about to time out, from the start line."""
    env = _env(M * n_member)
    pc.load_scattered_device(env, CASE, np.random.default_rng(M * n_member))
    c = pc.CASES[CASE]
    tmo = pc.timeout_steps(float(c.dT), c.time_limit)
    for m in range(M):
        for j, left in ((1, 1), (3, 4)):
            i = m * n_member + j
            env.p1[i] = env.p2[i] = float(c.START_POINT)
            env.v1[i] = env.v2[i] = float(c.start_vel)
            env.tf[i] = tmo - left  # winner bits zero
    torch.cuda.synchronize()
    return env


def _same(torch, a, b):
    if a.is_floating_point():
        a, b = torch.nan_to_num(a, nan=7.0), torch.nan_to_num(b, nan=7.0)
    return torch.equal(a, b)


def _check(torch, nets, M, n_member, T, opponent, final_observation=True, won_mask=True):
    env = _batch_env(torch, M, n_member)
    start = {name: getattr(env, name).clone() for name in STATE}
    traj = env.rollout_rainbow_many(T, nets[:M], opponent, final_observation=final_observation, won_mask=won_mask)
    assert (traj["final_observation"] is None) == (not final_observation)
    assert (traj["won_mask"] is None) == (not won_mask)
    words = n_member // 64

    def lone_run(m, net):
        lone = _env(n_member)
        sl = slice(m * n_member, (m + 1) * n_member)
        for name in STATE:
            getattr(lone, name).copy_(start[name][sl])
        return lone, lone.rollout_rainbow(T, net, opponent, final_observation=final_observation, won_mask=won_mask)

    for m in range(M):
        sl = slice(m * n_member, (m + 1) * n_member)
        lone, want = lone_run(m, nets[m])
        assert bool(want["done"].any()), f"member {m}: no episode ended inside its lone rollout"
        for k in ("obs", "rew", "flags", "done", "collision", "a1", "a2", "final_observation"):
            if want[k] is not None:
                assert _same(torch, traj[k][:, sl], want[k]), (m, k)
        if won_mask:
            assert torch.equal(traj["won_mask"][:, m * words:(m + 1) * words], want["won_mask"]), (m, "won_mask")
        for name in STATE:
            assert torch.equal(getattr(env, name)[sl], getattr(lone, name)), (m, name)
    if M > 1:  # member 0 under member 1's net acts differently: the mapping member -> net is seen
        _, other = lone_run(0, nets[1])
        _, own = lone_run(0, nets[0])
        assert not torch.equal(own["a1"], other["a1"])
        assert torch.equal(traj["a1"][:, :n_member], own["a1"])


@pytest.mark.parametrize("opponent", ["none", "self"])
@pytest.mark.parametrize("T", [1, 6])
@pytest.mark.parametrize("M,n_member", SHAPES)
def test_every_member_slice_equals_its_lone_rollout(torch, nets, M, n_member, T, opponent):
    _check(torch, nets, M, n_member, T, opponent)


def test_without_final_observation_and_won_mask(torch, nets):
    _check(torch, nets, 2, 576, 6, "self", final_observation=False, won_mask=False)


def test_python_refuses_what_the_launch_cannot_take(torch, nets):
    env = _env(3 * 64)
    with pytest.raises(ValueError, match="1..64 nets"):
        env.rollout_rainbow_many(2, [])
    with pytest.raises(ValueError, match="slices of a multiple of 64"):
        env.rollout_rainbow_many(2, nets[:2])  # 96 envs per member
    with pytest.raises(KeyError):
        env.rollout_rainbow_many(2, nets[:3], opponent="uniform")
