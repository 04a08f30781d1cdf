"""MergeVecEnv.rollout_rainbow_many(T, nets, opponent=<a list of RainbowNets>) (mg_rollout_rainbow_vs_many,
rainbow_rollout_kernel's <3, MANY> instance): every member's slice of every output is bit for bit what a lone
MergeVecEnv(n_member).rollout_rainbow(T, nets[m], opponent=opponents[m]) gives from the slice's state --
observations, rewards, the flag bytes, final observations, the member's won-mask words, the env state and the
episode records.

Member m plays against the next member's net, opponents[m] = nets[(m + 1) % M], and member 0's opponent actions
under nets[1] differ from those under its own net, so a wrong member -> opponent mapping (or the ego's net forwarded
twice) cannot pass. The batch is test_gpu_rainbow_rollout_many's: params case "A", scattered mid-episode states, two
envs of every slice about to time out, so episodes end inside every member's rollout whatever the nets do.
"""
import pytest

from test_gpu_rainbow_rollout_many import SHAPES, STATE, _batch_env, _env, _same
from test_gpu_rainbow_rollout_many import nets, torch  # noqa: F401  (module-scoped fixtures)

pytestmark = pytest.mark.gpu


def _check(torch, nets, M, n_member, T, final_observation=True, won_mask=True):  # noqa: F811
    opps = [nets[(m + 1) % M] for m in range(M)]
    env = _batch_env(torch, M, n_member)
    start = {name: getattr(env, name).clone() for name in STATE}
    traj = env.rollout_rainbow_many(T, nets[:M], opps, final_observation=final_observation, won_mask=won_mask)
    assert (traj["final_observation"] is None) == (not final_observation)
    assert (traj["won_mask"] is None) == (not won_mask)
    words = n_member // 64

    def lone_run(m, net, opp):
        lone = _env(n_member)
        sl = slice(m * n_member, (m + 1) * n_member)
        for name in STATE:
            getattr(lone, name).copy_(start[name][sl])
        return lone, lone.rollout_rainbow(T, net, opp, final_observation=final_observation, won_mask=won_mask)

    for m in range(M):
        sl = slice(m * n_member, (m + 1) * n_member)
        lone, want = lone_run(m, nets[m], opps[m])
        assert bool(want["done"].any()), f"member {m}: no episode ended inside its lone rollout"
        for k in ("obs", "rew", "flags", "done", "collision", "a1", "a2", "final_observation"):
            if want[k] is not None:
                assert _same(torch, traj[k][:, sl], want[k]), (m, k)
        if won_mask:
            assert torch.equal(traj["won_mask"][:, m * words:(m + 1) * words], want["won_mask"]), (m, "won_mask")
        for name in STATE:
            assert torch.equal(getattr(env, name)[sl], getattr(lone, name)), (m, name)
    if M > 1:  # member 0 against its own net is answered differently: the mapping member -> opponent is seen
        _, own = lone_run(0, nets[0], nets[0])
        assert not torch.equal(own["a2"], traj["a2"][:, :n_member])


@pytest.mark.parametrize("T", [1, 6])
@pytest.mark.parametrize("M,n_member", SHAPES)
def test_every_member_slice_equals_its_lone_rollout_vs(torch, nets, M, n_member, T):  # noqa: F811
    _check(torch, nets, M, n_member, T)


def test_vs_without_final_observation_and_won_mask(torch, nets):  # noqa: F811
    _check(torch, nets, 2, 576, 6, final_observation=False, won_mask=False)


def test_python_refuses_a_wrong_opponent_list_and_member_index(torch, nets):  # noqa: F811
    from merging_gym.rainbow_learn import RainbowReplay
    from merging_gym.rainbow_population import RainbowPopulation

    env = _env(3 * 64)
    with pytest.raises(ValueError, match="3 nets need 3 opponents"):
        env.rollout_rainbow_many(2, nets[:3], opponent=nets[:2])
    with pytest.raises(KeyError):
        env.rollout_rainbow_many(2, nets[:3], opponent="uniform")
    pop = RainbowPopulation(nets[:3], [RainbowReplay(300, device="cuda:0") for _ in range(3)], seed=range(3))
    for bad in ([1, 2, 3], [1, -1, 0], [1, 2], [1, 2, 1.0]):
        with pytest.raises(ValueError, match="opponent"):
            pop.collect(env, 2, opponent=bad)
