"""RainbowPopulation.collect / PrioritizedRainbowPopulation.collect with an opponent per member
(mg_rollout_rainbow_vs_many): three members of 64 envs, opponents [1, 2, a frozen RainbowNet] -- member 0 against
member 1's current acting net, member 1 against member 2's, member 2 against a checkpoint -- alternated with
learn(2), against the lone loops in lock-step (rollout_rainbow(T, learner.net, opponent=<the opponent's net>),
store_rollout and learn per member): the replays' contents (and trees), the counters, the learners' state, the
nets' packed bytes and the env slices bit for bit. Capacity 300 < 6 x 64, so the rings wrap in every collect. The
second round runs after learn(): an index names the member's CURRENT acting net, so member 0's opponent actions are
those of member 1's updated net."""

import pytest

import rainbow_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N_MEMBER, BATCH, T, CAPACITY, ROUNDS = 3, 64, 32, 6, 300, 2
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf")
NETS = ((3, False), (1, True), (2, False))  # (seed, soft) of the recorded nets: three different actors
FROZEN = (3, True)
KW = [dict(lr=0.001, gamma=0.99, seed=11, noise_seed=21), dict(lr=0.002, gamma=0.95, seed=12, noise_seed=22),
      dict(lr=0.0005, gamma=0.9, seed=13, noise_seed=23)]
ALPHAS, BETAS, PRIO_EPS = (0.6, 1.0, 0.4), (0.4, 1.0, 0.7), (1e-5, 1e-3, 0.0)


@pytest.fixture(scope="module")
def start():
    """The batch after 50 random steps: the state every run starts from."""
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(M * N_MEMBER, device=DEV)
    for k in range(50):
        env.step_random(3, step_idx=k)
    return {k: getattr(env, k).clone() for k in STATE}, env._ep_stats.clone()


def _load(env, start, lo, hi):
    state, stats = start
    for k in STATE:
        getattr(env, k).copy_(state[k][lo:hi])
    env._ep_stats.copy_(stats[lo:hi])


def _bytes(t):
    return t.contiguous().cpu().numpy().tobytes()


def _nets():
    return [R.state_dict(seed, soft) for seed, soft in NETS]


def _build(prioritized):
    """(the population and its replays, the lone learners and their replays)."""
    import merging_gym as mg

    kws = {k: [kw[k] for kw in KW] for k in KW[0]}
    if prioritized:
        replays = [mg.PrioritizedRainbowReplay(CAPACITY, alpha=a, device=DEV) for a in ALPHAS]
        pop = mg.PrioritizedRainbowPopulation(_nets(), replays, batch_size=BATCH, beta=BETAS, prio_eps=PRIO_EPS, **kws)
        lone_replays = [mg.PrioritizedRainbowReplay(CAPACITY, alpha=a, device=DEV) for a in ALPHAS]
        learners = [mg.PrioritizedRainbowLearner(_nets()[m], lone_replays[m], lr=KW[m]["lr"], gamma=KW[m]["gamma"],
                                                 batch_size=BATCH, seed=KW[m]["seed"],
                                                 generator=mg.DeviceNoise(KW[m]["noise_seed"]), device=DEV,
                                                 beta=BETAS[m], prio_eps=PRIO_EPS[m]) for m in range(M)]
    else:
        replays = [mg.RainbowReplay(CAPACITY, device=DEV) for _ in range(M)]
        pop = mg.RainbowPopulation(_nets(), replays, batch_size=BATCH, **kws)
        lone_replays = [mg.RainbowReplay(CAPACITY, device=DEV) for _ in range(M)]
        learners = [mg.RainbowLearner(_nets()[m], lone_replays[m], lr=KW[m]["lr"], gamma=KW[m]["gamma"],
                                      batch_size=BATCH, seed=KW[m]["seed"],
                                      generator=mg.DeviceNoise(KW[m]["noise_seed"]), device=DEV) for m in range(M)]
    return pop, replays, learners, lone_replays


@pytest.mark.parametrize("prioritized", [False, True])
def test_cross_play_collect_and_learn_equal_the_lone_loops(start, prioritized):
    import torch

    from merging_gym import MergeVecEnv, RainbowNet

    frozen = RainbowNet.from_state_dict(R.state_dict(*FROZEN), device=DEV)
    pop, replays, learners, lone_replays = _build(prioritized)
    env = MergeVecEnv(M * N_MEMBER, device=DEV)
    _load(env, start, 0, M * N_MEMBER)
    lone_envs = [MergeVecEnv(N_MEMBER, device=DEV) for _ in range(M)]
    for m in range(M):
        _load(lone_envs[m], start, m * N_MEMBER, (m + 1) * N_MEMBER)
    first_packed = _bytes(pop.nets[1].packed)
    for rnd in range(ROUNDS):
        obs0 = env.observe().clone()
        # member 0's opponent on the first observation, from member 1's acting net as it is NOW
        a2_now = pop.nets[1].act(obs0[:N_MEMBER], rotate=3).clone()
        traj = pop.collect(env, T, opponent=[1, 2, frozen])
        assert tuple(traj["a1"].shape) == (T, M * N_MEMBER)
        assert torch.equal(traj["a2"][0, :N_MEMBER], a2_now), rnd
        assert torch.equal(traj["a2"][0, 2 * N_MEMBER:], frozen.act(obs0[2 * N_MEMBER:], rotate=3)), rnd
        # the lone loops: every member acts against its opponent's net of this round, then all learn
        lone_opp = [learners[1].net, learners[2].net, frozen]
        for m in range(M):
            lone_obs0 = lone_envs[m].observe().clone()
            lone_traj = lone_envs[m].rollout_rainbow(T, learners[m].net, opponent=lone_opp[m])
            sl = slice(m * N_MEMBER, (m + 1) * N_MEMBER)
            for k in ("a1", "a2", "obs", "rew", "done"):
                assert _bytes(traj[k][:, sl]) == _bytes(lone_traj[k]), (rnd, m, k)
            lone_replays[m].store_rollout(lone_obs0, lone_traj)
        pop.learn(2)
        for m in range(M):
            learners[m].learn(2)
        for m in range(M):
            lo, hi = m * N_MEMBER, (m + 1) * N_MEMBER
            got, want = pop.member_state_dict(m), learners[m].state_dict()
            assert set(got) == set(want)
            for k in want:
                assert (_bytes(got[k]) == _bytes(want[k])) if k == "learner" else got[k] == want[k], (rnd, m, k)
            assert _bytes(pop.nets[m].packed) == _bytes(learners[m].net.packed), f"round {rnd}, member {m}: packed net"
            assert (int(replays[m]._counter.item()) == int(lone_replays[m]._counter.item())
                    == (rnd + 1) * T * N_MEMBER)
            assert _bytes(replays[m].memory) == _bytes(lone_replays[m].memory), f"round {rnd}, member {m}: memory"
            if prioritized:
                assert _bytes(replays[m]._tree) == _bytes(lone_replays[m]._tree), f"round {rnd}, member {m}: tree"
                assert replays[m].max_priority == lone_replays[m].max_priority
            for k in STATE:
                assert _bytes(getattr(env, k)[lo:hi]) == _bytes(getattr(lone_envs[m], k)), (rnd, m, k)
            assert _bytes(env._ep_stats[lo:hi]) == _bytes(lone_envs[m]._ep_stats), f"round {rnd}, member {m}: records"
        assert pop.learn_step_counter == [2 * (rnd + 1)] * M
        # the second round's opponent of member 0 is another net than the first round's
        assert _bytes(pop.nets[1].packed) != first_packed
