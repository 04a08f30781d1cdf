"""DQNPopulation.collect: the acting half of the population's loop -- one rollout_qnet_many and one
store_rollout_many for all members -- alternated with learn(), against M lone (MergeVecEnv with env_offset,
ReplayRing, DQNLearner) loops: the learners' state, the rings and the env slices bit for bit, and twice."""

import numpy as np
import pytest

import learn_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N_MEMBER, CAP, BATCH, ITERS = 3, 64, 2000, 32, 3
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf")
KW = [dict(lr=0.01, gamma=0.9, seed=11), dict(lr=0.005, gamma=0.95, seed=12), dict(lr=0.02, gamma=0.8, seed=13)]
EPS, OPP_EPS = [0.7, 0.2, 1.5], [0.7, 0.7, -0.3]


def _start():
    """The batch after 50 random steps: the state every run starts from."""
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(M * N_MEMBER, device=DEV)
    for k in range(50):
        env.step_random(3, step_idx=k)
    return {k: getattr(env, k).clone() for k in STATE}, env._ep_stats.clone(), env._step_idx


def _load(env, start, lo, hi):
    state, stats, step_idx = start
    for k in STATE:
        getattr(env, k).copy_(state[k][lo:hi])
    env._ep_stats.copy_(stats[lo:hi])
    env._step_idx = step_idx


def _bytes(t):
    return t.contiguous().cpu().numpy().tobytes()


def _run_population(start, nets, opponent):
    from merging_gym import DQNPopulation, MergeVecEnv, ReplayRing

    env = MergeVecEnv(M * N_MEMBER, device=DEV)
    _load(env, start, 0, M * N_MEMBER)
    rings = [ReplayRing(CAP, device=DEV) for _ in range(M)]
    pop = DQNPopulation(nets, rings, batch_size=BATCH, lr=[k["lr"] for k in KW], gamma=[k["gamma"] for k in KW],
                        seed=[k["seed"] for k in KW])
    for _ in range(ITERS):
        traj = pop.collect(env, 8, opponent=opponent, episilo=EPS, opp_episilo=OPP_EPS)
        assert tuple(traj["a1"].shape) == (8, M * N_MEMBER)
        pop.learn(2, filled_only=True)
    return pop, rings, env


@pytest.mark.parametrize("opponent", ["none", "self"])
def test_collect_and_learn_equal_the_lone_loops(opponent):
    from merging_gym import DQNLearner, MergeVecEnv, ReplayRing

    start = _start()
    nets = [lr.seeded_net(10, 5, 40 + m) for m in range(M)]
    pop, rings, env = _run_population(start, nets, opponent)
    assert env._step_idx == start[2] + 8 * ITERS
    assert pop.learn_step_counter == [2 * ITERS] * M
    for m in range(M):
        lo, hi = m * N_MEMBER, (m + 1) * N_MEMBER
        lone_env = MergeVecEnv(N_MEMBER, device=DEV, env_offset=lo)
        _load(lone_env, start, lo, hi)
        ring = ReplayRing(CAP, device=DEV)
        learner = DQNLearner(nets[m], ring, batch_size=BATCH, lr=KW[m]["lr"], gamma=KW[m]["gamma"], seed=KW[m]["seed"])
        for _ in range(ITERS):
            obs0 = lone_env.observe().clone()
            traj = lone_env.rollout_qnet(8, learner.qnet, KW[m]["seed"], opponent=opponent, episilo=EPS[m],
                                         opp_episilo=OPP_EPS[m])
            ring.store_rollout(obs0, traj)
            learner.learn(2, filled_only=True)
        got, want = pop.member_state_dict(m), learner.state_dict()
        assert set(got) == set(want)
        for k in want:
            if k == "learner":
                assert _bytes(got[k]) == _bytes(want[k]), f"member {m}: learner state"
            else:
                assert got[k] == want[k], (m, k)
        assert _bytes(pop.qnets[m].packed) == _bytes(learner.qnet.packed)
        assert int(rings[m]._counter.item()) == int(ring._counter.item()) > 0
        assert _bytes(rings[m].memory) == _bytes(ring.memory), f"member {m}: ring"
        for k in STATE:
            assert _bytes(getattr(env, k)[lo:hi]) == _bytes(getattr(lone_env, k)), (m, k)
        assert _bytes(env._ep_stats[lo:hi]) == _bytes(lone_env._ep_stats), f"member {m}: records"
    # the same run again: the same bytes
    pop2, rings2, env2 = _run_population(start, nets, opponent)
    assert _bytes(pop2._buf) == _bytes(pop._buf)
    for m in range(M):
        assert _bytes(rings2[m].memory) == _bytes(rings[m].memory) and _bytes(rings2[m]._counter) == _bytes(rings[m]._counter)
    for k in STATE:
        assert _bytes(getattr(env2, k)) == _bytes(getattr(env, k)), k


def test_collect_refuses_shared_rings():
    from merging_gym import DQNPopulation, MergeVecEnv, ReplayRing

    ring = ReplayRing(CAP, device=DEV)
    pop = DQNPopulation([lr.seeded_net(10, 5, 1)] * 2, [ring, ring], batch_size=BATCH)
    with pytest.raises(ValueError, match="rings are shared"):
        pop.collect(MergeVecEnv(128, device=DEV), 4)
