"""RainbowPopulation.collect: the acting half of the Rainbow population's loop -- one rollout_rainbow_many and one
store_rainbow_rollout_many for all members -- alternated with learn(), against M lone loops (MergeVecEnv,
RainbowReplay, RainbowLearner with DeviceNoise; rollout_rainbow and store_rollout): the learners' state, the packed
nets, the replay memories and counters and the env slices and records bit for bit, and twice. Capacity 1,000 holds
a collect's 8 x 64 transitions; capacity 300 does not, so the member store's newest-rows rule and its wrap-around
run on the device."""

import pytest

import rainbow_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
M, N_MEMBER, BATCH, ITERS, T = 3, 64, 32, 3, 8
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf")
NETS = ((3, False), (1, True), (2, False))  # (seed, soft) of the recorded nets: three different actors
KW = [dict(lr=0.001, gamma=0.99, seed=11, noise_seed=21), dict(lr=0.002, gamma=0.95, seed=12, noise_seed=22),
      dict(lr=0.0005, gamma=0.9, seed=13, noise_seed=23)]


def _start():
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


def _run_population(start, capacity, opponent):
    from merging_gym import MergeVecEnv, RainbowPopulation, RainbowReplay

    env = MergeVecEnv(M * N_MEMBER, device=DEV)
    _load(env, start, 0, M * N_MEMBER)
    replays = [RainbowReplay(capacity, device=DEV) for _ in range(M)]
    pop = RainbowPopulation(_nets(), replays, batch_size=BATCH, **{k: [kw[k] for kw in KW] for k in KW[0]})
    for _ in range(ITERS):
        traj = pop.collect(env, T, opponent=opponent)
        assert tuple(traj["a1"].shape) == (T, M * N_MEMBER)
        pop.learn(2)
    return pop, replays, env


@pytest.mark.parametrize("capacity,opponent", [(1000, "self"), (300, "none")])
def test_collect_and_learn_equal_the_lone_loops(capacity, opponent):
    from merging_gym import DeviceNoise, MergeVecEnv, RainbowLearner, RainbowReplay

    start = _start()
    pop, replays, env = _run_population(start, capacity, opponent)
    assert pop.learn_step_counter == [2 * ITERS] * M
    whole = pop.state_dict()
    for m in range(M):
        lo, hi = m * N_MEMBER, (m + 1) * N_MEMBER
        lone_env = MergeVecEnv(N_MEMBER, device=DEV)
        _load(lone_env, start, lo, hi)
        replay = RainbowReplay(capacity, device=DEV)
        kw = KW[m]
        learner = RainbowLearner(_nets()[m], replay, lr=kw["lr"], gamma=kw["gamma"], batch_size=BATCH, seed=kw["seed"],
                                 generator=DeviceNoise(kw["noise_seed"]), device=DEV)
        for _ in range(ITERS):
            obs0 = lone_env.observe().clone()
            replay.store_rollout(obs0, lone_env.rollout_rainbow(T, learner.net, opponent=opponent))
            learner.learn(2)
        got, want = pop.member_state_dict(m), learner.state_dict()
        assert set(got) == set(want)
        for k in want:
            if k == "learner":
                assert _bytes(got[k]) == _bytes(want[k]), f"member {m}: learner state"
                assert _bytes(whole["learners"][m]) == _bytes(want[k]), f"member {m}: state_dict()"
            else:
                assert got[k] == want[k], (m, k)
        for k in ("learn_step_counter", "draw_counter", "seed", "noise_seed"):
            assert whole[k][m] == want[k], (m, k)
        assert _bytes(pop.nets[m].packed) == _bytes(learner.net.packed), f"member {m}: packed net"
        assert int(replays[m]._counter.item()) == int(replay._counter.item()) == ITERS * T * N_MEMBER
        assert _bytes(replays[m].memory) == _bytes(replay.memory), f"member {m}: replay memory"
        for k in STATE:
            assert _bytes(getattr(env, k)[lo:hi]) == _bytes(getattr(lone_env, k)), (m, k)
        assert _bytes(env._ep_stats[lo:hi]) == _bytes(lone_env._ep_stats), f"member {m}: records"
    # the same run again: the same bytes
    pop2, replays2, env2 = _run_population(start, capacity, opponent)
    assert _bytes(pop2._buf) == _bytes(pop._buf)
    assert _bytes(pop2._packed) == _bytes(pop._packed)
    for m in range(M):
        assert _bytes(replays2[m].memory) == _bytes(replays[m].memory)
        assert _bytes(replays2[m]._counter) == _bytes(replays[m]._counter)
    for k in STATE:
        assert _bytes(getattr(env2, k)) == _bytes(getattr(env, k)), k
    assert _bytes(env2._ep_stats) == _bytes(env._ep_stats)


def test_collect_refuses_shared_replays():
    from merging_gym import MergeVecEnv, RainbowPopulation, RainbowReplay

    replay = RainbowReplay(1000, device=DEV)
    pop = RainbowPopulation(_nets()[:2], [replay, replay], batch_size=BATCH)
    with pytest.raises(ValueError, match="rings are shared"):
        pop.collect(MergeVecEnv(128, device=DEV), 4)
    assert int(replay._counter.item()) == 0


def test_member_store_refuses_a_prioritized_replay_and_a_replay_listed_twice():
    from merging_gym import MergeVecEnv, PrioritizedRainbowReplay, RainbowNet, RainbowReplay, store_rainbow_rollout_many

    env = MergeVecEnv(128, device=DEV)
    nets = [RainbowNet.from_state_dict(sd, device=DEV) for sd in _nets()[:2]]
    obs0 = env.observe()
    traj = env.rollout_rainbow_many(4, nets)
    plain, prio = RainbowReplay(1000, device=DEV), PrioritizedRainbowReplay(1000, device=DEV)
    with pytest.raises(ValueError, match="PrioritizedRainbowReplay"):
        store_rainbow_rollout_many([plain, prio], obs0, traj)
    with pytest.raises(ValueError, match="listed twice"):
        store_rainbow_rollout_many([plain, plain], obs0, traj)
    with pytest.raises(ValueError, match="one capacity"):
        store_rainbow_rollout_many([plain, RainbowReplay(500, device=DEV)], obs0, traj)
    assert int(plain._counter.item()) == 0 and int(prio._counter.item()) == 0
