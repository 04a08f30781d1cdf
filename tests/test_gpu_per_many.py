"""A population of prioritized Rainbow learners on the GPU. mg_rainbow_learn_prioritized_many against its host twin
(itself pinned to the lone host learner per member by test_per_many_host.py) at the shapes where the member forms
can go wrong and the lone ones cannot; one population that mixes the edge members; mg_per_store_many against its
host twin on every launch path; PrioritizedRainbowPopulation against M lone PrioritizedRainbowLearner(DeviceNoise)
loops through Python, with checkpoints, copy_member, per-call beta and the constructor's refusals. Every comparison
is bit for bit."""

import numpy as np
import pytest

import per_many_ref as pm
import per_model
import per_ref as P
import rainbow_learn_many_ref as many
import rainbow_ref
from learn_ref import bits

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 3


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


# ---------------------------------------------------------------------------- learn: device against host
# capacity 13 has C = 16, so leaves lie beyond the ring; B = 33 > 13 repeats indices in every update; (1024, 2): the
# largest batch and scratch stride, a full block of the update; (8, 64): both halves of the argument arrays;
# (33, 2, 3000): a tree of twelve levels.
@pytest.mark.parametrize("B,M,cap", [(1, 2, 13), (33, 3, 13), (1024, 2, 13), (8, 64, 13), (33, 2, 3000)])
def test_every_member_equals_the_host_twin(torch, B, M, cap):
    settings = pm.member_settings(M)
    pers, L, nf = pm.replays(settings, cap), many.learners(M), many.noise(U, M)
    got = pm.run_device_many(torch, L, settings, pers, B, U, nf)
    want = pm.run_host_many(L, settings, pers, B, U, nf)
    pm.assert_members_same(got, want, members=[0, 31, 32, 47, 63] if M == 64 else None)
    for m, (s, e) in enumerate(zip(settings, got[8])):
        assert (int(e.first_update), int(e.first_draw)) == (s["first_update"] + U, s["first_draw"] + U)
        assert (P.f64bits(got[7][m].tree) != P.f64bits(pers[m].tree)).any(), f"member {m}: the priorities moved"
    if B > 1:
        assert (got[5][:, 0] != got[5][:, 1]).any() and (bits(got[6][:, 0]) != bits(got[6][:, 1])).any()


def test_runs_repeat_and_k_updates_in_one_call_equal_k_calls(torch):
    settings = pm.member_settings(3)
    pers, L, nf = pm.replays(settings, 13), many.learners(3), many.noise(U, 3)
    a = pm.run_device_many(torch, L, settings, pers, 33, U, nf)
    b = pm.run_device_many(torch, L, settings, pers, 33, U, nf)
    c = pm.run_device_many(torch, L, settings, pers, 33, U, nf, calls=[1, 0, 2])
    for other in (b, c):
        pm.assert_members_same(other, a)
        assert (other[9] == a[9]).all()  # the packed nets
        assert [int(e.first_update) for e in other[8]] == [int(e.first_update) for e in a[8]]


def test_one_population_of_edge_members(torch):
    """Members with 0 and 1 stored transitions (len < 2: slot 0 with weight 1), a wrapped one, and one whose every
    row is done with a reward clamped onto the last atom, so its projected mass is dropped, loss_b is exactly 0 and,
    with prio_eps 0, loss_b + prio_eps <= 0: its priorities are left as they were."""
    cap, B = 13, 33
    settings = pm.member_settings(4)
    settings[3]["prio_eps"] = 0.0
    pers = pm.replays(settings, cap, counts=[0, 1, 3 * cap + 2, cap + 4])
    pers[3].rows[:, 22], pers[3].rows[:, 11] = 1.0, 25.0
    L, nf = many.learners(4), many.noise(U, 4)
    got = pm.run_device_many(torch, L, settings, pers, B, U, nf)
    want = pm.run_host_many(L, settings, pers, B, U, nf)
    pm.assert_members_same(got, want)
    for m in (0, 1):
        assert (got[5][:, m] == 0).all() and (got[6][:, m] == 1.0).all()
    assert (got[5][:, 2] != 0).any() and len(np.unique(got[6][:, 2])) > 1
    assert (got[1][:, 3] == 0.0).all() and (got[5][:, 3] != 0).any()
    assert (P.f64bits(got[7][3].tree) == P.f64bits(pers[3].tree)).all()  # every priority refused
    assert (P.f64bits(got[7][2].tree) != P.f64bits(pers[2].tree)).any()


# ---------------------------------------------------------------------------- store: device against host
# 1: the fill alone; 13 and 1025: the tail only; 5000: per-level launches, then the tail (test_gpu_per.py's EDGES)
@pytest.mark.parametrize("cap", [1, 13, 1025, 5000])
def test_store_many_equals_its_host_twin(torch, cap):
    """per_model.scenario_stores (one store of exactly the ring from a non-zero position, one larger than the ring)
    for three members that start at different counters, so their wrapped segments differ."""
    from merging_gym import _native as nat

    M = 3
    assert per_model.tail_level(cap) == (3 if cap == 5000 else 1)
    settings, start = pm.member_settings(M), pm.store_counters(M)
    host = [P.HostPer(cap, s["alpha"]) for s in settings]
    for h, c in zip(host, start):
        h.push_many(c, n=max(1, min(c, cap)))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731

    class Dev:  # what store_many reads of a HostPer, on the device
        def __init__(self, h):
            self.rows, self.tree, self.counter = up(h.rows), up(h.tree), up(h.counter.view(np.int64))
            self.alpha, self.capacity, self.nbytes = h.alpha, h.capacity, h.nbytes

    dev = [Dev(h) for h in host]
    stream = torch.cuda.current_stream(DEV).cuda_stream
    at = list(start)
    for r, (n, T) in enumerate(per_model.scenario_stores(cap)):
        batch, _ = pm.store_batch(n, T, M, at)
        nat.check(pm.store_many(nat.lib.mg_host_per_store_many, nat, host, batch, n, T), "mg_host_per_store_many")
        dbatch = {k: up(v) for k, v in batch.items()}
        nat.check(pm.store_many(nat.lib.mg_per_store_many, nat, dev, dbatch, n, T, pointer=lambda t: t.data_ptr(),
                                extra=(stream,)), "mg_per_store_many")
        torch.cuda.synchronize()
        for m in range(M):
            at[m] += n * T
            what = f"capacity {cap}, store {r} ({n} x {T}), member {m}"
            assert int(dev[m].counter.item()) == int(host[m].counter[0]) == at[m], what
            assert (P.f64bits(dev[m].tree.cpu().numpy()) == P.f64bits(host[m].tree)).all(), what + ": tree"
            assert (bits(dev[m].rows.cpu().numpy()) == bits(host[m].rows)).all(), what + ": rows"
        if r == 3:  # one member's max_priority rises: its later leaves differ from the others'
            host[1].update(np.array([0]), np.array([5.0], np.float32))
            dev[1].tree.copy_(up(host[1].tree))


# ---------------------------------------------------------------------------- through Python
MP, N_MEMBER, BATCH, T = 3, 64, 32, 4
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf")
NETS = ((3, False), (1, True), (2, False))
KW = [dict(lr=0.001, gamma=0.99, seed=11, noise_seed=21), dict(lr=0.002, gamma=0.95, seed=12, noise_seed=22),
      dict(lr=0.0005, gamma=0.9, seed=13, noise_seed=23)]
ALPHAS, BETAS, PRIO_EPS = (0.6, 1.0, 0.4), (0.4, 1.0, 0.7), (1e-5, 1e-3, 0.0)


def _start():
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(MP * N_MEMBER, device=DEV)
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
    return [rainbow_ref.state_dict(seed, soft) for seed, soft in NETS]


def _population(capacity, **kw):
    from merging_gym import PrioritizedRainbowPopulation, PrioritizedRainbowReplay

    replays = [PrioritizedRainbowReplay(capacity, alpha=a, device=DEV) for a in ALPHAS]
    args = dict({k: [s[k] for s in KW] for k in KW[0]}, batch_size=BATCH, beta=BETAS, prio_eps=PRIO_EPS)
    args.update(kw)
    return PrioritizedRainbowPopulation(_nets(), replays, **args), replays


def _lone(m, capacity):
    from merging_gym import DeviceNoise, PrioritizedRainbowLearner, PrioritizedRainbowReplay

    replay = PrioritizedRainbowReplay(capacity, alpha=ALPHAS[m], device=DEV)
    kw = KW[m]
    return PrioritizedRainbowLearner(_nets()[m], replay, lr=kw["lr"], gamma=kw["gamma"], batch_size=BATCH,
                                     seed=kw["seed"], generator=DeviceNoise(kw["noise_seed"]), device=DEV, beta=BETAS[m],
                                     prio_eps=PRIO_EPS[m]), replay


def _run_population(start, capacity, rounds=2):
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(MP * N_MEMBER, device=DEV)
    _load(env, start, 0, MP * N_MEMBER)
    pop, replays = _population(capacity)
    outs = []
    for _ in range(rounds):
        pop.collect(env, T)
        outs.append(pop.learn(3, return_loss=True, return_idx=True, return_weights=True))
    return pop, replays, env, outs


@pytest.mark.parametrize("capacity", [100, 1000])  # 100: one collect's 256 transitions exceed the ring
def test_collect_and_learn_equal_the_lone_loops(capacity):
    from merging_gym import MergeVecEnv

    start = _start()
    pop, replays, env, outs = _run_population(start, capacity)
    assert tuple(outs[0][1].shape) == (3, MP, BATCH) and tuple(outs[0][2].shape) == (3, MP, BATCH)
    for m in range(MP):
        lo, hi = m * N_MEMBER, (m + 1) * N_MEMBER
        lone_env = MergeVecEnv(N_MEMBER, device=DEV)
        _load(lone_env, start, lo, hi)
        learner, replay = _lone(m, capacity)
        for r in range(2):
            obs0 = lone_env.observe().clone()
            replay.store_rollout(obs0, lone_env.rollout_rainbow(T, learner.net))
            loss, idx, w = learner.learn(3, return_loss=True, return_idx=True, return_weights=True)
            assert _bytes(outs[r][0][:, m]) == _bytes(loss), f"member {m}, round {r}: loss"
            assert _bytes(outs[r][1][:, m]) == _bytes(idx) and _bytes(outs[r][2][:, m]) == _bytes(w), (m, r)
        got, want = pop.member_state_dict(m), learner.state_dict()
        assert set(got) == set(want)
        for k in want:
            assert (_bytes(got[k]) == _bytes(want[k])) if k == "learner" else got[k] == want[k], (m, k)
        assert _bytes(pop.nets[m].packed) == _bytes(learner.net.packed), f"member {m}: packed net"
        assert int(replays[m]._counter.item()) == int(replay._counter.item()) == 2 * T * N_MEMBER
        assert _bytes(replays[m].memory) == _bytes(replay.memory), f"member {m}: replay memory"
        assert _bytes(replays[m]._tree) == _bytes(replay._tree), f"member {m}: tree"
        assert replays[m].max_priority == replay.max_priority
        for k in STATE:
            assert _bytes(getattr(env, k)[lo:hi]) == _bytes(getattr(lone_env, k)), (m, k)
        # the member's state loads into a lone learner, and back
        other, _ = _lone(m, capacity)
        other.load_state_dict(got)
        assert _bytes(other.state_dict()["learner"]) == _bytes(want["learner"])
        pop.load_member_state_dict(m, other.state_dict())
        assert _bytes(pop.member_state_dict(m)["learner"]) == _bytes(want["learner"])
    # the same run again: the same bytes
    pop2, replays2, env2, _ = _run_population(start, capacity)
    assert _bytes(pop2._buf) == _bytes(pop._buf) and _bytes(pop2._packed) == _bytes(pop._packed)
    for m in range(MP):
        assert _bytes(replays2[m].memory) == _bytes(replays[m].memory)
        assert _bytes(replays2[m]._tree) == _bytes(replays[m]._tree)


def test_checkpoint_resumes_bit_for_bit_and_copy_member():
    from merging_gym import MergeVecEnv

    start = _start()
    whole, wreplays, _, _ = _run_population(start, 1000, rounds=2)
    env = MergeVecEnv(MP * N_MEMBER, device=DEV)
    _load(env, start, 0, MP * N_MEMBER)
    pop, replays = _population(1000)
    pop.collect(env, T)
    pop.learn(3)
    sd, rsd = pop.state_dict(), [r.state_dict() for r in replays]
    again, replays2 = _population(1000, seed=0, noise_seed=None)  # other seeds: the state brings its own
    again.load_state_dict(sd)
    for r, s in zip(replays2, rsd):
        r.load_state_dict(s)
    again.collect(env, T)
    again.learn(3)
    assert _bytes(again._buf) == _bytes(whole._buf) and _bytes(again._packed) == _bytes(whole._packed)
    assert again.learn_step_counter == whole.learn_step_counter == [6] * MP
    for a, b in zip(replays2, wreplays):
        assert _bytes(a._tree) == _bytes(b._tree) and _bytes(a.memory) == _bytes(b.memory)
    # copy_member: nets, moments and counters move; seeds, replay and tree stay (member 1 is a "soft" net, whose
    # gradients are never all zero)
    tree0 = _bytes(replays2[0]._tree)
    again.copy_member(1, 0)
    assert _bytes(again._buf[0]) == _bytes(again._buf[1]) and _bytes(again._packed[0]) == _bytes(again._packed[1])
    assert again.seed[0] == KW[0]["seed"] and _bytes(replays2[0]._tree) == tree0
    again.learn(1)
    assert _bytes(again._buf[0]) != _bytes(again._buf[1])  # its own replay, seed and tree from here on


def test_beta_per_call_as_a_scalar_and_as_a_sequence():
    from merging_gym import MergeVecEnv

    start = _start()

    def run(beta, ctor=None):
        env = MergeVecEnv(MP * N_MEMBER, device=DEV)
        _load(env, start, 0, MP * N_MEMBER)
        pop, _ = _population(1000, **({} if ctor is None else dict(beta=ctor)))
        pop.collect(env, T)
        return pop.learn(2, return_weights=True, beta=beta), pop

    (w_scalar, a), (w_seq, b), (w_ctor, c) = run(0.9), run([0.9, 0.9, 0.9]), run(None, ctor=0.9)
    assert _bytes(w_scalar) == _bytes(w_seq) == _bytes(w_ctor) and _bytes(a._buf) == _bytes(b._buf) == _bytes(c._buf)
    (w_own, d), (w_mixed, e) = run(None), run([0.4, 0.9, 0.7])
    assert _bytes(w_mixed[:, 0]) == _bytes(w_own[:, 0]) and _bytes(w_mixed[:, 2]) == _bytes(w_own[:, 2])
    assert _bytes(w_mixed[:, 1]) == _bytes(w_scalar[:, 1]) and _bytes(w_mixed[:, 1]) != _bytes(w_own[:, 1])
    with pytest.raises(ValueError, match="beta must be > 0"):
        a.learn(1, beta=[0.4, 0.0, 0.4])
    with pytest.raises(ValueError, match="beta: expected one value or 3"):
        a.learn(1, beta=[0.4, 0.4])
    assert a.learn_step_counter == [2] * MP


def test_constructor_and_store_refusals():
    from merging_gym import (PrioritizedRainbowPopulation, PrioritizedRainbowReplay, RainbowReplay,
                             store_prioritized_rollout_many)

    nets = _nets()[:2]
    new = lambda cap=100: PrioritizedRainbowReplay(cap, device=DEV)  # noqa: E731
    shared = new()
    with pytest.raises(ValueError, match="listed twice"):
        PrioritizedRainbowPopulation(nets, [shared, shared])
    with pytest.raises(ValueError, match="expected PrioritizedRainbowReplays, got a RainbowReplay"):
        PrioritizedRainbowPopulation(nets, [new(), RainbowReplay(100, device=DEV)])
    with pytest.raises(ValueError, match="share one capacity"):
        PrioritizedRainbowPopulation(nets, [new(), new(200)])
    for kw, text in ((dict(beta=0.0), "beta must be > 0"), (dict(beta=[0.4, -1.0]), "beta must be > 0"),
                     (dict(beta=[0.4] * 3), "beta: expected one value or 2"), (dict(prio_eps=-1e-6), "prio_eps must be >= 0"),
                     (dict(prio_eps=[0.0, 0.0, 0.0]), "prio_eps: expected one value or 2")):
        with pytest.raises(ValueError, match=text):
            PrioritizedRainbowPopulation(nets, [new(), new()], **kw)
    traj = dict(final_observation=None)
    with pytest.raises(ValueError, match="expected PrioritizedRainbowReplays, got a RainbowReplay"):
        store_prioritized_rollout_many([new(), RainbowReplay(100, device=DEV)], None, traj)
    with pytest.raises(ValueError, match="listed twice"):
        store_prioritized_rollout_many([shared, shared], None, traj)
