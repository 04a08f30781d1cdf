"""A population of DQN learners on the GPU: mg_dqn_learn_many through merging_gym.DQNPopulation against
the plain-C restatement run once per member and against lone DQNLearners, bit for bit; determinism, a
shared ring, unequal counters, the state round trips and copy_member."""

import numpy as np
import pytest

import learn_many_ref as mr
import learn_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ring(rows, counter):
    import torch

    from merging_gym import ReplayRing

    ring = ReplayRing(rows.shape[0], device=DEV, goal=rows.shape[1] == 24)
    ring.memory.copy_(torch.as_tensor(np.array(rows)))  # a copy: the shared fixtures are read-only
    ring._counter.fill_(int(counter))
    return ring


def _pop_kw(kws):
    return dict(lr=[k["lr"] for k in kws], gamma=[k["gamma"] for k in kws], eps=[k["eps"] for k in kws],
                betas=[(k["beta1"], k["beta2"]) for k in kws], target_period=[k["target_period"] for k in kws],
                seed=[k["seed"] for k in kws])


def _population(sd, rings, kws, batch, L0=None):
    """A DQNPopulation on device rings with the members' settings; with L0 [M, 4, P] its blocks and the
    members' first_update / first_draw are set as the restatement's runs start."""
    import torch

    from merging_gym import DQNPopulation

    nets = sd if isinstance(sd, list) else [sd] * len(kws)
    pop = DQNPopulation(nets, rings, batch_size=batch, **_pop_kw(kws))
    if L0 is not None:
        pop._buf.copy_(torch.as_tensor(np.ascontiguousarray(L0).reshape(len(kws), -1)))
        for m, kw in enumerate(kws):
            pop._members[m].first_update, pop._members[m].first_draw = kw["first_update"], kw["first_draw"]
    return pop


def _blocks(pop):
    return pop._buf.cpu().numpy().reshape(len(pop), 4, -1)


def _lone(sd, ring, kw, batch):
    from merging_gym import DQNLearner

    return DQNLearner(sd, ring, batch_size=batch, lr=kw["lr"], gamma=kw["gamma"], betas=(kw["beta1"], kw["beta2"]),
                      eps=kw["eps"], target_period=kw["target_period"], seed=kw["seed"])


def _same(a, b):
    import torch

    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


# ------------------------------------------------------------------ 5. population == restatement
CASES = [(10, 5, 128, 3), (11, 5, 32, 2), (10, 3, 5, 3), (10, 5, 1, 2), (10, 5, 8, 64)]


@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch,members", CASES)
def test_population_equals_restatement_bit_for_bit(in_dim, out_dim, batch, members, filled_only):
    """Four updates of members that differ in seed, lr, gamma, betas, eps, target_period, first_update,
    first_draw, ring and counter, the targets starting at half the eval nets: some members copy their
    target in an update in which others do not (at 64 members, members >= 32 on both sides)."""
    sd, rings, counters, kws, L0, ref_end, ref_loss, ref_rows = mr.reference(in_dim, out_dim, batch, members,
                                                                             filled_only, big=True)
    assert rings[0].shape[0] == 2000
    masks = mr.sync_masks(kws, mr.UPDATES)
    lo = 32 if members == 64 else 0
    assert any({m for m in s if m >= lo} and {m for m in range(lo, members) if m not in s} for s in masks)
    pop = _population(sd, [_ring(r, c) for r, c in zip(rings, counters)], kws, batch, L0)
    loss, rows = pop.learn(mr.UPDATES, filled_only=filled_only, return_loss=True, return_rows=True)
    assert tuple(loss.shape) == (mr.UPDATES, members) and tuple(rows.shape) == (mr.UPDATES, members, batch, 2 * in_dim + 2)
    mr.assert_members_equal(_blocks(pop), loss.cpu().numpy(), rows.cpu().numpy(), ref_end, ref_loss, ref_rows)
    assert pop.learn_step_counter == [kw["first_update"] + mr.UPDATES for kw in kws]
    assert pop.draw_counter == [kw["first_draw"] + mr.UPDATES for kw in kws]


# ------------------------------------------------------------------ 6. population == lone learners
def test_population_equals_lone_learners_through_python():
    import torch

    sd, rings, counters, kws, *_ = mr.reference(10, 5, 128, 3, False, big=True)
    dev_rings = [_ring(r, c) for r, c in zip(rings, counters)]
    nets = [lr.seeded_net(10, 5, 40 + m) for m in range(3)]
    pop = _population(nets, dev_rings, kws, 128)
    lone = [_lone(nets[m], dev_rings[m], kws[m], 128) for m in range(3)]
    for m in range(3):
        assert _same(pop.qnets[m].packed, lone[m].qnet.packed)
    got = torch.cat([pop.learn(2, return_loss=True), pop.learn(1, return_loss=True)])
    for m in range(3):
        want = torch.cat([lone[m].learn(2, return_loss=True), lone[m].learn(1, return_loss=True)])
        assert _same(got[:, m], want)
        assert _same(pop._buf[m], lone[m]._buf)
        assert _same(pop.qnets[m].packed, lone[m].qnet.packed)
        for a, b in zip(pop.qnets[m].fp32, lone[m].qnet.fp32):
            assert _same(a, b)
        assert (pop.learn_step_counter[m], pop.draw_counter[m]) == (lone[m].learn_step_counter, lone[m].draw_counter)
        assert list(pop.eval_state_dict(m)) == list(lr.KEYS) and _same(pop.target_state_dict(m)["fc2.weight"],
                                                                      lone[m].target_state_dict()["fc2.weight"])
    assert len(pop) == 3 and pop.learn_step_counter == [3, 3, 3]


# ------------------------------------------------------------------ 7. determinism
def test_k_updates_in_one_call_equal_k_calls_and_two_runs_are_identical():
    import torch

    sd, rings, counters, kws, L0, *_ = mr.reference(10, 5, 128, 3, False, big=True)
    runs = []
    for split in (False, False, True):
        pop = _population(sd, [_ring(r, c) for r, c in zip(rings, counters)], kws, 128, L0)
        if split:
            loss = torch.cat([pop.learn(1, return_loss=True) for _ in range(5)])
        else:
            loss = pop.learn(5, return_loss=True)
        runs.append((pop._buf.clone(), loss.clone(), pop._packed.clone()))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert _same(a, b)
    assert bool(torch.isfinite(runs[0][1]).all())


# ------------------------------------------------------------------ 8. one ring for all members
def test_members_may_share_one_ring():
    rows, sd = mr.fixture(10, 5, 32, big=True)
    kws = [mr.member_kw(m) for m in range(4)]
    kws[3] = dict(kws[1])  # members 1 and 3: the same seed, hyperparameters and counters
    ring = _ring(rows, rows.shape[0])
    L0 = mr.start_blocks(sd, 4)
    L0[3] = L0[1]
    pop = _population(sd, [ring] * 4, kws, 32, L0)
    loss, got_rows = pop.learn(mr.UPDATES, return_loss=True, return_rows=True)
    got = _blocks(pop)
    assert np.array_equal(lr.bits(got[1]), lr.bits(got[3])) and not np.array_equal(lr.bits(got[1]), lr.bits(got[2]))
    assert _same(pop.qnets[1].packed, pop.qnets[3].packed) and _same(loss[:, 1], loss[:, 3])
    refs = [lr.run_ref(L0[m], rows, rows.shape[0], 10, 5, 32, mr.UPDATES, **kws[m]) for m in range(4)]
    mr.assert_members_equal(got, loss.cpu().numpy(), got_rows.cpu().numpy(), np.stack([r[0] for r in refs]),
                            np.stack([r[1] for r in refs], axis=1), np.stack([r[2] for r in refs], axis=1))


# ------------------------------------------------------------------ 9. filled_only, unequal counters
def test_filled_only_with_unequal_counters():
    rows, sd = mr.fixture(10, 5, 32, big=True)
    kws = [mr.member_kw(m) for m in range(3)]
    half, _ = lr.half_filled(rows)
    rings, counters = [np.zeros_like(rows), half, rows], [0, rows.shape[0] // 2, rows.shape[0]]
    rings[0][0] = rows[0]  # a counter of 0 draws slot 0
    L0 = mr.start_blocks(sd, 3)
    pop = _population(sd, [_ring(r, c) for r, c in zip(rings, counters)], kws, 32, L0)
    loss, got_rows = pop.learn(mr.UPDATES, filled_only=True, return_loss=True, return_rows=True)
    refs = [lr.run_ref(L0[m], rings[m], counters[m], 10, 5, 32, mr.UPDATES, filled_only=True, **kws[m])
            for m in range(3)]
    mr.assert_members_equal(_blocks(pop), loss.cpu().numpy(), got_rows.cpu().numpy(), np.stack([r[0] for r in refs]),
                            np.stack([r[1] for r in refs], axis=1), np.stack([r[2] for r in refs], axis=1))
    g = got_rows.cpu().numpy()
    assert (g[:, 0] == rows[0]).all() and (np.abs(g[:, 1]).sum(axis=-1) > 0).all()


# ------------------------------------------------------------------ 10. state round trips
def _cpu(sd):
    import torch

    return {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in sd.items()}


def test_member_and_population_state_round_trips():
    sd, rings, counters, kws, L0, *_ = mr.reference(10, 5, 32, 3, False, big=True)
    dev_rings = [_ring(r, c) for r, c in zip(rings, counters)]
    pop = _population(sd, dev_rings, kws, 32, L0)
    pop.learn(2)
    saved = _cpu(pop.state_dict())
    # member -> lone learner
    lone = [_lone(lr.seeded_net(10, 5, 90 + m), dev_rings[m], kws[m], 32) for m in range(3)]
    for m in range(3):
        msd = _cpu(pop.member_state_dict(m))
        assert sorted(msd) == sorted(lone[m].state_dict())
        lone[m].load_state_dict(msd)
        assert _same(lone[m].qnet.packed, pop.qnets[m].packed)
        lone[m].learn(2)
    pop.learn(2)
    for m in range(3):
        assert _same(pop._buf[m], lone[m]._buf) and _same(pop.qnets[m].packed, lone[m].qnet.packed)
        assert (pop.learn_step_counter[m], pop.draw_counter[m]) == (lone[m].learn_step_counter, lone[m].draw_counter)
    # lone learner -> member of another population, whose seeds differ until the load
    other = _population(lr.seeded_net(10, 5, 77), dev_rings, [dict(kw, seed=1) for kw in kws], 32)
    for m in range(3):
        other.load_member_state_dict(m, _cpu(lone[m].state_dict()))
        assert _same(other.qnets[m].packed, lone[m].qnet.packed)
        lone[m].learn(2)
    other.learn(2)
    pop.learn(2)
    for m in range(3):
        assert _same(other._buf[m], lone[m]._buf) and _same(other.qnets[m].packed, lone[m].qnet.packed)
    assert _same(other._buf, pop._buf)
    # the whole population, saved mid-run
    fresh = _population(lr.seeded_net(10, 5, 78), dev_rings, [dict(kw, seed=2) for kw in kws], 32)
    fresh.load_state_dict(saved)
    assert (fresh.learn_step_counter, fresh.draw_counter) == (saved["learn_step_counter"], saved["draw_counter"])
    fresh.learn(4)
    assert _same(fresh._buf, pop._buf) and _same(fresh._packed, pop._packed)
    assert (fresh.learn_step_counter, fresh.draw_counter) == (pop.learn_step_counter, pop.draw_counter)


# ------------------------------------------------------------------ 11. copy_member
def test_copy_member_is_the_exploit_step():
    sd, rings, counters, kws, L0, *_ = mr.reference(10, 5, 32, 3, False, big=True)
    pop = _population(sd, [_ring(r, c) for r, c in zip(rings, counters)], kws, 32, L0)
    pop.learn(2)
    before = pop._buf.clone(), pop._packed.clone()
    steps, draws = pop.learn_step_counter, pop.draw_counter
    pop.copy_member(0, 2)
    assert _same(pop._buf[2], before[0][0]) and _same(pop.qnets[2].packed, before[1][0])
    assert _same(pop._buf[:2], before[0][:2]) and _same(pop._packed[:2], before[1][:2])
    assert pop.learn_step_counter == [steps[0], steps[1], steps[0]] and pop.draw_counter == [draws[0], draws[1], draws[0]]
    assert pop.seed[2] == kws[2]["seed"]
    loss = pop.learn(1, return_loss=True)
    start = before[0][0].cpu().numpy().reshape(4, -1)
    kw = dict(kws[2], first_update=steps[0], first_draw=draws[0])  # src's state, dst's own seed and hyperparameters
    want, want_loss, _, _ = lr.run_ref(start, rings[2], counters[2], 10, 5, 32, 1, **kw)
    assert np.array_equal(lr.bits(_blocks(pop)[2]), lr.bits(want))
    assert np.array_equal(lr.bits(loss[:, 2].cpu().numpy()), lr.bits(want_loss))
