"""Prioritized replay on the host (CPU): the host twins mg_host_per_* against tests/per_model.py, a model that
pushes one transition at a time and knows nothing of segments or level bounds, at the capacities the recorded
fixture does not reach: 1 and 2, powers of two (C == capacity), one past a power of two, and rings large enough
for several levels of several blocks each before the single-block tail. The device runs the same scenario in
tests/test_gpu_per.py."""
import numpy as np
import pytest

import per_model as M
import per_ref as P


def test_the_scenario_reaches_what_it_is_for():
    """The stores and update batches themselves, so a change to them cannot quietly drop an edge."""
    for cap in M.CAPACITIES:
        stores = M.scenario_stores(cap)
        assert len(stores) == 8 and all(n >= 1 for n, _ in stores)
        at, wrapped_whole_ring, overfull = 0, False, False
        for n, T in stores:
            wrapped_whole_ring |= n * T == cap and at % cap != 0
            overfull |= n * T > cap
            at += n * T
        assert overfull and (wrapped_whole_ring or cap in (1, 2, 5))  # at these three that store starts at slot 0
    rng = np.random.default_rng(0)
    for B in M.UPDATE_BATCHES:
        idx, prio = M.update_batch(rng, 40, B)
        assert -1 <= idx.min() and idx.max() <= 40
        assert B < 1024 or (idx.min(), idx.max()) == (-1, 40)  # both rejected ends
        assert (prio[prio > 0] >= 1e-3).all() and (prio <= 8).all()
        if B == 1:
            assert prio[0] > 0
            continue
        assert (prio[6::7] == -1).all() and prio[B - 1] == -1 and idx[B - 1] == idx[2] and prio[2] > 0
        assert idx[1] == idx[B - 2] and prio[1] > 0 and prio[B - 2] > 0 and prio[1] != prio[B - 2]
        assert idx[3] == idx[4] and prio[3] > 0 and prio[4] > 0 and prio[3] != prio[4]  # neighbours


def test_the_large_capacities_need_several_level_loops():
    """What the 5000 and 9000 rings are here for: a store that fills them goes through two and three per-level
    launches on the device before the single-block tail, the fixture's largest ring (3000) through one. The rule
    is restated on the constants csrc/mg_per.h holds, so the cases stay on those paths if the constants move."""
    assert [M.tail_level(c) for c in (3000, 4096, 5000, 9000)] == [2, 3, 3, 4]
    assert [M.tail_level(c) for c in (4083, 4084, 8167, 8168)] == [2, 3, 3, 4]


@pytest.mark.parametrize("alpha", M.ALPHAS)
@pytest.mark.parametrize("cap", M.CAPACITIES)
def test_host_twins_equal_the_model(cap, alpha):
    """Every node of both trees, max_priority and the counter bit for bit after every store and update; the
    sampled indices exactly and the weights within 1 fp32 step."""
    model, worst = M.run_scenario(cap, alpha, M.HostSubject(cap, alpha))
    print(f"capacity {cap}, alpha {alpha}: worst weight distance {worst} fp32 steps")
    assert worst <= 1
    assert model.counter == sum(n * T for n, T in M.scenario_stores(cap))


def test_capacity_one_draws_slot_zero_with_weight_one():
    """len < 2 whatever is stored: slot 0 with weight 1, and the one leaf is the whole tree."""
    h = P.HostPer(1, 0.6)
    assert h.C == 1 and h.nbytes == 8 * 6
    for count in (1, 4):
        h.push_many(count, n=count)
        idx, w = h.sample(7, 0.4, 3, count)
        assert len(h) == 1 and idx.tolist() == [0] * 7 and w.tolist() == [1.0] * 7
    h.update([0, 1, -1, 0], [2.0, 5.0, 5.0, -1.0])
    v = P.host_pow([2.0], [0.6])[0]
    assert h.sum[1] == h.min[1] == v and h.max_priority == 2.0
    model = M.PerModel(1, 0.6)
    model.push(5)
    model.update([0, 1, -1, 0], [2.0, 5.0, 5.0, -1.0])
    M.assert_same_tree(h.tree, h.counter[0], model, "capacity 1")


def test_the_model_keeps_the_last_valid_entry_of_a_slot():
    """The model's own rule, on a case small enough to read: slot 4's last entry is rejected, so the one before
    it stands; slot 9 is named once."""
    model = M.PerModel(13, 1.0)
    model.push(13)
    model.update([4, 9, 4, 4, 13, -1], [0.5, 3.0, 7.0, -0.25, 9.0, 9.0])
    assert model.sum[16 + 4] == model.min[16 + 4] == 7.0 and model.sum[16 + 9] == 3.0 and model.max_priority == 7.0
    assert model.sum[1] == 7.0 + 3.0 + 11.0 and model.min[1] == 1.0
    assert model.total(13) == model.sum[1] - 1.0 and model.total(2) == 1.0
    assert model.find(0.0, 13) == 0 and model.find(3.999, 13) == 3 and model.find(4.0, 13) == 4
    assert model.find(1e9, 13) == 12  # past the mass: the last leaf, kept below len
    h = P.HostPer(13, 1.0)
    h.push_many(13)
    h.update([4, 9, 4, 4, 13, -1], [0.5, 3.0, 7.0, -0.25, 9.0, 9.0])
    M.assert_same_tree(h.tree, h.counter[0], model, "13")
    assert h.total() == model.total(13)
