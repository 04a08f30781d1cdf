"""Prioritized replay on the GPU: mg_per_store / mg_per_sample / mg_per_update against the host twins bit for
bit (rows, counter, every node of both trees, max_priority, indices and weights), the same at the capacities
where the launch path changes against the one-push-at-a-time model of tests/per_model.py too, the alpha = 1
rounds of the reference's fixture on the device, mg_rainbow_learn_prioritized against its host twin, and the
Python class's checkpoint."""
import numpy as np
import pytest

import per_model as M
import per_ref as P
import rainbow_learn_ref as R
from learn_ref import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _device(torch, size, alpha):
    from merging_gym import PrioritizedRainbowReplay

    return PrioritizedRainbowReplay(size, alpha, device=DEV)


def _store(torch, rp, tr):
    dev = lambda x: None if x is None else torch.from_numpy(x).to(DEV)  # noqa: E731
    rp.store(dev(tr["obs_first"]), dev(tr["obs"]), dev(tr["a1"]), dev(tr["rew"]), dev(tr["done"]), dev(tr["final_obs"]),
             dev(tr.get("flags")))


def _assert_same_state(rp, h, what=""):
    assert int(rp._counter.item()) == int(h.counter[0]), what
    assert np.array_equal(bits(rp.memory.cpu().numpy()), bits(h.rows)), what
    got = rp._tree.cpu().numpy()
    diff = np.flatnonzero(P.f64bits(got)[1:] != P.f64bits(h.tree)[1:])  # sum's node 0 is unused
    assert diff.size == 0, f"{what}: {diff.size} tree doubles differ, first at {diff[:1] + 1}"


# (size, alpha, the stores as (n, T)): the last one of size 3000 is larger than the ring, wraps, and makes the
# rebuild span several blocks per level
STORES = ((6, 1.0, ((1, 1), (3, 1), (2, 3), (5, 2))), (13, 0.6, ((1, 1), (7, 1), (4, 3), (13, 2))),
          (3000, 0.6, ((1, 1), (300, 2), (1000, 4))))


@pytest.mark.parametrize("size,alpha,stores", STORES, ids=[f"size{s[0]}" for s in STORES])
def test_store_sample_update_equal_the_host_twins(torch, size, alpha, stores):
    rp, h = _device(torch, size, alpha), P.HostPer(size, alpha)
    _assert_same_state(rp, h, "fresh")
    at = 0
    for r, (n, T) in enumerate(stores):
        tr = P.transitions(n, T, first=at)
        at += n * T
        _store(torch, rp, tr)
        h.store(tr)
        _assert_same_state(rp, h, f"store {r}")
        for draw in range(2):
            idx, w = rp.sample_indices(P.BATCH, P.BETA, seed=5, draw=10 * r + draw)
            hidx, hw = h.sample(P.BATCH, P.BETA, 5, 10 * r + draw)
            assert np.array_equal(idx.cpu().numpy(), hidx) and np.array_equal(bits(w.cpu().numpy()), bits(hw)), (r, draw)
            prio = np.exp(np.random.default_rng(r).uniform(np.log(1e-3), np.log(8.0), P.BATCH)).astype(np.float32)
            rp.update_priorities(idx, torch.from_numpy(prio))
            h.update(hidx, prio)
            _assert_same_state(rp, h, f"update {r}.{draw}")
    assert len(rp) == min(at, size) and rp.max_priority == h.max_priority > 1.0


@pytest.mark.parametrize("batch", (1, 32, 1024))
def test_batches_with_heavy_duplicates(torch, batch):
    rp, h = _device(torch, 13, 0.6), P.HostPer(13, 0.6)
    tr = P.transitions(5, 4)
    _store(torch, rp, tr)
    h.store(tr)
    for draw in range(3):
        idx, w = rp.sample_indices(batch, 0.7, seed=9, draw=draw)
        hidx, hw = h.sample(batch, 0.7, 9, draw)
        assert np.array_equal(idx.cpu().numpy(), hidx) and np.array_equal(bits(w.cpu().numpy()), bits(hw))
        prio = np.exp(np.random.default_rng(draw).uniform(np.log(1e-3), np.log(8.0), batch)).astype(np.float32)
        prio[::5] = -1.0  # rejected entries are left out on both sides
        rp.update_priorities(idx, torch.from_numpy(prio))
        h.update(hidx, prio)
        _assert_same_state(rp, h, f"draw {draw}")
    assert batch == 1 or len(set(hidx.tolist())) < batch


class _DeviceAndHost:
    """The device buffer and its host twin behind the calls per_model.run_scenario makes: every call goes to both,
    the samples have to be the same bits, and the device's results are what the model is compared with."""

    def __init__(self, torch, cap, alpha):
        self.torch, self.rp, self.h = torch, _device(torch, cap, alpha), P.HostPer(cap, alpha)

    def store(self, tr):
        _store(self.torch, self.rp, tr)
        self.h.store(tr)

    def update(self, idx, prio):
        self.rp.update_priorities(self.torch.from_numpy(idx), self.torch.from_numpy(prio))
        self.h.update(idx, prio)

    def sample(self, batch, beta, seed, draw):
        idx, w = (t.cpu().numpy() for t in self.rp.sample_indices(batch, beta, seed=seed, draw=draw))
        hidx, hw = self.h.sample(batch, beta, seed, draw)
        assert np.array_equal(idx, hidx) and np.array_equal(bits(w), bits(hw)), (beta, draw)
        return idx, w

    def state(self):
        return self.rp._tree.cpu().numpy(), int(self.rp._counter.item())

    def same_state(self, what):
        _assert_same_state(self.rp, self.h, what)


# capacity: the launch path the scenario's stores reach on the device (the levels are the tail level of the store
# that fills the ring, asserted below)
EDGES = {1: "logC == 0: the fill alone, no level and no tail launch",
         2: "one level, in the tail",
         4: "C == capacity: no leaf beyond the ring",
         1025: "one past a power of two: 1023 leaves beyond the ring, every level in the tail",
         4096: "C == capacity over several blocks, tail level 3",
         5000: "tail level 3: two per-level launches, and the whole-ring store's two wrapped segments span several "
               "blocks each",
         9000: "tail level 4: three per-level launches"}
TAIL_LEVELS = {1: 1, 2: 1, 4: 1, 1025: 1, 4096: 3, 5000: 3, 9000: 4}


def test_the_edge_capacities_are_on_their_launch_paths():
    """The tail level of the store that fills each ring, from the library's own constants (per_model.tail_level
    reads them from csrc/mg_per.h), and the whole-ring store's start at capacity 5000: if the constants move,
    this fails before the cases below quietly leave their paths."""
    from merging_gym import _native

    assert {cap: M.tail_level(cap) for cap in EDGES} == TAIL_LEVELS
    assert (M.tail_level(4083), M.tail_level(4084), M.tail_level(8167), M.tail_level(8168)) == (2, 3, 3, 4)
    assert M.tail_level(3000) == 2  # the largest ring of the tests above: one per-level launch
    for cap in EDGES:
        C = _native.lib.mg_per_bytes(cap) // 8 // 4  # 8 (4 C + 2) bytes
        assert (C == cap) == (cap in (1, 2, 4, 4096)) and (C == 1) == (cap == 1)
    stores = M.scenario_stores(5000)
    start = sum(n * T for n, T in stores[:3]) % 5000
    assert stores[3] == (5000, 1) and min(start, 5000 - start) > 3 * 256  # both segments: more than three blocks


@pytest.mark.parametrize("alpha", M.ALPHAS)
@pytest.mark.parametrize("cap", tuple(EDGES))
def test_edge_capacities_equal_the_host_twins_and_the_model(torch, cap, alpha):
    """per_model.run_scenario on the device: the stores of per_model.scenario_stores (one of exactly the ring from
    a non-zero position, one larger than the ring), after each one updates of 1, 33 and 1024 entries with
    duplicates and rejected entries, and samples at beta 0.4 and 1.0. After every store and update the rows, the
    counter and every tree double equal the host twin's bit for bit, and every tree node and max_priority equal
    the one-push-at-a-time model's; the samples equal the host twin's bit for bit, the model's indices exactly
    and its weights within 1 fp32 step. EDGES[cap] names the launch path the capacity is here for."""
    both = _DeviceAndHost(torch, cap, alpha)
    both.same_state("fresh")
    model, worst = M.run_scenario(cap, alpha, both, after=both.same_state)
    print(f"capacity {cap} ({EDGES[cap]}), alpha {alpha}: worst weight distance {worst} fp32 steps")
    assert worst <= 1
    assert len(both.rp) == cap and both.rp.max_priority == model.max_priority


def test_capacity_one_on_the_device(torch):
    """PrioritizedRainbowReplay takes capacity 1 (RainbowReplay refuses only capacity < 1): one leaf that is the
    root, len < 2 for ever, so every draw is slot 0 with weight 1 and sample() refuses."""
    from merging_gym import RainbowReplay

    with pytest.raises(ValueError, match="capacity must be >= 1"):
        RainbowReplay(0, device=DEV)
    rp, h = _device(torch, 1, 0.6), P.HostPer(1, 0.6)
    for tr in (P.transitions(1, 1), P.transitions(2, 2, first=1)):
        _store(torch, rp, tr)
        h.store(tr)
    _assert_same_state(rp, h, "stores")
    assert np.array_equal(rp.memory.cpu().numpy()[0], P.expected_row(4))
    idx, w = rp.sample_indices(7, 0.4, seed=3, draw=0)
    assert idx.tolist() == [0] * 7 and w.tolist() == [1.0] * 7
    rp.update_priorities([0, 1, -1, 0], [2.0, 5.0, 5.0, -1.0])
    h.update([0, 1, -1, 0], [2.0, 5.0, 5.0, -1.0])
    _assert_same_state(rp, h, "update")
    assert len(rp) == 1 and rp.max_priority == 2.0 and rp._tree[1].item() == P.host_pow([2.0], [0.6])[0]
    with pytest.raises(ValueError, match="at least two stored transitions"):
        rp.sample(4, 0.4)


@pytest.mark.parametrize("size", (6, 13))
def test_alpha_one_fixture_rounds_on_the_device(torch, size):
    """The reference's own trees, S aside (the host twin pins it), bit for bit after every round."""
    g, key = P.golden(), P.scenario_key(size, 1.0)
    rp = _device(torch, size, 1.0)
    at = 0
    while at < size + size // 2 + 1:
        n = min(7, size + size // 2 + 1 - at)
        _store(torch, rp, P.transitions(n, 1, first=at))
        at += n
    seed, C = int(g[key + "/seed"]), len(g[key + "/sum"][0]) // 2
    for r in range(P.ROUNDS):
        idx, w = rp.sample_indices(P.BATCH, P.BETA, seed=seed, draw=r)
        rp.update_priorities(idx, torch.from_numpy(g[key + "/prio"][r]))
        tree = rp._tree.cpu().numpy()
        assert np.array_equal(idx.cpu().numpy(), g[key + "/idx"][r]), r
        assert np.array_equal(P.f64bits(tree[1:2 * C]), P.f64bits(g[key + "/sum"][r][1:])), r
        assert np.array_equal(P.f64bits(tree[2 * C + 1:4 * C]), P.f64bits(g[key + "/min"][r][1:])), r
        assert P.f64bits(tree[4 * C]) == P.f64bits(g[key + "/maxp"][r]), r
        assert P.ulp32_distance(w.cpu().numpy(), g[key + "/w"][r].astype(np.float32)).max() <= 1, r


@pytest.mark.parametrize("use_flags", (False, True), ids=("a1-done", "flags"))
def test_the_stores_leave_the_same_rows_and_counter(torch, use_flags):
    """P.store_case through RainbowReplay.store, PrioritizedRainbowReplay.store and mg_host_per_store: one store
    helper behind all three, so the rows and the counter are the same bits, and those of sequential pushes."""
    from merging_gym import RainbowReplay

    first, tr = P.transitions(P.STORE_FIRST, 1), P.store_case(use_flags)
    plain, per, h = RainbowReplay(P.STORE_CAP, device=DEV), _device(torch, P.STORE_CAP, 0.6), P.HostPer(P.STORE_CAP, 0.6)
    for rp in (plain, per):
        _store(torch, rp, first)
        _store(torch, rp, tr)
    h.store(first)
    h.store(tr)
    want, counter = P.pushed(*P.pushed(np.zeros((P.STORE_CAP, P.ROW), np.float32), 0, first), P.store_case(False))
    assert counter == P.STORE_FIRST + 20 == int(h.counter[0]) and np.array_equal(bits(h.rows), bits(want))
    for rp in (plain, per):
        assert int(rp._counter.item()) == counter, type(rp).__name__
        assert np.array_equal(bits(rp.memory.cpu().numpy()), bits(want)), type(rp).__name__
    _assert_same_state(per, h, "the tree")


def _prioritized(torch, h, B, eps=1e-5):
    """A PrioritizedRainbowLearner (the soft golden state, seed 3, noise generator 11, beta 0.4) on a device copy of
    the HostPer h."""
    from merging_gym import PrioritizedRainbowLearner

    rp = _device(torch, h.capacity, h.alpha)
    rp.memory.copy_(torch.from_numpy(h.rows))
    rp._counter.fill_(int(h.counter[0]))
    rp._tree.copy_(torch.from_numpy(h.tree))
    return PrioritizedRainbowLearner(R.golden_state(1, "soft"), rp, batch_size=B, seed=3,
                                     generator=torch.Generator().manual_seed(11), device=DEV, beta=0.4, prio_eps=eps)


def _learn_all(lr, U, beta):
    return lr.learn(U, return_loss=True, return_rows=True, return_proj=True, return_grads=True, return_idx=True,
                    return_weights=True, beta=beta)


def test_three_updates_in_one_call_equal_three_calls_of_one(torch):
    """U = 3, B = 32 on the wrapped ring of 13 (a 16-leaf tree), alpha 0.6, beta 0.5: learn(3) against learn(1)
    three times with equal noise generators, bit for bit -- the learner buffer, the acting net, every tree node and
    max_priority, the rows and the counter, and all six outputs concatenated."""
    h = P.learn_case(13, 0.6)
    whole, single = _prioritized(torch, h, 32), _prioritized(torch, h, 32)
    a = _learn_all(whole, 3, 0.5)
    b = [torch.cat(parts) for parts in zip(*(_learn_all(single, 1, 0.5) for _ in range(3)))]
    raw = lambda t: t.contiguous().view(torch.uint8)  # noqa: E731
    for k, (x, y) in enumerate(zip(a, b)):
        assert x.shape == y.shape and torch.equal(raw(x), raw(y)), k
    assert torch.equal(raw(whole._buf), raw(single._buf)) and torch.equal(whole.net.packed, single.net.packed)
    for name in ("_tree", "memory", "_counter"):
        assert torch.equal(raw(getattr(whole.replay, name)), raw(getattr(single.replay, name))), name
    assert (whole.learn_step_counter, single.draw_counter) == (3, 3)
    assert not np.array_equal(P.f64bits(whole.replay._tree.cpu().numpy()), P.f64bits(h.tree))  # priorities moved
    assert len(np.unique(a[4].cpu().numpy())) > 4  # a real sample


def _learner_against_its_host_twin(torch, size, alpha, B):
    """Three updates in one call from P.learn_case(size, alpha), beta 0.5: the learner buffer, all six outputs,
    every tree node and max_priority, the rows and the counter bit for bit, and the packed acting net. Returns
    the host twin's tuple and the tree before and after the call."""
    from merging_gym import RainbowNet

    U, beta, eps = 3, 0.5, 1e-5
    h = P.learn_case(size, alpha)
    before = h.tree.copy()
    lr = _prioritized(torch, h, B, eps)
    rp, sd = lr.replay, R.golden_state(1, "soft")
    got = [t.cpu().numpy() for t in _learn_all(lr, U, beta)]
    want = P.run_host_prioritized(R.learner_numpy(sd), h, B, U, beta, eps, seed=3, noise_f=R.noise(U))
    R.assert_same((lr._buf.cpu().numpy(), got[:4]), (want[0], list(want[1:5])))
    assert np.array_equal(got[4], want[5]) and np.array_equal(bits(got[5]), bits(want[6]))
    _assert_same_state(rp, h, "after learn")
    assert rp.max_priority == h.max_priority
    # the acting net equals mg_rainbow_pack of the result
    assert torch.equal(RainbowNet.from_state_dict(lr.current_state_dict(), device=DEV).packed, lr.net.packed)
    return want, before, h.tree


@pytest.mark.parametrize("size,alpha", ((13, 1.0), (13, 0.6), (3000, 1.0), (3000, 0.6)))
def test_prioritized_learner_equals_its_host_twin(torch, size, alpha):
    want, _, _ = _learner_against_its_host_twin(torch, size, alpha, 32)
    assert len(np.unique(want[6])) > 4 and (want[6] <= 1.0).all()  # real weights


@pytest.mark.parametrize("B,size,alpha", ((1, 13, 0.6), (33, 13, 0.6), (1024, 13, 1.0)),
                         ids=("one-row", "wave-and-a-row", "full-block"))
def test_prioritized_learner_at_the_batch_edges(torch, B, size, alpha):
    """The sample, the weighted update and the in-call priority write-back (loss_b + prio_eps into the tree) at
    B = 1, at a batch that is no multiple of a wave, and at B = 1024 = the update kernel's block, where its LDS
    arrays, its duplicate scan and its max reduction are full: on the ring of 13 at most 12 slots can be drawn,
    so the 1024 entries name each drawn slot 85 times on average (the heaviest several hundred times) and only the
    last valid entry of each may set the leaf."""
    want, before, after = _learner_against_its_host_twin(torch, size, alpha, B)
    idx, w, grads = want[5], want[6], want[4]
    assert (w > 0).all() and (w <= 1.0).all() and (B == 1 or len(np.unique(w)) > 4)  # real weights
    # real gradients: in every update, but for one row alone, which may be a row without one (R.EDGE_SEED's comment)
    assert (any if B == 1 else all)(np.count_nonzero(g) > 0 for g in grads)
    assert not np.array_equal(P.f64bits(after), P.f64bits(before))  # the priorities moved
    if B == 1024:
        counts = np.bincount(idx[0], minlength=size)
        assert counts[size - 1] == 0 and counts.sum() == B and counts.max() > 64 and np.count_nonzero(counts) > 4


def test_checkpoint_resumes_bit_for_bit(torch):
    a, b = _device(torch, 13, 0.6), _device(torch, 13, 0.6)
    _store(torch, a, P.transitions(9, 2))
    idx, _ = a.sample_indices(8, 0.4, 1, 0)
    a.update_priorities(idx, torch.linspace(0.1, 3.0, 8))
    b.load_state_dict(a.state_dict())
    for rp in (a, b):
        _store(torch, rp, P.transitions(3, 1, first=18))
    out = [rp.sample(16, 0.4, seed=2, draw=1) for rp in (a, b)]
    assert all(torch.equal(x, y) for x, y in zip(*out))
    assert torch.equal(a._tree.view(torch.int64)[1:], b._tree.view(torch.int64)[1:])
    assert out[0][5].dtype == torch.float32 and out[0][6].dtype == torch.int64 and len(out[0]) == 7
    with pytest.raises(ValueError):
        _device(torch, 13, 0.6).sample(4, 0.4)
    from merging_gym import RainbowLearner

    with pytest.raises(ValueError, match="PrioritizedRainbowLearner"):
        RainbowLearner(R.golden_state(1, "soft"), a)
