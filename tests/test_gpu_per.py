"""Prioritized replay on the GPU: mg_per_store / mg_per_sample / mg_per_update against the host twins bit for
bit (rows, counter, every node of both trees, max_priority, indices and weights), the alpha = 1 rounds of the
reference's fixture on the device, mg_rainbow_learn_prioritized against its host twin, and the Python class's
checkpoint."""
import numpy as np
import pytest

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


@pytest.mark.parametrize("size,alpha", ((13, 1.0), (13, 0.6), (3000, 1.0), (3000, 0.6)))
def test_prioritized_learner_equals_its_host_twin(torch, size, alpha):
    from merging_gym import RainbowNet

    B, U, beta, eps = 32, 3, 0.5, 1e-5
    h = P.learn_case(size, alpha)
    lr = _prioritized(torch, h, B, eps)
    rp, sd = lr.replay, R.golden_state(1, "soft")
    got = [t.cpu().numpy() for t in _learn_all(lr, U, beta)]
    want = P.run_host_prioritized(R.learner_numpy(sd), h, B, U, beta, eps, seed=3, noise_f=R.noise(U))
    R.assert_same((lr._buf.cpu().numpy(), got[:4]), (want[0], list(want[1:5])))
    assert np.array_equal(got[4], want[5]) and np.array_equal(bits(got[5]), bits(want[6]))
    assert len(np.unique(want[6])) > 4 and (want[6] <= 1.0).all()  # real weights
    _assert_same_state(rp, h, "after learn")
    # the acting net equals mg_rainbow_pack of the result
    assert torch.equal(RainbowNet.from_state_dict(lr.current_state_dict(), device=DEV).packed, lr.net.packed)


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
