"""Rainbow's compute_td_loss and its replay memory on the GPU: mg_rainbow_learn against the plain-C restatement
bit for bit, K updates in one call against K calls, the replay store against sequential pushes, the acting
net's packing, a bit-identical resume and the closed acting / learning loop."""
import numpy as np
import pytest

import rainbow_learn_ref as R
from learn_ref import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _replay(torch, ring, counter):
    from merging_gym import RainbowReplay

    rp = RainbowReplay(len(ring), device=DEV)
    rp.memory.copy_(torch.from_numpy(ring))
    rp._counter.fill_(counter)
    return rp


def _learner(torch, fam, ring, counter, batch, seed=3, noise_seed=11):
    from merging_gym import RainbowLearner

    return RainbowLearner(R.golden_state(1, fam), _replay(torch, ring, counter), batch_size=batch, seed=seed,
                          generator=torch.Generator().manual_seed(noise_seed), device=DEV)


def _all(learner, U):
    return [t.cpu().numpy() for t in learner.learn(U, return_loss=True, return_rows=True, return_proj=True,
                                                   return_grads=True)]


@pytest.mark.parametrize("capacity,counter", R.RINGS, ids=["partly-filled", "wrapped"])
@pytest.mark.parametrize("batch", R.BATCHES)
def test_device_learn_equals_the_restatement(torch, batch, capacity, counter):
    """learn(2), sync_target(), learn(1) on the cases of tests/test_rainbow_learn_host.py. The "default" family
    at B = 1 is kept as the saturated-softmax case: a zero-gradient update (see that file); the edge batches
    with real gradients are the test below."""
    fam = "soft" if batch in (32, 128) else "default"
    ring, c = R.ring_case(capacity, counter)
    want = R.sequence(R.run_ref, R.learner_numpy(R.golden_state(1, fam)), ring, c, batch)
    lr = _learner(torch, fam, ring, c, batch)
    out = _all(lr, 2)
    lr.sync_target()
    out += _all(lr, 1)
    R.assert_same((lr._buf.cpu().numpy(), out), want)
    assert (lr.learn_step_counter, lr.draw_counter) == (3, 3)


@pytest.mark.parametrize("capacity,counter", R.RINGS, ids=["partly-filled", "wrapped"])
@pytest.mark.parametrize("batch", R.EDGE_BATCHES)
def test_device_learn_equals_the_restatement_at_batch_edges(torch, batch, capacity, counter):
    """The same sequence from the "soft" state at B = 1, 33, 257 (the first batch past one block of items) and
    1024 (the largest): the backward and Adam launches of the lone learner on real gradients. Every update's
    gradient has non-zero entries, and the current parameters moved: the parameters after the first call differ
    from the start's, those after the second from the first call's (R.edge_reference checks the restatement,
    which the device equals bit for bit, update by update)."""
    L0, want = R.edge_reference(batch, capacity, counter)
    lr = _learner(torch, "soft", *R.ring_case(capacity, counter), batch, seed=R.EDGE_SEED)
    out = _all(lr, 2)
    mid = lr._buf[:R.NP].cpu().numpy()
    lr.sync_target()
    out += _all(lr, 1)
    end = lr._buf.cpu().numpy()
    R.assert_same((end, out), want)
    for grads in (out[3][0], out[3][1], out[7][0]):
        assert np.count_nonzero(grads) > 0 and np.isfinite(grads).all()
    assert (bits(mid) != bits(L0[:R.NP])).any() and (bits(end[:R.NP]) != bits(mid)).any()
    assert (lr.learn_step_counter, lr.draw_counter) == (3, 3)


def test_k_updates_in_one_call_equal_k_calls_and_runs_repeat(torch):
    ring, c = R.ring_case(64, 200)
    one, many, again = (_learner(torch, "soft", ring, c, 33) for _ in range(3))
    a = one.learn(3, return_loss=True)
    b = torch.cat([many.learn(1, return_loss=True) for _ in range(3)])
    d = again.learn(3, return_loss=True)
    for other, loss in ((many, b), (again, d)):
        assert torch.equal(a.view(torch.int32), loss.view(torch.int32))
        assert torch.equal(one._buf.view(torch.int32), other._buf.view(torch.int32))
        assert torch.equal(one.net.packed, other.net.packed)


def _emulate_pushes(ring, counter, obs_first, obs, a1, rew, done, final_obs):
    """Sequential replay_buffer.push calls in (step, env) order on a numpy ring."""
    T, n = a1.shape
    cap = len(ring)
    for t in range(T):
        for i in range(n):
            s = obs_first[i] if t == 0 else obs[t - 1, i]
            s2 = final_obs[t, i] if done[t, i] and final_obs is not None else obs[t, i]
            row = np.zeros(24, np.float32)
            row[:10], row[10], row[11], row[12:22], row[22] = s, a1[t, i], rew[t, i, 0], s2, done[t, i]
            ring[counter % cap] = row
            counter += 1
    return counter


@pytest.mark.parametrize("all_done_at", [None, 2])
@pytest.mark.parametrize("use_flags", [False, True])
def test_store_rollout_equals_sequential_pushes(torch, all_done_at, use_flags):
    """n = 96, T = 5 into a ring of 200 that already holds 150 rows: it wraps, and more is appended than fits."""
    from merging_gym import RainbowReplay

    n, T, cap = 96, 5, 200
    rng = np.random.default_rng(5)
    obs_first = rng.normal(size=(n, 10)).astype(np.float32)
    obs = rng.normal(size=(T, n, 10)).astype(np.float32)
    final_obs = rng.normal(size=(T, n, 10)).astype(np.float32)
    a1 = rng.integers(0, 5, (T, n)).astype(np.int8)
    rew = rng.normal(size=(T, n, 2)).astype(np.float32)
    done = (rng.random((T, n)) < 0.2).astype(np.uint8)
    if all_done_at is not None:
        done[all_done_at] = 1
    rp = RainbowReplay(cap, device=DEV)
    want = np.zeros((cap, 24), np.float32)
    first = rng.normal(size=(150, 24)).astype(np.float32)
    want[:150] = first
    rp.memory[:150].copy_(torch.from_numpy(first))
    rp._counter.fill_(150)
    assert len(rp) == 150
    dev = lambda x: torch.from_numpy(x).to(DEV)  # noqa: E731
    if use_flags:
        flags = np.zeros((T, n, 4), np.uint8)
        flags[..., 0], flags[..., 1], flags[..., 2] = a1.view(np.uint8), 9, done
        traj = {"obs": dev(obs), "rew": dev(rew), "a1": None, "done": None, "final_observation": dev(final_obs),
                "flags": dev(flags)}
    else:
        traj = {"obs": dev(obs), "rew": dev(rew), "a1": dev(a1), "done": dev(done), "final_observation": dev(final_obs)}
    rp.store_rollout(dev(obs_first), traj)
    counter = _emulate_pushes(want, 150, obs_first, obs, a1, rew, done, final_obs)
    assert int(rp._counter.item()) == counter == 150 + n * T and len(rp) == cap
    assert np.array_equal(bits(rp.memory.cpu().numpy()), bits(want))
    # push, the reference's single call, through the same kernel
    rp.push(list(obs_first[0]), 3, 1.5, list(obs[0, 0]), True)
    counter = _emulate_pushes(want, counter, obs_first[:1], obs[:1, :1], np.array([[3]], np.int8),
                              np.array([[[1.5, 0.0]]], np.float32), np.array([[1]], np.uint8), None)
    assert np.array_equal(bits(rp.memory.cpu().numpy()), bits(want)) and int(rp._counter.item()) == counter
    # sample: the five arrays at mg_replay_sample's slots, every row a stored one
    s, a, r, s2, d = rp.sample(32, seed=4, draw=9)
    assert (tuple(s.shape), tuple(a.shape), tuple(r.shape), tuple(s2.shape), tuple(d.shape)) == (
        (32, 10), (32,), (32,), (32, 10), (32,)) and a.dtype == torch.int64
    stored = {row.tobytes() for row in want}
    assert all(row.tobytes() in stored for row in rp.sample_rows(32, seed=4, draw=9).cpu().numpy())
    back = RainbowReplay(cap, device=DEV)
    back.load_state_dict(rp.state_dict())
    assert torch.equal(back.memory, rp.memory) and torch.equal(back._counter, rp._counter)


def test_acting_net_follows_the_learned_weights(torch):
    from merging_gym import RainbowNet

    ring, c = R.ring_case(64, 200)
    lr = _learner(torch, "soft", ring, c, 32)
    fresh = lambda: RainbowNet.from_state_dict(lr.current_state_dict(), device=DEV).packed  # noqa: E731
    before = lr.net.packed.clone()
    assert torch.equal(before, fresh())
    lr.learn(1)
    assert torch.equal(lr.net.packed, fresh())
    assert not torch.equal(lr.net.packed, before)
    # the host-side state is refreshed on access, never stale
    sd = lr.current_state_dict()
    assert all(torch.equal(lr.net.state[k], sd[k].cpu()) for k in sd)
    obs = torch.from_numpy(ring[:40, :10].copy()).to(DEV)
    q, act = lr.net.forward(obs)
    q2, act2 = RainbowNet.from_state_dict(sd, device=DEV).forward(obs)
    assert torch.equal(q, q2) and torch.equal(act, act2)


def test_resume_is_bit_identical(torch):
    ring, c = R.ring_case(64, 200)
    straight = _learner(torch, "soft", ring, c, 32)
    straight.learn(1)
    ck = {k: (v.clone() if hasattr(v, "clone") else v) for k, v in straight.state_dict().items()}
    resumed = _learner(torch, "default", ring, c, 32, seed=99, noise_seed=5)
    resumed.load_state_dict(ck)
    assert torch.equal(resumed.net.packed, straight.net.packed)
    a = straight.learn(2, return_loss=True)
    b = resumed.learn(2, return_loss=True)
    assert torch.equal(a.view(torch.int32), b.view(torch.int32))
    assert torch.equal(straight._buf.view(torch.int32), resumed._buf.view(torch.int32))
    assert torch.equal(straight.net.packed, resumed.net.packed)
    assert (resumed.learn_step_counter, resumed.draw_counter) == (3, 3)


def test_closed_loop_at_256_envs(torch):
    """rollout_rainbow, store_rollout, learn(2), then a rollout with learner.net from an env checkpoint equals the
    rollout of a fresh RainbowNet built from current_state_dict(), field for field."""
    from merging_gym import MergeVecEnv, RainbowLearner, RainbowNet, RainbowReplay

    n = 256
    env = MergeVecEnv(n, device=DEV, won_mask=True)
    env.reset()
    replay = RainbowReplay(10000, device=DEV)
    lr = RainbowLearner(R.golden_state(1, "soft"), replay, seed=1, generator=torch.Generator().manual_seed(2),
                        device=DEV)
    obs0 = env.observe().clone()
    traj = env.rollout_rainbow(8, lr.net)
    replay.store_rollout(obs0, traj)
    assert len(replay) == 8 * n
    loss = lr.learn(2, return_loss=True)
    assert torch.isfinite(loss).all()
    ck = env.state_dict()
    got = {k: v.clone() for k, v in env.rollout_rainbow(16, lr.net).items() if v is not None}
    env.load_state_dict(ck)
    fresh = RainbowNet.from_state_dict(lr.current_state_dict(), device=DEV)
    want = env.rollout_rainbow(16, fresh)
    for k, v in got.items():
        same = torch.equal(torch.nan_to_num(v, nan=7.0), torch.nan_to_num(want[k], nan=7.0)) if v.is_floating_point() \
            else torch.equal(v, want[k])
        assert same, k
