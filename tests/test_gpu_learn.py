"""DQN.learn on the GPU (ABI 21): mg_dqn_learn through merging_gym.DQNLearner against the plain-C
restatement bit for bit, its determinism and bookkeeping, and the closed acting / storing / learning
loop of scripts/main.py:189-220."""

import functools

import numpy as np
import pytest

import learn_ref as lr

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ring(rows, counter):
    import torch

    from merging_gym import ReplayRing

    ring = ReplayRing(rows.shape[0], device=DEV, goal=rows.shape[1] == 24)
    ring.memory.copy_(torch.as_tensor(rows))
    ring._counter.fill_(int(counter))
    return ring


def _learner(sd, ring, batch=128, **kw):
    from merging_gym import DQNLearner

    return DQNLearner(sd, ring, batch_size=batch, **kw)


def _blocks(learner):
    return learner._buf.cpu().numpy().reshape(4, -1)


@functools.lru_cache(maxsize=None)
def _reference(in_dim, out_dim, batch, filled_only):
    """The restatement's run of a bit-exact case, computed once: three updates with target_period 2
    from update 1 on a half-filled ring, the target net starting at half the eval net."""
    rows, sd = lr.case_fixture(in_dim, out_dim, batch)
    ring, counter = lr.half_filled(rows)
    L0 = lr.learner_array(sd)
    L0[1] *= np.float32(0.5)
    ref = lr.run_ref(L0, ring, counter, in_dim, out_dim, batch, 3, first_update=1, seed=7, first_draw=5,
                     filled_only=filled_only, target_period=2)
    return sd, ring, counter, ref


@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch", lr.CASES)
def test_device_learn_equals_restatement_bit_for_bit(in_dim, out_dim, batch, filled_only):
    sd, ring_np, counter, (ref, ref_loss, ref_rows, _) = _reference(in_dim, out_dim, batch, filled_only)
    learner = _learner(sd, _ring(ring_np, counter), batch, seed=7, target_period=2)
    learner._buf[learner._P:2 * learner._P] *= 0.5
    learner.learn_step_counter, learner.draw_counter = 1, 5
    loss, rows = learner.learn(3, filled_only=filled_only, return_loss=True, return_rows=True)
    got = _blocks(learner)
    assert np.array_equal(lr.bits(rows.cpu().numpy()), lr.bits(ref_rows))
    assert np.array_equal(lr.bits(loss.cpu().numpy()), lr.bits(ref_loss)), (loss, ref_loss)
    for blk, name in enumerate(("eval", "target", "m", "v")):
        bad = lr.bits(got[blk]) != lr.bits(ref[blk])
        assert not bad.any(), (name, int(bad.sum()), float(np.abs(got[blk] - ref[blk]).max()))
    assert (learner.learn_step_counter, learner.draw_counter) == (4, 8)


def _full_case(batch=128):
    rows, sd = lr.case_fixture(10, 5, batch)
    return sd, rows


def test_k_updates_in_one_call_equal_k_calls_and_two_runs_are_identical():
    import torch

    sd, rows = _full_case()
    runs = []
    for split in (False, False, True):
        learner = _learner(sd, _ring(rows, rows.shape[0]), seed=11, target_period=3)
        if split:
            loss = torch.cat([learner.learn(1, return_loss=True) for _ in range(5)])
        else:
            loss = learner.learn(5, return_loss=True)
        runs.append((learner._buf.clone(), loss.clone(), learner.qnet.packed.clone()))
    for other in runs[1:]:
        for a, b in zip(runs[0], other):
            assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    assert bool(torch.isfinite(runs[0][1]).all())


def test_rows_out_are_the_rings_samples():
    import torch

    sd, rows = _full_case(32)
    ring = _ring(*lr.half_filled(rows))
    for filled_only in (False, True):
        learner = _learner(sd, ring, 32, seed=1234)
        learner.draw_counter = 40
        _, got = learner.learn(3, filled_only=filled_only, return_loss=True, return_rows=True)
        for u in range(3):
            want = ring.sample_rows(32, seed=1234, draw=40 + u, filled_only=filled_only)
            assert torch.equal(got[u], want), (filled_only, u)


def test_packed_net_is_the_eval_nets_packing():
    import torch

    from merging_gym.policy import QNet

    sd, rows = _full_case()
    learner = _learner(sd, _ring(rows, rows.shape[0]))
    before = learner.qnet.packed.clone()
    assert torch.equal(before, QNet.from_state_dict(sd, device=DEV).packed)
    learner.learn(2)
    fresh = QNet.from_state_dict(learner.eval_state_dict(), device=DEV)
    assert torch.equal(learner.qnet.packed, fresh.packed) and not torch.equal(learner.qnet.packed, before)
    for a, b in zip(learner.qnet.fp32, fresh.fp32):
        assert torch.equal(a, b)
    # both dicts load into the reference's Net
    for d in (learner.eval_state_dict(), learner.target_state_dict()):
        assert list(d) == list(lr.KEYS) and d["fc1.weight"].shape == (200, 10) and d["out.bias"].shape == (5,)
    # the target is still the initial net: no copy fell after update 0
    assert torch.equal(learner.target_state_dict()["fc2.weight"].cpu(), torch.as_tensor(sd["fc2.weight"]))


def test_resume_from_a_state_dict_is_bit_identical():
    import torch

    from merging_gym.policy import QNet

    sd, rows = _full_case(96)
    ring = _ring(rows, rows.shape[0])
    straight = _learner(sd, ring, 96, seed=5, target_period=3)
    straight.learn(2)
    saved = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in straight.state_dict().items()}
    straight.learn(3)
    resumed = _learner(lr.seeded_net(10, 5, 99), ring, 96, seed=0, target_period=3)
    resumed.load_state_dict(saved)
    assert torch.equal(resumed.qnet.packed, QNet.from_state_dict(saved_eval(saved, straight), device=DEV).packed)
    resumed.learn(3)
    assert torch.equal(resumed._buf.view(torch.int32), straight._buf.view(torch.int32))
    assert torch.equal(resumed.qnet.packed, straight.qnet.packed)
    assert (resumed.learn_step_counter, resumed.draw_counter) == (5, 5)


def saved_eval(saved, learner):
    """The eval net inside a saved learner state, as a state dict."""
    flat = saved["learner"][:learner._P].numpy()
    return lr.split(flat, learner.in_dim, learner.out_dim)


def test_closed_loop_acts_with_the_learned_weights():
    """main.py:189-220 on the device at 256 envs: rollout_qnet -> store_rollout until the 2000-row
    ring is full -> learn(4) -> rollout_qnet with learner.qnet. The second rollout equals the one a
    fresh QNet built from eval_state_dict() produces from the same env checkpoint."""
    import torch

    from merging_gym import DQNLearner, MergeVecEnv, ReplayRing
    from merging_gym.policy import QNet

    env = MergeVecEnv(256, device=DEV)
    env.reset()
    ring = ReplayRing(2000, device=DEV)
    learner = DQNLearner(QNet.from_state_dict(lr.trained_net("l3"), device=DEV), ring)
    packed0 = learner.qnet.packed.clone()
    for _ in range(8):
        obs0 = env.observe().clone()
        traj = env.rollout_qnet(16, learner.qnet, seed=21)
        ring.store_rollout(obs0, traj)
        if ring.memory_counter >= ring.capacity:
            break
    assert ring.memory_counter >= ring.capacity
    loss = learner.learn(4, return_loss=True)
    assert bool(torch.isfinite(loss).all()) and not torch.equal(learner.qnet.packed, packed0)
    ckpt = env.state_dict()
    first = env._step_idx
    keys = ("obs", "rew", "flags", "final_observation", "won_mask")
    traj = env.rollout_qnet(16, learner.qnet, seed=21)
    got = {k: traj[k].clone() for k in keys}  # the env reuses its trajectory buffers
    env.load_state_dict(ckpt)
    fresh = QNet.from_state_dict(learner.eval_state_dict(), device=DEV)
    want = env.rollout_qnet(16, fresh, seed=21, first_step=first)
    for k in keys:
        a, b = got[k], want[k]
        if a.dtype.is_floating_point:  # final_observation is NaN where no episode ended
            a, b = a.view(torch.int32), b.view(torch.int32)
        assert torch.equal(a, b), k
