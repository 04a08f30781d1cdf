"""DQN.learn on the GPU at every accepted width (tests/width_cases.py): mg_dqn_learn and mg_dqn_learn_many
through merging_gym.DQNLearner and DQNPopulation against the plain-C restatement bit for bit, on rows whose
action column the reference's gather would raise on; the learned weights in both packed layouts and through
mg_qnet_forward against the oracle's MFMA model; the resume; and one fused rollout with a two-output net, whose
greedy choice must never come from a padding column."""

import numpy as np
import pytest

import learn_many_ref as mr
import learn_ref as lr
import merge_oracle as mo
import width_cases as wc
from test_gpu_learn_many import _blocks as _pop_blocks
from test_gpu_learn_many import _lone, _population, _same
from test_gpu_qnet import ALWAYS, _rollout_qnet_policy_and_transitions

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ring(rows, counter):
    """A bare ring of any row width: the learners read only row, memory, _counter, capacity and device."""
    import torch

    from merging_gym._base import RingBase

    ring = RingBase(rows.shape[0], rows.shape[1], DEV)
    ring.memory.copy_(torch.as_tensor(np.array(rows)))  # a copy: the shared fixtures are read-only
    ring._counter.fill_(int(counter))
    return ring


def _learner(sd, ring, batch, **kw):
    from merging_gym import DQNLearner

    return DQNLearner(sd, ring, batch_size=batch, **kw)


def _run_case(in_dim, out_dim, batch, filled_only):
    """The learner after wc.SEQUENCE from wc.reference's start, with what the call returned and the reference."""
    import torch

    sd, ring_np, counter, L0, ref = wc.reference(in_dim, out_dim, batch, filled_only)
    learner = _learner(sd, _ring(ring_np, counter), batch, seed=wc.SEQUENCE["seed"],
                       target_period=wc.SEQUENCE["target_period"])
    assert (learner.in_dim, learner.out_dim, learner._P) == (in_dim, out_dim, lr.num_params(in_dim, out_dim))
    learner._buf.copy_(torch.as_tensor(np.array(L0)).reshape(-1))
    learner.learn_step_counter, learner.draw_counter = wc.SEQUENCE["first_update"], wc.SEQUENCE["first_draw"]
    loss, rows = learner.learn(wc.SEQUENCE["num_updates"], filled_only=filled_only, return_loss=True, return_rows=True)
    return learner, loss, rows, ref


# ------------------------------------------------------------------ 1. device == restatement
@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch", wc.LEARN_CASES)
def test_device_learn_equals_restatement_at_every_width(in_dim, out_dim, batch, filled_only):
    learner, loss, rows, (ref, ref_loss, ref_rows, _) = _run_case(in_dim, out_dim, batch, filled_only)
    got = learner._buf.cpu().numpy().reshape(4, -1)
    assert np.array_equal(lr.bits(rows.cpu().numpy()), lr.bits(ref_rows))
    assert np.array_equal(lr.bits(loss.cpu().numpy()), lr.bits(ref_loss)), (loss, ref_loss)
    for blk, name in enumerate(("eval", "target", "m", "v")):
        bad = lr.bits(got[blk]) != lr.bits(ref[blk])
        assert not bad.any(), (name, int(bad.sum()), float(np.abs(got[blk] - ref[blk]).max()))
    assert (learner.learn_step_counter, learner.draw_counter) == (4, 8)


# ------------------------------------------------------------------ 2. the learned weights act
@pytest.mark.parametrize("in_dim,out_dim,batch", wc.LEARN_CASES)
def test_learned_weights_act_at_every_width(in_dim, out_dim, batch):
    """After the call the acting net is the eval net: both packed layouts (packed_out, written by the pack
    kernels' member forms) equal mg_qnet_pack of eval_state_dict(), and mg_qnet_forward on the first minibatch's
    states equals the oracle's MFMA model of that state dict, every bit."""
    import torch

    from merging_gym.policy import QNet

    learner, _, rows, (ref, _, _, _) = _run_case(in_dim, out_dim, batch, False)
    sd = learner.eval_state_dict()
    assert list(sd) == list(lr.KEYS)
    assert [tuple(sd[k].shape) for k in lr.KEYS] == [(200, in_dim), (200,), (100, 200), (100,), (out_dim, 100),
                                                     (out_dim,)]
    sd_np = {k: v.cpu().numpy() for k, v in sd.items()}
    want = lr.split(ref[0], in_dim, out_dim)
    for k in lr.KEYS:
        assert np.array_equal(lr.bits(sd_np[k]), lr.bits(want[k])), k
    fresh = QNet.from_state_dict(sd, device=DEV)
    before = QNet.from_state_dict(wc.width_net(in_dim, out_dim), device=DEV)
    assert torch.equal(learner.qnet.packed, fresh.packed) and not torch.equal(learner.qnet.packed, before.packed)
    states = rows[0][:, :in_dim].contiguous()
    q = learner.qnet.forward(states).cpu().numpy()
    model = mo.qnet_reference_mfma(sd_np, states.cpu().numpy())
    assert q.shape == (batch, out_dim) and np.array_equal(q.view(np.uint32), model.view(np.uint32))


# ------------------------------------------------------------------ 3. the population
@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch,members,updates", [(13, 8, 9, 3, mr.UPDATES), (1, 1, 1, 2, mr.UPDATES),
                                                                  (10, 8, 33, 64, 2)])
def test_population_equals_lone_learners_and_restatement_at_other_widths(in_dim, out_dim, batch, members, updates,
                                                                         filled_only):
    """Members that differ in ring, counter, seed, hyperparameters, first_update and first_draw
    (tests/learn_many_ref.py): every member equals its lone DQNLearner bit for bit -- blocks, losses, rows, both
    packed layouts, counters -- and the restatement's run of it (at 64 members: the first and the last)."""
    import torch

    sd, rings, counters, kws, L0 = wc.members_setup(in_dim, out_dim, members)
    dev_rings = [_ring(r, c) for r, c in zip(rings, counters)]
    pop = _population(sd, dev_rings, kws, batch, L0)
    loss, rows = pop.learn(updates, filled_only=filled_only, return_loss=True, return_rows=True)
    assert tuple(loss.shape) == (updates, members) and tuple(rows.shape) == (updates, members, batch, 2 * in_dim + 2)
    for m in range(members):
        lone = _lone(sd, dev_rings[m], kws[m], batch)
        lone._buf.copy_(torch.as_tensor(np.array(L0[m])).reshape(-1))
        lone.learn_step_counter, lone.draw_counter = kws[m]["first_update"], kws[m]["first_draw"]
        l1, r1 = lone.learn(updates, filled_only=filled_only, return_loss=True, return_rows=True)
        assert _same(loss[:, m], l1) and _same(rows[:, m], r1), m
        assert _same(pop._buf[m], lone._buf) and _same(pop.qnets[m].packed, lone.qnet.packed), m
        assert (pop.learn_step_counter[m], pop.draw_counter[m]) == (lone.learn_step_counter, lone.draw_counter)
    which = list(range(members)) if members <= 3 else [0, members - 1]
    ref_end, ref_loss, ref_rows = wc.members_reference(in_dim, out_dim, batch, members, filled_only, updates,
                                                       tuple(which))
    mr.assert_members_equal(_pop_blocks(pop)[which], loss.cpu().numpy()[:, which], rows.cpu().numpy()[:, which],
                            ref_end, ref_loss, ref_rows)
    assert pop.learn_step_counter == [kw["first_update"] + updates for kw in kws]
    assert bool(torch.isfinite(pop._buf).all()) and bool(torch.isfinite(loss).all())


# ------------------------------------------------------------------ 4. resume
def test_resume_is_bit_identical_at_13_to_8_and_refused_by_another_width():
    import torch

    from merging_gym.policy import QNet

    sd, ring_np, counter, _, _ = wc.reference(13, 8, 33, False)
    ring = _ring(ring_np, counter)
    straight = _learner(sd, ring, 33, seed=5, target_period=3)
    straight.learn(2)
    saved = {k: (v.cpu() if isinstance(v, torch.Tensor) else v) for k, v in straight.state_dict().items()}
    assert (saved["in_dim"], saved["out_dim"]) == (13, 8)
    straight.learn(3)
    resumed = _learner(lr.seeded_net(13, 8, 99), ring, 33, seed=0, target_period=3)
    resumed.load_state_dict(saved)
    eval_saved = lr.split(saved["learner"][:straight._P].numpy(), 13, 8)
    assert torch.equal(resumed.qnet.packed, QNet.from_state_dict(eval_saved, device=DEV).packed)
    resumed.learn(3)
    assert torch.equal(resumed._buf.view(torch.int32), straight._buf.view(torch.int32))
    assert torch.equal(resumed.qnet.packed, straight.qnet.packed)
    assert (resumed.learn_step_counter, resumed.draw_counter) == (5, 5)

    other = _learner(wc.width_net(12, 7), _ring(*lr.half_filled(wc.width_rows(12, 7, wc.CAPACITY, True))), 33)
    kept = other._buf.clone()
    with pytest.raises(ValueError, match="expected the state of a 12 -> 7 learner"):
        other.load_state_dict(saved)
    assert torch.equal(other._buf.view(torch.int32), kept.view(torch.int32)) and other.learn_step_counter == 0


# ------------------------------------------------------------------ 5. one rollout at a narrow width
def test_rollout_qnet_with_a_two_output_net_never_picks_a_padding_column(coracle):
    """A 10 -> 2 net from output rows 0 and 2 of the shipped checkpoint l1 with 100 taken off both biases: every Q
    is negative, so an argmax that looked at a zero padding column (2..7) would pick it. 577 envs x 8 steps
    without an opponent (the 32x32 layout), every clock three steps short of the timeout so that episodes end
    and q_eval is logged, checked by tests/test_gpu_qnet.py's checker as it stands. That checker indexes the
    net's Q row with every action taken, and a random action (0..4) would fall outside a two-column row: the
    ego's threshold is therefore 2^32 -- every action greedy, which the returned masks confirm -- and the
    checker then requires each action to be the argmax of the oracle MFMA model's two columns. Actions 0 and 1
    drive the env as its own actions 0 and 1."""
    import torch

    l1 = lr.trained_net("l1")
    sd = {k: np.ascontiguousarray(v[[0, 2]] if k.startswith("out.") else v, dtype=np.float32) for k, v in l1.items()}
    sd["out.bias"] = (sd["out.bias"] - np.float32(100.0)).astype(np.float32)
    assert sd["out.weight"].shape == (2, 100) and sd["out.bias"].shape == (2,)
    nets = {"l1": sd, "l3": sd}
    info = _rollout_qnet_policy_and_transitions(torch, coracle, nets, "none", 577, True, T=8, episilo=ALWAYS)
    assert info["g1"].all() and info["g1"].shape == (8, 577)
