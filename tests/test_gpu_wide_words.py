"""The device's streams, counters and long stores at 64-bit values. Every other GPU test keys its draws with seeds,
draw and step indices below 2^32, starts its rings at a counter of a few thousand and stores at most six groups
of write blocks, so the high key and counter words of every Philox call site, the ring arithmetic past 2^32 and
replay_group_scan's carry (csrc/mg_replay.h) run with zeros there. Here: each kernel that draws against its CPU
restatement at seeds, draws, steps and env indices whose 32-bit halves are all non-zero; every ring kind with a
memory_counter that crosses 2^32; stores of 66, 71 and 1,025 groups. Every comparison is exact."""

import io

import numpy as np
import pytest

import learn_ref as lr
import merge_oracle as mo
import rainbow_learn_ref as R
import wide_words as W

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
BATCH = 33


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


def _dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ------------------------------------------------------------------ B. the device streams
@pytest.mark.parametrize("opp", [True, False], ids=["both-random", "opponent-none"])
def test_step_and_rollout_random_at_wide_seed_step_and_env_index(torch, coracle, opp):
    """mg_step_random and mg_rollout_random (philox_block: counter (env, step div 8), key seed) with a high word in
    the env index, in step div 8 and in the seed. Six steps from 2^36 + 11: both parities, and step div 8 moves on
    at the sixth. Actions equal the C oracle's and the NumPy oracle's; the final state equals the C oracle's
    rollout; the fused rollout equals the step sequence."""
    import merge_numpy as mn
    from merging_gym import MergeVecEnv

    n, T, seed, k0, off = 300, 6, W.SEED_TOP, W.STEP_W, W.ENV_OFF_W
    a = MergeVecEnv(n, device=DEV, env_offset=off)
    b = MergeVecEnv(n, device=DEV, env_offset=off)
    traj = {k: v.clone() for k, v in b.rollout_random(T, seed, opponent_random=opp, first_step=k0).items()
            if v is not None}
    gidx = np.arange(n, dtype=np.uint64) + np.uint64(off)
    seen = set()
    for t in range(T):
        obs, rew, done, info = a.step_random(seed, opponent_random=opp, step_idx=k0 + t)
        a1, a2 = coracle.random_actions(n, off, seed, k0 + t, opp)
        n1, n2 = mn.random_actions(gidx, seed, k0 + t, opp)
        assert np.array_equal(a1, n1) and np.array_equal(a2, n2), t
        assert np.array_equal(a.a1_buf.cpu().numpy(), a1) and np.array_equal(a.a2_buf.cpu().numpy(), a2), t
        assert torch.equal(traj["a1"][t], a.a1_buf) and torch.equal(traj["a2"][t], a.a2_buf), t
        assert torch.equal(traj["obs"][t], obs) and torch.equal(traj["rew"][t], rew), t
        assert torch.equal(traj["done"][t], done) and torch.equal(traj["collision"][t], info["collision"]), t
        seen |= set(a1.tolist())
        # not the stream of the low words alone
        assert not np.array_equal(a1, coracle.random_actions(n, off, seed & 0xFFFFFFFF, k0 + t, opp)[0])
        assert not np.array_equal(a1, coracle.random_actions(n, off, seed, (k0 + t) & 0xFFFFFFFF, opp)[0])
        assert not np.array_equal(a1, coracle.random_actions(n, off & 0xFFFFFFFF, seed, k0 + t, opp)[0])
    assert seen == {0, 1, 2, 3, 4}
    e = coracle.new_envs(n)
    coracle.reset(e)
    coracle.rollout_random(e, T, seed, k0, opp, env_offset=off)
    for env in (a, b):
        for name, src in (("pos1", env.p1), ("pos2", env.p2), ("vel1", env.v1), ("vel2", env.v2), ("r1_acc", env.ret1),
                          ("r2_acc", env.ret2)):
            assert np.array_equal(src.cpu().numpy(), e[name]), name
        assert env._step_idx == k0 + T
    for name in ("tf", "returns", "counts", "_ep_stats"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name


@pytest.mark.parametrize("opponent", ["none", "uniform", "self"])
def test_rollout_qnet_draws_at_wide_seed_and_step(torch, coracle, opponent):
    """mg_rollout_qnet's epsilon-greedy stream (oracle.merge_oracle.qnet_policy_draws, the restatement
    tests/test_gpu_qnet.py uses) at seed SEED_W from step 2^36 + 11, EPISILO 0.7 (P(greedy) = 0.758): every action
    is the random pick where the draw explores and the argmax of the oracle's MFMA model of the forward where it
    does not -- no excusal -- for "none" and "uniform" (the OPP < 2 draw: call step div 2, so step >> 33 is live)
    and for "self" (philox_env_step per step, the opponent's draws exact too). The env index has a high word
    too (env_offset 2^33 + 5)."""
    from merging_gym import MergeVecEnv
    from merging_gym.policy import QNet, greedy_threshold

    n, T, seed, k0, off = 577, 6, W.SEED_W, W.STEP_W, W.ENV_OFF_W
    sd = lr.trained_net("l1")
    qnet = QNet.from_state_dict(sd, device=DEV)
    env = MergeVecEnv(n, device=DEV, env_offset=off)  # a shard whose global env indices exceed 2^32
    for k in range(60):  # scattered mid-episode states: the greedy choice varies from env to env
        env.step_random(5, step_idx=k)
    obs_in = env.observe().cpu().numpy().copy()
    traj = env.rollout_qnet(T, qnet, seed, opponent=opponent, first_step=k0)
    a1, a2, obs = (traj[k].cpu().numpy() for k in ("a1", "a2", "obs"))
    thr = greedy_threshold(0.7)
    form = "16x16" if opponent == "self" else "32x32"
    words = lambda c: coracle.philox_batch(n, off, seed, c)  # noqa: E731
    explored = greedy_n = moved = 0
    for t in range(T):
        ex, rnd1, ex2, rnd2 = mo.qnet_policy_draws(words, k0 + t, opponent)
        greedy = ex < thr
        best = mo.qnet_reference_mfma(sd, obs_in, form=form).argmax(1)
        assert np.array_equal(a1[t], np.where(greedy, best, rnd1)), t
        explored += int((~greedy).sum())
        greedy_n += int(greedy.sum())
        moved += int((rnd1 != best)[~greedy].sum())
        if opponent == "none":
            assert (a2[t] == -1).all()
        elif opponent == "uniform":
            assert np.array_equal(a2[t], rnd2), t
        else:
            g2 = ex2 < thr
            best2 = mo.qnet_reference_mfma(sd, obs_in, swap=True).argmax(1)
            assert np.array_equal(a2[t], np.where(g2, best2, rnd2)), t
            assert g2.any() and not g2.all()
        for o, s in ((off, seed & 0xFFFFFFFF), (off & 0xFFFFFFFF, seed)):  # not the low words' stream
            low = mo.qnet_policy_draws(lambda c: coracle.philox_batch(n, o, s, c), k0 + t, opponent)
            assert not np.array_equal(low[0], ex)
        obs_in = obs[t]
    # both branches ran, and exploring changed actions
    assert explored > n and greedy_n > 3 * n and moved > n // 2, (explored, greedy_n, moved)
    assert env._step_idx == k0 + T


@pytest.mark.parametrize("opponent", ["uniform", "self"])
def test_rollout_hdqn_streams_at_wide_seed_and_step(coracle, opponent):
    """mg_rollout_hdqn against tests/test_gpu_hdqn.py's restatement of its loop, unchanged, at seed SEED_W from
    step 2^36 + 11: the ego's stream (env, step), the fresh-goal stream (env ^ 2^63; "uniform" draws it per step and
    reads the opponent's action from it) and the self-play opponent's stream (env ^ 2^62), whose draws the
    restatement takes from the C oracle's Philox with the same 64-bit counters. Two launches of 16 steps from step
    208 of the episodes, so goals are reached and episodes end inside them."""
    from test_gpu_hdqn import _fused_hdqn_rollout

    _fused_hdqn_rollout(coracle, 577, opponent, T=16, seed=W.SEED_W, burn=208, first_step=W.STEP_W)


def _arange_ring(torch, cls, cap, counter, **kw):
    ring = cls(cap, device=DEV, **kw)
    ring.memory.copy_(torch.arange(cap * ring.row, dtype=torch.float32, device=DEV).view(cap, ring.row))
    ring._counter.fill_(counter)
    return ring


@pytest.mark.parametrize("counter", [1234, W.COUNTER_ABOVE], ids=["partly-filled", "counter-above-2^32"])
@pytest.mark.parametrize("filled_only", [False, True])
def test_sample_rows_at_wide_seed_and_draw(torch, coracle, filled_only, counter):
    """replay_sample_kernel: both key words and both words of the draw; with filled_only it draws among
    min(counter, capacity) rows of a 64-bit counter (2^32 + 17: its low word alone would leave 17 rows)."""
    from merging_gym import ReplayRing

    cap = 2000
    ring = _arange_ring(torch, ReplayRing, cap, counter)
    rows, idx = ring.sample_rows(4096, seed=W.SEED_W, draw=W.DRAW_W, filled_only=filled_only, return_index=True)
    want = mo.replay_sample_index(coracle, cap, counter, W.SEED_W, W.DRAW_W, 4096, filled_only)
    assert np.array_equal(idx.cpu().numpy(), want)
    assert np.array_equal(rows.cpu().numpy(), ring.memory.cpu().numpy()[want])
    for s, d in ((W.SEED_W & 0xFFFFFFFF, W.DRAW_W), (W.SEED_W, W.DRAW_W & 0xFFFFFFFF)):
        assert not np.array_equal(want, mo.replay_sample_index(coracle, cap, counter, s, d, 4096, filled_only))


def test_rainbow_sample_rows_at_wide_seed_and_draw(torch, coracle):
    from merging_gym import RainbowReplay

    cap, counter = 2000, 1234
    rp = _arange_ring(torch, RainbowReplay, cap, counter)
    rows = rp.sample_rows(4096, seed=W.SEED_W, draw=W.DRAW_W)
    want = mo.replay_sample_index(coracle, cap, counter, W.SEED_W, W.DRAW_W, 4096, True)
    assert np.array_equal(rows.cpu().numpy(), rp.memory.cpu().numpy()[want])
    rows = rp.sample_rows(4096, seed=W.SEED_MAX, draw=W.DRAW_MAX)
    want = mo.replay_sample_index(coracle, cap, counter, W.SEED_MAX, W.DRAW_MAX, 4096, True)
    assert np.array_equal(rows.cpu().numpy(), rp.memory.cpu().numpy()[want])


def _dqn_ring(torch, rows, counter):
    from merging_gym import ReplayRing

    ring = ReplayRing(rows.shape[0], device=DEV)
    ring.memory.copy_(torch.as_tensor(rows))
    ring._counter.fill_(int(counter))
    return ring


def _rainbow_replay(torch, ring, counter):
    from merging_gym import RainbowReplay

    rp = RainbowReplay(len(ring), device=DEV)
    rp.memory.copy_(torch.from_numpy(ring))
    rp._counter.fill_(int(counter))
    return rp


def _reload(torch, sd):
    """A checkpoint through torch.save / torch.load, as a resumed run reads it."""
    buf = io.BytesIO()
    torch.save(sd, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=True)


@pytest.mark.parametrize("filled_only", [False, True])
def test_dqn_learner_at_wide_seed_and_draw(torch, filled_only):
    """DQNLearner(seed=SEED_W) with draw_counter 2^40 + 3, batch 33, learn(2): compared as
    test_gpu_learn.py's test_device_learn_equals_restatement_bit_for_bit compares; the counters read back exactly
    and survive a saved state_dict."""
    from merging_gym import DQNLearner

    rows, sd = lr.case_fixture(10, 5, 32)
    ring_np, counter = lr.half_filled(rows)
    ref, ref_loss, ref_rows, _ = lr.run_ref(lr.learner_array(sd), ring_np, counter, 10, 5, BATCH, 2, seed=W.SEED_W,
                                            first_draw=W.DRAW_W, filled_only=filled_only)
    ring = _dqn_ring(torch, ring_np, counter)
    learner = DQNLearner(sd, ring, batch_size=BATCH, seed=W.SEED_W)
    learner.draw_counter = W.DRAW_W
    loss, got_rows = learner.learn(2, filled_only=filled_only, return_loss=True, return_rows=True)
    got = learner._buf.cpu().numpy().reshape(4, -1)
    assert np.array_equal(lr.bits(got_rows.cpu().numpy()), lr.bits(ref_rows))
    assert np.array_equal(lr.bits(loss.cpu().numpy()), lr.bits(ref_loss)), (loss, ref_loss)
    for blk, name in enumerate(("eval", "target", "m", "v")):
        bad = lr.bits(got[blk]) != lr.bits(ref[blk])
        assert not bad.any(), (name, int(bad.sum()), float(np.abs(got[blk] - ref[blk]).max()))
    assert (learner.learn_step_counter, learner.draw_counter, learner.seed) == (2, W.DRAW_W + 2, W.SEED_W)
    saved = _reload(torch, learner.state_dict())
    assert (saved["draw_counter"], saved["seed"]) == (W.DRAW_W + 2, W.SEED_W)
    resumed = DQNLearner(lr.seeded_net(10, 5, 99), ring, batch_size=BATCH, seed=0)
    resumed.load_state_dict(saved)
    assert (resumed.learn_step_counter, resumed.draw_counter, resumed.seed) == (2, W.DRAW_W + 2, W.SEED_W)
    a = learner.learn(1, filled_only=filled_only, return_rows=True)
    b = resumed.learn(1, filled_only=filled_only, return_rows=True)
    assert torch.equal(a, b) and torch.equal(learner._buf.view(torch.int32), resumed._buf.view(torch.int32))


def test_rainbow_learner_at_wide_seed_and_draw(torch):
    from merging_gym import RainbowLearner

    ring, c = R.ring_case(64, 200)
    want = R.run_ref(R.learner_numpy(R.golden_state(1, "default")), ring, c, BATCH, 2, 0, W.SEED_W, W.DRAW_W, R.noise(2))
    rp = _rainbow_replay(torch, ring, c)
    learner = RainbowLearner(R.golden_state(1, "default"), rp, batch_size=BATCH, seed=W.SEED_W,
                             generator=torch.Generator().manual_seed(11), device=DEV)
    learner.draw_counter = W.DRAW_W
    out = [t.cpu().numpy() for t in learner.learn(2, return_loss=True, return_rows=True, return_proj=True,
                                                  return_grads=True)]
    R.assert_same((learner._buf.cpu().numpy(), out), (want[0], list(want[1:])))
    assert (learner.learn_step_counter, learner.draw_counter, learner.seed) == (2, W.DRAW_W + 2, W.SEED_W)
    saved = _reload(torch, learner.state_dict())
    assert (saved["draw_counter"], saved["seed"]) == (W.DRAW_W + 2, W.SEED_W)
    resumed = RainbowLearner(R.golden_state(1, "soft"), rp, batch_size=BATCH, seed=1,
                             generator=torch.Generator().manual_seed(5), device=DEV)
    resumed.load_state_dict(saved)
    assert (resumed.learn_step_counter, resumed.draw_counter, resumed.seed) == (2, W.DRAW_W + 2, W.SEED_W)
    a, b = learner.learn(1, return_rows=True), resumed.learn(1, return_rows=True)
    assert torch.equal(a, b) and torch.equal(learner._buf.view(torch.int32), resumed._buf.view(torch.int32))


# ------------------------------------------------------------------ C. counters past 2^32
def _store(ring, d, kind, skip_ego_won=True):
    """One store of the inputs `d` (wide_words.store_inputs, as device tensors) as rows of `kind`."""
    args = [d[k] for k in ("obs0", "obs", "a1", "rew", "done", "fobs")]
    if kind == "dqn":
        ring.store(*args, d["words"], skip_ego_won=skip_ego_won)
    elif kind == "goal":
        ring.store(*args, skip_ego_won=False, goal=d["goal"], next_goal=d["goal2"], reward=d["r_int"])
    else:  # Goal_DQN's rows: the words are the no-break bits
        ring.store(*args, d["words"], True, reward=d["r_int"], meta_goal=d["goal2"])


def _oracle_store(mem, c, d, kind, skip_ego_won=True):
    n = d["a1"].shape[1]
    base = (d["obs0"], d["obs"], d["a1"], d["rew"], d["done"], d["fobs"])
    if kind == "dqn":
        return mo.replay_store(mem, c, *base, W.unpack_won(d["words"], n), skip_ego_won=skip_ego_won)
    if kind == "goal":
        return mo.replay_store(mem, c, *base, None, skip_ego_won=False, goal=d["goal"], next_goal=d["goal2"],
                               reward=d["r_int"])
    return mo.replay_store(mem, c, *base, W.unpack_won(d["words"], n), reward=d["r_int"], meta_goal=d["goal2"])


def _same_ring(ring, mem, c, what=""):
    assert ring.memory_counter == c, (what, ring.memory_counter, c)
    got = ring.memory.cpu().numpy()
    bad = np.flatnonzero((lr.bits(got) != lr.bits(mem)).any(axis=1))
    assert bad.size == 0, (what, f"{bad.size} of {len(mem)} rows differ, first {bad[:4].tolist()}")


@pytest.mark.parametrize("kind,cap", [("dqn", 5000), ("goal", 5000), ("meta", 5000), ("dqn", 7), ("goal", 300)])
def test_replay_ring_counter_crosses_2_to_32(torch, coracle, kind, cap):
    """577 x 9 transitions twice into a ring whose memory_counter starts at 2^32 - 100: the first store crosses
    2^32, the second starts above it (end, first, base, skip and slot0 of replay_write_kernel, the group scan's
    64-bit bases). Capacity 7 is far below one store: nearly every block is skipped whole. Capacity 300 is a
    seventeenth of one store of goal rows and more than one write block: a launch that skipped too little would
    write every slot seventeen times, from blocks that run side by side. Then what Python reads back: memory_counter, a filled-only sample (it draws among min(counter, cap) rows) and a saved state_dict."""
    from merging_gym import ReplayRing

    n, T = 577, 9
    rng = np.random.default_rng(cap + len(kind))
    ring = ReplayRing(cap, device=DEV, goal=kind == "goal")
    ring._counter.fill_(W.COUNTER_CROSS)
    mem = np.zeros((cap, ring.row), np.float32)
    c = W.COUNTER_CROSS
    for k in range(2):
        d = W.store_inputs(rng, n, T, goal=True)
        _store(ring, {key: _dev(v) for key, v in d.items()}, kind)
        c = _oracle_store(mem, c, d, kind)
        _same_ring(ring, mem, c, (kind, cap, k))
        assert c > 1 << 32  # crossed by the first store
    assert c > (1 << 32) + 2000
    rows, idx = ring.sample_rows(512, seed=W.SEED_W, draw=W.DRAW_W, filled_only=True, return_index=True)
    want = mo.replay_sample_index(coracle, cap, c, W.SEED_W, W.DRAW_W, 512, True)
    assert np.array_equal(idx.cpu().numpy(), want) and np.array_equal(rows.cpu().numpy(), mem[want])
    assert int(want.max()) > min(cap, 100) // 2  # among cap rows, not among counter mod 2^32
    back = ReplayRing(cap, device=DEV, goal=kind == "goal")
    back.load_state_dict(_reload(torch, ring.state_dict()))
    assert back.memory_counter == c and torch.equal(back.memory, ring.memory)


def test_rainbow_replay_counter_crosses_2_to_32(torch, coracle):
    """RainbowReplay.store_rollout and push (rl_store_kernel's (*counter + idx) % cap, counter_add_kernel) from
    2^32 - 100 against sequential pushes; len(), the sample and a saved state_dict."""
    from merging_gym import RainbowReplay
    from test_gpu_rainbow_learn import _emulate_pushes

    n, T, cap = 577, 9, 5000
    rng = np.random.default_rng(9)
    rp = RainbowReplay(cap, device=DEV)
    rp._counter.fill_(W.COUNTER_CROSS)
    assert len(rp) == cap
    want = np.zeros((cap, 24), np.float32)
    c = W.COUNTER_CROSS
    for k in range(2):
        d = W.store_inputs(rng, n, T)
        traj = {"obs": _dev(d["obs"]), "rew": _dev(d["rew"]), "a1": _dev(d["a1"]), "done": _dev(d["done"]),
                "final_observation": _dev(d["fobs"])}
        rp.store_rollout(_dev(d["obs0"]), traj)
        c = _emulate_pushes(want, c, d["obs0"], d["obs"], d["a1"], d["rew"], d["done"], d["fobs"])
        assert int(rp._counter.item()) == c == W.COUNTER_CROSS + (k + 1) * n * T
        assert np.array_equal(lr.bits(rp.memory.cpu().numpy()), lr.bits(want)), k
    rp.push(list(d["obs0"][0]), 3, 1.5, list(d["obs"][0, 0]), True)
    c = _emulate_pushes(want, c, d["obs0"][:1], d["obs"][:1, :1], np.array([[3]], np.int8),
                        np.array([[[1.5, 0.0]]], np.float32), np.array([[1]], np.uint8), None)
    assert int(rp._counter.item()) == c and np.array_equal(lr.bits(rp.memory.cpu().numpy()), lr.bits(want))
    assert len(rp) == cap and c > 1 << 32
    rows = rp.sample_rows(512, seed=W.SEED_W, draw=W.DRAW_W)
    idx = mo.replay_sample_index(coracle, cap, c, W.SEED_W, W.DRAW_W, 512, True)
    assert np.array_equal(rows.cpu().numpy(), want[idx]) and int(idx.max()) > cap // 2
    back = RainbowReplay(cap, device=DEV)
    back.load_state_dict(_reload(torch, rp.state_dict()))
    assert int(back._counter.item()) == c and len(back) == cap and torch.equal(back.memory, rp.memory)


def test_fused_goal_ring_counter_crosses_2_to_32(torch):
    """mg_rollout_hdqn's own goal ring (the store that advances the counter with counter_add_kernel) from
    2^32 - 100, two launches of 577 x 9 into 5,000 rows: slots and counter equal ReplayRing.store of the same
    trajectory into a twin ring at the same counter, and the oracle's replay_store."""
    from merging_gym import MergeVecEnv, ReplayRing
    from merging_gym.policy import NUM_GOALS, QNet
    from test_gpu_hdqn import _net

    n, T, cap = 577, 9, 5000
    rng = np.random.default_rng(21)
    meta, lower = (QNet.from_state_dict(_net(rng, i, o), device=DEV) for i, o in ((10, NUM_GOALS), (11, 5)))
    env = MergeVecEnv(n, device=DEV, final_observation=True)
    for k in range(60):
        env.step_random(5, opponent_random=False, step_idx=k)
    fused, twin = ReplayRing(cap, device=DEV, goal=True), ReplayRing(cap, device=DEV, goal=True)
    fused._counter.fill_(W.COUNTER_CROSS)
    twin._counter.fill_(W.COUNTER_CROSS)
    mem = np.zeros((cap, 24), np.float32)
    c = W.COUNTER_CROSS
    for k in range(2):
        obs0 = env.observe().clone()
        tr = env.rollout_hdqn(T, meta, lower, W.SEED_W, ring=fused)
        twin.store_rollout(obs0, tr, skip_ego_won=False, goal=tr["goal"], next_goal=tr["next_goal"], reward=tr["reward"])
        host = {key: tr[key].cpu().numpy() for key in ("obs", "a1", "rew", "done", "final_observation", "goal",
                                                       "next_goal", "reward")}
        c = mo.replay_store(mem, c, obs0.cpu().numpy(), host["obs"], host["a1"], host["rew"], host["done"],
                            host["final_observation"], None, skip_ego_won=False, goal=host["goal"],
                            next_goal=host["next_goal"], reward=host["reward"])
        assert fused.memory_counter == twin.memory_counter == c == W.COUNTER_CROSS + (k + 1) * n * T
        assert torch.equal(fused.memory.view(torch.int32), twin.memory.view(torch.int32)), k
        _same_ring(fused, mem, c, k)


def test_dqn_learner_reads_a_ring_whose_counter_is_above_2_to_32(torch, coracle):
    """learn_rows_live with filled_only: min(counter, cap) of a 64-bit counter (2^32 + 17; its low word alone would
    draw among 17 rows)."""
    from merging_gym import DQNLearner

    rows, sd = lr.case_fixture(10, 5, 32)
    ring = _dqn_ring(torch, rows, W.COUNTER_ABOVE)
    learner = DQNLearner(sd, ring, batch_size=BATCH, seed=W.SEED_W)
    learner.draw_counter = W.DRAW_W
    got = learner.learn(2, filled_only=True, return_rows=True).cpu().numpy()
    for u in range(2):
        idx = mo.replay_sample_index(coracle, len(rows), W.COUNTER_ABOVE, W.SEED_W, W.DRAW_W + u, BATCH, True)
        assert np.array_equal(lr.bits(got[u]), lr.bits(rows[idx])), u
        assert int(idx.max()) > 17


def test_rainbow_learner_reads_a_ring_whose_counter_is_above_2_to_32(torch, coracle):
    from merging_gym import RainbowLearner

    ring, _ = R.ring_case(64, 200)
    learner = RainbowLearner(R.golden_state(1, "soft"), _rainbow_replay(torch, ring, W.COUNTER_ABOVE), batch_size=BATCH,
                             seed=W.SEED_W, generator=torch.Generator().manual_seed(11), device=DEV)
    learner.draw_counter = W.DRAW_W
    got = learner.learn(2, return_rows=True).cpu().numpy()
    for u in range(2):
        idx = mo.replay_sample_index(coracle, 64, W.COUNTER_ABOVE, W.SEED_W, W.DRAW_W + u, BATCH, True)
        assert np.array_equal(lr.bits(got[u]), lr.bits(ring[idx])), u
        assert int(idx.max()) > 17


# ------------------------------------------------------------------ D. the group scan past 64 and past 1,024 groups
def _long_store(torch, n, T, kind, skip_ego_won=True):
    """The store twice. A ring larger than what is kept, sized from the oracle's count: every block's base shows
    in the ring and nothing is overwritten. Then 5,000 rows and the same store a second time: the wrap and the
    skip arithmetic with large bases. Returns (write blocks, groups, kept)."""
    from merging_gym import ReplayRing

    d = W.store_inputs(np.random.default_rng(1), n, T, goal=True)
    row = 24 if kind == "goal" else 22
    kept = _oracle_store(np.zeros((1, row), np.float32), 0, d, kind, skip_ego_won)
    blocks = -(-n // 256) * T
    dd = {key: _dev(v) for key, v in d.items()}
    for cap, stores in ((kept + 3, 1), (5000, 2)):
        ring = ReplayRing(cap, device=DEV, goal=kind == "goal")
        mem = np.zeros((cap, row), np.float32)
        c = 0
        for k in range(stores):
            _store(ring, dd, kind, skip_ego_won)
            c = _oracle_store(mem, c, d, kind, skip_ego_won)
            _same_ring(ring, mem, c, (n, T, kind, cap, k))
        assert c == stores * kept
        del ring
    return blocks, -(-blocks // 64), kept


@pytest.mark.parametrize("n,T,groups", [(3, 4200, 66), (3, 65600, 1025), (700, 1500, 71), (257, 300, 10)])
def test_long_narrow_stores_scan_many_groups(torch, n, T, groups):
    """The number of groups replay_group_scan walks is ceil(ceil(n / 256) T / 64), whatever the number of
    transitions: 66 groups (a second batch of 64 lanes, two of them live, the carry read), 1,025 (the second
    trip of the outer loop), 71 with blocks that keep up to 256 rows and a 188-env tail block, and the control of
    10 groups in one batch with a tail block of one env. Random won words (bits past n set), 10 % done rows."""
    blocks, ng, kept = _long_store(torch, n, T, "dqn")
    assert ng == groups and 0 < kept < n * T


def test_long_narrow_store_of_goal_rows(torch):
    """The 96-byte rows through the same scan: 3 x 4,200 goal rows, all kept (66 groups)."""
    blocks, ng, kept = _long_store(torch, 3, 4200, "goal")
    assert ng == 66 and kept == 3 * 4200


def test_long_narrow_store_without_the_filter(torch):
    """skip_ego_won=False: every block keeps its three rows, the largest group totals three envs can give."""
    blocks, ng, kept = _long_store(torch, 3, 4200, "dqn", skip_ego_won=False)
    assert ng == 66 and kept == 3 * 4200
