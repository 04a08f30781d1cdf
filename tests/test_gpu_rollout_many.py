"""MergeVecEnv.rollout_qnet_many (mg_rollout_qnet_many): M actors on slices of one env batch in one launch.

The contract is equality: member m of the launch is, byte for byte, a lone MergeVecEnv(n_member,
env_offset = m n_member) holding the slice's state and records and running rollout_qnet with member m's net,
seed and thresholds. The sizes put the member boundaries off the kernel's 1,024-env block grid (n_member =
1,088 = one full block and a 64-env partial one), where a block that took its envs or its limit from its block
index alone would run into the next member's rows. A second test pins the member launch to the oracle itself
(Philox draws per member seed, greedy choices, transitions, q_eval), so the first keeps its meaning whatever the
lone path is built on."""

import os

import numpy as np
import pytest

import merge_oracle as mo
from choice_check import ChoiceCheck, check_q_eval, exact_q, order_matched_q
from conftest import ROOT

pytestmark = pytest.mark.gpu

OBS_TOL = dict(rtol=1e-6, atol=1e-5)   # test_gpu_qnet.py's: fp32 outputs against the oracle's fp64
MAX_EXCUSED = {"l1": 1e-4, "l3": 1e-4}  # test_gpu_qnet.py's bounds (the measured share so far is 0)
ALWAYS, NEVER = float("inf"), float("-inf")  # greedy thresholds 2^32 and 0
T = 6
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf")
# per member, cycled: the ego's and the opponent's episilo (both extremes among the first three)
EPS = [(0.7, NEVER), (ALWAYS, 0.3), (NEVER, ALWAYS), (0.2, 0.7), (-0.3, 1.1)]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


@pytest.fixture(scope="module")
def nets():
    f = np.load(os.path.join(ROOT, "tests", "golden", "dqn_checkpoints.npz"))
    return {key: {name.split("/", 1)[1]: f[name] for name in f.files if name.startswith(key + "/")}
            for key in ("l1", "l3")}


def member_state_dict(nets, m):
    """Member m's net: l1 and l3 themselves for members 0 and 1, then one of them with every tensor scaled by
    its own deterministic factors near 1, so no two members share a net."""
    base = nets["l1" if m % 2 == 0 else "l3"]
    if m < 2:
        return base
    rng = np.random.default_rng(7000 + m)
    return {k: (v * (1.0 + 0.05 * rng.standard_normal(v.shape))).astype(np.float32) for k, v in base.items()}


@pytest.fixture(scope="module")
def qnets(torch, nets):
    from merging_gym.policy import QNet

    cache = {}

    def get(m):
        if m not in cache:
            cache[m] = QNet.from_state_dict(member_state_dict(nets, m), device="cuda:0")
        return cache[m]

    return get


@pytest.fixture(scope="module")
def starts(torch):
    """Per batch size: the start state (200 random steps, then every clock three steps short of the timeout, so
    every env finishes inside a six-step launch) and the statistics records, computed once and never changed."""
    from merging_gym import MergeVecEnv

    cache = {}

    def get(N):
        if N not in cache:
            env = MergeVecEnv(N, device="cuda:0")
            for k in range(200):
                env.step_random(18, step_idx=k)
            m = env._nat.TF_STEPS_MASK
            env.tf.copy_((env.tf & ~m) | 2498)
            cache[N] = ({k: getattr(env, k).clone() for k in STATE}, env._ep_stats.clone())
        return cache[N]

    return get


_ENVS = {}


def _env(n, offset):
    from merging_gym import MergeVecEnv

    if (n, offset) not in _ENVS:
        _ENVS[n, offset] = MergeVecEnv(n, device="cuda:0", env_offset=offset)
    return _ENVS[n, offset]


def _load(env, start, lo, hi):
    state, stats = start
    for k in STATE:
        getattr(env, k).copy_(state[k][lo:hi])
    env._ep_stats.copy_(stats[lo:hi])


def _cpu(traj):
    return {k: v.cpu().numpy().copy() for k, v in traj.items()}


def _opponents(opponent, qnets, M):
    """The launch's opponent argument and member m's for the lone run: a mode, or each member's own net --
    the next member's (cross-play), and for a population of one a net that is no member's."""
    if opponent != "nets":
        return opponent, [opponent] * M
    opp = [qnets((m + 1) % M if M > 1 else 1) for m in range(M)]
    return opp, opp


SIZES = [(M, n) for M in (1, 2, 3) for n in (64, 1088)]
CASES = [pytest.param(M, n, o, k0, id=f"M{M}-n{n}-{o}-k{k0}")
         for M, n in SIZES for o in ("none", "uniform", "self", "nets") for k0 in (500, 501)]
CASES += [pytest.param(64, 64, o, k0, id=f"M64-n64-{o}-k{k0}") for o in ("none", "nets") for k0 in (500, 501)]


@pytest.mark.parametrize("M,n,opponent,k0", CASES)
def test_member_equals_lone_rollout_bit_for_bit(torch, qnets, starts, M, n, opponent, k0):
    N = M * n
    start = starts(N)
    env = _env(N, 0)
    _load(env, start, 0, N)
    nets_m = [qnets(m) for m in range(M)]
    seeds = [17 + 1000003 * m for m in range(M)]
    eps = [EPS[m % len(EPS)][0] for m in range(M)]
    opp_eps = [EPS[m % len(EPS)][1] for m in range(M)]
    opp_many, opp_lone = _opponents(opponent, qnets, M)
    got = _cpu(env.rollout_qnet_many(T, nets_m, seeds, opponent=opp_many, episilo=eps, opp_episilo=opp_eps,
                                     first_step=k0))
    assert env._step_idx == k0 + T
    got_state = {k: getattr(env, k).cpu().numpy().copy() for k in STATE}
    got_stats = env._ep_stats.cpu().numpy().copy()
    assert set(got) == {"obs", "rew", "done", "collision", "a1", "a2", "final_observation", "won_mask", "flags"}
    assert got["won_mask"].shape == (T, N // 64)
    assert got["done"].sum(0).min() >= 1  # every env finished inside the launch
    w = n // 64
    for m in range(M):
        lone = _env(n, m * n)
        _load(lone, start, m * n, (m + 1) * n)
        ref = _cpu(lone.rollout_qnet(T, nets_m[m], seeds[m], opponent=opp_lone[m], episilo=eps[m],
                                     opp_episilo=opp_eps[m], first_step=k0))
        for key, r in ref.items():
            g = got[key][:, m * w:(m + 1) * w] if key == "won_mask" else got[key][:, m * n:(m + 1) * n]
            assert g.shape == r.shape, (key, g.shape, r.shape)
            if key == "final_observation":  # written where an env finished; other rows keep what they held
                d = ref["done"]
                assert d.tobytes() == got["done"][:, m * n:(m + 1) * n].tobytes()
                g, r = g[d], r[d]
            assert np.ascontiguousarray(g).tobytes() == r.tobytes(), f"member {m}: {key}"
        for k in STATE:
            assert got_state[k][m * n:(m + 1) * n].tobytes() == getattr(lone, k).cpu().numpy().tobytes(), (m, k)
        assert got_stats[m * n:(m + 1) * n].tobytes() == lone._ep_stats.cpu().numpy().tobytes(), f"member {m}: records"
    if M > 1:  # the members did act differently (own nets, seeds and thresholds)
        assert not np.array_equal(got["a1"][:, :n], got["a1"][:, n:2 * n])


@pytest.mark.parametrize("opponent", ["none", "cross"])
def test_member_launch_matches_the_oracle(torch, coracle, nets, qnets, starts, opponent):
    """M = 2, n_member = 1,088, nets (l1, l3); "cross": member 0 = l1 against l3, member 1 = l3 against l1.
    Checked as test_gpu_qnet.py's _rollout_qnet_policy_and_transitions checks the lone launch: the draws per
    member seed at the env's index in the batch, the greedy choices, the oracle's step with the kernel's
    actions, and q_eval with the kernel-order Q-values."""
    from merging_gym.policy import greedy_threshold

    M, n, k0 = 2, 1088, 501
    N = M * n
    keys, opp_keys = ["l1", "l3"], ["l3", "l1"]
    seeds, eps, opp_eps = [17, 90001], [0.7, 0.2], [0.3, 0.7]
    env = _env(N, 0)
    _load(env, starts(N), 0, N)
    envs = coracle.new_envs(N)
    for name, src in (("pos1", env.p1), ("vel1", env.v1), ("pos2", env.p2), ("vel2", env.v2),
                      ("r1_acc", env.ret1), ("r2_acc", env.ret2)):
        envs[name] = src.cpu().numpy()
    envs["steps"] = env.steps.cpu().numpy()
    envs["winner"] = env.winner.cpu().numpy()
    envs["time_stamp"] = mo.DEFAULT_PARAMS.clock(envs["steps"])
    obs_in = env.observe().cpu().numpy().copy()
    qe = env.q_eval.cpu().numpy().copy()
    qe_abs, qe_pin, qe_model = np.zeros(N), qe.copy(), qe.copy()
    cross = opponent == "cross"
    form = "16x16" if cross else "32x32"
    nets_m = [qnets(0), qnets(1)]
    traj = _cpu(env.rollout_qnet_many(T, nets_m, seeds, opponent=[qnets(1), qnets(0)] if cross else "none",
                                      episilo=eps, opp_episilo=opp_eps, first_step=k0))
    cc1 = [ChoiceCheck(f"member {m} ego {keys[m]} ({opponent})", max_frac=MAX_EXCUSED[keys[m]]) for m in range(M)]
    cc2 = [ChoiceCheck(f"member {m} opponent {opp_keys[m]}", max_frac=MAX_EXCUSED[opp_keys[m]]) for m in range(M)]
    for t in range(T):
        q = np.empty((N, 5))
        for m in range(M):
            s = slice(m * n, (m + 1) * n)
            ex, rnd1, ex2, rnd2 = mo.qnet_policy_draws(
                lambda c, m=m: coracle.philox_batch(n, m * n, seeds[m], c), k0 + t, "self" if cross else "none")
            o = obs_in[s]
            q[s] = mo.qnet_reference(nets[keys[m]], o, bf16=True)
            greedy = ex.astype(np.uint64) < np.uint64(greedy_threshold(eps[m]))
            cc1[m].check(traj["a1"][t][s], np.where(greedy, q[s].argmax(1), rnd1), greedy, q[s], f"step {t}",
                         q_exact=exact_q(nets[keys[m]], o, form=form))
            if cross:
                q2 = mo.qnet_reference(nets[opp_keys[m]], o, bf16=True, swap=True)
                g2 = ex2.astype(np.uint64) < np.uint64(greedy_threshold(opp_eps[m]))
                cc2[m].check(traj["a2"][t][s], np.where(g2, q2.argmax(1), rnd2), g2, q2, f"step {t}",
                             q_exact=exact_q(nets[opp_keys[m]], o, swap=True))
            else:
                assert (traj["a2"][t][s] == -1).all()
        o_obs, o_rew, o_done, o_coll, _, o_fobs, err = coracle.step(envs, traj["a1"][t], traj["a2"][t],
                                                                    autoreset=True, final_obs=True)
        assert err == 0
        np.testing.assert_array_equal(traj["done"][t], o_done.astype(bool), err_msg=str(t))
        np.testing.assert_array_equal(traj["collision"][t], o_coll.astype(bool), err_msg=str(t))
        np.testing.assert_allclose(traj["obs"][t], o_obs.astype(np.float32), **OBS_TOL)
        np.testing.assert_allclose(traj["rew"][t], o_rew.astype(np.float32), **OBS_TOL)
        d = o_done.astype(bool)
        np.testing.assert_allclose(traj["final_observation"][t][d], o_fobs[d].astype(np.float32), **OBS_TOL)
        a = traj["a1"][t].astype(np.int64)
        qe += np.where(d, q[np.arange(N), a], 0.0)
        qe_abs += np.where(d, np.abs(q).max(1), 0.0)
        for m in range(M):
            s = slice(m * n, (m + 1) * n)
            if d[s].any():
                qp = order_matched_q(nets_m[m], nets[keys[m]], obs_in[s], form)
                qe_pin[s] += np.where(d[s], qp[np.arange(n), a[s]], 0.0)
                qm = mo.qnet_reference_mfma(nets[keys[m]], obs_in[s], form=form).astype(np.float64)
                qe_model[s] += np.where(d[s], qm[np.arange(n), a[s]], 0.0)
        obs_in = traj["obs"][t]
    np.testing.assert_array_equal(env.p1.cpu().numpy(), envs["pos1"])
    np.testing.assert_array_equal(env.ret2.cpu().numpy(), envs["r2_acc"])
    assert traj["done"].sum(0).min() >= 1
    got_q = env.q_eval.cpu().numpy()
    for m in range(M):
        s = slice(m * n, (m + 1) * n)
        check_q_eval(got_q[s], qe[s], qe_abs[s], f"member {m} ego {keys[m]} ({opponent})", pinned=qe_pin[s],
                     model=qe_model[s])
        cc1[m].finish()
        if cross:
            cc2[m].finish()


def test_rollout_qnet_many_refusals(torch, nets, qnets):
    from merging_gym.policy import QNet

    env = _env(192, 0)
    q = [qnets(0), qnets(1), qnets(2)]
    with pytest.raises(ValueError, match="slices of a multiple of 64"):
        env.rollout_qnet_many(2, q[:2] + q[:2] + q[:1], 1)        # 192 is not 5 slices
    with pytest.raises(ValueError, match="slices of a multiple of 64"):
        env.rollout_qnet_many(2, q[:2], 1)                        # 96 is no multiple of 64
    for name in ("seed", "episilo", "opp_episilo"):
        kw = dict(seed=1)
        kw[name] = [1, 2]
        with pytest.raises(ValueError, match=f"{name}: expected one value or 3"):
            env.rollout_qnet_many(2, q, **kw)
    sd = {k: v.copy() for k, v in nets["l1"].items()}
    sd["out.weight"], sd["out.bias"] = sd["out.weight"][:3].copy(), sd["out.bias"][:3].copy()
    narrow = QNet.from_state_dict(sd, device="cuda:0")
    with pytest.raises(ValueError, match="one out_dim"):
        env.rollout_qnet_many(2, [q[0], narrow, q[2]], 1)
    with pytest.raises(ValueError, match="expected a mode or 3 nets"):
        env.rollout_qnet_many(2, q, 1, opponent=q[:2])
    with pytest.raises(ValueError, match="the ego nets' out_dim"):
        env.rollout_qnet_many(2, q, 1, opponent=[q[1], narrow, q[0]])
    sd = {k: v.copy() for k, v in nets["l1"].items()}
    sd["fc1.weight"] = np.concatenate([sd["fc1.weight"], sd["fc1.weight"][:, :1]], axis=1)
    wide = QNet.from_state_dict(sd, device="cuda:0")
    with pytest.raises(ValueError, match="in_dim 10"):
        env.rollout_qnet_many(2, [q[0], wide, q[2]], 1)
    with pytest.raises(ValueError, match="1..64 nets"):
        env.rollout_qnet_many(2, [], 1)
    k = env._step_idx
    assert env.rollout_qnet_many(2, q, 1)["a1"].shape == (2, 192) and env._step_idx == k + 2


def test_member_summaries_equal_the_lone_envs(torch, qnets, starts):
    M, n = 3, 64
    env = _env(M * n, 0)
    _load(env, starts(M * n), 0, M * n)
    env.rollout_qnet_many(T, [qnets(m) for m in range(M)], [5, 6, 7], first_step=500)
    got = env.member_summaries(M)
    assert len(got) == M and all(s["completed"] >= n for s in got)
    for m in range(M):
        lone = _env(n, m * n)
        _load(lone, starts(M * n), m * n, (m + 1) * n)
        lone.rollout_qnet(T, qnets(m), 5 + m, first_step=500)
        np.testing.assert_equal(got[m], lone.episode_summary(), err_msg=str(m))
    with pytest.raises(ValueError, match="equal slices"):
        env.member_summaries(5)
