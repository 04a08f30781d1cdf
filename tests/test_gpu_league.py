"""MergeVecEnv.rollout_qnet_league (mg_rollout_qnet_league): every ordered pair (ego i, opponent j) of K nets on
its own slice of one env batch, in one launch.

The contract is equality: pairing p = i K + j of the launch is, bit for bit, a lone MergeVecEnv(n_pair,
env_offset = env_offset + p n_pair) holding the slice's state and records and running rollout_qnet(T, qnets[i],
seed[i], opponent=qnets[j], episilo=eps[i], opp_episilo=eps[j]) -- every trajectory tensor, the won-mask words,
the state and the 64-byte records, compared on the device as raw bits. The nets are distinct and seeded, each
with its own seed and episilo; the batch sits at a non-zero env_offset and the launch at a non-zero first step;
timeout_steps is set to T through the params, so every env completes an episode inside the launch and the
records, final observations and q_eval sums are all exercised. Nothing here needs a tolerance."""

import numpy as np
import pytest

import guard_bands
import learn_ref as lr

pytestmark = pytest.mark.gpu

# csrc/mg_rollout_qnet.h: kQWsEnvs = 2 groups x 64 lanes x kQWsEnvWaves (4) x kQWsIlp (2), the envs one block of
# qnet_rollout_ws_kernel steps; a pairing of kQWsEnvs + 64 envs has a full block and a ragged one
KQWS_ENVS = 1024
ALWAYS, NEVER = float("inf"), float("-inf")  # greedy thresholds 2^32 and 0
# per net, cycled: 0 < eps < 1 first (both branches draw), then the extremes
EPS = [0.7, 0.3, ALWAYS, 0.5, NEVER]
OFFSET = 3_000_017   # the batch's env_offset: odd, past 2^21
K0 = 501             # the launch's first step: odd (the OPP 0 / 1 kernels pair their draws by step parity)
STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf")


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


_NETS, _ENVS, _STARTS = {}, {}, {}


def _net(k, out_dim):
    """Net k of a league at one out_dim: seeded, mixed signs, no two alike."""
    from merging_gym.policy import QNet

    if (k, out_dim) not in _NETS:
        _NETS[k, out_dim] = QNet.from_state_dict(lr.seeded_net(10, out_dim, 9000 + 37 * k + out_dim), device="cuda:0")
    return _NETS[k, out_dim]


def _env(n, offset, T, tag=""):
    """A cached MergeVecEnv(n, env_offset=offset) whose episodes time out after T steps."""
    from merging_gym import MergeVecEnv

    if (n, offset, tag) not in _ENVS:
        _ENVS[n, offset, tag] = MergeVecEnv(n, device="cuda:0", env_offset=offset)
    env = _ENVS[n, offset, tag]
    env.params.timeout_steps = T
    return env


def _start(N):
    """The start state of a batch of N envs (200 random steps from reset under the default params: spread
    positions, some cars arrived) and its statistics records, computed once and never changed."""
    from merging_gym import MergeVecEnv

    if N not in _STARTS:
        env = MergeVecEnv(N, device="cuda:0", env_offset=OFFSET)
        for k in range(200):
            env.step_random(18, step_idx=k)
        _STARTS[N] = ({k: getattr(env, k).clone() for k in STATE}, env._ep_stats.clone())
    return _STARTS[N]


def _load(env, start, lo, hi):
    state, stats = start
    for k in STATE:
        getattr(env, k).copy_(state[k][lo:hi])
    env._ep_stats.copy_(stats[lo:hi])


def _bits(torch, t):
    """A tensor's raw bits, contiguous: floats as integers of their width, so NaNs and -0.0 compare by bits."""
    t = t.contiguous()
    return t.view({4: torch.int32, 8: torch.int64}[t.element_size()]) if t.is_floating_point() else t


def _assert_pairing(torch, env, got, lone, ref, p, n, what):
    """Pairing p's columns of the league's trajectory `got`, its state and its records against the lone env."""
    sl, w = slice(p * n, (p + 1) * n), n // 64
    assert set(got) == set(ref)
    done = ref["done"]
    for key in ("obs", "rew", "flags", "done", "collision", "a1", "a2"):
        assert torch.equal(_bits(torch, got[key][:, sl]), _bits(torch, ref[key])), f"{what}: {key}"
    # written where an env finished; other rows keep what the buffer held
    assert torch.equal(_bits(torch, got["final_observation"][:, sl])[done], _bits(torch, ref["final_observation"])[done]), \
        f"{what}: final_observation"
    assert torch.equal(got["won_mask"][:, p * w:(p + 1) * w].contiguous(), ref["won_mask"]), f"{what}: won_mask"
    for k in STATE:
        assert torch.equal(_bits(torch, getattr(env, k)[sl]), _bits(torch, getattr(lone, k))), f"{what}: state {k}"
    assert torch.equal(_bits(torch, env._ep_stats[sl]), _bits(torch, lone._ep_stats)), f"{what}: records"


def _assert_completed(torch, env, start, got, out_dim=5):
    """Every env finished an episode inside the launch: timeout_steps = T ends an episode at the launch's last
    step at the latest. An env that was handed an action outside action_dict (out_dim > 5 only) is left out: that
    step takes the reference's KeyError path, which ends no episode, so the params cannot promise it one (in the
    out_dim 8 case 132 of the 1,152 envs see only actions of action_dict, and some of the others complete none).
    At out_dim <= 5 no env is left out: the assertion is completed.min() >= 1 over the whole batch."""
    completed = env.counts[:, 0] - start[1][:, 4:].view(torch.int32)[:, 0]
    valid = ((got["a1"] < 5) & (got["a2"] < 5)).all(0)
    print(f"completed: min {int(completed.min())} over all {completed.numel()} envs, "
          f"min {int(completed[valid].min())} over the {int(valid.sum())} with every action in action_dict")
    if out_dim <= 5:
        assert bool(valid.all())
    assert int(valid.sum()) > 0 and int(completed[valid].min()) >= 1


def _settings(K, out_dim):
    nets = [_net(k, out_dim) for k in range(K)]
    seeds = [17 + 1000003 * k for k in range(K)]
    eps = [EPS[k % len(EPS)] for k in range(K)]
    return nets, seeds, eps


def _lone(torch, start, nets, seeds, eps, K, n, T, p, first_step):
    """The lone env of pairing p, loaded with the slice's start state when first_step is given (else it
    continues), after its rollout_qnet; (env, trajectory)."""
    i, j = divmod(p, K)
    lone = _env(n, OFFSET + p * n, T, tag="lone")  # never the league's own env (K = 1: the same size and offset)
    if first_step is not None:
        _load(lone, start, p * n, (p + 1) * n)
    ref = lone.rollout_qnet(T, nets[i], seeds[i], opponent=nets[j], episilo=eps[i], opp_episilo=eps[j],
                            first_step=first_step)
    return lone, ref


CASES = [pytest.param(1, 64, 3, 5, id="K1-n64-T3-out5"),                       # P = 1
         pytest.param(3, 64, 4, 5, id="K3-n64-T4-out5"),                       # slices far smaller than a block
         pytest.param(2, KQWS_ENVS + 64, 3, 5, id="K2-n1088-T3-out5"),         # a ragged last block per pairing
         pytest.param(3, 128, 3, 8, id="K3-n128-T3-out8")]                     # greedy actions outside action_dict


@pytest.mark.parametrize("K,n,T,out_dim", CASES)
def test_every_pairing_equals_the_lone_rollout(torch, K, n, T, out_dim):
    N = K * K * n
    start = _start(N)
    env = _env(N, OFFSET, T)
    _load(env, start, 0, N)
    nets, seeds, eps = _settings(K, out_dim)
    got = env.rollout_qnet_league(T, nets, seeds, eps, first_step=K0)
    assert env._step_idx == K0 + T
    assert got["obs"].shape == (T, N, 10) and got["won_mask"].shape == (T, N // 64)
    _assert_completed(torch, env, start, got, out_dim)
    for p in range(K * K):
        lone, ref = _lone(torch, start, nets, seeds, eps, K, n, T, p, K0)
        _assert_pairing(torch, env, got, lone, ref, p, n, f"pairing {divmod(p, K)}")
    if K > 1:  # (i, j) and (j, i) did act differently: own nets, seeds and thresholds
        assert not torch.equal(got["a1"][:, n:2 * n], got["a1"][:, K * n:(K + 1) * n])
        assert not torch.equal(got["a2"][:, n:2 * n], got["a2"][:, K * n:(K + 1) * n])
    if out_dim > 5:  # the checked path was taken: some greedy action fell outside action_dict
        assert int((got["a1"] >= 5).sum()) > 0 and int((got["a2"] >= 5).sum()) > 0
    # a second call continues from _step_idx, as the lone envs continue
    got = env.rollout_qnet_league(T, nets, seeds, eps)
    assert env._step_idx == K0 + 2 * T
    for p in range(K * K):
        lone, ref = _lone(torch, start, nets, seeds, eps, K, n, T, p, None)
        assert lone._step_idx == K0 + 2 * T
        _assert_pairing(torch, env, got, lone, ref, p, n, f"second call, pairing {divmod(p, K)}")


def test_top_of_the_table(torch):
    """K = 64: 4,096 pairings of 64 envs, 262,144 envs in one launch. The four corners and 28 pairings drawn with
    a fixed seed are compared with lone calls -- a cap on run time, not on scope: the cases above compare every
    pairing at small K."""
    K, n, T = 64, 64, 2
    N = K * K * n
    start = _start(N)
    env = _env(N, OFFSET, T)
    _load(env, start, 0, N)
    nets, seeds, eps = _settings(K, 5)
    got = env.rollout_qnet_league(T, nets, seeds, eps, first_step=K0)
    _assert_completed(torch, env, start, got)
    corners = [0, K - 1, K * (K - 1), K * K - 1]
    rng = np.random.default_rng(64)
    drawn = [int(p) for p in rng.permutation(K * K) if int(p) not in corners][:28]
    for p in corners + drawn:
        lone, ref = _lone(torch, start, nets, seeds, eps, K, n, T, p, K0)
        _assert_pairing(torch, env, got, lone, ref, p, n, f"pairing {divmod(p, K)}")


def test_trajectory_false_changes_nothing(torch):
    """Two envs from one state, one call with the trajectory and one without: the same state and records; the
    call without returns None and leaves a poisoned trajectory buffer unwritten."""
    K, n, T = 2, 64, 3
    N = K * K * n
    start = _start(N)
    nets, seeds, eps = _settings(K, 5)
    a, b = _env(N, OFFSET, T), _env(N, OFFSET, T, tag="twin")
    _load(a, start, 0, N)
    _load(b, start, 0, N)
    _assert_completed(torch, a, start, a.rollout_qnet_league(T, nets, seeds, eps, first_step=K0))
    g = guard_bands.install(b, T)
    assert b.rollout_qnet_league(T, nets, seeds, eps, first_step=K0, trajectory=False) is None
    assert b._step_idx == K0 + T
    for k in STATE:
        assert torch.equal(_bits(torch, getattr(a, k)), _bits(torch, getattr(b, k))), k
    assert torch.equal(_bits(torch, a._ep_stats), _bits(torch, b._ep_stats))
    for name, (raw, _) in g.raw.items():  # the tensors and the bands around them: every byte still the prefill
        assert bool((raw == guard_bands.FILL).all()), name


def test_league_leaves_lone_and_many_alone(torch):
    """rollout_qnet_many with an opponent list arranged as the same K^2 pairings (K = 3: nine members) equals the
    league call bit for bit: the two paths agree."""
    K, n, T = 3, 64, 4
    N = K * K * n
    start = _start(N)
    nets, seeds, eps = _settings(K, 5)
    a, b = _env(N, OFFSET, T), _env(N, OFFSET, T, tag="twin")
    _load(a, start, 0, N)
    _load(b, start, 0, N)
    got = a.rollout_qnet_league(T, nets, seeds, eps, first_step=K0)
    ego = [p // K for p in range(K * K)]
    opp = [p % K for p in range(K * K)]
    ref = b.rollout_qnet_many(T, [nets[i] for i in ego], [seeds[i] for i in ego], opponent=[nets[j] for j in opp],
                              episilo=[eps[i] for i in ego], opp_episilo=[eps[j] for j in opp], first_step=K0)
    _assert_pairing(torch, a, got, b, ref, 0, N, "the whole batch")


def test_rollout_qnet_league_refusals(torch):
    from merging_gym.policy import QNet

    env = _env(576, OFFSET, 3)
    q = [_net(k, 5) for k in range(3)]
    with pytest.raises(ValueError, match="slices of a multiple of 64"):
        env.rollout_qnet_league(2, q[:2], 1)            # 576 / 4 = 144 is no multiple of 64
    with pytest.raises(ValueError, match="slices of a multiple of 64"):
        env.rollout_qnet_league(2, q + q[:2], 1)        # 576 is not 25 slices
    for name in ("seed", "episilo"):
        kw = dict(seed=1)
        kw[name] = [1, 2]
        with pytest.raises(ValueError, match=f"{name}: expected one value or 3"):
            env.rollout_qnet_league(2, q, **kw)
    with pytest.raises(ValueError, match="one out_dim"):
        env.rollout_qnet_league(2, [q[0], _net(1, 8), q[2]], 1)
    with pytest.raises(ValueError, match="in_dim 10"):
        env.rollout_qnet_league(2, [q[0], QNet.from_state_dict(lr.seeded_net(11, 5, 3), device="cuda:0"), q[2]], 1)
    with pytest.raises(ValueError, match="1..64 nets"):
        env.rollout_qnet_league(2, [], 1)
    k = env._step_idx
    assert env.rollout_qnet_league(2, q, 1)["a1"].shape == (2, 576) and env._step_idx == k + 2
