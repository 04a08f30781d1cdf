"""GPU parity away from the default mg_params: the kernels against the parametrised C oracle at the
cases of tests/params_cases.py, at the default suite's bars (flags exact, fp32 outputs at OBS_TOL,
fp64 state bit for bit). Sizes are the smallest that still leave a ragged last wave and a ragged
last block (1,000 and 577 envs).

Cases A, C, D and E keep every live angle inside arc_sincos's polynomial range, where host, device
and (to 1 ulp, absorbed by the box truncation in all but touching cases) glibc agree. Case B's wide
angles take the device library's sin / cos, one ulp from glibc's, which can move a touching-box
collision flag: B is compared flag for flag with the oracle on the CPU only (tests/test_host_step.py);
here it appears where the check does not depend on that ulp (the reset observation, q_eval on the
kernel's own inputs in tests/test_gpu_qnet.py).
"""

import numpy as np
import pytest

import merge_oracle as mo
import params_cases as pc

pytestmark = pytest.mark.gpu

OBS_TOL = dict(rtol=1e-6, atol=1e-5)


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


def _env(case, n, scattered=True, seed=0, **kw):
    from merging_gym import MergeVecEnv

    env = MergeVecEnv(n, device="cuda:0", **kw)
    pc.fill_native(env.params, case)
    env.reset()
    if scattered:
        pc.load_scattered_device(env, case, np.random.default_rng(seed))
    return env


def _check_state(env, envs):
    for name, key in (("p1", "pos1"), ("p2", "pos2"), ("v1", "vel1"), ("v2", "vel2"),
                      ("ret1", "r1_acc"), ("ret2", "r2_acc")):
        np.testing.assert_array_equal(getattr(env, name).cpu().numpy(), envs[key], err_msg=name)
    np.testing.assert_array_equal(env.winner.cpu().numpy(), envs["winner"])
    np.testing.assert_array_equal(env.steps.cpu().numpy(), envs["steps"])


def _check_step(out, ref, k):
    obs, rew, done, info = out
    o_obs, o_rew, o_done, o_coll, _, o_fobs, err = ref
    assert err == 0
    np.testing.assert_array_equal(done.cpu().numpy(), o_done.astype(bool), err_msg=f"done @ {k}")
    np.testing.assert_array_equal(info["collision"].cpu().numpy(), o_coll.astype(bool), err_msg=f"coll @ {k}")
    np.testing.assert_allclose(obs.cpu().numpy(), o_obs.astype(np.float32), **OBS_TOL, err_msg=f"obs @ {k}")
    np.testing.assert_allclose(rew.cpu().numpy(), o_rew.astype(np.float32), **OBS_TOL, err_msg=f"rew @ {k}")
    d = o_done.astype(bool)
    np.testing.assert_allclose(info["final_observation"].cpu().numpy()[d], o_fobs[d].astype(np.float32),
                               **OBS_TOL, err_msg=f"final_obs @ {k}")


@pytest.mark.parametrize("case", ["A", "C", "D", "E", "F"])
def test_config2_host_actions_autoreset_at_params(torch, coracle, case):
    """mg_step with host-drawn actions (None, valid ones) and gym.vector autoreset: 1,000 envs x 300
    steps from scattered states, every flag, observation, reward, final observation, the fp64 state
    and both scripts' episode statistics against the parametrised oracle."""
    n, steps = 1000, 300
    P = pc.CASES[case]
    rng = np.random.default_rng(11)
    env = _env(case, n, seed=1)
    envs = mo.oracle_envs_from(coracle, env, params=P)
    tmo = P.timeout_steps()
    assert env.params.timeout_steps == tmo
    ret_sum, counts = mo.new_stats(n)
    timeouts = 0
    for k in range(steps):
        a1 = rng.integers(0, 5, n).astype(np.int8)
        a2 = rng.integers(-1, 5, n).astype(np.int8)
        timeouts += int((envs["steps"] + 1 >= tmo).sum())
        out = env.step(torch.from_numpy(a1).cuda(), torch.from_numpy(a2).cuda())
        ref = coracle.step(envs, a1, a2, autoreset=True, final_obs=True, stats=(ret_sum, counts), params=P)
        _check_step(out, ref, k)
    _check_state(env, envs)
    st = env.episode_statistics()
    np.testing.assert_array_equal(st["counts"].cpu().numpy().astype(np.uint32), counts)
    np.testing.assert_array_equal(st["returns"].cpu().numpy(), ret_sum)
    # episodes finished, some collided, the ego arrived first in some, both win tests fired, timeouts
    assert counts[:, 0].sum() > 0 and counts[:, 1].sum() > 0 and counts[:, 2].sum() > 0
    assert counts[:, 4].sum() > 0 and counts[:, 5].sum() > 0 and timeouts > 0
    assert (ret_sum[:, 2] != ret_sum[:, 0]).any()


@pytest.mark.parametrize("case", ["A", "D"])
def test_reset_observe_and_autoreset_observation_at_params(torch, coracle, case):
    """mg_reset's observation equals the oracle's reset observation; the observation an autoreset
    writes -- computed on the host once per launch (Reset0) -- equals mg_reset's, computed on the
    device, bit for bit (every angle inside the shared polynomial); mg_observe of scattered states
    equals the oracle's observe() and is_collided()."""
    n = 1000
    P = pc.CASES[case]
    env = _env(case, n, scattered=False)
    reset_obs = env.obs.clone()
    o0 = coracle.reset(coracle.new_envs(n), P)
    np.testing.assert_allclose(reset_obs.cpu().numpy(), o0.astype(np.float32), **OBS_TOL)
    assert abs(float(np.arctan2(P.H, P.R)) - P.START_POINT / P.R) < 0.0625
    # every env one step from the timeout: the step finishes them all and autoreset writes Reset0
    env.tf.fill_(P.timeout_steps() - 1)
    obs, _, done, _ = env.step(torch.zeros(n, dtype=torch.int8, device="cuda"), None)
    assert bool(done.all())
    assert torch.equal(obs, reset_obs)
    assert bool((env.steps == 0).all())
    # observe / is_collided at scattered states
    pc.load_scattered_device(env, case, np.random.default_rng(5), share=1.0)
    envs = mo.oracle_envs_from(coracle, env, params=P)
    np.testing.assert_allclose(env.observe().cpu().numpy(), coracle.observe(envs, P).astype(np.float32), **OBS_TOL)
    coll = coracle.collided(envs, P)
    np.testing.assert_array_equal(env.coll.cpu().numpy(), coll)
    assert coll.sum() > 10


def test_reset_observation_sources_at_the_wide_angle(torch, coracle):
    """Case B (angle0 = 1.28): outside the polynomial range the host-computed reset observation of an
    autoreset (glibc's sin / cos) and mg_reset's (the device library's) may differ by the libraries'
    one ulp in fp64, so by at most 1 fp32 ulp after the rounding -- and no more; both are the oracle's
    reset observation at OBS_TOL."""
    n, case = 577, "B"
    P = pc.CASES[case]
    env = _env(case, n, scattered=False)
    reset_obs = env.obs.clone().cpu().numpy()
    o0 = coracle.reset(coracle.new_envs(n), P).astype(np.float32)
    np.testing.assert_allclose(reset_obs, o0, **OBS_TOL)
    env.tf.fill_(P.timeout_steps() - 1)
    obs, _, done, _ = env.step(torch.zeros(n, dtype=torch.int8, device="cuda"), None)
    assert bool(done.all())
    auto = obs.cpu().numpy()
    np.testing.assert_allclose(auto, o0, **OBS_TOL)
    np.testing.assert_array_max_ulp(auto, reset_obs, maxulp=1)
    print(f"[reset sources B] {int((auto != reset_obs).sum())} of {auto.size} values differ by 1 fp32 ulp")


@pytest.mark.parametrize("case", ["A", "C"])
def test_rollout_equals_step_sequence_at_params(torch, case):
    """mg_rollout_random is bit-identical to T launches of mg_step_random at non-default params:
    (n, T) = (577, 19), every output, the state and the whole statistics records."""
    n, T, seed = 577, 19, 77
    a, b = _env(case, n, seed=3), _env(case, n, seed=3)
    for name in ("p1", "v1", "p2", "v2", "tf"):
        assert torch.equal(getattr(a, name), getattr(b, name))
    traj = {key: v.clone() if v is not None else None
            for key, v in b.rollout_random(T, seed, first_step=180).items()}
    for t in range(T):
        obs, rew, done, info = a.step_random(seed, step_idx=180 + t)
        assert torch.equal(traj["obs"][t], obs), t
        assert torch.equal(traj["rew"][t], rew), t
        assert torch.equal(traj["done"][t], done), t
        assert torch.equal(traj["collision"][t], info["collision"]), t
        assert torch.equal(traj["a1"][t], a.a1_buf) and torch.equal(traj["a2"][t], a.a2_buf), t
        assert torch.equal(traj["final_observation"][t][done], info["final_observation"][done]), t
    for name in ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf", "returns", "counts", "_ep_stats"):
        assert torch.equal(getattr(a, name), getattr(b, name)), name
    assert int(traj["done"].sum()) > 20


def test_device_random_actions_step_at_params(torch, coracle):
    """mg_step_random at case A: the Philox actions equal the oracle's and every step equals the
    parametrised oracle's with them (both opponent kinds), 577 envs x 120 steps."""
    n, steps, seed, case = 577, 120, 99, "A"
    P = pc.CASES[case]
    env = _env(case, n, seed=4)
    envs = mo.oracle_envs_from(coracle, env, params=P)
    finished = 0
    for k in range(steps):
        out = env.step_random(seed, opponent_random=(k % 3 != 0), step_idx=k)
        a1, a2 = coracle.random_actions(n, 0, seed, k, k % 3 != 0)
        np.testing.assert_array_equal(env.a1_buf.cpu().numpy(), a1)
        np.testing.assert_array_equal(env.a2_buf.cpu().numpy(), a2)
        ref = coracle.step(envs, a1, a2, autoreset=True, final_obs=True, params=P)
        _check_step(out, ref, k)
        finished += int(ref[2].sum())
    _check_state(env, envs)
    assert finished > 50


def test_params_validation_on_the_device_entry_points(torch):
    """check_params runs before any launch: a timeout_steps the step count cannot reach is refused by
    mg_step, mg_reset, mg_observe and the rollout, and names the field."""
    from merging_gym import MergeVecEnv, _native

    env = MergeVecEnv(64, device="cuda:0")
    env.params.timeout_steps = 8192
    a = torch.zeros(64, dtype=torch.int8, device="cuda")
    for call in (lambda: env.step(a), env.reset, env.observe, lambda: env.step_random(1),
                 lambda: env.rollout_random(4, 1)):
        with pytest.raises(_native.NativeError, match="timeout_steps"):
            call()
    env.params.timeout_steps = 8191
    env.step(a)
