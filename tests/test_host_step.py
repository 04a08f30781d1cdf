"""The host step (mg_host_step / mg_host_reset / mg_host_observe, ABI 20): the kernels' own step
functions compiled for the CPU, on host arrays -- the single env's default backend (BASELINE
config 1). CPU suite: batched host steps against the C oracle (state bit-exact, flags exact, fp32
outputs to the rounding bar), every optional output of mg_outputs. GPU suite: host and kernel give
the same bytes for the same inputs."""

import ctypes

import numpy as np
import pytest

import merge_oracle as mo
import params_cases as pc

OBS_TOL = dict(rtol=1e-6, atol=1e-5)


class HostBatch:
    """n envs in host numpy arrays, laid out as the device SoA (include/merging_hip.h mg_state)."""

    def __init__(self, n, case=None):
        from merging_gym import _native

        self.nat, self.n = _native, n
        self.params = _native.default_params() if case is None else pc.native_params(case)
        self.s = {k: np.zeros(n) for k in ("p1", "v1", "p2", "v2", "ret1", "ret2")}
        self.tf = np.zeros(n, np.uint16)
        p = lambda a: ctypes.c_void_p(a.ctypes.data)  # noqa: E731
        self.state = _native.State(*(p(self.s[k]) for k in ("p1", "v1", "p2", "v2", "ret1", "ret2")), p(self.tf))
        self.obs = np.zeros((n, 10), np.float32)
        self.rew = np.zeros((n, 2), np.float32)
        self.flags = np.zeros((n, 4), np.uint8)
        self.fobs = np.full((n, 10), np.nan, np.float32)
        words = (n + 63) // 64
        self.done_mask = np.zeros(words, np.uint64)
        self.won_mask = np.zeros(words, np.uint64)
        self.err = np.zeros(1, np.int32)
        self.stats = np.zeros(n, _native.EPISODE_STATS_DTYPE)
        self.out = _native.Outputs(p(self.obs), p(self.rew), None, None, p(self.done_mask), p(self.fobs), None,
                                   p(self.err), p(self.won_mask), p(self.flags))
        self.st = _native.Stats(p(self.stats))

    def reset(self):
        rc = self.nat.lib.mg_host_reset(ctypes.byref(self.params), ctypes.byref(self.state), None,
                                        ctypes.byref(self.out), self.n)
        self.nat.check(rc, "mg_host_reset")

    def step(self, a1, a2=None, autoreset=True):
        a1 = np.ascontiguousarray(a1, np.int8)
        a2 = None if a2 is None else np.ascontiguousarray(a2, np.int8)
        self.fobs[:] = np.nan
        rc = self.nat.lib.mg_host_step(ctypes.byref(self.params), ctypes.byref(self.state),
                                       ctypes.c_void_p(a1.ctypes.data),
                                       None if a2 is None else ctypes.c_void_p(a2.ctypes.data),
                                       ctypes.byref(self.out), ctypes.byref(self.st), self.n,
                                       self.nat.AUTORESET if autoreset else 0)
        self.nat.check(rc, "mg_host_step")


def _bits(words, n):
    return np.unpackbits(words.view(np.uint8), bitorder="little")[:n].astype(bool)


def load_scattered(hb, coracle, case, rng, share=0.6):
    """Move a share of a freshly reset HostBatch's envs to params_cases.scatter states (mid-episode,
    some a few steps from the timeout) and return the C-oracle envs holding the same batch."""
    n = hb.n
    envs = coracle.new_envs(n)
    coracle.reset(envs, pc.CASES[case])
    p1, v1, p2, v2, steps, winner = pc.scatter(case, n, rng)
    sub = pc.oracle_envs(coracle, case, p1, v1, p2, v2, steps, winner)
    m = rng.random(n) < share
    envs[m] = sub[m]
    for name, key in (("p1", "pos1"), ("v1", "vel1"), ("p2", "pos2"), ("v2", "vel2")):
        hb.s[name][:] = envs[key]
    hb.tf[:] = (envs["steps"] | (envs["winner"] << 13)).astype(np.uint16)
    return envs


@pytest.mark.parametrize("opponent", ["uniform", "none", "mixed"])
def test_host_batch_equals_oracle(coracle, opponent):
    """Config-2 shape on the host path: 2,048 envs x 400 steps with autoreset, statistics, final
    observations, the interleaved step record and both ballot masks, against the C oracle."""
    _host_batch_vs_oracle(coracle, opponent, 2048, 400, None)


@pytest.mark.parametrize("opponent", ["uniform", "none", "mixed"])
@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E", "F"])
def test_host_batch_equals_oracle_at_params(coracle, case, opponent):
    """The same checks at the same bars away from the default mg_params (tests/params_cases.py): 512
    envs x 300 steps against the parametrised C oracle. A share of the envs starts from scattered
    states, some a few steps from timeout_steps, so finished episodes, collisions, both win tests and
    timeouts all occur without thousands of steps. B's wide angles are glibc's sin / cos on both sides
    here, so its flags are compared too."""
    _host_batch_vs_oracle(coracle, opponent, 512, 300, case)


def _host_batch_vs_oracle(coracle, opponent, n, steps, case):
    rng = np.random.default_rng(21)
    params = None if case is None else pc.CASES[case]
    tmo = (params or mo.DEFAULT_PARAMS).timeout_steps()
    hb = HostBatch(n, case)
    assert hb.params.timeout_steps == tmo
    hb.reset()
    envs = coracle.new_envs(n)
    np.testing.assert_allclose(hb.obs, coracle.reset(envs, params).astype(np.float32), **OBS_TOL)
    if case is not None:
        envs = load_scattered(hb, coracle, case, rng)
    ret_sum, counts = mo.new_stats(n)
    timeouts = 0
    for k in range(steps):
        a1 = rng.integers(0, 5, n).astype(np.int8)
        a2 = {"uniform": lambda: rng.integers(0, 5, n).astype(np.int8), "none": lambda: None,
              "mixed": lambda: rng.integers(-1, 5, n).astype(np.int8)}[opponent]()
        hb.step(a1, a2)
        won = None
        # the won bit is winner == 1 after the step, before autoreset: replay with step_with_won
        # on a copy for it, then the stats-keeping step on the real oracle envs
        probe = envs.copy()
        _, _, _, _, _, won, _ = mo.step_with_won(coracle, probe, a1, a2, params=params)
        last = envs["steps"] + 1 >= tmo
        o_obs, o_rew, o_done, o_coll, _, o_fobs, err = coracle.step(envs, a1, a2, autoreset=True, final_obs=True,
                                                                     stats=(ret_sum, counts), params=params)
        assert err == 0 and hb.err[0] == 0
        assert o_done[last].all()
        timeouts += int(last.sum())
        np.testing.assert_array_equal(hb.flags[:, 0].view(np.int8), a1)
        np.testing.assert_array_equal(hb.flags[:, 1].view(np.int8), -1 if a2 is None else a2)
        np.testing.assert_array_equal(hb.flags[:, 2], o_done, err_msg=f"done @ {k}")
        np.testing.assert_array_equal(hb.flags[:, 3], o_coll, err_msg=f"coll @ {k}")
        np.testing.assert_array_equal(_bits(hb.done_mask, n), o_done.astype(bool))
        np.testing.assert_array_equal(_bits(hb.won_mask, n), won)
        np.testing.assert_allclose(hb.obs, o_obs.astype(np.float32), **OBS_TOL, err_msg=f"obs @ {k}")
        np.testing.assert_allclose(hb.rew, o_rew.astype(np.float32), **OBS_TOL, err_msg=f"rew @ {k}")
        d = o_done.astype(bool)
        np.testing.assert_allclose(hb.fobs[d], o_fobs[d].astype(np.float32), **OBS_TOL)
        assert np.isnan(hb.fobs[~d]).all()
    for name, key in (("p1", "pos1"), ("v1", "vel1"), ("p2", "pos2"), ("v2", "vel2"), ("ret1", "r1_acc"),
                      ("ret2", "r2_acc")):
        np.testing.assert_array_equal(hb.s[name], envs[key], err_msg=name)  # fp64 state bit-exact
    np.testing.assert_array_equal(hb.tf & 0x1FFF, envs["steps"])
    np.testing.assert_array_equal((hb.tf & 0x6000) >> 13, envs["winner"])
    np.testing.assert_array_equal(hb.stats["ret"], ret_sum[:, :2])
    np.testing.assert_array_equal(hb.stats["ret_main"], ret_sum[:, 2])
    np.testing.assert_array_equal(hb.stats["counts"], counts)
    assert counts[:, 0].sum() > 0 and counts[:, 1].sum() > 0
    if case is not None:  # ego-first episodes, both win tests and the timeout occurred
        assert counts[:, 2].sum() > 0 and counts[:, 4].sum() > 0 and counts[:, 5].sum() > 0 and timeouts > 0


def test_host_invalid_actions_and_observe(coracle):
    """An action outside action_dict sets the error bits and advances the env exactly as far as the
    reference gets before its KeyError (the clock, plus the ego for a bad action2); mg_host_observe
    is observe() / is_collided() without a state change."""
    n = 256
    rng = np.random.default_rng(3)
    hb = HostBatch(n)
    hb.reset()
    envs = coracle.new_envs(n)
    coracle.reset(envs)
    for k in range(160):  # constant-speed pairs: many collide around step 151 (KAT A)
        a1 = rng.integers(0, 5, n).astype(np.int8)
        a1[: n // 2] = 2
        hb.step(a1, None, autoreset=False)
        coracle.step(envs, a1, None)
    bad = np.full(n, 3, np.int8)
    bad[::7] = 9
    a2 = np.full(n, 1, np.int8)
    a2[3::11] = 40
    hb.step(bad, a2, autoreset=False)
    _, _, _, _, _, _, err = coracle.step(envs, bad, a2)
    assert hb.err[0] == err == 3
    for name, key in (("p1", "pos1"), ("v1", "vel1"), ("p2", "pos2"), ("v2", "vel2"), ("ret1", "r1_acc")):
        np.testing.assert_array_equal(hb.s[name], envs[key], err_msg=name)
    np.testing.assert_array_equal(hb.tf & 0x1FFF, envs["steps"])
    # observe / is_collided, no state change
    before = {k: v.copy() for k, v in hb.s.items()}
    out = hb.nat.Outputs(ctypes.c_void_p(hb.obs.ctypes.data), None, None, None, None, None, None, None, None,
                         ctypes.c_void_p(hb.flags.ctypes.data))
    hb.nat.check(hb.nat.lib.mg_host_observe(ctypes.byref(hb.params), ctypes.byref(hb.state), ctypes.byref(out), n),
                 "mg_host_observe")
    np.testing.assert_allclose(hb.obs, coracle.observe(envs).astype(np.float32), **OBS_TOL)
    ref_coll = [mo.boxes_touch(*_boxes(p1, p2)) for p1, p2 in zip(envs["pos1"], envs["pos2"])]
    np.testing.assert_array_equal(hb.flags[:, 3].astype(bool), ref_coll)
    assert any(ref_coll)
    for k, v in before.items():
        np.testing.assert_array_equal(hb.s[k], v)


def _boxes(p1, p2):
    x1, y1 = mo.arc_position(p1, True)
    x2, y2 = mo.arc_position(p2, False)
    return mo.vehicle_box(y1, x1), mo.vehicle_box(y2, x2)


def test_host_entry_validation():
    from merging_gym import _native

    P = ctypes.byref(_native.default_params())
    rc = _native.lib.mg_host_step(P, ctypes.byref(_native.State()), None, None, ctypes.byref(_native.Outputs()),
                                  None, 4, 0)
    assert rc != 0 and b"NULL" in _native.lib.mg_last_error()
    assert _native.lib.mg_host_reset(None, None, None, None, 1) != 0
    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: n == 0
    st = ctypes.byref(_native.State(*([fake] * 7)))
    assert _native.lib.mg_host_step(P, st, fake, None, ctypes.byref(_native.Outputs()), None, 0, 0) == 0
    assert _native.lib.mg_host_observe(P, st, ctypes.byref(_native.Outputs()), 0) == 0


@pytest.mark.gpu
def test_host_step_equals_kernel():
    """The same inputs through mg_host_step and mg_step give the same bytes: every fp64 state word,
    the fp32 observations / rewards, the step record, the masks, the final observations and the
    statistics records. States span live episodes, finished ones driving on past the end point
    (the merge zone included) and the timeout; actions include None and invalid ones."""
    _host_step_equals_kernel(1 << 16, None)


@pytest.mark.gpu
@pytest.mark.parametrize("case", ["A", "C"])
def test_host_step_equals_kernel_at_params(case):
    """The same, every byte, at non-default mg_params (tests/params_cases.py): 4,096 envs, one launch.
    Both sides run the same source, so this pins the device compilation of every parameter's use to
    the host's, which tests/test_host_step.py compares with the parametrised oracle on the CPU."""
    _host_step_equals_kernel(4096, case)


def _host_step_equals_kernel(n, case):
    import torch

    from merging_gym import _native

    rng = np.random.default_rng(9)
    hb = HostBatch(n, case)
    c = pc.CASES[case or "default"]
    lo, hi = float(c.START_POINT) - 10, float(c.END_POINT) + 150  # 40 .. 1100 by default
    vmax = max(c.action_speeds) + 5.0
    near = 0.75 * c.VEHICLE_H
    hb.s["p1"][:] = rng.uniform(lo, hi, n)
    hb.s["p2"][:] = np.where(rng.random(n) < 0.3, hb.s["p1"] + rng.uniform(-near, near, n), rng.uniform(lo, hi, n))
    hb.s["v1"][:] = rng.uniform(0, vmax, n)
    hb.s["v2"][:] = rng.uniform(0, vmax, n)
    hb.s["ret1"][:] = rng.normal(0, 3, n)
    hb.s["ret2"][:] = rng.normal(0, 3, n)
    steps = rng.integers(0, hb.params.timeout_steps + 99, n)
    winner = rng.integers(0, 3, n)
    hb.tf[:] = (steps | (winner << 13) | ((rng.random(n) < 0.1) << 15)).astype(np.uint16)
    hb.stats["ret"] = rng.normal(0, 5, (n, 2))
    hb.stats["ret1_pending"] = rng.normal(0, 5, n)
    a1 = rng.integers(0, 5, n).astype(np.int8)
    a2 = rng.integers(-1, 5, n).astype(np.int8)
    a1[::997] = 7
    a2[5::1009] = 12
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in hb.s.items()}
    dtf = torch.from_numpy(hb.tf.view(np.int16).copy()).cuda()
    d = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dstate = _native.State(*(d(dev[k]) for k in ("p1", "v1", "p2", "v2", "ret1", "ret2")), d(dtf))
    dobs = torch.zeros((n, 10), dtype=torch.float32, device="cuda")
    drew = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    dflags = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    dfobs = torch.full((n, 10), float("nan"), device="cuda")
    words = (n + 63) // 64
    ddm = torch.zeros(words, dtype=torch.int64, device="cuda")
    dwm = torch.zeros(words, dtype=torch.int64, device="cuda")
    derr = torch.zeros(1, dtype=torch.int32, device="cuda")
    dstats = torch.from_numpy(hb.stats.view(np.uint8).reshape(n, 64).copy()).cuda()
    dout = _native.Outputs(d(dobs), d(drew), None, None, d(ddm), d(dfobs), None, d(derr), d(dwm), d(dflags))
    da1, da2 = torch.from_numpy(a1).cuda(), torch.from_numpy(a2).cuda()
    rc = _native.lib.mg_step(ctypes.byref(hb.params), ctypes.byref(dstate), d(da1), d(da2), ctypes.byref(dout),
                             ctypes.byref(_native.Stats(d(dstats))), n, _native.AUTORESET, None)
    _native.check(rc, "mg_step")
    torch.cuda.synchronize()
    hb.step(a1, a2)
    for k in hb.s:
        np.testing.assert_array_equal(dev[k].cpu().numpy().view(np.uint64), hb.s[k].view(np.uint64), err_msg=k)
    np.testing.assert_array_equal(dtf.cpu().numpy().view(np.uint16), hb.tf)
    np.testing.assert_array_equal(dobs.cpu().numpy().view(np.uint32), hb.obs.view(np.uint32))
    np.testing.assert_array_equal(dflags.cpu().numpy(), hb.flags)
    np.testing.assert_array_equal(ddm.cpu().numpy().view(np.uint64), hb.done_mask)
    np.testing.assert_array_equal(dwm.cpu().numpy().view(np.uint64), hb.won_mask)
    np.testing.assert_array_equal(dfobs.cpu().numpy(), hb.fobs)
    np.testing.assert_array_equal(dstats.cpu().numpy(), hb.stats.view(np.uint8).reshape(n, 64))
    np.testing.assert_array_equal(drew.cpu().numpy().view(np.uint32), hb.rew.view(np.uint32))
    assert derr.item() == hb.err[0] == 3
    assert hb.flags[:, 2].any() and hb.flags[:, 3].any() and np.isfinite(hb.fobs).any()


@pytest.mark.gpu
def test_host_step_equals_kernel_past_the_polynomial_range():
    """Far past the end point (|theta| >= 1/16: positions beyond ~2,875 m) sin / cos leave the shared
    polynomial: glibc on the host, the device library on the GPU. Live episodes reach this range (an
    arrived car keeps driving while the other runs the episode to the 2501-step timeout, to ~20 km),
    as do cars stepped on after a finished episode without autoreset. The state, rewards and flags stay bit-equal (they do
    not depend on sin / cos there: the cars are far apart), and the observations agree to 1 fp32 ulp
    (the doubles differ by at most an ulp before the fp32 rounding)."""
    import torch

    from merging_gym import _native

    n = 1 << 14
    rng = np.random.default_rng(10)
    hb = HostBatch(n)
    hb.s["p1"][:] = rng.uniform(2800, 20000, n)
    hb.s["p2"][:] = rng.uniform(-3000, 20000, n)
    hb.s["v1"][:] = rng.uniform(0, 45, n)
    hb.s["v2"][:] = rng.uniform(0, 45, n)
    hb.tf[:] = (rng.integers(0, 2600, n) | (rng.integers(0, 3, n) << 13)).astype(np.uint16)
    a1 = rng.integers(0, 5, n).astype(np.int8)
    a2 = rng.integers(-1, 5, n).astype(np.int8)
    dev = {k: torch.from_numpy(v.copy()).cuda() for k, v in hb.s.items()}
    dtf = torch.from_numpy(hb.tf.view(np.int16).copy()).cuda()
    d = lambda t: ctypes.c_void_p(t.data_ptr())  # noqa: E731
    dstate = _native.State(*(d(dev[k]) for k in ("p1", "v1", "p2", "v2", "ret1", "ret2")), d(dtf))
    dobs = torch.zeros((n, 10), dtype=torch.float32, device="cuda")
    drew = torch.zeros((n, 2), dtype=torch.float32, device="cuda")
    dflags = torch.zeros((n, 4), dtype=torch.uint8, device="cuda")
    dout = _native.Outputs(d(dobs), d(drew), None, None, None, None, None, None, None, d(dflags))
    da1, da2 = torch.from_numpy(a1).cuda(), torch.from_numpy(a2).cuda()
    rc = _native.lib.mg_step(ctypes.byref(hb.params), ctypes.byref(dstate), d(da1), d(da2), ctypes.byref(dout),
                             None, n, 0, None)
    _native.check(rc, "mg_step")
    torch.cuda.synchronize()
    hb.step(a1, a2, autoreset=False)
    for k in hb.s:
        np.testing.assert_array_equal(dev[k].cpu().numpy().view(np.uint64), hb.s[k].view(np.uint64), err_msg=k)
    np.testing.assert_array_equal(dtf.cpu().numpy().view(np.uint16), hb.tf)
    np.testing.assert_array_equal(dflags.cpu().numpy(), hb.flags)
    np.testing.assert_array_equal(drew.cpu().numpy().view(np.uint32), hb.rew.view(np.uint32))
    np.testing.assert_array_max_ulp(dobs.cpu().numpy(), hb.obs, maxulp=1)


def test_host_collision_test_over_the_whole_plane(coracle):
    """The step's collision test takes integer lateral edges where they equal the fp64 ones (y >= 8,
    csrc/mg_env.h vehicles_collide) and the fp64 form elsewhere. Pairs of cars placed over the
    whole reachable plane -- positions far past the end point, where the opponent's mirror arc
    crosses y = 8 and 0, and pairs packed within a few metres of each other around the merge point
    x = 0 -- collide exactly when the C oracle's fp64 boxes do (no autoreset, both cars held still)."""
    n = 1 << 16
    rng = np.random.default_rng(12)
    hb = HostBatch(n)
    base = rng.uniform(-3000, 9000, n)
    p1 = np.where(rng.random(n) < 0.5, base, rng.uniform(985, 1016, n))
    p2 = np.where(rng.random(n) < 0.7, p1 + rng.uniform(-10, 10, n), rng.uniform(-3000, 9000, n))
    for k, v in (("p1", p1), ("p2", p2)):
        hb.s[k][:] = v
    hb.s["v1"][:] = hb.s["v2"][:] = 0.0
    envs = coracle.new_envs(n)
    envs["pos1"], envs["pos2"] = p1, p2
    a1 = np.zeros(n, np.int8)  # target speed 0 from speed 0: the cars stay where they are
    hb.step(a1, None, autoreset=False)
    _, _, _, o_coll, _, _, err = coracle.step(envs, a1, None)
    assert err == 0
    np.testing.assert_array_equal(hb.flags[:, 3], o_coll)
    y2 = 150.0 - 30000.0 * (1 - np.cos(np.arctan2(1000, 30000) - p2 / 30000))
    # the fp64 branch runs (y2 < 8: the ego's arc stays at y >= 150, so those pairs never touch)
    assert o_coll.sum() > 1000 and (y2 < 8).sum() > 1000


def _near_touching_pairs(P, n, rng):
    """Positions (p1, p2) of n pairs of cars under P whose boxes nearly touch. The ego rides at
    y1 = W/2 + b1 and the opponent at y2 = W/2 - b2 with b = R (1 - cos theta) >= 0, so the lateral gap
    is b1 + b2 and x = R sin theta. Four populations:
      near    (most) gap within veh_w +- 1.2, both cars on the same side of the merge point, kept where
              |x1 - x2| <= veh_h + 1.2 -- about a fifth of them within veh_h +- 1.2;
      corner  a share of those resampled until |x1 - x2| is within veh_h +- 1.2 too;
      low     the ego a little above W/2 (b1 < 1) and the opponent placed veh_h +- 1.2 from it: with
              W/2 in [8, 2 veh_w) both lateral coordinates stay in that band (narrow boxes);
      plane   y1 over [W/2, 3 veh_w] and y2 over [0, W/2] with anything between them."""
    R, W, w, h = float(P.R), float(P.W), P.VEHICLE_W, P.VEHICLE_H
    ang0 = np.arctan2(P.H, P.R)
    th = lambda b: np.arccos(1.0 - b / R)  # noqa: E731
    m = 40 * n
    b2 = rng.uniform(0, min(W / 2, w + 1.2), m)
    b1 = rng.uniform(w - 1.2, w + 1.2, m) - b2
    ok = b1 >= 0
    b1, b2 = b1[ok], b2[ok]
    sgn = rng.choice([-1.0, 1.0], len(b1))
    t1, t2 = sgn * th(b1), sgn * th(b2)
    dx = np.abs(R * (np.sin(t1) - np.sin(t2)))
    near = np.flatnonzero(dx <= h + 1.2)
    corner = np.flatnonzero(np.abs(dx - h) <= 1.2)
    k_near, k_corner, k_low = int(0.45 * n), int(0.25 * n), int(0.15 * n)
    assert len(near) >= k_near and len(corner) >= k_corner, (len(near), len(corner))
    pick = np.concatenate([near[:k_near], corner[:k_corner]])
    t1, t2 = t1[pick], t2[pick]
    # low
    lb1 = rng.uniform(0, 1, k_low)
    lt1 = rng.choice([-1.0, 1.0], k_low) * th(lb1)
    ldx = rng.choice([-1.0, 1.0], k_low) * rng.uniform(h - 1.2, h + 1.2, k_low)
    lt2 = np.arcsin(np.sin(lt1) - ldx / R)
    # plane
    k_pl = n - len(pick) - k_low
    pt1 = rng.choice([-1.0, 1.0], k_pl) * th(rng.uniform(0, max(3 * w - W / 2, 1.0), k_pl))
    pt2 = rng.choice([-1.0, 1.0], k_pl) * th(rng.uniform(0, W / 2, k_pl))
    t1 = np.concatenate([t1, lt1, pt1])
    t2 = np.concatenate([t2, lt2, pt2])
    return R * (ang0 - t1), R * (ang0 - t2)


@pytest.mark.parametrize("w,h,W,R", [(14, 30, 24, 150), (40, 7, 60, 200), (5, 9, 18, 150)])
def test_host_collision_test_for_wide_boxes_at_small_y(coracle, w, h, W, R):
    """vehicles_collide's integer lateral edges (y >= 8) for boxes wider than the default: with
    veh_w / 2 > 2 a corner trunc(y) - veh_w / 2 is no longer within [y / 2, 2 y] for y in [8, 2 veh_w),
    where the default boxes' exactness argument lived. Pairs within veh_w +- 1.2 laterally and veh_h + 1.2
    longitudinally of each other (a share within veh_h +- 1.2: the corners), lateral coordinates on
    both sides of 8 and up to 3 veh_w, collide exactly when the parametrised C oracle's fp64 boxes do.
    R is small so that cars this close laterally can also be within a box length along the road; W
    puts the lane centre W / 2 inside [8, 2 veh_w)."""
    n = 1 << 16
    rng = np.random.default_rng(w)
    P = mo.OracleParams(R=R, H=R, W=W, VEHICLE_W=w, VEHICLE_H=h)
    p1, p2 = _near_touching_pairs(P, n, rng)
    hb = HostBatch(n, P)
    hb.s["p1"][:], hb.s["p2"][:] = p1, p2
    envs = coracle.new_envs(n)
    envs["pos1"], envs["pos2"] = p1, p2
    a1 = np.zeros(n, np.int8)  # target speed 0 from speed 0: the cars stay where they are
    hb.step(a1, None, autoreset=False)
    _, _, _, o_coll, _, _, err = coracle.step(envs, a1, None, params=P)
    assert err == 0
    np.testing.assert_array_equal(hb.s["p1"], p1)
    np.testing.assert_array_equal(hb.flags[:, 3], o_coll)
    np.testing.assert_array_equal(coracle.collided(envs, P), o_coll)
    ang0 = np.arctan2(R, R)
    y1 = W / 2 + R * (1 - np.cos(ang0 - p1 / R))
    y2 = W / 2 - R * (1 - np.cos(ang0 - p2 / R))
    band = (y1 >= 8) & (y1 < 2 * w) & (y2 >= 8) & (y2 < 2 * w)
    print(f"[collision plane {w}x{h}] {int(o_coll.sum())} collisions, {int(band.sum())} pairs with both y in "
          f"[8, {2 * w}), {int((band & o_coll.astype(bool)).sum())} of them colliding, y2 < 8: {int((y2 < 8).sum())}, "
          f"y1 max {y1.max():.1f}")
    assert o_coll.sum() > 1000 and band.sum() > 1000
    assert (y2 < 8).sum() > 1000 and y1.max() > 3 * w - 1 and y2.min() < 1


BAD_PARAMS = [
    ("timeout_steps", 0), ("timeout_steps", 8192), ("timeout_steps", -1),
    ("inv_R", 1.0 / 30000.0 * (1 + 2.0 ** -40)), ("qp_inv_nz", 1.0 / 90.0),
    ("R", 0.0), ("R", -30000.0), ("R", float("inf")), ("R", float("nan")),
    ("dT", 0.0), ("dT", -0.2), ("dT", float("inf")), ("dT", float("nan")),
    ("veh_w", 0), ("veh_w", -4), ("veh_h", 0), ("veh_h", -8),
]


@pytest.mark.parametrize("field,value", BAD_PARAMS)
def test_params_validation_names_the_field(field, value):
    """Every entry point that takes mg_params checks it on the host (csrc/mg_launch.h check_params):
    timeout_steps outside 1..8191 (the step count of mg_state.tf saturates at 8191, so a larger value
    would never time out), reciprocals that are not the rounded 1 / R and 1 / qp_nz (div_const needs
    them), and R, dT, veh_w, veh_h that are not positive and finite. The error names the field."""
    hb = HostBatch(4)
    hb.reset()
    setattr(hb.params, field, value)
    nat = hb.nat
    a1 = np.zeros(4, np.int8)
    calls = {
        "mg_host_step": lambda: nat.lib.mg_host_step(ctypes.byref(hb.params), ctypes.byref(hb.state),
                                                     ctypes.c_void_p(a1.ctypes.data), None, ctypes.byref(hb.out),
                                                     None, 4, 0),
        "mg_host_reset": lambda: nat.lib.mg_host_reset(ctypes.byref(hb.params), ctypes.byref(hb.state), None,
                                                       ctypes.byref(hb.out), 4),
        "mg_host_observe": lambda: nat.lib.mg_host_observe(ctypes.byref(hb.params), ctypes.byref(hb.state),
                                                           ctypes.byref(hb.out), 4),
    }
    before = {k: v.copy() for k, v in hb.s.items()}
    for what, call in calls.items():
        rc = call()
        msg = nat.lib.mg_last_error().decode()
        assert rc != 0 and field in msg and "mg_params" in msg, (what, rc, msg)
    for k, v in before.items():
        np.testing.assert_array_equal(hb.s[k], v)  # nothing ran
    with pytest.raises(nat.NativeError, match=field):
        hb.step(a1)


def test_largest_timeout_steps_is_accepted_and_times_out(coracle):
    """timeout_steps = 8191, the largest the step count can reach, is accepted and the episode times
    out on step 8191 exactly: a stopped pair (target speed 0, the opponent None from speed 0) started
    at step 8150 is done on the 41st step and not before. The oracle's time limit is set so that its
    clock rule gives the same step."""
    n = 3
    P = mo.OracleParams(start_vel=0.0, time_limit=8190 * 0.2 + 0.1)
    assert P.timeout_steps() == 8191
    hb = HostBatch(n, P)
    assert hb.params.timeout_steps == 8191
    hb.reset()
    hb.tf[:] = 8150
    envs = coracle.new_envs(n)
    coracle.reset(envs, P)
    envs["steps"] = 8150
    envs["time_stamp"] = P.clock(envs["steps"])
    a1 = np.zeros(n, np.int8)
    for k in range(8151, 8193):
        hb.step(a1, None, autoreset=False)
        _, _, o_done, _, _, _, _ = coracle.step(envs, a1, None, params=P)
        assert (hb.flags[:, 2] == (k >= 8191)).all(), k
        np.testing.assert_array_equal(hb.flags[:, 2], o_done)
        np.testing.assert_array_equal(hb.tf & 0x1FFF, min(k, 8191))


def test_fill_native_reproduces_the_default_params():
    """params_cases.fill_native's recipe for the derived fields (angle0, inv_R, the qp_* constants,
    timeout_steps by accumulation) gives mg_params_default's struct byte for byte at the default
    values, so the cases' structs are derived the way the library derives its own."""
    from merging_gym import _native

    assert bytes(pc.native_params("default")) == bytes(_native.default_params())
    for case in "ABCDEF":
        P = pc.native_params(case)
        assert P.inv_R == 1.0 / P.R and P.qp_inv_nz == 1.0 / P.qp_nz and 1 <= P.timeout_steps <= 8191
        assert abs(P.qp_nz * P.qp_inv_nz - 1) < 1e-15 and abs(P.qp_z0 / P.qp_nz * P.prediction_t - 1) < 1e-12
