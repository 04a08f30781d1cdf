"""may_finish_next (csrc/mg_rollout_qnet.h): the config-5 kernels evaluate the ego's Q-net for an env whose
next step may end its episode even when the ego explores, because main.py:221 logs
eval_net(state)[action] of every episode's last step. The predicate must therefore flag EVERY step
that ends an episode. This restates it in numpy (same fp32 inputs: the observation the kernel keeps
in its tile row) and drives the C oracle through random, L0 and constant-action play -- collisions,
both arrival orders, same-step ties and timeouts at step 2501 -- checking that no finishing step goes
unflagged and that few steps are flagged. The device function itself is checked through q_eval
parity on the GPU (tests/test_gpu_qnet.py: an unflagged finish with a random action would log a value
of the observation instead of a Q-value)."""

from __future__ import annotations

import numpy as np
import pytest

import dataclasses

import merge_oracle
import params_cases as pc

DEFAULT = pc.CASES["default"]


def finish_bound(case=DEFAULT):
    """csrc/mg_rollout_qnet.h finish_bound's collision reach (lat, lon) for a case's params, restated:
    the passes climb from below until lat stops changing (the least fixed point of its own bound), with
    |sin| capped at 1 and lat at veh_w + 1.25 + 2 dl, rounded up to fp32."""
    veh_w, veh_h, R, dT = case.VEHICLE_W, case.VEHICLE_H, float(case.R), float(case.dT)
    dl = dT * (max(max(case.action_speeds), case.start_vel) + 0.5)
    cap = veh_w + 1.25 + 2.0 * dl
    lat = veh_w + 1.75
    for _ in range(4096):
        sn = min(1.0, np.sqrt(2.0 * lat / R) + dl / R)
        nxt = min(cap, veh_w + 1.0 + max(0.75, 2.0 * dl * sn + 0.25))
        if not nxt > lat:
            break
        lat = nxt
    latf = np.float32(lat)
    if latf < lat:
        latf = np.nextafter(latf, np.float32(np.inf))
    return latf, np.float32(veh_h + 1)


def launch_constants(case=DEFAULT):
    """FinishBound as launched (finish_bound in csrc/mg_rollout_qnet.h) plus the two mg_params fields
    may_finish_next reads: (smin, smax, g, lat, lon, dt, timeout_steps)."""
    f = np.float32
    _, z, ztn, _ = merge_oracle.qpgen2_factor(float(case.prediction_t))
    lat, lon = finish_bound(case)
    return (f(min(case.action_speeds)) - f(0.5), f(max(case.action_speeds)) + f(0.5),
            f(float(case.dT) * z[0] / ztn) * f(1.01), lat, lon, f(case.dT), case.timeout_steps())


def test_finish_bound_defaults_and_scaling():
    """The default params keep round 5's proven 5.75 / 9 m; the reach grows with the boxes, with a
    tighter arc (the lateral drift per step) and with faster action speeds."""
    rep = dataclasses.replace
    assert finish_bound() == (np.float32(5.75), np.float32(9.0))
    lat, lon = finish_bound(rep(DEFAULT, VEHICLE_W=14, VEHICLE_H=30))
    assert lat >= 15.75 and lon == 31.0
    lat_tight, _ = finish_bound(rep(DEFAULT, R=300.0))
    assert lat_tight > 5.75
    lat_fast, _ = finish_bound(rep(DEFAULT, R=3000.0, action_speeds=(0, 50, 100, 150, 200)))
    assert lat_fast > lat_tight - 1.0 and lat_fast > 5.75


@pytest.mark.parametrize("case", list(pc.CASES))
def test_finish_bound_is_a_bound(case):
    """The returned lat satisfies the inequality it is derived from, evaluated on lat itself:
    lat >= veh_w + 1 + max(0.75, 2 dl min(1, sqrt(2 lat / R) + dl / R) + 0.25). Four passes from below
    stopped under it at R = 300 with speeds to 200 (68.18 against the fixed point 71.24)."""
    c = pc.CASES[case]
    lat = float(finish_bound(c)[0])
    dl = float(c.dT) * (max(max(c.action_speeds), c.start_vel) + 0.5)
    need = c.VEHICLE_W + 1 + max(0.75, 2 * dl * min(1.0, np.sqrt(2 * lat / c.R) + dl / c.R) + 0.25)
    assert lat >= need, (case, lat, need)
    assert lat <= c.VEHICLE_W + 1.25 + 2 * dl + 1e-4


def may_finish(obs64, winner, steps, B=None):
    smin, smax, g, lat, lon, dt, timeout = B or launch_constants()
    o = obs64.astype(np.float32)
    f = np.float32
    ego = o[:, 3] < dt * np.maximum(o[:, 4], smax) + f(0.5)
    opp = o[:, 8] < dt * np.maximum(o[:, 9], smax) + f(0.5)
    arrive = np.where(winner == 1, opp, np.where(winner == 2, ego, ego & opp))
    spread = np.maximum(smax, np.maximum(o[:, 4], o[:, 9])) - np.minimum(smin, np.minimum(o[:, 4], o[:, 9]))
    rel = dt * (np.abs(o[:, 2]) + g * spread) + f(0.5)
    coll = (-o[:, 1] < lat) & (np.abs(o[:, 0]) < lon + rel)
    return (steps + 1 >= timeout) | arrive | coll


@pytest.fixture(scope="module")
def co():
    return merge_oracle.COracle(merge_oracle.build_c_oracle())


def _run(co, a1_fn, a2_fn, n, steps, rng, case=None):
    params = None if case is None else pc.CASES[case]
    B = launch_constants(params or DEFAULT)
    envs = co.new_envs(n)
    obs = co.reset(envs, params)
    flagged = finishes = missed = 0
    for k in range(steps):
        flag = may_finish(obs, envs["winner"], envs["steps"], B)
        a1, a2 = a1_fn(k, rng), a2_fn(k, rng)
        obs, rew, done, coll, status, _, err = co.step(envs, a1, a2, autoreset=True, params=params)
        assert err == 0
        d = done.astype(bool)
        missed += int((d & ~flag).sum())
        finishes += int(d.sum())
        flagged += int(flag.sum())
    return finishes, missed, flagged / (n * steps)


def test_may_finish_covers_every_finish(co):
    _covers_every_finish(co, None, 2048, 0.05, 1000, 10000)


@pytest.mark.parametrize("case", ["A", "B", "C", "D", "E"])
def test_may_finish_covers_every_finish_at_params(co, case):
    """Away from the default geometry (tests/params_cases.py) on the parametrised C oracle: no finish
    goes unflagged. The flagged share of a case -- over the env-steps of its three policies together --
    only has to stop the predicate passing by flagging everything (< 0.2); measured 0.9 % (A), 5.2 % (B),
    19.6 % (C), 5.5 % (D), 1.1 % (E). C's share is high because its episodes are short, not because the
    predicate is loose: the 14 x 30 boxes on a 24 m wide road collide in most episodes after about 14
    steps, the last four of them within reach (10.4 % in sticky play, 25 to 30 % in random play)."""
    _covers_every_finish(co, case, 1024, 0.2, 300, 3000)


def _covers_every_finish(co, case, n, max_frac, min_fin, min_total):
    rng = np.random.default_rng(5)
    timeout = (pc.CASES[case] if case else DEFAULT).timeout_steps()
    cases = {
        # uniform random both players (the bench / config-5 exploration regime)
        "uniform": (lambda k, r: r.integers(0, 5, n).astype(np.int8), lambda k, r: r.integers(0, 5, n).astype(np.int8)),
        # ego random, opponent None (L0)
        "l0": (lambda k, r: r.integers(0, 5, n).astype(np.int8), lambda k, r: None),
        # sticky policies: an action held for a random number of steps, so cars meet at every
        # speed difference and long episodes reach the timeout
        "sticky": (None, None),
    }
    held1 = rng.integers(0, 5, n).astype(np.int8)
    held2 = rng.integers(-1, 5, n).astype(np.int8)

    def sticky1(k, r):
        ch = r.random(n) < 0.02
        held1[ch] = r.integers(0, 5, int(ch.sum()))
        return held1.copy()

    def sticky2(k, r):
        ch = r.random(n) < 0.02
        held2[ch] = r.integers(-1, 5, int(ch.sum()))
        return held2.copy()

    cases["sticky"] = (sticky1, sticky2)
    total = 0
    flagged = env_steps = 0.0
    for name, (f1, f2) in cases.items():
        steps = 700 if name != "sticky" else timeout + 199
        fin, missed, frac = _run(co, f1, f2, n, steps, rng, case)
        assert missed == 0, (case, name, missed, fin)
        assert fin > min_fin, (case, name, fin)
        if case is None:
            assert frac < max_frac, (case, name, frac)
        total += fin
        flagged += frac * n * steps
        env_steps += n * steps
        print(f"[may_finish] {case or 'default'} {name}: {fin} finishes, all flagged; "
              f"{100 * frac:.2f} % of env-steps flagged")
    print(f"[may_finish] {case or 'default'}: {100 * flagged / env_steps:.2f} % of all env-steps flagged")
    assert flagged / env_steps < max_frac, (case, flagged / env_steps)
    assert total > min_total


def test_may_finish_known_answer_episodes(co):
    # SURVEY.md 8(a) KATs A-G: constant actions, collisions, arrivals in both orders, timeouts
    kats = [(2, -1), (0, -1), (4, -1), (4, 0), (0, 4), (3, 3), (1, 1)]
    n = len(kats)
    a1 = np.array([a for a, _ in kats], np.int8)
    a2 = np.array([b for _, b in kats], np.int8)
    envs = co.new_envs(n)
    obs = co.reset(envs)
    ends = np.zeros(n, np.int64)
    for k in range(2600):
        flag = may_finish(obs, envs["winner"], envs["steps"])
        obs, _, done, _, _, _, err = co.step(envs, a1, a2, autoreset=True)
        d = done.astype(bool)
        assert not (d & ~flag).any(), (k, np.flatnonzero(d & ~flag))
        ends[(ends == 0) & d] = k + 1
    assert ends.tolist() == [151, 2501, 225, 2501, 2501, 106, 288]
