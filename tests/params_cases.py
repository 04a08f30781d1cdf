"""Non-default mg_params cases shared by the tests (a plain module, not a conftest).

mg_params is public ABI (include/merging_hip.h) and every field is read on the hot path, so the
kernels are compared with the oracle away from the reference's default constants too. Each case is a
merge_oracle.OracleParams (what the oracle runs) and native_params(case) is the mg_params the library
runs, with every derived field recomputed the way mg_params_default does it for the defaults.

Cases A-D use values the reference itself can take through its module globals and action_dict;
tests/golden/reference_params_golden.npz pins the parametrised oracle to the reference's own runs of
them. Case E changes the three numbers the reference writes as literals (reset speed, reward
reference speed, time limit): the reference cannot run it, so for those fields the oracle is a
restatement with the literal replaced, and nothing more. Case F (an odd W) is an addition of the tests':
it is the one case in which the road width reaches an output at all.
"""

from __future__ import annotations

import numpy as np

import merge_oracle as mo

CASES = {
    "default": mo.OracleParams(),
    # every field off default at once; odd veh_h; angle0 = 0.040
    "A": mo.OracleParams(R=20000, H=800, W=120, dT=0.1, START_POINT=30, END_POINT=760,
                         action_speeds=(0, 7.5, 15, 22.5, 33), VEHICLE_W=6, VEHICLE_H=11, prediction_t=2.0,
                         RFirst=3.5, RSecond=0.25, RCollision=-4, vel_penalty=0.01, time_penalty=0.125),
    # the tight arc: angle0 = 1.28, sin / cos outside the polynomial range
    "B": mo.OracleParams(R=300, action_speeds=(0, 50, 100, 150, 200)),
    # both cars ride at y ~ 12 +- d, inside [8, 2 veh_w); unsorted speeds; angle0 = 0.0555
    "C": mo.OracleParams(R=9000, H=500, W=24, dT=0.5, START_POINT=10, END_POINT=480,
                         action_speeds=(40, 0, 20, 10, 30), VEHICLE_W=14, VEHICLE_H=30, prediction_t=5.0),
    # angle0 = 0.0588, just inside 1/16; 50 m per step; MPC gain 0.357 per step
    "D": mo.OracleParams(R=17000, dT=0.25, action_speeds=(0, 50, 100, 150, 200), VEHICLE_W=5, VEHICLE_H=9,
                         prediction_t=0.7),
    # the three literals; start_vel > max(speeds) takes finish_bound's other branch
    "E": mo.OracleParams(start_vel=33.0, vel_ref=12.5, time_limit=60, action_speeds=(0, 5, 10, 15, 25)),
    # a lane centre W / 2 = 16.5 that is no integer. In A-E it is one, and then W drops out of every
    # output: the observation holds only differences of lateral coordinates, and the boxes' pygame
    # truncation commutes with an integer offset -- a kernel with 150.0 for W / 2 passes A-E.
    "F": mo.OracleParams(R=9000, H=500, W=33, dT=0.25, START_POINT=10, END_POINT=480, VEHICLE_W=7, VEHICLE_H=12),
}

REFERENCE_CASES = ("A", "B", "C", "D")  # the ones the reference can run (the golden file's)


def timeout_steps(dT, limit=500) -> int:
    """The first k at which k sequential fp64 additions of dT exceed the limit (merging_env.py:141-142:
    `time_stamp += dT; time_stamp > limit`). Computed by accumulation, not by division: dT = 0.1 gives
    5000 (the sum overshoots 500 one step early), 0.25 gives 2001, 0.5 gives 1001, 0.2 gives 2501."""
    t, k = 0.0, 0
    while not t > limit:
        t += dT
        k += 1
    return k


def fill_native(P, case):
    """Set the mg_params P (a _native.Params, e.g. a MergeVecEnv's .params) to `case` in place: the
    plain fields, then the derived ones -- angle0, inv_R, end_point, the qp_* constants of the horizon
    and timeout_steps. Returns P."""
    c = CASES[case] if isinstance(case, str) else case
    P.R, P.H, P.W, P.dT = float(c.R), float(c.H), float(c.W), float(c.dT)
    P.r_first, P.r_second, P.r_collision = float(c.RFirst), float(c.RSecond), float(c.RCollision)
    P.vel_penalty, P.time_penalty = float(c.vel_penalty), float(c.time_penalty)
    P.start_point, P.end_point = float(c.START_POINT), float(c.END_POINT)
    P.start_vel, P.vel_ref, P.prediction_t = float(c.start_vel), float(c.vel_ref), float(c.prediction_t)
    for a, v in enumerate(c.action_speeds):
        P.action_speed[a] = float(v)
    P.veh_w, P.veh_h = int(c.VEHICLE_W), int(c.VEHICLE_H)
    P.angle0 = float(np.arctan2(c.H, c.R))
    P.inv_R = 1.0 / float(c.R)
    _, z, ztn, vsmall = mo.qpgen2_factor(float(c.prediction_t))
    P.qp_nz, P.qp_z0, P.qp_vsmall = ztn, z[0], vsmall
    P.qp_inv_nz = 1.0 / ztn
    P.timeout_steps = timeout_steps(float(c.dT), c.time_limit)
    return P


def native_params(case):
    """A fresh _native.Params for `case`: default_params() plus fill_native."""
    from merging_gym import _native

    return fill_native(_native.default_params(), case)


def scatter(case, n, rng, near_timeout=0.2):
    """Scattered mid-episode states for `case`, so a few hundred steps see collisions, arrivals in both
    orders and timeouts instead of thousands of steps from reset: positions between the start and a
    little past the end point (a share of the pairs within a box length of each other), speeds over the
    action speeds' range, and a share of the envs `near_timeout` within 40 steps of timeout_steps.
    Returns (p1, v1, p2, v2, steps, winner): winner follows from the positions (a car past the end
    point has arrived; the further one first), as live episodes have it."""
    c = CASES[case] if isinstance(case, str) else case
    lo, hi = float(c.START_POINT), float(c.END_POINT)
    vmax = float(max(max(c.action_speeds), c.start_vel))
    p1 = rng.uniform(lo, hi + 0.02 * (hi - lo), n)
    close = rng.random(n) < 0.4
    p2 = np.where(close, p1 + rng.uniform(-1.5, 1.5, n) * (c.VEHICLE_H + 2), rng.uniform(lo, hi + 0.02 * (hi - lo), n))
    v1, v2 = rng.uniform(0, vmax, n), rng.uniform(0, vmax, n)
    tmo = timeout_steps(float(c.dT), c.time_limit)
    steps = np.where(rng.random(n) < near_timeout, tmo - rng.integers(1, 40, n), rng.integers(0, max(1, tmo // 2), n))
    steps = np.maximum(steps, 0)
    a1, a2 = p1 > hi, p2 >= hi
    both = a1 & a2  # both past the end point would be a finished episode: pull the ego back
    p1 = np.where(both, hi - rng.uniform(1, 50, n), p1)
    a1 = p1 > hi
    winner = np.where(a1, 1, np.where(a2, 2, 0))
    return p1, v1, p2, v2, steps.astype(np.int64), winner.astype(np.int64)


def oracle_envs(coracle, case, p1, v1, p2, v2, steps, winner):
    """C-oracle envs holding these states: the clock is the same sequential fp64 sum of dT."""
    c = CASES[case] if isinstance(case, str) else case
    envs = coracle.new_envs(len(p1))
    envs["pos1"], envs["vel1"], envs["pos2"], envs["vel2"] = p1, v1, p2, v2
    envs["steps"], envs["winner"] = steps, winner
    envs["time_stamp"] = c.clock(steps)
    return envs


def load_scattered_device(env, case, rng, share=0.6):
    """Move a share of a freshly reset MergeVecEnv's envs (its .params already filled for `case`) to
    scatter() states: positions, speeds, step count and winner; returns and statistics stay zero."""
    import torch

    n = env.num_envs
    p1, v1, p2, v2, steps, winner = scatter(case, n, rng)
    m = rng.random(n) < share
    c = CASES[case] if isinstance(case, str) else case
    pick = lambda a, fresh: np.where(m, a, fresh)  # noqa: E731
    for name, a, fresh in (("p1", p1, float(c.START_POINT)), ("p2", p2, float(c.START_POINT)),
                           ("v1", v1, float(c.start_vel)), ("v2", v2, float(c.start_vel))):
        getattr(env, name).copy_(torch.from_numpy(pick(a, fresh)))
    tf = (pick(steps, 0) | (pick(winner, 0) << 13)).astype(np.uint16)
    env.tf.copy_(torch.from_numpy(tf.view(np.int16)))
    torch.cuda.synchronize()
