"""CPU oracle for the MergingEnv step path -- TEST INFRASTRUCTURE ONLY.

Only tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg may import this module,
and only as the checker or the timed CPU baseline. The product (merging_gym) never calls it:
its step runs in libmerging_hip.so and fails loudly without it.

Two restatements of the reference algorithm live here:

* ``PyMergeEnv`` -- a scalar, pure-Python env with the reference's list API and its exact
  Python value types (int 0 rewards, int 900 gaps after reset, ...). It follows
  merging_gym/envs/merging_env.py (reference @ /root/reference) function by function:
  lon2coord :48-58, observe :118-132, action_to_acc :134-136 -> scripts/helper.py:152-191,
  step :138-195, is_collided :198-206, reset :208-230, corners :232-239.
* ``COracle`` -- ctypes binding of oracle/merge_oracle.c (same algorithm in C, batched,
  OpenMP), for the GPU parity tests at 4,096+ envs and for the CPU baseline.

Parity pinning: both are checked against tests/golden/reference_golden.npz, produced by
running the reference's own MergeEnv (tests/golden/gen_golden.py). Three third-party
boundaries (quadprog's QP solve, pygame Rect/Vector2, shapely intersects) were not
installable here; the oracle restates them (quadprog's qpgen2 equality step, C (int)
truncation + fp64 corner arithmetic, closed-box overlap) and their parity is pinned only
through the reference's call sites ("Oracle").
"""

from __future__ import annotations

import ctypes
import dataclasses
import math
import os
import subprocess

import numpy as np

# merging_env.py:22-46, :101 (values, not code)
R = 30000
H, W = 1000, 300
DT = 0.2
R_FIRST, R_SECOND, R_COLLISION = 2.0, 1.0, -10
VEL_PENALTY, TIME_PENALTY = 0.001, 0
START_POINT, END_POINT = 50, H - 50
VEHICLE_W, VEHICLE_H = 4, 8
PREDICTION_T = 3.0
ACTION_SPEED = {0: 0, 1: 10, 2: 20, 3: 30, 4: 40}


@dataclasses.dataclass(frozen=True)
class OracleParams:
    """The reference's module-level constants (merging_env.py:22-46), its action_dict (:101) and the
    three numbers it writes as literals: the reset speed start_vel (:216-217), the reward's reference
    speed vel_ref (:158-159) and the time limit (:142, `time_stamp += dT; time_stamp > limit` on the
    fp64 clock). Values keep the Python type they are given (the reference's ints stay ints, so an
    observation after reset holds the int END_POINT - START_POINT). Parameters travel per call:
    PyMergeEnv(params) and the params= argument of COracle's methods; None is DEFAULT_PARAMS."""

    R: float = R
    H: float = H
    W: float = W
    dT: float = DT
    RFirst: float = R_FIRST
    RSecond: float = R_SECOND
    RCollision: float = R_COLLISION
    vel_penalty: float = VEL_PENALTY
    time_penalty: float = TIME_PENALTY
    START_POINT: float = START_POINT
    END_POINT: float = END_POINT
    VEHICLE_W: int = VEHICLE_W
    VEHICLE_H: int = VEHICLE_H
    prediction_t: float = PREDICTION_T
    action_speeds: tuple = tuple(ACTION_SPEED[a] for a in range(5))
    start_vel: float = 20.0
    vel_ref: float = 20.0
    time_limit: float = 500

    def timeout_steps(self) -> int:
        """The first step whose clock exceeds the limit: the number of sequential fp64 additions of
        dT (from the int 0 of reset) after which time_stamp > time_limit."""
        t, k = 0, 0
        while not t > self.time_limit:
            t += self.dT
            k += 1
        return k

    def clock(self, steps):
        """time_stamp after `steps` steps (array or int): the same sequential fp64 sum."""
        steps = np.asarray(steps)
        top = int(steps.max()) if steps.size else 0
        ts = np.concatenate([[0.0], np.cumsum(np.full(top, float(self.dT)))])
        return ts[steps]

    def as_c(self) -> "OracleParamsC":
        c = OracleParamsC()
        for cname, name in _C_PARAM_FIELDS:
            setattr(c, cname, float(getattr(self, name)))
        c.action_speed = (ctypes.c_double * 5)(*[float(v) for v in self.action_speeds])
        c.veh_w, c.veh_h = int(self.VEHICLE_W), int(self.VEHICLE_H)
        return c


_C_PARAM_FIELDS = (("R", "R"), ("H", "H"), ("W", "W"), ("dT", "dT"), ("r_first", "RFirst"),
                   ("r_second", "RSecond"), ("r_collision", "RCollision"), ("vel_penalty", "vel_penalty"),
                   ("time_penalty", "time_penalty"), ("start_point", "START_POINT"),
                   ("end_point", "END_POINT"), ("prediction_t", "prediction_t"), ("start_vel", "start_vel"),
                   ("vel_ref", "vel_ref"), ("time_limit", "time_limit"))


class OracleParamsC(ctypes.Structure):
    """struct oracle_params in merge_oracle.c."""

    _fields_ = [(c, ctypes.c_double) for c, _ in _C_PARAM_FIELDS] + [
        ("action_speed", ctypes.c_double * 5), ("veh_w", ctypes.c_int32), ("veh_h", ctypes.c_int32)]


DEFAULT_PARAMS = OracleParams()


def arc_position(lon, ego: bool, params: OracleParams | None = None):
    """lon2coord (merging_env.py:48-58): longitudinal x and lateral y on the mirrored arcs."""
    p = params or DEFAULT_PARAMS
    theta = np.arctan2(p.H, p.R) - lon / p.R
    x = p.R * np.sin(theta)
    bulge = p.R - p.R * np.cos(theta)
    return x, (p.W / 2 + bulge) if ego else (p.W / 2 - bulge)


_QP_CACHE = {}


def qpgen2_factor(t):
    """The part of quadprog 0.1.11's qpgen2 that depends only on the horizon t, for mpc_1d's QP
    (helper.py:152-191 -> qpsolvers 1.8.0 -> quadprog.solve_qp, G = P = D'D + 0.01 I, one
    equality with normal n = A[1]): dpofa (G = R'R), dpori (J = R^-1, lower triangle zeroed), then
    for the normal n: d = J'n, z = J d and z'n, each sum in the Fortran loop order; plus qpgen2's
    vsmall probe. Restated from the published algorithm (Goldfarb & Idnani 1983 as coded in
    Turlach's solve.QP.f; LINPACK dpofa / dpori); quadprog is not in this image, so bit parity
    with it is unpinned. Returns (n, z, z'n, vsmall) for n of the positive sign."""
    if t in _QP_CACHE:
        return _QP_CACHE[t]
    steps = 10
    dt = t / steps
    # A[1] = row [0 1] of a^k b for k = 9..0 (helper.py:166-170): 0 * 0 + 1 * dt
    n = [0.0 * 0.0 + 1.0 * dt for _ in range(steps)]
    g = [[0.0] * steps for _ in range(steps)]  # g[i][j] = G(i, j), symmetric
    for i in range(steps - 1):
        g[i][i] += 1.0
        g[i + 1][i + 1] += 1.0
        g[i][i + 1] -= 1.0
        g[i + 1][i] -= 1.0
    for i in range(steps):
        g[i][i] += 0.01
    a = [row[:] for row in g]
    for j in range(steps):  # dpofa: upper triangle
        s = 0.0
        for k in range(j):
            dot = 0.0
            for m in range(k):
                dot = dot + a[m][k] * a[m][j]
            tk = (a[k][j] - dot) / a[k][k]
            a[k][j] = tk
            s = s + tk * tk
        a[j][j] = math.sqrt(a[j][j] - s)
    for k in range(steps):  # dpori
        a[k][k] = 1.0 / a[k][k]
        tk = -a[k][k]
        for i in range(k):
            a[i][k] = tk * a[i][k]
        for j in range(k + 1, steps):
            tj = a[k][j]
            a[k][j] = 0.0
            if tj != 0.0:
                for i in range(k + 1):
                    a[i][j] = a[i][j] + tj * a[i][k]
    for j in range(steps):  # lower triangle of dmat set to zero
        for i in range(j + 1, steps):
            a[i][j] = 0.0
    d = []
    for i in range(steps):
        s = 0.0
        for j in range(steps):
            s = s + a[j][i] * n[j]
        d.append(s)
    z = [0.0] * steps
    for j in range(steps):
        for i in range(steps):
            z[i] = z[i] + a[i][j] * d[j]
    ztn = 0.0
    for i in range(steps):
        ztn = ztn + z[i] * n[i]
    vsmall = 1e-60
    while True:
        vsmall = vsmall + vsmall
        if vsmall * 0.1 + 1.0 > 1.0 and vsmall * 0.2 + 1.0 > 1.0:
            break
    _QP_CACHE[t] = (n, z, ztn, vsmall)
    return _QP_CACHE[t]


def first_accel(x0, v0, xt, vt, t):
    """mpc_1d(...).action() (helper.py:152-191) restated as quadprog's qpgen2 solves it.

    The reference keeps only the velocity row of the 10-step constraint (:172-173, :182): the
    residual is b = vt - (0 x0 + 1 v0), the equality's normal n = A[1]. qpsolvers hands quadprog
    C = -n, b_c = -b; qpgen2 starts at the unconstrained minimiser sol = 0, evaluates the
    residual -b_c + C'sol, zeroes it below vsmall, negates an equality whose residual is positive,
    and takes the full step t = -sv / z'n along z = J J'n. The sign flips are exact negations, so
    the magnitudes come from qpgen2_factor(t)."""
    n, z, ztn, vsmall = qpgen2_factor(t)
    rhs = vt - (0.0 * x0 + 1.0 * v0)
    sol0 = -0.0  # dposl on a = -q = -0.0 leaves every entry -0.0 (the unconstrained minimiser)
    res = rhs  # -b_c + sum(C * sol), the products all zero
    if abs(res) < vsmall:
        res = 0.0
    if not res:
        return sol0  # nothing violated
    sign = 1.0 if res > 0 else -1.0  # positive residual: C negated back to +n
    sv = -abs(res)
    tt = -sv / ztn
    return sol0 + tt * (sign * z[0])


def vehicle_box(lateral, longitudinal, params: OracleParams | None = None):
    """corners(agent, y=x, x=y, 0) (merging_env.py:232-239) as a closed box.

    pygame's Rect(center=(lateral, longitudinal)) truncates the float centre with a C (int)
    cast and subtracts w//2, h//2 (w=VEHICLE_W=4 lateral, h=VEHICLE_H=8 longitudinal; the
    surfaces are make_surface(ones([4, 8])), :97-98). Each Vector2 corner is
    (corner - pivot).rotate(0) * 1.0 + pivot in fp64.
    """
    p = params or DEFAULT_PARAMS
    left = int(lateral) - p.VEHICLE_W // 2
    top = int(longitudinal) - p.VEHICLE_H // 2
    xs = [(float(c) - lateral) + lateral for c in (left, left + p.VEHICLE_W)]
    ys = [(float(c) - longitudinal) + longitudinal for c in (top, top + p.VEHICLE_H)]
    return min(xs), max(xs), min(ys), max(ys)


def boxes_touch(b1, b2) -> bool:
    """shapely Polygon.intersects for two axis-aligned rectangles: closed overlap."""
    return b1[0] <= b2[1] and b2[0] <= b1[1] and b1[2] <= b2[3] and b2[2] <= b1[3]


class PyMergeEnv:
    """Scalar restatement of MergeEnv's step/reset path with the reference's list API."""

    def __init__(self, params: OracleParams | None = None):
        self.params = params or DEFAULT_PARAMS
        self.action_dict = dict(enumerate(self.params.action_speeds))
        self.reset()

    def reset(self):
        # merging_env.py:208-230 (deterministic start; the random start is commented out)
        p = self.params
        self.done = False
        self.winner = None
        self.time_stamp = 0
        self.state1 = {"pos": p.START_POINT, "vel": p.start_vel, "acc": 0.0}
        self.state2 = {"pos": p.START_POINT, "vel": p.start_vel, "acc": 0.0}
        self.r1_accumulate = 0
        self.r2_accumulate = 0
        return self.observe()

    def observe(self):
        p = self.params
        x1, y1 = arc_position(self.state1["pos"], True, p)
        x2, y2 = arc_position(self.state2["pos"], False, p)
        s1, s2 = self.state1, self.state2
        return [x2 - x1, y2 - y1, s2["vel"] - s1["vel"], p.END_POINT - s1["pos"], s1["vel"],
                x1 - x2, y1 - y2, s1["vel"] - s2["vel"], p.END_POINT - s2["pos"], s2["vel"]]

    def _advance(self, car, action):
        p = self.params
        vt = self.action_dict[action]  # KeyError for an invalid action, as the reference
        car["acc"] = first_accel(car["pos"], car["vel"], car["pos"] + vt * p.prediction_t, vt,
                                 p.prediction_t)
        car["vel"] = max(0, car["vel"] + car["acc"] * p.dT)
        car["pos"] += car["vel"] * p.dT

    def collided(self):
        p = self.params
        x1, y1 = arc_position(self.state1["pos"], True, p)
        x2, y2 = arc_position(self.state2["pos"], False, p)
        return boxes_touch(vehicle_box(y1, x1, p), vehicle_box(y2, x2, p))

    def step(self, action1, action2=None):
        # merging_env.py:138-195
        p = self.params
        self.time_stamp += p.dT
        if self.time_stamp > p.time_limit:
            self.done = True
        info = {"collision": False}
        self._advance(self.state1, action1)
        if action2 is None:
            self.state2["acc"] = 0
            self.state2["vel"] = max(0, self.state2["vel"] + 0 * p.dT)
            self.state2["pos"] += self.state2["vel"] * p.dT
        else:
            self._advance(self.state2, action2)
        obs = self.observe()
        r1 = -p.time_penalty - p.vel_penalty * np.abs(self.state1["vel"] - p.vel_ref)
        r2 = -p.time_penalty - p.vel_penalty * np.abs(self.state2["vel"] - p.vel_ref)
        # arrival: ego strict, opponent non-strict; the first arrival wins
        if self.state1["pos"] > p.END_POINT:
            if self.winner is None:
                self.winner, r1 = 1, r1 + p.RFirst
            elif self.winner == 1:
                r1 = 0
            else:
                r1, self.done = r1 + p.RSecond, True
        if self.state2["pos"] >= p.END_POINT:
            if self.winner is None:
                self.winner, r2 = 2, r2 + p.RFirst
            elif self.winner == 2:
                r2 = 0
            else:
                r2, self.done = r2 + p.RSecond, True
        if self.collided():
            self.done = True
            r1 += p.RCollision
            r2 += p.RCollision
            info["collision"] = True
        # np.float64 -> float so the list holds plain Python numbers like the reference's
        r1 = r1 if isinstance(r1, int) else float(r1)
        r2 = r2 if isinstance(r2, int) else float(r2)
        self.r1_accumulate += r1
        self.r2_accumulate += r2
        return [_plain(v) for v in obs], [r1, r2], self.done, info


def _plain(v):
    return v if isinstance(v, int) else float(v)


# --------------------------------------------------------------------------- C oracle

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "build", "libmerge_oracle.so")


class OracleEnvC(ctypes.Structure):
    """struct oracle_env in merge_oracle.c (one env, the reference's state fields)."""

    _fields_ = [
        ("pos1", ctypes.c_double), ("vel1", ctypes.c_double), ("acc1", ctypes.c_double),
        ("pos2", ctypes.c_double), ("vel2", ctypes.c_double), ("acc2", ctypes.c_double),
        ("time_stamp", ctypes.c_double), ("r1_acc", ctypes.c_double), ("r2_acc", ctypes.c_double),
        ("ep_reward_main", ctypes.c_double), ("winner", ctypes.c_int32), ("done", ctypes.c_int32),
        ("steps", ctypes.c_int32), ("pad_", ctypes.c_int32),
    ]


STATS_DOC = "ret_sum [n,3]: r1_accumulate, r2_accumulate, main.py ep_reward; counts [n,6]: " \
    "episodes, collisions, ego_first, steps, win_main, win_hdqn"


def new_stats(n):
    """Zeroed (ret_sum [n,3] f64, counts [n,6] u32) for COracle.step / rollout_random."""
    return np.zeros((n, 3)), np.zeros((n, 6), np.uint32)


ENV_DTYPE = np.dtype([(n, np.float64) for n in (
    "pos1", "vel1", "acc1", "pos2", "vel2", "acc2", "time_stamp", "r1_acc", "r2_acc", "ep_reward_main")]
    + [("winner", np.int32), ("done", np.int32), ("steps", np.int32), ("pad_", np.int32)])


def build_c_oracle(force: bool = False) -> str:
    """Compile oracle/merge_oracle.c with gcc (no contraction, no fast-math)."""
    if force or not os.path.exists(LIB_PATH) or (
            os.path.getmtime(LIB_PATH) < os.path.getmtime(os.path.join(_HERE, "merge_oracle.c"))):
        subprocess.check_call(["make", "-s", "-C", _HERE])
    return LIB_PATH


def _ptr(a, ctype):
    return a.ctypes.data_as(ctypes.POINTER(ctype)) if a is not None else None


class COracle:
    """Batched C restatement. Arrays are numpy; envs is a structured array of ENV_DTYPE."""

    def __init__(self, path: str | None = None):
        path = path or LIB_PATH
        if not os.path.exists(path):
            raise FileNotFoundError(f"{path} missing: run `make -C oracle` (or __graft_entry__.build())")
        lib = ctypes.CDLL(path)
        P = ctypes.POINTER
        lib.oracle_reset_batch.argtypes = [ctypes.c_void_p, ctypes.c_int64, P(ctypes.c_double)]
        lib.oracle_observe_batch.argtypes = [ctypes.c_void_p, ctypes.c_int64, P(ctypes.c_double)]
        lib.oracle_step_batch.argtypes = [
            ctypes.c_void_p, ctypes.c_int64, P(ctypes.c_int8), P(ctypes.c_int8), ctypes.c_int32,
            P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_uint8), P(ctypes.c_uint8),
            P(ctypes.c_double), P(ctypes.c_double), P(ctypes.c_uint32), P(ctypes.c_uint32),
            ctypes.c_int32]
        lib.oracle_step_batch.restype = ctypes.c_int32
        lib.oracle_philox4x32_10.argtypes = [P(ctypes.c_uint32), P(ctypes.c_uint32), P(ctypes.c_uint32)]
        lib.oracle_random_actions.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
                                              ctypes.c_uint64, ctypes.c_int32, P(ctypes.c_int8),
                                              P(ctypes.c_int8)]
        lib.oracle_rollout_random.argtypes = [
            ctypes.c_void_p, ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64,
            ctypes.c_uint64, ctypes.c_int32, ctypes.c_int64, P(ctypes.c_double), P(ctypes.c_uint32)]
        lib.oracle_rollout_random.restype = ctypes.c_int64
        lib.oracle_philox_batch.argtypes = [ctypes.c_int64, ctypes.c_int64, ctypes.c_uint64, ctypes.c_uint64,
                                            P(ctypes.c_uint32)]
        lib.oracle_mpc_first_accel.argtypes = [ctypes.c_double] * 5
        lib.oracle_mpc_first_accel.restype = ctypes.c_double
        PP = P(OracleParamsC)
        lib.oracle_reset_batch_p.argtypes = [PP] + lib.oracle_reset_batch.argtypes
        lib.oracle_observe_batch_p.argtypes = [PP] + lib.oracle_observe_batch.argtypes
        lib.oracle_collided_batch_p.argtypes = [PP, ctypes.c_void_p, ctypes.c_int64, P(ctypes.c_uint8)]
        lib.oracle_step_batch_p.argtypes = [PP] + lib.oracle_step_batch.argtypes[:-1]
        lib.oracle_step_batch_p.restype = ctypes.c_int32
        lib.oracle_rollout_random_p.argtypes = [PP] + lib.oracle_rollout_random.argtypes
        lib.oracle_rollout_random_p.restype = ctypes.c_int64
        lib.oracle_mpc_first_accel_p.argtypes = [PP, ctypes.c_double, ctypes.c_double, ctypes.c_int32]
        lib.oracle_mpc_first_accel_p.restype = ctypes.c_double
        lib.oracle_params_size.restype = ctypes.c_int32
        if lib.oracle_params_size() != ctypes.sizeof(OracleParamsC):
            raise ImportError("oracle_params layout differs between merge_oracle.c and merge_oracle.py")
        lib.oracle_set_threads.argtypes = [ctypes.c_int32]
        lib.oracle_max_threads.restype = ctypes.c_int32
        self.lib = lib

    def set_threads(self, n: int) -> None:
        self.lib.oracle_set_threads(int(n))

    def max_threads(self) -> int:
        return int(self.lib.oracle_max_threads())

    @staticmethod
    def new_envs(n: int) -> np.ndarray:
        return np.zeros(n, dtype=ENV_DTYPE)

    def observe(self, envs: np.ndarray, params: OracleParams | None = None) -> np.ndarray:
        """observe() (merging_env.py:118-132) of every env in fp64, no state change."""
        obs = np.empty((len(envs), 10), np.float64)
        if params is None:
            self.lib.oracle_observe_batch(envs.ctypes.data, len(envs), _ptr(obs, ctypes.c_double))
        else:
            self.lib.oracle_observe_batch_p(ctypes.byref(params.as_c()), envs.ctypes.data, len(envs),
                                            _ptr(obs, ctypes.c_double))
        return obs

    def reset(self, envs: np.ndarray, params: OracleParams | None = None) -> np.ndarray:
        obs = np.empty((len(envs), 10), np.float64)
        if params is None:
            self.lib.oracle_reset_batch(envs.ctypes.data, len(envs), _ptr(obs, ctypes.c_double))
        else:
            self.lib.oracle_reset_batch_p(ctypes.byref(params.as_c()), envs.ctypes.data, len(envs),
                                          _ptr(obs, ctypes.c_double))
        return obs

    def collided(self, envs: np.ndarray, params: OracleParams | None = None) -> np.ndarray:
        """is_collided() (merging_env.py:198-206) of every env, no state change."""
        coll = np.empty(len(envs), np.uint8)
        self.lib.oracle_collided_batch_p(ctypes.byref((params or DEFAULT_PARAMS).as_c()), envs.ctypes.data,
                                         len(envs), _ptr(coll, ctypes.c_uint8))
        return coll

    def step(self, envs, a1, a2=None, autoreset=False, final_obs=False, stats=None, params=None):
        """One step of every env. Returns obs[n,10] f64, rew[n,2] f64, done[n] u8, coll[n] u8,
        status[n] u32 (MG_ST_* bits), and final_obs[n,10] (NaN rows for envs not finished).
        stats = (ret_sum [n,3] f64, counts [n,6] u32), accumulated at autoreset: the sums of
        r1_accumulate, r2_accumulate and main.py's winner-filtered ep_reward; episodes,
        collisions, ego-first arrivals, steps, main.py:225 wins and hdqn.py:342 wins
        (STATS_DOC)."""
        n = len(envs)
        a1 = np.ascontiguousarray(a1, np.int8)
        a2 = None if a2 is None else np.ascontiguousarray(a2, np.int8)
        obs = np.empty((n, 10), np.float64)
        rew = np.empty((n, 2), np.float64)
        done = np.empty(n, np.uint8)
        coll = np.empty(n, np.uint8)
        status = np.empty(n, np.uint32)
        fobs = np.full((n, 10), np.nan) if final_obs else None
        ret_sum, counts = (None, None) if stats is None else stats
        args = (envs.ctypes.data, n, _ptr(a1, ctypes.c_int8), _ptr(a2, ctypes.c_int8),
                int(bool(autoreset)), _ptr(obs, ctypes.c_double), _ptr(rew, ctypes.c_double),
                _ptr(done, ctypes.c_uint8), _ptr(coll, ctypes.c_uint8), _ptr(fobs, ctypes.c_double),
                _ptr(ret_sum, ctypes.c_double), _ptr(counts, ctypes.c_uint32),
                _ptr(status, ctypes.c_uint32))
        if params is None:
            err = self.lib.oracle_step_batch(*args, 0)
        else:
            err = self.lib.oracle_step_batch_p(ctypes.byref(params.as_c()), *args)
        return obs, rew, done, coll, status, fobs, err

    def mpc_first_accel(self, x0, v0, xt, vt, t=3.0):
        """mpc_1d(x0, v0, xt, vt, t).action() with the QP solved in C (helper.py:152-191)."""
        return float(self.lib.oracle_mpc_first_accel(x0, v0, xt, vt, t))

    def mpc_first_accel_p(self, params: OracleParams, x0, v0, action):
        """action_to_acc (merging_env.py:134-136, :147) of `action` from (x0, v0) under params."""
        return float(self.lib.oracle_mpc_first_accel_p(ctypes.byref(params.as_c()), x0, v0, int(action)))

    def philox(self, ctr, key):
        c = np.ascontiguousarray(ctr, np.uint32)
        k = np.ascontiguousarray(key, np.uint32)
        out = np.empty(4, np.uint32)
        self.lib.oracle_philox4x32_10(_ptr(c, ctypes.c_uint32), _ptr(k, ctypes.c_uint32),
                                      _ptr(out, ctypes.c_uint32))
        return out

    def philox_batch(self, n, env_offset, seed, step_idx):
        """[n, 4] uint32 Philox words for (env_offset + i, step_idx) under key seed."""
        out = np.empty((n, 4), np.uint32)
        self.lib.oracle_philox_batch(n, env_offset, seed, step_idx, _ptr(out, ctypes.c_uint32))
        return out

    def random_actions(self, n, env_offset, seed, step_idx, opponent_random):
        a1 = np.empty(n, np.int8)
        a2 = np.empty(n, np.int8)
        self.lib.oracle_random_actions(n, env_offset, seed, step_idx, int(opponent_random),
                                       _ptr(a1, ctypes.c_int8), _ptr(a2, ctypes.c_int8))
        return a1, a2

    def rollout_random(self, envs, steps, seed, first_step, opponent_random, env_offset=0,
                       stats=None, params=None):
        """`steps` autoreset steps with Philox actions (the bench workload). Returns the
        number of env-steps done."""
        ret_sum, counts = (None, None) if stats is None else stats
        args = (envs.ctypes.data, len(envs), int(steps), int(seed), int(first_step),
                int(opponent_random), int(env_offset), _ptr(ret_sum, ctypes.c_double),
                _ptr(counts, ctypes.c_uint32))
        if params is None:
            return int(self.lib.oracle_rollout_random(*args))
        return int(self.lib.oracle_rollout_random_p(ctypes.byref(params.as_c()), *args))


# --------------------------------------------------------------------------- DQN policy oracle

def qnet_reference(weights, obs, bf16: bool = True, swap: bool = False):
    """The reference Net (scripts/main.py:30-47) on CPU: fc1 -> ReLU -> fc2 -> ReLU -> out.

    bf16=True rounds the input, every weight and each hidden activation to bf16 (round to
    nearest even) and sums in fp32 -- what the MFMA kernel computes up to summation order.
    bf16=False is the reference's own fp32 forward. swap feeds state[5:] + state[:5]
    (main.py:199)."""
    import torch

    x = torch.as_tensor(np.asarray(obs, np.float32))
    if swap:
        x = torch.cat([x[:, 5:], x[:, :5]], dim=1)
    ws = [torch.as_tensor(np.asarray(weights[k], np.float32)) for k in
          ("fc1.weight", "fc2.weight", "out.weight")]
    bs = [torch.as_tensor(np.asarray(weights[k], np.float32)) for k in ("fc1.bias", "fc2.bias", "out.bias")]
    rnd = (lambda t: t.to(torch.bfloat16).to(torch.float32)) if bf16 else (lambda t: t)
    h = rnd(x)
    for i, (w, b) in enumerate(zip(ws, bs)):
        h = h @ rnd(w).T + b
        if i < 2:
            h = rnd(torch.relu(h))
    return h.numpy()


def _bf16(a):
    """fp32 -> bf16 (round to nearest even) -> back, as v_cvt_pk_bf16_f32 / static_cast<__bf16>."""
    import torch

    return torch.as_tensor(np.asarray(a, np.float32)).to(torch.bfloat16).to(torch.float32).numpy()


def _bias_parts(b):
    """csrc/mg_qnet.h qnet_pack_kernel's three-way split b = hi + mid + lo of an fp32 bias into bf16
    parts (the padded K slots whose input is 1.0)."""
    b = np.asarray(b, np.float32)
    hi = _bf16(b)
    r = (b - hi).astype(np.float32)
    mid = _bf16(r)
    lo = _bf16((r - mid).astype(np.float32))
    return hi, mid, lo


def _unit1(kb, g, j):  # csrc/mg_qnet.h qnet_unit1: hidden-1 unit at k = 8 g + j of layer-2 k-block kb
    return 32 * kb + (j & 3) + 8 * (j >> 2) + 16 * (g & 1) + 4 * (g >> 1)


def _unit2(kb, g, j):  # csrc/mg_qnet.h qnet_unit2: hidden-2 unit at k = 8 g + j of layer-3 k-block kb
    return 32 * kb + 16 * (j >> 2) + 4 * g + (j & 3)


def _unit32(s, h, j):  # the 32x32 layout: unit at k = 8 h + j of k-block s
    return 16 * s + 8 * (j >> 2) + 4 * h + (j & 3)


def _k_order(unit, blocks, groups):
    return np.array([unit(kb, g, j) for kb in range(blocks) for g in range(groups) for j in range(8)])


_MFMA_LIB = None


def _mfma_lib():
    """oracle_mfma_layer / oracle_mfma_dots of the C oracle: the gfx950 bf16 MFMA accumulation rule."""
    global _MFMA_LIB
    if _MFMA_LIB is None:
        lib = ctypes.CDLL(build_c_oracle())
        P = ctypes.c_void_p
        lib.oracle_mfma_layer.argtypes = [ctypes.c_int64, ctypes.c_int32, ctypes.c_int32, P, P, P]
        lib.oracle_mfma_dots.argtypes = [ctypes.c_int64, ctypes.c_int32, P, P, P, P]
        _MFMA_LIB = lib
    return _MFMA_LIB


def bf16_bits(a):
    """fp32 -> bf16 bit patterns, round to nearest even (v_cvt_pk_bf16_f32)."""
    u = np.ascontiguousarray(a, np.float32).view(np.uint32).astype(np.uint64)
    return ((u + 0x7FFF + ((u >> 16) & 1)) >> 16).astype(np.uint16)


def mfma_dots(a_bits, b_bits, c):
    """out[r] = c[r] + sum_k a[r, k] b[r, k] as one chain of bf16 MFMAs accumulates it (oracle_mfma_dots):
    a_bits, b_bits [n, K] bf16 bit patterns, c [n] fp32. See oracle_mfma_layer's rule (merge_oracle.c)."""
    a = np.ascontiguousarray(a_bits, np.uint16)
    b = np.ascontiguousarray(b_bits, np.uint16)
    c = np.ascontiguousarray(c, np.float32)
    out = np.empty(len(c), np.float32)
    _mfma_lib().oracle_mfma_dots(len(c), a.shape[1], a.ctypes.data, b.ctypes.data, c.ctypes.data, out.ctypes.data)
    return out


def qnet_reference_mfma(weights, x, swap: bool = False, form: str = "16x16", rule: str = "mfma"):
    """The Net forward (scripts/main.py:30-47, scripts/hdqn.py:38-55: fc1 -> ReLU -> fc2 -> ReLU -> out)
    as the kernels' matrix cores compute it: bf16 operands in the kernels' packed k order, each layer
    one chain of MFMAs per output.
    rule "mfma" (default): the gfx950 accumulation rule measured in round 6 (oracle_mfma_layer in
      merge_oracle.c: per group of 8 k, products truncated toward zero and the running value floored
      onto 2^(nom - 24), the sum floored onto 2^(E - 31) and rounded to nearest even); it reproduces
      every one of 4.0 M probe outputs of both instructions (tests/test_oracle_mfma.py,
      profiles/r06/mfma_rule.txt) and mg_qnet_forward's Q rows bit for bit (profiles/r06/mfma_order.txt).
    rule "exact8": round 5's model (each group's exact sum rounded once into the accumulator), kept for
      the order study; rule "exact": each MFMA's exact K sum rounded once.
      layer 1   one 32x32x16 MFMA over the 16 input slots: features 0..in-1, b1's three bf16 parts at
                slots 13..15 (inputs 1.0);
      layer 2   form "16x16" (net opponents, h-DQN, mg_qnet_forward): 7 k-blocks of 32 hidden-1 units
                in qnet_unit1 order; "32x32" (config 5 without a net opponent): 14 blocks of 16;
                b2's parts at units 200..202 (outputs 1.0);
      layer 3   likewise over hidden-2 (qnet_unit2 order / blocks of 16), b3's parts at units 100..102.
    ReLU after the bf16 rounding of each hidden accumulator (v_cvt_pk_bf16_f32 then max_i16(., 0)).
    x: [n, in] fp32 (10 or 11 features); swap feeds x[5:] + x[:5] (in 10 only). Returns q [n, out]."""
    x = np.asarray(x, np.float32)
    if swap:
        x = np.concatenate([x[:, 5:], x[:, :5]], axis=1)
    n, din = x.shape
    w1, w2, w3 = (np.asarray(weights[k], np.float32) for k in ("fc1.weight", "fc2.weight", "out.weight"))
    b1, b2, b3 = (np.asarray(weights[k], np.float32) for k in ("fc1.bias", "fc2.bias", "out.bias"))
    if form == "16x16":
        o2, o3, blk = _k_order(_unit1, 7, 4), _k_order(_unit2, 4, 4), 32
    elif form == "32x32":
        o2, o3, blk = _k_order(_unit32, 14, 2), _k_order(_unit32, 8, 2), 16
    else:
        raise ValueError(form)

    def matrix(w, b, kin, kpad, ones_at):
        m = np.zeros((w.shape[0], kpad), np.float32)
        m[:, :kin] = _bf16(w)
        for j, part in enumerate(_bias_parts(b)):
            m[:, ones_at + j] = part
        return m

    def layer(h, m, blk):
        if rule == "mfma":
            hb, mb = bf16_bits(h), bf16_bits(m)
            out = np.empty((h.shape[0], m.shape[0]), np.float32)
            _mfma_lib().oracle_mfma_layer(h.shape[0], h.shape[1], m.shape[0], hb.ctypes.data, mb.ctypes.data,
                                          out.ctypes.data)
            return out
        ld = np.longdouble
        acc = np.zeros((h.shape[0], m.shape[0]), np.float32)
        g = 8 if rule == "exact8" else blk
        for k0 in range(0, m.shape[1], g):
            s = h[:, k0:k0 + g].astype(ld) @ m[:, k0:k0 + g].astype(ld).T  # exact
            acc = (acc.astype(ld) + s).astype(np.float32)
        return acc

    def hidden(acc, width, ones_at):
        h = np.zeros((acc.shape[0], width), np.float32)
        h[:, :acc.shape[1]] = np.maximum(_bf16(acc), 0.0)  # -0.0 -> +0.0 as max_i16
        h[:, ones_at:ones_at + 3] = 1.0
        return h

    xin = np.zeros((n, 16), np.float32)
    xin[:, :din] = _bf16(x)
    xin[:, 13:16] = 1.0
    a1 = layer(xin, matrix(w1, b1, din, 16, 13), 16)
    h1 = np.ascontiguousarray(hidden(a1, 16 * 14, 200)[:, o2])
    a2 = layer(h1, np.ascontiguousarray(matrix(w2, b2, 200, 16 * 14, 200)[:, o2]), blk)
    h2 = np.ascontiguousarray(hidden(a2, 128, 100)[:, o3])
    return layer(h2, np.ascontiguousarray(matrix(w3, b3, 100, 128, 100)[:, o3]), blk)


def qnet_policy_draws(words, step, opponent):
    """The epsilon-greedy draws of mg_rollout_qnet at global step `step` (csrc/mg_rollout_qnet.h
    qnet_policy_step_n, ABI 20), restated: words(c) -> [n, 4] uint32 Philox4x32-10 words of counter
    (gi, c) for the envs checked. opponent "none" / "uniform" (two draws per step, one call per two
    steps): words (x, y) of call step div 2 on even steps, (z, w) on odd ones; explore = the first,
    the random action floor(5 w / 2^32) of the second -- or with the uniform opponent the pair
    x = floor(25 w / 2^32), a1 = x div 5, a2 = x mod 5. Net opponents ("self" / "other"): call `step`,
    (x, y) the ego's explore / random action, (z, w) the opponent's. Returns (explore [n] u64,
    random a1 [n], opponent explore [n] u64 or None, random a2 [n] or None)."""
    if opponent in ("none", "uniform"):
        u = words(step >> 1).astype(np.uint64)
        ex, pick = (u[:, 2], u[:, 3]) if step & 1 else (u[:, 0], u[:, 1])
        if opponent == "none":
            return ex, (pick * 5) >> 32, None, None
        x = (pick * 25) >> 32
        return ex, x // 5, None, x % 5
    u = words(step).astype(np.uint64)
    return u[:, 0], (u[:, 1] * 5) >> 32, u[:, 2], (u[:, 3] * 5) >> 32


def hdqn_fresh_draws(words, step, opponent):
    """The fresh-goal draws (explore, goal word) of mg_rollout_hdqn at global step `step` from stream
    B (counter gi ^ 2^63; csrc/mg_rollout_hdqn.h fresh_goal_words, ABI 20), restated: words(c) -> [n, 4]
    uint32 words of counter (gi ^ 2^63, c). Every opponent but "uniform": one call per two steps --
    call step div 2, words (x, y) on even steps, (z, w) on odd ones. "uniform": call `step`, (x, y),
    and z is the opponent's action word. Returns (explore, goal word, uniform-opponent word or None);
    `step` is taken mod 2^64 (a launch at step 0 draws its first goals at step 2^64 - 1)."""
    step %= 1 << 64
    if opponent == "uniform":
        u = words(step)
        return u[:, 0], u[:, 1], u[:, 2]
    u = words(step >> 1)
    return (u[:, 2], u[:, 3], None) if step & 1 else (u[:, 0], u[:, 1], None)


# --------------------------------------------------------------------------- replay memory oracle

def goal_status64(obs):
    """hdqn.py's goal_status (:223-236) of fp64 observation rows [N, 10] (dx1 = obs[:, 0],
    v2 = obs[:, 9]), evaluated in fp64 as the reference's Python floats are."""
    obs = np.asarray(obs, np.float64)
    dx1, v2 = obs[:, 0], obs[:, 9]
    return np.where(dx1 < -0.5 * v2, 0, np.where(dx1 < 0.5 * v2, 1, 2))


def stats_reduce_fixed(records):
    """mg_stats_reduce's totals (include/merging_hip.h, csrc/mg_stats_reduce.h stats_reduce_kernel) restated
    in numpy, operation for operation: records [n, 8] f64 (the 64-byte mg_episode_stats rows) ->
    (four f64 sums of ret[0], ret[1], ret_main, q_eval; six int64 counts). Blocks of 1,024 records; thread t
    of 256 adds records t, t + 256, t + 512, t + 768 of its block onto -0.0 in that order; the 256
    values fold in halves (v[t] + v[t + o], o = 128 ... 1); the block partials the same way, thread t
    adding partials t, t + 256, ... in order. Padding is -0.0, the exact additive identity. The
    logging loops this replaces (hdqn.py:330-346, main.py:221-228) keep running sums per episode;
    their order is not reproducible across a parallel batch, this one is."""
    rec = np.ascontiguousarray(records, np.float64).reshape(-1, 8)
    n = rec.shape[0]
    cnt = rec[:, 4:].copy().view(np.uint32)[:, :6].astype(np.int64).sum(0)

    def fold(v):  # [..., 256] -> [...]
        o = v.shape[-1] // 2
        while o >= 1:
            v = v[..., :o] + v[..., o:2 * o]
            o //= 2
        return v[..., 0]

    nb = (n + 1023) // 1024
    sums = []
    for k in (0, 1, 2, 7):
        col = np.full(max(nb, 1) * 1024, -0.0)
        col[:n] = rec[:, k]
        x = col.reshape(-1, 4, 256)
        acc = ((x[:, 0] + x[:, 1]) + x[:, 2]) + x[:, 3]  # (-0.0 + x0) = x0 exactly
        part = fold(acc)[:nb]
        m = max(1, (nb + 255) // 256)
        p = np.full(m * 256, -0.0)
        p[:nb] = part
        p = p.reshape(m, 256)
        a = np.full(256, -0.0)
        for row in p:
            a = a + row
        sums.append(float(fold(a)))
    return sums, [int(c) for c in cnt]


def oracle_envs_from(coracle, state, idx=None, params=None):
    """C-oracle envs holding a device batch's state (MergeVecEnv or its state_dict), for replaying
    it from mid-episode: positions, speeds, returns, step count, winner, the float clock the
    count stands for, and main.py's running ep_reward (r1_accumulate, or the ego's
    ret1_pending once winner == 1 -- what the device keeps, include/merging_hip.h)."""
    get = (lambda name: getattr(state, name)) if not isinstance(state, dict) else state.__getitem__
    sel = (lambda t: t) if idx is None else (lambda t: t[idx])
    host = lambda name: sel(get(name)).cpu().numpy()  # noqa: E731
    tf = host("tf").astype(np.int64) & 0xFFFF
    n = len(tf)
    envs = coracle.new_envs(n)
    for name, key in (("p1", "pos1"), ("v1", "vel1"), ("p2", "pos2"), ("v2", "vel2"), ("ret1", "r1_acc"),
                      ("ret2", "r2_acc")):
        envs[key] = host(name)
    envs["steps"] = tf & 0x1FFF
    envs["winner"] = (tf & 0x6000) >> 13
    envs["done"] = (tf & 0x8000) != 0
    envs["time_stamp"] = np.cumsum(np.full(8200, float((params or DEFAULT_PARAMS).dT)))[
        np.maximum(envs["steps"] - 1, 0)] * (envs["steps"] > 0)
    pending = None
    if isinstance(state, dict) and "episode_stats" in state:
        pending = sel(state["episode_stats"])[:, 3].cpu().numpy()
    elif not isinstance(state, dict) and getattr(state, "_ep_stats", None) is not None:
        pending = sel(state._ep_stats)[:, 3].cpu().numpy()
    envs["ep_reward_main"] = envs["r1_acc"] if pending is None else np.where(envs["winner"] == 1, pending,
                                                                              envs["r1_acc"])
    return envs


def step_with_won(coracle, envs, a1, a2=None, params=None):
    """One autoreset step of the C oracle that also reports env.winner == 1 after the step,
    read before the reset (the kernels' won bit; main.py:209). Returns obs (reset observation
    where done), rew, done, coll, final_obs (NaN rows where not done), won, err."""
    obs, rew, done, coll, _, _, err = coracle.step(envs, a1, a2, autoreset=False, params=params)
    won = envs["winner"] == 1
    d = done.astype(bool)
    fobs = np.full_like(obs, np.nan)
    fobs[d] = obs[d]
    if d.any():
        sub = envs[d]
        obs[d] = coracle.reset(sub, params)
        envs[d] = sub
    return obs, rew, done, coll, fobs, won, err


def replay_store(memory, counter, obs_first, obs, a1, rew, done=None, final_obs=None, won=None,
                 skip_ego_won=True, goal=None, next_goal=None, reward=None, meta_goal=None):
    """DQN.store_transition (scripts/main.py:115-119) applied to T steps of n envs in (t, i)
    order -- the order of stepping envs 0..n-1 each step and storing in turn -- with main.py:209's
    `if env.winner is not 1` filter. Row = np.hstack((s, [a, r], s')) with s the observation
    before the step, r the ego's reward, s' the terminal observation where done. Rows are
    float32 (the reference's float64 memory is read back through torch.FloatTensor, main.py:131-135).
    Vectorised; only the newest len(memory) transitions are written, as sequential stores leave
    them. Returns the new memory_counter.

    goal / next_goal [T, n]: hdqn.py's lower-level rows (HDQN.store_transition :180-184 on
    goal_state = [goal] + state, :291 and :304): [goal, s, a, r, next_goal, s'], 24 floats.
    reward [T, n] replaces the ego's env reward as r (hdqn.py:314's intrinsic reward).

    meta_goal [T, n]: Goal_DQN's memory instead (Goal_DQN.store_transition, hdqn.py:97-101, called
    at :325 once the inner loop broke, with state = next_state after :320 and goal the :303
    choice): rows [s', meta_goal, reward, s'] (22 floats) for the transitions whose `won` bit is
    clear -- here the mask marks the steps that did NOT end an inner loop -- and reward the
    extrinsic reward summed since that loop began (:286, :313)."""
    a1 = np.asarray(a1)
    T, n = a1.shape
    cap = memory.shape[0]
    obs = np.asarray(obs, np.float32).reshape(T, n, -1)
    prev = np.concatenate([np.asarray(obs_first, np.float32)[None], obs[:-1]], axis=0)
    nxt = obs.copy()
    if done is not None and final_obs is not None:
        d = np.asarray(done, bool).reshape(T, n)
        nxt[d] = np.asarray(final_obs, np.float32).reshape(T, n, -1)[d]
    keep = np.ones((T, n), bool)
    if (skip_ego_won or meta_goal is not None) and won is not None:
        keep = ~np.asarray(won, bool).reshape(T, n)
    r = (np.asarray(rew, np.float32).reshape(T, n, 2)[..., :1] if reward is None
         else np.asarray(reward, np.float32).reshape(T, n, 1))
    a = a1[..., None].astype(np.float32)
    if meta_goal is not None:  # Goal_DQN rows: [s', goal, extrinsic reward, s'] (:325)
        cols = [nxt, np.asarray(meta_goal, np.float32).reshape(T, n, 1), r, nxt]
    elif goal is None:
        cols = [prev, a, r, nxt]
    else:  # hdqn.py:180-184 on goal_state = [goal] + state (:291, :304)
        g = np.asarray(goal, np.float32).reshape(T, n, 1)
        g2 = np.asarray(next_goal, np.float32).reshape(T, n, 1)
        cols = [g, prev, a, r, g2, nxt]
    rows = np.concatenate(cols, axis=2)[keep]
    k = len(rows)
    last = rows[max(0, k - cap):]
    slots = (counter + np.arange(max(0, k - cap), k)) % cap
    memory[slots] = last
    return counter + k


def replay_sample_index(coracle, capacity, counter, seed, draw, batch, filled_only=False):
    """Slots of mg_replay_sample: floor(u0 * M / 2^32), u = Philox4x32-10(key seed, counter
    (b, draw)); M = capacity (np.random.choice(MEMORY_CAPACITY, BATCH_SIZE), main.py:130) or
    min(counter, capacity) (>= 1) when filled_only."""
    m = capacity if not filled_only else max(1, min(counter, capacity))
    u = coracle.philox_batch(batch, 0, seed, draw)
    return ((u[:, 0].astype(np.uint64) * np.uint64(m)) >> np.uint64(32)).astype(np.int64)
