"""Golden vectors of the reference's own MergeEnv at non-default constants (tests/params_cases.py A-D).

A sibling of gen_golden.py (same stand-ins for the absent third-party packages, same Recorder): the
reference is imported read-only at run time, its module globals (merging_env.py:22-46) are set to a
case's values BEFORE MergeEnv is constructed (the vehicle surfaces take VEHICLE_W / VEHICLE_H in
__init__, :97-98), and env.action_dict (:101) is replaced. Only what the runs produce is committed
(tests/golden/reference_params_golden.npz).

Per case, traces of the same kinds as the default file's: constant-action episodes that collide, that
arrive in both orders and that time out, plus random play with and without an opponent. A timeout
trace does not step through thousands of uneventful steps: after reset() its clock is set to the
value `<trace>_k0` sequential additions of dT give (the recorded row `time` shows it), and the episode
runs from there.

Case E of params_cases.py (start_vel, vel_ref, the time limit) is NOT here: those three numbers are
literals in the reference's source (:216-217, :158-159, :142), so the reference cannot run it. For
these fields the oracle is a restatement with the literal replaced, and nothing more.

Usage:  python tests/golden/gen_params_golden.py
"""

from __future__ import annotations

import contextlib
import io
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
OUT = os.path.join(HERE, "reference_params_golden.npz")

GLOBALS = ("R", "H", "W", "dT", "RFirst", "RSecond", "RCollision", "vel_penalty", "time_penalty",
           "START_POINT", "END_POINT", "VEHICLE_W", "VEHICLE_H", "prediction_t")

# constant-action episodes: (a1, a2 or None) as ranks of the case's action speeds, slowest = 0
KATS = {"same": (3, 3), "ego": (4, None), "opp": (2, 4), "slow": (2, 2)}
TIMEOUTS = {"toL0": (0, None), "toOpp": (0, 4)}
TAIL = 250  # steps a timeout trace runs before the limit


def make_env(gen, case):
    import gym  # the stand-in gen_golden wrote

    mod = sys.modules["merging_gym.envs.merging_env"]
    for name in GLOBALS:
        setattr(mod, name, getattr(case, name))
    with contextlib.redirect_stdout(io.StringIO()):
        env = gym.make("merging_env-v0").unwrapped
    env.action_dict = dict(enumerate(case.action_speeds))
    return env


def main():
    sys.path[:0] = [HERE, os.path.join(ROOT, "tests"), os.path.join(ROOT, "oracle")]
    import gen_golden as gen
    import params_cases as pc

    gen.load_reference_env()
    out = {}
    rng = np.random.default_rng(20260101)
    for name in pc.REFERENCE_CASES:
        case = pc.CASES[name]
        env = make_env(gen, case)
        seen = {"coll": 0, "w1": 0, "w2": 0, "timeout": 0}

        def keep(tag, rec, k0=0):
            d = rec.arrays(f"{name}_{tag}")
            done = d[f"{name}_{tag}_done"]
            stop = int(np.argmax(done)) + 1 if done.any() and not d[f"{name}_{tag}_reset"][1:].any() else len(done)
            out.update({k: v[:stop] for k, v in d.items()})
            out[f"{name}_{tag}_k0"] = np.asarray(k0, np.int32)
            fin = np.flatnonzero(done[:stop])
            for i in fin:
                coll = d[f"{name}_{tag}_coll"][i]
                seen["coll"] += int(coll)
                if not coll and d[f"{name}_{tag}_time"][i] > 500:
                    seen["timeout"] += 1
                elif not coll:
                    seen["w1" if d[f"{name}_{tag}_winner"][i] == 1 else "w2"] += 1

        rank = [int(a) for a in np.argsort(case.action_speeds)]
        act = lambda r: None if r is None else rank[r]  # noqa: E731

        for tag, (a1, a2) in KATS.items():
            a1, a2 = act(a1), act(a2)
            rec = gen.Recorder()
            gen.run_trace(env, [a1] * 700, [a2] * 700, reset_on_done=False, max_steps=700, rec=rec)
            keep(tag, rec)
        tmo = pc.timeout_steps(case.dT)
        ts = case.clock(np.arange(tmo + 1))
        for tag, (a1, a2) in TIMEOUTS.items():
            a1, a2 = act(a1), act(a2)
            rec = gen.Recorder()
            k0 = tmo - TAIL
            with contextlib.redirect_stdout(io.StringIO()):
                obs = env.reset()
            env.time_stamp = float(ts[k0])
            rec.add(env, -1, -1, obs, [0.0, 0.0], False, None, True)
            for _ in range(TAIL + 5):
                with contextlib.redirect_stdout(io.StringIO()):
                    obs, rew, done, info = env.step(a1, a2)
                rec.add(env, a1, a2, obs, rew, done, info, False)
            keep(tag, rec, k0)
        for tag, opp_random in (("rndL0", False), ("rndRR", True)):
            rec = gen.Recorder()
            steps = 300
            a1 = rng.integers(0, 5, steps)
            a2 = rng.integers(0, 5, steps) if opp_random else np.full(steps, -1)
            gen.run_trace(env, list(a1), [int(x) for x in a2], reset_on_done=True, max_steps=steps, rec=rec)
            keep(tag, rec)
        print(name, seen)
        assert all(seen.values()), (name, seen)  # collision, both arrival orders and a timeout occur
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT} ({os.path.getsize(OUT) / 1e6:.2f} MB, {len(out)} arrays)")


if __name__ == "__main__":
    main()
