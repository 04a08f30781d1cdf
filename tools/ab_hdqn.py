"""In-process A/B of libmerging_hip.so variants on the fused h-DQN acting loop (mg_rollout_hdqn,
scripts/hdqn.py:280-323), through the package's own API: every variant library is bound like the
in-tree one (_native._load) and swapped in as _native.lib between timed windows, so the env batch,
the nets (packed once per variant: they share the ABI) and the stream are the same for all of them.

    python tools/ab_hdqn.py tools/variants/lib_*.so [--envs N] [--rounds R] [--launches L] [--equal]

Prints the median kernel time per 16-step launch (HIP events on the launch stream) per variant and
leg: h-DQN L0, the uniform opponent, self-play, another checkpoint's nets (read from L2), L0 with
the fused goal ring, L0 with Goal_DQN's columns (goal_memory).

--equal: before any timing, every library runs the same launches from the same
env.load_state_dict state -- n = 1000 and n = 577, T = 16, each of the four opponents, ring and
goal_memory on, a first launch (fresh goals) and the one that continues it (carried goals and sums,
a ring counter off zero) -- and every returned tensor, the env state_dict, the ring's memory and
counter and the episode statistics must equal the first library's bit for bit: exit status 1 at
the first difference, naming the tensor. (final_observation is compared on the rows that ended;
the kernel writes no others.)
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from merging_gym import MergeVecEnv, ReplayRing, _native  # noqa: E402
from merging_gym.policy import NUM_GOALS, QNet  # noqa: E402

LEGS = ("hdqn_L0", "hdqn_uniform", "hdqn_self", "hdqn_other", "hdqn_ring", "hdqn_goal_memory")


def equal_outputs(libs, nets, T=16):
    """Run the --equal launches under every library; the first (library, tensor name) that differs from
    the first library's, or None."""
    for n in (1000, 577):
        env = MergeVecEnv(n, device="cuda", final_observation=True)
        for k in range(190):  # mid-episode: goals are reached and episodes end inside the launches
            env.step_random(5, opponent_random=False, step_idx=k)
        start = env.state_dict()
        for opp in ("hdqn_L0", "hdqn_uniform", "hdqn_self", "hdqn_other"):
            ref = None
            for name, lib in libs.items():
                _native.lib = lib
                meta, lower, opps = nets[name]
                env.load_state_dict(start)
                ring = ReplayRing(n * T // 3 + 7, device="cuda", goal=True)  # wraps inside a launch
                got = {}
                for launch in range(2):
                    tr = env.rollout_hdqn(T, meta, lower, 9, opponent=opps[opp], first_step=190 + launch * T,
                                          ring=ring, goal_memory=True)
                    for k, v in tr.items():
                        if v is not None:
                            got[f"launch {launch} {k}"] = (v[tr["done"]] if k == "final_observation" else v).clone()
                got.update({f"state_dict {k}": v.clone() for k, v in env.state_dict().items() if hasattr(v, "clone")})
                got.update({"ring memory": ring.memory.clone(), "ring counter": ring._counter.clone(),
                            "returns": env.returns.clone(), "counts": env.counts.clone(), "q_eval": env.q_eval.clone()})
                if ref is None:
                    ref = got
                    continue
                if got.keys() != ref.keys():
                    return name, f"{opp} n={n}: tensors {sorted(got.keys() ^ ref.keys())}"
                for k, v in got.items():
                    if v.shape != ref[k].shape or not np.array_equal(v.cpu().numpy().view(np.uint8),
                                                                     ref[k].cpu().numpy().view(np.uint8)):
                        return name, f"{opp} n={n}: {k}"
    return None


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("libs", nargs="+")
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--launches", type=int, default=8)
    ap.add_argument("--T", type=int, default=16)
    ap.add_argument("--equal", action="store_true", help="first check the libraries' outputs are bit-equal")
    a = ap.parse_args()
    libs = {os.path.basename(p): _native._load(p) for p in a.libs}
    rng = None

    def net(i, o):  # bench.py's hdqn_leg nets: torch.nn.Linear's signed default initialisation
        nonlocal rng
        sd = {}
        for name, (r, c) in zip(("fc1", "fc2", "out"), [(200, i), (100, 200), (o, 100)]):
            sd[f"{name}.weight"] = rng.uniform(-c ** -0.5, c ** -0.5, (r, c)).astype(np.float32)
            sd[f"{name}.bias"] = rng.uniform(-c ** -0.5, c ** -0.5, r).astype(np.float32)
        return QNet.from_state_dict(sd, device="cuda")

    # every variant packs its own copies of the same nets (the packed layout may differ between them)
    nets = {}
    for name, lib in libs.items():
        _native.lib = lib
        rng = np.random.default_rng(0)
        meta, lower, meta_op, lower_op = net(10, NUM_GOALS), net(11, 5), net(10, NUM_GOALS), net(11, 5)
        nets[name] = (meta, lower, {"hdqn_L0": "none", "hdqn_uniform": "uniform", "hdqn_self": "self",
                                    "hdqn_other": (meta_op, lower_op)})
    if a.equal:
        diff = equal_outputs(libs, nets)
        if diff is not None:
            print(f"NOT EQUAL: {diff[0]} differs from {next(iter(libs))} in {diff[1]}", flush=True)
            sys.exit(1)
        print(f"equal: {' '.join(libs)} agree bit for bit", flush=True)
    env = MergeVecEnv(a.envs, device="cuda", final_observation=False)
    ring = ReplayRing(1 << 24, device="cuda", goal=True)  # bench.py's hdqn_leg ring
    k = 1_000_000
    for _ in range(200):
        env.rollout_random(a.T, 7, first_step=k)
        k += a.T
    res = {name: {leg: [] for leg in LEGS} for name in libs}
    ev = [(torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)) for _ in range(a.launches)]
    for r in range(a.rounds + 1):  # round 0 warms every variant up and is not kept
        for name in (list(libs) if r % 2 == 0 else list(reversed(libs))):
            _native.lib = libs[name]
            meta, lower, opps = nets[name]
            for leg in LEGS:
                kw = dict(opponent=opps.get(leg, "none"), ring=ring if leg == "hdqn_ring" else None,
                          goal_memory=leg == "hdqn_goal_memory")
                for j in range(a.launches):
                    ev[j][0].record()
                    env.rollout_hdqn(a.T, meta, lower, 11, first_step=k, final_observation=False, **kw)
                    ev[j][1].record()
                    k += a.T
                torch.cuda.synchronize()
                if r:
                    res[name][leg] += [e0.elapsed_time(e1) for e0, e1 in ev]
    for name, d in res.items():
        print(f"{name:22s} " + "   ".join(f"{leg} {statistics.median(v):6.3f} ms" for leg, v in d.items()), flush=True)


if __name__ == "__main__":
    main()
