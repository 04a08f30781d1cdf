"""Time of the acting half of a Rainbow population's loop on the device (not part of bench.py).

    python tools/rainbow_population_act_bench.py [--out profiles/rainbow_population_act_bench.json]
                                                 [--window 0.3] [--repeats 3] [--vs]

The method is tools/population_act_bench.py's. One iteration is observe + a rollout at T = 16 + the store into
replays of 10,000 rows, for M members of n_member envs:
  many_us   microseconds per iteration through ONE MergeVecEnv of M * n_member envs: observe(),
            rollout_rainbow_many, rainbow_learn.store_rainbow_rollout_many -- four launches for all members;
  lone_us   the same M members as M separate MergeVecEnvs, each in turn observe(), rollout_rainbow,
            RainbowReplay.store_rollout -- 4 M launches, the only way to do it without the member entry points;
for M in {2, 8, 64}, n_member in {1,024, 16,384} and the opponents "none" and "self". Both sides run in one process,
alternating inside every repeat so that drift of a shared machine hits both, after a warm-up; a window is as many
iterations as fill `window` seconds (sized from a first timed iteration), between HIP events around the host loop
that enqueues them, so host time a side cannot hide is in its figure. Each figure is the best of `repeats`; the runs
are kept, and spread = (max - min) / min of a side's own repeats. not_slower: many_us <= lone_us * (1 + the larger
of the two spreads).
  member_indexing   M = 1 at N = 2^20 beside the lone kernel on the same env (rollout only, and rollout + store):
                    what the member indexing itself costs.
  --vs              the "vs another net" leg alone, merged into the --out file as "vs_points" (every other key
                    stays): member m against the net of member (m + 1) % M -- rollout_rainbow_many(T, nets,
                    opponent=[...]) beside M lone rollout_rainbow(T, nets[m], opponent=nets[(m + 1) % M]) + store in
                    turn -- for M in {2, 8, 64} at 1,024 envs per member.
The nets are the reference's initialisation with drawn noise and the envs start from reset: with autoreset the mix
of states settles within the warm-up, and both sides see the same states (the member launch equals the lone ones
bit for bit).
"""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from population_act_bench import spread, windows  # noqa: E402
from rainbow_learn_bench import torch_rainbow  # noqa: E402

MEMBERS = [2, 8, 64]
N_MEMBER = [1024, 16384]
T, CAP = 16, 10000


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rainbow_population_act_bench.json"))
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--vs", action="store_true", help="only the cross-play leg, merged into --out as vs_points")
    args = ap.parse_args()

    import torch

    from merging_gym import MergeVecEnv, RainbowNet, RainbowReplay, _native
    from merging_gym.rainbow_learn import store_rainbow_rollout_many

    if not torch.cuda.is_available():
        sys.exit("rainbow_population_act_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    torch.manual_seed(0)
    all_nets = []
    for _ in range(max(MEMBERS)):
        current, _ = torch_rainbow(torch, "cpu")
        all_nets.append(RainbowNet.from_state_dict({k: v.detach() for k, v in current.state_dict().items()},
                                                   device=dev))
        all_nets[-1].packed  # packed now, outside every window
    setup = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "T": T, "capacity": CAP,
             "window_s": args.window, "repeats": args.repeats}
    result = dict(setup, points=[])
    points = result["points"]
    if args.vs:
        with open(args.out) as f:
            result = json.load(f)
        result["vs_setup"] = setup
        points = result["vs_points"] = []
    for M in MEMBERS:
        for n in N_MEMBER[:1] if args.vs else N_MEMBER:
            env = MergeVecEnv(M * n, device=dev)
            envs = [MergeVecEnv(n, device=dev) for _ in range(M)]
            replays = [RainbowReplay(CAP, device=dev) for _ in range(M)]
            lone_replays = [RainbowReplay(CAP, device=dev) for _ in range(M)]
            nets = all_nets[:M]
            against = [nets[(m + 1) % M] for m in range(M)]
            for opponent in ("next_member",) if args.vs else ("none", "self"):

                def many():
                    obs0 = env.observe()
                    opp = against if args.vs else opponent
                    store_rainbow_rollout_many(replays, obs0, env.rollout_rainbow_many(T, nets, opp))

                def lone():
                    for m in range(M):
                        obs0 = envs[m].observe()
                        opp = against[m] if args.vs else opponent
                        lone_replays[m].store_rollout(obs0, envs[m].rollout_rainbow(T, nets[m], opp))

                (many_us, lone_us), iters = windows(torch, (many, lone), args.window, args.repeats)
                tol = max(spread(many_us), spread(lone_us))
                point = {"members": M, "n_member": n, "opponent": opponent, "many_us": min(many_us),
                         "many_us_runs": many_us, "many_spread": spread(many_us), "lone_us": min(lone_us),
                         "lone_us_runs": lone_us, "lone_spread": spread(lone_us), "iterations": iters,
                         "speedup": min(lone_us) / min(many_us),
                         "many_env_steps_per_s": M * n * T / (min(many_us) * 1e-6),
                         "not_slower": min(many_us) <= min(lone_us) * (1.0 + tol)}
                points.append(point)
                print(json.dumps(point), flush=True)
            del env, envs, replays, lone_replays
            torch.cuda.empty_cache()
    if args.vs:
        result["vs_not_slower_at_every_point"] = all(p["not_slower"] for p in points)
        with open(args.out, "w") as f:
            json.dump(result, f, indent=1, sort_keys=True)
            f.write("\n")
        print(f"merged vs_points into {args.out}")
        return
    # what the member indexing itself costs: one member on 2^20 envs beside the lone kernel, the same env
    env = MergeVecEnv(1 << 20, device=dev)
    replay = RainbowReplay(CAP, device=dev)
    indexing = {}
    for opponent in ("none", "self"):
        sides = (lambda: env.rollout_rainbow_many(T, all_nets[:1], opponent),
                 lambda: env.rollout_rainbow(T, all_nets[0], opponent),
                 lambda: store_rainbow_rollout_many([replay], env.observe(),
                                                    env.rollout_rainbow_many(T, all_nets[:1], opponent)),
                 lambda: replay.store_rollout(env.observe(), env.rollout_rainbow(T, all_nets[0], opponent)))
        runs, iters = windows(torch, sides, args.window, args.repeats)
        names = ("rollout_many_us", "rollout_lone_us", "rollout_store_many_us", "rollout_store_lone_us")
        entry = {"iterations": iters}
        for name, r in zip(names, runs):
            entry[name] = min(r)
            entry[name + "_runs"] = r
            entry[name.replace("_us", "_spread")] = spread(r)
        entry["rollout_many_minus_lone_relative"] = (
            (entry["rollout_many_us"] - entry["rollout_lone_us"]) / entry["rollout_lone_us"])
        entry["rollout_store_many_minus_lone_relative"] = (
            (entry["rollout_store_many_us"] - entry["rollout_store_lone_us"]) / entry["rollout_store_lone_us"])
        indexing[opponent] = entry
        print(json.dumps({"member_indexing": {opponent: entry}}), flush=True)
    result["member_indexing"] = {"n": 1 << 20, **indexing}
    result["not_slower_at_every_point"] = all(p["not_slower"] for p in result["points"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"not_slower_at_every_point": result["not_slower_at_every_point"]}))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
