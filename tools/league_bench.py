"""Time of a league evaluation -- the K x K cross-play payoff matrix -- on the device (not part of bench.py).

    python tools/league_bench.py [--out profiles/league_bench.json] [--window 0.3] [--repeats 3]
                                 [--parent-root DIR] [--processes 3]

For K in {2, 4, 8, 16, 32, 64} nets, n_pair in {64, 1,024} envs per pairing and T = 16 steps, the same matrix
two ways, both in one process and alternating inside every repeat so that drift of a shared machine hits both:
  league     DQNPopulation.cross_play on ONE MergeVecEnv of K^2 n_pair envs: clear_statistics, one
             rollout_qnet_league launch (no trajectory), league_summary = one mg_stats_reduce_many (two launches)
             and one host copy;
  existing   what the library offered before: the K^2 pairings as members of ceil(K^2 / 64) rollout_qnet_many calls
             with opponent lists, on as many env batches of up to 64 n_pair envs, then member_summaries on each
             (per member two launches, an allocation and a host copy).
Each way is timed whole ("total") and in its halves ("rollout": the launches that play; "summary": statistics to
host matrices), microseconds per evaluation. A window is as many evaluations as fill `window` seconds (sized from a
first timed one, at least two), between HIP events around the host loop that enqueues them and ends in a
synchronise, so host time a side cannot hide is in its figure. Each figure is the best of `repeats` windows after a
warm-up; the runs are kept, and spread = (max - min) / min of a side's own repeats. not_slower: league <= existing
* (1 + the larger of the two spreads). For K <= 8 the rollout half is one launch on both sides; rollout_within_spread
says whether the two agree within that spread.

  m1_check   rollout_qnet and rollout_qnet_many (one member) at 2^20 envs, opponent none and a net: what the
             kernels that existed before cost now. With --parent-root (a checkout of the parent commit with its
             library built) the same figures are taken from that tree too, in `processes` fresh processes per tree,
             the two trees alternating; within_spread: |result - parent| / parent <= the larger spread of the two
             trees' own runs. Without it the parent side is recorded as not measured.
The nets are torch's default initialisation and the envs start from reset: with autoreset the mix of states settles
within the warm-up.
"""

from __future__ import annotations

import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

NETS = [2, 4, 8, 16, 32, 64]
N_PAIR = [64, 1024]
T, MAX_MEMBERS = 16, 64
M1_ENVS = 1 << 20
M1_FIGURES = ("rollout_qnet_none_us", "rollout_qnet_net_us", "rollout_qnet_many_none_us", "rollout_qnet_many_net_us")


def spread(runs):
    return (max(runs) - min(runs)) / min(runs)


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def windows(torch, sides, window_s, repeats, warmup=2):
    """Per side (a callable running one evaluation): microseconds per evaluation in each of `repeats` windows of
    at least window_s seconds, the sides alternating inside every repeat."""
    iters = []
    for fn in sides:
        for _ in range(warmup):
            fn()
        one = max(timed(torch, fn), 1.0)
        iters.append(max(2, int(window_s * 1e6 / one) + 1))
    runs = [[] for _ in sides]
    for _ in range(repeats):
        for k, fn in enumerate(sides):
            runs[k].append(timed(torch, lambda: [fn() for _ in range(iters[k])]) / iters[k])
    return runs, iters


def make_qnets(torch, count, dev):
    """`count` reference Nets (main.py:30-47: 10 -> 200 -> 100 -> 5) of torch's default initialisation, packed."""
    from merging_gym.policy import QNet

    torch.manual_seed(0)
    qnets = []
    for _ in range(count):
        layers = {"fc1": torch.nn.Linear(10, 200), "fc2": torch.nn.Linear(200, 100), "out": torch.nn.Linear(100, 5)}
        sd = {f"{name}.{p}": getattr(layer, p).detach() for name, layer in layers.items() for p in ("weight", "bias")}
        qnets.append(QNet.from_state_dict(sd, device=dev))
    return qnets


def m1_worker(root, window, repeats):
    """One process on the tree at `root`: the four M = 1 figures, printed as one JSON line."""
    sys.path.insert(0, os.path.join(root, "merging-gym_amd"))
    import torch

    from merging_gym import MergeVecEnv, _native

    dev = torch.device("cuda", 0)
    qnets = make_qnets(torch, 2, dev)
    env = MergeVecEnv(M1_ENVS, device=dev)
    sides = (lambda: env.rollout_qnet(T, qnets[0], 0, opponent="none"),
             lambda: env.rollout_qnet(T, qnets[0], 0, opponent=qnets[1]),
             lambda: env.rollout_qnet_many(T, qnets[:1], 0, opponent="none"),
             lambda: env.rollout_qnet_many(T, qnets[:1], 0, opponent=[qnets[1]]))
    runs, iters = windows(torch, sides, window, repeats, warmup=3)
    print(json.dumps({"m1": {name: r for name, r in zip(M1_FIGURES, runs)}, "iterations": iters,
                      "build": _native.build_info()}), flush=True)


def m1_check(args):
    """The M = 1 figures of this tree and, with --parent-root, of the parent's, from alternating fresh processes."""
    trees = {"result": ROOT}
    if args.parent_root:
        trees["parent"] = os.path.abspath(args.parent_root)
    runs = {name: {f: [] for f in M1_FIGURES} for name in trees}
    builds = {}
    for _ in range(args.processes):
        for name, root in trees.items():
            out = subprocess.run([sys.executable, os.path.abspath(__file__), "--m1-worker", root, "--window",
                                  str(args.window), "--repeats", str(args.repeats)], capture_output=True, text=True,
                                 timeout=600)
            if out.returncode != 0:
                sys.exit(f"m1 worker on {name} failed:\n{out.stderr[-2000:]}")
            line = json.loads([ln for ln in out.stdout.splitlines() if ln.startswith('{"m1"')][-1])
            builds[name] = line["build"]
            for f in M1_FIGURES:
                runs[name][f] += line["m1"][f]
    check = {"n": M1_ENVS, "T": T, "processes": args.processes, "builds": builds, "figures": {}}
    for f in M1_FIGURES:
        entry = {"result_us": min(runs["result"][f]), "result_us_runs": runs["result"][f],
                 "result_spread": spread(runs["result"][f])}
        if "parent" in trees:
            tol = max(entry["result_spread"], spread(runs["parent"][f]))
            entry.update(parent_us=min(runs["parent"][f]), parent_us_runs=runs["parent"][f],
                         parent_spread=spread(runs["parent"][f]))
            entry["result_minus_parent_relative"] = (entry["result_us"] - entry["parent_us"]) / entry["parent_us"]
            entry["within_spread"] = abs(entry["result_minus_parent_relative"]) <= tol
        else:
            entry["parent_us"] = "not measured"
        check["figures"][f] = entry
    if "parent" in trees:
        check["within_spread_at_every_figure"] = all(e["within_spread"] for e in check["figures"].values())
    return check


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "league_bench.json"))
    ap.add_argument("--window", type=float, default=0.3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--parent-root", default=None)
    ap.add_argument("--processes", type=int, default=3)
    ap.add_argument("--m1-worker", default=None, metavar="ROOT")
    args = ap.parse_args()
    if args.m1_worker:
        return m1_worker(args.m1_worker, args.window, args.repeats)

    sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))
    import torch

    from merging_gym import DQNPopulation, MergeVecEnv, ReplayRing, _native

    if not torch.cuda.is_available():
        sys.exit("league_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    qnets = make_qnets(torch, max(NETS), dev)
    ring = ReplayRing(64, device=dev)  # cross_play touches no ring: one shared by every member will do
    result = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "T": T,
              "window_s": args.window, "repeats": args.repeats, "points": []}
    names = ("league_total", "existing_total", "league_rollout", "existing_rollout", "league_summary",
             "existing_summary")
    for K in NETS:
        pop = DQNPopulation(qnets[:K], [ring] * K, seed=range(K))
        nets = pop.qnets
        pairs = K * K
        for n in N_PAIR:
            env = MergeVecEnv(pairs * n, device=dev)
            # the existing path: the pairings in order, up to 64 to a batch, batch b at the league's env indices
            chunks = [list(range(lo, min(lo + MAX_MEMBERS, pairs))) for lo in range(0, pairs, MAX_MEMBERS)]
            envs = [MergeVecEnv(len(c) * n, device=dev, env_offset=c[0] * n) for c in chunks]
            egos = [[nets[p // K] for p in c] for c in chunks]
            opps = [[nets[p % K] for p in c] for c in chunks]
            seeds = [[p // K for p in c] for c in chunks]

            def league_rollout():
                env.rollout_qnet_league(T, nets, pop.seed, trajectory=False)

            def existing_rollout():
                for e, ego, opp, sd in zip(envs, egos, opps, seeds):
                    e.rollout_qnet_many(T, ego, sd, opponent=opp)

            def existing_summary():
                return [s for e, c in zip(envs, chunks) for s in e.member_summaries(len(c))]

            def existing_total():
                for e in envs:
                    e.clear_statistics()
                existing_rollout()
                return existing_summary()

            sides = (lambda: pop.cross_play(env, T), existing_total, league_rollout, existing_rollout,
                     lambda: env.league_summary(K), existing_summary)
            runs, iters = windows(torch, sides, args.window, args.repeats)
            point = {"nets": K, "n_pair": n, "pairings": pairs, "envs": pairs * n, "existing_batches": len(chunks),
                     "iterations": dict(zip(names, iters))}
            for name, r in zip(names, runs):
                point[name + "_us"] = min(r)
                point[name + "_us_runs"] = r
                point[name + "_spread"] = spread(r)
            for half in ("total", "rollout", "summary"):
                a, b = point[f"league_{half}_us"], point[f"existing_{half}_us"]
                tol = max(point[f"league_{half}_spread"], point[f"existing_{half}_spread"])
                point[f"{half}_speedup"] = b / a
                point[f"{half}_not_slower"] = a <= b * (1.0 + tol)
            if len(chunks) == 1:  # one launch on both sides
                tol = max(point["league_rollout_spread"], point["existing_rollout_spread"])
                point["rollout_within_spread"] = (abs(point["league_rollout_us"] - point["existing_rollout_us"])
                                                  <= tol * point["existing_rollout_us"])
            point["not_slower"] = point["total_not_slower"]
            result["points"].append(point)
            print(json.dumps(point), flush=True)
            del env, envs
            torch.cuda.empty_cache()
        del pop
    result["not_slower_at_every_point"] = all(p["not_slower"] for p in result["points"])
    result["m1_check"] = m1_check(args)
    print(json.dumps({"m1_check": result["m1_check"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({"not_slower_at_every_point": result["not_slower_at_every_point"]}))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
