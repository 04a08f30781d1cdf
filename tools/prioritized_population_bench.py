"""Time of one update of a population of prioritized Rainbow learners on the device (not part of bench.py).

    python tools/prioritized_population_bench.py [--out profiles/prioritized_population_bench.json] [--updates 200]

tools/rainbow_population_bench.py's legs, alternation, repeats and spread, on prioritized agents. For
RainbowDQN(10, 5) at batch 32 and 128 and M in {1, 2, 4, 8, 16, 32, 64} members, in one process on one GPU, each
member on its own full 10,000-row PrioritizedRainbowReplay (alpha 0.6; a tree that 64 rounds of update_priorities
have shaped, as tools/rainbow_learn_bench.py shapes its one) with its own seed, beta 0.4, the noise drawn on the
device:
  population_us   microseconds per update of all M members through PrioritizedRainbowPopulation.learn(updates): HIP
                  events around one call that enqueues all of them (the noise launch and the pack included), after
                  `warmup` untimed updates;
  lone_in_turn_us the same M agents as M PrioritizedRainbowLearner(DeviceNoise)s on the same replays, learn(updates)
                  called on each in turn inside one pair of events: the only way to train M prioritized agents
                  without the population;
  lone_us         one lone PrioritizedRainbowLearner(DeviceNoise), timed the same way;
each the best of `repeats`, the three legs alternating inside every repeat so that drift of a shared machine hits all
of them; the runs are kept beside the minima, and spread = (max - min) / min of a leg's own repeats.
  bend            the smallest M whose population_us exceeds 1.5 x the population's at M = 1.
  not_slower_than_lone_in_turn  population_us <= lone_in_turn_us at every measured point; `slower_points` lists the
                  others with the margin = the larger spread of the two legs.
  collect         one iteration of the acting half at 1,024 envs per member and 16 steps: collect_us through
                  PrioritizedRainbowPopulation.collect (observe, one rollout, the member store with the trees'
                  launches), collect_lone_in_turn_us the lone loop's observe, rollout_rainbow and store_rollout for
                  each member in turn on an env of its own.
The replays hold seeded random rows and the nets torch's default initialisation: the time of an update does not
depend on the values.
"""

from __future__ import annotations

import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from rainbow_learn_bench import fill, timed, torch_rainbow  # noqa: E402
from rainbow_population_bench import BATCHES, MEMBERS, spread  # noqa: E402

CAPACITY, ALPHA, BETA = 10000, 0.6, 0.4
COLLECT_ENVS, COLLECT_STEPS = 1024, 16


def shaped_replay(torch, dev, seed):
    """A full PrioritizedRainbowReplay of random rows under a tree that 64 rounds of updates have shaped."""
    from merging_gym import PrioritizedRainbowReplay

    per = PrioritizedRainbowReplay(CAPACITY, ALPHA, device=dev)
    per.store(torch.rand((CAPACITY, 10), device=dev), torch.rand((1, CAPACITY, 10), device=dev),
              torch.zeros((1, CAPACITY), dtype=torch.int8, device=dev), torch.rand((1, CAPACITY, 2), device=dev))
    fill(torch, per, dev)
    for r in range(64):
        idx, _ = per.sample_indices(1024, BETA, seed=seed, draw=r)
        per.update_priorities(idx, torch.rand(1024, device=dev) * 4.0 + 1e-3)
    return per


def collect_cost(torch, dev, nets, members, repeats):
    """One collect iteration of `members` agents, population against the lone loops in turn, alternating."""
    from merging_gym import (DeviceNoise, MergeVecEnv, PrioritizedRainbowLearner, PrioritizedRainbowPopulation,
                             PrioritizedRainbowReplay)

    new = lambda: PrioritizedRainbowReplay(1 << 20, ALPHA, device=dev)  # noqa: E731
    replays = [new() for _ in range(members)]
    pop = PrioritizedRainbowPopulation(nets[:members], replays, seed=range(members))
    env = MergeVecEnv(members * COLLECT_ENVS, device=dev)
    lone = [PrioritizedRainbowLearner(nets[m], new(), seed=m, generator=DeviceNoise()) for m in range(members)]
    envs = [MergeVecEnv(COLLECT_ENVS, device=dev) for _ in range(members)]

    def in_turn():
        for learner, e in zip(lone, envs):
            obs0 = e.observe().clone()  # the lone loop as rainbow_learn.py documents it
            learner.replay.store_rollout(obs0, e.rollout_rainbow(COLLECT_STEPS, learner.net))

    p_us, t_us = [], []
    for rep in range(repeats + 1):  # the first pass warms up
        p, t = timed(torch, lambda: pop.collect(env, COLLECT_STEPS)), timed(torch, in_turn)
        if rep:
            p_us.append(p), t_us.append(t)
    return {"members": members, "envs_per_member": COLLECT_ENVS, "num_steps": COLLECT_STEPS, "capacity": 1 << 20,
            "collect_us": min(p_us), "collect_us_runs": p_us, "collect_spread": spread(p_us),
            "collect_lone_in_turn_us": min(t_us), "collect_lone_in_turn_us_runs": t_us,
            "collect_lone_in_turn_spread": spread(t_us), "speedup_vs_lone_in_turn": min(t_us) / min(p_us)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "prioritized_population_bench.json"))
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--collect-members", type=int, default=8)
    args = ap.parse_args()

    import torch

    from merging_gym import DeviceNoise, PrioritizedRainbowLearner, PrioritizedRainbowPopulation, _native

    if not torch.cuda.is_available():
        sys.exit("prioritized_population_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "updates": args.updates,
              "warmup": args.warmup, "repeats": args.repeats, "capacity": CAPACITY, "alpha": ALPHA, "beta": BETA,
              "batches": {}}
    torch.manual_seed(0)
    replays = [shaped_replay(torch, dev, seed=2 + m) for m in range(max(MEMBERS))]
    single_replay = shaped_replay(torch, dev, seed=1)
    nets = []
    for _ in range(max(MEMBERS)):
        net, _ = torch_rainbow(torch, dev)
        nets.append({k: v.detach() for k, v in net.state_dict().items()})
    for batch in BATCHES:
        by_m = {}
        for M in MEMBERS:
            pop = PrioritizedRainbowPopulation(nets[:M], replays[:M], batch_size=batch, seed=range(M), beta=BETA)
            lone = [PrioritizedRainbowLearner(nets[m], replays[m], batch_size=batch, seed=m, generator=DeviceNoise(),
                                              beta=BETA) for m in range(M)]
            single = PrioritizedRainbowLearner(nets[0], single_replay, batch_size=batch, seed=0, generator=DeviceNoise(),
                                               beta=BETA)
            pop.learn(args.warmup)
            single.learn(args.warmup)
            for learner in lone:
                learner.learn(args.warmup)
            p_us, t_us, s_us = [], [], []
            for _ in range(args.repeats):
                p_us.append(timed(torch, lambda: pop.learn(args.updates)) / args.updates)
                t_us.append(timed(torch, lambda: [learner.learn(args.updates) for learner in lone]) / args.updates)
                s_us.append(timed(torch, lambda: single.learn(args.updates)) / args.updates)
            entry = {"population_us": min(p_us), "population_us_runs": p_us, "population_spread": spread(p_us),
                     "lone_in_turn_us": min(t_us), "lone_in_turn_us_runs": t_us, "lone_in_turn_spread": spread(t_us),
                     "lone_us": min(s_us), "lone_us_runs": s_us, "lone_spread": spread(s_us),
                     "speedup_vs_lone_in_turn": min(t_us) / min(p_us), "population_us_per_member": min(p_us) / M}
            by_m[str(M)] = entry
            print(json.dumps({f"b{batch} M={M}": entry}), flush=True)
            del pop, lone, single
        base = by_m["1"]["population_us"]
        slower = {m: {"population_minus_lone_in_turn_relative": e["population_us"] / e["lone_in_turn_us"] - 1.0,
                      "margin": max(e["population_spread"], e["lone_in_turn_spread"])}
                  for m, e in by_m.items() if e["population_us"] > e["lone_in_turn_us"]}
        result["batches"][f"b{batch}"] = {
            "members": by_m,
            "bend": next((M for M in MEMBERS if by_m[str(M)]["population_us"] > 1.5 * base), None),
            "not_slower_than_lone_in_turn": not slower, "slower_points": slower,
            "m1_population_minus_lone_relative": (base - by_m["1"]["lone_us"]) / by_m["1"]["lone_us"]}
    result["collect"] = collect_cost(torch, dev, nets, args.collect_members, args.repeats)
    print(json.dumps({"collect": result["collect"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({b: {k: v for k, v in r.items() if k != "members"} for b, r in result["batches"].items()}))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
