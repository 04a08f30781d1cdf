"""Time of one update of a population of DQN learners on the device (not part of bench.py).

    python tools/learn_population_bench.py [--out profiles/learn_population_bench.json] [--updates 200] [--warmup 20]

For the 10 -> 5 net at batch 128 and M in {1, 2, 4, 8, 16, 32, 64} members, in one process on one GPU, each
member on its own 2,000-row ring with its own seed:
  population_us   microseconds per update of all M members through DQNPopulation.learn(updates): HIP events
                  around one call that enqueues all of them, after `warmup` untimed updates;
  lone_in_turn_us the same M agents as M DQNLearners, learn(updates) called on each in turn inside one pair of
                  events: the only way to train M agents without the population (one call per learner is the
                  cheapest form of it: no host work per update);
  lone_us         one lone DQNLearner, timed the same way;
each the best of `repeats`, the three legs alternating inside every repeat so that drift of a shared machine
hits all of them; the runs are kept beside the minima, and spread = (max - min) / min of a leg's own repeats.
  launches        kernel launches per update of the whole population and the repack's launches per call, counted
                  from torch.profiler's kernel records of a separate pass of 20 updates in which no target copy
                  falls (null if the profiler gave no kernel records); launches_with_target_copy: the same count
                  for a population whose target_period is 1, so that every update carries the copy.
  bend            the smallest M whose population_us exceeds 1.5 x the population's at M = 1: where the largest
                  launches stop fitting on the device at once.
The rings hold seeded random rows and the nets torch's default initialisation: the time does not depend on the
values.
"""

from __future__ import annotations

import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))

from learn_bench import timed, torch_learner  # noqa: E402

MEMBERS = [1, 2, 4, 8, 16, 32, 64]
IN_DIM, OUT_DIM, BATCH = 10, 5, 128


def launch_counts(torch, pop, updates=20):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            pop.learn(updates)
            torch.cuda.synchronize()
        names = {}
        for ev in prof.events():
            t = getattr(ev, "device_time", None)
            if t is None:
                t = getattr(ev, "cuda_time", 0.0)
            if not t or ("learn_" not in ev.name and "qnet" not in ev.name):
                continue
            found = re.search(r"(learn_\w+|qnet\w*_kernel)", ev.name)
            short = found.group(1) if found else ev.name
            names[short] = names.get(short, 0) + 1
        if not names:
            return None
        update = sum(c for k, c in names.items() if "pack" not in k)
        pack = sum(c for k, c in names.items() if "pack" in k)
        return {"per_update": update / updates, "repack_per_call": pack, "kernels": dict(sorted(names.items()))}
    except Exception as e:  # noqa: BLE001 - the count is optional, the timings are not
        return {"error": repr(e)}


def spread(runs):
    return (max(runs) - min(runs)) / min(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_population_bench.json"))
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from merging_gym import DQNLearner, DQNPopulation, ReplayRing, _native

    if not torch.cuda.is_available():
        sys.exit("learn_population_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "updates": args.updates,
              "warmup": args.warmup, "repeats": args.repeats, "in_dim": IN_DIM, "out_dim": OUT_DIM, "batch": BATCH,
              "members": {}}
    torch.manual_seed(0)
    rings = []
    for _ in range(max(MEMBERS)):
        ring = ReplayRing(2000, device=dev)
        ring.memory.copy_(torch.rand(ring.memory.shape, device=dev) * 10.0)
        ring.memory[:, IN_DIM] = torch.randint(0, OUT_DIM, (2000,), device=dev).float()
        ring._counter.fill_(2000)
        rings.append(ring)
    nets = []
    for _ in range(max(MEMBERS)):
        eval_net, _ = torch_learner(torch, IN_DIM, OUT_DIM, dev)
        nets.append({k: v.detach() for k, v in eval_net.state_dict().items()})
    for M in MEMBERS:
        pop = DQNPopulation(nets[:M], rings[:M], batch_size=BATCH, seed=range(M))
        lone = [DQNLearner(nets[m], rings[m], batch_size=BATCH, seed=m) for m in range(M)]
        single = DQNLearner(nets[0], rings[0], batch_size=BATCH, seed=0)
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
                 "speedup_vs_lone_in_turn": min(t_us) / min(p_us),
                 "population_us_per_member": min(p_us) / M,
                 "launches": launch_counts(torch, pop),
                 # every update with a target copy due: the eighth launch
                 "launches_with_target_copy": launch_counts(
                     torch, DQNPopulation(nets[:M], rings[:M], batch_size=BATCH, target_period=1))}
        result["members"][str(M)] = entry
        print(json.dumps({f"M={M}": entry}), flush=True)
        del pop, lone, single
    base = result["members"]["1"]["population_us"]
    result["bend"] = next((M for M in MEMBERS if result["members"][str(M)]["population_us"] > 1.5 * base), None)
    result["faster_than_lone_in_turn_at_every_m_ge_2"] = all(
        result["members"][str(M)]["population_us"] < result["members"][str(M)]["lone_in_turn_us"] for M in MEMBERS[1:])
    one = result["members"]["1"]
    result["m1_population_minus_lone_relative"] = (one["population_us"] - one["lone_us"]) / one["lone_us"]
    result["m1_spread_of_repeats"] = max(one["population_spread"], one["lone_spread"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({k: result[k] for k in ("bend", "faster_than_lone_in_turn_at_every_m_ge_2",
                                             "m1_population_minus_lone_relative", "m1_spread_of_repeats")}))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
