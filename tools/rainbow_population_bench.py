"""Time of one update of a population of Rainbow learners on the device (not part of bench.py).

    python tools/rainbow_population_bench.py [--out profiles/rainbow_population_bench.json] [--updates 200] [--warmup 20]

For RainbowDQN(10, 5) at batch 32 and 128 and M in {1, 2, 4, 8, 16, 32, 64} members, in one process on one GPU,
each member on its own full 10,000-row replay with its own seed, the noise drawn on the device:
  population_us   microseconds per update of all M members through RainbowPopulation.learn(updates): HIP events
                  around one call that enqueues all of them (the noise launch and the pack included), after `warmup`
                  untimed updates;
  lone_in_turn_us the same M agents as M RainbowLearner(DeviceNoise)s, learn(updates) called on each in turn inside
                  one pair of events: the only way to train M agents without the population;
  lone_us         one lone RainbowLearner(DeviceNoise), timed the same way;
each the best of `repeats`, the three legs alternating inside every repeat so that drift of a shared machine hits all
of them; the runs are kept beside the minima, and spread = (max - min) / min of a leg's own repeats.
  bend            the smallest M whose population_us exceeds 1.5 x the population's at M = 1.
  not_slower_than_lone_in_turn  population_us <= lone_in_turn_us at every measured point.
The replays hold seeded random rows and the nets torch's default initialisation: the time does not depend on the
values.
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

MEMBERS = [1, 2, 4, 8, 16, 32, 64]
BATCHES = [32, 128]


def spread(runs):
    return (max(runs) - min(runs)) / min(runs)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rainbow_population_bench.json"))
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from merging_gym import DeviceNoise, RainbowLearner, RainbowPopulation, RainbowReplay, _native

    if not torch.cuda.is_available():
        sys.exit("rainbow_population_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "updates": args.updates,
              "warmup": args.warmup, "repeats": args.repeats, "capacity": 10000, "batches": {}}
    torch.manual_seed(0)
    replays = []
    for _ in range(max(MEMBERS)):
        replay = RainbowReplay(10000, device=dev)
        fill(torch, replay, dev)
        replay._counter.fill_(10000)
        replays.append(replay)
    nets = []
    for _ in range(max(MEMBERS)):
        net, _ = torch_rainbow(torch, dev)
        nets.append({k: v.detach() for k, v in net.state_dict().items()})
    for batch in BATCHES:
        by_m = {}
        for M in MEMBERS:
            pop = RainbowPopulation(nets[:M], replays[:M], batch_size=batch, seed=range(M))
            lone = [RainbowLearner(nets[m], replays[m], batch_size=batch, seed=m, generator=DeviceNoise())
                    for m in range(M)]
            single = RainbowLearner(nets[0], replays[0], batch_size=batch, seed=0, generator=DeviceNoise())
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
        result["batches"][f"b{batch}"] = {
            "members": by_m,
            "bend": next((M for M in MEMBERS if by_m[str(M)]["population_us"] > 1.5 * base), None),
            "not_slower_than_lone_in_turn": all(e["population_us"] <= e["lone_in_turn_us"] for e in by_m.values()),
            "m1_population_minus_lone_relative": (base - by_m["1"]["lone_us"]) / by_m["1"]["lone_us"]}
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps({b: {k: v for k, v in r.items() if k != "members"} for b, r in result["batches"].items()}))
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
