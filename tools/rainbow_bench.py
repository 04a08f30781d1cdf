"""Time of Rainbow's acting loop on the device (not part of bench.py).

    python tools/rainbow_bench.py [--out profiles/rainbow_bench.json] [--envs 1048576] [--steps 16]
                                  [--only fused_vs,composed_vs,fused_self_beside_vs --repeats 9]

In one process on one GPU, 2^20 envs, T = 16 steps per launch, 10 untimed then 40 timed launches between two HIP
events (as bench.py times its Q-net legs), each leg `--repeats` times with the legs alternating so that drift of
a shared machine hits all of them:
  fused_none / fused_self        MergeVecEnv.rollout_rainbow, opponent "none" / "self": one launch per T steps;
  composed_none / composed_self  the same steps as separate launches: RainbowNet.forward per view
                                 (mg_rainbow_forward), then MergeVecEnv.step -- 2 or 3 launches per step;
  fused_vs / composed_vs         against ANOTHER Rainbow net: rollout_rainbow(T, net, opponent=other) in one launch
                                 (mg_rollout_rainbow_vs), and the only route without it -- net.act(obs),
                                 other.act(obs, rotate=3), env.step, three launches per step;
  fused_self_beside_vs           fused_self once more, for a run of the vs legs alone (--only): mode 2 beside mode 3
                                 in the same windows;
  qnet_self                      the DQN's rollout_qnet(..., opponent="self") for scale (the checkpoint bench.py
                                 uses).
--only runs the named legs alone and merges them into the --out file, whose other legs and keys stay as they are
(the legs measured together are listed under "merged_runs").
Per leg: us_per_step (median of the repeats, all repeats listed, the best one and the spread (max - min) / median
beside it), env_steps_per_s, and for the Rainbow legs
flops_per_s and fraction_of_bf16_peak in the reference's own FLOPs: 2 x (10 x 32 + 32 x 64 + 2 x 64 x 64 + 64 x 51 +
64 x 255) = 60,288 FLOP per env and view, against the 2.5 PFLOP/s dense bf16 peak of the MI355X. That is a
whole-launch rate (forward, head and env step together) over the matrix peak, not a kernel's share of it.
"""

from __future__ import annotations

import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))

FLOP_PER_VIEW = 2 * (10 * 32 + 32 * 64 + 2 * 64 * 64 + 64 * 51 + 64 * 255)  # ranbowdqn.py:508-515
BF16_PEAK = 2.5e15


def rainbow_net(torch, dev, seed=0):
    """RainbowDQN(10, 5)'s shapes with torch's default initialisation and unit noise scale: the time does not
    depend on the values."""
    from merging_gym.rainbow import NOISY, PLAIN, SHAPES, RainbowNet

    g = torch.Generator().manual_seed(seed)
    sd = {}
    for name in PLAIN:
        o, i = SHAPES[name]
        sd[f"{name}.weight"] = (torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5
        sd[f"{name}.bias"] = (torch.rand(o, generator=g) * 2 - 1) / i ** 0.5
    for name in NOISY:
        o, i = SHAPES[name]
        sd[f"{name}.weight_mu"] = (torch.rand(o, i, generator=g) * 2 - 1) / i ** 0.5
        sd[f"{name}.bias_mu"] = (torch.rand(o, generator=g) * 2 - 1) / i ** 0.5
        sd[f"{name}.weight_sigma"] = torch.full((o, i), 0.4 / i ** 0.5)
        sd[f"{name}.bias_sigma"] = torch.full((o,), 0.4 / o ** 0.5)
        sd[f"{name}.weight_epsilon"] = torch.zeros(o, i)
        sd[f"{name}.bias_epsilon"] = torch.zeros(o)
    net = RainbowNet.from_state_dict(sd, device=dev)
    net.reset_noise(generator=g)
    return net


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rainbow_bench.json"))
    ap.add_argument("--envs", type=int, default=1 << 20)
    ap.add_argument("--steps", type=int, default=16)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--only", default="", help="comma-separated legs to run alone and merge into --out")
    args = ap.parse_args()

    import numpy as np
    import torch

    from merging_gym import MergeVecEnv, _native
    from merging_gym.policy import QNet

    if not torch.cuda.is_available():
        sys.exit("rainbow_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    n, T = args.envs, args.steps
    net, other = rainbow_net(torch, dev), rainbow_net(torch, dev, seed=1)
    f = np.load(os.path.join(ROOT, "tests", "golden", "dqn_checkpoints.npz"))
    qnet = QNet.from_state_dict({k.split("/", 1)[1]: f[k] for k in f.files if k.startswith("l1/")}, device=dev)
    env = MergeVecEnv(n, device=dev)
    env.rollout_random(200, 1, first_step=0, final_observation=False, won_mask=False)  # mid-episode batch

    def fused(opponent):
        return lambda: env.rollout_rainbow(T, net, opponent=opponent, final_observation=False, won_mask=False)

    def composed(opponent):
        def run():
            obs = env.observe()
            for _ in range(T):
                a1 = net.act(obs, 0)
                a2 = net.act(obs, 3) if opponent == "self" else None
                obs = env.step(a1, a2)[0]
        return run

    def composed_vs():
        obs = env.observe()
        for _ in range(T):
            obs = env.step(net.act(obs, 0), other.act(obs, 3))[0]

    state = {"k": 10_000_000}

    def qnet_self():
        env.rollout_qnet(T, qnet, 1, opponent="self", first_step=state["k"], final_observation=False, won_mask=False)
        state["k"] += T

    legs = {"fused_none": (fused("none"), 1), "fused_self": (fused("self"), 2),
            "composed_none": (composed("none"), 1), "composed_self": (composed("self"), 2),
            "fused_vs": (fused(other), 2), "composed_vs": (composed_vs, 2),
            "fused_self_beside_vs": (fused("self"), 2), "qnet_self": (qnet_self, 0)}
    only = [k for k in args.only.split(",") if k]
    if only:
        unknown = [k for k in only if k not in legs]
        if unknown:
            sys.exit(f"--only: unknown legs {unknown}; the legs are {list(legs)}")
        legs = {k: legs[k] for k in only}

    def timed(fn):
        for _ in range(args.warmup):
            fn()
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        for _ in range(args.launches):
            fn()
        b.record()
        torch.cuda.synchronize()
        return a.elapsed_time(b) * 1e3 / (args.launches * T)  # microseconds per step

    runs = {k: [] for k in legs}
    for _ in range(args.repeats):
        for name, (fn, _) in legs.items():
            runs[name].append(timed(fn))
    setup = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "envs": n, "steps_per_launch": T,
             "warmup_launches": args.warmup, "timed_launches": args.launches}
    if only:
        with open(args.out) as fh:
            result = json.load(fh)
        result.setdefault("merged_runs", []).append(dict(setup, legs=only, repeats=args.repeats))
    else:
        result = dict(setup, flop_per_env_and_view=FLOP_PER_VIEW, bf16_peak_flops=BF16_PEAK, legs={})
    for name, (_, views) in legs.items():
        us = statistics.median(runs[name])
        entry = {"us_per_step": us, "us_per_step_runs": runs[name], "env_steps_per_s": n / (us * 1e-6),
                 "us_per_step_best": min(runs[name]), "spread": (max(runs[name]) - min(runs[name])) / us}
        if views:
            entry["views"] = views
            entry["flops_per_s"] = views * FLOP_PER_VIEW * n / (us * 1e-6)
            entry["fraction_of_bf16_peak"] = entry["flops_per_s"] / BF16_PEAK
        result["legs"][name] = entry
    if not only:
        result["fused_over_composed"] = {}
    for k in ("none", "self", "vs"):
        if f"composed_{k}" in legs and f"fused_{k}" in legs:
            result["fused_over_composed"][k] = (result["legs"][f"composed_{k}"]["us_per_step"]
                                                / result["legs"][f"fused_{k}"]["us_per_step"])
    if "fused_vs" in legs and "fused_self_beside_vs" in legs:  # the same run's mode 2 beside mode 3
        result["vs_over_self"] = (result["legs"]["fused_vs"]["us_per_step"]
                                  / result["legs"]["fused_self_beside_vs"]["us_per_step"])
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        json.dump(result, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: round(result["legs"][k]["us_per_step"], 2) for k in legs}))


if __name__ == "__main__":
    main()
