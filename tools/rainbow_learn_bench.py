"""Time of one Rainbow update (compute_td_loss) on the device (not part of bench.py).

    python tools/rainbow_learn_bench.py [--out profiles/rainbow_learn_bench.json] [--updates 200] [--warmup 20]

Per batch size (32, the reference's, and 128) in one process on one GPU:
  ours_us        microseconds per update of RainbowLearner.learn(updates): HIP events around one call that draws
                 the noise factors on the host, uploads them once and enqueues every update, after `warmup`
                 untimed updates;
  device_noise_us
                 the same call of a RainbowLearner(generator=DeviceNoise()): the factors drawn by
                 rainbow_noise_kernel on the stream (one launch per call, not per update), no host draw and no
                 upload; timed exactly as ours_us, alternating with it;
  torch_us       ranbowdqn.py's compute_td_loss (:554-609) in eager torch on device tensors -- both forwards,
                 the projection with index_add_, the clamped cross-entropy, Adam, both reset_noise calls (drawn
                 on the host as the reference draws them) -- fed by RainbowReplay.sample, timed the same way;
  prioritized_us the same call on a PrioritizedRainbowReplay (alpha 0.6, beta 0.4) of the same rows, whose tree 64
                 rounds of update_priorities have shaped: nine launches per update, the sample before and the
                 priority update behind the seven;
  launches       kernel launches per update and per_launch_us = ours_us / launches;
  kernels        per kernel, the mean device time of one launch and the launches per update, from
                 torch.profiler's kernel records of a separate pass of 20 updates. null if the profiler gave
                 no kernel records. The rainbow_noise_kernel row is the device-noise learner's (the host-noise
                 learner never launches it); device_noise_kernels is that learner's whole breakdown.
"store": one store of n = 2^20 envs x T = 16 steps through mg_rainbow_replay_store (uniform_us) and through
mg_per_store (prioritized_us: the rows, the written leaves, their ancestors level by level), per ring capacity.
Best of `repeats` alternating runs. The replay memory holds seeded random rows and the nets their default
initialisation: the time does not depend on the values.
"""

from __future__ import annotations

import argparse
import json
import math
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))

BATCHES = (32, 128)
PER_LAUNCHES = 9  # the sample, the seven, the priority update
LAUNCHES = 7  # rows + both forwards + projection + dlogits, four backward launches, Adam + loss, noise + effective


def torch_rainbow(torch, dev):
    """RainbowDQN(10, 5) and compute_td_loss in eager torch on `dev`."""
    import torch.nn as nn
    import torch.nn.functional as F

    atoms, vmin, vmax = 51, -10.0, 10.0

    class Noisy(nn.Module):
        def __init__(self, i, o):
            super().__init__()
            self.i, self.o = i, o
            r = 1 / math.sqrt(i)
            self.weight_mu = nn.Parameter(torch.empty(o, i).uniform_(-r, r))
            self.weight_sigma = nn.Parameter(torch.full((o, i), 0.4 / math.sqrt(i)))
            self.bias_mu = nn.Parameter(torch.empty(o).uniform_(-r, r))
            self.bias_sigma = nn.Parameter(torch.full((o,), 0.4 / math.sqrt(o)))
            self.register_buffer("weight_epsilon", torch.zeros(o, i))
            self.register_buffer("bias_epsilon", torch.zeros(o))
            self.reset_noise()

        @staticmethod
        def scale(n):
            x = torch.randn(n)
            return x.sign().mul(x.abs().sqrt())

        def reset_noise(self):
            self.weight_epsilon.copy_(self.scale(self.o).ger(self.scale(self.i)))
            self.bias_epsilon.copy_(self.scale(self.o))

        def forward(self, x):
            return F.linear(x, self.weight_mu + self.weight_sigma * self.weight_epsilon,
                            self.bias_mu + self.bias_sigma * self.bias_epsilon)

    class Net(nn.Module):
        def __init__(self):
            super().__init__()
            self.linear1, self.linear2 = nn.Linear(10, 32), nn.Linear(32, 64)
            self.noisy_value1, self.noisy_value2 = Noisy(64, 64), Noisy(64, atoms)
            self.noisy_advantage1, self.noisy_advantage2 = Noisy(64, 64), Noisy(64, 5 * atoms)

        def forward(self, x):
            x = F.relu(self.linear2(F.relu(self.linear1(x))))
            v = self.noisy_value2(F.relu(self.noisy_value1(x))).view(-1, 1, atoms)
            a = self.noisy_advantage2(F.relu(self.noisy_advantage1(x))).view(-1, 5, atoms)
            return F.softmax(v + a - a.mean(1, keepdim=True), dim=2)

        def reset_noise(self):
            for m in (self.noisy_value1, self.noisy_value2, self.noisy_advantage1, self.noisy_advantage2):
                m.reset_noise()

    current, target = Net().to(dev), Net().to(dev)
    target.load_state_dict(current.state_dict())
    opt = torch.optim.Adam(current.parameters(), 0.001)
    support = torch.linspace(vmin, vmax, atoms, device=dev)
    state = {"draw": 0}

    def learn(replay, batch):
        s, a, r, s2, done = replay.sample(batch, seed=1, draw=state["draw"])
        state["draw"] += 1
        with torch.no_grad():
            nd = target(s2) * support
            nd = nd[torch.arange(batch, device=dev), nd.sum(2).max(1)[1]]
            tz = (r[:, None] + (1 - done[:, None]) * 0.99 * support[None]).clamp(vmin, vmax)
            b = (tz - vmin) / ((vmax - vmin) / (atoms - 1))
            lo, up = b.floor().long(), b.ceil().long()
            off = (torch.arange(batch, device=dev) * atoms)[:, None]
            proj = torch.zeros(batch * atoms, device=dev)
            proj.index_add_(0, (lo + off).view(-1), (nd * (up.float() - b)).view(-1))
            proj.index_add_(0, (up + off).view(-1), (nd * (b - lo.float())).view(-1))
        dist = current(s)[torch.arange(batch, device=dev), a]
        dist.data.clamp_(0.01, 0.99)
        loss = -(proj.view(batch, atoms) * dist.log()).sum(1).mean()
        opt.zero_grad()
        loss.backward()
        opt.step()
        current.reset_noise()
        target.reset_noise()

    return current, learn


def timed(torch, fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    a.record()
    fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) * 1e3  # microseconds


def kernel_breakdown(torch, learner, updates=20):
    try:
        from torch.profiler import ProfilerActivity, profile

        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            learner.learn(updates)
            torch.cuda.synchronize()
        rows = {}
        for ev in prof.events():
            m = re.search(r"(rl_\w+_kernel|learn_\w+_kernel|per_\w+_kernel|rainbow_pack_kernel|rainbow_noise_kernel)", ev.name)
            if not m:
                continue
            t = getattr(ev, "device_time", None)
            if t is None:
                t = getattr(ev, "cuda_time", 0.0)
            if not t:
                continue
            cnt, tot = rows.get(m.group(1), (0, 0.0))
            rows[m.group(1)] = (cnt + 1, tot + float(t))
        if not rows:
            return None
        return {k: {"per_update": c / updates, "mean_us": tot / c} for k, (c, tot) in sorted(rows.items())}
    except Exception as e:  # noqa: BLE001 - the breakdown is optional, the timings are not
        return {"error": repr(e)}


def fill(torch, replay, dev):
    n = replay.capacity
    replay.memory.copy_(torch.rand(replay.memory.shape, device=dev) * 10.0)
    replay.memory[:, 10] = torch.randint(0, 5, (n,), device=dev).float()
    replay.memory[:, 22] = torch.randint(0, 2, (n,), device=dev).float()


def store_cost(torch, dev, repeats, n=1 << 20, T=16, capacities=(10000, 1 << 20)):
    from merging_gym import PrioritizedRainbowReplay, RainbowReplay

    obs_first = torch.rand((n, 10), device=dev)
    obs, rew = torch.rand((T, n, 10), device=dev), torch.rand((T, n, 2), device=dev)
    a1 = torch.randint(0, 5, (T, n), device=dev).to(torch.int8)
    done = (torch.rand((T, n), device=dev) < 0.01).to(torch.uint8)
    out = {"n": n, "num_steps": T, "capacities": {}}
    for cap in capacities:
        rings = {"uniform_us": RainbowReplay(cap, device=dev), "prioritized_us": PrioritizedRainbowReplay(cap, 0.6, device=dev)}
        runs = {k: [] for k in rings}
        for rep_ in range(repeats + 1):  # the first pass warms up
            for k, ring in rings.items():
                t = timed(torch, lambda: ring.store(obs_first, obs, a1, rew, done, obs))
                if rep_:
                    runs[k].append(t)
        out["capacities"][str(cap)] = {**{k: min(v) for k, v in runs.items()}, **{k + "_runs": v for k, v in runs.items()}}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rainbow_learn_bench.json"))
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from merging_gym import DeviceNoise, PrioritizedRainbowLearner, PrioritizedRainbowReplay, RainbowLearner, RainbowReplay, _native

    if not torch.cuda.is_available():
        sys.exit("rainbow_learn_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "updates": args.updates,
              "warmup": args.warmup, "launches_per_update": LAUNCHES, "batches": {}}
    for batch in BATCHES:
        torch.manual_seed(0)
        replay = RainbowReplay(10000, device=dev)
        fill(torch, replay, dev)
        replay._counter.fill_(10000)
        per = PrioritizedRainbowReplay(10000, 0.6, device=dev)
        per.store(torch.rand((10000, 10), device=dev), torch.rand((1, 10000, 10), device=dev),
                  torch.zeros((1, 10000), dtype=torch.int8, device=dev), torch.rand((1, 10000, 2), device=dev))
        per.memory.copy_(replay.memory)
        for r in range(64):
            idx, _ = per.sample_indices(1024, 0.4, seed=2, draw=r)
            per.update_priorities(idx, torch.rand(1024, device=dev) * 4.0 + 1e-3)
        net, torch_learn = torch_rainbow(torch, dev)
        learner = RainbowLearner({k: v.detach() for k, v in net.state_dict().items()}, replay, batch_size=batch)
        plearner = PrioritizedRainbowLearner({k: v.detach() for k, v in net.state_dict().items()}, per, batch_size=batch)
        dlearner = RainbowLearner({k: v.detach() for k, v in net.state_dict().items()}, replay, batch_size=batch,
                                  generator=DeviceNoise())
        learner.learn(args.warmup)
        dlearner.learn(args.warmup)
        plearner.learn(args.warmup)
        for _ in range(args.warmup):
            torch_learn(replay, batch)
        ours, ref, prio, devn = [], [], [], []
        for _ in range(args.repeats):  # alternating, so drift of the shared machine hits both
            ours.append(timed(torch, lambda: learner.learn(args.updates)) / args.updates)
            devn.append(timed(torch, lambda: dlearner.learn(args.updates)) / args.updates)
            prio.append(timed(torch, lambda: plearner.learn(args.updates)) / args.updates)
            ref.append(timed(torch, lambda: [torch_learn(replay, batch) for _ in range(args.updates)]) / args.updates)
        entry = {"batch": batch, "ours_us": min(ours), "ours_us_runs": ours, "torch_us": min(ref), "torch_us_runs": ref,
                 "launches": LAUNCHES, "per_launch_us": min(ours) / LAUNCHES,
                 "speedup_vs_torch": min(ref) / min(ours), "kernels": kernel_breakdown(torch, learner),
                 "prioritized_us": min(prio), "prioritized_us_runs": prio, "prioritized_launches": PER_LAUNCHES,
                 "prioritized_kernels": kernel_breakdown(torch, plearner),
                 "device_noise_us": min(devn), "device_noise_us_runs": devn,
                 "device_noise_vs_ours": min(devn) / min(ours),
                 "device_noise_kernels": kernel_breakdown(torch, dlearner)}
        noise_row = (entry["device_noise_kernels"] or {}).get("rainbow_noise_kernel")
        if noise_row and isinstance(entry["kernels"], dict) and "error" not in entry["kernels"]:
            entry["kernels"]["rainbow_noise_kernel"] = noise_row
        result["batches"][f"b{batch}"] = entry
        print(json.dumps({f"b{batch}": entry}), flush=True)
    result["store"] = store_cost(torch, dev, args.repeats)
    print(json.dumps({"store": result["store"]}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
