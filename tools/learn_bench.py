"""Time of one DQN.learn update on the device (not part of bench.py).

    python tools/learn_bench.py [--out profiles/learn_bench.json] [--updates 200] [--warmup 20]

Per shape -- batch 128 for the three nets (10 -> 5 DQN, 11 -> 5 HDQN, 10 -> 3 Goal_DQN) and batch 1024
for 10 -> 5 -- in one process on one GPU:
  ours_us        microseconds per update of DQNLearner.learn(updates): HIP events around one call that
                 enqueues all of them, after `warmup` untimed updates;
  torch_us       the reference's learn() (scripts/main.py:122-157) in eager torch on the same device,
                 fed by ReplayRing.sample, timed the same way;
  launches       kernel launches per update and per_launch_us = ours_us / launches: the update is a
                 dependent chain of launches, so this is the figure to hold against a launch's cost;
  kernels        per kernel, the mean device time of one launch and the launches per update, from
                 torch.profiler's kernel records of a separate pass of 20 updates (tracing slows the
                 host, so the two figures above are taken with it off). null if the profiler gave no
                 kernel records.
The ring holds seeded random rows and the nets torch's default initialisation: the time does not depend
on the values.
"""

from __future__ import annotations

import argparse
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))

SHAPES = [("dqn_10_5_b128", 10, 5, 128), ("hdqn_11_5_b128", 11, 5, 128), ("goal_10_3_b128", 10, 3, 128),
          ("dqn_10_5_b1024", 10, 5, 1024)]
LAUNCHES = 7  # layer 1 + gather, layer 2, layer 3 + target, three backward layers, Adam


def torch_learner(torch, in_dim, out_dim, dev):
    import torch.nn as nn
    import torch.nn.functional as F

    class Net(nn.Module):  # main.py:30-47
        def __init__(self):
            super().__init__()
            self.fc1, self.fc2, self.out = nn.Linear(in_dim, 200), nn.Linear(200, 100), nn.Linear(100, out_dim)

        def forward(self, x):
            return self.out(F.relu(self.fc2(F.relu(self.fc1(x)))))

    eval_net, target_net = Net().to(dev), Net().to(dev)
    opt = torch.optim.Adam(eval_net.parameters(), lr=0.01)
    state = {"step": 0}

    def learn(ring, batch):  # main.py:122-157
        if state["step"] % 100 == 0:
            target_net.load_state_dict(eval_net.state_dict())
        s, a, r, s2 = ring.sample(batch, seed=1, draw=state["step"])
        state["step"] += 1
        q_eval = eval_net(s).gather(1, a)
        q_next = target_net(s2).detach()
        am = eval_net(s2).detach().max(1)[1]
        q_target = r + 0.9 * q_next.gather(1, am.view(-1, 1))
        loss = F.mse_loss(q_eval, q_target)
        opt.zero_grad()
        loss.backward()
        opt.step()

    return eval_net, learn


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
            name = ev.name
            if "learn_" not in name and "qnet" not in name:
                continue
            t = getattr(ev, "device_time", None)
            if t is None:
                t = getattr(ev, "cuda_time", 0.0)
            if not t:
                continue
            m = re.search(r"(learn_\w+|qnet\w*_kernel)", name)
            short = m.group(1) if m else name
            cnt, tot = rows.get(short, (0, 0.0))
            rows[short] = (cnt + 1, tot + float(t))
        if not rows:
            return None
        return {k: {"per_update": c / updates, "mean_us": tot / c} for k, (c, tot) in sorted(rows.items())}
    except Exception as e:  # noqa: BLE001 - the breakdown is optional, the timings are not
        return {"error": repr(e)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "learn_bench.json"))
    ap.add_argument("--updates", type=int, default=200)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--repeats", type=int, default=3)
    args = ap.parse_args()

    import torch

    from merging_gym import DQNLearner, ReplayRing, _native

    if not torch.cuda.is_available():
        sys.exit("learn_bench needs the GPU: a time taken elsewhere says nothing")
    dev = torch.device("cuda", 0)
    result = {"device": torch.cuda.get_device_name(0), "build": _native.build_info(), "updates": args.updates,
              "warmup": args.warmup, "launches_per_update": LAUNCHES, "shapes": {}}
    for name, in_dim, out_dim, batch in SHAPES:
        torch.manual_seed(0)
        ring = ReplayRing(2000, device=dev, goal=in_dim == 11)
        ring.memory.copy_(torch.rand(ring.memory.shape, device=dev) * 10.0)
        ring.memory[:, in_dim] = torch.randint(0, out_dim, (2000,), device=dev).float()
        ring._counter.fill_(2000)
        eval_net, torch_learn = torch_learner(torch, in_dim, out_dim, dev)
        learner = DQNLearner({k: v.detach() for k, v in eval_net.state_dict().items()}, ring, batch_size=batch)
        learner.learn(args.warmup)
        for _ in range(args.warmup):
            torch_learn(ring, batch)
        ours, ref = [], []
        for _ in range(args.repeats):  # alternating, so drift of the shared machine hits both
            ours.append(timed(torch, lambda: learner.learn(args.updates)) / args.updates)
            ref.append(timed(torch, lambda: [torch_learn(ring, batch) for _ in range(args.updates)]) / args.updates)
        entry = {"in_dim": in_dim, "out_dim": out_dim, "batch": batch,
                 "ours_us": min(ours), "ours_us_runs": ours, "torch_us": min(ref), "torch_us_runs": ref,
                 "launches": LAUNCHES, "per_launch_us": min(ours) / LAUNCHES,
                 "speedup_vs_torch": min(ref) / min(ours), "kernels": kernel_breakdown(torch, learner)}
        result["shapes"][name] = entry
        print(json.dumps({name: entry}), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1, sort_keys=True)
        f.write("\n")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
