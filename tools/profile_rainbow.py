"""Workload and summary of the Rainbow rollout's SQ counter passes (tools/pmc_rainbow.sh).

    python tools/profile_rainbow.py                        # the workload rocprofv3 wraps: 4 launches per opponent
    python tools/profile_rainbow.py --summarise DIR --out profiles/pmc_rainbow.json

The workload: 2^20 envs, T = 16, rollout_rainbow with opponent "none" and "self", 4 launches each after one
warm-up launch. The summary takes, per kernel instance, the mean over its dispatches of every counter collected
(VALUBusy and MfmaUtil are rocprofv3's derived metrics: issue cycles of the SIMDs, and matrix-pipe busy cycles,
over the kernel's GPU time) and the instruction counts per 64-env forward.
"""

from __future__ import annotations

import argparse
import csv
import glob
import json
import os
import sys
from collections import defaultdict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "merging-gym_amd"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
ENVS, T = 1 << 20, 16


def workload():
    import torch

    from merging_gym import MergeVecEnv
    from rainbow_bench import rainbow_net

    dev = torch.device("cuda", 0)
    net = rainbow_net(torch, dev)
    env = MergeVecEnv(ENVS, device=dev)
    env.rollout_random(200, 1, first_step=0, final_observation=False, won_mask=False)
    for opponent in ("none", "self"):
        for _ in range(5):
            env.rollout_rainbow(T, net, opponent=opponent, final_observation=False, won_mask=False)
    torch.cuda.synchronize()


def summarise(pmc_dir, out):
    vals = defaultdict(lambda: defaultdict(list))
    for p in glob.glob(os.path.join(pmc_dir, "**", "*counter_collection.csv"), recursive=True):
        per = defaultdict(float)
        for r in csv.DictReader(open(p)):
            if "rainbow_rollout" not in r["Kernel_Name"]:
                continue
            k = "rainbow_rollout<2>" if "2" in r["Kernel_Name"].split("rainbow_rollout_kernel")[1][:6] else "rainbow_rollout<0>"
            per[(k, r["Counter_Name"], r["Dispatch_Id"])] += float(r["Counter_Value"])
        for (k, c, _), v in per.items():
            vals[k][c].append(v)
    res = {}
    for k, cs in sorted(vals.items()):
        mean = {c: sum(v) / len(v) for c, v in sorted(cs.items())}
        views = 2 if k.endswith("<2>") else 1
        forwards = ENVS / 64 * T * views
        row = {"per_dispatch": mean, "forwards_per_dispatch": forwards}
        for c in ("SQ_INSTS_VALU", "SQ_INSTS_MFMA", "SQ_INSTS_LDS", "SQ_INSTS_SALU"):
            if c in mean:
                row[c + "_per_forward"] = mean[c] / forwards
        res[k] = row
    with open(out, "w") as fh:
        json.dump(res, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps({k: {c: round(v, 2) for c, v in r.items() if c.endswith("_per_forward")} for k, r in res.items()}))
    print(json.dumps({k: {c: round(r["per_dispatch"][c], 2) for c in ("VALUBusy", "MfmaUtil") if c in r["per_dispatch"]}
                      for k, r in res.items()}))


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--summarise")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pmc_rainbow.json"))
    a = ap.parse_args()
    if a.summarise:
        summarise(a.summarise, a.out)
    else:
        workload()
