"""The lone Rainbow learners before and after a change: tools/rainbow_learn_bench.py's figures of two builds side by side.

    python tools/rainbow_learn_lone_compare.py --parent P1.json P2.json P3.json --new N1.json N2.json N3.json
                                               [--order "P N P N P N"] [--out profiles/rainbow_learn_lone_compare.json]

Each argument is the JSON one process of tools/rainbow_learn_bench.py wrote, for the parent commit's build and for the
changed one; run the processes alternately on one GPU so that drift hits both, and pass the order they ran in as
--order (it is recorded: the legs with host work between launches follow it). Needs no GPU itself. For every figure
(ours_us: host noise, device_noise_us, prioritized_us; B = 32 and 128) it keeps each process's best and its repeats
and applies the rule the Rainbow commits use for an unchanged path:

    parent_best_plus_spread = min(parent's per-process bests) + (max - min of them) = the largest of them
    new_best_within         = min(new's per-process bests) <= parent_best_plus_spread

new_processes_above lists the new processes whose own best lies above the bound, so that they are not hidden by the
best; every_best_within_parent_best_plus_spread is the conjunction over the figures.
"""

from __future__ import annotations

import argparse
import json
import os

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIGURES = ("ours_us", "device_noise_us", "prioritized_us")


def compare(parent, new, order=None):
    out = {"what": "tools/rainbow_learn_bench.py on the parent commit's build and on this one, alternately, one process "
                   "per file; microseconds per update, each process's best of its repeats and the repeats",
           "order": order, "device": new[0]["device"], "parent_build": parent[0]["build"], "build": new[0]["build"], "figures": {}}
    for b in sorted(new[0]["batches"], key=lambda k: int(k[1:])):
        for k in FIGURES:
            pv = [r["batches"][b][k] for r in parent]
            nv = [r["batches"][b][k] for r in new]
            bound = min(pv) + (max(pv) - min(pv))
            out["figures"][f"{b}.{k}"] = {
                "parent": pv, "parent_runs": [r["batches"][b][k + "_runs"] for r in parent],
                "new": nv, "new_runs": [r["batches"][b][k + "_runs"] for r in new],
                "parent_best_plus_spread": bound, "new_best": min(nv), "new_best_within": min(nv) <= bound,
                "new_processes_above": [v for v in nv if v > bound]}
    out["every_best_within_parent_best_plus_spread"] = all(f["new_best_within"] for f in out["figures"].values())
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parent", nargs="+", required=True)
    ap.add_argument("--new", nargs="+", required=True)
    ap.add_argument("--order", default=None, help="the order the processes ran in, e.g. 'P N P N P N'")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "rainbow_learn_lone_compare.json"))
    args = ap.parse_args()
    load = lambda paths: [json.load(open(p)) for p in paths]  # noqa: E731
    out = compare(load(args.parent), load(args.new), args.order)
    with open(args.out, "w") as f:
        json.dump(out, f, indent=1, sort_keys=True)
        f.write("\n")
    for name, fig in out["figures"].items():
        print(name, "parent", [round(v, 2) for v in fig["parent"]], "new", [round(v, 2) for v in fig["new"]],
              "bound", round(fig["parent_best_plus_spread"], 2), "ok" if fig["new_best_within"] else "ABOVE")
    print(f"wrote {args.out}")


if __name__ == "__main__":
    main()
