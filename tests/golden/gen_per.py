#!/usr/bin/env python
"""Generate tests/golden/per_golden.npz from the reference's own PrioritizedReplayBuffer
(scripts/ranbowdqn.py:326-437 with its SegmentTree classes, :130-262), imported as gen_rainbow.py imports the script.

Per scenario of tests/per_ref.py (size, alpha): 1.5 size + 1 pushes (the ring wraps), then 40 rounds of
sample(32, 0.4) and update_priorities with fp32 priorities, log-uniform in [1e-3, 8]. random.random is fed the
library's own uniforms (mg_host_per_uniform(b, draw = round, seed)), so the tests can draw the same numbers;
states and actions are pushed as np.ndarray (NumPy 2's np.array(list, copy=False) raises in _encode_sample).

Recorded per round: the uniforms, S = sum(0, len - 1), the indices, the fp64 weights, the priorities, and after
the update max_priority, the leaves at the round's indices and -- for the trees of at most 16 leaves -- every
node of both trees. At the end: all leaves of both trees.

What makes index equality at alpha = 0.6 legitimate is asserted here on the reference alone: no mass lies
within 2^-20 (relative to S) of a prefix boundary of its tree, so an error of the library's pow far below that
cannot move a draw across a leaf. The seed of a scenario is the first one for which that holds on every draw;
it is recorded. Every scenario has duplicate indices within a round.

Run from the repository root with the library built:  python tests/golden/gen_per.py
"""

import copy
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path[:0] = [os.path.dirname(HERE), os.path.join(os.path.dirname(os.path.dirname(HERE)), "merging-gym_amd")]
OUT = os.path.join(HERE, "per_golden.npz")
MARGIN = 2.0 ** -20


class Unsafe(Exception):
    pass


def pushed(mod, size, alpha):
    buf = mod.PrioritizedReplayBuffer(size, alpha)
    for k in range(size + size // 2 + 1):
        buf.push(np.full(10, float(k)), np.array(k % 5), k / 8.0, np.full(10, k + 0.5), True)
    return buf


def run(mod, size, alpha, seed, base):
    import per_ref

    feed = []
    mod.random.random = lambda: feed.pop(0)
    buf = copy.deepcopy(base)  # the pushes do not depend on the seed
    C = buf._it_sum._capacity
    rng = np.random.default_rng(1000 + seed)
    rec = {name: [] for name in ("u", "S", "idx", "w", "prio", "maxp", "leaf_at_idx", "sum", "min")}
    dups = 0
    for r in range(per_ref.ROUNDS):
        u = [per_ref.uniform(b, r, seed) for b in range(per_ref.BATCH)]
        S = buf._it_sum.sum(0, len(buf._storage) - 1)
        bounds = np.cumsum(np.array(buf._it_sum._value[C:C + size]))
        mass = np.array(u) * S
        if np.abs(mass[:, None] - bounds[None, :]).min() <= MARGIN * S or mass.min() <= MARGIN * S:
            raise Unsafe
        feed[:] = u
        out = buf.sample(per_ref.BATCH, per_ref.BETA)
        assert not feed
        w, idx = np.asarray(out[5], np.float64), np.asarray(out[6], np.int64)
        assert np.array_equal(out[0][:, 0] % size, idx % size) and (idx < len(buf._storage) - 1).all()
        dups += per_ref.BATCH - len(set(idx.tolist()))
        prio = np.exp(rng.uniform(np.log(1e-3), np.log(8.0), per_ref.BATCH)).astype(np.float32)
        buf.update_priorities(idx.tolist(), [float(p) for p in prio])
        for name, v in (("u", u), ("S", S), ("idx", idx), ("w", w), ("prio", prio), ("maxp", buf._max_priority),
                        ("leaf_at_idx", [buf._it_sum[int(i)] for i in idx])):
            rec[name].append(v)
        if C <= 16:
            rec["sum"].append(list(buf._it_sum._value))
            rec["min"].append(list(buf._it_min._value))
    assert dups > 0, "no duplicate index in the scenario"
    out = {k: np.array(v) for k, v in rec.items() if v}
    out["final_sum_leaves"] = np.array(buf._it_sum._value[C:])
    out["final_min_leaves"] = np.array(buf._it_min._value[C:])
    out["seed"] = np.array(seed, np.int64)
    out["len"] = np.array(len(buf._storage), np.int64)
    # every inner node of the reference is the op of its children, bit for bit
    v = buf._it_sum._value
    assert all(v[i] == v[2 * i] + v[2 * i + 1] for i in range(1, C))
    return out


def main():
    from gen_rainbow import load_reference_module
    from merging_gym import _native  # noqa: F401  (before the loader puts its stand-in package in its place)
    import per_ref

    mod = load_reference_module()
    out = {}
    for size, alpha in per_ref.SCENARIOS:
        base = pushed(mod, size, alpha)
        for seed in range(100000):
            try:
                rec = run(mod, size, alpha, seed, base)
            except Unsafe:
                continue
            break
        else:
            raise SystemExit(f"no safe seed for size {size}, alpha {alpha}")
        print(f"size {size} alpha {alpha}: seed {seed}")
        for k, v in rec.items():
            out[f"{per_ref.scenario_key(size, alpha)}/{k}"] = v
    np.savez_compressed(OUT, **out)
    print(f"wrote {OUT}: {os.path.getsize(OUT)} bytes")


if __name__ == "__main__":
    main()
