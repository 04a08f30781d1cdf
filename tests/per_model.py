"""An independent model of the prioritized buffer: SumSegmentTree, MinSegmentTree and PrioritizedReplayBuffer
(scripts/ranbowdqn.py:130-262, :326-437) restated with Python floats and lists, one transition at a time. It
shares nothing with the library's store: no segments, no level bounds, no launches. A bulk store is `count`
single pushes, each a leaf set and a walk to the root, so a level bound that is one node short in the library
(and in the host twin, which sizes its loops with the same bound) shows here as a stale node.

Then the scenario both sides of the comparison run (tests/test_per_model_host.py on the host twins,
tests/test_gpu_per.py on the device): SCENARIO_STORES, update_batch and run_scenario."""

from __future__ import annotations

import math

import numpy as np

import per_ref as P

CAPACITIES = (1, 2, 3, 4, 5, 8, 1024, 1025, 4096, 5000, 9000)
ALPHAS = (1.0, 0.6)
UPDATE_BATCHES = (1, 33, 1024)
SAMPLE_BATCH, SAMPLE_BETAS, SAMPLE_SEED = 64, (0.4, 1.0), 5


class PerModel:
    def __init__(self, capacity, alpha):
        self.cap, self.alpha = int(capacity), float(alpha)
        self.C = 1
        while self.C < self.cap:
            self.C *= 2
        self.sum = [0.0] * (2 * self.C)  # node 1 the root, leaf i at C + i, node 0 unused
        self.min = [math.inf] * (2 * self.C)
        self.max_priority = 1.0
        self.counter = 0

    def __len__(self):
        return min(self.counter, self.cap)

    def leaf(self, p):
        """priority ** alpha as the library takes it: the priority itself at alpha 1, else the library's own pow
        (pinned against libm by test_pow_error_against_libm), so the model's bits are the library's for any alpha."""
        return float(p) if self.alpha == 1.0 else float(P.host_pow([float(p)], [self.alpha])[0])

    def _set(self, slot, value):
        node = self.C + slot
        self.sum[node] = self.min[node] = value
        node //= 2
        while node >= 1:
            self.sum[node] = self.sum[2 * node] + self.sum[2 * node + 1]
            self.min[node] = min(self.min[2 * node], self.min[2 * node + 1])
            node //= 2

    def push(self, count):
        value = self.leaf(self.max_priority)  # max_priority does not move during pushes
        for _ in range(int(count)):
            self._set(self.counter % self.cap, value)
            self.counter += 1

    def update(self, idx, prio):
        """Entries in order; one is left out unless 0 <= idx < len and prio > 0 (what the reference's asserts let
        through)."""
        length = len(self)
        for i, p in zip(np.asarray(idx).tolist(), np.asarray(prio, np.float32).tolist()):
            if not (0 <= i < length and p > 0):
                continue
            self._set(i, self.leaf(p))
            self.max_priority = max(self.max_priority, p)

    def _range_sum(self, lo, hi, node, first, last):
        """Leaves lo .. hi under `node`, which covers first .. last: the halves of a straddling range are summed
        left + right, which fixes the association."""
        if lo == first and hi == last:
            return self.sum[node]
        mid = (first + last) // 2
        if hi <= mid:
            return self._range_sum(lo, hi, 2 * node, first, mid)
        if lo > mid:
            return self._range_sum(lo, hi, 2 * node + 1, mid + 1, last)
        left = self._range_sum(lo, mid, 2 * node, first, mid)
        return left + self._range_sum(mid + 1, hi, 2 * node + 1, mid + 1, last)

    def total(self, length):
        """The mass the draws are scaled by: the leaves 0 .. length - 2 (the reference's prefix ends one slot
        short). length >= 2."""
        return self._range_sum(0, length - 2, 1, 0, self.C - 1)

    def find(self, mass, length):
        """The prefix-sum descent, kept below length."""
        node = 1
        while node < self.C:
            left = self.sum[2 * node]
            if left > mass:
                node = 2 * node
            else:
                mass -= left
                node = 2 * node + 1
        return min(node - self.C, length - 1)

    def weight(self, idx, length, beta):
        root = self.sum[1]
        p_min, p_sample = self.min[1] / root, self.sum[self.C + idx] / root
        return np.float32(((p_sample * length) ** -beta) / ((p_min * length) ** -beta))

    def sample(self, batch, beta, seed, draw):
        """(idx [batch], weights [batch] fp32) of draw `draw`: the library's uniforms (pinned against the recorded
        ones by test_the_uniforms_are_the_recorded_ones) through find and weight."""
        length = len(self)
        total = self.total(length)
        idx = [self.find(P.uniform(b, draw, seed) * total, length) for b in range(batch)]
        return np.array(idx, np.int64), np.array([self.weight(i, length, beta) for i in idx], np.float32)


def assert_same_tree(tree, counter, model, what=""):
    """A library tree buffer (sum[2 C], min[2 C], max_priority, pad) and its counter against the model: every node
    1 .. 2 C - 1 of both trees and max_priority as fp64 bit patterns."""
    C = model.C
    tree = np.asarray(tree, np.float64)
    assert tree.size == 4 * C + 2 and int(counter) == model.counter, what
    for name, got, want in (("sum", tree[1:2 * C], model.sum[1:]), ("min", tree[2 * C + 1:4 * C], model.min[1:])):
        diff = np.flatnonzero(P.f64bits(got) != P.f64bits(np.array(want, np.float64)))
        assert diff.size == 0, f"{what}: {diff.size} {name} nodes differ from the model, first at {diff[:1] + 1}"
    assert P.f64bits(tree[4 * C:4 * C + 1])[0] == P.f64bits(np.array([model.max_priority]))[0], f"{what}: max_priority"


def scenario_stores(cap):
    """(n envs, T steps) of the stores, in order."""
    stores = ((1, 1), (cap // 2, 1), (cap // 3, 2),
              (cap, 1),  # exactly one ring from a non-zero position: two segments that cover every slot
              (cap - 1, 1),
              (cap + 3, 1),  # more than fits
              (2, 1), (cap // 2 + 1, 3))
    return tuple((max(n, 1), T) for n, T in stores)


def update_batch(rng, length, B):
    """(idx [B] int64, prio [B] fp32): indices drawn from -1 .. length, so both rejected ends are in; priorities
    log-uniform in [1e-3, 8] with every seventh one -1. From B = 33 on, slot v is named twice with positive
    priorities (the later one has to win) and slot w once with a positive priority and then, as the batch's last
    entry, with -1: the last valid entry wins, not the last entry. Slot x is named by two neighbouring entries,
    the nearest pair a scan for later duplicates can miss."""
    idx = rng.integers(-1, length + 1, B).astype(np.int64)
    prio = np.exp(rng.uniform(np.log(1e-3), np.log(8.0), B)).astype(np.float32)
    prio[6::7] = -1.0
    if B >= 33:
        v, w, x = (int(s) for s in rng.integers(0, length, 3))
        idx[[1, B - 2]], idx[[2, B - 1]], idx[[3, 4]] = v, w, x
        prio[B - 1] = -1.0
        assert (prio[[1, 2, 3, 4, B - 2]] > 0).all()  # none of them is a seventh
    return idx, prio


def tail_level(count):
    """The library's per_tail_level restated on its own constants, read from csrc/mg_per.h: the first level j >= 1
    whose launch bound (count >> j) + slack fits the single block of kPerTail threads. A store of `count` slots
    goes through tail_level(count) - 1 per-level launches before the single-block tail."""
    import os
    import re

    from merging_gym import build

    with open(os.path.join(os.path.dirname(build.SRC), "mg_per.h")) as f:
        text = f.read()
    slack = int(re.search(r"per_level_items\(int64_t count, int j\) \{ return \(count >> j\) \+ (\d+); \}", text).group(1))
    block = int(re.search(r"constexpr int kPerTail = (\d+);", text).group(1))
    j = 1
    while (count >> j) + slack > block:
        j += 1
    return j


class HostSubject:
    """per_ref.HostPer behind the calls run_scenario makes."""

    def __init__(self, cap, alpha):
        self.h = P.HostPer(cap, alpha)

    def store(self, tr):
        self.h.store(tr)

    def update(self, idx, prio):
        self.h.update(idx, prio)

    def sample(self, batch, beta, seed, draw):
        return self.h.sample(batch, beta, seed, draw)

    def state(self):
        return self.h.tree, int(self.h.counter[0])


def run_scenario(cap, alpha, subject, after=None):
    """The stores of scenario_stores through `subject` and the model. After each store the full tree; then per
    B of UPDATE_BATCHES one update and the full tree again, and a sample of 64 per beta: the indices the model's
    exactly, the weights within 1 fp32 step of the model's fp64 expression (the bar of the reference's recorded
    weights in test_alpha_one_fixture_rounds_on_the_device). With fewer than two transitions: slot 0, weight 1.
    after(what): the caller's own check of the subject after every store and update. At the end the leaves at and
    beyond the capacity are still 0.0 and +inf. Returns (model, the worst weight distance seen)."""
    model = PerModel(cap, alpha)
    rng = np.random.default_rng(cap)
    at = draw = worst = 0
    for r, (n, T) in enumerate(scenario_stores(cap)):
        subject.store(P.transitions(n, T, first=at))
        model.push(n * T)
        at += n * T
        what = f"capacity {cap}, store {r} ({n} x {T})"
        assert_same_tree(*subject.state(), model, what)
        if after:
            after(what)
        length = len(model)
        assert length == min(at, cap)
        for B in UPDATE_BATCHES:
            idx, prio = update_batch(rng, length, B)
            subject.update(idx, prio)
            model.update(idx, prio)
            assert_same_tree(*subject.state(), model, f"{what}, update of {B}")
            if after:
                after(f"{what}, update of {B}")
            for beta in SAMPLE_BETAS:
                got_idx, got_w = subject.sample(SAMPLE_BATCH, beta, SAMPLE_SEED, draw)
                if length >= 2:
                    want_idx, want_w = model.sample(SAMPLE_BATCH, beta, SAMPLE_SEED, draw)
                    assert np.array_equal(got_idx, want_idx), f"{what}, B {B}, beta {beta}: indices"
                    assert (got_w > 0).all() and (got_w <= 1).all(), f"{what}, B {B}, beta {beta}"
                    worst = max(worst, int(P.ulp32_distance(got_w, want_w).max()))
                else:
                    assert got_idx.tolist() == [0] * SAMPLE_BATCH and got_w.tolist() == [1.0] * SAMPLE_BATCH, what
                draw += 1
    assert model.max_priority > 1.0  # the updates raised it, so later stores wrote other leaves than the first
    tree, _ = subject.state()
    tree, C = np.asarray(tree, np.float64), model.C
    assert (tree[C + cap:2 * C] == 0.0).all() and np.isposinf(tree[3 * C + cap:4 * C]).all()
    return model, worst
