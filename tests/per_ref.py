"""Helpers of the prioritized replay's tests: the host twins (mg_host_per_*) on numpy memory, transitions to
store, and the fixture tests/golden/per_golden.npz (made by tests/golden/gen_per.py from the reference's own
PrioritizedReplayBuffer)."""

from __future__ import annotations

import ctypes
import functools
import os

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROW = 24
# (size, alpha): the fixture's scenarios -- 1.5 size + 1 pushes, then ROUNDS rounds of sample(BATCH, BETA) and
# update_priorities
SCENARIOS = ((6, 1.0), (13, 1.0), (13, 0.6), (3000, 0.6))
ROUNDS, BATCH, BETA = 40, 32, 0.4


def scenario_key(size, alpha):
    return f"n{size}_a{str(alpha).replace('.', 'p')}"


@functools.lru_cache(maxsize=1)
def golden():
    return np.load(os.path.join(HERE, "golden", "per_golden.npz"))


def aligned(nbytes, dtype, align=16):
    """A zeroed numpy array of nbytes bytes viewed as dtype, its first byte at a multiple of `align`."""
    raw = np.zeros(nbytes + align, dtype=np.uint8)
    off = -raw.ctypes.data % align
    return raw[off:off + nbytes].view(dtype)


def transitions(n, T, first=0):
    """Arrays of T steps of n envs, transition k = first + t n + i recognisable in its row: s = k everywhere,
    s' = k + 0.5 (from final_obs: every step is done), a = k % 5, r = k / 8."""
    k = first + np.arange(T * n, dtype=np.int64).reshape(T, n)
    s2 = np.repeat((k + 0.5).astype(np.float32)[:, :, None], 10, axis=2)
    s = np.repeat(k.astype(np.float32)[:, :, None], 10, axis=2)
    # store() takes s of step t > 0 from obs[t - 1]: give it final_obs as s' and obs as the next step's s
    obs = np.concatenate([s[1:], np.zeros((1, n, 10), np.float32)], axis=0)
    return dict(obs_first=np.ascontiguousarray(s[0]), obs=np.ascontiguousarray(obs), final_obs=np.ascontiguousarray(s2),
                a1=(k % 5).astype(np.int8), rew=np.ascontiguousarray(np.stack([k / 8.0, 0 * k], axis=2).astype(np.float32)),
                done=np.ones((T, n), np.uint8))


def expected_row(k):
    """The row transitions() gives transition k (done everywhere, so s' comes from final_obs)."""
    row = np.zeros(ROW, np.float32)
    row[:10], row[10], row[11], row[12:22], row[22] = k, k % 5, k / 8.0, k + 0.5, 1.0
    return row


STORE_CAP, STORE_FIRST = 13, 3


def store_case(use_flags):
    """n = 5 envs x T = 4 steps for a ring of STORE_CAP that holds STORE_FIRST rows: 20 transitions, so the oldest
    are skipped, the ring wraps and every slot is written. Two steps in three are done (s' from final_obs), the
    others take s' from obs. With use_flags the action and done travel as a rollout's [T, N, 4] bytes in place of
    a1 / done."""
    tr = transitions(5, 4, first=STORE_FIRST)
    k = STORE_FIRST + np.arange(20).reshape(4, 5)
    tr["done"] = (k % 3 != 0).astype(np.uint8)
    if use_flags:
        flags = np.zeros((4, 5, 4), np.uint8)
        flags[..., 0], flags[..., 1], flags[..., 2] = tr["a1"].view(np.uint8), 9, tr["done"]
        tr = dict(tr, flags=flags, a1=None, done=None)
    return tr


def pushed(ring, counter, tr):
    """Sequential replay_buffer.push calls of tr (with a1 and done) in (step, env) order on a copy of a numpy
    ring: (ring, counter)."""
    ring = ring.copy()
    T, n = tr["a1"].shape
    for t in range(T):
        for i in range(n):
            row = np.zeros(ROW, np.float32)
            row[:10] = tr["obs_first"][i] if t == 0 else tr["obs"][t - 1, i]
            row[10], row[11], row[22] = tr["a1"][t, i], tr["rew"][t, i, 0], tr["done"][t, i]
            row[12:22] = tr["final_obs"][t, i] if tr["done"][t, i] else tr["obs"][t, i]
            ring[counter % len(ring)] = row
            counter += 1
    return ring, counter


def learn_case(size, alpha):
    """A wrapped HostPer with recorded observations as rows and a tree 10 rounds of updates have shaped."""
    import rainbow_learn_ref as R

    h = HostPer(size, alpha)
    h.push_many(size + size // 2 + 1, n=min(size, 500))
    h.rows[:] = R.replay_rows(size)
    for r in range(10):
        idx, _ = h.sample(BATCH, BETA, 1, r)
        h.update(idx, np.exp(np.random.default_rng(r).uniform(np.log(1e-3), np.log(8.0), BATCH)).astype(np.float32))
    return h


def transitions_struct(nat, tr, pointer=lambda a: a.ctypes.data):
    p = lambda name: None if tr.get(name) is None else pointer(tr[name])  # noqa: E731
    return nat.Transitions(p("obs_first"), p("obs"), p("final_obs"), p("a1"), p("rew"), p("done"), None, None, None,
                           None, p("flags"), None)


class HostPer:
    """PrioritizedReplayBuffer(capacity, alpha) on host memory through the host twins."""

    def __init__(self, capacity, alpha):
        from merging_gym import _native

        self.nat, self.lib = _native, _native.lib
        self.capacity, self.alpha = int(capacity), float(alpha)
        self.C = 1
        while self.C < capacity:
            self.C *= 2
        self.nbytes = int(self.lib.mg_per_bytes(self.capacity))
        assert self.nbytes == 8 * (4 * self.C + 2)
        self.tree = aligned(self.nbytes, np.float64)
        self.rows = aligned(4 * ROW * self.capacity, np.float32).reshape(self.capacity, ROW)
        self.counter = np.zeros(1, np.uint64)
        self.check(self.lib.mg_host_per_init(self.tree.ctypes.data, self.nbytes, self.capacity), "mg_host_per_init")

    def check(self, rc, what):
        self.nat.check(rc, what)

    sum = property(lambda self: self.tree[:2 * self.C])
    min = property(lambda self: self.tree[2 * self.C:4 * self.C])
    max_priority = property(lambda self: self.tree[4 * self.C])

    def __len__(self):
        return min(int(self.counter[0]), self.capacity)

    def clone(self):
        other = HostPer(self.capacity, self.alpha)
        other.tree[:], other.rows[:], other.counter[:] = self.tree, self.rows, self.counter
        return other

    def store(self, tr):
        T, n = tr["rew"].shape[:2]
        X = transitions_struct(self.nat, tr)
        self.check(self.lib.mg_host_per_store(self.rows.ctypes.data, self.counter.ctypes.data, self.capacity,
                                              ctypes.byref(X), n, T, self.tree.ctypes.data, self.nbytes, self.alpha),
                   "mg_host_per_store")

    def push_many(self, count, n=1):
        """`count` transitions in stores of n envs x 1 step (the last one narrower)."""
        at = int(self.counter[0])
        while count > 0:
            m = min(n, count)
            self.store(transitions(m, 1, first=at))
            at, count = at + m, count - m

    def sample(self, batch, beta, seed=0, draw=0):
        idx, w = np.full(batch, -7, np.int64), np.full(batch, np.nan, np.float32)
        self.check(self.lib.mg_host_per_sample(self.tree.ctypes.data, self.nbytes, self.counter.ctypes.data, self.capacity,
                                               beta, seed, draw, batch, idx.ctypes.data, w.ctypes.data),
                   "mg_host_per_sample")
        return idx, w

    def update(self, idx, priority):
        idx = np.ascontiguousarray(idx, np.int64)
        priority = np.ascontiguousarray(priority, np.float32)
        self.check(self.lib.mg_host_per_update(self.tree.ctypes.data, self.nbytes, self.counter.ctypes.data, self.capacity,
                                               self.alpha, idx.ctypes.data, priority.ctypes.data, len(idx)),
                   "mg_host_per_update")

    def total(self):
        out = np.zeros(1, np.float64)
        self.check(self.lib.mg_host_per_total(self.tree.ctypes.data, self.nbytes, self.counter.ctypes.data, self.capacity,
                                              out.ctypes.data), "mg_host_per_total")
        return out[0]


def uniform(b, draw, seed):
    from merging_gym import _native

    return float(_native.lib.mg_host_per_uniform(b, draw, seed))


def host_pow(x, y):
    from merging_gym import _native

    x, y = np.ascontiguousarray(x, np.float64), np.ascontiguousarray(y, np.float64)
    out = np.empty_like(x)
    _native.check(_native.lib.mg_host_per_pow(x.ctypes.data, y.ctypes.data, out.ctypes.data, x.size), "mg_host_per_pow")
    return out


def f64bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def ulp32_distance(a, b):
    """|a - b| in fp32 steps, for positive finite fp32 arrays."""
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


def run_host_prioritized(L, per, B, U, beta, prio_eps, first_update=0, seed=0, first_draw=0, noise_f=None):
    """mg_host_rainbow_learn_prioritized on a copy of L and on `per` (a HostPer, whose tree it updates): (L,
    loss [U], rows [U, B, 24], proj [U, B, 51], grads [U, P], idx [U, B], weights [U, B])."""
    import rainbow_learn_ref as R

    nat = per.nat
    L = np.array(L, dtype=np.float32, copy=True)
    nf = np.ascontiguousarray(noise_f, dtype=np.float32)
    assert nf.shape == (U, 2, R.NF)
    loss, rows, proj, grads = R._outs(U, B)
    idx, w = np.full((U, B), -7, np.int64), np.full((U, B), np.nan, np.float32)
    nbytes = int(nat.lib.mg_rainbow_learn_prioritized_scratch_bytes(B))
    scratch = aligned(nbytes, np.float32)
    Lp = aligned(4 * L.size, np.float32)
    Lp[:] = L
    h = R.HYPER
    hs = nat.DqnHyper(h["lr"], h["gamma"], h["beta1"], h["beta2"], h["eps"], 1, 0)
    rc = nat.lib.mg_host_rainbow_learn_prioritized(
        Lp.ctypes.data, per.rows.ctypes.data, per.counter.ctypes.data, per.capacity, B, U, first_update, seed, first_draw,
        ctypes.byref(hs), nf.ctypes.data, loss.ctypes.data, rows.ctypes.data, proj.ctypes.data, grads.ctypes.data,
        scratch.ctypes.data, nbytes, per.tree.ctypes.data, per.nbytes, per.alpha, beta, prio_eps, idx.ctypes.data,
        w.ctypes.data)
    nat.check(rc, "mg_host_rainbow_learn_prioritized")
    return Lp.copy(), loss, rows, proj, grads, idx, w
