"""mg_host_rainbow_replay_store_many, the host twin of the member store (the functions the kernel compiles), against
a numpy restatement of the row rule include/merging_hip.h states at mg_rainbow_replay_store_many, and against the
rows mg_host_per_store writes from a contiguous copy of each member's slice.

M = 3 members on one [T, 3 n_member, ...] batch; the three rings start at counters 0, 3 and capacity - 1, prefilled
with a sentinel that every slot the rule does not name must keep. Capacity 7 is below T n_member for the wider
shapes (only the newest rows survive, the ring wraps), 1,000 is above all of them.
"""
import ctypes

import numpy as np
import pytest

import per_ref as P

M = 3
SENTINEL = np.float32(-7.0)
ROW = P.ROW


def _batch(n_member, T, use_flags, with_final):
    """One [T, N, ...] batch of random transitions, N = M n_member, with done and not-done steps in it."""
    N = M * n_member
    rng = np.random.default_rng(1000 * n_member + 10 * T + 2 * use_flags + with_final)
    tr = dict(obs_first=rng.standard_normal((N, 10)).astype(np.float32),
              obs=rng.standard_normal((T, N, 10)).astype(np.float32),
              final_obs=rng.standard_normal((T, N, 10)).astype(np.float32) if with_final else None,
              a1=rng.integers(0, 5, (T, N)).astype(np.int8),
              rew=rng.standard_normal((T, N, 2)).astype(np.float32),
              done=(rng.random((T, N)) < 0.4).astype(np.uint8))
    tr["done"].reshape(-1)[:2] = (1, 0)  # N >= 3: both kinds whatever the draw
    assert tr["done"].any() and not tr["done"].all()
    if use_flags:
        flags = np.zeros((T, N, 4), np.uint8)
        flags[..., 0], flags[..., 1], flags[..., 2], flags[..., 3] = tr["a1"].view(np.uint8), 9, tr["done"], 1
        tr = dict(tr, flags=flags)
    return tr


def _call_form(tr, use_flags):
    """What the call is given: the flags buffer in place of a1 / done, or the two arrays."""
    return dict(tr, a1=None, done=None) if use_flags else dict(tr, flags=None)


def _rule(ring, counter, tr, m, n_member, T):
    """The header's rule for member m on a copy of its ring: (ring, counter)."""
    ring = ring.copy()
    cap, total = len(ring), T * n_member
    for k in range(total):
        if total > cap and k < total - cap:
            continue
        t, j = divmod(k, n_member)
        c = m * n_member + j
        done = bool(tr["done"][t, c])
        row = np.zeros(ROW, np.float32)
        row[:10] = tr["obs_first"][c] if t == 0 else tr["obs"][t - 1, c]
        row[10], row[11] = tr["a1"][t, c], tr["rew"][t, c, 0]
        row[12:22] = tr["final_obs"][t, c] if done and tr["final_obs"] is not None else tr["obs"][t, c]
        row[22] = 1.0 if done else 0.0
        ring[(counter + k) % cap] = row
    return ring, counter + total


def _slice(tr, m, n_member):
    """A contiguous copy of member m's columns."""
    cols = slice(m * n_member, (m + 1) * n_member)
    cut = lambda a, axis: None if a is None else np.ascontiguousarray(a[cols] if axis == 0 else a[:, cols])  # noqa: E731
    return {k: cut(v, 0 if k == "obs_first" else 1) for k, v in tr.items()}


@pytest.mark.parametrize("with_final", (True, False), ids=("final_obs", "no_final_obs"))
@pytest.mark.parametrize("use_flags", (True, False), ids=("flags", "a1_done"))
@pytest.mark.parametrize("capacity", (7, 1000))
@pytest.mark.parametrize("T", (1, 4))
@pytest.mark.parametrize("n_member", (1, 5, 64))
def test_member_store_matches_the_rule_and_the_lone_store(n_member, T, capacity, use_flags, with_final):
    from merging_gym import _native

    full = _batch(n_member, T, use_flags, with_final)
    given = _call_form(full, use_flags)
    starts = (0, 3, capacity - 1)
    rings = [P.aligned(4 * ROW * capacity, np.float32).reshape(capacity, ROW) for _ in range(M)]
    counters = [np.array([c], np.uint64) for c in starts]
    for r in rings:
        r[:] = SENTINEL
    X = P.transitions_struct(_native, given)
    rows = (ctypes.c_void_p * M)(*(r.ctypes.data for r in rings))
    ctrs = (ctypes.c_void_p * M)(*(c.ctypes.data for c in counters))
    rc = _native.lib.mg_host_rainbow_replay_store_many(rows, ctrs, M, capacity, ctypes.byref(X), n_member, T)
    _native.check(rc, "mg_host_rainbow_replay_store_many")

    for m in range(M):
        start = np.full((capacity, ROW), SENTINEL, np.float32)
        want, want_counter = _rule(start, starts[m], full, m, n_member, T)
        # the rule names min(T n_member, capacity) slots (a row's last float is 0); every other keeps the sentinel
        assert (want[:, ROW - 1] == 0).sum() == min(T * n_member, capacity)
        assert (rings[m][:, ROW - 1] == SENTINEL).sum() == capacity - min(T * n_member, capacity)
        np.testing.assert_array_equal(rings[m], want, err_msg=f"member {m}: the header's rule")
        assert int(counters[m][0]) == starts[m] + T * n_member == want_counter

        lone = P.HostPer(capacity, 0.6)  # the prioritized store's host twin writes the lone store's rows
        lone.rows[:] = SENTINEL
        lone.counter[0] = starts[m]
        lone.store(_slice(given, m, n_member))
        np.testing.assert_array_equal(rings[m], lone.rows, err_msg=f"member {m}: mg_host_per_store on the slice")
        assert int(lone.counter[0]) == int(counters[m][0])
