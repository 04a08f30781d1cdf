"""The DQN nets at every accepted width (include/merging_hip.h: 1 <= in_dim <= 13, 1 <= out_dim <= 8): the
shapes, seeded nets and synthetic replay rows that tests/test_learn_widths_host.py, test_gpu_qnet_widths.py
and test_gpu_learn_widths.py share, and the plain-C restatement's runs of them (tests/learn_ref.py's
run_ref), each computed once."""

from __future__ import annotations

import functools

import numpy as np

import learn_many_ref as mr
import learn_ref as lr

# (in_dim, out_dim): the four corners; one inside each limit; the meta-net at num_goals 8 and 1 (mg_rollout_hdqn
# takes 1..8 goals and that is Goal_DQN's out_dim); 11 -> 2; an interior point
WIDTHS = [(1, 1), (1, 8), (13, 1), (13, 8), (12, 7), (10, 8), (10, 1), (11, 2), (5, 4)]

# (in_dim, out_dim, batch): every width at the smallest batches at which a tile can go wrong -- one row, one row
# past the 8-row tile of learn_l2_kernel and learn_l3_kernel, 33 -- and 128 once
LEARN_CASES = [(1, 1, 1), (1, 1, 9), (13, 8, 1), (13, 8, 9), (13, 8, 33), (12, 7, 33), (1, 8, 9), (13, 1, 9),
               (10, 8, 128), (10, 1, 33), (11, 2, 9), (5, 4, 33), (2, 2, 5)]
CAPACITY = 64
# the sequence of test_host_learn_equals_restatement_bit_for_bit: three updates from update 1 with target_period 2
# (the target copy falls inside the call), the target starting at half the eval net
SEQUENCE = dict(num_updates=3, first_update=1, seed=7, first_draw=5, target_period=2)


def width_net(in_dim, out_dim):
    """A seeded Net(in_dim, out_dim) of mixed signs: both ReLU branches are met."""
    return lr.seeded_net(in_dim, out_dim, 10 * in_dim + out_dim)


def width_rows(in_dim, out_dim, capacity, odd_actions):
    """[capacity, 2 in + 2] fp32 replay rows [s, a, r, s']: states uniform in [-1, 1), actions 0 .. out - 1,
    rewards uniform in [-2, 2). odd_actions: the action column of rows 0..3 holds what the reference's gather
    would raise on -- -1, out + 3, NaN, out - 0.5."""
    rng = np.random.default_rng(100 * in_dim + out_dim)
    rows = np.empty((capacity, 2 * in_dim + 2), dtype=np.float32)
    rows[:, :in_dim] = rng.uniform(-1.0, 1.0, (capacity, in_dim))
    rows[:, in_dim] = rng.integers(0, out_dim, capacity)
    rows[:, in_dim + 1] = rng.uniform(-2.0, 2.0, capacity)
    rows[:, in_dim + 2:] = rng.uniform(-1.0, 1.0, (capacity, in_dim))
    if odd_actions:
        rows[:4, in_dim] = (-1.0, out_dim + 3.0, np.nan, out_dim - 0.5)
    return rows


def clamped(rows, in_dim, out_dim):
    """A copy of `rows` whose action column holds what include/merging_hip.h says the learner uses: the column
    truncated to int (main.py:133's astype(int)), kept inside 0 .. out - 1, NaN as 0."""
    out = np.array(rows, dtype=np.float32, copy=True)
    for i, a in enumerate(rows[:, in_dim].tolist()):
        if a != a:  # NaN
            k = 0
        else:
            k = min(max(int(a), 0), out_dim - 1)  # int() truncates toward zero
        out[i, in_dim] = k
    return out


def start_learner(in_dim, out_dim):
    """[4, P]: eval from width_net, the target at half of it (so a missed copy shows), zero moments."""
    L0 = lr.learner_array(width_net(in_dim, out_dim))
    L0[1] *= np.float32(0.5)
    return L0


@functools.lru_cache(maxsize=None)
def reference(in_dim, out_dim, batch, filled_only):
    """The restatement's run of a LEARN_CASES entry on a half-filled 64-row ring with odd actions, shared by the
    host and the device tests: (state dict, ring, counter, start [4, P], (end, loss, rows, None))."""
    sd = width_net(in_dim, out_dim)
    ring, counter = lr.half_filled(width_rows(in_dim, out_dim, CAPACITY, True))
    L0 = start_learner(in_dim, out_dim)
    ref = lr.run_ref(L0, ring, counter, in_dim, out_dim, batch, filled_only=filled_only, **SEQUENCE)
    for a in (ring, L0, *ref[:3]):
        a.setflags(write=False)
    return sd, ring, counter, L0, ref


@functools.lru_cache(maxsize=None)
def members_setup(in_dim, out_dim, members):
    """A population at one width, as tests/learn_many_ref.py makes them: (state dict, rings, counters, member
    settings, start [M, 4, P]) -- every member its own roll of the odd-action rows, counter, seed and
    hyperparameters."""
    sd = width_net(in_dim, out_dim)
    rings, counters = mr.member_rings(width_rows(in_dim, out_dim, CAPACITY, True), members)
    kws = [mr.member_kw(m) for m in range(members)]
    L0 = mr.start_blocks(sd, members)
    for a in (L0, *rings):
        a.setflags(write=False)
    return sd, rings, counters, kws, L0


@functools.lru_cache(maxsize=None)
def member_reference(in_dim, out_dim, batch, members, m, filled_only, updates):
    """The restatement's run of member m of members_setup's population: (end [4, P], loss [U], rows [U, B, RF])."""
    _, rings, counters, kws, L0 = members_setup(in_dim, out_dim, members)
    return lr.run_ref(L0[m], rings[m], counters[m], in_dim, out_dim, batch, updates, filled_only=filled_only,
                      **kws[m])[:3]


def members_reference(in_dim, out_dim, batch, members, filled_only, updates, which=None):
    """member_reference of the members `which` (all by default) stacked as learn_many_ref.assert_members_equal
    takes them: end [len, 4, P], loss [U, len], rows [U, len, B, RF]."""
    refs = [member_reference(in_dim, out_dim, batch, members, m, filled_only, updates)
            for m in (range(members) if which is None else which)]
    return np.stack([r[0] for r in refs]), np.stack([r[1] for r in refs], axis=1), np.stack([r[2] for r in refs], axis=1)
