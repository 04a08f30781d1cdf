"""Prioritized replay on the host (CPU): the host twins mg_host_per_* -- the functions the kernels compile --
against tests/golden/per_golden.npz, the recorded behaviour of the reference's own PrioritizedReplayBuffer
(tests/golden/gen_per.py). alpha = 1: every node of both trees, max_priority, S and the indices bit for bit
after every round. alpha = 0.6: the indices, and the leaves within the bound of the library's pow. The weights
within one fp32 step of the reference's."""
import ctypes
import math

import numpy as np
import pytest

import per_ref as P

# max relative error of mg_host_per_pow against libm pow over x on a 200,001-point log grid in [1e-5, 10] and
# y in POW_YS, measured 2026-10-20: 1.03e-15 (9.3 x 2^-53, at y = 0.7). The bound is 4 x that, for the grid's
# gaps, and has to stay below 2^-26: two such errors in the weights' quotient then stay below 2^-24, so the
# fp32 rounding moves by at most one step.
POW_MEASURED = 1.03e-15
POW_BOUND = 4 * POW_MEASURED
POW_YS = (0.4, 0.5, 0.6, 0.7, 1.0, -0.4, -0.6, -1.0)
assert POW_BOUND < 2.0 ** -26


def replay(size, alpha):
    """The scenario through the host twins: yields (round, host, S, idx, w) after the round's update."""
    g, key = P.golden(), P.scenario_key(size, alpha)
    h = P.HostPer(size, alpha)
    h.push_many(size + size // 2 + 1, n=7)  # stores of seven transitions: the ring wraps inside a store
    assert len(h) == int(g[key + "/len"]) == size
    seed = int(g[key + "/seed"])
    for r in range(P.ROUNDS):
        S = h.total()
        idx, w = h.sample(P.BATCH, P.BETA, seed, r)
        h.update(idx, g[key + "/prio"][r])
        yield r, h, S, idx, w


def test_the_uniforms_are_the_recorded_ones():
    g = P.golden()
    for size, alpha in P.SCENARIOS:
        key = P.scenario_key(size, alpha)
        u = np.array([[P.uniform(b, r, int(g[key + "/seed"])) for b in range(P.BATCH)] for r in range(P.ROUNDS)])
        assert np.array_equal(P.f64bits(u), P.f64bits(g[key + "/u"]))
        assert (u >= 0).all() and (u < 1).all() and len(np.unique(u)) == u.size


@pytest.mark.parametrize("size", (6, 13))
def test_alpha_one_equals_the_reference_bit_for_bit(size):
    g, key = P.golden(), P.scenario_key(size, 1.0)
    for r, h, S, idx, w in replay(size, 1.0):
        assert P.f64bits(S) == P.f64bits(g[key + "/S"][r]), r
        assert np.array_equal(idx, g[key + "/idx"][r]), r
        assert np.array_equal(P.f64bits(h.sum[1:]), P.f64bits(g[key + "/sum"][r][1:])), r  # node 0 is unused
        assert np.array_equal(P.f64bits(h.min[1:]), P.f64bits(g[key + "/min"][r][1:])), r
        assert P.f64bits(h.max_priority) == P.f64bits(g[key + "/maxp"][r]), r
        assert P.ulp32_distance(w, g[key + "/w"][r].astype(np.float32)).max() <= 1, r


@pytest.mark.parametrize("size", (13, 3000))
def test_alpha_06_indices_equal_and_leaves_within_the_pow_bound(size):
    g, key = P.golden(), P.scenario_key(size, 0.6)
    worst = 0.0
    for r, h, S, idx, w in replay(size, 0.6):
        assert np.array_equal(idx, g[key + "/idx"][r]), r
        want = g[key + "/leaf_at_idx"][r]
        worst = max(worst, float(np.max(np.abs(h.sum[h.C + idx] - want) / want)))
        assert abs(S - g[key + "/S"][r]) <= 2 * POW_BOUND * g[key + "/S"][r], r  # a sum of positive leaves
        assert P.f64bits(h.max_priority) == P.f64bits(g[key + "/maxp"][r]), r
        assert P.ulp32_distance(w, g[key + "/w"][r].astype(np.float32)).max() <= 1, r
        assert np.array_equal(P.f64bits(h.sum[h.C:h.C + size]), P.f64bits(h.min[h.C:h.C + size])), r
    for name, tree in (("final_sum_leaves", h.sum), ("final_min_leaves", h.min)):
        want, got = g[f"{key}/{name}"][:size], tree[h.C:h.C + size]
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
    print(f"size {size}: leaves' max relative error {worst:.3g} (bound {POW_BOUND:.3g})")
    assert worst <= POW_BOUND
    # the tree is a pure function of its leaves
    assert all(h.sum[i] == h.sum[2 * i] + h.sum[2 * i + 1] and h.min[i] == min(h.min[2 * i], h.min[2 * i + 1])
               for i in range(1, h.C))


def test_pow_error_against_libm():
    xs = np.exp(np.linspace(math.log(1e-5), math.log(10.0), 200001))
    worst = 0.0
    for y in POW_YS:
        got = P.host_pow(xs, np.full_like(xs, y))
        want = np.array([math.pow(float(x), y) for x in xs])
        worst = max(worst, float(np.max(np.abs(got - want) / want)))
    g = P.golden()
    for size, alpha in P.SCENARIOS:  # the fixture's own arguments
        p = g[P.scenario_key(size, alpha) + "/prio"].astype(np.float64).ravel()
        for y in (0.6, -P.BETA):
            want = np.array([math.pow(float(x), y) for x in p])
            worst = max(worst, float(np.max(np.abs(P.host_pow(p, np.full_like(p, y)) - want) / want)))
    print(f"per_pow: max relative error {worst:.3g} = {worst / 2.0 ** -53:.2f} x 2^-53 (bound {POW_BOUND:.3g})")
    assert worst <= POW_BOUND
    assert P.host_pow([1.0, 1.0, 2.0], [0.6, -0.4, 1.0]).tolist() == [1.0, 1.0, 2.0]
    assert np.isnan(P.host_pow([0.0, -1.0, np.nan, np.inf, 1e-310], [0.6] * 5)).all()


@pytest.mark.parametrize("size,alpha", ((6, 1.0), (13, 0.6), (3000, 0.6)))
def test_fresh_buffer_weights_are_one_and_newest_slot_is_never_drawn(size, alpha):
    h = P.HostPer(size, alpha)
    h.push_many(size - 2, n=5)  # partly filled: len = size - 2, the newest slot size - 3
    seen = set()
    for draw in range(40):
        idx, w = h.sample(P.BATCH, P.BETA, 3, draw)
        assert (w == 1.0).all()
        seen.update(idx.tolist())
    assert max(seen) <= len(h) - 2 and min(seen) == 0
    h.push_many(size, n=3)  # wrapped: the newest slot is (counter - 1) % size, yet the prefix ends at len - 2
    for draw in range(40):
        idx, w = h.sample(P.BATCH, P.BETA, 3, draw)
        assert (w == 1.0).all() and idx.max() <= size - 2


@pytest.mark.parametrize("pushes", (0, 1))
def test_fewer_than_two_transitions_draw_slot_zero_with_weight_one(pushes):
    h = P.HostPer(13, 0.6)
    h.push_many(pushes)
    idx, w = h.sample(5, 0.4)
    assert idx.tolist() == [0] * 5 and w.tolist() == [1.0] * 5


def test_duplicate_index_the_last_one_wins_and_rejected_entries_are_left_out():
    h = P.HostPer(13, 1.0)
    h.push_many(13)
    before = h.tree.copy()
    h.update([4, 9, 4, 4], [0.5, 3.0, 7.0, 0.25])
    assert h.sum[h.C + 4] == h.min[h.C + 4] == 0.25 and h.sum[h.C + 9] == 3.0 and h.max_priority == 7.0
    leaves = before[h.C:2 * h.C].copy()
    leaves[4], leaves[9] = 0.25, 3.0
    assert h.sum[1] == ((leaves[0:2].sum() + leaves[2:4].sum()) + (leaves[4:6].sum() + leaves[6:8].sum())) + (
        (leaves[8:10].sum() + leaves[10:12].sum()) + (leaves[12:14].sum() + leaves[14:16].sum()))
    assert h.min[1] == 0.25
    now = h.tree.copy()
    h.update([2, -1, 13, 5, 6], [0.0, 1.0, 1.0, -2.0, np.nan])  # priority <= 0, idx outside 0 .. len - 1, NaN
    assert np.array_equal(P.f64bits(h.tree), P.f64bits(now))


def test_store_larger_than_the_ring_keeps_the_newest_and_rebuilds_every_node():
    h = P.HostPer(3000, 0.6)
    h.push_many(10, n=10)
    h.update(np.arange(9), np.linspace(0.5, 4.0, 9).astype(np.float32))
    h.store(P.transitions(1000, 4, first=10))  # 4,000 transitions into 3,000 slots, from position 10
    assert int(h.counter[0]) == 4010
    for k in (1010, 2999, 3000, 4009):
        assert np.array_equal(h.rows[k % 3000], P.expected_row(k)), k
    v = P.host_pow([4.0], [0.6])[0]  # max_priority ** alpha
    assert (h.sum[h.C:h.C + 3000] == v).all() and (h.min[h.C:h.C + 3000] == v).all()
    assert (h.sum[h.C + 3000:] == 0.0).all() and np.isinf(h.min[h.C + 3000:]).all()
    assert all(h.sum[i] == h.sum[2 * i] + h.sum[2 * i + 1] and h.min[i] == min(h.min[2 * i], h.min[2 * i + 1])
               for i in range(1, h.C))


@pytest.mark.parametrize("use_flags", (False, True), ids=("a1-done", "flags"))
def test_host_store_equals_sequential_pushes(use_flags):
    """P.store_case (the device stores' test runs it too): 20 transitions into the ring of 13 from position 3,
    the action and done from a1 / done or from a rollout's flags."""
    h = P.HostPer(P.STORE_CAP, 0.6)
    first = P.transitions(P.STORE_FIRST, 1)
    h.store(first)
    h.store(P.store_case(use_flags))
    want, counter = P.pushed(*P.pushed(np.zeros((P.STORE_CAP, P.ROW), np.float32), 0, first), P.store_case(False))
    assert int(h.counter[0]) == counter == P.STORE_FIRST + 20
    assert np.array_equal(h.rows.view(np.uint32), want.view(np.uint32))
    assert set(want[:, 22].tolist()) == {0.0, 1.0}  # both sources of s'
    v = h.sum[h.C]  # max_priority ** alpha of the fresh tree, in every written leaf
    assert v == 1.0 and (h.sum[h.C:h.C + P.STORE_CAP] == v).all() and (h.min[h.C:h.C + P.STORE_CAP] == v).all()


def test_tree_round_trip_continues_bit_for_bit():
    """What PrioritizedRainbowReplay.state_dict carries: the rows, the counter and the tree buffer."""
    runs = []
    for resume_at in (None, 17):
        out = []
        for r, h, S, idx, w in replay(13, 0.6):
            out.append((idx.copy(), w.copy()))
            if r == resume_at:
                saved = (h.tree.copy(), h.rows.copy(), h.counter.copy())
                h.tree[:] = np.nan
                h.rows[:] = 0
                h.counter[:] = 0
                h.tree[:], h.rows[:], h.counter[:] = saved
        runs.append((out, h.tree.copy()))
    assert all(np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) for a, b in zip(*[r[0] for r in runs]))
    assert np.array_equal(P.f64bits(runs[0][1]), P.f64bits(runs[1][1]))


def _refusals():
    from merging_gym import _native

    lib = _native.lib
    h = P.HostPer(13, 0.6)
    tr = P.transitions(4, 2)
    X = P.transitions_struct(_native, tr)
    t, nb, c, rows = h.tree.ctypes.data, h.nbytes, h.counter.ctypes.data, h.rows.ctypes.data
    idx, w, pr = np.zeros(8, np.int64), np.zeros(8, np.float32), np.ones(8, np.float32)
    i, wp, pp = idx.ctypes.data, w.ctypes.data, pr.ctypes.data
    ref = ctypes.byref
    cases = []
    for pre, dev in (("mg_per_", (None,)), ("mg_host_per_", ())):
        init, store = getattr(lib, pre + "init"), getattr(lib, pre + "store")
        sample, update = getattr(lib, pre + "sample"), getattr(lib, pre + "update")
        cases += [
            (pre + "init: NULL pointer", lambda dev=dev, f=init: f(None, nb, 13, *dev)),
            (pre + "init: need 1 <= capacity <= 2^32", lambda dev=dev, f=init: f(t, nb, 0, *dev)),
            (pre + "init: the tree buffer must be 16-byte aligned", lambda dev=dev, f=init: f(t + 8, nb, 13, *dev)),
            (pre + "init: tree buffer smaller than mg_per_bytes(capacity)", lambda dev=dev, f=init: f(t, nb - 1, 13, *dev)),
            (pre + "store: NULL pointer", lambda dev=dev, f=store: f(None, c, 13, ref(X), 4, 2, t, nb, 0.6, *dev)),
            (pre + "store: NULL pointer", lambda dev=dev, f=store: f(rows, c, 13, ref(X), 4, 2, None, nb, 0.6, *dev)),
            (pre + "store: n < 0 or num_steps < 0", lambda dev=dev, f=store: f(rows, c, 13, ref(X), -4, 2, t, nb, 0.6, *dev)),
            (pre + "store: the tree buffer must be 16-byte aligned",
             lambda dev=dev, f=store: f(rows, c, 13, ref(X), 4, 2, t + 8, nb, 0.6, *dev)),
            (pre + "store: tree buffer smaller than mg_per_bytes(capacity)",
             lambda dev=dev, f=store: f(rows, c, 13, ref(X), 4, 2, t, nb - 8, 0.6, *dev)),
            (pre + "store: need alpha > 0", lambda dev=dev, f=store: f(rows, c, 13, ref(X), 4, 2, t, nb, 0.0, *dev)),
            (pre + "store: need alpha > 0", lambda dev=dev, f=store: f(rows, c, 13, ref(X), 4, 2, t, nb, float("nan"), *dev)),
            (pre + "sample: NULL pointer", lambda dev=dev, f=sample: f(None, nb, c, 13, 0.4, 0, 0, 8, i, wp, *dev)),
            (pre + "sample: NULL pointer", lambda dev=dev, f=sample: f(t, nb, None, 13, 0.4, 0, 0, 8, i, wp, *dev)),
            (pre + "sample: NULL pointer", lambda dev=dev, f=sample: f(t, nb, c, 13, 0.4, 0, 0, 8, None, wp, *dev)),
            (pre + "sample: NULL pointer", lambda dev=dev, f=sample: f(t, nb, c, 13, 0.4, 0, 0, 8, i, None, *dev)),
            (pre + "sample: need beta > 0", lambda dev=dev, f=sample: f(t, nb, c, 13, 0.0, 0, 0, 8, i, wp, *dev)),
            (pre + "sample: need beta > 0", lambda dev=dev, f=sample: f(t, nb, c, 13, -0.4, 0, 0, 8, i, wp, *dev)),
            (pre + "sample: need 1 <= batch <= 1024", lambda dev=dev, f=sample: f(t, nb, c, 13, 0.4, 0, 0, 0, i, wp, *dev)),
            (pre + "sample: need 1 <= batch <= 1024", lambda dev=dev, f=sample: f(t, nb, c, 13, 0.4, 0, 0, 1025, i, wp, *dev)),
            (pre + "sample: tree buffer smaller than mg_per_bytes(capacity)",
             lambda dev=dev, f=sample: f(t, nb, c, 17, 0.4, 0, 0, 8, i, wp, *dev)),
            (pre + "sample: the tree buffer must be 16-byte aligned",
             lambda dev=dev, f=sample: f(t + 8, nb, c, 13, 0.4, 0, 0, 8, i, wp, *dev)),
            (pre + "sample: counter and idx_out must be 8-byte, weight_out 4-byte aligned",
             lambda dev=dev, f=sample: f(t, nb, c, 13, 0.4, 0, 0, 8, i + 4, wp, *dev)),
            (pre + "sample: counter and idx_out must be 8-byte, weight_out 4-byte aligned",
             lambda dev=dev, f=sample: f(t, nb, c, 13, 0.4, 0, 0, 8, i, wp + 2, *dev)),
            (pre + "update: NULL pointer", lambda dev=dev, f=update: f(None, nb, c, 13, 0.6, i, pp, 8, *dev)),
            (pre + "update: NULL pointer", lambda dev=dev, f=update: f(t, nb, c, 13, 0.6, None, pp, 8, *dev)),
            (pre + "update: NULL pointer", lambda dev=dev, f=update: f(t, nb, c, 13, 0.6, i, None, 8, *dev)),
            (pre + "update: need alpha > 0", lambda dev=dev, f=update: f(t, nb, c, 13, -1.0, i, pp, 8, *dev)),
            (pre + "update: need 1 <= batch <= 1024", lambda dev=dev, f=update: f(t, nb, c, 13, 0.6, i, pp, 0, *dev)),
            (pre + "update: need 1 <= batch <= 1024", lambda dev=dev, f=update: f(t, nb, c, 13, 0.6, i, pp, 1025, *dev)),
            (pre + "update: need 1 <= capacity <= 2^32", lambda dev=dev, f=update: f(t, nb, c, 2 ** 32 + 1, 0.6, i, pp, 8, *dev)),
            (pre + "update: tree buffer smaller than mg_per_bytes(capacity)",
             lambda dev=dev, f=update: f(t, 64, c, 13, 0.6, i, pp, 8, *dev)),
            (pre + "update: counter and idx must be 8-byte, priority 4-byte aligned",
             lambda dev=dev, f=update: f(t, nb, c + 4, 13, 0.6, i, pp, 8, *dev)),
        ]
    return h, (tr, X, idx, w, pr), cases


def test_every_refusal_text():
    """The device entry points refuse before anything is launched, so they are checked here too."""
    from merging_gym import _native

    h, keep, cases = _refusals()
    before = h.tree.copy()
    for text, call in cases:
        assert call() != 0, text
        assert _native.lib.mg_last_error().decode() == text
    assert np.array_equal(P.f64bits(h.tree), P.f64bits(before)) and int(h.counter[0]) == 0
    assert _native.lib.mg_per_bytes(0) == 0 and _native.lib.mg_per_bytes(2 ** 32 + 1) == 0
    assert _native.lib.mg_per_bytes(1) == 8 * 6 and _native.lib.mg_per_bytes(3000) == 8 * (4 * 4096 + 2)
