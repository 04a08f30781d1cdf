"""The prioritized population's host twins without a GPU: mg_host_rainbow_learn_prioritized_many against
mg_host_rainbow_learn_prioritized run once per member, and mg_host_per_store_many against mg_host_per_store per
member, bit for bit, with members that differ in every field and stand at different counters; the members'
isolation; the refusals with the member named, which change nothing."""

import ctypes

import numpy as np
import pytest

import per_many_ref as pm
import per_model
import per_ref as P
import rainbow_learn_many_ref as many
from learn_ref import bits

U, CAP = 3, 13
CASES = [(32, 1), (33, 3), (8, 64)]  # (batch, members); 33 > 13: every update repeats indices


@pytest.fixture(scope="module")
def runs():
    """Per case, computed once: (settings, replays, the many twin's outputs, the lone twin's per member)."""
    cache = {}

    def get(B, M):
        if (B, M) not in cache:
            settings = pm.member_settings(M)
            pers, L, nf = pm.replays(settings, CAP), many.learners(M), many.noise(U, M)
            cache[B, M] = (settings, pers, pm.run_host_many(L, settings, pers, B, U, nf),
                           pm.run_lone(L, settings, pers, B, U, nf))
        return cache[B, M]

    return get


@pytest.mark.parametrize("B,M", CASES)
def test_every_member_equals_the_lone_host_learner(runs, B, M):
    settings, pers, got, want = runs(B, M)
    pm.assert_members_same(got, want)
    for m, (s, e) in enumerate(zip(settings, got[8])):
        assert (int(e.first_update), int(e.first_draw)) == (s["first_update"] + U, s["first_draw"] + U)
        assert got[7][m].counter[0] == pers[m].counter[0]  # learning moves no ring
        assert (P.f64bits(got[7][m].tree) != P.f64bits(pers[m].tree)).any()  # the priorities moved


def test_the_members_differ(runs):
    """Not M copies: no two members draw the same slots, weigh them alike or end with the same model."""
    _, _, got, _ = runs(33, 3)
    for a in range(3):
        for b in range(a + 1, 3):
            assert (bits(got[0][a]) != bits(got[0][b])).any()
            assert (got[5][:, a] != got[5][:, b]).any() and (bits(got[6][:, a]) != bits(got[6][:, b])).any()
    assert (got[6] > 0).all() and (got[6] <= 1).all() and len(np.unique(got[6])) > 3


def test_k_updates_in_one_call_equal_k_calls(runs):
    settings, pers, got, _ = runs(33, 3)
    again = pm.run_host_many(many.learners(3), settings, pers, 33, U, many.noise(U, 3), calls=[1, 0, 2])
    pm.assert_members_same(again, got)
    assert [int(e.first_update) for e in again[8]] == [int(e.first_update) for e in got[8]]


@pytest.mark.parametrize("what", ["tree", "seed"])
def test_a_member_touches_no_other_member(runs, what):
    """Member 0's tree (one more priority update) or seed changed: every other member's outputs, tree and model keep
    their bits, and member 0's own move (member 0 is a "soft" net: a "default" one's gradient can be exactly zero)."""
    settings, pers, got, _ = runs(33, 3)
    settings = [dict(s) for s in settings]
    pers = [h.clone() for h in pers]
    if what == "tree":
        pers[0].update(np.arange(4), np.array([7.5, 0.02, 3.0, 0.4], np.float32))
    else:
        settings[0]["seed"] += 1
    other = pm.run_host_many(many.learners(3), settings, pers, 33, U, many.noise(U, 3))
    pm.assert_members_same(other, got, members=[1, 2])
    assert (other[5][:, 0] != got[5][:, 0]).any() and (bits(other[0][0]) != bits(got[0][0])).any()


def test_one_population_of_edge_members():
    """The members test_gpu_per_many.py mixes, here against the lone host learner: 0 and 1 stored transitions (slot
    0 with weight 1), a wrapped one, and one whose every row is done with a reward clamped onto the last atom, so
    loss_b is exactly 0 and, with prio_eps 0, every priority is refused and the tree is left as it was."""
    settings = pm.member_settings(4)
    settings[3]["prio_eps"] = 0.0
    pers = pm.replays(settings, CAP, counts=[0, 1, 3 * CAP + 2, CAP + 4])
    pers[3].rows[:, 22], pers[3].rows[:, 11] = 1.0, 25.0
    L, nf = many.learners(4), many.noise(U, 4)
    got = pm.run_host_many(L, settings, pers, 33, U, nf)
    pm.assert_members_same(got, pm.run_lone(L, settings, pers, 33, U, nf))
    for m in (0, 1):
        assert (got[5][:, m] == 0).all() and (got[6][:, m] == 1.0).all()
    assert (got[5][:, 2] != 0).any() and len(np.unique(got[6][:, 2])) > 1
    assert (got[1][:, 3] == 0.0).all() and (got[5][:, 3] != 0).any()
    assert (P.f64bits(got[7][3].tree) == P.f64bits(pers[3].tree)).all()
    assert (P.f64bits(got[7][2].tree) != P.f64bits(pers[2].tree)).any()


# ---------------------------------------------------------------------------- the store
@pytest.mark.parametrize("cap", [1, 13, 1025, 5000])
def test_store_many_equals_the_lone_store_per_member(cap):
    """per_model.scenario_stores through mg_host_per_store_many (three members from different counters, alphas 1.0 /
    0.6 in turn, one batch with the rollout's flags) and through mg_host_per_store member by member."""
    from merging_gym import _native as nat

    M = 3
    settings = pm.member_settings(M)
    start = pm.store_counters(M)
    got, want = ([P.HostPer(cap, s["alpha"]) for s in settings] for _ in range(2))
    for hs in (got, want):
        for h, c in zip(hs, start):
            h.push_many(c, n=max(1, min(c, cap)))
    at = list(start)
    for r, (n, T) in enumerate(per_model.scenario_stores(cap)):
        batch, parts = pm.store_batch(n, T, M, at)
        nat.check(pm.store_many(nat.lib.mg_host_per_store_many, nat, got, batch, n, T), "mg_host_per_store_many")
        for m in range(M):
            want[m].store(parts[m])
            at[m] += n * T
            assert got[m].counter[0] == want[m].counter[0] == at[m], (r, m)
            assert (P.f64bits(got[m].tree) == P.f64bits(want[m].tree)).all(), f"store {r} ({n} x {T}), member {m}: tree"
            assert (bits(got[m].rows) == bits(want[m].rows)).all(), f"store {r} ({n} x {T}), member {m}: rows"
        if r == 3:  # raise one member's max_priority, so its later leaves differ from the others'
            for hs in (got, want):
                hs[1].update(np.array([0]), np.array([5.0], np.float32))
    assert len({h.counter[0] % cap for h in got}) == min(M, cap)  # the members' segments differed to the end
    if cap > 1:
        assert (P.f64bits(got[0].tree) != P.f64bits(got[1].tree)).any()


# ---------------------------------------------------------------------------- refusals
def _learn_args(B=8, M=2, U=1):
    """A valid call's pieces: (settings, HostPers, the learner block, noise, scratch, nbytes)."""
    from merging_gym import _native as nat

    settings = pm.member_settings(M)
    hs = pm.replays(settings, CAP, rounds=1)
    nbytes = M * int(nat.lib.mg_rainbow_learn_prioritized_scratch_bytes(B))
    return settings, hs, P.aligned(4 * M * many.LEARNER, np.float32), many.noise(U, M), P.aligned(nbytes, np.float32), nbytes


def _learn_call(nat, a, B=8, U=1, per=None, trees=None, rows=None, tree_bytes=None, nbytes=None, idx=None, w=None):
    settings, hs, L, nf, scratch, nb = a
    M = len(settings)
    members, p = pm.member_arrays(nat, settings, rows or [h.rows.ctypes.data for h in hs],
                                  [h.counter.ctypes.data for h in hs], trees or [h.tree.ctypes.data for h in hs])
    rc = nat.lib.mg_host_rainbow_learn_prioritized_many(
        L.ctypes.data, members, M, CAP, B, U, nf.ctypes.data, None, None, None, None, scratch.ctypes.data,
        nb if nbytes is None else nbytes, None if per == "null" else p, hs[0].nbytes if tree_bytes is None else tree_bytes,
        idx, w)
    return rc, nat.lib.mg_last_error().decode(), members


def test_learn_refusals_name_the_member_and_change_nothing():
    from merging_gym import _native as nat

    a = _learn_args()
    settings, hs = a[0], a[1]
    what = "mg_host_rainbow_learn_prioritized_many: "
    t = [h.tree.ctypes.data for h in hs]
    before = [(h.tree.copy(), h.rows.copy(), int(h.counter[0])) for h in hs]
    L0 = a[2].copy()

    def refused(text, **kw):
        rc, msg, members = _learn_call(nat, a, **kw)
        assert rc == 1 and msg == what + text, msg
        assert all((int(e.first_update), int(e.first_draw)) == (s["first_update"], s["first_draw"])
                   for e, s in zip(members, settings))

    refused("NULL pointer", per="null")
    refused("member 1: NULL pointer (tree)", trees=[t[0], None])
    refused("member 1: the tree buffer must be 16-byte aligned", trees=[t[0], t[1] + 8])
    refused("tree buffer smaller than mg_per_bytes(capacity)", tree_bytes=hs[0].nbytes - 1)
    for field, bad, text in (("alpha", 0.0, "need alpha > 0"), ("beta", -0.5, "need beta > 0"),
                             ("beta", float("nan"), "need beta > 0"), ("prio_eps", -1e-9, "need prio_eps >= 0")):
        keep, settings[1][field] = settings[1][field], bad
        refused("member 1: " + text)
        settings[1][field] = keep
    buf = np.zeros(64, np.int64)
    refused("idx_out must be 8-byte, weight_out 4-byte aligned", idx=buf.ctypes.data + 4)
    refused("idx_out must be 8-byte, weight_out 4-byte aligned", w=buf.ctypes.data + 2)
    refused("scratch smaller than members * mg_rainbow_learn_prioritized_scratch_bytes(batch)", nbytes=a[5] - 1)
    shared = "member 1: its tree or rows are another member's (learning writes the tree: a shared replay has no defined order)"
    refused(shared, trees=[t[0], t[0]])
    refused(shared, rows=[hs[0].rows.ctypes.data] * 2)
    # mg_rainbow_learn_many's own refusals come first, in its order
    rc, msg, _ = _learn_call(nat, a, B=0, per="null")
    assert rc == 1 and msg == what + "need 1 <= batch <= 1024"
    for h, (tree, rows, counter) in zip(hs, before):
        assert (P.f64bits(h.tree) == P.f64bits(tree)).all() and (bits(h.rows) == bits(rows)).all()
        assert int(h.counter[0]) == counter
    assert (bits(a[2]) == bits(L0)).all()
    rc, msg, members = _learn_call(nat, a)  # and the call they all varied is a valid one
    assert rc == 0 and int(members[0].first_update) == settings[0]["first_update"] + 1


def test_device_learn_refuses_the_same_before_any_launch():
    """The device entry point's argument checks need no GPU: the table comes behind mg_rainbow_learn_many's checks,
    the trees behind the table."""
    from merging_gym import _native as nat

    a = _learn_args()
    settings, hs, L, nf, scratch, nb = a
    members, per = pm.member_arrays(nat, settings, [h.rows.ctypes.data for h in hs], [h.counter.ctypes.data for h in hs],
                                    [hs[0].tree.ctypes.data] * 2)
    table = P.aligned(int(nat.lib.mg_rainbow_learn_many_table_bytes(2)), np.uint8)

    def call(table_bytes):
        rc = nat.lib.mg_rainbow_learn_prioritized_many(
            L.ctypes.data, table.ctypes.data, table_bytes, members, 2, CAP, 8, 1, nf.ctypes.data, None, None, None, None,
            None, 0, scratch.ctypes.data, nb, per, hs[0].nbytes, None, None, None)
        return rc, nat.lib.mg_last_error().decode()

    assert call(table.nbytes - 1) == (1, "mg_rainbow_learn_prioritized_many: table smaller than "
                                         "mg_rainbow_learn_many_table_bytes(members)")
    rc, msg = call(table.nbytes)
    assert rc == 1 and msg.startswith("mg_rainbow_learn_prioritized_many: member 1: its tree or rows are another")
    assert int(members[0].first_update) == settings[0]["first_update"]


def test_store_refusals_name_the_member_and_change_nothing():
    from merging_gym import _native as nat

    hs = [P.HostPer(CAP, a) for a in (1.0, 0.6)]
    for h in hs:
        h.push_many(5)
    before = [(h.tree.copy(), h.rows.copy()) for h in hs]
    batch, _ = pm.store_batch(3, 2, 2, [5, 5])
    X = P.transitions_struct(nat, batch)
    ptrs = lambda vals: (ctypes.c_void_p * 2)(*vals)  # noqa: E731
    rows, counters = ptrs(h.rows.ctypes.data for h in hs), ptrs(h.counter.ctypes.data for h in hs)
    t = [h.tree.ctypes.data for h in hs]

    def refused(text, who="mg_host_per_store_many", trees=t, tree_bytes=hs[0].nbytes, alphas=(1.0, 0.6), members=2,
                r=rows):
        al = None if alphas is None else (ctypes.c_double * 2)(*alphas)
        tp = None if trees is None else ptrs(trees)
        args = (r, counters, members, CAP, ctypes.byref(X), 3, 2, tp, tree_bytes, al)
        rc = getattr(nat.lib, who)(*args, *((None,) if who == "mg_per_store_many" else ()))
        assert rc == 1 and nat.lib.mg_last_error().decode() == f"{who}: {text}", nat.lib.mg_last_error()

    for who in ("mg_host_per_store_many", "mg_per_store_many"):  # the device call refuses before any launch
        refused("need 1 <= members <= 64", who, members=65)
        refused("a ring is listed twice (two members' appends to one ring have no defined order)", who,
                r=ptrs([hs[0].rows.ctypes.data] * 2))
        refused("NULL pointer", who, trees=None)
        refused("NULL pointer", who, alphas=None)
        refused("member 1: NULL pointer (tree)", who, trees=[t[0], None])
        refused("member 0: the tree buffer must be 16-byte aligned", who, trees=[t[0] + 8, t[1]])
        refused("tree buffer smaller than mg_per_bytes(capacity)", who, tree_bytes=hs[0].nbytes - 8)
        refused("member 1: need alpha > 0", who, alphas=(1.0, 0.0))
        refused("member 1: its tree is another member's (two members' stores to one tree have no defined order)", who,
                trees=[t[0], t[0]])
    for h, (tree, r) in zip(hs, before):
        assert (P.f64bits(h.tree) == P.f64bits(tree)).all() and (bits(h.rows) == bits(r)).all() and h.counter[0] == 5
