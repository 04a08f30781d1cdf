"""Helpers of the DQN population tests: the members' differing settings, their rings, the plain-C
restatement run once per member (tests/learn_ref.py's run_ref: the yardstick of every member) and the
host twin's call (mg_host_dqn_learn_many)."""

from __future__ import annotations

import ctypes
import functools

import numpy as np

import learn_ref as lr

U64 = 0xFFFFFFFFFFFFFFFF
PERIODS = (2, 3, 1)  # with first_update = m: in update 1 member 0 (t = 1) and member 1 (t = 2) keep their
                     # targets while member 2 copies; so do members 3k, 3k + 1, 3k + 2 of a larger population
UPDATES = 4


def member_kw(m):
    """Member m's own seed (64-bit), hyperparameters and counters: no two of a population's agree in all."""
    return dict(seed=((7 + m) * 0x9E3779B97F4A7C15) & U64, lr=0.01 * (1 + 0.25 * (m % 5)), gamma=0.9 - 0.01 * (m % 7),
                beta1=0.9 - 0.02 * (m % 4), beta2=0.999 - 0.001 * (m % 3), eps=1e-8 * (1 + m % 3),
                target_period=PERIODS[m % 3], first_update=m, first_draw=5 + 3 * m)


def sync_masks(kws, updates):
    """Per update, the set of members whose target copy is due."""
    return [{m for m, kw in enumerate(kws) if (kw["first_update"] + u) % kw["target_period"] == 0}
            for u in range(updates)]


def fixture(in_dim, out_dim, batch, big=False):
    """(rows, state dict): learn_ref.case_fixture, or with `big` always a 2,000-row memory (10 -> 3 then
    learns from L0_memory, whose actions 3 and 4 the learner keeps inside its three)."""
    if big and (in_dim, out_dim) == (10, 3):
        return lr.memory("L0_memory"), lr.seeded_net(10, 3, 3)
    return lr.case_fixture(in_dim, out_dim, batch)


def member_rings(rows, members):
    """Per member the fixture's rows rolled by its own offset, the first half stored; counters that differ."""
    rings, counters = [], []
    for m in range(members):
        ring, half = lr.half_filled(np.roll(rows, 37 * m + 11, axis=0))
        rings.append(ring)
        counters.append(half - m)
    return rings, counters


def start_blocks(sd, members):
    """[M, 4, P]: every member from the state dict, scaled a little per member, the target at half the
    eval block so that a missed or spurious copy shows."""
    L = np.stack([lr.learner_array(sd)] * members)
    for m in range(members):
        L[m, 0] *= np.float32(1.0 - 0.01 * (m % 9))
        L[m, 1] = L[m, 0] * np.float32(0.5)
    return L


@functools.lru_cache(maxsize=None)
def reference(in_dim, out_dim, batch, members, filled_only, big=False, updates=UPDATES):
    """The restatement's runs of a population case, computed once and shared: (state dict, rings, counters,
    member settings, start [M, 4, P], end [M, 4, P], loss [U, M], rows [U, M, B, RF])."""
    rows, sd = fixture(in_dim, out_dim, batch, big)
    rings, counters = member_rings(rows, members)
    kws = [member_kw(m) for m in range(members)]
    L0 = start_blocks(sd, members)
    end, loss, got = [], [], []
    for m in range(members):
        e, l, r, _ = lr.run_ref(L0[m], rings[m], counters[m], in_dim, out_dim, batch, updates,
                                filled_only=filled_only, **kws[m])
        end.append(e), loss.append(l), got.append(r)
    for a in (L0, *rings):
        a.setflags(write=False)
    return sd, rings, counters, kws, L0, np.stack(end), np.stack(loss, axis=1), np.stack(got, axis=1)


def member_array(rings, counters, kws):
    """(the mg_dqn_member array, what it points to): host rings and counters, kept alive by the caller."""
    from merging_gym import _native

    M = len(kws)
    keep = [np.ascontiguousarray(r, dtype=np.float32) for r in rings]
    cnt = [np.array([c], dtype=np.uint64) for c in counters]
    arr = (_native.DqnMember * M)()
    for m, kw in enumerate(kws):
        arr[m] = _native.DqnMember(keep[m].ctypes.data, cnt[m].ctypes.data, kw["seed"], kw["first_update"],
                                   kw["first_draw"],
                                   _native.DqnHyper(kw["lr"], kw["gamma"], kw["beta1"], kw["beta2"], kw["eps"],
                                                    kw["target_period"], 0))
    return arr, (keep, cnt)


def run_host_many(L0, rings, counters, kws, in_dim, out_dim, batch, updates, filled_only=False, members=None):
    """mg_host_dqn_learn_many on a copy of L0 [M, 4, P]: (learners, loss [U, M], rows [U, M, B, RF], the
    member array after the call)."""
    from merging_gym import _native

    M = len(kws)
    L = np.array(L0, dtype=np.float32, copy=True)
    arr, keep = members if members is not None else member_array(rings, counters, kws)
    rf = 2 * in_dim + 2
    loss = np.zeros((updates, M), dtype=np.float32)
    got = np.zeros((updates, M, batch, rf), dtype=np.float32)
    nbytes = _native.lib.mg_dqn_learn_scratch_bytes(batch, in_dim, out_dim) * M
    scratch = np.zeros(nbytes // 4, dtype=np.float32)
    assert L.ctypes.data % 16 == 0 and scratch.ctypes.data % 16 == 0
    rc = _native.lib.mg_host_dqn_learn_many(L.ctypes.data, arr, M, rings[0].shape[0], rf, in_dim, out_dim, batch,
                                            updates, int(filled_only), loss.ctypes.data, got.ctypes.data,
                                            scratch.ctypes.data, nbytes)
    _native.check(rc, "mg_host_dqn_learn_many")
    return L, loss, got, (arr, keep)


def assert_members_equal(got, loss, rows, ref_end, ref_loss, ref_rows):
    """Bit for bit on every member's eval, target, m and v, every loss and every sampled row."""
    assert np.array_equal(lr.bits(rows), lr.bits(ref_rows))
    assert np.array_equal(lr.bits(loss), lr.bits(ref_loss)), (loss, ref_loss)
    for m in range(ref_end.shape[0]):
        for blk, name in enumerate(("eval", "target", "m", "v")):
            bad = lr.bits(got[m, blk]) != lr.bits(ref_end[m, blk])
            assert not bad.any(), (m, name, int(bad.sum()), float(np.abs(got[m, blk] - ref_end[m, blk]).max()))
