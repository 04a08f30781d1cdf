"""Helpers of the prioritized population's tests: M member settings that differ in every field, host replays
(per_ref.HostPer) at different counters, the lone host twin (mg_host_rainbow_learn_prioritized) once per member --
the reference of every comparison -- and the calls of the member entry points on host and device memory."""

from __future__ import annotations

import ctypes

import numpy as np

import per_ref as P
import rainbow_learn_many_ref as many
import rainbow_learn_ref as R
from learn_ref import bits

NAMES = ("learner", "loss", "rows", "proj", "grads", "idx", "weights")


def member_settings(members):
    """rainbow_learn_many_ref's settings (every member on its own replay) with the prioritized fields: alpha 1.0
    and 0.6 in turn, beta 0.4 and 1.0 in turn (but in steps of two, so all four pairs occur), prio_eps of its own."""
    out = many.member_settings(members)
    for m, s in enumerate(out):
        s.update(ring=m, alpha=(1.0, 0.6)[m % 2], beta=(0.4, 1.0)[(m // 2) % 2], prio_eps=1e-5 * (1 + m % 4))
    return out


def replay_counts(members, cap):
    """The transitions pushed per member: wrapped, partly filled (never fewer than two) and wrapped several times
    in turn, no two neighbours alike."""
    return [(cap + cap // 2 + 1 + m, max(2, cap // 2 + 1 + m % 3), 3 * cap + m)[m % 3] for m in range(members)]


def replays(settings, cap, counts=None, rounds=6):
    """One HostPer per member with its alpha: replay_counts' pushes, recorded observations as rows (other rows per
    member) and a tree that `rounds` rounds of sample and update have shaped."""
    out = []
    for m, (s, count) in enumerate(zip(settings, counts or replay_counts(len(settings), cap))):
        h = P.HostPer(cap, s["alpha"])
        h.push_many(count, n=min(cap, 500))
        rows = R.replay_rows(cap, seed=7 + m)
        rows[len(h):] = 0.0
        h.rows[:] = rows
        for r in range(rounds if len(h) >= 2 else 0):
            idx, _ = h.sample(P.BATCH, P.BETA, 1 + m, r)
            h.update(idx, np.exp(np.random.default_rng(100 * m + r).uniform(np.log(1e-3), np.log(8.0), P.BATCH))
                     .astype(np.float32))
        out.append(h)
    return out


def _hyper(nat, s):
    return nat.DqnHyper(s["lr"], s["gamma"], s["beta1"], s["beta2"], s["eps"], 1, 0)


def run_lone(L, settings, pers, B, U, noise_f):
    """mg_host_rainbow_learn_prioritized once per member on copies of L[m] and clones of pers[m]: (L [M, ...],
    loss [U, M], rows [U, M, B, 24], proj, grads, idx [U, M, B], weights [U, M, B], the clones as the calls left
    them)."""
    outs, after = [], []
    for m, s in enumerate(settings):
        h = pers[m].clone()
        nat = h.nat
        Lp = P.aligned(4 * many.LEARNER, np.float32)
        Lp[:] = L[m]
        nf = np.ascontiguousarray(noise_f[:, m], dtype=np.float32)
        loss, rows, proj, grads = R._outs(U, B)
        idx, w = np.full((U, B), -7, np.int64), np.full((U, B), np.nan, np.float32)
        nbytes = int(nat.lib.mg_rainbow_learn_prioritized_scratch_bytes(B))
        scratch = P.aligned(nbytes, np.float32)
        hs = _hyper(nat, s)
        rc = nat.lib.mg_host_rainbow_learn_prioritized(
            Lp.ctypes.data, h.rows.ctypes.data, h.counter.ctypes.data, h.capacity, B, U, s["first_update"], s["seed"],
            s["first_draw"], ctypes.byref(hs), nf.ctypes.data, loss.ctypes.data, rows.ctypes.data, proj.ctypes.data,
            grads.ctypes.data, scratch.ctypes.data, nbytes, h.tree.ctypes.data, h.nbytes, h.alpha, s["beta"],
            s["prio_eps"], idx.ctypes.data, w.ctypes.data)
        nat.check(rc, "mg_host_rainbow_learn_prioritized")
        outs.append((Lp.copy(), loss, rows, proj, grads, idx, w))
        after.append(h)
    return (np.stack([o[0] for o in outs]),) + tuple(np.stack([o[k] for o in outs], axis=1) for k in range(1, 7)) + (after,)


def member_arrays(nat, settings, row_ptrs, counter_ptrs, tree_ptrs):
    """((mg_dqn_member * M), (mg_per_member * M)) of the settings."""
    members = many.member_array(settings, row_ptrs, counter_ptrs)
    per = (nat.PerMember * len(settings))(*(nat.PerMember(t, s["alpha"], s["beta"], s["prio_eps"])
                                            for t, s in zip(tree_ptrs, settings)))
    return members, per


def outs(U, M, B):
    return many.outs(U, M, B) + (np.full((U, M, B), -7, np.int64), np.full((U, M, B), np.nan, np.float32))


def run_host_many(L, settings, pers, B, U, noise_f, calls=None):
    """mg_host_rainbow_learn_prioritized_many on a copy of L and clones of pers, in one call or in the `calls`
    chunk sizes: run_lone's tuple, then the member array as the calls left it."""
    from merging_gym import _native as nat

    M = len(settings)
    hs = [h.clone() for h in pers]
    Lp = P.aligned(4 * M * many.LEARNER, np.float32)
    Lp[:] = np.asarray(L, np.float32).reshape(-1)
    members, per = member_arrays(nat, settings, [h.rows.ctypes.data for h in hs], [h.counter.ctypes.data for h in hs],
                                 [h.tree.ctypes.data for h in hs])
    nbytes = M * int(nat.lib.mg_rainbow_learn_prioritized_scratch_bytes(B))
    scratch = P.aligned(nbytes, np.float32)
    nf = np.ascontiguousarray(noise_f, dtype=np.float32)
    o = outs(U, M, B)
    u0 = 0
    for n in calls or [U]:
        rc = nat.lib.mg_host_rainbow_learn_prioritized_many(
            Lp.ctypes.data, members, M, hs[0].capacity, B, n, nf[u0:].ctypes.data if n else None,
            *(a[u0:].ctypes.data for a in o[:4]), scratch.ctypes.data, nbytes, per, hs[0].nbytes,
            o[4][u0:].ctypes.data, o[5][u0:].ctypes.data)
        nat.check(rc, "mg_host_rainbow_learn_prioritized_many")
        u0 += n
    return (Lp.reshape(M, many.LEARNER).copy(), *o, hs, members)


def run_device_many(torch, L, settings, pers, B, U, noise_f, calls=None, dev="cuda:0"):
    """mg_rainbow_learn_prioritized_many on device copies: run_host_many's tuple (the replays read back into
    clones), then the packed nets."""
    from merging_gym import _native as nat

    lib, M = nat.lib, len(settings)
    stream = torch.cuda.current_stream(dev).cuda_stream
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)  # noqa: E731
    Ld, nf = up(np.asarray(L, np.float32)), up(np.asarray(noise_f, np.float32))
    rows, trees = [up(h.rows) for h in pers], [up(h.tree) for h in pers]
    counters = [up(h.counter.view(np.int64)) for h in pers]
    members, per = member_arrays(nat, settings, [t.data_ptr() for t in rows], [t.data_ptr() for t in counters],
                                 [t.data_ptr() for t in trees])
    tbytes = lib.mg_rainbow_learn_many_table_bytes(M)
    table = torch.empty(tbytes, dtype=torch.uint8, device=dev)
    nat.check(lib.mg_rainbow_learn_many_init(table.data_ptr(), tbytes, members, M, stream), "init")
    sbytes = M * lib.mg_rainbow_learn_prioritized_scratch_bytes(B)
    scratch = torch.empty(sbytes // 4, dtype=torch.float32, device=dev)
    stride = lib.mg_rainbow_packed_bytes()
    packed = torch.zeros((M, stride), dtype=torch.uint8, device=dev)
    o = [up(a) for a in outs(U, M, B)]
    u0 = 0
    for n in calls or [U]:
        rc = lib.mg_rainbow_learn_prioritized_many(
            Ld.data_ptr(), table.data_ptr(), tbytes, members, M, pers[0].capacity, B, n,
            nf[u0:].data_ptr() if n else None, *(a[u0:].data_ptr() for a in o[:4]), packed.data_ptr(), stride,
            scratch.data_ptr(), sbytes, per, pers[0].nbytes, o[4][u0:].data_ptr(), o[5][u0:].data_ptr(), stream)
        nat.check(rc, "mg_rainbow_learn_prioritized_many")
        u0 += n
    torch.cuda.synchronize()
    hs = []
    for h, r, t, c in zip(pers, rows, trees, counters):
        g = h.clone()
        g.rows[:], g.tree[:], g.counter[:] = r.cpu().numpy(), t.cpu().numpy(), c.cpu().numpy().view(np.uint64)
        hs.append(g)
    return (Ld.cpu().numpy(), *(a.cpu().numpy() for a in o), hs, members, packed.cpu().numpy())


def assert_members_same(got, want, members=None):
    """Bit for bit, member by member: the learner block, the six outputs, every double of the tree (max_priority
    included), the rows and the counter."""
    for m in (range(got[0].shape[0]) if members is None else members):
        for k, name in enumerate(NAMES):
            a, b = (got[k][m], want[k][m]) if k == 0 else (got[k][:, m], want[k][:, m])
            a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
            diff = np.flatnonzero(a.view(np.uint8).ravel() != b.view(np.uint8).ravel())
            assert diff.size == 0, f"member {m}: {name}: {diff.size} bytes differ, first at {diff[:1]}"
        g, w = got[7][m], want[7][m]
        diff = np.flatnonzero(P.f64bits(g.tree) != P.f64bits(w.tree))
        assert diff.size == 0, f"member {m}: {diff.size} tree doubles differ, first at {diff[:1]}"
        assert (bits(g.rows) == bits(w.rows)).all() and g.counter[0] == w.counter[0], f"member {m}: rows or counter"


# ---------------------------------------------------------------------------- the member store
def store_counters(members):
    """Where each member's ring stands before per_model.scenario_stores: all different, so the two wrapped segments
    of a store differ from member to member."""
    return [0] + [3 + 4 * m for m in range(1, members)]


def store_batch(n, T, members, first):
    """One [T, members * n, ...] batch whose member slices are P.transitions(n, T, first[m]), with the rollout's
    flags in place of a1 and done: (batch, the slices)."""
    parts = [P.transitions(n, T, first=f) for f in first]
    cat = lambda k, ax: np.ascontiguousarray(np.concatenate([p[k] for p in parts], axis=ax))  # noqa: E731
    flags = np.zeros((T, members * n, 4), np.uint8)
    flags[..., 0], flags[..., 2] = cat("a1", 1).view(np.uint8), cat("done", 1)
    batch = dict(obs_first=cat("obs_first", 0), obs=cat("obs", 1), final_obs=cat("final_obs", 1), rew=cat("rew", 1),
                 flags=flags)
    return batch, parts


def store_many(lib_call, nat, hs, batch, n, T, pointer=lambda a: a.ctypes.data, extra=()):
    """One call of mg_host_per_store_many (or the device entry point, with `extra` = its stream) into the HostPers
    (or device buffers behind `pointer`)."""
    M = len(hs)
    X = P.transitions_struct(nat, batch, pointer)
    rows = (ctypes.c_void_p * M)(*(pointer(h.rows) for h in hs))
    counters = (ctypes.c_void_p * M)(*(pointer(h.counter) for h in hs))
    trees = (ctypes.c_void_p * M)(*(pointer(h.tree) for h in hs))
    alphas = (ctypes.c_double * M)(*(h.alpha for h in hs))
    return lib_call(rows, counters, M, hs[0].capacity, ctypes.byref(X), n, T, trees, hs[0].nbytes, alphas, *extra)
