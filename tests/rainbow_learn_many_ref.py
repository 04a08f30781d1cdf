"""Helpers of the Rainbow population's tests: M member settings that differ in every field, the restatement
(rainbow_learn_ref.run_ref) once per member, and the host twin's call (mg_host_rainbow_learn_many)."""

from __future__ import annotations

import numpy as np

import rainbow_learn_ref as ref
from rainbow_learn_ref import NE, NF, NP, NZ, RINGS, ROW

LEARNER = 4 * NP + 2 * NE + 52


def member_settings(members):
    """One dict per member: seed, first_update, first_draw, lr, gamma, beta1, beta2, eps all differ; the rings
    alternate RINGS[0] (partly filled) and RINGS[1] (wrapped), and the last member shares member 0's ring
    (`ring` is an index into rings())."""
    out = []
    for m in range(members):
        out.append(dict(seed=(3 + 1000003 * m) & (2 ** 64 - 1), first_update=2 * m, first_draw=5 * m + 1,
                        lr=0.001 * (1 + 0.5 * (m % 7)), gamma=0.99 - 0.01 * (m % 5), beta1=0.9 - 0.05 * (m % 3),
                        beta2=0.999 - 0.01 * (m % 4), eps=1e-8 * (1 + m % 6), ring=m))
    if members > 1:
        out[-1]["ring"] = 0
    return out


def rings(members):
    """(ring [capacity, 24], counter) per member index: RINGS[0] and RINGS[1] in turn, other rows per member."""
    return [ref.ring_case(*RINGS[m % 2], seed=7 + m) for m in range(members)]


def learners(members):
    """[members, LEARNER]: the golden nets, the two families and seeds in turn, so no two neighbours are equal."""
    fams = [("soft", 1), ("default", 1)]
    L = np.stack([ref.learner_numpy(ref.golden_state(seed, fam)) for fam, seed in fams])
    out = L[np.arange(members) % len(fams)].copy()
    out[:, :NP] *= (1.0 + np.arange(members, dtype=np.float32)[:, None] / 256.0)  # every member's own weights
    out[:, NP:2 * NP] = out[:, :NP]
    return out


def noise(U, members):
    """[U, members, 2, 1124]: rainbow_learn_ref.noise's torch factors, one stream per member."""
    return np.stack([ref.noise(U, seed=11 + m) for m in range(members)], axis=1).copy()


def run_ref_members(L, settings, ring_list, B, U, noise_f):
    """run_ref once per member: (L [M, ...], loss [U, M], rows [U, M, B, 24], proj [U, M, B, 51], grads [U, M, P])."""
    outs = []
    for m, s in enumerate(settings):
        ring, counter = ring_list[s["ring"]]
        outs.append(ref.run_ref(L[m], ring, counter, B, U, s["first_update"], s["seed"], s["first_draw"],
                                noise_f[:, m], lr=s["lr"], gamma=s["gamma"], beta1=s["beta1"], beta2=s["beta2"],
                                eps=s["eps"]))
    return (np.stack([o[0] for o in outs]),) + tuple(np.stack([o[k] for o in outs], axis=1) for k in range(1, 5))


def aligned(n, dtype=np.float32):
    """n zeroed elements at a 16-byte boundary (a view: keep it alive)."""
    item = np.dtype(dtype).itemsize
    raw = np.zeros(n + 16 // item, dtype=dtype)
    off = (-raw.ctypes.data % 16) // item
    return raw[off:off + n]


def member_array(settings, ring_ptrs, counter_ptrs):
    """(mg_dqn_member * M) of the settings; ring_ptrs / counter_ptrs per ring index."""
    from merging_gym import _native

    arr = (_native.DqnMember * len(settings))()
    for m, s in enumerate(settings):
        arr[m] = _native.DqnMember(ring_ptrs[s["ring"]], counter_ptrs[s["ring"]], s["seed"], s["first_update"],
                                   s["first_draw"],
                                   _native.DqnHyper(s["lr"], s["gamma"], s["beta1"], s["beta2"], s["eps"], 1, 0))
    return arr


def outs(U, M, B):
    return (np.zeros((U, M), np.float32), np.zeros((U, M, B, ROW), np.float32), np.zeros((U, M, B, NZ), np.float32),
            np.zeros((U, M, NP), np.float32))


def run_host_members(L, settings, ring_list, B, U, noise_f, calls=None):
    """mg_host_rainbow_learn_many on a copy of L, in one call or in the `calls` chunk sizes: the same tuple as
    run_ref_members, then the member array as the calls left it."""
    from merging_gym import _native

    M = len(settings)
    Lp = aligned(M * LEARNER)
    Lp[:] = np.asarray(L, np.float32).reshape(-1)
    rs = [np.ascontiguousarray(r, dtype=np.float32) for r, _ in ring_list]
    cs = [np.array([c], dtype=np.uint64) for _, c in ring_list]
    members = member_array(settings, [r.ctypes.data for r in rs], [c.ctypes.data for c in cs])
    nbytes = M * _native.lib.mg_rainbow_learn_scratch_bytes(B)
    scratch = aligned(nbytes // 4)
    nf = np.ascontiguousarray(noise_f, dtype=np.float32)
    loss, rows, proj, grads = outs(U, M, B)
    u0 = 0
    for n in calls or [U]:
        rc = _native.lib.mg_host_rainbow_learn_many(
            Lp.ctypes.data, members, M, rs[0].shape[0], B, n, nf[u0:].ctypes.data if n else None,
            loss[u0:].ctypes.data, rows[u0:].ctypes.data, proj[u0:].ctypes.data, grads[u0:].ctypes.data,
            scratch.ctypes.data, nbytes)
        _native.check(rc, "mg_host_rainbow_learn_many")
        u0 += n
    return Lp.reshape(M, LEARNER).copy(), loss, rows, proj, grads, members


def assert_members_same(got, want):
    """Bit for bit, member by member, through rainbow_learn_ref.assert_same."""
    for m in range(got[0].shape[0]):
        try:
            ref.assert_same((got[0][m], [g[:, m] for g in got[1:5]]), (want[0][m], [w[:, m] for w in want[1:5]]))
        except AssertionError as e:
            raise AssertionError(f"member {m}: {e}") from None
