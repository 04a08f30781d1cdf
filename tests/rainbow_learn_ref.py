"""Helpers of the Rainbow learner's tests: the plain-C restatement (tests/native/rainbow_learn_ref.c, compiled
with the C compiler at test time and loaded with ctypes), the nets of tests/golden/rainbow_golden.npz, replay
rows built from the reference's recorded observations, and the host twin's call."""

from __future__ import annotations

import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from learn_ref import bits, cc  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rainbow_learn_ref.c")
HYPER = dict(lr=0.001, gamma=0.99, beta1=0.9, beta2=0.999, eps=1e-8)  # ranbowdqn.py:645, :569, Adam's defaults
BATCHES = (1, 32, 33, 128)
RINGS = ((64, 40), (64, 200))  # (capacity, counter): partly filled, wrapped
NP, NE, NF, NZ, ROW = 58884, 28210, 1124, 51, 24

_u64, _i64, _i32, _dbl, _P = ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_double, ctypes.c_void_p


@functools.lru_cache(maxsize=1)
def build_ref():
    out = os.path.join(tempfile.mkdtemp(prefix="rainbow_learn_ref."), "librainbow_learn_ref.so")
    subprocess.check_call([cc(), "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-o", out, SRC, "-lm"])
    lib = ctypes.CDLL(out)
    lib.rainbow_learn_ref.argtypes = [_P, _P, _u64, _i64, _i32, _i32, _u64, _u64, _u64, _dbl, _dbl, _dbl, _dbl, _dbl,
                                      _P, _P, _P, _P, _P]
    lib.rainbow_project_ref.argtypes = [_P, ctypes.c_float, ctypes.c_float, ctypes.c_float, _P, _P]
    lib.rainbow_project_ref.restype = None
    lib.rainbow_log_ref.argtypes = [ctypes.c_float]
    lib.rainbow_log_ref.restype = ctypes.c_float
    lib.rainbow_log_scan.argtypes = [_P, ctypes.c_float, ctypes.c_float, _P, _P, _P]
    lib.rainbow_log_scan.restype = _i64
    return lib


def fixture(fam, u):
    """(state, grads) of tests/golden/rainbow_learn_{fam}_u{u}_*.npz."""
    return _golden(f"rainbow_learn_{fam}_u{u}_state.npz"), _golden(f"rainbow_learn_{fam}_u{u}_grads.npz")


def fixture_learner(fam, u):
    """The learner buffer of the recorded before-state: the current model as recorded; the target's parameters
    are update 0's current ones (update_target's copy), its noise as recorded."""
    import torch

    st, st0 = fixture(fam, u)[0], fixture(fam, 0)[0]
    cur = {k[4:]: torch.from_numpy(np.array(st[k])) for k in st.files if k.startswith("cur/")}
    tgt = {k[4:]: torch.from_numpy(np.array(st0[k])) for k in st0.files if k.startswith("cur/")}
    tgt.update({k[4:]: torch.from_numpy(np.array(st[k])) for k in st.files if k.startswith("tgt/")})
    from merging_gym import rainbow_learn

    return rainbow_learn.learner_array(cur, tgt).numpy().copy()


def ring_of_chosen_rows(rows, capacity=4096):
    """(ring, counter, seed): a full ring in which minibatch row b's slot holds rows[b], for the first seed whose
    slots are distinct. The slots are read off the host twin's sampled rows of a ring that stores its row numbers."""
    B = len(rows)
    probe = np.zeros((capacity, ROW), np.float32)
    probe[:, 0] = np.arange(capacity)
    L = np.zeros(4 * NP + 2 * NE + 52, np.float32)
    for seed in range(100):
        slots = run_host(L, probe, capacity, B, 1, seed=seed, noise_f=np.zeros((1, 2, NF), np.float32))[2][0, :, 0]
        slots = slots.astype(np.int64)
        if len(set(slots.tolist())) == B:
            ring = np.zeros((capacity, ROW), np.float32)
            ring[slots] = rows
            return ring, capacity, seed
    raise AssertionError("no seed with distinct slots")


@functools.lru_cache(maxsize=None)
def _golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def golden_state(seed=1, fam="soft"):
    """RainbowDQN.state_dict() (torch tensors) of tests/golden/rainbow_golden.npz: 'default' as constructed,
    'soft' with linear1.weight / 1024 (gen_rainbow.py's two families)."""
    import torch

    z = _golden("rainbow_golden.npz")
    pre = f"s{seed}/sd/"
    sd = {k[len(pre):]: torch.from_numpy(np.array(z[k], dtype=np.float32)) for k in z.files if k.startswith(pre)}
    if fam == "soft":
        sd["linear1.weight"] = sd["linear1.weight"] / 1024.0
    return sd


def replay_rows(capacity, seed=7):
    """[capacity, 24] fp32 rows: consecutive recorded observations as s and s', actions 0..4, rewards that hit
    both clamps and give integral b, done both ways."""
    obs = np.asarray(_golden("reference_golden.npz")["katB_obs"], dtype=np.float32)
    rng = np.random.default_rng(seed)
    at = rng.integers(0, len(obs) - 1, capacity)
    rows = np.zeros((capacity, ROW), dtype=np.float32)
    rows[:, :10] = obs[at]
    rows[:, 12:22] = obs[at + 1]
    rows[:, 10] = rng.integers(0, 5, capacity)
    rows[:, 11] = rng.choice(np.array([-10.0, 10.0, 0.0, 0.4, 1.2, 2.0, -0.001, 1.0, 25.0, -0.37], np.float32), capacity)
    rows[:, 22] = rng.integers(0, 2, capacity)
    return rows


def ring_case(capacity, counter, seed=7):
    """(ring, counter): what `counter` pushes leave in a ring of `capacity` rows (the rest still zero)."""
    rows = replay_rows(capacity, seed)
    if counter < capacity:
        rows[counter:] = 0.0
    return rows, counter


def learner_numpy(sd):
    from merging_gym import rainbow_learn

    return rainbow_learn.learner_array(sd).numpy().copy()


def noise(num_updates, seed=11):
    import torch

    from merging_gym import rainbow_learn

    g = torch.Generator().manual_seed(seed)
    return rainbow_learn.noise_factors(num_updates, g).numpy().copy()


def sync_target(L):
    L[NP:2 * NP] = L[:NP]
    L[4 * NP + NE:4 * NP + 2 * NE] = L[4 * NP:4 * NP + NE]


def _outs(U, B):
    return (np.zeros(U, np.float32), np.zeros((U, B, ROW), np.float32), np.zeros((U, B, NZ), np.float32),
            np.zeros((U, NP), np.float32))


def run_ref(L, ring, counter, B, U, first_update=0, seed=0, first_draw=0, noise_f=None, **hyper):
    """The restatement on a copy of L: (L, loss [U], rows [U, B, 24], proj [U, B, 51], grads [U, P])."""
    h = dict(HYPER, **hyper)
    L = np.array(L, dtype=np.float32, copy=True)
    ring = np.ascontiguousarray(ring, dtype=np.float32)
    nf = np.ascontiguousarray(noise_f, dtype=np.float32)
    assert nf.shape == (U, 2, NF)
    loss, rows, proj, grads = _outs(U, B)
    rc = build_ref().rainbow_learn_ref(L.ctypes.data, ring.ctypes.data, counter, ring.shape[0], B, U, first_update, seed,
                                       first_draw, h["lr"], h["gamma"], h["beta1"], h["beta2"], h["eps"], nf.ctypes.data,
                                       loss.ctypes.data, rows.ctypes.data, proj.ctypes.data, grads.ctypes.data)
    assert rc == 0
    return L, loss, rows, proj, grads


def run_host(L, ring, counter, B, U, first_update=0, seed=0, first_draw=0, noise_f=None, **hyper):
    """mg_host_rainbow_learn on a copy of L: the same tuple as run_ref."""
    from merging_gym import _native

    h = dict(HYPER, **hyper)
    L = np.array(L, dtype=np.float32, copy=True)
    ring = np.ascontiguousarray(ring, dtype=np.float32)
    nf = np.ascontiguousarray(noise_f, dtype=np.float32)
    cnt = np.array([counter], dtype=np.uint64)
    loss, rows, proj, grads = _outs(U, B)
    nbytes = _native.lib.mg_rainbow_learn_scratch_bytes(B)
    scratch = np.zeros(nbytes // 4 + 4, dtype=np.float32)
    off = (-scratch.ctypes.data % 16) // 4
    Lp = np.zeros(L.size + 4, dtype=np.float32)
    lo = (-Lp.ctypes.data % 16) // 4
    Lp[lo:lo + L.size] = L
    hs = _native.DqnHyper(h["lr"], h["gamma"], h["beta1"], h["beta2"], h["eps"], 1, 0)
    rc = _native.lib.mg_host_rainbow_learn(Lp.ctypes.data + 4 * lo, ring.ctypes.data, cnt.ctypes.data, ring.shape[0], B, U,
                                           first_update, seed, first_draw, ctypes.byref(hs), nf.ctypes.data,
                                           loss.ctypes.data, rows.ctypes.data, proj.ctypes.data, grads.ctypes.data,
                                           scratch.ctypes.data + 4 * off, nbytes)
    _native.check(rc, "mg_host_rainbow_learn")
    return Lp[lo:lo + L.size].copy(), loss, rows, proj, grads


def sequence(run, L0, ring, counter, B, seed=3):
    """learn(2), sync_target(), learn(1) through `run`: (final L, [outputs of the two calls])."""
    nf = noise(3)
    L, *out1 = run(L0, ring, counter, B, 2, 0, seed, 0, nf[:2])
    sync_target(L)
    L, *out2 = run(L, ring, counter, B, 1, 2, seed, 2, nf[2:])
    return L, out1 + out2


# The batch edges with real gradients: one row, a wave and a row, the first batch past one block of items, the
# largest batch. The "soft" family: "default" saturates the softmax, and at B = 1 its gradient is exactly zero.
EDGE_BATCHES = (1, 33, 257, 1024)
# The minibatch seed of those cases. 25 of replay_rows(64)'s rows have no gradient at all: a done row whose
# clamped reward falls on an atom has l == u in the projection, both shares are zero and its mass is dropped, as
# in the reference, so proj is zero and so is the loss. With one row per update the seed decides whether an update
# draws such a row; 36 is the first seed from 3 (sequence()'s default) on whose three draws have a gradient on
# both RINGS, chosen by the restatement, not by the library.
EDGE_SEED = 36


@functools.lru_cache(maxsize=None)
def edge_reference(batch, capacity, counter):
    """The restatement's sequence() from the "soft" golden state under EDGE_SEED, computed once for the host and
    the device test (read-only arrays), after its own check that every one of the three updates is a real one: a
    gradient with non-zero entries, and current parameters that moved. The parameters after each update come
    from the restatement run one update per call, whose end has to be sequence()'s end bit for bit."""
    L0 = learner_numpy(golden_state(1, "soft"))
    ring, c = ring_case(capacity, counter)
    want = sequence(run_ref, L0, ring, c, batch, seed=EDGE_SEED)
    nf, L, moved, nonzero = noise(3), L0, [], []
    for u in range(3):
        if u == 2:
            L = L.copy()
            sync_target(L)
        after, _, _, _, grads = run_ref(L, ring, c, batch, 1, u, EDGE_SEED, u, nf[u:u + 1])
        assert np.array_equal(bits(grads[0]), bits((want[1][3][u] if u < 2 else want[1][7][0]))), u
        moved.append(int(np.count_nonzero(bits(after[:NP]) != bits(L[:NP]))))
        nonzero.append(int(np.count_nonzero(grads[0])))
        L = after
    assert np.array_equal(bits(L), bits(want[0]))
    print(f"B {batch}, ring {(capacity, counter)}: non-zero gradients per update {nonzero}, parameters moved {moved}")
    assert min(nonzero) > 0 and min(moved) > 0, (nonzero, moved)
    for a in (want[0], *want[1]):
        a.setflags(write=False)
    return L0, want


NAMES = ("loss", "rows", "proj", "grads") * 2
BLOCKS = (("current", 0, NP), ("target", NP, 2 * NP), ("m", 2 * NP, 3 * NP), ("v", 3 * NP, 4 * NP),
          ("noise current", 4 * NP, 4 * NP + NE), ("noise target", 4 * NP + NE, 4 * NP + 2 * NE))


def assert_same(got, want):
    """Bit for bit: the learner's blocks, then every loss, sampled row, proj and gradient."""
    (Lg, og), (Lw, ow) = got, want
    for name, a, b in BLOCKS:
        diff = np.flatnonzero(bits(Lg[a:b]) != bits(Lw[a:b]))
        assert diff.size == 0, f"{name}: {diff.size} of {b - a} differ, first at {diff[:1]}"
    for name, x, y in zip(NAMES, og, ow):
        diff = np.flatnonzero(bits(x).ravel() != bits(y).ravel())
        assert diff.size == 0, f"{name}: {diff.size} of {x.size} differ, first at {diff[:1]}"
