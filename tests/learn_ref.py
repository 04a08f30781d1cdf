"""Helpers of the DQN.learn tests: the plain-C restatement (tests/native/dqn_learn_ref.c, compiled
with the C compiler at test time and loaded with ctypes), the fixtures (the trained nets of
tests/golden/dqn_checkpoints.npz, the reference's memories of tests/golden/replay_golden.npz cast to
fp32 as ReplayRing holds them, seeded nets for the h-DQN shapes) and the host twin's call."""

from __future__ import annotations

import ctypes
import functools
import os
import subprocess
import tempfile

import numpy as np

from native_build import cc  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "dqn_learn_ref.c")
KEYS = ("fc1.weight", "fc1.bias", "fc2.weight", "fc2.bias", "out.weight", "out.bias")
# (in_dim, out_dim, batch) of the bit-exact cases; (memory, net) each shape runs on. The last three fall off
# the kernels' tile edges: one row; fewer rows than a layer-2 row tile or a layer-3 block (8 each) with out = 3;
# one row past a tile, on the goal rows.
CASES = [(10, 5, 128), (10, 5, 32), (10, 5, 96), (11, 5, 128), (10, 3, 128), (10, 5, 1), (10, 3, 5), (11, 5, 9)]
HYPER = dict(lr=0.01, gamma=0.9, beta1=0.9, beta2=0.999, eps=1e-8)  # main.py:13-14, Adam's defaults

_u64, _i64, _i32, _dbl = ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_double


@functools.lru_cache(maxsize=1)
def build_ref():
    """The restatement as a shared library in a fresh temporary directory (kept for the process)."""
    out = os.path.join(tempfile.mkdtemp(prefix="dqn_learn_ref."), "libdqn_learn_ref.so")
    subprocess.check_call([cc(), "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-o", out, SRC, "-lm"])
    lib = ctypes.CDLL(out)
    lib.dqn_learn_params.argtypes = [_i32, _i32]
    lib.dqn_learn_ref.argtypes = [ctypes.c_void_p, ctypes.c_void_p, _u64, _i64, _i32, _i32, _i32, _i32, _u64, _u64,
                                  _u64, _i32, _dbl, _dbl, _dbl, _dbl, _dbl, _i32, ctypes.c_void_p, ctypes.c_void_p,
                                  ctypes.c_void_p]
    return lib


def num_params(in_dim, out_dim):
    return 200 * in_dim + 200 + 100 * 200 + 100 + 100 * out_dim + out_dim


@functools.lru_cache(maxsize=None)
def _golden(name):
    return np.load(os.path.join(HERE, "golden", name))


def trained_net(tag):
    """State dict (numpy fp32) of a trained Net 10 -> 5: 'l1' or 'l3'."""
    z = _golden("dqn_checkpoints.npz")
    return {k: np.ascontiguousarray(z[f"{tag}/{k}"], dtype=np.float32) for k in KEYS}


def seeded_net(in_dim, out_dim, seed):
    """A Net with torch's default Linear initialisation (uniform in +-1/sqrt(fan_in)) from numpy's
    seeded generator: mixed signs, so both ReLU branches are met."""
    rng = np.random.default_rng(seed)
    sd = {}
    for name, (o, i) in (("fc1", (200, in_dim)), ("fc2", (100, 200)), ("out", (out_dim, 100))):
        a = 1.0 / np.sqrt(i)
        sd[f"{name}.weight"] = rng.uniform(-a, a, (o, i)).astype(np.float32)
        sd[f"{name}.bias"] = rng.uniform(-a, a, o).astype(np.float32)
    return sd


def memory(name):
    """One of the reference's memories as fp32 rows: L0_memory, RR_memory (2000 x 22), HL0_memory
    (2000 x 24), HL0_meta_memory (200 x 22)."""
    return np.ascontiguousarray(_golden("replay_golden.npz")[name], dtype=np.float32)


def case_fixture(in_dim, out_dim, batch=128):
    """(rows, state dict) of a case: the trained l3 on RR_memory at batch 128 and, since most hidden
    units of the trained nets are dead on these rows (1 % of fc1's gradient is non-zero), a seeded
    10 -> 5 net on L0_memory at the other batch sizes; a seeded 11 -> 5 net on the goal rows, a seeded
    10 -> 3 net on Goal_DQN's rows."""
    if (in_dim, out_dim) == (10, 5):
        if batch == 128:
            return memory("RR_memory"), trained_net("l3")
        return memory("L0_memory"), seeded_net(10, 5, 5)
    if (in_dim, out_dim) == (11, 5):
        return memory("HL0_memory"), seeded_net(11, 5, 11)
    if (in_dim, out_dim) == (10, 3):
        return memory("HL0_meta_memory"), seeded_net(10, 3, 3)
    raise KeyError((in_dim, out_dim))


def learner_array(sd):
    """[4, P] fp32: eval and target from the state dict, zero m and v (mg_dqn_learner_init)."""
    flat = np.concatenate([np.asarray(sd[k], dtype=np.float32).ravel() for k in KEYS])
    L = np.zeros((4, flat.size), dtype=np.float32)
    L[0] = L[1] = flat
    return L


def split(flat, in_dim, out_dim):
    """The six tensors of a flat [P] block, by name."""
    shapes = ((200, in_dim), (200,), (100, 200), (100,), (out_dim, 100), (out_dim,))
    out, at = {}, 0
    for k, s in zip(KEYS, shapes):
        n = int(np.prod(s))
        out[k] = flat[at:at + n].reshape(s)
        at += n
    assert at == flat.size
    return out


def run_ref(learner, rows, counter, in_dim, out_dim, batch, num_updates, first_update=0, seed=0, first_draw=0,
            filled_only=False, target_period=100, grads=False, **hyper):
    """The restatement on a copy of `learner`: (learner, loss [U], rows [U, B, RF], grads [U, P] or None)."""
    h = dict(HYPER, **hyper)
    L = np.array(learner, dtype=np.float32, copy=True)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    assert rows.shape[1] == 2 * in_dim + 2 and L.shape == (4, num_params(in_dim, out_dim))
    loss = np.zeros(num_updates, dtype=np.float32)
    got = np.zeros((num_updates, batch, rows.shape[1]), dtype=np.float32)
    g = np.zeros((num_updates, L.shape[1]), dtype=np.float32) if grads else None
    rc = build_ref().dqn_learn_ref(L.ctypes.data, rows.ctypes.data, counter, rows.shape[0], in_dim, out_dim, batch,
                                   num_updates, first_update, seed, first_draw, int(filled_only), h["lr"], h["gamma"],
                                   h["beta1"], h["beta2"], h["eps"], target_period, loss.ctypes.data, got.ctypes.data,
                                   g.ctypes.data if grads else None)
    assert rc == 0
    return L, loss, got, g


def hyper_struct(target_period=100, **hyper):
    from merging_gym import _native

    h = dict(HYPER, **hyper)
    return _native.DqnHyper(h["lr"], h["gamma"], h["beta1"], h["beta2"], h["eps"], target_period, 0)


def run_host(learner, rows, counter, in_dim, out_dim, batch, num_updates, first_update=0, seed=0, first_draw=0,
             filled_only=False, target_period=100, **hyper):
    """mg_host_dqn_learn on a copy of `learner`: (learner, loss [U], rows [U, B, RF])."""
    from merging_gym import _native

    L = np.array(learner, dtype=np.float32, copy=True)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    cnt = np.array([counter], dtype=np.uint64)
    loss = np.zeros(num_updates, dtype=np.float32)
    got = np.zeros((num_updates, batch, rows.shape[1]), dtype=np.float32)
    nbytes = _native.lib.mg_dqn_learn_scratch_bytes(batch, in_dim, out_dim)
    scratch = np.zeros(nbytes // 4, dtype=np.float32)
    h = hyper_struct(target_period, **hyper)
    for a in (L, rows, scratch):
        assert a.ctypes.data % 16 == 0
    rc = _native.lib.mg_host_dqn_learn(L.ctypes.data, rows.ctypes.data, cnt.ctypes.data, rows.shape[0],
                                       rows.shape[1], in_dim, out_dim, batch, num_updates, first_update, seed,
                                       first_draw, int(filled_only), ctypes.byref(h), loss.ctypes.data,
                                       got.ctypes.data, scratch.ctypes.data, nbytes)
    _native.check(rc, "mg_host_dqn_learn")
    return L, loss, got


def half_filled(rows):
    """(ring, counter): the first half of a memory stored, the rest still zero (main.py:92)."""
    half = rows.shape[0] // 2
    ring = np.zeros_like(rows)
    ring[:half] = rows[:half]
    return ring, half


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float32).view(np.uint32)
