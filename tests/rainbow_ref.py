"""Helpers of the Rainbow tests: the restatement of the acting forward in the tests' own words, from the
contract in include/merging_hip.h ("Rainbow acting") alone, and the fixtures.

Matrix layers: bf16 operands (round to nearest even), one chain of gfx950 MFMAs per output through
merge_oracle.mfma_dots (the C oracle's accumulation rule) with the k axis in the packed order; the head by the
plain-C restatement tests/native/rainbow_head_ref.c, compiled at test time and loaded with ctypes (it shares no
code with csrc/, like dqn_learn_ref.c)."""

from __future__ import annotations

import ctypes
import functools
import os
import shutil
import subprocess
import tempfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rainbow_head_ref.c")
SEEDS = (1, 2, 3)
ATOMS, ACTIONS, LOGITS = 51, 5, 306
LAYERS = ("linear1", "linear2", "noisy_value1", "noisy_value2", "noisy_advantage1", "noisy_advantage2")
NOISY = LAYERS[2:]


def cc():
    return os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc") or shutil.which("clang")


@functools.lru_cache(maxsize=1)
def head_lib():
    out = os.path.join(tempfile.mkdtemp(prefix="rainbow_head_ref."), "librainbow_head_ref.so")
    subprocess.check_call([cc(), "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math", "-Wall",
                           "-o", out, SRC, "-lm"])
    lib = ctypes.CDLL(out)
    P = ctypes.c_void_p
    lib.rainbow_exp_ref.argtypes = [P, P, ctypes.c_int64]
    lib.rainbow_head_ref.argtypes = [P, P, P, P, ctypes.c_int64]
    lib.rainbow_exp_ref.restype = lib.rainbow_head_ref.restype = None
    return lib


def support():
    import torch

    return torch.linspace(-10, 10, ATOMS).numpy()  # ranbowdqn.py:546


def head_ref(logits, z=None):
    """(q [n, 5], action [n]) of logits [n, 306] by the C restatement."""
    lg = np.ascontiguousarray(logits, np.float32).reshape(-1, LOGITS)
    z = np.ascontiguousarray(support() if z is None else z, np.float32)
    q = np.empty((len(lg), ACTIONS), np.float32)
    act = np.empty(len(lg), np.int8)
    head_lib().rainbow_head_ref(lg.ctypes.data, z.ctypes.data, q.ctypes.data, act.ctypes.data, len(lg))
    return q, act


def exp_ref(x):
    x = np.ascontiguousarray(x, np.float32)
    y = np.empty_like(x)
    head_lib().rainbow_exp_ref(x.ctypes.data, y.ctypes.data, x.size)
    return y


def head_host(logits, z=None):
    """The same through the library's mg_host_rainbow_head."""
    from merging_gym import _native

    lg = np.ascontiguousarray(logits, np.float32).reshape(-1, LOGITS)
    z = np.ascontiguousarray(support() if z is None else z, np.float32)
    q = np.empty((len(lg), ACTIONS), np.float32)
    act = np.empty(len(lg), np.int8)
    _native.check(_native.lib.mg_host_rainbow_head(lg.ctypes.data, z.ctypes.data, q.ctypes.data, act.ctypes.data,
                                                   len(lg)), "mg_host_rainbow_head")
    return q, act


# ---- fixtures
@functools.lru_cache(maxsize=None)
def golden(name="rainbow_golden.npz"):
    return np.load(os.path.join(HERE, "golden", name))


@functools.lru_cache(maxsize=1)
def observations():
    """Every katB_obs row of reference_golden.npz, fp32 as torch.FloatTensor(state) makes them."""
    return np.ascontiguousarray(np.load(os.path.join(HERE, "golden", "reference_golden.npz"))["katB_obs"], np.float32)


def state_dict(seed, soft=False):
    """The recorded RainbowDQN.state_dict() of a seed as torch tensors; soft: linear1.weight / 1024."""
    import torch

    z = golden()
    pre = f"s{seed}/sd/"
    sd = {k[len(pre):]: torch.from_numpy(np.array(z[k])) for k in z.files if k.startswith(pre)}
    if soft:
        sd["linear1.weight"] = sd["linear1.weight"] / 1024.0
    return sd


def effective_ref(sd):
    """The twelve effective tensors (numpy fp32) in the tests' own words: mu + sigma * epsilon, one fp32
    product and one fp32 sum per element (ranbowdqn.py:468-470)."""
    out = {}
    for name in LAYERS:
        for leaf in ("weight", "bias"):
            if name in NOISY:
                mu, sg, ep = (np.asarray(sd[f"{name}.{leaf}_{p}"], np.float32) for p in ("mu", "sigma", "epsilon"))
                out[f"{name}.{leaf}"] = (mu + (sg * ep).astype(np.float32)).astype(np.float32)
            else:
                out[f"{name}.{leaf}"] = np.asarray(sd[f"{name}.{leaf}"], np.float32)
    return out


# ---- the matrix layers
def _bf16(a):
    import merge_oracle

    return merge_oracle.bf16_bits(np.ascontiguousarray(a, np.float32))


def _bf16_f32(a):
    return (_bf16(a).astype(np.uint32) << 16).view(np.float32)


def _bias_parts(b):
    """hi + mid + lo == b exactly, each a bf16 value."""
    b = np.asarray(b, np.float32)
    hi = _bf16_f32(b)
    r = (b - hi).astype(np.float32)
    mid = _bf16_f32(r)
    return hi, mid, (r - mid).astype(np.float32)


def _k_order(K):
    """The hidden unit at packed position k of a later layer: within a k-block of 32, k = 8 g + j holds unit
    32 kb + 16 (j >> 2) + 4 g + (j & 3)."""
    k = np.arange(K)
    kb, g, j = k >> 5, (k >> 3) & 3, k & 7
    return 32 * kb + 16 * (j >> 2) + 4 * g + (j & 3)


def _chain(x_bits, w_bits, c):
    """out[r, m] = the MFMA chain over k of x[r, k] w[m, k] from c[m]: x [n, K], w [M, K] bf16 bits."""
    import merge_oracle

    n, K = x_bits.shape
    M = w_bits.shape[0]
    a = np.broadcast_to(w_bits[None, :, :], (n, M, K)).reshape(n * M, K)
    b = np.broadcast_to(x_bits[:, None, :], (n, M, K)).reshape(n * M, K)
    c0 = np.broadcast_to(np.asarray(c, np.float32)[None, :], (n, M)).reshape(n * M)
    return merge_oracle.mfma_dots(a, b, c0).reshape(n, M)


def _hidden(acc):
    """One bf16 rounding, then max(., +0) (a negative zero becomes +0): the bf16 bits."""
    bits = _bf16(acc)
    return np.where(bits & 0x8000, np.uint16(0), bits).astype(np.uint16)


def logits_ref(eff, obs, rotate=0):
    """The head's inputs [n, 306] (value [51], advantage [5][51]) of observations [n, 10]."""
    obs = np.asarray(obs, np.float32)
    n = len(obs)
    x = np.zeros((n, 32), np.float32)
    x[:, :10] = obs[:, (np.arange(10) + rotate) % 10]
    x[:, 10:13] = 1.0
    w1 = np.zeros((32, 32), np.float32)
    w1[:, :10] = eff["linear1.weight"]
    for j, part in enumerate(_bias_parts(eff["linear1.bias"])):
        w1[:, 10 + j] = part
    h = _hidden(_chain(_bf16(x), _bf16(w1), np.zeros(32, np.float32)))

    def later(hbits, name):
        o = _k_order(hbits.shape[1])
        w = _bf16(eff[f"{name}.weight"])
        return _chain(np.ascontiguousarray(hbits[:, o]), np.ascontiguousarray(w[:, o]), eff[f"{name}.bias"])

    h = _hidden(later(h, "linear2"))
    hv = _hidden(later(h, "noisy_value1"))
    ha = _hidden(later(h, "noisy_advantage1"))
    return np.concatenate([later(hv, "noisy_value2"), later(ha, "noisy_advantage2")], axis=1)


def forward_ref(eff, obs, rotate=0):
    """(logits, q, action) of the whole restatement."""
    lg = logits_ref(eff, obs, rotate)
    q, act = head_ref(lg)
    return lg, q, act


@functools.lru_cache(maxsize=None)
def forward_fixture(seed, soft, rotate):
    """The restatement on every fixture observation for one recorded net and view, computed once."""
    lg, q, act = forward_ref(effective_ref(state_dict(seed, soft)), observations(), rotate)
    for a in (lg, q, act):
        a.setflags(write=False)
    return lg, q, act


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)
