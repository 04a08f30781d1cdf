"""Helpers of the device-noise tests: the plain-C restatement of the stream (tests/native/rainbow_noise_ref.c,
compiled with the C compiler at test time and loaded with ctypes, as rainbow_learn_ref.py builds its own), the
library's host twins as numpy calls, and the inputs the CPU and the GPU tests share."""

from __future__ import annotations

import ctypes
import functools
import math
import os
import subprocess
import tempfile

import numpy as np

from learn_ref import bits, cc  # noqa: F401  (re-exported)

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "native", "rainbow_noise_ref.c")
NF = 1124
# (noise_seed, first_update, U): the plain case, the update index crossing the counter's low word, a 64-bit seed
CASES = ((0, 0, 1), (11, 2 ** 32 - 1, 3), (2 ** 63 + 5, 0, 3))

_u64, _i64, _i32, _P = ctypes.c_uint64, ctypes.c_int64, ctypes.c_int32, ctypes.c_void_p


@functools.lru_cache(maxsize=1)
def build_ref():
    out = os.path.join(tempfile.mkdtemp(prefix="rainbow_noise_ref."), "librainbow_noise_ref.so")
    subprocess.check_call([cc(), "-O2", "-std=c11", "-fPIC", "-shared", "-ffp-contract=off", "-fno-fast-math",
                           "-Wall", "-o", out, SRC, "-lm"])
    lib = ctypes.CDLL(out)
    lib.noise_ref.argtypes = [_u64, _u64, _i32, _P]
    lib.noise_ref.restype = None
    lib.uniform_ref_fill.argtypes = [_u64, _u64, _i32, _P]
    lib.uniform_ref_fill.restype = None
    lib.ndtri_ref.argtypes = [_P, _P, _i64]
    lib.ndtri_ref.restype = None
    return lib


def noise_ref(noise_seed, first_update, U):
    """[U, 2, 1124] fp32 of the restatement."""
    out = np.zeros((U, 2, NF), np.float32)
    build_ref().noise_ref(noise_seed, first_update, U, out.ctypes.data)
    return out


def uniforms_ref(noise_seed, first_update, U):
    """[U, 2, 1124] fp64: the restatement's uniforms (steps 1 and 2 of the contract)."""
    out = np.zeros((U, 2, NF), np.float64)
    build_ref().uniform_ref_fill(noise_seed, first_update, U, out.ctypes.data)
    return out


def ndtri_ref(u):
    u = np.ascontiguousarray(u, dtype=np.float64)
    z = np.zeros_like(u)
    build_ref().ndtri_ref(u.ctypes.data, z.ctypes.data, u.size)
    return z


def noise_host(noise_seed, first_update, U):
    """[U, 2, 1124] fp32 of mg_host_rainbow_noise."""
    from merging_gym import _native

    out = np.zeros((U, 2, NF), np.float32)
    _native.check(_native.lib.mg_host_rainbow_noise(noise_seed, first_update, U, out.ctypes.data),
                  "mg_host_rainbow_noise")
    return out


def ndtri_host(u):
    from merging_gym import _native

    u = np.ascontiguousarray(u, dtype=np.float64)
    z = np.zeros_like(u)
    _native.check(_native.lib.mg_host_rainbow_ndtri(u.ctypes.data, z.ctypes.data, u.size), "mg_host_rainbow_ndtri")
    return z


def _neighbours(x):
    return [np.nextafter(x, 0.0), x, np.nextafter(x, 1.0)]


@functools.lru_cache(maxsize=1)
def edge_uniforms():
    """The inverse CDF's edge list: the branch edges 0.5 -+ 0.425 and e^-25, 1 - e^-25 with their fp64
    neighbours, then 2^-53, 1 - 2^-53 and 0.5 * 2^-52 (the stream's smallest uniform)."""
    tail = math.exp(-25.0)
    u = []
    for x in (0.5 - 0.425, 0.5 + 0.425, tail, 1.0 - tail):
        u += _neighbours(np.float64(x))
    u += [2.0 ** -53, 1.0 - 2.0 ** -53, 0.5 * 2.0 ** -52]
    u = np.array(u, dtype=np.float64)
    u.setflags(write=False)
    return u


@functools.lru_cache(maxsize=1)
def stream_uniforms():
    """4,096 uniforms of the stream (the restatement's, seed 11 from update 2^32 - 1), read-only."""
    u = uniforms_ref(*CASES[1]).reshape(-1)[:4096].copy()
    u.setflags(write=False)
    return u


def same_bits(a, b):
    """Bit for bit, NaNs included."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    view = np.uint64 if a.dtype == np.float64 else np.uint32
    return a.shape == b.shape and a.dtype == b.dtype and bool(np.array_equal(a.view(view), b.view(view)))
