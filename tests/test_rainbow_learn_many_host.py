"""mg_host_rainbow_learn_many and mg_host_rainbow_noise_many without a GPU: the population's host twin against the
plain-C restatement run once per member, bit for bit, with members that differ in every field; the population's
noise against mg_host_rainbow_noise per member; the counters a call leaves behind."""

import ctypes

import numpy as np
import pytest

import rainbow_learn_many_ref as many
from learn_ref import bits

U = 3
CASES = [(1, 2), (5, 3), (33, 3), (32, 4)]  # (batch, members); 33: a member stride rounded as rl_scratch's sections


@pytest.fixture(scope="module")
def runs():
    """Per case, computed once: (settings, host outputs, restatement outputs)."""
    cache = {}

    def get(B, M):
        if (B, M) not in cache:
            settings, ring_list = many.member_settings(M), many.rings(M)
            L, nf = many.learners(M), many.noise(U, M)
            cache[B, M] = (settings, many.run_host_members(L, settings, ring_list, B, U, nf),
                           many.run_ref_members(L, settings, ring_list, B, U, nf))
        return cache[B, M]

    return get


@pytest.mark.parametrize("B,M", CASES)
def test_every_member_equals_the_restatement(runs, B, M):
    _, got, want = runs(B, M)
    many.assert_members_same(got, want)


@pytest.mark.parametrize("B,M", CASES)
def test_the_members_differ(runs, B, M):
    """The comparison above is not of M copies: no two members end with the same current model or loss."""
    _, got, _ = runs(B, M)
    for a in range(M):
        for b in range(a + 1, M):
            assert (bits(got[0][a]) != bits(got[0][b])).any()
            assert (bits(got[1][:, a]) != bits(got[1][:, b])).any()


def test_counters_advance_by_the_updates(runs):
    settings, got, _ = runs(5, 3)
    for s, e in zip(settings, got[5]):
        assert (int(e.first_update), int(e.first_draw)) == (s["first_update"] + U, s["first_draw"] + U)
        assert int(e.seed) == s["seed"]


def test_k_updates_in_one_call_equal_k_calls(runs):
    settings, got, _ = runs(5, 3)
    again = many.run_host_members(many.learners(3), settings, many.rings(3), 5, U, many.noise(U, 3), calls=[2, 0, 1])
    many.assert_members_same(again, got)
    assert [int(e.first_update) for e in again[5]] == [int(e.first_update) for e in got[5]]


def test_a_refused_call_leaves_the_counters():
    from merging_gym import _native

    settings = many.member_settings(2)
    members = many.member_array(settings, [1 << 20] * 2, [1 << 20] * 2)
    rc = _native.lib.mg_host_rainbow_learn_many(ctypes.c_void_p(1 << 20), members, 2, 64, 0, 3, ctypes.c_void_p(1 << 20),
                                                None, None, None, None, ctypes.c_void_p(1 << 20), 1 << 30)
    assert rc == 1 and _native.lib.mg_last_error() == b"mg_host_rainbow_learn_many: need 1 <= batch <= 1024"
    for s, e in zip(settings, members):
        assert (int(e.first_update), int(e.first_draw)) == (s["first_update"], s["first_draw"])


def test_noise_many_equals_the_lone_noise_per_member():
    """Unequal first_update, one seed >= 2^63 and one first_update >= 2^32: the 64-bit words arrive whole."""
    from merging_gym import _native
    from merging_gym.rainbow_learn import device_noise_factors

    seeds = np.array([7, (1 << 63) + 12345, 99], dtype=np.uint64)
    first = np.array([0, 3, (1 << 32) + 5], dtype=np.uint64)
    out = np.full((U, 3, 2, many.NF), np.nan, np.float32)
    rc = _native.lib.mg_host_rainbow_noise_many(seeds.ctypes.data, first.ctypes.data, 3, U, out.ctypes.data)
    _native.check(rc, "mg_host_rainbow_noise_many")
    for m in range(3):
        want = device_noise_factors(U, int(seeds[m]), int(first[m])).numpy()
        assert (bits(out[:, m]) == bits(want)).all(), f"member {m}"
    assert (bits(out[:, 0]) != bits(out[:, 2])).any()
    # no update: nothing is written
    out[:] = 5.0
    assert _native.lib.mg_host_rainbow_noise_many(seeds.ctypes.data, first.ctypes.data, 3, 0, out.ctypes.data) == 0
    assert (out == 5.0).all()
