"""The population's acting entry points without a GPU: mg_rollout_qnet_many, mg_replay_store_many and
mg_replay_scratch_many_bytes are exported and declared, ABI 21 and merging_gym.__all__ are unchanged, every
argument check fires before anything is launched (fake pointers, never dereferenced), nothing-to-do calls return
0, the scratch size follows the header's formula, and the host code runs under AddressSanitizer and
UndefinedBehaviorSanitizer in a stand-alone program."""

import ctypes
import inspect
import os
import re

import pytest

from conftest import ROOT
from native_build import hipcc, run_sanitized_driver

FAKE = 1 << 20  # never dereferenced: validation fails first


@pytest.fixture(scope="module")
def nat():
    from merging_gym import _native

    return _native


def test_symbols_are_exported_and_declared(nat):
    lib = nat.lib
    assert lib.mg_abi_version() == 21 and nat.ABI_VERSION == 21
    with open(os.path.join(ROOT, "include", "merging_hip.h")) as f:
        header = f.read()
    assert re.search(r"#define MG_ABI_VERSION 21\b", header)
    for name in ("mg_rollout_qnet_many", "mg_replay_store_many", "mg_replay_scratch_many_bytes"):
        assert hasattr(lib, name), name
        assert re.search(r"^(int|size_t) %s\(" % name, header, re.M), name
    assert "typedef struct mg_qnet_actor {" in header
    assert ctypes.sizeof(nat.QnetActor) == 40


def test_public_python_surface():
    import merging_gym
    from merging_gym import replay
    from merging_gym.envs.vector_env import MergeVecEnv

    assert merging_gym.__all__ == ["MergeEnv", "MergeEnvExtend", "MergeVecEnv", "ReplayRing", "DQNLearner",
                                   "RainbowNet", "RainbowReplay", "RainbowLearner", "make", "ENV_IDS"]

    def params(f, skip=1):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[skip:]]

    E = inspect.Parameter.empty
    assert params(MergeVecEnv.rollout_qnet_many) == [
        ("num_steps", E), ("qnets", E), ("seed", E), ("opponent", "none"), ("episilo", 0.7), ("opp_episilo", 0.7),
        ("first_step", None), ("final_observation", True), ("won_mask", True)]
    assert params(MergeVecEnv.member_summaries) == [("members", E)]
    assert params(replay.store_rollout_many, 0) == [("rings", E), ("obs_first", E), ("traj", E), ("skip_ego_won", True)]
    assert params(merging_gym.DQNPopulation.collect) == [
        ("env", E), ("num_steps", E), ("seed", None), ("opponent", "none"), ("episilo", 0.7), ("opp_episilo", 0.7),
        ("skip_ego_won", True)]
    assert "pop.collect(env, 16)" in inspect.getmodule(merging_gym.DQNPopulation).__doc__


def _actors(nat, M, edits=None):
    arr = (nat.QnetActor * max(M, 1))()
    for m in range(max(M, 1)):
        arr[m] = nat.QnetActor(FAKE + 4096 * m, FAKE + 4096 * m + 64, m, 1 << 31, 1 << 30)
    for (m, field), v in (edits or {}).items():
        setattr(arr[m], field, v)
    return arr


def test_rollout_many_argument_checks(nat):
    lib = nat.lib
    params = nat.default_params()
    state = nat.State(*([FAKE] * 7))
    traj = nat.Traj()
    good = dict(params=ctypes.byref(params), state=ctypes.byref(state), traj=ctypes.byref(traj), n_member=1088,
                members=3, num_steps=6, actors=_actors(nat, 3), out_dim=5, mode=0)

    def call(**kw):
        a = dict(good, **kw)
        return lib.mg_rollout_qnet_many(a["params"], a["state"], a["traj"], None, a["n_member"], a["members"], 0, 500,
                                        a["num_steps"], a["actors"], a["out_dim"], a["mode"], nat.AUTORESET, None)

    def refused(msg, **kw):
        assert call(**kw) != 0
        assert msg in lib.mg_last_error(), lib.mg_last_error()

    for n in (0, 65, -1):
        refused(b"mg_rollout_qnet_many: need 1 <= members <= 64", members=n)
    refused(b"mg_rollout_qnet_many: n_member < 0", n_member=-64)
    for n in (1, 63, 96, 1000):
        refused(b"n_member must be a multiple of 64 (a won-mask word covers 64 envs", n_member=n)
    refused(b"exceeds the grid limit", n_member=1 << 40)
    refused(b"params is NULL", params=None)
    refused(b"mg_state has a NULL array", state=None)
    refused(b"traj is NULL", traj=None)
    refused(b"actors is NULL", actors=None)
    refused(b"num_steps >= 0 and 1 <= out_dim <= 8", num_steps=-1)
    for d in (0, 9):
        refused(b"num_steps >= 0 and 1 <= out_dim <= 8", out_dim=d)
    for mode in (-1, 4):
        refused(b"opponent_mode must be 0 (None), 1 (uniform), 2 (same net) or 3", mode=mode)
    refused(b"member 1: net must be a 16-byte aligned packed Q-net", actors=_actors(nat, 3, {(1, "net"): None}))
    refused(b"member 2: net must be a 16-byte aligned packed Q-net", actors=_actors(nat, 3, {(2, "net"): FAKE + 8}), mode=2)
    refused(b"member 0: opponent_mode 3 needs opp_net", actors=_actors(nat, 3, {(0, "opp_net"): None}), mode=3)
    refused(b"member 2: opponent_mode 3 needs opp_net", actors=_actors(nat, 3, {(2, "opp_net"): FAKE + 4}), mode=3)
    assert call(actors=_actors(nat, 3, {(2, "opp_net"): None}), mode=2, num_steps=0) == 0  # read in mode 3 only
    bad_traj = nat.Traj(FAKE + 4)
    refused(b"traj.obs must be 16-byte", traj=ctypes.byref(bad_traj))
    # nothing to do is a success, with every other argument valid
    assert call(n_member=0) == 0 and call(num_steps=0) == 0 and call(n_member=0, mode=3) == 0


def test_store_many_argument_checks_and_scratch_size(nat):
    lib = nat.lib
    # the header's formula: members * mg_replay_scratch_bytes(n_member, num_steps); 0 outside 1 .. 64 members
    for n, T, M in ((320, 3, 3), (1088, 16, 64)):
        one = lib.mg_replay_scratch_bytes(n, T)
        nb = -(-n // 256) * T
        ng = -(-nb // 64)
        assert one == (8 + ng * 8 + nb * 4 + ng * 4 + 7) // 8 * 8
        assert lib.mg_replay_scratch_many_bytes(n, T, M) == M * one
    for M in (0, 65, -1):
        assert lib.mg_replay_scratch_many_bytes(320, 3, M) == 0
    assert lib.mg_replay_scratch_many_bytes(0, 3, 3) == 0 and lib.mg_replay_scratch_many_bytes(320, 0, 3) == 0

    def ptrs(M, edits=None):
        rows = (ctypes.c_void_p * max(M, 1))(*(FAKE + 65536 * (m + 1) for m in range(max(M, 1))))
        counters = (ctypes.c_void_p * max(M, 1))(*(FAKE + 8 * m for m in range(max(M, 1))))
        for (which, m), v in (edits or {}).items():
            (rows if which == "rows" else counters)[m] = v
        return rows, counters

    def transitions(**kw):
        f = dict(obs_first=FAKE, obs=FAKE, final_obs=FAKE, rew=FAKE, won_mask=FAKE, flags=FAKE)
        f.update(kw)
        return nat.Transitions(**f)

    sb = lib.mg_replay_scratch_many_bytes(320, 3, 3)
    good = dict(ptrs=ptrs(3), members=3, capacity=2000, row_floats=22, tr=transitions(), n_member=320, num_steps=3,
                scratch=FAKE, scratch_bytes=sb)

    def call(**kw):
        a = dict(good, **kw)
        rows, counters = a["ptrs"]
        return lib.mg_replay_store_many(rows, counters, a["members"], a["capacity"], a["row_floats"],
                                        None if a["tr"] is None else ctypes.byref(a["tr"]), a["n_member"],
                                        a["num_steps"], 1, a["scratch"], a["scratch_bytes"], None)

    def refused(msg, **kw):
        assert call(**kw) != 0
        err = lib.mg_last_error()
        assert msg in err and err.startswith(b"mg_replay_store_many: "), err

    for n in (0, 65, -1):
        refused(b"need 1 <= members <= 64", members=n)
    refused(b"NULL pointer", ptrs=(None, ptrs(3)[1]))
    refused(b"NULL pointer", ptrs=(ptrs(3)[0], None))
    refused(b"NULL pointer", tr=None)
    refused(b"NULL pointer (a member's rows or counter)", ptrs=ptrs(3, {("rows", 2): None}))
    refused(b"NULL pointer (a member's rows or counter)", ptrs=ptrs(3, {("counters", 1): None}))
    refused(b"rows and counter must be 8-byte aligned", ptrs=ptrs(3, {("rows", 1): FAKE + 4}))
    refused(b"rows and counter must be 8-byte aligned", ptrs=ptrs(3, {("counters", 2): FAKE + 4}))
    refused(b"a ring is listed twice", ptrs=ptrs(3, {("rows", 2): FAKE + 65536}))
    refused(b"a ring is listed twice", ptrs=ptrs(3, {("counters", 2): FAKE + 8}))
    refused(b"capacity < 1", capacity=0)
    refused(b"22-float rows only", row_floats=24)
    for name in ("goal", "next_goal", "meta_goal"):
        refused(b"22-float rows only", tr=transitions(**{name: FAKE}))
    refused(b"n_member < 0 or num_steps < 0", n_member=-64)
    refused(b"n_member < 0 or num_steps < 0", num_steps=-1)
    for n in (1, 100, 319):
        refused(b"n_member must be a multiple of 64", n_member=n)
    for name in ("obs_first", "obs", "rew"):
        refused(b"obs_first, obs, a1 (or flags) and rew are required", tr=transitions(**{name: None}))
    refused(b"obs_first, obs, a1 (or flags) and rew are required", tr=transitions(flags=None))
    for name in ("obs_first", "obs", "final_obs", "rew", "won_mask"):
        refused(b"must be 8-byte aligned", tr=transitions(**{name: FAKE + 4}))
    refused(b"must be 8-byte aligned", scratch=FAKE + 4)
    refused(b"reward must be 4-byte aligned", tr=transitions(reward=FAKE + 2))
    refused(b"scratch smaller than mg_replay_scratch_many_bytes", scratch=None)
    refused(b"scratch smaller than mg_replay_scratch_many_bytes", scratch_bytes=sb - 8)
    refused(b"num_steps too large", n_member=64, num_steps=200000,
            scratch_bytes=lib.mg_replay_scratch_many_bytes(64, 200000, 3))
    assert call(n_member=0, scratch=None, scratch_bytes=0) == 0
    assert call(num_steps=0, scratch=None, scratch_bytes=0) == 0


@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_population_acting_host_code_under_asan_ubsan(tmp_path):
    """tests/native/population_act_sanitize.cpp (its own main): every argument check of the two entry points at
    M = 1, 3 and 64 on exactly sized member lists. No GPU, nothing loaded into Python."""
    r = run_sanitized_driver("population_act_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "population_act sanitizer run: 0 failures" in r.stdout
