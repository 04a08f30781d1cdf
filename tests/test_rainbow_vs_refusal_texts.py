"""The exact text of every refusal of the Rainbow rollouts against another net: mg_rollout_rainbow_vs and
mg_rollout_rainbow_vs_many.

The argument checks run before anything is read or launched, so fake, never-dereferenced pointers drive both entries
on a host without a GPU. Each row names the arguments that differ from a call that would pass every check and the
whole mg_last_error() text (the return code is hipErrorInvalidValue, 1). A row with two bad arguments pins which
check fires first. The checks of params, state, traj and its buffers are the siblings' own
(mg_rollout_rainbow / mg_rollout_rainbow_many), text for text; the net, opponent and num_steps texts start with the
entry point's name, and the member call names the first offending member.

No row passes every check with something to do: such a call would launch on the fake pointers.
"""
import ctypes
import os
import re

import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2
GRID = 0x7fffffff * 256  # the most envs a grid of 256-thread blocks covers; a multiple of 64

VS, MANY = "mg_rollout_rainbow_vs", "mg_rollout_rainbow_vs_many"

R_PARAMS = b"params is NULL"
R_TIMEOUT = b"mg_params: timeout_steps must be in 1..8191 (the step count of mg_state.tf saturates at 8191)"
R_STATE = b"mg_state has a NULL array"
R_TRAJ = b"traj is NULL (pass a zeroed mg_traj)"
R_ALIGN = b"traj.obs must be 16-byte, rew/final_obs 8-byte, flags 4-byte aligned"
R_N = b"n < 0"

V = b"mg_rollout_rainbow_vs: "
V_NET = V + b"net must be a 16-byte aligned packed Rainbow net"
V_OPP = V + b"opponent must be a 16-byte aligned packed Rainbow net"
V_STEPS = V + b"need 0 <= num_steps <= 65535 (split longer rollouts)"

M_ = b"mg_rollout_rainbow_vs_many: "
M_MEMBERS = M_ + b"need 1 <= members <= 64"
M_NEG = M_ + b"n_member < 0"
M_64 = M_ + (b"n_member must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so no two "
             b"members may share one)")
M_GRID = M_ + b"members * n_member exceeds the grid limit"
M_NETS = M_ + b"nets is NULL (members packed Rainbow nets)"
M_OPPS = M_ + b"opponents is NULL (members packed Rainbow nets)"
M_NET = M_ + b"member %d: net must be a 16-byte aligned packed Rainbow net"
M_OPP = M_ + b"member %d: opponent must be a 16-byte aligned packed Rainbow net"
M_STEPS = M_ + b"need 0 <= num_steps <= 65535 (split longer rollouts)"


def _past_grid(members):
    """The first multiple of 64 with members * n_member past the grid limit."""
    return (GRID // members // 64 + 1) * 64


# (case, overrides, mg_last_error()), in the entry point's order of checks
VS_TABLE = [
    ("params NULL", dict(no_params=True), R_PARAMS),
    ("params.timeout_steps = 0", dict(params=dict(timeout_steps=0)), R_TIMEOUT),
    ("n < 0", dict(n=-1), R_N),
    ("state NULL", dict(no_state=True), R_STATE),
    ("state array NULL", dict(state=dict(tf=None)), R_STATE),
    ("traj NULL", dict(no_traj=True), R_TRAJ),
    ("net NULL", dict(net=None), V_NET),
    ("net misaligned", dict(net=ODD8), V_NET),
    ("opponent NULL", dict(opp=None), V_OPP),
    ("opponent misaligned", dict(opp=ODD8), V_OPP),
    ("num_steps < 0", dict(num_steps=-1), V_STEPS),
    ("num_steps 65536", dict(num_steps=65536), V_STEPS),
    ("traj.obs misaligned", dict(traj=dict(obs=ODD8)), R_ALIGN),
    ("traj.final_obs misaligned", dict(traj=dict(final_obs=ODD4)), R_ALIGN),
    ("traj.rew misaligned", dict(traj=dict(rew=ODD4)), R_ALIGN),
    ("traj.flags misaligned", dict(traj=dict(flags=ODD2)), R_ALIGN),
    ("params before state", dict(no_params=True, no_state=True), R_PARAMS),
    ("traj before the net", dict(no_traj=True, net=None), R_TRAJ),
    ("the net before the opponent", dict(net=ODD8, opp=None), V_NET),
    ("the opponent before num_steps", dict(opp=None, num_steps=-1), V_OPP),
    ("num_steps before alignment", dict(num_steps=65536, traj=dict(rew=ODD4)), V_STEPS),
    ("alignment before the empty call", dict(num_steps=0, traj=dict(flags=ODD2)), R_ALIGN),
    ("alignment before the empty batch", dict(n=0, traj=dict(obs=ODD8)), R_ALIGN),
]

MANY_TABLE = [
    ("members 0", dict(members=0), M_MEMBERS),
    ("members 65", dict(members=65), M_MEMBERS),
    ("members -1", dict(members=-1), M_MEMBERS),
    ("n_member < 0", dict(n=-64), M_NEG),
    ("n_member 1", dict(n=1), M_64),
    ("n_member 96", dict(n=96), M_64),
    ("members * n_member past the grid", dict(n=_past_grid(3)), M_GRID),
    ("64 members past the grid", dict(members=64, n=_past_grid(64)), M_GRID),
    ("params NULL", dict(no_params=True), R_PARAMS),
    ("params.timeout_steps = 0", dict(params=dict(timeout_steps=0)), R_TIMEOUT),
    ("state NULL", dict(no_state=True), R_STATE),
    ("state array NULL", dict(state=dict(tf=None)), R_STATE),
    ("traj NULL", dict(no_traj=True), R_TRAJ),
    ("nets NULL", dict(no_nets=True), M_NETS),
    ("member 0's net NULL", dict(nets={0: None}), M_NET % 0),
    ("member 2's net misaligned", dict(nets={2: ODD8}), M_NET % 2),
    ("opponents NULL", dict(no_opps=True), M_OPPS),
    ("member 0's opponent NULL", dict(opps={0: None}), M_OPP % 0),
    ("member 1's opponent NULL", dict(opps={1: None}), M_OPP % 1),
    ("member 2's opponent misaligned", dict(opps={2: ODD8}), M_OPP % 2),
    ("num_steps < 0", dict(num_steps=-1), M_STEPS),
    ("num_steps 65536", dict(num_steps=65536), M_STEPS),
    ("traj.obs misaligned", dict(traj=dict(obs=ODD8)), R_ALIGN),
    ("traj.final_obs misaligned", dict(traj=dict(final_obs=ODD4)), R_ALIGN),
    ("traj.rew misaligned", dict(traj=dict(rew=ODD4)), R_ALIGN),
    ("traj.flags misaligned", dict(traj=dict(flags=ODD2)), R_ALIGN),
    ("members before n_member", dict(members=0, n=-64), M_MEMBERS),
    ("n_member < 0 before its multiple", dict(n=-1), M_NEG),
    ("n_member's multiple before the grid", dict(n=_past_grid(3) + 1), M_64),
    ("grid before params", dict(n=_past_grid(3), no_params=True), M_GRID),
    ("params before state", dict(no_params=True, no_state=True), R_PARAMS),
    ("state before traj", dict(no_state=True, no_traj=True), R_STATE),
    ("traj before nets", dict(no_traj=True, no_nets=True), R_TRAJ),
    ("nets before opponents", dict(no_nets=True, no_opps=True), M_NETS),
    ("a member's net before opponents NULL", dict(nets={2: None}, no_opps=True), M_NET % 2),
    ("member 2's net before member 0's opponent", dict(nets={2: ODD8}, opps={0: None}), M_NET % 2),
    ("member 0's opponent before member 1's", dict(opps={0: ODD8, 1: None}), M_OPP % 0),
    ("the opponents before num_steps", dict(opps={2: None}, num_steps=-1), M_OPP % 2),
    ("num_steps before alignment", dict(num_steps=65536, traj=dict(rew=ODD4)), M_STEPS),
    ("alignment before the empty call", dict(num_steps=0, traj=dict(flags=ODD2)), R_ALIGN),
    ("alignment before the empty batch", dict(n=0, traj=dict(obs=ODD8)), R_ALIGN),
]


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _struct(cls, fields):
    return cls(**{k: _ptr(v) for k, v in fields.items()})


def _batch(g):
    from merging_gym import _native

    P = _native.default_params()
    for k, v in g("params", {}).items():
        setattr(P, k, v)
    P = None if g("no_params", False) else ctypes.byref(P)
    state = {k: FAKE for k, _ in _native.State._fields_}
    state.update(g("state", {}))
    st = None if g("no_state", False) else ctypes.byref(_struct(_native.State, state))
    traj = None if g("no_traj", False) else ctypes.byref(_struct(_native.Traj, g("traj", {})))
    return P, st, traj


def _call_vs(over):
    """mg_rollout_rainbow_vs with arguments that pass every check, except for `over`: (return, error text)."""
    from merging_gym import _native

    a = dict(over)
    g = a.pop
    P, st, traj = _batch(g)
    args = (P, st, traj, None, g("n", 128), g("num_steps", 4), g("net", FAKE + 131072), g("opp", FAKE + 262144), 1,
            None)
    assert not a, f"unknown overrides {a}"
    rc = _native.lib.mg_rollout_rainbow_vs(*args)
    return rc, _native.lib.mg_last_error()


def _call_many(over):
    """mg_rollout_rainbow_vs_many with arguments that pass every check, except for `over`."""
    from merging_gym import _native

    a = dict(over)
    g = a.pop
    members = g("members", 3)
    count = min(max(members, 1), 64)  # entries the lists hold: a refused member count reads none of them
    P, st, traj = _batch(g)
    nets = (ctypes.c_void_p * count)(*(FAKE + 131072 * m for m in range(count)))
    opps = (ctypes.c_void_p * count)(*(FAKE + 131072 * ((m + 1) % count) for m in range(count)))
    for lst, name in ((nets, "nets"), (opps, "opps")):
        for m, v in g(name, {}).items():
            lst[m] = v
    args = (P, st, traj, None, g("n", 128), members, g("num_steps", 4), None if g("no_nets", False) else nets,
            None if g("no_opps", False) else opps, 1, None)
    assert not a, f"unknown overrides {a}"
    rc = _native.lib.mg_rollout_rainbow_vs_many(*args)
    return rc, _native.lib.mg_last_error()


@pytest.mark.parametrize("case,over,text", VS_TABLE, ids=[r[0] for r in VS_TABLE])
def test_lone_refusal(case, over, text):
    assert _call_vs(over) == (1, text)


@pytest.mark.parametrize("case,over,text", MANY_TABLE, ids=[r[0] for r in MANY_TABLE])
def test_member_refusal(case, over, text):
    assert _call_many(over) == (1, text)


@pytest.mark.parametrize("call,table", [(_call_vs, VS_TABLE), (_call_many, MANY_TABLE)], ids=[VS, MANY])
def test_nothing_to_do_returns_0_behind_every_check_only(call, table):
    """n == 0 and num_steps == 0 succeed with every argument valid (an opponent equal to the net too); a fault of
    any check is still refused with its own text: every check precedes that return, and so any device work."""
    empties = (dict(n=0), dict(num_steps=0))
    for empty in empties:
        assert call(empty)[0] == 0
    assert _call_vs(dict(num_steps=0, opp=FAKE + 131072))[0] == 0
    assert _call_many(dict(num_steps=0, opps={0: FAKE, 1: FAKE, 2: FAKE}))[0] == 0
    for case, over, text in table:
        for empty in empties:
            if not set(empty) & set(over):
                assert call(dict(over, **empty)) == (1, text), (case, empty)


def test_member_count_boundaries():
    """0 and 65 members are refused (the table); 1 and 64 pass the member count and every per-member check on
    exactly sized lists."""
    for members in (1, 64):
        last = members - 1
        assert _call_many(dict(members=members, num_steps=0))[0] == 0
        assert _call_many(dict(members=members, nets={last: ODD8})) == (1, M_NET % last)
        assert _call_many(dict(members=members, opps={last: None})) == (1, M_OPP % last)
        assert _call_many(dict(members=members, n=_past_grid(members))) == (1, M_GRID)
        assert _call_many(dict(members=members, n=_past_grid(members) - 64, no_params=True)) == (1, R_PARAMS)


def test_the_siblings_keep_refusing_mode_3():
    """The new calls are beside the old ones: opponent_mode 3 of mg_rollout_rainbow / _many stays refused."""
    from merging_gym import _native

    st = ctypes.byref(_struct(_native.State, {k: FAKE for k, _ in _native.State._fields_}))
    P, traj = ctypes.byref(_native.default_params()), ctypes.byref(_native.Traj())
    rc = _native.lib.mg_rollout_rainbow(P, st, traj, None, 128, 4, FAKE, 3, 1, None)
    assert (rc, _native.lib.mg_last_error()) == (
        1, b"mg_rollout_rainbow: opponent_mode must be 0 (None) or 2 (the same net on state[3:] + state[:3])")
    nets = (ctypes.c_void_p * 2)(FAKE, FAKE + 131072)
    rc = _native.lib.mg_rollout_rainbow_many(P, st, traj, None, 64, 2, 4, nets, 3, 1, None)
    assert (rc, _native.lib.mg_last_error()) == (
        1, b"mg_rollout_rainbow_many: opponent_mode must be 0 (None) or 2 (the same net on state[3:] + state[:3])")


def test_abi_version_stays_21():
    from merging_gym import _native

    assert _native.lib.mg_abi_version() == 21 == _native.ABI_VERSION


def test_header_declares_and_library_exports_both_entries():
    from merging_gym import _native

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "merging_hip.h")
    with open(header) as f:
        text = f.read()
    index = text[:text.index("#ifndef MERGING_HIP_H_")]
    for name, nargs in ((VS, 10), (MANY, 11)):
        assert re.search(r"^int %s\(" % name, text, re.M), f"{name} is not declared"
        assert name in index, f"{name} is not in the header's index"
        f = getattr(_native.lib, name)  # an AttributeError here: the library does not export it
        assert f.argtypes is not None and len(f.argtypes) == nargs
        assert f.restype is ctypes.c_int
