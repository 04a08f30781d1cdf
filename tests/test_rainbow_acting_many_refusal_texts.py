"""The exact text of every refusal of the Rainbow population's acting entry points: mg_rollout_rainbow_many,
mg_rainbow_replay_store_many and its host twin mg_host_rainbow_replay_store_many.

The argument checks run before anything is read or launched, so fake, never-dereferenced pointers drive the two
device entries on a host without a GPU; the host twin gets real rings and counters, and every refused call must
leave the counters as they were. Each row names an entry point, the arguments that differ from a call that would
pass every check, and the whole mg_last_error() text (the return code is hipErrorInvalidValue, 1). A row with two
bad arguments pins which check fires first. Where a lone counterpart exists (mg_rollout_rainbow,
mg_rainbow_replay_store) the words and the order are its own, with the member entry's name in front.

No row passes every check of a device entry with something to do: such a call would launch on the fake pointers.
"""
import ctypes
import os
import re

import numpy as np
import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2
GRID = 0x7fffffff * 256  # the most envs a grid of 256-thread blocks covers; a multiple of 64

ROLL, STORE, HOST = "mg_rollout_rainbow_many", "mg_rainbow_replay_store_many", "mg_host_rainbow_replay_store_many"

R = b"mg_rollout_rainbow_many: "
R_MEMBERS = R + b"need 1 <= members <= 64"
R_NEG = R + b"n_member < 0"
R_64 = R + (b"n_member must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so no two "
            b"members may share one)")
R_GRID = R + b"members * n_member exceeds the grid limit"
R_PARAMS = b"params is NULL"
R_TIMEOUT = b"mg_params: timeout_steps must be in 1..8191 (the step count of mg_state.tf saturates at 8191)"
R_STATE = b"mg_state has a NULL array"
R_TRAJ = b"traj is NULL (pass a zeroed mg_traj)"
R_NETS = R + b"nets is NULL (members packed Rainbow nets)"
R_NET = R + b"member %d: net must be a 16-byte aligned packed Rainbow net"
R_STEPS = R + b"need 0 <= num_steps <= 65535 (split longer rollouts)"
R_MODE = R + b"opponent_mode must be 0 (None) or 2 (the same net on state[3:] + state[:3])"
R_ALIGN = b"traj.obs must be 16-byte, rew/final_obs 8-byte, flags 4-byte aligned"


def _store_texts(entry):
    s = entry.encode() + b": "
    return dict(
        MEMBERS=s + b"need 1 <= members <= 64", NULL=s + b"NULL pointer",
        NULL1=s + b"NULL pointer (a member's rows or counter)",
        AL1=s + b"every member's rows and counter must be 8-byte aligned",
        TWICE=s + b"a ring is listed twice (two members' appends to one ring have no defined order)",
        CAP=s + b"need 1 <= capacity <= 2^32", NEG=s + b"n_member < 0 or num_steps < 0",
        GOAL=s + b"goal, next_goal, reward and meta_goal must be NULL (Rainbow rows have none)",
        REQ=s + b"obs_first, obs, a1 (or flags) and rew are required",
        AL4=s + b"the float buffers must be 4-byte aligned", GRID=s + b"n_member * num_steps exceeds the grid limit")


def _past_grid(members):
    """The first multiple of 64 with members * n_member past the grid limit."""
    return (GRID // members // 64 + 1) * 64


# (case, overrides, mg_last_error()), in the entry point's order of checks
ROLL_TABLE = [
    ("members 0", dict(members=0), R_MEMBERS),
    ("members 65", dict(members=65), R_MEMBERS),
    ("members -1", dict(members=-1), R_MEMBERS),
    ("n_member < 0", dict(n=-64), R_NEG),
    ("n_member 1", dict(n=1), R_64),
    ("n_member 1000", dict(n=1000), R_64),
    ("members * n_member past the grid", dict(n=_past_grid(3)), R_GRID),
    ("64 members past the grid", dict(members=64, n=_past_grid(64)), R_GRID),
    ("params NULL", dict(no_params=True), R_PARAMS),
    ("params.timeout_steps = 0", dict(params=dict(timeout_steps=0)), R_TIMEOUT),
    ("state NULL", dict(no_state=True), R_STATE),
    ("state array NULL", dict(state=dict(tf=None)), R_STATE),
    ("traj NULL", dict(no_traj=True), R_TRAJ),
    ("nets NULL", dict(no_nets=True), R_NETS),
    ("member 0's net NULL", dict(nets={0: None}), R_NET % 0),
    ("member 1's net NULL", dict(nets={1: None}), R_NET % 1),
    ("member 2's net misaligned", dict(nets={2: ODD8}), R_NET % 2),
    ("num_steps < 0", dict(num_steps=-1), R_STEPS),
    ("num_steps 65536", dict(num_steps=65536), R_STEPS),
    ("mode 1", dict(mode=1), R_MODE),
    ("mode 3", dict(mode=3), R_MODE),
    ("mode -1", dict(mode=-1), R_MODE),
    ("traj.obs misaligned", dict(traj=dict(obs=ODD8)), R_ALIGN),
    ("traj.final_obs misaligned", dict(traj=dict(final_obs=ODD4)), R_ALIGN),
    ("traj.rew misaligned", dict(traj=dict(rew=ODD4)), R_ALIGN),
    ("traj.flags misaligned", dict(traj=dict(flags=ODD2)), R_ALIGN),
    ("members before n_member", dict(members=0, n=-64), R_MEMBERS),
    ("n_member < 0 before its multiple", dict(n=-1), R_NEG),
    ("n_member's multiple before the grid", dict(n=_past_grid(3) + 1), R_64),
    ("grid before params", dict(n=_past_grid(3), no_params=True), R_GRID),
    ("params before state", dict(no_params=True, no_state=True), R_PARAMS),
    ("state before traj", dict(no_state=True, no_traj=True), R_STATE),
    ("traj before nets", dict(no_traj=True, no_nets=True), R_TRAJ),
    ("nets before a member's net", dict(no_nets=True, num_steps=-1), R_NETS),
    ("member 0's net before member 1's", dict(nets={0: ODD8, 1: None}), R_NET % 0),
    ("the nets before num_steps", dict(nets={2: None}, num_steps=-1), R_NET % 2),
    ("num_steps before the mode", dict(num_steps=65536, mode=1), R_STEPS),
    ("the mode before alignment", dict(mode=1, traj=dict(rew=ODD4)), R_MODE),
    ("alignment before the empty call", dict(num_steps=0, traj=dict(flags=ODD2)), R_ALIGN),
    ("alignment before the empty batch", dict(n=0, traj=dict(obs=ODD8)), R_ALIGN),
]

# the store's rows: the texts carry the entry's name, so one table serves the device entry and the host twin
STORE_TABLE = [
    ("members 0", dict(members=0), "MEMBERS"),
    ("members 65", dict(members=65), "MEMBERS"),
    ("members -1", dict(members=-1), "MEMBERS"),
    ("rows NULL", dict(no_rows=True), "NULL"),
    ("counters NULL", dict(no_counters=True), "NULL"),
    ("tr NULL", dict(no_tr=True), "NULL"),
    ("member 2's rows NULL", dict(rows={2: None}), "NULL1"),
    ("member 1's counter NULL", dict(counters={1: None}), "NULL1"),
    ("member 1's rows misaligned", dict(rows={1: "odd"}), "AL1"),
    ("member 2's counter misaligned", dict(counters={2: "odd"}), "AL1"),
    ("member 2's rows are member 0's", dict(rows={2: 0}), "TWICE"),
    ("member 2's counter is member 1's", dict(counters={2: 1}), "TWICE"),
    ("capacity 0", dict(capacity=0), "CAP"),
    ("capacity 2^32 + 1", dict(capacity=(1 << 32) + 1), "CAP"),
    ("n_member < 0", dict(n=-1), "NEG"),
    ("num_steps < 0", dict(num_steps=-1), "NEG"),
    ("goal set", dict(tr=dict(goal=FAKE)), "GOAL"),
    ("next_goal set", dict(tr=dict(next_goal=FAKE)), "GOAL"),
    ("reward set", dict(tr=dict(reward=FAKE)), "GOAL"),
    ("meta_goal set", dict(tr=dict(meta_goal=FAKE)), "GOAL"),
    ("obs_first NULL", dict(tr=dict(obs_first=None)), "REQ"),
    ("obs NULL", dict(tr=dict(obs=None)), "REQ"),
    ("neither a1 nor flags", dict(tr=dict(flags=None)), "REQ"),
    ("rew NULL", dict(tr=dict(rew=None)), "REQ"),
    ("obs_first misaligned", dict(tr=dict(obs_first=ODD2)), "AL4"),
    ("obs misaligned", dict(tr=dict(obs=ODD2)), "AL4"),
    ("final_obs misaligned", dict(tr=dict(final_obs=ODD2)), "AL4"),
    ("rew misaligned", dict(tr=dict(rew=ODD2)), "AL4"),
    ("n_member past the grid", dict(n=GRID // 3 + 1), "GRID"),
    ("members before NULL", dict(members=65, no_rows=True), "MEMBERS"),
    ("NULL before a member's NULL", dict(no_tr=True, rows={0: None}), "NULL"),
    ("a member's NULL before its alignment", dict(rows={1: "odd"}, counters={1: None}), "NULL1"),
    ("a member's alignment before its twin", dict(rows={1: 0}, counters={1: "odd"}), "AL1"),
    ("member 0's alignment before member 1's NULL", dict(rows={0: "odd"}, counters={1: None}), "AL1"),
    ("member 1's twin before member 2's NULL", dict(rows={1: 0, 2: None}), "TWICE"),
    ("the member list before capacity", dict(counters={2: 1}, capacity=0), "TWICE"),
    ("capacity before n_member", dict(capacity=0, n=-1), "CAP"),
    ("n_member before the goals", dict(n=-1, tr=dict(goal=FAKE)), "NEG"),
    ("the goals before the empty call", dict(tr=dict(reward=FAKE), num_steps=0), "GOAL"),
    ("required before alignment", dict(tr=dict(rew=None, obs=ODD2)), "REQ"),
    ("alignment before the grid", dict(tr=dict(rew=ODD2), n=GRID // 3 + 1), "AL4"),
]
# refused only behind the return of a call with nothing to do
STORE_BEHIND_EMPTY = [dict(tr=dict(obs=None)), dict(tr=dict(rew=ODD2))]


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _struct(cls, fields):
    return cls(**{k: _ptr(v) for k, v in fields.items()})


def _call_roll(over):
    """mg_rollout_rainbow_many with arguments that pass every check, except for `over`: (return, error text)."""
    from merging_gym import _native

    a = dict(over)
    g = a.pop
    members = g("members", 3)
    count = min(max(members, 1), 64)  # entries the list holds: a refused member count reads none of them
    P = _native.default_params()
    for k, v in g("params", {}).items():
        setattr(P, k, v)
    P = None if g("no_params", False) else ctypes.byref(P)
    state = {k: FAKE for k, _ in _native.State._fields_}
    state.update(g("state", {}))
    st = None if g("no_state", False) else ctypes.byref(_struct(_native.State, state))
    traj = None if g("no_traj", False) else ctypes.byref(_struct(_native.Traj, g("traj", {})))
    nets = (ctypes.c_void_p * count)(*(FAKE + 131072 * m for m in range(count)))
    for m, v in g("nets", {}).items():
        nets[m] = v
    args = (P, st, traj, None, g("n", 128), members, g("num_steps", 4), None if g("no_nets", False) else nets,
            g("mode", 2), 1, None)
    assert not a, f"unknown overrides {a}"
    rc = _native.lib.mg_rollout_rainbow_many(*args)
    return rc, _native.lib.mg_last_error()


def _call_store(entry, over):
    """A store entry with arguments that pass every check, except for `over`: (return, error text, the counters
    before and after -- real host memory for the host twin, whose rings are real too)."""
    from merging_gym import _native

    a = dict(over)
    g = a.pop
    members = g("members", 3)
    count = min(max(members, 1), 64)
    host = entry == HOST
    n, T, capacity = g("n", 2), g("num_steps", 3), g("capacity", 50)
    keep = []
    if host:
        rings = [np.zeros((50, 24), np.float32) for _ in range(count)]
        ctr = np.arange(count, dtype=np.uint64) + 5
        row_at = [r.ctypes.data for r in rings]
        ctr_at = [ctr.ctypes.data + 8 * m for m in range(count)]
        keep += rings
    else:
        ctr = None
        row_at = [FAKE + 65536 * (m + 1) for m in range(count)]
        ctr_at = [FAKE + 8 * m for m in range(count)]
    rows, counters = (ctypes.c_void_p * count)(*row_at), (ctypes.c_void_p * count)(*ctr_at)
    for lst, at, name in ((rows, row_at, "rows"), (counters, ctr_at, "counters")):
        for m, v in g(name, {}).items():  # None, "odd" (this member's own pointer + 4) or another member's index
            lst[m] = None if v is None else at[m] + 4 if v == "odd" else at[v]
    tr = dict(obs_first=FAKE, obs=FAKE, final_obs=FAKE, rew=FAKE, flags=FAKE)
    tr.update(g("tr", {}))
    tr = None if g("no_tr", False) else ctypes.byref(_struct(_native.Transitions, tr))
    args = (None if g("no_rows", False) else rows, None if g("no_counters", False) else counters, members, capacity,
            tr, n, T) + (() if host else (None,))
    assert not a, f"unknown overrides {a}"
    before = None if ctr is None else ctr.copy()
    rc = getattr(_native.lib, entry)(*args)
    text = _native.lib.mg_last_error()
    return rc, text, before, ctr


@pytest.mark.parametrize("case,over,text", ROLL_TABLE, ids=[r[0] for r in ROLL_TABLE])
def test_rollout_refusal(case, over, text):
    assert _call_roll(over) == (1, text)


@pytest.mark.parametrize("entry", (STORE, HOST))
@pytest.mark.parametrize("case,over,key", STORE_TABLE, ids=[r[0] for r in STORE_TABLE])
def test_store_refusal_changes_no_counter(case, over, key, entry):
    rc, text, before, after = _call_store(entry, over)
    assert (rc, text) == (1, _store_texts(entry)[key])
    if entry == HOST:
        np.testing.assert_array_equal(after, before)


def test_rollout_nothing_to_do_returns_0_behind_every_earlier_check_only():
    """n_member == 0 and num_steps == 0 succeed with every argument valid; a fault of any check before that
    return is still refused with its own text."""
    empties = (dict(n=0), dict(num_steps=0))
    for empty in empties:
        assert _call_roll(empty)[0] == 0
        assert _call_roll(dict(empty, mode=0))[0] == 0
    for case, over, text in ROLL_TABLE:
        for empty in empties:
            if not set(empty) & set(over):
                assert _call_roll(dict(over, **empty)) == (1, text), (case, empty)


@pytest.mark.parametrize("entry", (STORE, HOST))
def test_store_nothing_to_do_returns_0_behind_every_earlier_check_only(entry):
    """The same for the stores, whose later checks (the required arrays, their alignment, the grid) are not looked
    at by a call with nothing to do; such a call moves no counter."""
    texts = _store_texts(entry)
    empties = (dict(n=0), dict(num_steps=0))
    for empty in empties:
        rc, text, before, after = _call_store(entry, empty)
        assert rc == 0
        if entry == HOST:
            np.testing.assert_array_equal(after, before)
        for over in STORE_BEHIND_EMPTY:
            assert _call_store(entry, dict(over, **empty))[0] == 0
    seen_last = False
    for case, over, key in STORE_TABLE:
        if seen_last and key != "GOAL":
            continue
        seen_last |= key == "GOAL"  # the check right before the return
        for empty in empties:
            if not set(empty) & set(over):
                assert _call_store(entry, dict(over, **empty))[:2] == (1, texts[key]), (case, empty)
    assert seen_last


def test_member_count_boundaries():
    """0 and 65 members are refused (the tables); 1 and 64 pass the member count and every per-member check on
    exactly sized lists: the empty call returns 0, and a later fault is refused with its own text."""
    for members in (1, 64):
        last = members - 1
        assert _call_roll(dict(members=members, num_steps=0))[0] == 0
        assert _call_roll(dict(members=members, mode=1)) == (1, R_MODE)
        assert _call_roll(dict(members=members, nets={last: ODD8})) == (1, R_NET % last)
        assert _call_roll(dict(members=members, n=_past_grid(members))) == (1, R_GRID)
        assert _call_roll(dict(members=members, n=_past_grid(members) - 64, no_params=True)) == (1, R_PARAMS)
        for entry in (STORE, HOST):
            texts = _store_texts(entry)
            assert _call_store(entry, dict(members=members, num_steps=0))[0] == 0
            assert _call_store(entry, dict(members=members, capacity=0))[:2] == (1, texts["CAP"])
            assert _call_store(entry, dict(members=members, rows={last: None}))[:2] == (1, texts["NULL1"])


def test_abi_version_stays_21():
    from merging_gym import _native

    assert _native.lib.mg_abi_version() == 21 == _native.ABI_VERSION


def test_header_declares_and_native_binds_the_three_entries():
    from merging_gym import _native

    header = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "merging_hip.h")
    with open(header) as f:
        text = f.read()
    index = text[:text.index("#ifndef MERGING_HIP_H_")]
    for name, nargs in ((ROLL, 11), (STORE, 8), (HOST, 7)):
        assert re.search(r"^int %s\(" % name, text, re.M), f"{name} is not declared"
        assert name in index, f"{name} is not in the header's index"
        f = getattr(_native.lib, name)
        assert f.argtypes is not None and len(f.argtypes) == nargs
        assert f.restype is ctypes.c_int
