"""The exact text of every refusal of the population's acting entry points and of the lone replay store:
mg_replay_store, mg_replay_store_many and mg_rollout_qnet_many (mg_rollout_qnet's are in test_refusal_texts.py).

The argument checks run before any launch, so fake, never-dereferenced pointers drive them on a host without a
GPU. Each row names an entry point, the arguments that differ from a call that would pass every check, and the
whole mg_last_error() text of the refusal (the return code is hipErrorInvalidValue, 1). A row with two bad
arguments pins which check fires first: there is one for every adjacent pair of checks. The nothing-to-do calls
(n == 0, num_steps == 0) return 0 only once every earlier check has passed, and before any later one.

No row passes every check with something to do: such a call would launch on the fake pointers. That is why the
chunk limit is pinned from above only (the first num_steps it refuses), not by a call one step below it.
"""
import ctypes

import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2
GRID = 0x7fffffff * 256  # the most envs a grid of 256-env blocks covers; a multiple of 64
# a write block walks 2 steps and the grid's second dimension holds 65535 chunks: the first num_steps past it
CHUNKS = 2 * 65535 + 1

S = b"mg_replay_store: "
S_NULL = S + b"NULL pointer"
S_CAP = S + b"capacity < 1"
S_ROW = S + b"row_floats must be 22, or 24 with both goal and next_goal set"
S_META = S + b"meta_goal (Goal_DQN rows) needs reward and won_mask (no_break) and no goal"
S_NEG = S + b"n < 0 or num_steps < 0"
S_REQ = S + b"obs_first, obs, a1 (or flags) and rew are required"
S_AL8 = S + b"float buffers and scratch must be 8-byte aligned"
S_AL4 = S + b"goal, next_goal and reward must be 4-byte aligned"
S_GRID = S + b"n * num_steps exceeds the grid limit"
S_SCR = S + b"scratch smaller than mg_replay_scratch_bytes(n, num_steps)"
S_CHUNK = S + b"num_steps too large"

M = b"mg_replay_store_many: "
M_MEMBERS = M + b"need 1 <= members <= 64"
M_NULL = M + b"NULL pointer"
M_NULL1 = M + b"NULL pointer (a member's rows or counter)"
M_AL1 = M + b"every member's rows and counter must be 8-byte aligned"
M_TWICE = M + b"a ring is listed twice (two members' appends to one ring have no defined order)"
M_CAP = M + b"capacity < 1"
M_ROW = M + b"22-float rows only: row_floats must be 22 and goal, next_goal, meta_goal NULL"
M_NEG = M + b"n_member < 0 or num_steps < 0"
M_64 = M + b"n_member must be a multiple of 64 (a member's won bits begin a word of the mask)"
M_REQ = M + b"obs_first, obs, a1 (or flags) and rew are required"
M_AL8 = M + b"float buffers, won_mask and scratch must be 8-byte aligned"
M_AL4 = M + b"reward must be 4-byte aligned"
M_GRID = M + b"n_member * num_steps exceeds the grid limit"
M_SCR = M + b"scratch smaller than mg_replay_scratch_many_bytes(n_member, num_steps, members)"
M_CHUNK = M + b"num_steps too large"

Q = b"mg_rollout_qnet_many: "
Q_MEMBERS = Q + b"need 1 <= members <= 64"
Q_NEG = Q + b"n_member < 0"
Q_64 = Q + (b"n_member must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so no two "
            b"members may share one)")
Q_GRID = Q + b"members * n_member exceeds the grid limit"
Q_PARAMS = b"params is NULL"
Q_TIMEOUT = b"mg_params: timeout_steps must be in 1..8191 (the step count of mg_state.tf saturates at 8191)"
Q_STATE = b"mg_state has a NULL array"
Q_TRAJ = b"traj is NULL (pass a zeroed mg_traj)"
Q_ACTORS = Q + b"actors is NULL (members mg_qnet_actor entries)"
Q_DIMS = Q + b"need num_steps >= 0 and 1 <= out_dim <= 8"
Q_MODE = Q + b"opponent_mode must be 0 (None), 1 (uniform), 2 (same net) or 3 (each member's opp_net)"
Q_NET = Q + b"member %d: net must be a 16-byte aligned packed Q-net"
Q_OPP = Q + b"member %d: opponent_mode 3 needs opp_net, a 16-byte aligned packed Q-net"
Q_ALIGN = b"traj.obs must be 16-byte, rew/final_obs 8-byte, flags 4-byte aligned"

LONE, MANY, ROLL = "mg_replay_store", "mg_replay_store_many", "mg_rollout_qnet_many"
ROW1 = FAKE + 65536   # member 0's rows in the default member list
CTR1 = FAKE + 8       # member 1's counter


def _past_grid(members):
    """The first multiple of 64 with members * n_member past the grid limit."""
    return (GRID // members // 64 + 1) * 64


# (case, entry point, overrides, mg_last_error()), in each entry point's order of checks
TABLE = [
    # ---- mg_replay_store
    ("rows NULL", LONE, dict(rows=None), S_NULL),
    ("counter NULL", LONE, dict(counter=None), S_NULL),
    ("tr NULL", LONE, dict(no_tr=True), S_NULL),
    ("capacity 0", LONE, dict(capacity=0), S_CAP),
    ("row_floats 23", LONE, dict(row_floats=23), S_ROW),
    ("row_floats 24 without goals", LONE, dict(row_floats=24), S_ROW),
    ("row_floats 22 with goals", LONE, dict(tr=dict(goal=FAKE, next_goal=FAKE)), S_ROW),
    ("goal without next_goal", LONE, dict(row_floats=24, tr=dict(goal=FAKE)), S_ROW),
    ("next_goal without goal", LONE, dict(tr=dict(next_goal=FAKE)), S_ROW),
    ("meta_goal with goal", LONE, dict(row_floats=24, tr=dict(goal=FAKE, next_goal=FAKE, meta_goal=FAKE, reward=FAKE)),
     S_META),
    ("meta_goal without reward", LONE, dict(tr=dict(meta_goal=FAKE)), S_META),
    ("meta_goal without won_mask", LONE, dict(tr=dict(meta_goal=FAKE, reward=FAKE, won_mask=None)), S_META),
    ("n < 0", LONE, dict(n=-1), S_NEG),
    ("num_steps < 0", LONE, dict(num_steps=-1), S_NEG),
    ("obs_first NULL", LONE, dict(tr=dict(obs_first=None)), S_REQ),
    ("obs NULL", LONE, dict(tr=dict(obs=None)), S_REQ),
    ("neither a1 nor flags", LONE, dict(tr=dict(flags=None)), S_REQ),
    ("rew NULL", LONE, dict(tr=dict(rew=None)), S_REQ),
    ("rows misaligned", LONE, dict(rows=ODD4), S_AL8),
    ("obs_first misaligned", LONE, dict(tr=dict(obs_first=ODD4)), S_AL8),
    ("obs misaligned", LONE, dict(tr=dict(obs=ODD4)), S_AL8),
    ("final_obs misaligned", LONE, dict(tr=dict(final_obs=ODD4)), S_AL8),
    ("rew misaligned", LONE, dict(tr=dict(rew=ODD4)), S_AL8),
    ("scratch misaligned", LONE, dict(scratch=ODD4), S_AL8),
    ("goal misaligned", LONE, dict(row_floats=24, tr=dict(goal=ODD2, next_goal=FAKE)), S_AL4),
    ("next_goal misaligned", LONE, dict(row_floats=24, tr=dict(goal=FAKE, next_goal=ODD2)), S_AL4),
    ("reward misaligned", LONE, dict(tr=dict(reward=ODD2)), S_AL4),
    ("n past the grid", LONE, dict(n=GRID + 1), S_GRID),
    ("scratch NULL", LONE, dict(scratch=None), S_SCR),
    ("scratch 8 bytes short", LONE, dict(scratch_short=8), S_SCR),
    ("the first num_steps past 65535 chunks", LONE, dict(num_steps=CHUNKS), S_CHUNK),
    ("NULL before capacity", LONE, dict(counter=None, capacity=0), S_NULL),
    ("capacity before row_floats", LONE, dict(capacity=0, row_floats=23), S_CAP),
    ("row_floats before meta_goal", LONE, dict(row_floats=23, tr=dict(meta_goal=FAKE)), S_ROW),
    ("meta_goal before n", LONE, dict(tr=dict(meta_goal=FAKE), n=-1), S_META),
    ("n before the empty call", LONE, dict(n=-1, num_steps=0), S_NEG),
    ("num_steps before the empty call", LONE, dict(n=0, num_steps=-1), S_NEG),
    ("required before alignment", LONE, dict(tr=dict(rew=None, obs=ODD4)), S_REQ),
    ("8-byte before 4-byte alignment", LONE, dict(rows=ODD4, tr=dict(reward=ODD2)), S_AL8),
    ("alignment before the grid", LONE, dict(tr=dict(reward=ODD2), n=GRID + 1), S_AL4),
    ("grid before scratch", LONE, dict(n=GRID + 1, scratch=None), S_GRID),
    ("scratch before chunks", LONE, dict(num_steps=CHUNKS, scratch_short=8), S_SCR),

    # ---- mg_replay_store_many
    ("members 0", MANY, dict(members=0), M_MEMBERS),
    ("members 65", MANY, dict(members=65), M_MEMBERS),
    ("members -1", MANY, dict(members=-1), M_MEMBERS),
    ("rows NULL", MANY, dict(no_rows=True), M_NULL),
    ("counters NULL", MANY, dict(no_counters=True), M_NULL),
    ("tr NULL", MANY, dict(no_tr=True), M_NULL),
    ("member 2's rows NULL", MANY, dict(rows={2: None}), M_NULL1),
    ("member 1's counter NULL", MANY, dict(counters={1: None}), M_NULL1),
    ("member 1's rows misaligned", MANY, dict(rows={1: ODD4}), M_AL1),
    ("member 2's counter misaligned", MANY, dict(counters={2: ODD4}), M_AL1),
    ("member 2's rows are member 0's", MANY, dict(rows={2: ROW1}), M_TWICE),
    ("member 2's counter is member 1's", MANY, dict(counters={2: CTR1}), M_TWICE),
    ("capacity 0", MANY, dict(capacity=0), M_CAP),
    ("row_floats 24", MANY, dict(row_floats=24), M_ROW),
    ("goal set", MANY, dict(tr=dict(goal=FAKE)), M_ROW),
    ("next_goal set", MANY, dict(tr=dict(next_goal=FAKE)), M_ROW),
    ("meta_goal set", MANY, dict(tr=dict(meta_goal=FAKE)), M_ROW),
    ("n_member < 0", MANY, dict(n=-64), M_NEG),
    ("num_steps < 0", MANY, dict(num_steps=-1), M_NEG),
    ("n_member 1", MANY, dict(n=1), M_64),
    ("n_member 96", MANY, dict(n=96), M_64),
    ("obs_first NULL", MANY, dict(tr=dict(obs_first=None)), M_REQ),
    ("obs NULL", MANY, dict(tr=dict(obs=None)), M_REQ),
    ("neither a1 nor flags", MANY, dict(tr=dict(flags=None)), M_REQ),
    ("rew NULL", MANY, dict(tr=dict(rew=None)), M_REQ),
    ("obs_first misaligned", MANY, dict(tr=dict(obs_first=ODD4)), M_AL8),
    ("obs misaligned", MANY, dict(tr=dict(obs=ODD4)), M_AL8),
    ("final_obs misaligned", MANY, dict(tr=dict(final_obs=ODD4)), M_AL8),
    ("rew misaligned", MANY, dict(tr=dict(rew=ODD4)), M_AL8),
    ("won_mask misaligned", MANY, dict(tr=dict(won_mask=ODD4)), M_AL8),
    ("scratch misaligned", MANY, dict(scratch=ODD4), M_AL8),
    ("reward misaligned", MANY, dict(tr=dict(reward=ODD2)), M_AL4),
    ("n_member past the grid", MANY, dict(n=GRID + 64), M_GRID),
    ("scratch NULL", MANY, dict(scratch=None), M_SCR),
    ("scratch 8 bytes short", MANY, dict(scratch_short=8), M_SCR),
    ("scratch sized for the lone store", MANY, dict(scratch_lone=True), M_SCR),
    ("the first num_steps past 65535 chunks", MANY, dict(num_steps=CHUNKS), M_CHUNK),
    ("members before NULL", MANY, dict(members=65, no_rows=True), M_MEMBERS),
    ("NULL before a member's NULL", MANY, dict(no_tr=True, rows={0: None}), M_NULL),
    ("a member's NULL before its alignment", MANY, dict(rows={1: ODD4}, counters={1: None}), M_NULL1),
    ("a member's alignment before its twin", MANY, dict(rows={1: ROW1}, counters={1: ODD4}), M_AL1),
    ("member 0's alignment before member 1's NULL", MANY, dict(rows={0: ODD4}, counters={1: None}), M_AL1),
    ("member 1's twin before member 2's NULL", MANY, dict(rows={1: ROW1, 2: None}), M_TWICE),
    ("the member list before capacity", MANY, dict(counters={2: CTR1}, capacity=0), M_TWICE),
    ("capacity before row_floats", MANY, dict(capacity=0, row_floats=24), M_CAP),
    ("row_floats before n_member", MANY, dict(tr=dict(goal=FAKE), n=-64), M_ROW),
    ("n_member < 0 before its multiple", MANY, dict(n=-1), M_NEG),
    ("num_steps < 0 before n_member's multiple", MANY, dict(n=96, num_steps=-1), M_NEG),
    ("n_member's multiple before the empty call", MANY, dict(n=96, num_steps=0), M_64),
    ("required before alignment", MANY, dict(tr=dict(rew=None, won_mask=ODD4)), M_REQ),
    ("8-byte before 4-byte alignment", MANY, dict(tr=dict(won_mask=ODD4, reward=ODD2)), M_AL8),
    ("alignment before the grid", MANY, dict(tr=dict(reward=ODD2), n=GRID + 64), M_AL4),
    ("grid before scratch", MANY, dict(n=GRID + 64, scratch=None), M_GRID),
    ("scratch before chunks", MANY, dict(num_steps=CHUNKS, scratch_short=8), M_SCR),

    # ---- mg_rollout_qnet_many
    ("members 0", ROLL, dict(members=0), Q_MEMBERS),
    ("members 65", ROLL, dict(members=65), Q_MEMBERS),
    ("members -1", ROLL, dict(members=-1), Q_MEMBERS),
    ("n_member < 0", ROLL, dict(n=-64), Q_NEG),
    ("n_member 1", ROLL, dict(n=1), Q_64),
    ("n_member 1000", ROLL, dict(n=1000), Q_64),
    ("members * n_member past the grid", ROLL, dict(n=_past_grid(3)), Q_GRID),
    ("64 members past the grid", ROLL, dict(members=64, n=_past_grid(64)), Q_GRID),
    ("params NULL", ROLL, dict(no_params=True), Q_PARAMS),
    ("params.timeout_steps = 0", ROLL, dict(params=dict(timeout_steps=0)), Q_TIMEOUT),
    ("state NULL", ROLL, dict(no_state=True), Q_STATE),
    ("state array NULL", ROLL, dict(state=dict(tf=None)), Q_STATE),
    ("traj NULL", ROLL, dict(no_traj=True), Q_TRAJ),
    ("actors NULL", ROLL, dict(no_actors=True), Q_ACTORS),
    ("num_steps < 0", ROLL, dict(num_steps=-1), Q_DIMS),
    ("out_dim 0", ROLL, dict(out_dim=0), Q_DIMS),
    ("out_dim 9", ROLL, dict(out_dim=9), Q_DIMS),
    ("mode -1", ROLL, dict(mode=-1), Q_MODE),
    ("mode 4", ROLL, dict(mode=4), Q_MODE),
    ("member 1's net NULL", ROLL, dict(actors={(1, "net"): None}), Q_NET % 1),
    ("member 2's net misaligned", ROLL, dict(actors={(2, "net"): ODD8}, mode=2), Q_NET % 2),
    ("member 0's opp_net NULL", ROLL, dict(actors={(0, "opp_net"): None}, mode=3), Q_OPP % 0),
    ("member 2's opp_net misaligned", ROLL, dict(actors={(2, "opp_net"): ODD8}, mode=3), Q_OPP % 2),
    ("traj.obs misaligned", ROLL, dict(traj=dict(obs=ODD8)), Q_ALIGN),
    ("traj.final_obs misaligned", ROLL, dict(traj=dict(final_obs=ODD4)), Q_ALIGN),
    ("traj.rew misaligned", ROLL, dict(traj=dict(rew=ODD4)), Q_ALIGN),
    ("traj.flags misaligned", ROLL, dict(traj=dict(flags=ODD2)), Q_ALIGN),
    ("members before n_member", ROLL, dict(members=0, n=-64), Q_MEMBERS),
    ("n_member < 0 before its multiple", ROLL, dict(n=-1), Q_NEG),
    ("n_member's multiple before the grid", ROLL, dict(n=_past_grid(3) + 1), Q_64),
    ("grid before params", ROLL, dict(n=_past_grid(3), no_params=True), Q_GRID),
    ("params before state", ROLL, dict(no_params=True, no_state=True), Q_PARAMS),
    ("state before traj", ROLL, dict(no_state=True, no_traj=True), Q_STATE),
    ("traj before actors", ROLL, dict(no_traj=True, no_actors=True), Q_TRAJ),
    ("actors before out_dim", ROLL, dict(no_actors=True, out_dim=9), Q_ACTORS),
    ("out_dim before mode", ROLL, dict(out_dim=0, mode=4), Q_DIMS),
    ("mode before the nets", ROLL, dict(mode=4, actors={(0, "net"): None}), Q_MODE),
    ("a member's net before its opp_net", ROLL, dict(mode=3, actors={(1, "net"): ODD8, (1, "opp_net"): None}),
     Q_NET % 1),
    ("member 0's opp_net before member 1's net", ROLL, dict(mode=3, actors={(0, "opp_net"): ODD8, (1, "net"): None}),
     Q_OPP % 0),
    ("the nets before alignment", ROLL, dict(actors={(2, "net"): None}, traj=dict(rew=ODD4)), Q_NET % 2),
    ("alignment before the empty call", ROLL, dict(num_steps=0, traj=dict(flags=ODD2)), Q_ALIGN),
    ("alignment before the empty batch", ROLL, dict(n=0, traj=dict(obs=ODD8)), Q_ALIGN),
]

# what makes a call one with nothing to do, and (entry, overrides) that would be refused only behind that return
EMPTY = {LONE: (dict(n=0), dict(num_steps=0)), MANY: (dict(n=0), dict(num_steps=0)),
         ROLL: (dict(n=0), dict(num_steps=0))}
BEHIND_EMPTY = [
    (LONE, dict(tr=dict(obs=None))), (LONE, dict(rows=ODD4)), (LONE, dict(tr=dict(reward=ODD2))),
    (LONE, dict(scratch=None)),
    (MANY, dict(tr=dict(rew=None))), (MANY, dict(tr=dict(won_mask=ODD4))), (MANY, dict(tr=dict(reward=ODD2))),
    (MANY, dict(scratch=None)),
]


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _struct(cls, fields):
    return cls(**{k: _ptr(v) for k, v in fields.items()})


def _call(entry, over):
    """Call `entry` with arguments that pass every check, except for `over`; (return value, error text)."""
    from merging_gym import _native

    lib = _native.lib
    a = dict(over)
    g = a.pop
    members = g("members", 3)
    count = min(max(members, 1), 64)  # entries the lists hold: a refused member count reads none of them
    if entry in (LONE, MANY):
        tr = dict(obs_first=FAKE, obs=FAKE, final_obs=FAKE, rew=FAKE, won_mask=FAKE, flags=FAKE)
        tr.update(g("tr", {}))
        tr = None if g("no_tr", False) else ctypes.byref(_struct(_native.Transitions, tr))
        n, num_steps = g("n", 64), g("num_steps", 3)
        capacity, row_floats, scratch = g("capacity", 2000), g("row_floats", 22), g("scratch", FAKE)
        short, lone_size = g("scratch_short", 0), g("scratch_lone", False)
    if entry == LONE:
        size = lib.mg_replay_scratch_bytes(n, num_steps) - short
        args = (_ptr(g("rows", ROW1)), _ptr(g("counter", FAKE)), capacity, row_floats, tr, n, num_steps, 1,
                _ptr(scratch), size, None)
    elif entry == MANY:
        rows = (ctypes.c_void_p * count)(*(FAKE + 65536 * (m + 1) for m in range(count)))
        counters = (ctypes.c_void_p * count)(*(FAKE + 8 * m for m in range(count)))
        for m, v in g("rows", {}).items():
            rows[m] = v
        for m, v in g("counters", {}).items():
            counters[m] = v
        size = (lib.mg_replay_scratch_bytes(n, num_steps) if lone_size
                else lib.mg_replay_scratch_many_bytes(n, num_steps, members)) - short
        args = (None if g("no_rows", False) else rows, None if g("no_counters", False) else counters, members,
                capacity, row_floats, tr, n, num_steps, 1, _ptr(scratch), size, None)
    elif entry == ROLL:
        P = _native.default_params()
        for k, v in g("params", {}).items():
            setattr(P, k, v)
        P = None if g("no_params", False) else ctypes.byref(P)
        state = {k: FAKE for k, _ in _native.State._fields_}
        state.update(g("state", {}))
        st = None if g("no_state", False) else ctypes.byref(_struct(_native.State, state))
        traj = None if g("no_traj", False) else ctypes.byref(_struct(_native.Traj, g("traj", {})))
        actors = (_native.QnetActor * count)()
        for m in range(count):
            actors[m] = _native.QnetActor(FAKE + 4096 * m, FAKE + 4096 * m + 64, m, 1 << 31, 1 << 30)
        for (m, field), v in g("actors", {}).items():
            setattr(actors[m], field, v)
        args = (P, st, traj, None, g("n", 128), members, 0, 500, g("num_steps", 4),
                None if g("no_actors", False) else actors, g("out_dim", 5), g("mode", 0), 1, None)
    assert not a, f"unknown overrides {a}"
    rc = getattr(lib, entry)(*args)
    return rc, lib.mg_last_error()


@pytest.mark.parametrize("case,entry,over,text", TABLE, ids=[f"{r[1]}-{r[0]}" for r in TABLE])
def test_refusal(case, entry, over, text):
    assert _call(entry, over) == (1, text)


@pytest.mark.parametrize("entry", (LONE, MANY, ROLL))
def test_nothing_to_do_returns_0_behind_every_earlier_check_only(entry):
    """n == 0 and num_steps == 0 succeed with every argument valid; a fault of any check before that return is
    still refused with its own text, and a fault of any check behind it is not looked at."""
    empties = EMPTY[entry]
    for empty in empties:
        assert _call(entry, empty)[0] == 0
        if entry == ROLL:
            assert _call(entry, dict(empty, mode=3))[0] == 0
    last = {LONE: S_NEG, MANY: M_64, ROLL: Q_ALIGN}[entry]  # the check right before the return
    seen_last = False
    for case, e, over, text in TABLE:
        if e != entry or seen_last and text != last:
            continue
        seen_last |= text == last
        for empty in empties:
            if set(empty) & set(over):
                continue
            assert _call(entry, dict(over, **empty)) == (1, text), (case, empty)
    assert seen_last
    for e, over in BEHIND_EMPTY:
        if e == entry:
            for empty in empties:
                assert _call(entry, dict(over, **empty))[0] == 0, (over, empty)


@pytest.mark.parametrize("entry", (MANY, ROLL))
def test_member_count_boundaries(entry):
    """0 and 65 members are refused (the table); 1 and 64 pass the member count and every per-member check on
    exactly sized lists: the empty call returns 0, and a later fault is refused with its own text."""
    for members in (1, 64):
        assert _call(entry, dict(members=members, num_steps=0))[0] == 0
        if entry == MANY:
            assert _call(entry, dict(members=members, capacity=0)) == (1, M_CAP)
            assert _call(entry, dict(members=members, rows={members - 1: None})) == (1, M_NULL1)
            assert _call(entry, dict(members=members, scratch_short=8)) == (1, M_SCR)
        else:
            assert _call(entry, dict(members=members, out_dim=9)) == (1, Q_DIMS)
            assert _call(entry, dict(members=members, actors={(members - 1, "net"): ODD8})) == (1, Q_NET % (members - 1))
            assert _call(entry, dict(members=members, n=_past_grid(members))) == (1, Q_GRID)
            assert _call(entry, dict(members=members, n=_past_grid(members) - 64, no_params=True)) == (1, Q_PARAMS)
