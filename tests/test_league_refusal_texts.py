"""The exact text of every refusal of the league's two entry points, mg_rollout_qnet_league and
mg_stats_reduce_many, in the style of test_acting_refusal_texts.py.

The argument checks run before any launch, so fake, never-dereferenced pointers drive them on a host without a
GPU. Each row names an entry point, the arguments that differ from a call that would pass every check, and the
whole mg_last_error() text of the refusal (the return code is hipErrorInvalidValue, 1). A row with two bad
arguments pins which check fires first: there is one for every adjacent pair of checks. The nothing-to-do calls
of the rollout (n_pair == 0, num_steps == 0) return 0 only once every check has passed.

No row passes every check with something to do: such a call would launch on the fake pointers. That is also why
mg_stats_reduce_many has no nothing-to-do row: with n_segment == 0 it still launches its second pass, which
writes the empty totals (tests/test_gpu_stats_reduce_many.py).
"""
import ctypes

import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2
GRID = 0x7fffffff * 256  # the most envs a grid of 256-env blocks covers; a multiple of 64
RED_GRID = 0x7fffffff * 1024  # the most records of one segment: a grid of 1,024-record blocks

L = b"mg_rollout_qnet_league: "
L_NETS = L + b"need 1 <= nets <= 64"
L_NEG = L + b"n_pair < 0"
L_64 = L + (b"n_pair must be a multiple of 64 (a won-mask word covers 64 envs and is stored whole, so no two "
            b"pairings may share one)")
L_GRID = L + b"nets * nets * n_pair exceeds the grid limit"
L_PARAMS = b"params is NULL"
L_TIMEOUT = b"mg_params: timeout_steps must be in 1..8191 (the step count of mg_state.tf saturates at 8191)"
L_STATE = b"mg_state has a NULL array"
L_TRAJ = b"traj is NULL (pass a zeroed mg_traj)"
L_LEAGUE = L + b"league is NULL (nets mg_league_net entries)"
L_DIMS = L + b"need num_steps >= 0 and 1 <= out_dim <= 8"
L_NET = L + b"net %d: net must be a 16-byte aligned packed Q-net"
L_ALIGN = b"traj.obs must be 16-byte, rew/final_obs 8-byte, flags 4-byte aligned"

R = b"mg_stats_reduce_many: "
R_SEG = R + b"need 1 <= segments <= 4096"
R_NEG = R + b"n_segment < 0"
R_NULL = R + b"NULL pointer"
R_ALIGN = R + b"rec and scratch must be 16-byte, totals 8-byte aligned"
R_GRID = R + b"n_segment exceeds the grid limit"
R_SCR = R + b"scratch smaller than mg_stats_reduce_many_scratch_bytes(n_segment, segments)"

ROLL, RED = "mg_rollout_qnet_league", "mg_stats_reduce_many"


def _past_grid(nets):
    """The first multiple of 64 with nets * nets * n_pair past the grid limit."""
    return (GRID // (nets * nets) // 64 + 1) * 64


# (case, entry point, overrides, mg_last_error()), in each entry point's order of checks
TABLE = [
    # ---- mg_rollout_qnet_league
    ("nets 0", ROLL, dict(nets=0), L_NETS),
    ("nets 65", ROLL, dict(nets=65), L_NETS),
    ("nets -1", ROLL, dict(nets=-1), L_NETS),
    ("n_pair < 0", ROLL, dict(n=-64), L_NEG),
    ("n_pair 1", ROLL, dict(n=1), L_64),
    ("n_pair 1000", ROLL, dict(n=1000), L_64),
    ("nets * nets * n_pair past the grid", ROLL, dict(n=_past_grid(3)), L_GRID),
    ("64 nets past the grid", ROLL, dict(nets=64, n=_past_grid(64)), L_GRID),
    ("params NULL", ROLL, dict(no_params=True), L_PARAMS),
    ("params.timeout_steps = 0", ROLL, dict(params=dict(timeout_steps=0)), L_TIMEOUT),
    ("state NULL", ROLL, dict(no_state=True), L_STATE),
    ("state array NULL", ROLL, dict(state=dict(tf=None)), L_STATE),
    ("traj NULL", ROLL, dict(no_traj=True), L_TRAJ),
    ("league NULL", ROLL, dict(no_league=True), L_LEAGUE),
    ("num_steps < 0", ROLL, dict(num_steps=-1), L_DIMS),
    ("out_dim 0", ROLL, dict(out_dim=0), L_DIMS),
    ("out_dim 9", ROLL, dict(out_dim=9), L_DIMS),
    ("net 1 NULL", ROLL, dict(league={1: None}), L_NET % 1),
    ("net 2 misaligned", ROLL, dict(league={2: ODD8}), L_NET % 2),
    ("traj.obs misaligned", ROLL, dict(traj=dict(obs=ODD8)), L_ALIGN),
    ("traj.final_obs misaligned", ROLL, dict(traj=dict(final_obs=ODD4)), L_ALIGN),
    ("traj.rew misaligned", ROLL, dict(traj=dict(rew=ODD4)), L_ALIGN),
    ("traj.flags misaligned", ROLL, dict(traj=dict(flags=ODD2)), L_ALIGN),
    ("nets before n_pair", ROLL, dict(nets=0, n=-64), L_NETS),
    ("n_pair < 0 before its multiple", ROLL, dict(n=-1), L_NEG),
    ("n_pair's multiple before the grid", ROLL, dict(n=_past_grid(3) + 1), L_64),
    ("grid before params", ROLL, dict(n=_past_grid(3), no_params=True), L_GRID),
    ("params before state", ROLL, dict(no_params=True, no_state=True), L_PARAMS),
    ("state before traj", ROLL, dict(no_state=True, no_traj=True), L_STATE),
    ("traj before league", ROLL, dict(no_traj=True, no_league=True), L_TRAJ),
    ("league before out_dim", ROLL, dict(no_league=True, out_dim=9), L_LEAGUE),
    ("out_dim before the nets", ROLL, dict(out_dim=0, league={0: None}), L_DIMS),
    ("net 0 before net 1", ROLL, dict(league={0: ODD8, 1: None}), L_NET % 0),
    ("the nets before alignment", ROLL, dict(league={2: None}, traj=dict(rew=ODD4)), L_NET % 2),
    ("alignment before the empty call", ROLL, dict(num_steps=0, traj=dict(flags=ODD2)), L_ALIGN),
    ("alignment before the empty batch", ROLL, dict(n=0, traj=dict(obs=ODD8)), L_ALIGN),

    # ---- mg_stats_reduce_many
    ("segments 0", RED, dict(segments=0), R_SEG),
    ("segments 4097", RED, dict(segments=4097), R_SEG),
    ("segments -1", RED, dict(segments=-1), R_SEG),
    ("n_segment < 0", RED, dict(n=-1), R_NEG),
    ("totals NULL", RED, dict(totals=None), R_NULL),
    ("rec NULL", RED, dict(rec=None), R_NULL),
    ("totals NULL with nothing to sum", RED, dict(totals=None, n=0), R_NULL),
    ("rec misaligned", RED, dict(rec=ODD8), R_ALIGN),
    ("scratch misaligned", RED, dict(scratch=ODD8), R_ALIGN),
    ("totals misaligned", RED, dict(totals=ODD4), R_ALIGN),
    ("totals misaligned with nothing to sum", RED, dict(totals=ODD4, n=0), R_ALIGN),
    ("n_segment past the grid", RED, dict(n=RED_GRID + 1, scratch_bytes=1 << 62), R_GRID),
    ("scratch NULL", RED, dict(scratch=None), R_SCR),
    ("scratch 8 bytes short", RED, dict(scratch_short=8), R_SCR),
    ("scratch sized for one segment", RED, dict(scratch_lone=True), R_SCR),
    ("scratch sized for 1,024 records at 1,025", RED, dict(n=1025, scratch_bytes=3 * 80), R_SCR),
    ("segments before n_segment", RED, dict(segments=0, n=-1), R_SEG),
    ("n_segment before NULL", RED, dict(n=-1, totals=None), R_NEG),
    ("NULL before alignment", RED, dict(rec=None, totals=ODD4), R_NULL),
    ("alignment before the grid", RED, dict(scratch=ODD8, n=RED_GRID + 1), R_ALIGN),
    ("grid before scratch", RED, dict(n=RED_GRID + 1, scratch=None), R_GRID),
]

# (entry, overrides) that would be refused only behind the rollout's nothing-to-do return: there are none -- every
# check of mg_rollout_qnet_league stands before it -- so the table's last rows pin that the return comes last
EMPTY = (dict(n=0), dict(num_steps=0))


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
    if entry == ROLL:
        nets = g("nets", 3)
        count = min(max(nets, 1), 64)  # entries the list holds: a refused count reads none of them
        P = _native.default_params()
        for k, v in g("params", {}).items():
            setattr(P, k, v)
        P = None if g("no_params", False) else ctypes.byref(P)
        state = {k: FAKE for k, _ in _native.State._fields_}
        state.update(g("state", {}))
        st = None if g("no_state", False) else ctypes.byref(_struct(_native.State, state))
        traj = None if g("no_traj", False) else ctypes.byref(_struct(_native.Traj, g("traj", {})))
        league = (_native.LeagueNet * count)()
        for k in range(count):
            league[k] = _native.LeagueNet(FAKE + 4096 * k, k, 1 << 31)
        for k, v in g("league", {}).items():
            league[k].net = v
        args = (P, st, traj, None, g("n", 128), nets, 0, 500, g("num_steps", 4),
                None if g("no_league", False) else league, g("out_dim", 5), 1, None)
    else:
        n, segments = g("n", 2112), g("segments", 3)
        size = (lib.mg_stats_reduce_scratch_bytes(n) if g("scratch_lone", False)
                else lib.mg_stats_reduce_many_scratch_bytes(n, segments)) - g("scratch_short", 0)
        size = g("scratch_bytes", size)
        args = (_ptr(g("rec", FAKE)), n, segments, _ptr(g("totals", FAKE + 8)), _ptr(g("scratch", FAKE)), size, None)
    assert not a, f"unknown overrides {a}"
    rc = getattr(lib, entry)(*args)
    return rc, lib.mg_last_error()


@pytest.mark.parametrize("case,entry,over,text", TABLE, ids=[f"{r[1]}-{r[0]}" for r in TABLE])
def test_refusal(case, entry, over, text):
    assert _call(entry, over) == (1, text)


def test_nothing_to_do_returns_0_behind_every_check():
    """n_pair == 0 and num_steps == 0 succeed with every argument valid; a fault of any check is still refused
    with its own text (no check stands behind that return)."""
    for empty in EMPTY:
        assert _call(ROLL, empty)[0] == 0
    for case, e, over, text in TABLE:
        if e != ROLL:
            continue
        for empty in EMPTY:
            if set(empty) & set(over):
                continue
            assert _call(ROLL, dict(over, **empty)) == (1, text), (case, empty)


def test_net_count_boundaries():
    """0 and 65 nets are refused (the table); 1 and 64 pass the count and every per-net check on exactly sized
    lists: the empty call returns 0, and a later fault is refused with its own text."""
    for nets in (1, 64):
        assert _call(ROLL, dict(nets=nets, num_steps=0))[0] == 0
        assert _call(ROLL, dict(nets=nets, out_dim=9)) == (1, L_DIMS)
        assert _call(ROLL, dict(nets=nets, league={nets - 1: ODD8})) == (1, L_NET % (nets - 1))
        assert _call(ROLL, dict(nets=nets, n=_past_grid(nets))) == (1, L_GRID)
        assert _call(ROLL, dict(nets=nets, n=_past_grid(nets) - 64, no_params=True)) == (1, L_PARAMS)


def test_segment_count_boundaries_and_scratch_sizes():
    """1 and 4,096 segments pass the count (a later fault is refused with its own text); the scratch is
    `segments` lone scratches, and 0 for a count the call refuses."""
    from merging_gym import _native

    lib = _native.lib
    for segments in (1, 4096):
        assert _call(RED, dict(segments=segments, scratch_short=8)) == (1, R_SCR)
        assert _call(RED, dict(segments=segments, totals=ODD4)) == (1, R_ALIGN)
        for n in (0, 1, 1024, 1025, 2112):
            assert lib.mg_stats_reduce_many_scratch_bytes(n, segments) == segments * lib.mg_stats_reduce_scratch_bytes(n)
    assert lib.mg_stats_reduce_scratch_bytes(1024) == 80 and lib.mg_stats_reduce_scratch_bytes(1025) == 160
    for segments in (0, -1, 4097):
        assert lib.mg_stats_reduce_many_scratch_bytes(2112, segments) == 0
