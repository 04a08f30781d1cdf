"""The exact text and code of every refusal of the rollout, Q-net and learner-init entry points.

The argument checks run before any launch, so fake, never-dereferenced pointers drive them on a
host without a GPU. Each row names an entry point, the arguments that differ from a call that
would pass every check, and the return code and mg_last_error() text of the refusal. Where a row
gives two bad arguments at once it also pins which check fires first.
"""
import ctypes

import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2
INF = float("inf")
AUTORESET = 1           # MG_AUTORESET
ROLLOUTS = ("mg_rollout_random", "mg_rollout_qnet", "mg_rollout_hdqn")

ALIGN = b"traj.obs must be 16-byte, rew/final_obs 8-byte, flags 4-byte aligned"
TIMEOUT = b"mg_params: timeout_steps must be in 1..8191 (the step count of mg_state.tf saturates at 8191)"

# (case, overrides, return code, mg_last_error()) of all three rollouts
EVERY_ROLLOUT = [
    ("params NULL", dict(no_params=True), 1, b"params is NULL"),
    ("n < 0", dict(n=-1), 1, b"n < 0"),
    ("n past the grid", dict(n=0x7fffffff * 256 + 1), 1, b"n exceeds the grid limit"),
    ("state NULL", dict(no_state=True), 1, b"mg_state has a NULL array"),
    ("state array NULL", dict(state=dict(tf=None)), 1, b"mg_state has a NULL array"),
    ("params before n", dict(no_params=True, n=-1), 1, b"params is NULL"),
    ("n before state", dict(n=-1, no_state=True), 1, b"n < 0"),
    ("state before traj", dict(no_state=True, no_traj=True), 1, b"mg_state has a NULL array"),
    ("traj NULL", dict(no_traj=True), 1, b"traj is NULL (pass a zeroed mg_traj)"),
    ("traj.obs misaligned", dict(traj=dict(obs=ODD8)), 1, ALIGN),
    ("traj.final_obs misaligned", dict(traj=dict(final_obs=ODD4)), 1, ALIGN),
    ("traj.rew misaligned", dict(traj=dict(rew=ODD4)), 1, ALIGN),
    ("traj.flags misaligned", dict(traj=dict(flags=ODD2)), 1, ALIGN),
]

STEPS = b"need 0 <= num_steps <= 65535 (split longer rollouts)"
QNET = b"net must be a 16-byte aligned packed Q-net"
QDIMS = b"need num_steps >= 0 and 1 <= out_dim <= 8"
QMODE = b"opponent_mode must be 0 (None), 1 (uniform), 2 (same net) or 3 (opp_net)"
QOPP = b"opponent_mode 3 needs opp_net, a 16-byte aligned packed Q-net"
HRING = b"ring_rows needs ring_counter, capacity >= 1 and 16-byte alignment"
HGOAL = b"goal is NULL (an [n] int8 device array)"
HNETS = b"meta_net / lower_net must be 16-byte aligned packed Q-nets"
HDIMS = b"need num_steps >= 0, 1 <= num_goals <= 8, 0 <= reset_goal < num_goals"
HMODE = b"opponent_mode must be 0 (None), 1 (uniform), 2 (self-play) or 3 (other h-DQN)"
HGOP = b"opponent_mode 2 / 3 needs goal_op (an [n] int8 device array)"
HOPP = b"opponent_mode 3 needs 16-byte aligned opp_meta_net / opp_lower_net (mg_qnet_fragments copies)"
HACC = b"ext_reward / no_break need ext_acc (an [n] double device array)"
PACK_DIMS = b"mg_qnet_pack: need 1 <= in_dim <= 13, 1 <= out_dim <= 8"
FWD_DIMS = b"mg_qnet_forward: need 1 <= in_dim <= 13 (swap_halves: in_dim 10)"
FRAG_ALIGN = b"mg_qnet_fragments: buffers must be 16-byte aligned"
INIT_DIMS = b"mg_dqn_learner_init: need 1 <= in_dim <= 13, 1 <= out_dim <= 8"
INIT_ALIGN = b"mg_dqn_learner_init: learner must be 16-byte, the tensors 4-byte aligned"
TENSORS = ("fc1_w", "fc1_b", "fc2_w", "fc2_b", "out_w", "out_b")

# (case, entry point, overrides, return code, mg_last_error())
TABLE = [(c, e, o, rc, t) for e in ROLLOUTS for c, o, rc, t in EVERY_ROLLOUT] + [
    ("params.timeout_steps = 0", "mg_rollout_random", dict(params=dict(timeout_steps=0)), 1, TIMEOUT),
    ("params.timeout_steps = 8192", "mg_rollout_random", dict(params=dict(timeout_steps=8192)), 1, TIMEOUT),
    ("params.R = 0", "mg_rollout_random", dict(params=dict(R=0.0)), 1, b"mg_params: R must be positive and finite"),
    ("params.dT = inf", "mg_rollout_random", dict(params=dict(dT=INF)), 1,
     b"mg_params: dT must be positive and finite"),
    ("params.veh_w = 0", "mg_rollout_random", dict(params=dict(veh_w=0)), 1, b"mg_params: veh_w must be positive"),
    ("params.veh_h = -1", "mg_rollout_random", dict(params=dict(veh_h=-1)), 1, b"mg_params: veh_h must be positive"),
    ("params.inv_R = 1", "mg_rollout_random", dict(params=dict(inv_R=1.0)), 1,
     b"mg_params: inv_R must be 1 / R, rounded"),
    ("params.qp_inv_nz = 0.5", "mg_rollout_random", dict(params=dict(qp_inv_nz=0.5)), 1,
     b"mg_params: qp_inv_nz must be 1 / qp_nz, rounded"),
    ("num_steps < 0", "mg_rollout_random", dict(num_steps=-1), 1, STEPS),
    ("num_steps > 65535", "mg_rollout_random", dict(num_steps=65536), 1, STEPS),
    ("traj before num_steps", "mg_rollout_random", dict(no_traj=True, num_steps=-1), 1,
     b"traj is NULL (pass a zeroed mg_traj)"),
    ("num_steps before alignment", "mg_rollout_random", dict(num_steps=65536, traj=dict(obs=ODD8)), 1, STEPS),
    ("alignment before the empty batch", "mg_rollout_random", dict(n=0, traj=dict(obs=ODD8)), 1, ALIGN),

    ("net NULL", "mg_rollout_qnet", dict(net=None), 1, QNET),
    ("net misaligned", "mg_rollout_qnet", dict(net=ODD8), 1, QNET),
    ("num_steps < 0", "mg_rollout_qnet", dict(num_steps=-1), 1, QDIMS),
    ("out_dim 0", "mg_rollout_qnet", dict(out_dim=0), 1, QDIMS),
    ("out_dim 9", "mg_rollout_qnet", dict(out_dim=9), 1, QDIMS),
    ("mode -1", "mg_rollout_qnet", dict(mode=-1), 1, QMODE),
    ("mode 4", "mg_rollout_qnet", dict(mode=4, opp_net=FAKE), 1, QMODE),
    ("mode 3 without opp_net", "mg_rollout_qnet", dict(mode=3), 1, QOPP),
    ("mode 3 opp_net misaligned", "mg_rollout_qnet", dict(mode=3, opp_net=ODD8), 1, QOPP),
    ("traj before net", "mg_rollout_qnet", dict(no_traj=True, net=None), 1, b"traj is NULL (pass a zeroed mg_traj)"),
    ("net before out_dim", "mg_rollout_qnet", dict(net=ODD8, out_dim=9), 1, QNET),
    ("out_dim before mode", "mg_rollout_qnet", dict(out_dim=0, mode=4), 1, QDIMS),
    ("mode before opp_net", "mg_rollout_qnet", dict(mode=4, opp_net=ODD8), 1, QMODE),
    ("opp_net before alignment", "mg_rollout_qnet", dict(mode=3, traj=dict(rew=ODD4)), 1, QOPP),
    ("alignment before the empty batch", "mg_rollout_qnet", dict(num_steps=0, traj=dict(flags=ODD2)), 1, ALIGN),

    ("ring without counter", "mg_rollout_hdqn", dict(ring=FAKE, cap=16), 1, HRING),
    ("ring capacity 0", "mg_rollout_hdqn", dict(ring=FAKE, counter=FAKE, cap=0), 1, HRING),
    ("ring misaligned", "mg_rollout_hdqn", dict(ring=ODD8, counter=FAKE, cap=16), 1, HRING),
    ("ring before params", "mg_rollout_hdqn", dict(ring=FAKE, no_params=True), 1, HRING),
    ("goal NULL", "mg_rollout_hdqn", dict(goal=None), 1, HGOAL),
    ("meta NULL", "mg_rollout_hdqn", dict(meta=None), 1, HNETS),
    ("lower NULL", "mg_rollout_hdqn", dict(lower=None), 1, HNETS),
    ("meta misaligned", "mg_rollout_hdqn", dict(meta=ODD8), 1, HNETS),
    ("lower misaligned", "mg_rollout_hdqn", dict(lower=ODD8), 1, HNETS),
    ("num_steps < 0", "mg_rollout_hdqn", dict(num_steps=-1), 1, HDIMS),
    ("num_goals 0", "mg_rollout_hdqn", dict(num_goals=0), 1, HDIMS),
    ("num_goals 9", "mg_rollout_hdqn", dict(num_goals=9, reset_goal=0), 1, HDIMS),
    ("reset_goal < 0", "mg_rollout_hdqn", dict(reset_goal=-1), 1, HDIMS),
    ("reset_goal = num_goals", "mg_rollout_hdqn", dict(reset_goal=3), 1, HDIMS),
    ("mode -1", "mg_rollout_hdqn", dict(mode=-1), 1, HMODE),
    ("mode 4", "mg_rollout_hdqn", dict(mode=4, goal_op=FAKE), 1, HMODE),
    ("mode 2 without goal_op", "mg_rollout_hdqn", dict(mode=2), 1, HGOP),
    ("mode 3 without goal_op", "mg_rollout_hdqn", dict(mode=3, opp_meta=FAKE, opp_lower=FAKE), 1, HGOP),
    ("mode 3 without opp_meta", "mg_rollout_hdqn", dict(mode=3, goal_op=FAKE, opp_lower=FAKE), 1, HOPP),
    ("mode 3 without opp_lower", "mg_rollout_hdqn", dict(mode=3, goal_op=FAKE, opp_meta=FAKE), 1, HOPP),
    ("mode 3 opp_meta misaligned", "mg_rollout_hdqn", dict(mode=3, goal_op=FAKE, opp_meta=ODD8, opp_lower=FAKE), 1,
     HOPP),
    ("mode 3 opp_lower misaligned", "mg_rollout_hdqn", dict(mode=3, goal_op=FAKE, opp_meta=FAKE, opp_lower=ODD8), 1,
     HOPP),
    ("ext_reward without ext_acc", "mg_rollout_hdqn", dict(htraj=dict(ext_reward=FAKE)), 1, HACC),
    ("no_break without ext_acc", "mg_rollout_hdqn", dict(htraj=dict(no_break=FAKE)), 1, HACC),
    ("no_break misaligned", "mg_rollout_hdqn", dict(htraj=dict(no_break=ODD4), ext_acc=FAKE), 1,
     b"no_break must be 8-byte aligned"),
    ("without MG_AUTORESET", "mg_rollout_hdqn", dict(flags=0), 1,
     b"mg_rollout_hdqn needs MG_AUTORESET (hdqn.py resets every episode)"),
    ("traj before goal", "mg_rollout_hdqn", dict(no_traj=True, goal=None), 1, b"traj is NULL (pass a zeroed mg_traj)"),
    ("goal before nets", "mg_rollout_hdqn", dict(goal=None, meta=None), 1, HGOAL),
    ("nets before num_goals", "mg_rollout_hdqn", dict(lower=ODD8, num_goals=0), 1, HNETS),
    ("num_goals before mode", "mg_rollout_hdqn", dict(reset_goal=3, mode=4), 1, HDIMS),
    ("mode before goal_op", "mg_rollout_hdqn", dict(mode=4, goal_op=None), 1, HMODE),
    ("goal_op before opp nets", "mg_rollout_hdqn", dict(mode=3), 1, HGOP),
    ("opp nets before ext_acc", "mg_rollout_hdqn", dict(mode=3, goal_op=FAKE, htraj=dict(ext_reward=FAKE)), 1, HOPP),
    ("ext_acc before no_break", "mg_rollout_hdqn", dict(htraj=dict(no_break=ODD4)), 1, HACC),
    ("no_break before alignment", "mg_rollout_hdqn",
     dict(htraj=dict(no_break=ODD4), ext_acc=FAKE, traj=dict(obs=ODD8)), 1, b"no_break must be 8-byte aligned"),
    ("alignment before MG_AUTORESET", "mg_rollout_hdqn", dict(flags=0, traj=dict(obs=ODD8)), 1, ALIGN),
] + [(f"{k} NULL", "mg_qnet_pack", {k: None}, 1, b"mg_qnet_pack: NULL pointer") for k in (*TENSORS, "packed")] + [
    ("in_dim 0", "mg_qnet_pack", dict(in_dim=0), 1, PACK_DIMS),
    ("in_dim 14", "mg_qnet_pack", dict(in_dim=14), 1, PACK_DIMS),
    ("out_dim 0", "mg_qnet_pack", dict(out_dim=0), 1, PACK_DIMS),
    ("out_dim 9", "mg_qnet_pack", dict(out_dim=9), 1, PACK_DIMS),
    ("packed misaligned", "mg_qnet_pack", dict(packed=ODD8), 1, b"mg_qnet_pack: packed buffer must be 16-byte aligned"),
    ("NULL before dims", "mg_qnet_pack", dict(out_b=None, in_dim=0), 1, b"mg_qnet_pack: NULL pointer"),
    ("dims before alignment", "mg_qnet_pack", dict(out_dim=9, packed=ODD8), 1, PACK_DIMS),

    ("packed NULL", "mg_qnet_forward", dict(packed=None), 1, b"mg_qnet_forward: NULL pointer"),
    ("x NULL", "mg_qnet_forward", dict(x=None), 1, b"mg_qnet_forward: NULL pointer"),
    ("q NULL", "mg_qnet_forward", dict(q=None), 1, b"mg_qnet_forward: NULL pointer"),
    ("n < 0", "mg_qnet_forward", dict(n=-1), 1, b"n < 0"),
    ("in_dim 0", "mg_qnet_forward", dict(in_dim=0), 1, FWD_DIMS),
    ("in_dim 14", "mg_qnet_forward", dict(in_dim=14), 1, FWD_DIMS),
    ("swap_halves with in_dim 11", "mg_qnet_forward", dict(in_dim=11, swap=1), 1, FWD_DIMS),
    ("packed misaligned", "mg_qnet_forward", dict(packed=ODD8), 1, b"packed net must be 16-byte aligned"),
    ("NULL before n", "mg_qnet_forward", dict(q=None, n=-1), 1, b"mg_qnet_forward: NULL pointer"),
    ("n before in_dim", "mg_qnet_forward", dict(n=-1, in_dim=0), 1, b"n < 0"),
    ("in_dim before alignment", "mg_qnet_forward", dict(in_dim=14, packed=ODD8), 1, FWD_DIMS),
    ("alignment before the empty batch", "mg_qnet_forward", dict(n=0, packed=ODD8), 1,
     b"packed net must be 16-byte aligned"),

    ("packed NULL", "mg_qnet_fragments", dict(packed=None), 1, b"mg_qnet_fragments: NULL pointer"),
    ("fragments NULL", "mg_qnet_fragments", dict(fragments=None), 1, b"mg_qnet_fragments: NULL pointer"),
    ("packed misaligned", "mg_qnet_fragments", dict(packed=ODD8), 1, FRAG_ALIGN),
    ("fragments misaligned", "mg_qnet_fragments", dict(fragments=ODD8), 1, FRAG_ALIGN),
    ("NULL before alignment", "mg_qnet_fragments", dict(packed=None, fragments=ODD8), 1,
     b"mg_qnet_fragments: NULL pointer"),
] + [(f"{k} NULL", "mg_dqn_learner_init", {k: None}, 1, b"mg_dqn_learner_init: NULL pointer")
     for k in ("learner", *TENSORS)] + [
    ("in_dim 0", "mg_dqn_learner_init", dict(in_dim=0), 1, INIT_DIMS),
    ("in_dim 14", "mg_dqn_learner_init", dict(in_dim=14), 1, INIT_DIMS),
    ("out_dim 0", "mg_dqn_learner_init", dict(out_dim=0), 1, INIT_DIMS),
    ("out_dim 9", "mg_dqn_learner_init", dict(out_dim=9), 1, INIT_DIMS),
    ("learner misaligned", "mg_dqn_learner_init", dict(learner=ODD8), 1, INIT_ALIGN),
] + [(f"{k} misaligned", "mg_dqn_learner_init", {k: ODD2}, 1, INIT_ALIGN) for k in TENSORS] + [
    ("NULL before dims", "mg_dqn_learner_init", dict(out_b=None, out_dim=9), 1, b"mg_dqn_learner_init: NULL pointer"),
    ("dims before alignment", "mg_dqn_learner_init", dict(in_dim=14, learner=ODD8), 1, INIT_DIMS),
] + [(f"{k} {v}", e, {k: v}, 0, None)  # the byte counts of out-of-range dims are zero, with no error text
     for e in ("mg_dqn_learner_bytes", "mg_dqn_learn_scratch_bytes")
     for k, v in (("in_dim", 0), ("in_dim", 14), ("out_dim", 0), ("out_dim", 9))] + [
    ("batch 0", "mg_dqn_learn_scratch_bytes", dict(batch=0), 0, None),
    ("batch 1025", "mg_dqn_learn_scratch_bytes", dict(batch=1025), 0, None),
]


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _struct(cls, fields):
    return cls(**{k: _ptr(v) for k, v in fields.items()})


def _call(entry, over):
    """Call `entry` with arguments that pass every check, except for `over`; (return value, error text)."""
    from merging_gym import _native

    a = dict(over)
    g = a.pop
    if entry in ROLLOUTS:
        P = _native.default_params()
        for k, v in g("params", {}).items():
            setattr(P, k, v)
        P = None if g("no_params", False) else ctypes.byref(P)
        state = {n: FAKE for n, _ in _native.State._fields_}
        state.update(g("state", {}))
        st = None if g("no_state", False) else ctypes.byref(_struct(_native.State, state))
        traj = None if g("no_traj", False) else ctypes.byref(_struct(_native.Traj, g("traj", {})))
        n, num_steps, flags = g("n", 16), g("num_steps", 4), g("flags", AUTORESET)
    if entry == "mg_rollout_random":
        args = (P, st, traj, None, n, 0, 1, 0, num_steps, 1, flags, None)
    elif entry == "mg_rollout_qnet":
        args = (P, st, traj, None, n, 0, 1, 0, num_steps, _ptr(g("net", FAKE)), g("out_dim", 5), 1 << 31,
                g("mode", 0), 1 << 31, _ptr(g("opp_net", None)), flags, None)
    elif entry == "mg_rollout_hdqn":
        ht = ctypes.byref(_struct(_native.HdqnTraj, g("htraj", {})))
        args = (P, st, traj, ht, None, _ptr(g("goal", FAKE)), _ptr(g("goal_op", None)), _ptr(g("ext_acc", None)), n, 0,
                1, 0, num_steps, _ptr(g("meta", FAKE)), g("num_goals", 3), _ptr(g("lower", FAKE)), g("reset_goal", 0),
                1 << 31, g("mode", 0), _ptr(g("opp_meta", None)), _ptr(g("opp_lower", None)), _ptr(g("ring", None)),
                _ptr(g("counter", None)), g("cap", 0), flags, None)
    elif entry == "mg_qnet_pack":
        args = (*[_ptr(g(k, FAKE)) for k in TENSORS], g("in_dim", 10), g("out_dim", 5), _ptr(g("packed", FAKE)), None)
    elif entry == "mg_qnet_forward":
        args = (_ptr(g("packed", FAKE)), _ptr(g("x", FAKE)), g("in_dim", 10), g("swap", 0), _ptr(g("q", FAKE)),
                g("n", 4), None)
    elif entry == "mg_qnet_fragments":
        args = (_ptr(g("packed", FAKE)), _ptr(g("fragments", FAKE)), None)
    elif entry == "mg_dqn_learner_init":
        args = (*[_ptr(g(k, FAKE)) for k in ("learner", *TENSORS)], g("in_dim", 10), g("out_dim", 5), None)
    elif entry == "mg_dqn_learner_bytes":
        args = (g("in_dim", 10), g("out_dim", 5))
    elif entry == "mg_dqn_learn_scratch_bytes":
        args = (g("batch", 32), g("in_dim", 10), g("out_dim", 5))
    assert not a, f"unknown overrides {a}"
    rc = getattr(_native.lib, entry)(*args)
    return rc, (None if entry.endswith("_bytes") else _native.lib.mg_last_error())


@pytest.mark.parametrize("case,entry,over,code,text", TABLE, ids=[f"{r[1]}-{r[0]}" for r in TABLE])
def test_refusal(case, entry, over, code, text):
    assert _call(entry, over) == (code, text)


def test_the_arguments_behind_the_overrides_pass_every_check():
    """With no env to step the same calls return success, and in-range dims give byte counts."""
    for entry in ROLLOUTS:
        assert _call(entry, dict(n=0))[0] == 0
    assert _call("mg_qnet_forward", dict(n=0))[0] == 0
    assert _call("mg_dqn_learner_bytes", {})[0] > 0 and _call("mg_dqn_learn_scratch_bytes", {})[0] > 0
