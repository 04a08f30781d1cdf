"""The exact text and code of every refusal of the Rainbow entry points, in the style of
tests/test_refusal_texts.py: the argument checks run before any launch, so fake, never-dereferenced pointers
drive them on a host without a GPU. A row with two bad arguments pins which check fires first."""
import ctypes

import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2
AUTORESET = 1           # MG_AUTORESET

TENSORS = ("linear1_w", "linear1_b", "linear2_w", "linear2_b", "value1_w", "value1_b", "value2_w", "value2_b",
           "advantage1_w", "advantage1_b", "advantage2_w", "advantage2_b", "support")
DIMS = ("in_dim", "hidden1", "hidden2", "hidden_stream", "num_actions", "num_atoms")
GOOD_DIMS = dict(zip(DIMS, (10, 32, 64, 64, 5, 51)))

ALIGN = b"traj.obs must be 16-byte, rew/final_obs 8-byte, flags 4-byte aligned"
SHAPE = b"mg_rainbow_pack: only RainbowDQN(10, 5) is packed: in_dim 10, hidden 32 / 64 / 64, 5 actions, 51 atoms"
PACK_NULL = b"mg_rainbow_pack: NULL pointer"
PACK_ALIGN4 = b"mg_rainbow_pack: the tensors must be 4-byte aligned"
FWD_NET = b"mg_rainbow_forward: packed must be a 16-byte aligned packed Rainbow net"
FWD_ROT = b"mg_rainbow_forward: need 0 <= rotate < 10"
FWD_ALIGN = b"mg_rainbow_forward: obs, logits and q must be 4-byte aligned"
RO_NET = b"mg_rollout_rainbow: net must be a 16-byte aligned packed Rainbow net"
RO_MODE = b"mg_rollout_rainbow: opponent_mode must be 0 (None) or 2 (the same net on state[3:] + state[:3])"
STEPS = b"need 0 <= num_steps <= 65535 (split longer rollouts)"
HEAD_NULL = b"mg_host_rainbow_head: logits or support is NULL"
HEAD_ALIGN = b"mg_host_rainbow_head: logits, support and q must be 4-byte aligned"

# (case, entry point, overrides, return code, mg_last_error())
TABLE = [(f"{k} NULL", "mg_rainbow_pack", {k: None}, 1, PACK_NULL) for k in (*TENSORS, "packed")] + [
    (f"{k} off by one", "mg_rainbow_pack", {k: GOOD_DIMS[k] + 1}, 1, SHAPE) for k in DIMS] + [
    ("the DQN's Net", "mg_rainbow_pack", dict(hidden1=200, hidden2=100), 1, SHAPE),
    ("packed misaligned", "mg_rainbow_pack", dict(packed=ODD8), 1, b"mg_rainbow_pack: packed buffer must be 16-byte aligned"),
    ("tensor misaligned", "mg_rainbow_pack", dict(value2_b=ODD2), 1, PACK_ALIGN4),
    ("NULL before shape", "mg_rainbow_pack", dict(support=None, num_atoms=11), 1, PACK_NULL),
    ("shape before alignment", "mg_rainbow_pack", dict(num_actions=3, packed=ODD8), 1, SHAPE),

    ("obs NULL", "mg_rainbow_forward", dict(obs=None), 1, b"mg_rainbow_forward: obs is NULL"),
    ("packed NULL", "mg_rainbow_forward", dict(packed=None), 1, FWD_NET),
    ("packed misaligned", "mg_rainbow_forward", dict(packed=ODD8), 1, FWD_NET),
    ("rotate -1", "mg_rainbow_forward", dict(rotate=-1), 1, FWD_ROT),
    ("rotate 10", "mg_rainbow_forward", dict(rotate=10), 1, FWD_ROT),
    ("n < 0", "mg_rainbow_forward", dict(n=-1), 1, b"n < 0"),
    ("n past the grid", "mg_rainbow_forward", dict(n=0x7fffffff * 256 + 1), 1, b"n exceeds the grid limit"),
    ("q misaligned", "mg_rainbow_forward", dict(q=ODD2), 1, FWD_ALIGN),
    ("logits misaligned", "mg_rainbow_forward", dict(logits=ODD2), 1, FWD_ALIGN),
    ("obs before packed", "mg_rainbow_forward", dict(obs=None, packed=None), 1, b"mg_rainbow_forward: obs is NULL"),
    ("packed before rotate", "mg_rainbow_forward", dict(packed=ODD8, rotate=10), 1, FWD_NET),
    ("rotate before n", "mg_rainbow_forward", dict(rotate=10, n=-1), 1, FWD_ROT),
    ("alignment before the empty batch", "mg_rainbow_forward", dict(n=0, q=ODD2), 1, FWD_ALIGN),

    ("params NULL", "mg_rollout_rainbow", dict(no_params=True), 1, b"params is NULL"),
    ("n < 0", "mg_rollout_rainbow", dict(n=-1), 1, b"n < 0"),
    ("state array NULL", "mg_rollout_rainbow", dict(state=dict(tf=None)), 1, b"mg_state has a NULL array"),
    ("traj NULL", "mg_rollout_rainbow", dict(no_traj=True), 1, b"traj is NULL (pass a zeroed mg_traj)"),
    ("net NULL", "mg_rollout_rainbow", dict(net=None), 1, RO_NET),
    ("net misaligned", "mg_rollout_rainbow", dict(net=ODD8), 1, RO_NET),
    ("num_steps < 0", "mg_rollout_rainbow", dict(num_steps=-1), 1, STEPS),
    ("num_steps > 65535", "mg_rollout_rainbow", dict(num_steps=65536), 1, STEPS),
    ("mode 1 (uniform)", "mg_rollout_rainbow", dict(mode=1), 1, RO_MODE),
    ("mode 3", "mg_rollout_rainbow", dict(mode=3), 1, RO_MODE),
    ("mode -1", "mg_rollout_rainbow", dict(mode=-1), 1, RO_MODE),
    ("traj.obs misaligned", "mg_rollout_rainbow", dict(traj=dict(obs=ODD8)), 1, ALIGN),
    ("traj.flags misaligned", "mg_rollout_rainbow", dict(traj=dict(flags=ODD2)), 1, ALIGN),
    ("traj before net", "mg_rollout_rainbow", dict(no_traj=True, net=None), 1, b"traj is NULL (pass a zeroed mg_traj)"),
    ("net before num_steps", "mg_rollout_rainbow", dict(net=ODD8, num_steps=-1), 1, RO_NET),
    ("num_steps before mode", "mg_rollout_rainbow", dict(num_steps=65536, mode=1), 1, STEPS),
    ("mode before alignment", "mg_rollout_rainbow", dict(mode=1, traj=dict(rew=ODD4)), 1, RO_MODE),
    ("alignment before the empty batch", "mg_rollout_rainbow", dict(num_steps=0, traj=dict(flags=ODD2)), 1, ALIGN),

    ("n < 0", "mg_host_rainbow_head", dict(n=-1), 1, b"n < 0"),
    ("logits NULL", "mg_host_rainbow_head", dict(logits=None), 1, HEAD_NULL),
    ("support NULL", "mg_host_rainbow_head", dict(support=None), 1, HEAD_NULL),
    ("logits misaligned", "mg_host_rainbow_head", dict(logits=ODD2), 1, HEAD_ALIGN),
    ("q misaligned", "mg_host_rainbow_head", dict(q=ODD2), 1, HEAD_ALIGN),
    ("n before NULL", "mg_host_rainbow_head", dict(n=-1, logits=None), 1, b"n < 0"),
    ("x NULL", "mg_host_rainbow_exp", dict(x=None), 1, b"mg_host_rainbow_exp: NULL pointer"),
    ("y NULL", "mg_host_rainbow_exp", dict(y=None), 1, b"mg_host_rainbow_exp: NULL pointer"),
]


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _struct(cls, fields):
    return cls(**{k: _ptr(v) for k, v in fields.items()})


def _call(entry, over):
    """Call `entry` with arguments that pass every check, except for `over`; (return value, error text). The
    host entry points get n = 0 unless overridden, so a fake pointer is never read."""
    from merging_gym import _native

    a = dict(over)
    g = a.pop
    if entry == "mg_rainbow_pack":
        args = (*[_ptr(g(k, FAKE)) for k in TENSORS], *[g(k, GOOD_DIMS[k]) for k in DIMS], _ptr(g("packed", FAKE)), None)
    elif entry == "mg_rainbow_forward":
        args = (_ptr(g("packed", FAKE)), _ptr(g("obs", FAKE)), g("rotate", 3), _ptr(g("logits", FAKE)),
                _ptr(g("q", FAKE)), _ptr(g("action", FAKE)), g("n", 4), None)
    elif entry == "mg_rollout_rainbow":
        P = _native.default_params()
        P = None if g("no_params", False) else ctypes.byref(P)
        state = {n: FAKE for n, _ in _native.State._fields_}
        state.update(g("state", {}))
        st = ctypes.byref(_struct(_native.State, state))
        traj = None if g("no_traj", False) else ctypes.byref(_struct(_native.Traj, g("traj", {})))
        args = (P, st, traj, None, g("n", 16), g("num_steps", 4), _ptr(g("net", FAKE)), g("mode", 2), AUTORESET, None)
    elif entry == "mg_host_rainbow_head":
        args = (_ptr(g("logits", FAKE)), _ptr(g("support", FAKE)), _ptr(g("q", FAKE)), _ptr(g("action", FAKE)), g("n", 0))
    elif entry == "mg_host_rainbow_exp":
        args = (_ptr(g("x", FAKE)), _ptr(g("y", FAKE)), g("n", 0))
    assert not a, f"unknown overrides {a}"
    rc = getattr(_native.lib, entry)(*args)
    return rc, _native.lib.mg_last_error()


@pytest.mark.parametrize("case,entry,over,code,text", TABLE, ids=[f"{r[1]}-{r[0]}" for r in TABLE])
def test_refusal(case, entry, over, code, text):
    assert _call(entry, over) == (code, text)


def test_the_arguments_behind_the_overrides_pass_every_check():
    """With nothing to compute the same calls return success, and the packed size is the documented one."""
    from merging_gym import _native

    assert _call("mg_rainbow_forward", dict(n=0))[0] == 0
    assert _call("mg_rollout_rainbow", dict(n=0))[0] == 0
    assert _call("mg_rollout_rainbow", dict(num_steps=0, mode=0))[0] == 0
    assert _call("mg_host_rainbow_head", {}) == (0, b"")
    assert _call("mg_host_rainbow_exp", {}) == (0, b"")
    assert _native.lib.mg_rainbow_packed_bytes() == 74192
    assert _native.lib.mg_abi_version() == 21  # the entry points are additive
