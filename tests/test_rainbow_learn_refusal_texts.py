"""The exact text and code of every refusal of the Rainbow learning entry points, in the style of
tests/test_rainbow_refusal_texts.py: the argument checks run before any launch or read, so fake,
never-dereferenced pointers drive them on a host without a GPU. A row with two bad arguments pins which check
fires first."""
import ctypes

import pytest

FAKE = 1 << 20          # 16-byte aligned
ODD8 = (1 << 20) + 8    # 8-byte aligned only
ODD4 = (1 << 20) + 4
ODD2 = (1 << 20) + 2

ST = "mg_rainbow_replay_store"
ST_NULL = b"mg_rainbow_replay_store: NULL pointer"
ST_CAP = b"mg_rainbow_replay_store: need 1 <= capacity <= 2^32"
ST_NEG = b"mg_rainbow_replay_store: n < 0 or num_steps < 0"
ST_EXTRA = b"mg_rainbow_replay_store: goal, next_goal, reward and meta_goal must be NULL (Rainbow rows have none)"
ST_REQ = b"mg_rainbow_replay_store: obs_first, obs, a1 (or flags) and rew are required"
ST_ALIGN = b"mg_rainbow_replay_store: rows and counter must be 8-byte, the float buffers 4-byte aligned"
ST_GRID = b"mg_rainbow_replay_store: n * num_steps exceeds the grid limit"


def learn_texts(what):
    w = what.encode()
    return dict(null=w + b": NULL pointer", batch=w + b": need 1 <= batch <= 1024",
                cap=w + b": need 1 <= capacity <= 2^32", neg=w + b": num_updates < 0",
                noise=w + b": noise is NULL (num_updates x 2 x 1124 factors)",
                beta=w + b": need 0 <= beta1 < 1 and 0 <= beta2 < 1",
                align=w + b": learner, scratch and packed_out must be 16-byte, rows and counter 8-byte, noise and the "
                          b"optional outputs 4-byte aligned",
                scratch=w + b": scratch smaller than mg_rainbow_learn_scratch_bytes(batch)")


def learn_rows(what, device):
    t = learn_texts(what)
    rows = [(f"{k} NULL", what, {k: None}, 1, t["null"]) for k in ("learner", "rows", "counter", "scratch")] + [
        ("hyper NULL", what, dict(no_hyper=True), 1, t["null"]),
        ("batch 0", what, dict(batch=0), 1, t["batch"]),
        ("batch 1025", what, dict(batch=1025), 1, t["batch"]),
        ("capacity 0", what, dict(capacity=0), 1, t["cap"]),
        ("capacity 2^32 + 1", what, dict(capacity=(1 << 32) + 1), 1, t["cap"]),
        ("num_updates -1", what, dict(num_updates=-1), 1, t["neg"]),
        ("noise NULL", what, dict(noise=None), 1, t["noise"]),
        ("beta1 1", what, dict(beta1=1.0), 1, t["beta"]),
        ("beta2 -0.1", what, dict(beta2=-0.1), 1, t["beta"]),
        ("learner misaligned", what, dict(learner=ODD8), 1, t["align"]),
        ("rows misaligned", what, dict(rows=ODD4), 1, t["align"]),
        ("counter misaligned", what, dict(counter=ODD4), 1, t["align"]),
        ("noise misaligned", what, dict(noise=ODD2), 1, t["align"]),
        ("loss_out misaligned", what, dict(loss_out=ODD2), 1, t["align"]),
        ("proj_out misaligned", what, dict(proj_out=ODD2), 1, t["align"]),
        ("grads_out misaligned", what, dict(grads_out=ODD2), 1, t["align"]),
        ("scratch misaligned", what, dict(scratch=ODD8), 1, t["align"]),
        ("scratch one byte short", what, dict(scratch_short=1), 1, t["scratch"]),
        ("NULL before batch", what, dict(rows=None, batch=0), 1, t["null"]),
        ("batch before capacity", what, dict(batch=0, capacity=0), 1, t["batch"]),
        ("capacity before num_updates", what, dict(capacity=0, num_updates=-1), 1, t["cap"]),
        ("noise before beta", what, dict(noise=None, beta1=2.0), 1, t["noise"]),
        ("beta before alignment", what, dict(beta2=1.0, rows=ODD4), 1, t["beta"]),
        ("alignment before scratch size", what, dict(rows_out=ODD2, scratch_short=8), 1, t["align"]),
    ]
    if device:
        rows.append(("packed_out misaligned", what, dict(packed_out=ODD8), 1, t["align"]))
    return rows


# (case, entry point, overrides, return code, mg_last_error())
TABLE = [(f"{k} NULL", ST, {k: None}, 1, ST_NULL) for k in ("rows", "counter")] + [
    ("tr NULL", ST, dict(no_tr=True), 1, ST_NULL),
    ("capacity 0", ST, dict(capacity=0), 1, ST_CAP),
    ("capacity 2^32 + 1", ST, dict(capacity=(1 << 32) + 1), 1, ST_CAP),
    ("n < 0", ST, dict(n=-1), 1, ST_NEG),
    ("num_steps < 0", ST, dict(num_steps=-1), 1, ST_NEG),
] + [(f"{k} set", ST, dict(tr={k: FAKE}), 1, ST_EXTRA) for k in ("goal", "next_goal", "reward", "meta_goal")] + [
    (f"{k} NULL", ST, dict(tr={k: None}), 1, ST_REQ) for k in ("obs_first", "obs", "rew")] + [
    ("a1 and flags NULL", ST, dict(tr=dict(a1=None)), 1, ST_REQ),
    ("rows misaligned", ST, dict(rows=ODD4), 1, ST_ALIGN),
    ("counter misaligned", ST, dict(counter=ODD4), 1, ST_ALIGN),
    ("obs misaligned", ST, dict(tr=dict(obs=ODD2)), 1, ST_ALIGN),
    ("final_obs misaligned", ST, dict(tr=dict(final_obs=ODD2)), 1, ST_ALIGN),
    ("rew misaligned", ST, dict(tr=dict(rew=ODD2)), 1, ST_ALIGN),
    ("past the grid", ST, dict(n=1 << 40, num_steps=2), 1, ST_GRID),
    ("NULL before capacity", ST, dict(rows=None, capacity=0), 1, ST_NULL),
    ("capacity before n", ST, dict(capacity=0, n=-1), 1, ST_CAP),
    ("extra before the empty batch", ST, dict(n=0, tr=dict(goal=FAKE)), 1, ST_EXTRA),
    ("required before alignment", ST, dict(rows=ODD4, tr=dict(rew=None)), 1, ST_REQ),
] + learn_rows("mg_rainbow_learn", True) + learn_rows("mg_host_rainbow_learn", False) + [
    ("n < 0", "mg_host_rainbow_project", dict(n=-1), 1, b"n < 0"),
] + [(f"{k} NULL", "mg_host_rainbow_project", {k: None}, 1, b"mg_host_rainbow_project: NULL pointer")
     for k in ("next_dist", "reward", "done", "support", "proj")] + [
    (f"{k} misaligned", "mg_host_rainbow_project", {k: ODD2}, 1,
     b"mg_host_rainbow_project: the arrays must be 4-byte aligned") for k in ("next_dist", "reward", "proj")] + [
    ("n before NULL", "mg_host_rainbow_project", dict(n=-1, proj=None), 1, b"n < 0"),
    ("n < 0", "mg_host_rainbow_log", dict(n=-1), 1, b"n < 0"),
    ("x NULL", "mg_host_rainbow_log", dict(x=None), 1, b"mg_host_rainbow_log: NULL pointer"),
    ("y NULL", "mg_host_rainbow_log", dict(y=None), 1, b"mg_host_rainbow_log: NULL pointer"),
]


def _ptr(v):
    return None if v is None else ctypes.c_void_p(v)


def _call(entry, over):
    """Call `entry` with arguments that pass every check, except for `over`; (return value, error text)."""
    from merging_gym import _native

    a = dict(over)
    g = a.pop
    if entry == ST:
        fields = dict(obs_first=FAKE, obs=FAKE, final_obs=FAKE, a1=FAKE, rew=FAKE, done=FAKE)
        fields.update(g("tr", {}))
        tr = None if g("no_tr", False) else ctypes.byref(_native.Transitions(**{k: _ptr(v) for k, v in fields.items()}))
        args = (_ptr(g("rows", FAKE)), _ptr(g("counter", FAKE)), g("capacity", 100), tr, g("n", 4), g("num_steps", 2), None)
    elif entry in ("mg_rainbow_learn", "mg_host_rainbow_learn"):
        batch = g("batch", 32)
        hyper = _native.DqnHyper(0.001, 0.99, g("beta1", 0.9), g("beta2", 0.999), 1e-8, 1, 0)
        nbytes = _native.lib.mg_rainbow_learn_scratch_bytes(32) - g("scratch_short", 0)
        args = [_ptr(g("learner", FAKE)), _ptr(g("rows", FAKE)), _ptr(g("counter", FAKE)), g("capacity", 100), batch,
                g("num_updates", 1), 0, 0, 0, None if g("no_hyper", False) else ctypes.byref(hyper),
                _ptr(g("noise", FAKE)), _ptr(g("loss_out", FAKE)), _ptr(g("rows_out", FAKE)), _ptr(g("proj_out", FAKE)),
                _ptr(g("grads_out", FAKE))]
        if entry == "mg_rainbow_learn":
            args += [_ptr(g("packed_out", FAKE))]
        args += [_ptr(g("scratch", FAKE)), nbytes]
        if entry == "mg_rainbow_learn":
            args += [None]
    elif entry == "mg_host_rainbow_project":
        args = (_ptr(g("next_dist", FAKE)), _ptr(g("reward", FAKE)), _ptr(g("done", FAKE)), _ptr(g("support", FAKE)), 0.99,
                _ptr(g("proj", FAKE)), g("n", 0))
    elif entry == "mg_host_rainbow_log":
        args = (_ptr(g("x", FAKE)), _ptr(g("y", FAKE)), g("n", 0))
    assert not a, f"unknown overrides {a}"
    rc = getattr(_native.lib, entry)(*args)
    return rc, _native.lib.mg_last_error()


@pytest.mark.parametrize("case,entry,over,code,text", TABLE, ids=[f"{r[1]}-{r[0]}" for r in TABLE])
def test_refusal(case, entry, over, code, text):
    assert _call(entry, over) == (code, text)


def test_the_arguments_behind_the_overrides_pass_every_check():
    """With nothing to compute the same calls return success, and the sizes are the documented ones."""
    from merging_gym import _native

    assert _call(ST, dict(n=0))[0] == 0
    assert _call(ST, dict(num_steps=0))[0] == 0
    assert _call("mg_host_rainbow_project", {}) == (0, b"")
    assert _call("mg_host_rainbow_log", {}) == (0, b"")
    assert _native.lib.mg_rainbow_learner_bytes() == 4 * (4 * 58884 + 2 * 28210 + 52)
    assert _native.lib.mg_rainbow_learn_scratch_bytes(0) == 0 and _native.lib.mg_rainbow_learn_scratch_bytes(1025) == 0
    assert _native.lib.mg_rainbow_learn_scratch_bytes(32) % 16 == 0
    assert _native.lib.mg_abi_version() == 21  # the entry points are additive
