"""A population of DQN learners without a GPU: the host twin (mg_host_dqn_learn_many) against the
plain-C restatement run once per member, bit for bit; what the entry points refuse, the size helpers at
their edges, K updates in one call against K calls; the public interface of merging_gym.DQNPopulation;
and the host code under AddressSanitizer and UndefinedBehaviorSanitizer in a stand-alone program."""

import ctypes
import inspect

import numpy as np
import pytest

import learn_many_ref as mr
import learn_ref as lr
from native_build import hipcc, run_sanitized_driver


# ------------------------------------------------------------------ 1. host twin == restatement
@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch", [(10, 5, 5), (11, 5, 32), (10, 3, 128)])
def test_host_population_equals_restatement_bit_for_bit(in_dim, out_dim, batch, filled_only):
    """Three members that differ in seed, lr, gamma, betas, eps, target_period, first_update, first_draw
    and ring, four updates: in update 1 member 2 copies its target and members 0 and 1 do not."""
    _, rings, counters, kws, L0, ref_end, ref_loss, ref_rows = mr.reference(in_dim, out_dim, batch, 3, filled_only)
    masks = mr.sync_masks(kws, mr.UPDATES)
    assert any(0 < len(s) < 3 for s in masks)
    got, loss, rows, (arr, _) = mr.run_host_many(L0, rings, counters, kws, in_dim, out_dim, batch, mr.UPDATES,
                                                 filled_only)
    mr.assert_members_equal(got, loss, rows, ref_end, ref_loss, ref_rows)
    for m, kw in enumerate(kws):  # the call advanced the members' counters
        assert (arr[m].first_update, arr[m].first_draw) == (kw["first_update"] + 4, kw["first_draw"] + 4)
        assert not np.array_equal(got[m, 0], L0[m, 0]) and not np.array_equal(got[m, 1], L0[m, 1])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(loss))
    assert len({rows[0, m].tobytes() for m in range(3)}) == 3  # own rings, own draws


def test_one_call_of_k_updates_equals_k_calls_on_the_host():
    _, rings, counters, kws, L0, *_ = mr.reference(10, 5, 5, 3, False)
    one, loss, rows, _ = mr.run_host_many(L0, rings, counters, kws, 10, 5, 5, 4)
    L, members, losses = L0, None, []
    for _ in range(4):  # the member array carries the counters from call to call
        L, l1, _, members = mr.run_host_many(L, rings, counters, kws, 10, 5, 5, 1, members=members)
        losses.append(l1[0])
    assert np.array_equal(lr.bits(L), lr.bits(one)) and np.array_equal(lr.bits(np.stack(losses)), lr.bits(loss))


# ------------------------------------------------------------------ 2. what the entry points refuse
def test_population_argument_errors_without_gpu():
    from merging_gym import _native

    lib = _native.lib
    assert lib.mg_abi_version() == 21
    assert ctypes.sizeof(_native.DqnMember) == 5 * 8 + ctypes.sizeof(_native.DqnHyper) == 88
    assert lib.mg_dqn_learn_many_table_bytes(0) == 0 and lib.mg_dqn_learn_many_table_bytes(65) == 0
    assert lib.mg_dqn_learn_many_table_bytes(1) == 48 and lib.mg_dqn_learn_many_table_bytes(64) == 64 * 48
    assert lib.mg_dqn_learn_many_table_bytes(-1) == 0

    fake = 1 << 20  # never dereferenced: validation fails first
    one = lib.mg_dqn_learn_scratch_bytes(128, 10, 5)
    packed = lib.mg_qnet_packed_bytes()

    def members(n=3, edits=None):
        arr = (_native.DqnMember * max(n, 1))()
        for m in range(max(n, 1)):
            arr[m] = _native.DqnMember(fake, fake, m, 0, 0, lr.hyper_struct(100))
        for (m, field), v in (edits or {}).items():
            if field in ("rows", "counter", "seed"):
                setattr(arr[m], field, v)
            else:
                setattr(arr[m].hyper, field, v)
        return arr

    good = dict(learners=fake, table=fake, table_bytes=3 * 48, member=members(), members=3, capacity=2000,
                row_floats=22, in_dim=10, out_dim=5, batch=128, num_updates=1, filled_only=0, loss_out=None,
                rows_out=None, packed_out=None, packed_stride=packed, scratch=fake, scratch_bytes=3 * one)

    def call(host=False, **kw):
        a = dict(good, **kw)
        mid = [a["member"], a["members"], a["capacity"], a["row_floats"], a["in_dim"], a["out_dim"], a["batch"],
               a["num_updates"], a["filled_only"], a["loss_out"], a["rows_out"]]
        if host:
            return lib.mg_host_dqn_learn_many(a["learners"], *mid, a["scratch"], a["scratch_bytes"])
        return lib.mg_dqn_learn_many(a["learners"], a["table"], a["table_bytes"], *mid, a["packed_out"],
                                     a["packed_stride"], a["scratch"], a["scratch_bytes"], None)

    def refused(msg, both=True, **kw):
        for host in ((False, True) if both else (False,)):
            assert call(host=host, **kw) != 0
            err = lib.mg_last_error()
            assert msg in err and err.startswith(b"mg_host_dqn_learn_many: " if host else b"mg_dqn_learn_many: "), err

    for n in (0, 65, -1):
        refused(b"need 1 <= members <= 64", members=n)
    for name in ("learners", "member", "scratch"):
        refused(b"NULL pointer", **{name: None})
    refused(b"NULL pointer", both=False, table=None)
    refused(b"NULL pointer", member=members(edits={(1, "rows"): None}))
    refused(b"NULL pointer", member=members(edits={(2, "counter"): None}), filled_only=1)
    assert call(host=True, member=members(edits={(2, "counter"): None}), num_updates=0) == 0  # read only with filled_only
    for bad in (dict(in_dim=0, row_floats=2), dict(in_dim=14, row_floats=30), dict(out_dim=0), dict(out_dim=9)):
        refused(b"1 <= in_dim <= 13, 1 <= out_dim <= 8", **bad)
    refused(b"row_floats must be 2 * in_dim + 2", row_floats=24)
    refused(b"1 <= batch <= 1024", batch=0)
    refused(b"1 <= batch <= 1024", batch=1025)
    refused(b"capacity", capacity=0)
    refused(b"capacity", capacity=(1 << 32) + 1)
    refused(b"num_updates", num_updates=-1)
    refused(b"member 1: target_period must be >= 1", member=members(edits={(1, "target_period"): 0}))
    refused(b"member 2: need 0 <= beta1 < 1 and 0 <= beta2 < 1", member=members(edits={(2, "beta1"): 1.0}))
    refused(b"member 0: need 0 <= beta1 < 1 and 0 <= beta2 < 1", member=members(edits={(0, "beta2"): -0.1}))
    refused(b"member 1: rows and counter must be 8-byte aligned", member=members(edits={(1, "rows"): fake + 4}))
    refused(b"member 2: rows and counter must be 8-byte aligned", member=members(edits={(2, "counter"): fake + 4}))
    refused(b"aligned", learners=fake + 8)
    refused(b"aligned", scratch=fake + 8)
    refused(b"aligned", loss_out=fake + 2)
    refused(b"aligned", rows_out=fake + 2)
    refused(b"aligned", both=False, packed_out=fake + 8)
    refused(b"packed_stride a multiple of 16", both=False, packed_out=fake, packed_stride=packed + 8)
    refused(b"packed_stride smaller than mg_qnet_packed_bytes()", both=False, packed_out=fake, packed_stride=packed - 16)
    refused(b"table must be 16-byte aligned", both=False, table=fake + 8)
    refused(b"scratch smaller than members * mg_dqn_learn_scratch_bytes", scratch_bytes=3 * one - 4)
    refused(b"table smaller than mg_dqn_learn_many_table_bytes(members)", both=False, table_bytes=3 * 48 - 1)
    # nothing to do is a success before anything is read, and leaves the counters alone
    arr = members()
    assert call(num_updates=0, member=arr) == 0 and call(host=True, num_updates=0, member=arr) == 0
    assert (arr[0].first_update, arr[0].first_draw) == (0, 0)

    def init(**kw):
        a = dict(table=fake, table_bytes=3 * 48, member=members(), members=3)
        a.update(kw)
        return lib.mg_dqn_learn_many_init(a["table"], a["table_bytes"], a["member"], a["members"], None)

    for kw, msg in ((dict(members=0), b"need 1 <= members <= 64"), (dict(members=65), b"need 1 <= members <= 64"),
                    (dict(member=None), b"NULL pointer"), (dict(table=None), b"NULL pointer"),
                    (dict(member=members(edits={(0, "rows"): None})), b"NULL pointer"),
                    (dict(member=members(edits={(1, "target_period"): 0})), b"member 1: target_period must be >= 1"),
                    (dict(member=members(edits={(2, "beta2"): 1.0})), b"member 2: need 0 <= beta1 < 1"),
                    (dict(table=fake + 8), b"table must be 16-byte aligned"),
                    (dict(table_bytes=3 * 48 - 1), b"table smaller than mg_dqn_learn_many_table_bytes(members)")):
        assert init(**kw) != 0
        err = lib.mg_last_error()
        assert msg in err and err.startswith(b"mg_dqn_learn_many_init: "), err


# ------------------------------------------------------------------ 3. the public interface
def test_population_class_is_reachable_and_has_the_stated_signatures():
    import merging_gym

    cls = merging_gym.DQNPopulation
    assert cls.__name__ == "DQNPopulation"
    assert merging_gym.__all__ == ["MergeEnv", "MergeEnvExtend", "MergeVecEnv", "ReplayRing", "DQNLearner",
                                   "RainbowNet", "RainbowReplay", "RainbowLearner", "make", "ENV_IDS"]

    def params(f):
        return [(p.name, p.default) for p in list(inspect.signature(f).parameters.values())[1:]]

    E = inspect.Parameter.empty
    assert params(cls.__init__) == [("nets", E), ("rings", E), ("lr", 0.01), ("gamma", 0.9), ("batch_size", 128),
                                    ("target_period", 100), ("betas", (0.9, 0.999)), ("eps", 1e-8), ("seed", 0),
                                    ("device", None)]
    assert params(cls.learn) == [("num_updates", 1), ("filled_only", False), ("return_loss", False),
                                 ("return_rows", False)]
    for name in ("qnets", "eval_state_dict", "target_state_dict", "member_state_dict", "load_member_state_dict",
                 "state_dict", "load_state_dict", "copy_member", "__len__", "learn_step_counter", "draw_counter"):
        assert name == "qnets" or hasattr(cls, name), name


# ------------------------------------------------------------------ 4. the host code under the sanitizers
@pytest.mark.skipif(hipcc() is None, reason="hipcc not found")
def test_population_host_code_under_asan_ubsan(tmp_path):
    """tests/native/learn_many_sanitize.cpp (its own main): the host twin on exactly sized heap buffers at
    M = 3, B = 5 and M = 64, B = 1; the device entry points only refuse. No GPU, nothing loaded into Python."""
    r = run_sanitized_driver("learn_many_sanitize", tmp_path)
    assert r.returncode == 0, r.stdout + r.stderr[-2000:]
    assert "learn_many sanitizer run: 0 failures" in r.stdout
