"""DQN.learn without a GPU (ABI 21): the library's host twin (mg_host_dqn_learn, the per-element
functions the kernels run) against the plain-C restatement bit for bit; the restatement against
torch's own learn() (scripts/main.py:122-157) in fp32 and fp64; and what the entry points refuse."""

import ctypes

import numpy as np
import pytest

import learn_ref as lr


# ------------------------------------------------------------------ 1. host code == restatement
@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch", lr.CASES)
def test_host_learn_equals_restatement_bit_for_bit(in_dim, out_dim, batch, filled_only):
    """Three updates with target_period 2 from update 1 (the target copy falls inside the call, before
    update 2) on a half-filled ring: eval, target, m, v, every loss and every sampled row agree bit
    for bit."""
    rows, sd = lr.case_fixture(in_dim, out_dim, batch)
    ring, counter = lr.half_filled(rows)
    L0 = lr.learner_array(sd)
    L0[1] *= np.float32(0.5)  # a target that differs from eval until the copy
    kw = dict(num_updates=3, first_update=1, seed=7, first_draw=5, filled_only=filled_only, target_period=2)
    ref, ref_loss, ref_rows, _ = lr.run_ref(L0, ring, counter, in_dim, out_dim, batch, **kw)
    got, got_loss, got_rows = lr.run_host(L0, ring, counter, in_dim, out_dim, batch, **kw)
    assert np.array_equal(lr.bits(got_rows), lr.bits(ref_rows))
    assert np.array_equal(lr.bits(got_loss), lr.bits(ref_loss)), (got_loss, ref_loss)
    for blk, name in enumerate(("eval", "target", "m", "v")):
        assert np.array_equal(lr.bits(got[blk]), lr.bits(ref[blk])), name
    # the run did something: the copy happened (target = eval before update 2, not the halved start)
    # and the parameters moved
    assert not np.array_equal(got[1], L0[1]) and not np.array_equal(got[0], L0[0])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(got_loss))
    if not filled_only:  # the unfilled half is drawn too
        assert (np.abs(got_rows).sum(axis=2) == 0).any()
    else:
        assert (np.abs(got_rows).sum(axis=2) > 0).all()


def test_one_call_of_k_updates_equals_k_calls_on_the_host():
    rows, sd = lr.case_fixture(10, 5)
    L0 = lr.learner_array(sd)
    one, loss, _ = lr.run_host(L0, rows, 2000, 10, 5, 32, 4, first_update=98, first_draw=98, target_period=100)
    L, losses = L0, []
    for u in range(4):
        L, l1, _ = lr.run_host(L, rows, 2000, 10, 5, 32, 1, first_update=98 + u, first_draw=98 + u,
                               target_period=100)
        losses.append(l1[0])
    assert np.array_equal(lr.bits(L), lr.bits(one)) and np.array_equal(lr.bits(np.array(losses)), lr.bits(loss))


# ------------------------------------------------------------------ 2. restatement vs torch fp32 / fp64
def _torch_learn(sd, batches, in_dim, dtype, updates):
    """The reference's learn() (main.py:122-157) in torch at `dtype` on the given minibatches:
    per update (loss, gradients by name, parameters by name)."""
    import torch
    import torch.nn as nn
    import torch.nn.functional as F

    class Net(nn.Module):  # main.py:30-47
        def __init__(self, out_dim):
            super().__init__()
            self.fc1, self.fc2, self.out = nn.Linear(in_dim, 200), nn.Linear(200, 100), nn.Linear(100, out_dim)

        def forward(self, x):
            return self.out(F.relu(self.fc2(F.relu(self.fc1(x)))))

    out_dim = sd["out.bias"].shape[0]
    eval_net, target_net = Net(out_dim).to(dtype), Net(out_dim).to(dtype)
    eval_net.load_state_dict({k: torch.as_tensor(v).to(dtype) for k, v in sd.items()})
    opt = torch.optim.Adam(eval_net.parameters(), lr=lr.HYPER["lr"])
    res = []
    for u in range(updates):
        if u % 100 == 0:
            target_net.load_state_dict(eval_net.state_dict())
        rows = torch.as_tensor(batches[u])
        s = rows[:, :in_dim].to(dtype)
        a = rows[:, in_dim:in_dim + 1].to(torch.int64)
        r = rows[:, in_dim + 1:in_dim + 2].to(dtype)
        s2 = rows[:, -in_dim:].to(dtype)
        q_eval = eval_net(s).gather(1, a)
        q_next = target_net(s2).detach()
        q_eval4next = eval_net(s2).detach()
        top2 = torch.topk(q_eval4next, 2, dim=1).values
        gap = float(((top2[:, 0] - top2[:, 1]) / top2.abs().max(dim=1).values).min())
        am = q_eval4next.max(1)[1]
        q_target = r + lr.HYPER["gamma"] * q_next[range(len(am)), am].view(-1, 1)
        loss = F.mse_loss(q_eval, q_target)
        opt.zero_grad()
        loss.backward()
        grads = {k: p.grad.detach().double().numpy().copy() for k, p in eval_net.named_parameters()}
        opt.step()
        params = {k: p.detach().double().numpy().copy() for k, p in eval_net.named_parameters()}
        res.append((float(loss.detach()), grads, params, gap))
    return res


def _errors(run, ref64, upto):
    """Per tensor, over the run's updates: max|g - g64| / max|g64| and max|p - p64| / lr; the loss's
    relative error."""
    g_err, p_err, l_err = {}, {}, 0.0
    for u in range(upto):
        loss, grads, params = run[u][:3]
        loss64, g64, p64 = ref64[u][:3]
        l_err = max(l_err, abs(loss - loss64) / abs(loss64))
        for k in lr.KEYS:
            diff, den = float(np.abs(grads[k] - g64[k]).max()), float(np.abs(g64[k]).max())
            g_err[k] = max(g_err.get(k, 0.0), diff / den if den > 0 else (0.0 if diff == 0 else np.inf))
            if params is not None:
                p_err[k] = max(p_err.get(k, 0.0), float(np.abs(params[k] - p64[k]).max() / lr.HYPER["lr"]))
    return g_err, p_err, l_err


def _ours(sd, rows, in_dim, out_dim, batch, updates, seed):
    L, loss, batches, grads = lr.run_ref(lr.learner_array(sd), rows, rows.shape[0], in_dim, out_dim, batch, updates,
                                         seed=seed, grads=True)
    run = []
    L1 = lr.learner_array(sd)
    for u in range(updates):  # the parameters after each update: one update at a time
        L1, _, _, _ = lr.run_ref(L1, rows, rows.shape[0], in_dim, out_dim, batch, 1, first_update=u, first_draw=u,
                                 seed=seed)
        run.append((float(loss[u]), {k: v.astype(np.float64) for k, v in lr.split(grads[u], in_dim, out_dim).items()},
                    {k: v.astype(np.float64) for k, v in lr.split(L1[0], in_dim, out_dim).items()}))
    assert np.array_equal(lr.bits(L1), lr.bits(L))
    return run, batches


# the seed of the minibatch draws: with it every sampled row's two best eval(s') values differ by more
# than 1e-4 relative in fp64 (asserted below), so no rounding can flip the Double-DQN argmax
SEED = 3
UPDATES, BATCH = 6, 128


@pytest.mark.parametrize("net,mem", [("l1", "L0_memory"), ("l3", "RR_memory")])
def test_restatement_is_as_close_to_fp64_as_torch_fp32(net, mem):
    """Our fixed-order fp32 against torch's fp32, both measured against torch's fp64 on the same
    minibatches, six updates from a trained net. The bars (ours <= max(4 x torch-fp32's own error in
    this run, 1e-6) for every tensor's gradient and parameters; loss <= max(4 x torch's, B 2^-24)) hold
    because both are fp32 sums of the same <= 200 products in different orders."""
    import torch

    sd, rows = lr.trained_net(net), lr.memory(mem)
    ours, batches = _ours(sd, rows, 10, 5, BATCH, UPDATES, SEED)
    t64 = _torch_learn(sd, batches, 10, torch.float64, UPDATES)
    t32 = _torch_learn(sd, batches, 10, torch.float32, UPDATES)
    gap = min(r[3] for r in t64)
    print(f"\n[learn {net}/{mem}] smallest top-two gap of eval(s') in fp64: {gap:.3e}")
    assert gap > 1e-4
    og, op, ol = _errors(ours, t64, UPDATES)
    tg, tp, tl = _errors(t32, t64, UPDATES)
    for k in lr.KEYS:
        print(f"[learn {net}/{mem}] {k:11s} grad err ours {og[k]:.3e} torch32 {tg[k]:.3e}   "
              f"param err / lr ours {op[k]:.3e} torch32 {tp[k]:.3e}")
    print(f"[learn {net}/{mem}] loss rel err ours {ol:.3e} torch32 {tl:.3e}")
    for k in lr.KEYS:
        assert og[k] <= max(4 * tg[k], 1e-6), (k, og[k], tg[k])
        assert op[k] <= max(4 * tp[k], 1e-6), (k, op[k], tp[k])
    assert ol <= max(4 * tl, BATCH * 2.0 ** -24), (ol, tl)


def test_first_update_from_the_reference_initialisation():
    """From the reference's fresh weights (uniform_(0, 1), main.py:35-39) only update 1's loss and
    gradients are compared, with the same bars: Adam's first step is +-lr by the gradient's sign, so
    parameters from this start are not comparable."""
    import torch

    torch.manual_seed(0)
    sd = {}
    for name, (o, i) in (("fc1", (200, 10)), ("fc2", (100, 200)), ("out", (5, 100))):
        lin = torch.nn.Linear(i, o)
        lin.weight.data.uniform_(0, 1)
        sd[f"{name}.weight"], sd[f"{name}.bias"] = lin.weight.detach().numpy().copy(), lin.bias.detach().numpy().copy()
    rows = lr.memory("L0_memory")
    _, loss, batches, grads = lr.run_ref(lr.learner_array(sd), rows, rows.shape[0], 10, 5, BATCH, 1, seed=SEED,
                                         grads=True)
    ours = [(float(loss[0]), {k: v.astype(np.float64) for k, v in lr.split(grads[0], 10, 5).items()}, None)]
    t64 = _torch_learn(sd, batches, 10, torch.float64, 1)
    t32 = _torch_learn(sd, batches, 10, torch.float32, 1)
    assert t64[0][3] > 1e-4
    og, _, ol = _errors(ours, t64, 1)
    tg, _, tl = _errors([(t32[0][0], t32[0][1], None)], t64, 1)
    for k in lr.KEYS:
        print(f"\n[learn uniform init] {k:11s} grad err ours {og[k]:.3e} torch32 {tg[k]:.3e}", end="")
        assert og[k] <= max(4 * tg[k], 1e-6), (k, og[k], tg[k])
    print(f"\n[learn uniform init] loss rel err ours {ol:.3e} torch32 {tl:.3e}")
    assert ol <= max(4 * tl, BATCH * 2.0 ** -24), (ol, tl)


# ------------------------------------------------------------------ 3. what the entry points refuse
def test_learn_argument_errors_without_gpu():
    from merging_gym import _native

    lib = _native.lib
    assert _native.ABI_VERSION == 21 and lib.mg_abi_version() == 21
    assert ctypes.sizeof(_native.DqnHyper) == 5 * 8 + 2 * 4
    # four blocks of P fp32: 10 -> 5 has main.py's 22,805 parameters
    assert lib.mg_dqn_learner_bytes(10, 5) == 16 * 22805
    assert lib.mg_dqn_learner_bytes(11, 5) == 16 * 23005 and lib.mg_dqn_learner_bytes(10, 3) == 16 * 22603
    assert lib.mg_dqn_learner_bytes(14, 5) == 0 and lib.mg_dqn_learner_bytes(10, 9) == 0
    assert lib.mg_dqn_learner_bytes(0, 5) == 0 and lib.mg_dqn_learner_bytes(10, 0) == 0

    def scratch(B, i, o):  # rows, h1 and h2 of three passes, d, dq, dh2, dh1, the gradient: each rounded up to 4 floats
        r4 = lambda n: (n + 3) // 4 * 4  # noqa: E731
        return 4 * (r4(B * (2 * i + 2)) + r4(3 * B * 200) + r4(3 * B * 100) + r4(B) + r4(8 * B) + r4(100 * B) +
                    r4(200 * B) + r4(lr.num_params(i, o)))
    assert lib.mg_dqn_learn_scratch_bytes(128, 10, 5) == scratch(128, 10, 5) == 721504
    assert lib.mg_dqn_learn_scratch_bytes(1, 13, 8) == scratch(1, 13, 8)
    assert lib.mg_dqn_learn_scratch_bytes(1024, 11, 5) == scratch(1024, 11, 5)
    assert lib.mg_dqn_learn_scratch_bytes(1025, 10, 5) == 0 and lib.mg_dqn_learn_scratch_bytes(0, 10, 5) == 0
    assert lib.mg_dqn_learn_scratch_bytes(128, 14, 5) == 0 and lib.mg_dqn_learn_scratch_bytes(128, 10, 9) == 0

    fake = ctypes.c_void_p(1 << 20)  # never dereferenced: validation fails first
    odd16, odd8, odd4 = (ctypes.c_void_p((1 << 20) + k) for k in (8, 4, 2))
    big = 1 << 24
    good = dict(learner=fake, rows=fake, counter=fake, capacity=2000, row_floats=22, in_dim=10, out_dim=5, batch=128,
                num_updates=1, filled_only=0, hyper=lr.hyper_struct(100), loss_out=None, rows_out=None,
                packed_out=None, scratch=fake, scratch_bytes=big)

    def call(host=False, **kw):
        a = dict(good, **kw)
        h = a["hyper"]
        args = [a["learner"], a["rows"], a["counter"], a["capacity"], a["row_floats"], a["in_dim"], a["out_dim"],
                a["batch"], a["num_updates"], 0, 0, 0, a["filled_only"], ctypes.byref(h) if h is not None else None,
                a["loss_out"], a["rows_out"]]
        if host:
            return lib.mg_host_dqn_learn(*args, a["scratch"], a["scratch_bytes"])
        return lib.mg_dqn_learn(*args, a["packed_out"], a["scratch"], a["scratch_bytes"], None)

    def refused(msg, **kw):
        for host in (False, True):
            assert call(host=host, **kw) != 0
            err = lib.mg_last_error()
            assert msg in err and (b"mg_host_dqn_learn" if host else b"mg_dqn_learn") in err, err

    for name in ("learner", "rows", "hyper", "scratch"):
        refused(b"NULL", **{name: None})
    refused(b"NULL", counter=None, filled_only=1)
    for bad in (dict(in_dim=0, row_floats=2), dict(in_dim=14, row_floats=30), dict(out_dim=0), dict(out_dim=9)):
        refused(b"1 <= in_dim <= 13, 1 <= out_dim <= 8", **bad)
    refused(b"row_floats must be 2 * in_dim + 2", row_floats=24)
    refused(b"row_floats must be 2 * in_dim + 2", in_dim=11)
    refused(b"1 <= batch <= 1024", batch=0)
    refused(b"1 <= batch <= 1024", batch=1025)
    refused(b"capacity", capacity=0)
    refused(b"capacity", capacity=(1 << 32) + 1)
    refused(b"num_updates", num_updates=-1)
    refused(b"target_period", hyper=lr.hyper_struct(0))
    refused(b"beta1", hyper=lr.hyper_struct(100, beta1=1.0))
    refused(b"beta2", hyper=lr.hyper_struct(100, beta2=-0.1))
    refused(b"aligned", learner=odd16)
    refused(b"aligned", scratch=odd16)
    refused(b"aligned", rows=odd8)
    refused(b"aligned", counter=odd8)
    refused(b"aligned", loss_out=odd4)
    refused(b"aligned", rows_out=odd4)
    assert call(packed_out=odd16) != 0 and b"aligned" in lib.mg_last_error()
    refused(b"scratch smaller than mg_dqn_learn_scratch_bytes", scratch_bytes=scratch(128, 10, 5) - 4)
    # nothing to do is a success before anything is read
    assert call(num_updates=0) == 0 and call(host=True, num_updates=0) == 0

    def init(**kw):
        a = dict(learner=fake, t=[fake] * 6, in_dim=10, out_dim=5)
        a.update(kw)
        return lib.mg_dqn_learner_init(a["learner"], *a["t"], a["in_dim"], a["out_dim"], None)
    assert init(learner=None) != 0 and b"mg_dqn_learner_init: NULL" in lib.mg_last_error()
    for k in range(6):
        assert init(t=[None if i == k else fake for i in range(6)]) != 0 and b"NULL" in lib.mg_last_error()
    assert init(in_dim=14) != 0 and b"in_dim" in lib.mg_last_error()
    assert init(out_dim=9) != 0 and b"out_dim" in lib.mg_last_error()
    assert init(learner=odd16) != 0 and b"aligned" in lib.mg_last_error()
    assert init(t=[odd4] + [fake] * 5) != 0 and b"aligned" in lib.mg_last_error()
