"""Rainbow's compute_td_loss on the host (CPU): mg_host_rainbow_learn -- the functions the kernels compile --
against the plain-C restatement bit for bit, the projection against the reference's recorded proj_dist bit
for bit, one update against the reference's fp64 run within the bars of tests/test_learn_host.py, the
library's log against logf over every fp32 in [0.01, 0.99], and the noise against RainbowNet.reset_noise."""
import ctypes

import numpy as np
import pytest

import rainbow_learn_ref as R
from learn_ref import bits

FAMS = ("default", "soft")


@pytest.fixture(scope="module")
def learner0():
    return {fam: R.learner_numpy(R.golden_state(1, fam)) for fam in FAMS}


@pytest.mark.parametrize("capacity,counter", R.RINGS, ids=["partly-filled", "wrapped"])
@pytest.mark.parametrize("batch", R.BATCHES)
def test_host_twin_equals_the_restatement(learner0, batch, capacity, counter):
    """learn(2), sync_target(), learn(1): current, target, m, v, both noise blocks, every loss, sampled row,
    proj and gradient. The "default" family at B = 1 is kept as the saturated-softmax case: its first update's
    gradient is exactly zero and no parameter moves (host twin, wrapped ring, measured), and at B = 33 the
    largest gradient entry is 2e-4. The edge batches with real gradients are the test below."""
    fam = "soft" if batch in (32, 128) else "default"
    ring, c = R.ring_case(capacity, counter)
    want = R.sequence(R.run_ref, learner0[fam], ring, c, batch)
    got = R.sequence(R.run_host, learner0[fam], ring, c, batch)
    R.assert_same(got, want)
    assert np.isfinite(want[1][0]).all() and np.abs(want[1][3]).max() > 0  # a real update: finite loss, gradients


@pytest.mark.parametrize("capacity,counter", R.RINGS, ids=["partly-filled", "wrapped"])
@pytest.mark.parametrize("batch", R.EDGE_BATCHES)
def test_host_twin_equals_the_restatement_at_batch_edges(batch, capacity, counter):
    """The same sequence from the "soft" state at B = 1, 33, 257 (the first batch past one block of items) and
    1024 (the largest). Every update's gradient has non-zero entries and moves the current parameters
    (R.edge_reference checks the latter update by update), so none of these cases passes on zeros."""
    L0, want = R.edge_reference(batch, capacity, counter)
    got = R.sequence(R.run_host, L0, *R.ring_case(capacity, counter), batch, seed=R.EDGE_SEED)
    R.assert_same(got, want)
    for grads in (got[1][3][0], got[1][3][1], got[1][7][0]):
        assert np.count_nonzero(grads) > 0 and np.isfinite(grads).all()
    assert np.isfinite(got[1][0]).all() and np.isfinite(got[1][4]).all()
    assert (bits(got[0][:R.NP]) != bits(L0[:R.NP])).any()


def test_sampled_rows_are_the_filled_rows_only():
    ring, c = R.ring_case(64, 40)
    rows = R.run_host(R.learner_numpy(R.golden_state(1, "soft")), ring, c, 128, 1, seed=5, noise_f=R.noise(1))[2][0]
    stored = {r.tobytes() for r in ring[:40]}
    assert all(r.tobytes() in stored for r in rows) and len({r.tobytes() for r in rows}) > 20


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("u", (0, 1))
def test_projection_equals_the_reference(fam, u):
    """mg_host_rainbow_project on the reference's gathered next_dist gives its proj_dist bit for bit."""
    from merging_gym import _native

    st = R.fixture(fam, u)[0]
    nd = np.ascontiguousarray(st["next_dist"], np.float32)
    rows = st["rows"]
    r, d = np.ascontiguousarray(rows[:, 11]), np.ascontiguousarray(rows[:, 22])
    z = R.learner_numpy(R.golden_state(1, fam))[-52:-1].copy()
    proj = np.full_like(nd, np.nan)
    _native.check(_native.lib.mg_host_rainbow_project(nd.ctypes.data, r.ctypes.data, d.ctypes.data, z.ctypes.data, 0.99,
                                                      proj.ctypes.data, len(nd)), "mg_host_rainbow_project")
    assert np.array_equal(bits(proj), bits(st["proj_dist"]))
    b = (np.clip(r[:, None] + (1 - d[:, None]) * np.float32(0.99) * z[None], -10, 10) + 10) / np.float32(0.4)
    assert (b == np.floor(b)).mean() > 0.05  # integral b (dropped mass) is exercised
    ref = np.zeros(51, np.float32)  # and the restatement agrees
    R.build_ref().rainbow_project_ref(nd[3].ctypes.data, r[3], d[3], np.float32(0.99), z.ctypes.data, ref.ctypes.data)
    assert np.array_equal(bits(ref), bits(proj[3]))


@pytest.mark.parametrize("fam", FAMS)
@pytest.mark.parametrize("u", (0, 1))
def test_one_update_against_the_reference(fam, u):
    """From the recorded before-state, on the recorded minibatch: per tensor max|g - g64| /
    max|g64| <= max(4 x the reference's own fp32 error, 1e-6); the loss within max(4 x the reference's, B 2^-24).
    Both sides are fp32 evaluations of the same sums in different orders."""
    from merging_gym import rainbow_learn

    st, gr = R.fixture(fam, u)
    rows = np.ascontiguousarray(st["rows"], np.float32)
    ring, counter, seed = R.ring_of_chosen_rows(rows)
    L0 = R.fixture_learner(fam, u)
    L, loss, got_rows, proj, grads = R.run_host(L0, ring, counter, len(rows), 1, first_update=u, seed=seed,
                                                noise_f=R.noise(1))
    assert np.array_equal(bits(got_rows[0]), bits(rows))
    # the target's forward sums in another order than torch's, so proj is close, not equal (the projection
    # itself is pinned bit for bit by test_projection_equals_the_reference)
    print(f"{fam} u{u} proj: max |ours - the reference's| {np.abs(proj[0] - st['proj_dist']).max():.3g}")
    loss64 = float(st["loss64"])
    ref_err = abs(float(st["loss32"]) - loss64) / abs(loss64)
    our_err = abs(float(loss[0]) - loss64) / abs(loss64)
    print(f"{fam} u{u} loss: ours {our_err:.3g}, the reference's {ref_err:.3g}")
    worst = []
    at = 0
    for k in rainbow_learn.PARAM_KEYS:
        g64 = gr[f"g64/{k}"]
        g = grads[0, at:at + g64.size].reshape(g64.shape).astype(np.float64)
        at += g64.size
        scale = np.abs(g64).max()
        ours, theirs = np.abs(g - g64).max() / scale, np.abs(gr[f"d32/{k}"]).max() / scale
        print(f"{fam} u{u} {k}: ours {ours:.3g}, the reference's {theirs:.3g}")
        if ours > max(4 * theirs, 1e-6):
            worst.append((k, ours, theirs))
    assert at == R.NP
    assert not worst, worst
    assert our_err <= max(4 * ref_err, len(rows) * 2.0 ** -24)


def test_log_against_logf_over_the_clamp_range():
    """Every fp32 in [0.01, 0.99]: the library's log is within 1 ulp of logf -- rb_exp's recorded distance from
    expf -- and equals the restatement's bit for bit."""
    from merging_gym import _native

    fn = ctypes.cast(_native.lib.mg_host_rainbow_log, ctypes.c_void_p)
    count, off, off_ref = ctypes.c_int64(), ctypes.c_int64(), ctypes.c_int64()
    worst = R.build_ref().rainbow_log_scan(fn, np.float32(0.01), np.float32(0.99), ctypes.byref(count),
                                           ctypes.byref(off), ctypes.byref(off_ref))
    print(f"log: {count.value} values, {off.value} differ from logf, the largest distance {worst} ulp")
    assert count.value > 5.4e7 and off_ref.value == 0
    assert 0 <= worst <= 1


def test_noise_after_a_learn_is_reset_noise_twice(learner0):
    """After learn(1) the current model's buffers are a twin generator's first RainbowNet.reset_noise draw, the
    target's the second (ranbowdqn.py:606-607)."""
    import torch

    from merging_gym import rainbow_learn
    from merging_gym.rainbow import RainbowNet

    ring, c = R.ring_case(64, 200)
    g = torch.Generator().manual_seed(123)
    nf = rainbow_learn.noise_factors(1, g).numpy()
    L = R.run_host(learner0["soft"], ring, c, 32, 1, noise_f=nf)[0]
    twin = RainbowNet.from_state_dict(R.golden_state(1, "soft"))
    g2 = torch.Generator().manual_seed(123)
    buf = torch.from_numpy(L)
    for model in (0, 1):
        twin.reset_noise(g2)
        sd = rainbow_learn.model_state_dict(buf, model)
        for k in rainbow_learn.EPS_KEYS:
            assert torch.equal(sd[k], twin.state[k]), (model, k)
    assert not torch.equal(rainbow_learn.model_state_dict(buf, 0)["noisy_value1.weight_epsilon"],
                           rainbow_learn.model_state_dict(buf, 1)["noisy_value1.weight_epsilon"])


def test_state_dicts_have_the_references_keys(learner0):
    from merging_gym import rainbow_learn

    import torch

    sd = R.golden_state(1, "soft")
    back = rainbow_learn.model_state_dict(torch.from_numpy(learner0["soft"]), 0)
    assert list(back) == list(sd)
    assert all(torch.equal(back[k], sd[k]) for k in sd)
    assert rainbow_learn.NUM_PARAMS == R.NP and rainbow_learn.NUM_EPS == R.NE and rainbow_learn.NUM_FACTORS == R.NF
