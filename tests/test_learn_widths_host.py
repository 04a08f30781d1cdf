"""DQN.learn at every accepted width without a GPU (tests/width_cases.py): the host twins (mg_host_dqn_learn,
mg_host_dqn_learn_many: the per-element functions the kernels run) against the plain-C restatement bit for bit
on rows whose action column the reference's gather would raise on; the documented clamp of that column as a
property of the library alone; and the restatement against torch's own learn() in fp32 and fp64 with
tests/test_learn_host.py's bars."""

import ctypes

import numpy as np
import pytest

import learn_many_ref as mr
import learn_ref as lr
import width_cases as wc
from test_learn_host import _errors, _ours, _torch_learn


# ------------------------------------------------------------------ 1. host twin == restatement
@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch", wc.LEARN_CASES)
def test_host_learn_equals_restatement_at_every_width(in_dim, out_dim, batch, filled_only):
    """wc.SEQUENCE on a half-filled 64-row ring whose rows 0..3 hold the actions -1, out + 3, NaN and out - 0.5:
    eval, target, m, v, every loss and every sampled row agree bit for bit."""
    _, ring, counter, L0, (ref, ref_loss, ref_rows, _) = wc.reference(in_dim, out_dim, batch, filled_only)
    got, got_loss, got_rows = lr.run_host(L0, ring, counter, in_dim, out_dim, batch, filled_only=filled_only,
                                          **wc.SEQUENCE)
    assert np.array_equal(lr.bits(got_rows), lr.bits(ref_rows))
    assert np.array_equal(lr.bits(got_loss), lr.bits(ref_loss)), (got_loss, ref_loss)
    for blk, name in enumerate(("eval", "target", "m", "v")):
        bad = lr.bits(got[blk]) != lr.bits(ref[blk])
        assert not bad.any(), (name, int(bad.sum()), float(np.abs(got[blk] - ref[blk]).max()))
    # the copy happened, the parameters moved, and a NaN action reached nothing but its own column
    assert not np.array_equal(got[1], L0[1]) and not np.array_equal(got[0], L0[0])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(got_loss))
    unfilled = np.abs(np.nan_to_num(got_rows, nan=1.0)).sum(axis=2) == 0
    if not filled_only:
        assert unfilled.any()
    else:
        assert not unfilled.any()


# ------------------------------------------------------------------ 2. the clamp, from the library alone
def _host_with_scratch(L0, rows, in_dim, out_dim, batch, updates):
    """mg_host_dqn_learn on all of `rows` (filled_only off): (learner, loss, sampled rows, the scratch after the
    last update)."""
    from merging_gym import _native

    L = np.array(L0, dtype=np.float32, copy=True)
    rows = np.ascontiguousarray(rows, dtype=np.float32)
    cnt = np.array([rows.shape[0]], dtype=np.uint64)
    loss = np.zeros(updates, dtype=np.float32)
    got = np.zeros((updates, batch, rows.shape[1]), dtype=np.float32)
    nbytes = _native.lib.mg_dqn_learn_scratch_bytes(batch, in_dim, out_dim)
    scratch = np.zeros(nbytes // 4, dtype=np.float32)
    h = lr.hyper_struct(2)
    rc = _native.lib.mg_host_dqn_learn(L.ctypes.data, rows.ctypes.data, cnt.ctypes.data, rows.shape[0], rows.shape[1],
                                       in_dim, out_dim, batch, updates, 1, 7, 5, 0, ctypes.byref(h), loss.ctypes.data,
                                       got.ctypes.data, scratch.ctypes.data, nbytes)
    _native.check(rc, "mg_host_dqn_learn")
    return L, loss, got, scratch


@pytest.mark.parametrize("in_dim,out_dim", [(10, 5), (13, 8), (1, 1)])
def test_odd_actions_learn_as_their_documented_clamp(in_dim, out_dim):
    """A ring of the four odd rows alone (-1, out + 3, NaN, out - 0.5), so every draw hits one: the library gives
    the same learner, losses and -- in its scratch: activations, d, dq, both input gradients, the parameter
    gradient -- everything else, bit for bit, as on the rows with 0, out - 1, 0 and out - 1 written out
    (width_cases.clamped, from the header's words). The sampled rows differ in the action column alone."""
    B, U = 9, 3
    odd = wc.width_rows(in_dim, out_dim, 4, True)
    clean = wc.clamped(odd, in_dim, out_dim)
    assert clean[:, in_dim].tolist() == [0.0, out_dim - 1.0, 0.0, out_dim - 1.0]
    L0 = wc.start_learner(in_dim, out_dim)
    a = _host_with_scratch(L0, odd, in_dim, out_dim, B, U)
    b = _host_with_scratch(L0, clean, in_dim, out_dim, B, U)
    assert np.array_equal(lr.bits(a[0]), lr.bits(b[0])) and np.array_equal(lr.bits(a[1]), lr.bits(b[1]))
    assert np.all(np.isfinite(a[0])) and np.all(np.isfinite(a[1])) and not np.array_equal(a[0][0], L0[0])
    rf = 2 * in_dim + 2
    other = np.arange(rf) != in_dim
    assert np.array_equal(lr.bits(a[2][..., other]), lr.bits(b[2][..., other]))
    assert np.array_equal(lr.bits(wc.clamped(a[2].reshape(-1, rf), in_dim, out_dim)), lr.bits(b[2].reshape(-1, rf)))
    drawn = {lr.bits(np.float32(v)).item() for v in a[2][..., in_dim].ravel()}
    assert drawn == {lr.bits(np.float32(v)).item() for v in odd[:, in_dim]}  # all four odd values were sampled
    # the scratch: the minibatch rows first (include/merging_hip.h's sections, each rounded up to 4 floats),
    # then everything the update computed, the gradient [P] last
    nrows = (B * rf + 3) // 4 * 4
    assert np.array_equal(lr.bits(a[3][nrows:]), lr.bits(b[3][nrows:]))
    P = lr.num_params(in_dim, out_dim)
    g = a[3][-((P + 3) // 4 * 4):][:P]
    assert np.all(np.isfinite(a[3][nrows:])) and np.count_nonzero(g) > 100
    rows_a, rows_b = a[3][:B * rf].reshape(B, rf), b[3][:B * rf].reshape(B, rf)
    assert np.array_equal(lr.bits(rows_a), lr.bits(a[2][-1])) and np.array_equal(lr.bits(rows_b), lr.bits(b[2][-1]))


# ------------------------------------------------------------------ 3. the population's host twin
@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("in_dim,out_dim,batch", [(13, 8, 9), (1, 1, 1)])
def test_host_population_equals_restatement_at_the_corner_widths(in_dim, out_dim, batch, filled_only):
    """Three members, each on its own roll of the odd-action rows with its own counter, seed, hyperparameters,
    first_update and first_draw (tests/learn_many_ref.py), four updates: every member equals the restatement's
    run of it alone."""
    M = 3
    _, rings, counters, kws, L0 = wc.members_setup(in_dim, out_dim, M)
    ref_end, ref_loss, ref_rows = wc.members_reference(in_dim, out_dim, batch, M, filled_only, mr.UPDATES)
    masks = mr.sync_masks(kws, mr.UPDATES)
    assert any(0 < len(s) < M for s in masks)
    got, loss, rows, (arr, _) = mr.run_host_many(L0, rings, counters, kws, in_dim, out_dim, batch, mr.UPDATES,
                                                 filled_only)
    mr.assert_members_equal(got, loss, rows, ref_end, ref_loss, ref_rows)
    for m, kw in enumerate(kws):
        assert (arr[m].first_update, arr[m].first_draw) == (kw["first_update"] + mr.UPDATES, kw["first_draw"] + mr.UPDATES)
        assert not np.array_equal(got[m, 0], L0[m, 0]) and not np.array_equal(got[m, 1], L0[m, 1])
    assert np.all(np.isfinite(got)) and np.all(np.isfinite(loss))
    assert len({rows[:, m].tobytes() for m in range(M)}) == M  # own rings, own draws


# ------------------------------------------------------------------ 4. restatement vs torch fp32 / fp64
UPDATES = 4
MAX_SEED = 8


@pytest.mark.parametrize("in_dim,out_dim,batch", [(13, 8, 33), (1, 2, 9), (12, 7, 33)])
def test_restatement_is_as_close_to_fp64_as_torch_fp32_at_other_widths(in_dim, out_dim, batch):
    """tests/test_learn_host.py's comparison and bars, unchanged (ours <= max(4 x torch-fp32's own error, 1e-6)
    per tensor for gradients and parameters; loss <= max(4 x torch's, B 2^-24)), on four updates from a seeded
    net over a full ring of clean rows (torch's gather raises on the odd ones). The minibatch seed is the first
    from 0 with which torch's fp64 run keeps every sampled row's two best eval(s') values more than 1e-4 apart
    (relative), so no rounding can flip the Double-DQN argmax. out_dim = 1 has no second-best value: that width
    is covered bit for bit by the restatement above.
    Measured (every error is in DESIGN.md section 5): 13 -> 8 B 33: seed 0, gap 7.1e-4; 1 -> 2 B 9: seed 0,
    gap 2.7e-2; 12 -> 7 B 33: seed 0, gap 1.8e-2, ours up to 3.2 x torch-fp32's error against the bar of 4."""
    import torch

    sd, rows = wc.width_net(in_dim, out_dim), wc.width_rows(in_dim, out_dim, wc.CAPACITY, False)
    for seed in range(MAX_SEED):
        ours, batches = _ours(sd, rows, in_dim, out_dim, batch, UPDATES, seed)
        t64 = _torch_learn(sd, batches, in_dim, torch.float64, UPDATES)
        gap = min(r[3] for r in t64)
        if gap > 1e-4:
            break
    tag = f"learn {in_dim}->{out_dim} B={batch}"
    print(f"\n[{tag}] seed {seed}, smallest top-two gap of eval(s') in fp64: {gap:.3e}")
    assert gap > 1e-4
    t32 = _torch_learn(sd, batches, in_dim, torch.float32, UPDATES)
    og, op, ol = _errors(ours, t64, UPDATES)
    tg, tp, tl = _errors(t32, t64, UPDATES)
    for k in lr.KEYS:
        print(f"[{tag}] {k:11s} grad err ours {og[k]:.3e} torch32 {tg[k]:.3e}   "
              f"param err / lr ours {op[k]:.3e} torch32 {tp[k]:.3e}")
    print(f"[{tag}] loss rel err ours {ol:.3e} torch32 {tl:.3e}")
    for k in lr.KEYS:
        assert og[k] <= max(4 * tg[k], 1e-6), (k, og[k], tg[k])
        assert op[k] <= max(4 * tp[k], 1e-6), (k, op[k], tp[k])
    assert ol <= max(4 * tl, batch * 2.0 ** -24), (ol, tl)
