"""The prioritized Rainbow learner on the host (CPU): mg_host_rainbow_learn_prioritized -- the functions the
kernels compile -- against mg_host_rainbow_learn where the two must agree bit for bit, and against a restatement
of the weighted order in Python that takes each row's unweighted loss and gradient from the uniform learner at
batch 1."""
import numpy as np
import pytest

import per_ref as P
import rainbow_learn_ref as R
from learn_ref import bits

SEED, BETA, EPS = 3, 0.5, 1e-5


def test_unit_weights_on_one_repeated_row_equal_the_uniform_learner():
    """A fresh tree gives every weight exactly 1; with one row stored everywhere every index reads the row the
    uniform draw reads. Then w_b * (1 / B) is 1 / B and the weighted loss sum is the plain one."""
    B, size = 32, 13
    L0 = R.learner_numpy(R.golden_state(1, "soft"))
    h = P.HostPer(size, 0.6)
    h.push_many(size + 5, n=4)
    h.rows[:] = R.replay_rows(size)[4]
    nf = R.noise(1)
    want = R.run_host(L0, h.rows, int(h.counter[0]), B, 1, seed=SEED, noise_f=nf)
    got = P.run_host_prioritized(L0, h, B, 1, BETA, EPS, seed=SEED, noise_f=nf)
    assert (got[6] == 1.0).all() and len(set(got[5].ravel().tolist())) > 4
    R.assert_same((got[0], list(got[1:5])), (want[0], list(want[1:])))


def _case(size=13, alpha=0.6):
    h = P.HostPer(size, alpha)
    h.push_many(size + size // 2 + 1, n=5)
    h.rows[:] = R.replay_rows(size)
    for r in range(6):
        idx, _ = h.sample(P.BATCH, P.BETA, 1, r)
        h.update(idx, np.exp(np.random.default_rng(r).uniform(np.log(1e-3), np.log(8.0), P.BATCH)).astype(np.float32))
    return h


def test_three_updates_in_one_call_equal_three_calls_of_one():
    """U = 3, B = 32 on the wrapped ring of 13 (a 16-leaf tree), alpha 0.6, beta 0.5, from the device test's
    starting point: call u of the three runs with first_update = first_draw = u and noise slice u. Bit for bit:
    the learner buffer, every tree node and max_priority, the rows and the counter, and all six outputs
    concatenated."""
    B, U = 32, 3
    L0 = R.learner_numpy(R.golden_state(1, "soft"))
    nf = R.noise(U)
    start = P.learn_case(13, 0.6)
    single, whole = start.clone(), start.clone()
    L, seq = L0, []
    for u in range(U):
        seq.append(P.run_host_prioritized(L, single, B, 1, BETA, EPS, first_update=u, seed=SEED, first_draw=u,
                                          noise_f=nf[u:u + 1]))
        L = seq[-1][0]
    all3 = P.run_host_prioritized(L0, whole, B, U, BETA, EPS, seed=SEED, noise_f=nf)
    assert np.array_equal(bits(all3[0]), bits(L))
    assert np.array_equal(P.f64bits(whole.tree), P.f64bits(single.tree))
    assert np.array_equal(bits(whole.rows), bits(single.rows)) and whole.counter[0] == single.counter[0]
    for k in range(1, 7):
        assert np.array_equal(all3[k].view(np.uint8), np.concatenate([s[k] for s in seq]).view(np.uint8)), k
    assert not np.array_equal(P.f64bits(whole.tree), P.f64bits(start.tree))  # the priorities moved
    assert len(np.unique(all3[5])) > 4 and len(np.unique(all3[6])) > 1  # a real sample with real weights


def _weighted_order(B):
    """Three updates, one call each. Per update: idx and w are the sample of the tree as it stands; loss_out is
    the chain over fp32(w_b * loss_b) times fp32(1 / B); the priorities written back are fp32(loss_b + fp32(eps))
    (rows whose loss is not positive are left out, as update_priorities' assert would refuse them); the gradient
    is sum_b (w_b / B) g_b. loss_b and g_b come from the uniform learner run on row idx[b] alone (batch 1, where
    1 / B is 1), from the same learner state. The gradient's bound: every element is a chain of at most
    B + 255 + 64 fp32 terms (the batch, the widest layer, the layers above), each rounded to 2^-24 relative, so
    |g - g64| <= (B + 319) 2^-24 max|g64| over the whole gradient, g64 the fp64 combination. Then the three updates in one
    call give the same bits."""
    U = 3
    L0 = R.learner_numpy(R.golden_state(1, "soft"))
    nf = R.noise(U)
    h = _case()
    mine, whole = h.clone(), h.clone()
    L, inv_b = L0, np.float32(1.0 / B)
    seq, real = [], []
    for u in range(U):
        idx, w = mine.sample(B, BETA, SEED, u)
        lossb, gb = np.zeros(B, np.float32), []
        for b in range(B):
            one = R.run_host(L, mine.rows[idx[b]][None, :], 1, 1, 1, first_update=u, seed=SEED, first_draw=u,
                             noise_f=nf[u:u + 1])
            lossb[b] = one[1][0]
            gb.append(one[4][0].astype(np.float64))
        acc = np.float32(0.0)
        for b in range(B):
            acc = np.float32(acc + np.float32(w[b] * lossb[b]))
        mine.update(idx, lossb + np.float32(EPS))
        out = P.run_host_prioritized(L, h, B, 1, BETA, EPS, first_update=u, seed=SEED, first_draw=u, noise_f=nf[u:u + 1])
        L = out[0]
        seq.append(out)
        assert np.array_equal(out[5][0], idx) and np.array_equal(bits(out[6][0]), bits(w)), u
        assert bits(out[1])[0] == bits(np.float32(acc * inv_b)), u
        assert np.array_equal(bits(out[2][0]), bits(mine.rows[idx])), u
        assert np.array_equal(P.f64bits(h.tree), P.f64bits(mine.tree)), u
        g64 = sum(float(w[b]) / B * gb[b] for b in range(B))
        diff, scale = np.abs(out[4][0] - g64).max(), np.abs(g64).max()
        err = diff / scale if scale > 0 else (0.0 if diff == 0 else np.inf)  # a zero gradient has to be exactly zero
        print(f"update {u}: weights {w.min():.3g}..{w.max():.3g}, gradient error {err:.3g}")
        assert err <= (B + 319) * 2.0 ** -24, u
        real.append((scale > 0, bool((lossb + np.float32(EPS) > 0).any())))
        assert (w > 0).all() and (w <= 1).all(), u
        # a batch of several rows has several weights, a positive priority and a gradient in every update; one row
        # alone may be a row whose projected mass is dropped (zero loss, zero gradient) or whose loss is negative
        # (its priority is refused and the tree stays), so there it is asked of the three updates together
        assert B == 1 or (len(np.unique(w)) > 1 and all(real[-1])), u
    assert any(r[0] for r in real) and any(r[1] for r in real), real
    all3 = P.run_host_prioritized(L0, whole, B, U, BETA, EPS, seed=SEED, noise_f=nf)
    assert np.array_equal(bits(all3[0]), bits(L)) and np.array_equal(P.f64bits(whole.tree), P.f64bits(h.tree))
    for k in range(1, 7):
        assert np.array_equal(all3[k].view(np.uint8), np.concatenate([s[k] for s in seq]).view(np.uint8)), k


def test_weighted_order_restated_in_python():
    _weighted_order(8)


@pytest.mark.parametrize("B", (1, 33))
def test_weighted_order_restated_in_python_at_batch_edges(B):
    """_weighted_order at one row (the chain over the batch is one term, 1 / B is 1) and at a batch that is no
    multiple of a wave; its gradient bound (B + 319) 2^-24 holds as derived there."""
    _weighted_order(B)
