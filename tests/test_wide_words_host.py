"""The learners' host twins at 64-bit seeds, draws and update counts (no GPU): every other host test keys the
minibatch draws with a seed and a draw below 2^32, so the high key word k1 and the high counter word c3 of
learn_slot's Philox call (csrc/mg_learn_core.h, host branch) and of the two plain-C restatements
(tests/native/dqn_learn_ref.c, rainbow_learn_ref.c) are zero there, and Adam's step count stays below 2^32.
Every comparison is bit for bit."""

import numpy as np
import pytest

import learn_ref as lr
import merge_oracle as mo
import rainbow_learn_ref as R
import wide_words as W

BATCH, UPDATES = 33, 2


def _join(lo, hi):
    return int(lo) | (int(hi) << 32)


# ------------------------------------------------------------------ 1. the three Philox restatements and the KATs
def _slots_dqn(run, seed, draw):
    sd = lr.seeded_net(10, 5, 5)
    return run(lr.learner_array(sd), W.probe_ring(22), W.PROBE_CAP, 10, 5, BATCH, 1, seed=seed, first_draw=draw)[2][0, :, 0]


def _slots_rainbow(run, seed, draw):
    L = np.zeros(4 * R.NP + 2 * R.NE + 52, np.float32)  # only the sampled rows are read back
    return run(L, W.probe_ring(R.ROW), W.PROBE_CAP, BATCH, 1, seed=seed, first_draw=draw,
               noise_f=np.zeros((1, 2, R.NF), np.float32))[2][0, :, 0]


PHILOX_SITES = {"host twin (DQN)": lambda s, d: _slots_dqn(lr.run_host, s, d),
                "host twin (Rainbow)": lambda s, d: _slots_rainbow(R.run_host, s, d),
                "dqn_learn_ref.c": lambda s, d: _slots_dqn(lr.run_ref, s, d),
                "rainbow_learn_ref.c": lambda s, d: _slots_rainbow(R.run_ref, s, d)}


@pytest.mark.parametrize("site", list(PHILOX_SITES))
@pytest.mark.parametrize("kat", range(3))
def test_philox_of_the_learners_against_the_known_answers(coracle, site, kat):
    """A ring of 2^16 rows that stores its row numbers: slot = (x 2^16) >> 32 shows the top 16 bits of Philox
    word x for counter (b, 0, draw lo, draw hi) under key (seed lo, seed hi). The learners' entry points set
    c0 = b < 1024 and c1 = b >> 32 = 0, so of the published vectors only the first (c0 = c1 = 0, at b = 0) is
    reachable as it stands and is asserted against the published word; the second and third give their c2, c3
    and both key words (every one non-zero), and the words for c0 = b, c1 = 0 come from the C oracle's Philox,
    which this test pins to all three published vectors first. c1 itself is left to the C oracle
    (tests/test_philox.py)."""
    ctr, key, out = W.KATS[kat]
    assert np.array_equal(coracle.philox(ctr, key), np.array(out, np.uint32))
    seed, draw = _join(*key), _join(ctr[2], ctr[3])
    got = PHILOX_SITES[site](seed, draw).astype(np.int64)
    want = np.array([int(coracle.philox([b, 0, ctr[2], ctr[3]], key)[0]) >> 16 for b in range(BATCH)])
    assert np.array_equal(got, want), (site, got[:4], want[:4])
    assert np.array_equal(want, mo.replay_sample_index(coracle, W.PROBE_CAP, W.PROBE_CAP, seed, draw, BATCH))
    if ctr[0] == 0 and ctr[1] == 0:
        assert got[0] == out[0] >> 16  # the published word itself
    assert len(set(got.tolist())) > BATCH // 2  # slots, not a constant


# ------------------------------------------------------------------ 2. both learners at wide seeds and draws
WIDE = [(W.SEED_W, W.DRAW_W), (W.SEED_MAX, W.DRAW_MAX), (W.SEED_TOP, W.DRAW_WRAP)]
WIDE_IDS = ["seed_w-draw_w", "max-seed-and-draw", "draw-wraps"]


def _want_rows(coracle, ring, counter, seed, draw, filled_only):
    return np.stack([ring[mo.replay_sample_index(coracle, len(ring), counter, seed, (draw + u) & W.U64, BATCH,
                                                 filled_only)] for u in range(UPDATES)])


@pytest.mark.parametrize("filled_only", [False, True])
@pytest.mark.parametrize("seed,draw", WIDE, ids=WIDE_IDS)
def test_dqn_host_learn_at_wide_seed_and_draw(coracle, seed, draw, filled_only):
    """mg_host_dqn_learn: the sampled rows are the ring at the oracle's slots, and eval, target, m, v, the losses
    and the rows equal the restatement bit for bit. The third case's first_draw + 1 wraps to 0."""
    rows, sd = lr.case_fixture(10, 5, 32)
    ring, counter = lr.half_filled(rows)
    L0 = lr.learner_array(sd)
    kw = dict(num_updates=UPDATES, seed=seed, first_draw=draw, filled_only=filled_only)
    ref, ref_loss, ref_rows, _ = lr.run_ref(L0, ring, counter, 10, 5, BATCH, **kw)
    got, got_loss, got_rows = lr.run_host(L0, ring, counter, 10, 5, BATCH, **kw)
    want_rows = _want_rows(coracle, ring, counter, seed, draw, filled_only)
    assert np.array_equal(lr.bits(got_rows), lr.bits(want_rows))
    assert np.array_equal(lr.bits(ref_rows), lr.bits(want_rows))
    assert np.array_equal(lr.bits(got_loss), lr.bits(ref_loss)), (got_loss, ref_loss)
    for blk, name in enumerate(("eval", "target", "m", "v")):
        assert np.array_equal(lr.bits(got[blk]), lr.bits(ref[blk])), name
    assert not np.array_equal(got[0], L0[0]) and np.all(np.isfinite(got)) and np.all(np.isfinite(got_loss))
    # the draws differ from the ones the low words alone would give
    low = _want_rows(coracle, ring, counter, seed & 0xFFFFFFFF, draw & 0xFFFFFFFF, filled_only)
    assert not np.array_equal(want_rows, low)


@pytest.mark.parametrize("seed,draw", WIDE, ids=WIDE_IDS)
def test_rainbow_host_learn_at_wide_seed_and_draw(coracle, seed, draw):
    """mg_host_rainbow_learn (it always draws among the stored rows) on a wrapped ring of 64 rows."""
    ring, counter = R.ring_case(64, 200)
    L0 = R.learner_numpy(R.golden_state(1, "default"))
    nf = R.noise(UPDATES)
    Lw, *want = R.run_ref(L0, ring, counter, BATCH, UPDATES, 0, seed, draw, nf)
    Lg, *got = R.run_host(L0, ring, counter, BATCH, UPDATES, 0, seed, draw, nf)
    R.assert_same((Lg, got), (Lw, want))
    want_rows = _want_rows(coracle, ring, counter, seed, draw, True)
    assert np.array_equal(lr.bits(got[1]), lr.bits(want_rows))
    assert np.isfinite(got[0]).all() and np.abs(got[3]).max() > 0
    assert not np.array_equal(want_rows, _want_rows(coracle, ring, counter, seed & 0xFFFFFFFF, draw & 0xFFFFFFFF, True))


# ------------------------------------------------------------------ 3. Adam's scalars at a large update count
LATE = [10**6, (1 << 32) + 5]  # pow(beta, t + 1) has underflowed; t + 1 needs more than 32 bits


@pytest.mark.parametrize("first_update", LATE)
def test_dqn_host_adam_at_a_large_update_count(first_update):
    """target_period 2: the target copy falls on update 10^6 (the call's first) and on 2^32 + 6 (its second), so
    first_update + u is also tested as the 64-bit operand of the modulo."""
    rows, sd = lr.case_fixture(10, 5, 32)
    ring, counter = lr.half_filled(rows)
    L0 = lr.learner_array(sd)
    L0[1] *= np.float32(0.5)
    kw = dict(num_updates=UPDATES, first_update=first_update, seed=7, first_draw=5, target_period=2)
    ref, ref_loss, ref_rows, _ = lr.run_ref(L0, ring, counter, 10, 5, BATCH, **kw)
    got, got_loss, got_rows = lr.run_host(L0, ring, counter, 10, 5, BATCH, **kw)
    assert np.array_equal(lr.bits(got_rows), lr.bits(ref_rows)) and np.array_equal(lr.bits(got_loss), lr.bits(ref_loss))
    for blk, name in enumerate(("eval", "target", "m", "v")):
        assert np.array_equal(lr.bits(got[blk]), lr.bits(ref[blk])), name
    assert np.all(np.isfinite(got)) and not np.array_equal(got[0], L0[0]) and not np.array_equal(got[1], L0[1])
    # the bias corrections are gone by now: the same call at update 0 moves the parameters differently
    early, _, _ = lr.run_host(L0, ring, counter, 10, 5, BATCH, **dict(kw, first_update=first_update % 2))
    assert not np.array_equal(early[0], got[0])


@pytest.mark.parametrize("first_update", LATE)
def test_rainbow_host_adam_at_a_large_update_count(first_update):
    ring, counter = R.ring_case(64, 200)
    L0 = R.learner_numpy(R.golden_state(1, "soft"))
    nf = R.noise(UPDATES)
    Lw, *want = R.run_ref(L0, ring, counter, BATCH, UPDATES, first_update, 3, 0, nf)
    Lg, *got = R.run_host(L0, ring, counter, BATCH, UPDATES, first_update, 3, 0, nf)
    R.assert_same((Lg, got), (Lw, want))
    assert np.isfinite(Lg).all() and not np.array_equal(Lg[:R.NP], L0[:R.NP])
    early = R.run_host(L0, ring, counter, BATCH, UPDATES, 0, 3, 0, nf)[0]
    assert not np.array_equal(early[:R.NP], Lg[:R.NP])
