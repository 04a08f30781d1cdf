"""mg_stats_reduce_many (distributed.device_totals_many, MergeVecEnv.member_totals / league_summary) and
DQNPopulation.cross_play.

The segmented reduction is the lone one with the segment in the grid, so segment s of its output is, to the bit,
mg_stats_reduce on records [s n_segment, (s + 1) n_segment) -- and the oracle's restatement of that fixed order on
the slice. The shapes put a segment below, at and past one 1,024-record block, past two, at the most segments the
call takes, and at no record at all. league_summary and cross_play are then pinned to what exists: the summary of
each slice, with exact float equality, and the three calls cross_play is made of."""

import ctypes

import numpy as np
import pytest

import guard_bands
import learn_ref as lr
import merge_oracle as mo

pytestmark = pytest.mark.gpu

NEG_ZERO = np.array(-0.0).view(np.uint64)


def _records(n, seed):
    """test_stats_reduce_fixed_order's records: mixed signs, magnitudes spread over 18 decades, -0.0, denormal-scale
    values and counts up to 2^31."""
    rng = np.random.default_rng(seed)
    rec = np.zeros((max(n, 1), 8))[:n]
    rec[:, :4] = rng.normal(0, 1, (n, 4)) * 10.0 ** rng.integers(-12, 6, (n, 4))
    rec[:, 7] = rng.normal(0, 1, n) * 10.0 ** rng.integers(-6, 4, n)  # q_eval
    if n:
        rec[:: 7, 0] = -0.0
        rec[:: 11, 2] = rng.uniform(-1e-300, 1e-300, rec[:: 11, 2].shape)
    cnt = rec[:, 4:].view(np.uint32)
    cnt[:, :6] = rng.integers(0, 1 << 31, (n, 6), dtype=np.uint32)
    return rec


SHAPES = [(1, 1), (64, 9), (1023, 3), (1024, 3), (1025, 3), (2112, 2), (64, 4096), (0, 5)]


@pytest.mark.parametrize("n_segment,segments", SHAPES, ids=[f"n{n}-S{s}" for n, s in SHAPES])
def test_every_segment_equals_the_lone_reduction(n_segment, segments):
    import torch

    from merging_gym import _native
    from merging_gym.distributed import device_totals, device_totals_many

    n, S = n_segment, segments
    rec = _records(n * S, 1000 * S + n)
    dev = torch.from_numpy(rec.copy()).cuda()
    got = device_totals_many(dev, S)
    assert got.shape == (S, 10) and got.dtype == torch.int64
    # the lone reduction of every slice, collected on the device: one copy
    lone = torch.stack([device_totals(dev[s * n:(s + 1) * n]) for s in range(S)])
    assert torch.equal(got, lone)
    tot = got.cpu().numpy()
    for s in range(S):
        sums, counts = mo.stats_reduce_fixed(rec[s * n:(s + 1) * n])
        assert tot[s, :4].view(np.uint64).tolist() == np.array(sums, np.float64).view(np.uint64).tolist(), s
        assert tot[s, 4:].tolist() == counts, s
    if n == 0:  # the empty segments: zero counts, and -0.0 (the additive identity) with its sign bit
        assert (tot[:, 4:] == 0).all()
        assert (tot[:, :4].view(np.uint64) == NEG_ZERO).all()
    # the same call on exactly sized totals and scratch inside guard bands: nothing past totals[segments] or past
    # the scratch is written, and the result is the same
    g = guard_bands.Guarded(torch, dev.device)
    totals = g.tensor("totals", (S, 10), torch.int64)
    bytes_ = int(_native.lib.mg_stats_reduce_many_scratch_bytes(n, S))
    assert bytes_ == S * ((n + 1023) // 1024) * 80
    scratch = g.tensor("scratch", (max(bytes_, 16) // 8,), torch.int64)
    stream = torch.cuda.current_stream(dev.device)
    rc = _native.lib.mg_stats_reduce_many(ctypes.c_void_p(dev.data_ptr()), n, S, ctypes.c_void_p(totals.data_ptr()),
                                          ctypes.c_void_p(scratch.data_ptr()), bytes_,
                                          ctypes.c_void_p(stream.cuda_stream))
    _native.check(rc, "mg_stats_reduce_many")
    assert torch.equal(totals, got)
    g.assert_bands_intact()
    if bytes_ == 0:  # and an unused scratch is not touched at all
        assert bool((g.raw["scratch"][0] == guard_bands.FILL).all())


def test_device_totals_many_refusals():
    import torch

    from merging_gym.distributed import device_totals_many

    dev = torch.zeros((192, 8), dtype=torch.float64, device="cuda")
    for segments in (0, 5, 4097):
        with pytest.raises(ValueError, match="equal runs"):
            device_totals_many(dev, segments)


STATE = ("p1", "v1", "p2", "v2", "ret1", "ret2", "tf")


def test_league_summary_and_cross_play():
    """K = 3 on 9 slices of 64 envs. league_summary(3)[key][i, j] is summarize() of slice 3 i + j for every key,
    exactly; cross_play returns the matrices of the three calls it is made of, clears the statistics the env
    held before, and leaves the rings, the learners' buffers, their counters and the packed nets as they were."""
    import torch

    from merging_gym import DQNPopulation, MergeVecEnv, ReplayRing
    from merging_gym.distributed import summarize

    K, n, T = 3, 64, 8
    N = K * K * n
    rings = [ReplayRing(64, device="cuda:0") for _ in range(K)]
    for k, r in enumerate(rings):  # rows and counters a store would have left
        r.memory.copy_(torch.from_numpy(np.random.default_rng(k).normal(size=tuple(r.memory.shape)).astype(np.float32)))
        r._counter.fill_(40 + k)
    pop = DQNPopulation([lr.seeded_net(10, 5, 500 + k) for k in range(K)], rings, seed=[11, 12, 13])
    env = MergeVecEnv(N, device="cuda:0", env_offset=7 * N)
    env.params.timeout_steps = 4  # every env completes two episodes in eight steps
    for k in range(12):           # and the env holds statistics of its own before the league plays
        env.step_random(5, step_idx=k)
    start = {k: getattr(env, k).clone() for k in STATE}
    stats = env._ep_stats.clone()
    assert int(env.counts[:, 0].min()) >= 2
    eps = [0.7, 0.4, 0.9]

    def restart():
        for k in STATE:
            getattr(env, k).copy_(start[k])
        env._ep_stats.copy_(stats)
        env._step_idx = 500

    restart()
    env.clear_statistics()
    assert env.rollout_qnet_league(T, pop.qnets, pop.seed, eps, trajectory=False) is None
    totals = env.member_totals(K * K)
    assert totals.shape == (K * K, 10) and totals.is_cuda
    pay = env.league_summary(K)
    keys = set(summarize(env.returns[:n], env.counts[:n]))
    assert set(pay) == keys
    for p in range(K * K):
        i, j = divmod(p, K)
        ref = summarize(env.returns[p * n:(p + 1) * n], env.counts[p * n:(p + 1) * n])
        assert ref["completed"] >= 2 * n
        for key in keys:
            m = pay[key]
            assert m.shape == (K, K) and not m.is_cuda
            assert m.dtype == (torch.int64 if key == "completed" else torch.float64), key
            assert m[i, j].item() == ref[key], (key, i, j, m[i, j].item(), ref[key])
    assert len({float(v) for v in pay["mean_return_ego"].flatten()}) > 1  # the pairings did fare differently

    before = ([r.memory.clone() for r in rings], [r._counter.clone() for r in rings], pop._buf.clone(),
              pop._packed.clone(), pop.learn_step_counter, pop.draw_counter, pop.seed)
    restart()
    again = pop.cross_play(env, T, episilo=eps)
    assert env._step_idx == 500 + T
    assert set(again) == keys
    for key in keys:
        assert torch.equal(again[key], pay[key]), key  # the same matrices: the earlier statistics were cleared
    for r, mem, ctr in zip(rings, before[0], before[1]):
        assert torch.equal(r.memory, mem) and torch.equal(r._counter, ctr)
    assert torch.equal(pop._buf, before[2]) and torch.equal(pop._packed, before[3])
    assert (pop.learn_step_counter, pop.draw_counter, pop.seed) == before[4:]
    with pytest.raises(ValueError, match="equal slices"):
        env.member_totals(5)
    with pytest.raises(ValueError, match="1..64 nets"):
        env.league_summary(65)
