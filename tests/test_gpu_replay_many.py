"""replay.store_rollout_many (mg_replay_store_many): one [T, N, ...] rollout into M rings in three launches.

Member m's ring and counter must end byte for byte as ReplayRing.store leaves them when given a contiguous
copy of the member's slice. The tensors are synthetic, so the won mask is the test's: random at several
densities, one member whose every bit is set (it keeps nothing: ring and counter untouched) and one all clear.
n_member = 320 is one 256-env write block and a partial one and puts the member boundaries off the 256 grid;
T = 3 leaves half a chunk; the counters start at 0, short of a wrap, and above 2^32."""

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CAP, GUARD, CANARY, FRESH = 2000, 4, -12345.5, -7.0
STARTS = [0, 1990, (1 << 32) + 123, 7, 1999, 4001]
DENSITY = [0.1, 0.5, 0.9]


@pytest.fixture(scope="module")
def torch():
    import torch as t

    return t


def _ring(torch, start):
    """A ReplayRing of CAP rows whose memory lies inside a larger buffer, GUARD canary rows on either side."""
    from merging_gym import ReplayRing

    ring = ReplayRing(CAP, device="cuda:0")
    whole = torch.full((CAP + 2 * GUARD, ring.row), CANARY, dtype=torch.float32, device="cuda:0")
    ring.memory = whole[GUARD:GUARD + CAP]
    ring.memory.fill_(FRESH)
    ring._counter.fill_(start)
    return ring, whole


def _batch(torch, M, n, T, seed):
    """Synthetic [T, N, ...] rollout tensors and the won mask: member 1 all set, member 2 all clear, the others
    random at a density of their own."""
    N = M * n
    g = torch.Generator(device="cpu").manual_seed(seed)
    dev = "cuda:0"
    flags = torch.zeros((T, N, 4), dtype=torch.uint8)
    flags[..., 0] = torch.randint(0, 5, (T, N), generator=g).to(torch.uint8)
    flags[..., 1] = 255  # a2 = -1
    flags[..., 2] = (torch.rand((T, N), generator=g) < 0.3).to(torch.uint8)
    won = torch.zeros((T, N), dtype=torch.bool)
    for m in range(M):
        s = slice(m * n, (m + 1) * n)
        if m == 1:
            won[:, s] = True
        elif m != 2:
            won[:, s] = torch.rand((T, n), generator=g) < DENSITY[m % 3]
    bits = won.reshape(T, N // 64, 64).to(torch.int64)
    words = (bits << torch.arange(64, dtype=torch.int64)).sum(-1)  # bit 63 wraps into the sign: the same bits
    traj = {"obs": torch.randn((T, N, 10), generator=g).to(dev), "rew": torch.randn((T, N, 2), generator=g).to(dev),
            "flags": flags.to(dev), "final_observation": torch.randn((T, N, 10), generator=g).to(dev),
            "won_mask": words.to(dev)}
    return torch.randn((N, 10), generator=g).to(dev), traj, won


def _check(torch, M, n, T, skip):
    from merging_gym.replay import store_rollout_many

    obs0, traj, won = _batch(torch, M, n, T, 100 * M + n + T)
    starts = [STARTS[(m + T) % len(STARTS)] for m in range(M)]
    rings, wholes = zip(*(_ring(torch, s) for s in starts))
    store_rollout_many(rings, obs0, traj, skip_ego_won=skip)
    w = n // 64
    for m in range(M):
        s = slice(m * n, (m + 1) * n)
        ref, _ = _ring(torch, starts[m])
        _store_slice(ref, obs0, traj, s, m, w, skip)
        kept = int((~won[:, s]).sum()) if skip else T * n
        assert int(rings[m]._counter.item()) == int(ref._counter.item()) == starts[m] + kept, m
        assert rings[m].memory.cpu().numpy().tobytes() == ref.memory.cpu().numpy().tobytes(), f"member {m}"
        if kept == 0:  # nothing kept: the ring was never written
            assert bool((rings[m].memory == FRESH).all())
        else:
            assert bool((rings[m].memory != FRESH).any())
        guard = torch.cat([wholes[m][:GUARD], wholes[m][GUARD + CAP:]])
        assert bool((guard == CANARY).all()), f"member {m}: canary rows"


def _store_slice(ref, obs0, traj, s, m, w, skip):
    """ReplayRing.store on a contiguous copy of the member's slice (the mask words repacked: n_member is a
    multiple of 64, so they are the member's own words)."""
    flags = traj["flags"][:, s].contiguous()
    ref.store(obs0[s].contiguous(), traj["obs"][:, s].contiguous(), flags[..., 0].view(ref._torch.int8),
              traj["rew"][:, s].contiguous(), final_obs=traj["final_observation"][:, s].contiguous(),
              won_mask=traj["won_mask"][:, m * w:(m + 1) * w].contiguous(), skip_ego_won=skip, flags=flags)


@pytest.mark.parametrize("skip", [True, False], ids=["skip-won", "keep-all"])
@pytest.mark.parametrize("T", [1, 3, 4])
@pytest.mark.parametrize("n", [64, 320])
@pytest.mark.parametrize("M", [1, 3, 64])
def test_member_store_equals_lone_store_bit_for_bit(torch, M, n, T, skip):
    _check(torch, M, n, T, skip)


@pytest.mark.parametrize("skip", [True, False], ids=["skip-won", "keep-all"])
def test_member_store_overflow_keeps_the_newest_rows(torch, skip):
    """n_member = 1,088, T = 3: 3,264 rows per member into 2,000 slots (fewer where the won filter drops some)."""
    _check(torch, 2, 1088, 3, skip)


def test_member_store_refusals(torch):
    from merging_gym import ReplayRing
    from merging_gym.replay import store_rollout_many

    obs0, traj, _ = _batch(torch, 2, 64, 2, 5)
    a, b = ReplayRing(CAP, device="cuda:0"), ReplayRing(CAP, device="cuda:0")
    with pytest.raises(ValueError, match="listed twice"):
        store_rollout_many([a, a], obs0, traj)
    with pytest.raises(ValueError, match="goal rings are refused"):
        store_rollout_many([a, ReplayRing(CAP, device="cuda:0", goal=True)], obs0, traj)
    with pytest.raises(ValueError, match="one capacity"):
        store_rollout_many([a, ReplayRing(CAP + 1, device="cuda:0")], obs0, traj)
    with pytest.raises(ValueError, match="slices of a multiple of 64"):
        store_rollout_many([a, b, ReplayRing(CAP, device="cuda:0")], obs0, traj)
    with pytest.raises(ValueError, match="final_observation"):
        store_rollout_many([a, b], obs0, dict(traj, final_observation=None))
    with pytest.raises(ValueError, match="won_mask"):
        store_rollout_many([a, b], obs0, dict(traj, won_mask=None))
    # the library's own check of the pointers, under the Python one: two members on one ring's memory
    c = ReplayRing(CAP, device="cuda:0")
    c.memory = a.memory
    with pytest.raises(a._nat.NativeError, match="listed twice"):
        store_rollout_many([a, c], obs0, traj)
    assert int(a._counter.item()) == 0 and int(b._counter.item()) == 0
    store_rollout_many([a, b], obs0, dict(traj, won_mask=None), skip_ego_won=False)
    assert int(a._counter.item()) == 128 and int(b._counter.item()) == 128
