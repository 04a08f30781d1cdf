"""A population of Rainbow learners on the GPU: mg_rainbow_learn_many against the plain-C restatement run once per
member, bit for bit; RainbowPopulation against M lone RainbowLearner(DeviceNoise)s through Python; the population's
noise against its host twin; determinism; the target copy under a member mask; checkpoints and copy_member; the
constructor's refusals."""
import numpy as np
import pytest

import rainbow_learn_many_ref as many
import rainbow_learn_ref as R
from learn_ref import bits

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
U = 3


@pytest.fixture(scope="module")
def torch():
    import torch

    return torch


def _replay(torch, ring, counter):
    from merging_gym import RainbowReplay

    rp = RainbowReplay(len(ring), device=DEV)
    rp.memory.copy_(torch.from_numpy(np.ascontiguousarray(ring, dtype=np.float32)))
    rp._counter.fill_(counter)
    return rp


def run_device_members(torch, L, settings, ring_list, B, num_updates, noise_f, calls=None):
    """mg_rainbow_learn_many on device copies: run_ref_members' tuple, then the member array and the packed nets."""
    from merging_gym import _native

    lib, M = _native.lib, len(settings)
    stream = torch.cuda.current_stream(DEV).cuda_stream
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, dtype=np.float32)).to(DEV)  # noqa: E731
    Ld, nf = f32(L), f32(noise_f)
    replays = [_replay(torch, r, c) for r, c in ring_list]
    members = many.member_array(settings, [r.memory.data_ptr() for r in replays],
                                [r._counter.data_ptr() for r in replays])
    tbytes = lib.mg_rainbow_learn_many_table_bytes(M)
    table = torch.empty(tbytes, dtype=torch.uint8, device=DEV)
    _native.check(lib.mg_rainbow_learn_many_init(table.data_ptr(), tbytes, members, M, stream), "init")
    sbytes = M * lib.mg_rainbow_learn_scratch_bytes(B)
    scratch = torch.empty(sbytes // 4, dtype=torch.float32, device=DEV)
    stride = lib.mg_rainbow_packed_bytes()
    packed = torch.zeros((M, stride), dtype=torch.uint8, device=DEV)
    outs = [torch.zeros(s, dtype=torch.float32, device=DEV)
            for s in ((num_updates, M), (num_updates, M, B, R.ROW), (num_updates, M, B, R.NZ), (num_updates, M, R.NP))]
    u0 = 0
    for n in calls or [num_updates]:
        rc = lib.mg_rainbow_learn_many(Ld.data_ptr(), table.data_ptr(), tbytes, members, M, len(ring_list[0][0]), B, n,
                                       nf[u0:].data_ptr() if n else None, *(o[u0:].data_ptr() for o in outs),
                                       packed.data_ptr(), stride, scratch.data_ptr(), sbytes, stream)
        _native.check(rc, "mg_rainbow_learn_many")
        u0 += n
    torch.cuda.synchronize()
    return (Ld.cpu().numpy(), *(o.cpu().numpy() for o in outs), members, packed.cpu().numpy())


@pytest.mark.parametrize("B,M", [(1, 2), (33, 3), (128, 2), (8, 64), (1024, 2)])
def test_every_member_equals_the_restatement(torch, B, M):
    """(1024, 2): the largest batch, so the largest per-member scratch stride."""
    settings, ring_list = many.member_settings(M), many.rings(M)
    L, nf = many.learners(M), many.noise(U, M)
    got = run_device_members(torch, L, settings, ring_list, B, U, nf)
    want = many.run_ref_members(L, settings, ring_list, B, U, nf)
    many.assert_members_same(got, want)
    for m in ([0, 31, 32, 47, 63] if M == 64 else range(M)):  # the mask's and the argument arrays' top half too
        assert (bits(got[0][m]) == bits(want[0][m])).all() and (bits(got[1][:, m]) == bits(want[1][:, m])).all()
        assert (bits(got[0][m][2 * R.NP:3 * R.NP]) == bits(want[0][m][2 * R.NP:3 * R.NP])).all()  # Adam's m
    # the "soft" members moved (a "default" member's softmax saturates: at B = 1 its gradient is exactly zero,
    # at B = 33 it has non-zero entries of at most 2e-4, so nothing is asked of those members here)
    assert all((bits(got[0][m][:R.NP]) != bits(L[m][:R.NP])).any() for m in range(0, M, 2))
    for s, e in zip(settings, got[5]):
        assert (int(e.first_update), int(e.first_draw)) == (s["first_update"] + U, s["first_draw"] + U)


def test_runs_repeat_and_k_updates_in_one_call_equal_k_calls(torch):
    settings, ring_list = many.member_settings(3), many.rings(3)
    L, nf = many.learners(3), many.noise(U, 3)
    a = run_device_members(torch, L, settings, ring_list, 33, U, nf)
    b = run_device_members(torch, L, settings, ring_list, 33, U, nf)
    c = run_device_members(torch, L, settings, ring_list, 33, U, nf, calls=[1, 0, 2])
    for other in (b, c):
        many.assert_members_same(other, a)
        assert (other[6] == a[6]).all()  # the packed nets
        assert [int(e.first_update) for e in other[5]] == [int(e.first_update) for e in a[5]]


def test_noise_many_equals_its_host_twin(torch):
    from merging_gym import _native

    seeds = np.array([7, (1 << 63) + 12345, 99], dtype=np.uint64)
    first = np.array([0, 3, (1 << 32) + 5], dtype=np.uint64)
    host = np.zeros((2, 3, 2, R.NF), np.float32)
    _native.check(_native.lib.mg_host_rainbow_noise_many(seeds.ctypes.data, first.ctypes.data, 3, 2, host.ctypes.data),
                  "mg_host_rainbow_noise_many")
    dev = torch.zeros((2, 3, 2, R.NF), dtype=torch.float32, device=DEV)
    rc = _native.lib.mg_rainbow_noise_many(seeds.ctypes.data, first.ctypes.data, 3, 2, dev.data_ptr(),
                                           torch.cuda.current_stream(DEV).cuda_stream)
    _native.check(rc, "mg_rainbow_noise_many")
    assert (bits(dev.cpu().numpy()) == bits(host)).all()
    assert np.isfinite(host).all() and (host != 0).all()


# ---------------------------------------------------------------------------- through Python
SEEDS, NSEEDS = (3, 4, 5), (11, 1 << 63, 13)
LRS, GAMMAS, BETAS, EPSS = (0.001, 0.002, 0.0005), (0.99, 0.95, 0.9), ((0.9, 0.999), (0.8, 0.99), (0.85, 0.995)), \
    (1e-8, 1e-7, 2e-8)


def _nets(M=3):
    return [R.golden_state(1, "soft" if m % 2 == 0 else "default") for m in range(M)]


def _pair(torch, B=32, M=3):
    """(population, the M lone learners it must equal), each on replays of its own with the same rows."""
    from merging_gym import DeviceNoise, RainbowLearner, RainbowPopulation

    ring_list = many.rings(M)
    pop = RainbowPopulation(_nets(M), [_replay(torch, *rc) for rc in ring_list], lr=LRS[:M], gamma=GAMMAS[:M],
                            batch_size=B, seed=SEEDS[:M], noise_seed=NSEEDS[:M], betas=BETAS[:M], eps=EPSS[:M], device=DEV)
    lone = [RainbowLearner(_nets(M)[m], _replay(torch, *ring_list[m]), lr=LRS[m], gamma=GAMMAS[m], batch_size=B,
                           seed=SEEDS[m], generator=DeviceNoise(NSEEDS[m]), device=DEV, betas=BETAS[m], eps=EPSS[m])
            for m in range(M)]
    return pop, lone


def _same(torch, a, b):
    """Bit for bit, whatever the dtype and the strides."""
    return a.shape == b.shape and a.dtype == b.dtype and a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def _assert_members(torch, pop, lone, what=""):
    for m, lr in enumerate(lone):
        assert _same(torch, pop._buf[m], lr._buf), f"{what}: member {m}'s learner block"
        assert _same(torch, pop.nets[m].packed, lr.net.packed), f"{what}: member {m}'s packed net"
        assert (pop.learn_step_counter[m], pop.draw_counter[m]) == (lr.learn_step_counter, lr.draw_counter)


def test_population_equals_lone_learners(torch):
    pop, lone = _pair(torch)
    assert len(pop) == 3 and pop.seed == list(SEEDS) and pop.noise_seed == list(NSEEDS)
    _assert_members(torch, pop, lone, "as built")
    obs = torch.from_numpy(R.replay_rows(64, seed=5)[:, :10].copy()).to(DEV)
    for n in (2, 1):
        loss = pop.learn(n, return_loss=True)
        assert tuple(loss.shape) == (n, 3)
        for m, lr in enumerate(lone):
            assert _same(torch, loss[:, m], lr.learn(n, return_loss=True)), f"member {m}'s losses"
        _assert_members(torch, pop, lone, f"after learn({n})")
        for m, lr in enumerate(lone):
            for mine, theirs in zip(pop.nets[m].forward(obs, logits=True), lr.net.forward(obs, logits=True)):
                assert _same(torch, mine, theirs), f"member {m}'s forward"
            mine, theirs = pop.nets[m].state, lr.net.state  # read back lazily from the member's block
            assert all(torch.equal(mine[k], theirs[k]) for k in theirs)
    assert pop.learn_step_counter == [3, 3, 3] and pop.draw_counter == [3, 3, 3]
    assert not _same(torch, pop._buf[0], pop._buf[2])
    rows, proj, grads = pop.learn(1, return_rows=True, return_proj=True, return_grads=True)
    assert (tuple(rows.shape), tuple(proj.shape), tuple(grads.shape)) == ((1, 3, 32, 24), (1, 3, 32, 51), (1, 3, R.NP))
    assert pop.learn(0) is None and pop.learn_step_counter == [4, 4, 4]


def test_members_act_with_the_learned_weights_and_noise(torch):
    """env.rollout_rainbow(T, pop.nets[m]) is the lone learner's rollout, and a fresh net packed from the member's
    current model (noise included) is the member's packed net."""
    from merging_gym import MergeVecEnv, RainbowNet

    pop, lone = _pair(torch, B=8)
    before = pop._packed.clone()
    pop.learn(2)
    for lr in lone:
        lr.learn(2)
    for m in (0, 2):
        assert not _same(torch, pop.nets[m].packed, before[m])
        fresh = RainbowNet.from_state_dict(pop.current_state_dict(m), device=DEV)
        assert _same(torch, pop.nets[m].packed, fresh.packed)
        mine = MergeVecEnv(128, device=DEV).rollout_rainbow(4, pop.nets[m])
        theirs = MergeVecEnv(128, device=DEV).rollout_rainbow(4, lone[m].net)
        for k in ("obs", "a1", "rew", "done"):
            assert _same(torch, mine[k], theirs[k]), f"member {m}'s {k}"
    with pytest.raises(RuntimeError, match="owns this net's noise"):
        pop.nets[0].reset_noise()


def test_noise_seed_defaults_to_the_minibatch_seed(torch):
    from merging_gym import RainbowPopulation

    pop = RainbowPopulation(_nets(2), [_replay(torch, *many.rings(1)[0])] * 2, seed=[8, 9], batch_size=4, device=DEV)
    assert pop.noise_seed == [8, 9]


def test_sync_target_under_a_mask(torch):
    pop, lone = _pair(torch, B=8)
    pop.learn(2)
    for lr in lone:
        lr.learn(2)
    before = pop._buf.clone()
    pop.sync_target([1])
    NP, NE, EPS = R.NP, R.NE, 4 * R.NP
    assert _same(torch, pop._buf[0], before[0]) and _same(torch, pop._buf[2], before[2])
    assert _same(torch, pop._buf[1, NP:2 * NP], before[1, :NP])
    assert _same(torch, pop._buf[1, EPS + NE:EPS + 2 * NE], before[1, EPS:EPS + NE])
    assert not _same(torch, before[1, NP:2 * NP], before[1, :NP])
    lone[1].sync_target()
    assert _same(torch, pop._buf[1], lone[1]._buf)
    pop.sync_target()
    for lr in (lone[0], lone[2]):
        lr.sync_target()
    _assert_members(torch, pop, lone, "after sync_target()")
    pop.learn(1)
    for lr in lone:
        lr.learn(1)
    _assert_members(torch, pop, lone, "an update after the copy")
    with pytest.raises(IndexError):
        pop.sync_target([3])
    for bad in (3, -1):  # a negative index is no member from the end
        for call in (pop.current_state_dict, pop.target_state_dict, pop.member_state_dict,
                     lambda m: pop.copy_member(0, m), lambda m: pop.copy_member(m, 0),
                     lambda m: pop.load_member_state_dict(m, pop.member_state_dict(0)), lambda m: pop.sync_target([m])):
            with pytest.raises(IndexError):
                call(bad)


def test_member_state_loads_into_a_lone_learner_and_back(torch):
    from merging_gym import DeviceNoise, RainbowLearner

    pop, lone = _pair(torch, B=8)
    pop.learn(2)
    for lr in lone:
        lr.learn(2)
    sd = pop.member_state_dict(1)
    theirs = lone[1].state_dict()
    assert set(sd) == set(theirs) and all(k == "learner" or sd[k] == theirs[k] for k in sd)
    assert _same(torch, sd["learner"], theirs["learner"])
    fresh = RainbowLearner(_nets()[0], lone[1].replay, lr=LRS[1], gamma=GAMMAS[1], batch_size=8, seed=0,
                           generator=DeviceNoise(0), device=DEV, betas=BETAS[1], eps=EPSS[1])
    fresh.load_state_dict(sd)
    a, b = pop.learn(1, return_loss=True)[:, 1], fresh.learn(1, return_loss=True)
    assert _same(torch, a, b) and _same(torch, pop._buf[1], fresh._buf) and _same(torch, pop.nets[1].packed,
                                                                                  fresh.net.packed)
    # and back: member 1's state into member 0's seat of another population with member 1's hyperparameters
    lone[1].learn(1)
    other, _ = _pair(torch, B=8)
    other.load_member_state_dict(1, lone[1].state_dict())
    assert _same(torch, other._buf[1], lone[1]._buf) and _same(torch, other.nets[1].packed, lone[1].net.packed)
    x, y = other.learn(1, return_loss=True)[:, 1], lone[1].learn(1, return_loss=True)
    assert _same(torch, x, y) and _same(torch, other._buf[1], lone[1]._buf)
    with pytest.raises(ValueError, match="torch"):
        other.load_member_state_dict(0, dict(lone[0].state_dict(), noise="torch"))


def test_state_dict_round_trip_mid_run(torch):
    pop, _ = _pair(torch, B=8)
    pop.learn(2)
    sd = pop.state_dict()
    want = pop.learn(2, return_loss=True)
    resumed, _ = _pair(torch, B=8)
    resumed.load_state_dict(sd)
    from merging_gym import RainbowNet

    for m in range(3):  # the load repacked every member from its new current model
        fresh = RainbowNet.from_state_dict(resumed.current_state_dict(m), device=DEV)
        assert _same(torch, resumed.nets[m].packed, fresh.packed), f"member {m}'s packed net after the load"
    with pytest.raises(ValueError, match="torch"):
        resumed.load_state_dict(dict(sd, noise="torch"))
    got = resumed.learn(2, return_loss=True)
    assert _same(torch, got, want) and _same(torch, resumed._buf, pop._buf) and _same(torch, resumed._packed, pop._packed)
    assert resumed.learn_step_counter == pop.learn_step_counter == [4, 4, 4]


def test_copy_member(torch):
    pop, lone = _pair(torch, B=8)
    pop.learn(2)
    buf2 = pop._buf[2].clone()
    pop.copy_member(0, 1)
    assert _same(torch, pop._buf[1], pop._buf[0]) and _same(torch, pop.nets[1].packed, pop.nets[0].packed)
    assert _same(torch, pop._buf[2], buf2)
    assert pop.seed == list(SEEDS) and pop.noise_seed == list(NSEEDS)  # dst keeps its seeds
    # member 1 continues as a lone learner with member 0's state under member 1's seeds and hyperparameters
    lone[1].load_state_dict(dict(pop.member_state_dict(0), seed=SEEDS[1], noise_seed=NSEEDS[1]))
    a, b = pop.learn(1, return_loss=True)[:, 1], lone[1].learn(1, return_loss=True)
    assert _same(torch, a, b) and _same(torch, pop._buf[1], lone[1]._buf)
    assert not _same(torch, pop._buf[1], pop._buf[0])


def test_constructor_refusals(torch):
    from merging_gym import PrioritizedRainbowReplay, RainbowPopulation, RainbowReplay

    small, other = RainbowReplay(64, device=DEV), RainbowReplay(32, device=DEV)
    with pytest.raises(ValueError, match="PrioritizedRainbowReplay"):
        RainbowPopulation(_nets(2), [small, PrioritizedRainbowReplay(64, device=DEV)], device=DEV)
    with pytest.raises(ValueError, match="share one capacity"):
        RainbowPopulation(_nets(2), [small, other], device=DEV)
    with pytest.raises(ValueError, match="lives on"):
        RainbowPopulation(_nets(2), [small, small], device="cuda:1")
    with pytest.raises(ValueError, match="2 nets need 2 replays"):
        RainbowPopulation(_nets(2), [small], device=DEV)
    with pytest.raises(ValueError, match="1..64 members"):
        RainbowPopulation([], [], device=DEV)
    with pytest.raises(ValueError, match="expected one value or 2"):
        RainbowPopulation(_nets(2), [small, small], lr=[0.1, 0.2, 0.3], device=DEV)
